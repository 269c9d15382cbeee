"""
Domain-parameter derivatives with respect to EVERY parameter of every family, column by column: the reverse-mode sweep
(vs_rollout_vjp_params / k_rollout_vjp_dp) and the forward-mode sensitivities (vs_set_rollout_sens / k_rollout_play_sens) in
consecutive passes of four indices over all P, and the layers that cut a longer list of names into such passes for the user
(DifferentiableRollout, TrajectoryMatchSampler.evaluate_grad).

Every parameter has a line of its own in E::calc_consts<C> (vecsim_envs.h), with C = Dual<NP> the whole source of its tangent; the
WRT sets of the other derivative tests reach 18 of the 64.  Shapes and draws are theirs (derivative_cases.params_case: 150 lanes, T =
24, lanes 0 .. 9 end early, +-5 % per-lane parameters), the reference is derivative_cases.all_param_oracle, and the rule is the
per-column one (within_per_column: 3e-3 |g| + 3e-4 x the column's own largest smooth entry, at most a 2e-3 share of bad entries,
more than 0.9 of the entries smooth), each column per PARAM_UNIT of its parameter.  The passes end raggedly: 17 = 4 + 4 + 4 + 4 + 1,
11 = 4 + 4 + 3, 5 = 4 + 1, 3 = one pass of 3, 8 and 20 in full passes.

Every one of the 64 columns is in one of three states:
  * checked by the per-column rule against the oracle (the non-null columns);
  * asserted == 0.0 in every lane (NULL_COLUMNS "exact": the parameter reaches float-valued code only -- a dead-zone comparison, the
    bounds of the action or state box -- so its tangent never leaves calc_consts);
  * asserted below CANCEL_FLOOR = 3e-4 x the largest entry of the family's smallest non-null column (NULL_COLUMNS "cancels": the
    ball-on-beam's ball_radius, whose r^2 cancels in J_ball / r^2 and leaves fp32 rounding in the tangent; the smallest real column
    is beam_thickness, 1.86e-2 in the oracle).
NULL_COLUMNS (derivative_cases.py) says which state each null column is in and why.  Worst error / tolerance per column is printed
with -s (DESIGN.md sections 8c and 8k).  Measured on the MI355X: reverse mode against the oracle at most 0.016 (ball balancer,
ball_radius), 0.004 (cartpole, pole_mass), 0.002 and below elsewhere; forward against reverse mode at most 0.002, the Gauss-Newton
diagonal at most 0.004 (both ball_radius); no bad entry anywhere; ball_radius of the ball-on-beam 3.9e-8 against its floor 5.6e-6.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from derivative_cases import (CANCEL_FLOOR, FAMILIES, HIDDEN_FAMILIES, KW, MAX_STEPS, N, NULL_COLUMNS, N_EDGE, STARTS, STATE_BUFFERS, T,  # noqa: E402
                              all_param_oracle, case_cotangents, check_hidden_block, check_hidden_start, dev, hidden_conditions, hidden_start,
                              null_columns, open_loop_hidden_reference, params_case, record_mode2, scaled_hidden, smooth_per_column,
                              within_per_column)

ENVS = {"qq-su": "QQubeSwingUpSim", "qcp-su": "QCartPoleSwingUpSim", "qbb": "QBallBalancerSim"}


@pytest.fixture(scope="module")
def vs():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import simurlacra_amd

    return simurlacra_amd


def passes_of_four(P):
    """all parameter indices 0 .. P - 1 in consecutive passes of VS_SENS_MAX_PARAMS = 4, the last one as short as it comes"""
    return [list(range(j, min(j + 4, P))) for j in range(0, P, 4)]


def recorded(vs, name, hidden=None):
    """a handle whose rows 0 .. T - 1 hold the playback rollouts of the case, recorded in mode 2 in one launch; hidden [N, H]: the
    initial hidden state in place of reset's"""
    c = params_case(name)
    e = vs.VecSimEnv(name, N, max_steps=MAX_STEPS, **KW[name])
    return record_mode2(e, T, c["params"], lambda e: e.set_policy_playback(c["acts"]), c["init"], (T,), hidden=hidden)


def sweep_all(vs, e, P, **cot):
    """rollout_vjp_params over all P indices in passes of four -> d_params [N, P] float32 in the raw unit (torch, device); d_act and
    d_init of every pass are the first pass's bits"""
    out = torch.empty(N, P, device="cuda")
    first = None
    for idx in passes_of_four(P):
        da, di, dp = e.rollout_vjp_params(T, idx, **cot)
        assert tuple(dp.shape) == (len(idx), e.ld) and not dp[:, N:].any()
        out[:, idx] = vs.lanes_first(dp, N)
        first = first or (da, di)
        assert torch.equal(da, first[0]) and torch.equal(di, first[1]), idx
    assert bool(first[0].any()) and bool(torch.isfinite(out).all())
    return out


def check_columns(name, tag, got, f1, f2, want=None):
    """got [N, P] (per PARAM_UNIT) against the oracle's f1 (smooth where f1 and f2 agree) -- or, with `want`, against another device
    path on every entry --: the per-column rule on the non-null columns, the null columns apart.  Prints worst error / tolerance
    per column."""
    names = params_case(name)["ref"].param_names
    null = null_columns(f1, f2)
    assert np.flatnonzero(null).tolist() == sorted(NULL_COLUMNS[name])
    live = np.flatnonzero(~null)
    smooth = smooth_per_column(f1[:, live], f2[:, live])
    assert smooth.mean() > 0.9, (name, tag, float(smooth.mean()))  # from the oracle alone
    ref = f1[:, live] if want is None else want[:, live]
    bad, worst = within_per_column(got[:, live], ref, smooth if want is None else np.ones(smooth.shape, dtype=bool))
    top = int(worst.argmax())
    print(f"{name} {tag}: smooth {smooth.mean():.3f}, bad share {bad:.2e}, worst error / tolerance {worst[top]:.3f} ({names[live[top]]}); "
          + ", ".join(f"{names[j]} {w:.3f}" for j, w in zip(live, worst)))
    floor = CANCEL_FLOOR * np.abs(f1[:, live]).max(axis=0).min()  # (of the smallest non-null column, from the oracle)
    for j, (kind, why) in NULL_COLUMNS[name].items():
        cols = [got[:, j]] + ([] if want is None else [want[:, j]])
        for col in cols:
            if kind == "exact":
                assert not col.any(), (name, tag, why)
            else:
                print(f"{name} {tag}: {names[j]} cancels: largest entry {np.abs(col).max():.3e}, floor {floor:.3e}")
                assert np.abs(col).max() < floor, (name, tag, why, float(np.abs(col).max()), floor)
    assert bad < 2e-3, (name, tag, bad, dict(zip((names[j] for j in live), worst.round(3))))


# --------------------------------------------------------------------------------------------------------- reverse mode
@pytest.mark.parametrize("name", FAMILIES)
def test_reverse_mode_every_parameter_against_the_fp64_oracle(vs, name):
    """g_rew, g_obs and g_last all given; all P columns of d_params against the all-parameter oracle"""
    L = vs._lib
    c, o = params_case(name), all_param_oracle(name)
    P = o.f1.shape[1]
    assert P == vs.env_dims(name)["P"] and list(c["ref"].param_names) == vs.param_names(name)
    e = recorded(vs, name)
    assert np.array_equal(e.rollout_lengths(N, T)[0].cpu().numpy(), o.length)
    assert (o.length[:N_EDGE] < T).any() and (o.length[N_EDGE:] == T).mean() > 0.9  # lanes that end early, lanes that run through
    before = [e.get(getattr(L, b)).copy() for b in STATE_BUFFERS]
    got = sweep_all(vs, e, P, **case_cotangents(vs, c, e, T, last="g_last")).cpu().numpy().astype(np.float64) * o.unit
    for b, x in zip(STATE_BUFFERS, before):
        assert np.array_equal(x, e.get(getattr(L, b)), equal_nan=True), b
    assert e.error_count() == 0
    e.close()
    check_columns(name, "reverse mode", got, o.f1, o.f2)


@pytest.mark.parametrize("start", STARTS)
@pytest.mark.parametrize("name", HIDDEN_FAMILIES)
def test_reverse_mode_hidden_adjoint_and_the_same_bits(vs, name, start):
    """vs_rollout_vjp_params promises vs_rollout_vjp's bits for d_act and d_init: the full [S + H] rows are compared with array_equal
    from the hidden state that reset leaves and from hidden_start(), and the hidden rows are held to the oracle per column like
    vs_rollout_vjp's own (test_gpu_rollout_vjp.py).  From hidden_start() all P columns of d_params are compared with the all-parameter
    oracle recomputed from that start.  Worst error / tolerance is printed with -s (DESIGN.md sections 8d and 8k)."""
    c = params_case(name)
    g1, g2, length, _ = open_loop_hidden_reference(name, start)
    hidden_conditions(name, g1, g2)  # from the oracle alone, before the device is asked
    hidden = hidden_start(name, c) if start == "perturbed" else None
    e = recorded(vs, name, hidden=hidden)
    if hidden is None:
        assert np.array_equal(e.rollout_lengths(N, T)[0].cpu().numpy(), length)
    else:
        check_hidden_start(e, hidden, length)
    cot = case_cotangents(vs, c, e, T, last="g_last")
    P = vs.env_dims(name)["P"]
    da, di, _ = e.rollout_vjp_params(T, [0], **cot)
    ra, ri = e.rollout_vjp(T, g_rew=cot["g_rew"], g_obs=cot["g_obs"], g_state_last=cot["g_last"])
    assert tuple(di.shape) == (c["ref"].S + c["ref"].H, e.ld) and torch.equal(da, ra) and torch.equal(di, ri)
    assert e.ld > N and not di[:, N:].any()
    check_hidden_block(f"{name} vs_rollout_vjp_params from {start}", scaled_hidden(vs, c, di), g1, g2)
    if start == "perturbed":
        o = all_param_oracle(name, start)
        assert np.array_equal(o.length, length)
        got = sweep_all(vs, e, P, **cot).cpu().numpy().astype(np.float64) * o.unit  # (every pass: the first pass's d_act and d_init)
        check_columns(name, f"reverse mode from {start}", got, o.f1, o.f2)
    assert e.error_count() == 0
    e.close()


# --------------------------------------------------------------------------------------------------------- forward mode
@pytest.mark.parametrize("name", FAMILIES)
def test_forward_mode_every_parameter(vs, name):
    """The weighted squared discrepancy against target = recorded observation - resid: VS_ROLLOUT_GRAD of vs_set_rollout_sens passes
    over all P indices against d_params of the sweep with g_obs[k][q] = 2 w_q (obs_k[q] - target_k[q]) -- two independent fp32 paths
    that share calc_consts<Dual> and dynamics<Dual> and nothing else -- and every pass's Gauss-Newton diagonal against
    sum w (d obs / d theta_j)^2 from the oracle's central differences of the observations."""
    L = vs._lib
    c, o = params_case(name), all_param_oracle(name)
    P, w = o.f1.shape[1], c["weights"]
    e = recorded(vs, name)
    obs = torch.cat([e.traj_tensors(T)["obs"], e.tensor(L.VS_OBS)[:, :N].t()[None]], dim=0).cpu().numpy()  # [T + 1, N, O]
    inside = (np.arange(T + 1)[:, None] <= o.length[None, :])[:, :, None]
    obs = np.where(inside, obs, 0.0).astype(np.float32).transpose(1, 0, 2)      # [N, T + 1, O]; rows behind a lane's end are not read
    target = (obs - c["resid"]).astype(np.float32)
    g_obs = ((np.float32(2.0) * w)[None, None, :] * (obs - target)).astype(np.float32)
    rev = sweep_all(vs, e, P, g_obs=vs.lanes_last(dev(g_obs), e.ld)).cpu().numpy().astype(np.float64) * o.unit
    assert e.error_count() == 0
    e.close()
    f = vs.VecSimEnv(name, N, max_steps=MAX_STEPS, **KW[name])
    f.set_auto_reset(False)
    f.set_policy_playback(c["acts"])
    f.set_rollout_target(target, w)
    fwd, gn = np.zeros((N, P)), np.zeros((N, P))
    for idx in passes_of_four(P):
        f.set_rollout_sens(idx)
        f.set_params(c["params"])
        f.reset(init_state=c["init"])
        f.step_policy(T)
        assert np.array_equal(f.get(L.VS_STEPCOUNT), o.length)
        grad, full = f.rollout_grad().cpu().numpy(), f.rollout_gn().cpu().numpy()
        assert grad.shape == (N, len(idx)) and full.shape == (N, len(idx), len(idx)) and np.isfinite(grad).all() and np.isfinite(full).all()
        fwd[:, idx], gn[:, idx] = grad, np.diagonal(full, axis1=1, axis2=2)
    assert f.error_count() == 0
    f.close()
    fwd, gn = fwd * o.unit, gn * o.unit ** 2
    check_columns(name, "forward against reverse mode", fwd, o.disc1, o.disc2, want=rev)
    check_columns(name, "Gauss-Newton diagonal", gn, o.gn1, o.gn2)


# ------------------------------------------------------------------------------------ the layers that split for the user
@pytest.mark.parametrize("name", ["qcp-su", "qbb"])
def test_differentiable_rollout_with_every_name(vs, name):
    """names= all P names (17: four passes and one of one; 20: five full passes) in three batches of lanes: .grad is the raw entry
    point's passes of four on the very handles, bit for bit and in the order of the names; finite; 0.0 in the exact-zero columns"""
    c = params_case(name)
    names = vs.param_names(name)
    P = len(names)
    env = getattr(vs, ENVS[name])(max_steps=MAX_STEPS, **KW[name])
    roll = vs.DifferentiableRollout(env, batch_lanes=64)
    acts, init, w_obs = dev(c["acts"]), dev(c["init"]), dev(c["g_obs"])
    th = dev(c["params"]).requires_grad_(True)

    def loss_of(obs, rew, lengths):
        return vs.discounted_return(rew, lengths, 0.97).sum() + (w_obs * obs).sum() + 0.5 * (obs ** 2).sum()

    obs, rew, lengths = roll(acts, init, domain_params=th, names=names)
    assert len(roll._vecs) == 3
    g_obs, g_rew = torch.autograd.grad(loss_of(obs, rew, lengths), (obs, rew), retain_graph=True)
    loss_of(obs, rew, lengths).backward()
    assert tuple(th.grad.shape) == (N, P) and bool(torch.isfinite(th.grad).all())
    want = torch.empty(N, P, device="cuda")
    for b, (n0, n1) in enumerate(roll._batches(N)):
        v = roll._vecs[b][0]
        cot = dict(g_rew=vs.lanes_last(g_rew[n0:n1], v.ld), g_obs=vs.lanes_last(g_obs[n0:n1], v.ld))
        for idx in passes_of_four(P):
            want[n0:n1, idx] = vs.lanes_first(v.rollout_vjp_params(T, idx, **cot)[2], n1 - n0)
    assert torch.equal(th.grad, want)
    exact = [j for j, (kind, _) in NULL_COLUMNS[name].items() if kind == "exact"]
    live = [j for j in range(P) if j not in NULL_COLUMNS[name]]
    assert len(exact) == len(NULL_COLUMNS[name]) and not th.grad[:, exact].any()
    assert bool(th.grad[:, live].any(dim=0).all()) and bool(th.grad[:, live].any(dim=1).all())
    # the names in another order: the same columns in that order
    order = list(range(P - 1, -1, -1))
    th2 = dev(c["params"][:, order]).requires_grad_(True)
    obs2, rew2, lengths2 = roll(acts, init, domain_params=th2, names=[names[j] for j in order])
    assert torch.equal(obs2, obs) and torch.equal(rew2, rew)
    loss_of(obs2, rew2, lengths2).backward()
    assert torch.equal(th2.grad, th.grad[:, order])
    roll.close()


def test_sampler_gradient_with_every_name(vs):
    """TrajectoryMatchSampler.evaluate_grad(wrt = all 11 names of qq-su, gauss_newton=False): 4 + 4 + 3, the columns of its own
    passes of four, bit for bit; the two volt thresholds are exactly 0"""
    from test_gpu_trajectory_grad import qq_segments

    name = "qq-su"
    env = vs.QQubeSwingUpSim(dt=0.004, max_steps=100)
    names = vs.param_names(name)
    lens = (40, 25, 33)
    inits = np.array([[0.1, 0.5, 8.0, -15.0], [-0.2, 2.5, -6.0, 18.0], [0.0, -1.0, 10.0, 12.0]], dtype=np.float32)
    acts, obs_recs = qq_segments(vs, vs.nominal_params(name), lens, inits)
    w = np.array([1.0, 1.0, 1.0, 1.0, 0.1, 0.1], dtype=np.float32)
    smp = vs.TrajectoryMatchSampler(env, acts, obs_recs, inits, obs_weights=w, batch_lanes=6, chunk=16)  # 4 candidates: 2 batches
    cands = [dict(mass_pend_pole=0.03, length_pend_pole=0.14), dict(mass_rot_pole=0.11), dict(motor_resistance=9.0, motor_back_emf=0.05),
             dict(damping_rot_pole=1e-3, damping_pend_pole=2e-5)]
    res = smp.evaluate_grad(cands, wrt=names, gauss_newton=False)
    assert res.gn is None and tuple(res.grad.shape) == (4, 3, 11) and res.wrt == tuple(names) and bool(torch.isfinite(res.grad).all())
    assert torch.equal(res.loss, smp.evaluate(cands).loss) and bool((res.loss > 0).all())
    for idx in passes_of_four(11):
        part = smp.evaluate_grad(cands, wrt=[names[j] for j in idx], gauss_newton=False)
        assert torch.equal(part.grad, res.grad[:, :, idx]) and torch.equal(part.loss, res.loss), idx
    assert sorted(NULL_COLUMNS[name]) == [9, 10] and not res.grad[:, :, 9:].any() and bool(res.grad[:, :, :9].any(dim=1).all())
    smp.close()
