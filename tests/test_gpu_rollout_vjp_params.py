"""
vs_rollout_vjp_params / k_rollout_vjp_dp: the reverse-mode sweep over recorded rollouts with the gradient with respect to domain
parameters next to it, VecSimEnv.rollout_vjp_params and DifferentiableRollout with a parameter tensor.

Shapes are those of test_gpu_trajectory_grad.py and test_gpu_rollout_vjp.py: 150 lanes (three waves, the last one partial), T = 24
steps, max_steps = 50, one recording per lane with actions strictly inside the box and outside the dead zones, lanes 0 .. 9 start at
the edge of the state space and end early, +-5 % per-lane parameters, the WRT index sets and the dts of test_gpu_trajectory_grad.py:
all three files take them from derivative_cases.py, and the first two share the draws of their case() (playback_case).

Derivatives are compared per unit RELATIVE change of a parameter (d / d log theta = theta d / d theta), which puts the columns of one
family in one unit, with the project's tolerance (3e-3 |g| + 3e-4 max |g|, at most a 2e-3 share of bad entries; against the oracle on
the entries that are smooth: central differences at relative steps 1e-6 and 1e-5 agree to 1e-4, and more than 0.9 of them must be).
Worst error / tolerance is printed with -s.

The function the oracle differentiates is the kernel's by the project's convention (vecsim_envs.h): the reward FUNCTION, the bounds of
the spaces, the initial state and the initial hidden state are constants with respect to the parameters.  The reward still depends on
them through the states it is evaluated at; its own constants do not move: phi() evaluates step_rew with the unperturbed parameters
on the perturbed trajectory (the ball-on-beam's reward scale is a function of g, one of its WRT parameters).
"""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from derivative_cases import (FAMILIES, KW, MAX_STEPS, N, N_EDGE, SPLITS, STATE_BUFFERS, T, WRT, case_cotangents, dev,  # noqa: E402
                              lengths_of, oracle_rollout, params_case, phi, record_mode2, smooth_global, within_global)


@pytest.fixture(scope="module")
def vs():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import simurlacra_amd

    return simurlacra_amd


case = params_case  # (shared with test_gpu_param_derivatives_all: the same draws)


@functools.lru_cache(maxsize=None)
def oracle_reference(name, t_steps=T):
    """central differences of Phi at relative steps 1e-6 and 1e-5 with respect to the WRT parameters of every lane, per unit relative
    change: two arrays [N, G], and the oracle's lane lengths.  The initial hidden state comes from the oracle's reset under the
    unperturbed parameters and is held; a lane's length is held at its unperturbed value (the branch taken)."""
    c = case(name)
    ref = c["ref"]
    P0 = c["params"].astype(np.float64)
    s0, a0 = c["init"].astype(np.float64), c["acts"].astype(np.float64)[:, :t_steps]
    h0 = ref.reset(P0, s0, True)["hidden"]
    length = lengths_of(oracle_rollout(ref, P0, s0, h0, a0).done)
    out = []
    for h in (1e-6, 1e-5):
        g = np.zeros((N, len(WRT[name])))
        for j, pj in enumerate(WRT[name]):
            lo, hi = P0.copy(), P0.copy()
            hi[:, pj] *= 1.0 + h
            lo[:, pj] *= 1.0 - h
            g[:, j] = (phi(c, hi, P0, s0, h0, a0, length) - phi(c, lo, P0, s0, h0, a0, length)) / (2.0 * h)
        out.append(g)
    return out[0], out[1], length


def recorded(vs, name, splits=(T,), n=N, t_steps=T):
    """a handle whose rows 0 .. t_steps - 1 hold the playback rollouts of the case, recorded in mode 2 by step_policy in the given
    launches"""
    c = case(name)
    e = vs.VecSimEnv(name, n, max_steps=MAX_STEPS, **KW[name])
    acts = c["acts"][:n, :max(t_steps, 2)]
    return record_mode2(e, t_steps, c["params"][:n], lambda e: e.set_policy_playback(acts), c["init"][:n], splits)


def cotangents(vs, name, e, t_steps=T):
    return case_cotangents(vs, case(name), e, t_steps, last="g_last")


def per_log_theta(vs, name, d_params, n=N, wrt=None):
    """d_params [G, ld] of the device -> [n, G] float64 per unit relative change of the parameter"""
    th = case(name)["params"][:n][:, WRT[name] if wrt is None else wrt].astype(np.float64)
    assert (th != 0).all()
    return vs.lanes_first(d_params, n).cpu().numpy().astype(np.float64) * th


# ------------------------------------------------------------------------ 1. against forward mode, an independent path
@pytest.mark.parametrize("name", FAMILIES)
def test_against_the_forward_mode_sensitivities(vs, name):
    """The weighted squared discrepancy against a target table: VS_ROLLOUT_GRAD of a vs_set_rollout_sens run (forward mode, tangents
    carried from step to step) against d_params of the sweep with g_obs[k][q] = 2 w_q (obs_k[q] - target_k[q]) and no g_rew.  Both
    sides are fp32 with different summation orders.  Worst error / tolerance is printed with -s."""
    L = vs._lib
    c = case(name)
    w = c["weights"]
    e = recorded(vs, name)
    obs = torch.cat([e.traj_tensors(T)["obs"], e.tensor(L.VS_OBS)[:, :N].t()[None]], dim=0).cpu().numpy()  # [T + 1, N, O]
    length = e.rollout_lengths(N, T)[0].cpu().numpy()
    assert (length[:N_EDGE] < T).any() and (length[N_EDGE:] == T).mean() > 0.9
    inside = (np.arange(T + 1)[:, None] <= length[None, :])[:, :, None]
    obs = np.where(inside, obs, 0.0).astype(np.float32).transpose(1, 0, 2)      # [N, T + 1, O]; rows behind a lane's end are not read
    target = (obs - c["resid"]).astype(np.float32)
    g_obs = ((np.float32(2.0) * w)[None, None, :] * (obs - target)).astype(np.float32)
    _, _, dp = e.rollout_vjp_params(T, WRT[name], g_obs=vs.lanes_last(dev(g_obs), e.ld))
    got = per_log_theta(vs, name, dp)
    assert e.error_count() == 0
    e.close()
    f = vs.VecSimEnv(name, N, max_steps=MAX_STEPS, **KW[name])
    f.set_auto_reset(False)
    f.set_params(c["params"])
    f.set_policy_playback(c["acts"])
    f.set_rollout_target(target, w)
    f.set_rollout_sens(WRT[name])
    f.reset(init_state=c["init"])
    f.step_policy(T)
    assert np.array_equal(f.get(L.VS_STEPCOUNT), length)
    want = f.rollout_grad().cpu().numpy().astype(np.float64) * c["params"][:, WRT[name]].astype(np.float64)
    f.close()
    assert np.isfinite(got).all() and want.any(axis=1).all()
    bad, worst = within_global(got, want)
    print(f"{name}: against forward mode: bad share {bad:.2e}, worst error / tolerance {worst:.3f}")
    assert bad < 2e-3, (name, bad, worst)


# ----------------------------------------------------------------------------------------- 2. against the fp64 oracle
def against_oracle(vs, name, n=N, t_steps=T):
    f1, f2, length = oracle_reference(name, t_steps)
    smooth = smooth_global(f1, f2)
    assert smooth.mean() > 0.9, (name, float(smooth.mean()))  # from the oracle alone
    e = recorded(vs, name, splits=(t_steps,), n=n, t_steps=t_steps)
    assert np.array_equal(e.rollout_lengths(n, t_steps)[0].cpu().numpy(), length[:n])
    _, _, dp = e.rollout_vjp_params(t_steps, WRT[name], **cotangents(vs, name, e, t_steps))
    got = per_log_theta(vs, name, dp, n)
    assert e.error_count() == 0 and not dp[:, n:].any()
    e.close()
    assert np.isfinite(got).all()
    bad, worst = within_global(got, f1[:n], smooth[:n])
    print(f"{name} n = {n} T = {t_steps}: smooth {smooth.mean():.3f}, bad share {bad:.2e}, worst error / tolerance {worst:.3f}")
    assert bad < 2e-3, (name, n, t_steps, bad, worst)
    return length


@pytest.mark.parametrize("name", FAMILIES)
def test_against_the_fp64_oracle(vs, name):
    """Random cotangents on rewards, observations and the last state.  Worst error / tolerance is printed with -s."""
    length = against_oracle(vs, name)
    assert (length[:N_EDGE] < T).any() and (length[N_EDGE:] == T).mean() > 0.9  # lanes that end early, lanes that run through


# ------------------------------------------------------------------------------------------ 4. T = 1, n = 1, n = 65
@pytest.mark.parametrize("name", ["qq-su", "qbb"])
@pytest.mark.parametrize("n,t_steps", [(N, 1), (1, T), (65, T)])
def test_one_step_one_lane_and_a_second_wave_of_one_lane(vs, name, n, t_steps):
    against_oracle(vs, name, n, t_steps)


# ------------------------------------------------------------------------------------------------- 3. exact structure
ALL_BUFFERS = STATE_BUFFERS + ("VS_EPSTAT_COUNT", "VS_EPSTAT_RETSUM", "VS_EPSTAT_LENSUM", "VS_PARAMS", "VS_CONSTS")


@pytest.mark.parametrize("name", ["qq-su", "qcp-su", "qbb"])
def test_exact_structure(vs, name):
    L = vs._lib
    c = case(name)
    wrt = WRT[name]
    e = recorded(vs, name, SPLITS)
    cot = cotangents(vs, name, e)
    # the handle also gets a target and sensitivities, filled by a non-recording run of the same rollouts: the records stay
    e.set_rollout_target(np.zeros((N, T + 1, c["ref"].O), dtype=np.float32), c["weights"])
    e.set_rollout_sens(wrt[:2])
    e.reset(init_state=c["init"])
    e.step_policy(T)

    def snapshot():
        bufs = [e.get(getattr(L, b)).copy() for b in ALL_BUFFERS]
        tt = e.traj_tensors(T)
        bufs += [tt["rec"].clone().cpu().numpy(), tt["done"].clone().cpu().numpy(), e.rollout_loss().clone().cpu().numpy(), e.rollout_grad().clone().cpu().numpy(),
                 e.rollout_gn().clone().cpu().numpy(), e.get(L.VS_ROLLOUT_SENS).copy()]
        return bufs

    before = snapshot()
    assert before[-3].any() and before[-1].any()
    da, di, dp = e.rollout_vjp_params(T, wrt, **cot)
    # ---- state, records, flags, counters and the VS_ROLLOUT_* buffers of the handle are untouched
    for k, (x, y) in enumerate(zip(before, snapshot())):
        assert np.array_equal(x, y, equal_nan=True), k
    # ---- d_act and d_init are vs_rollout_vjp's bits
    ra, ri = e.rollout_vjp(T, g_rew=cot["g_rew"], g_obs=cot["g_obs"], g_state_last=cot["g_last"])
    assert torch.equal(da, ra) and torch.equal(di, ri)
    # ---- two calls return the same bits
    assert all(torch.equal(a, b) for a, b in zip(e.rollout_vjp_params(T, wrt, **cot), (da, di, dp)))
    # ---- lanes >= n hold zeros; rows of d_act behind a lane's end are 0; every lane has a gradient in every column
    length = e.rollout_lengths(N, T)[0].cpu().numpy()
    assert e.ld > N and not da[..., N:].any() and not di[..., N:].any() and not dp[..., N:].any()
    d_act = vs.lanes_first(da, N).cpu().numpy()
    early = np.flatnonzero(length < T)
    assert early.size > 0 and (early < N_EDGE).all()
    for n in early:
        assert not d_act[n, length[n]:].any() and d_act[n, :length[n]].all()
    assert tuple(dp.shape) == (len(wrt), e.ld) and bool(dp[:, :N].any(dim=0).all()) and bool(torch.isfinite(dp).all())
    # ---- n_params = 3 is the first three columns of four (the same kernel with an unseeded column)
    d3 = e.rollout_vjp_params(T, wrt[:3], **cot)
    assert torch.equal(d3[2], dp[:3]) and torch.equal(d3[0], da) and torch.equal(d3[1], di)
    # ---- swapping two indices swaps the columns
    sw = [wrt[1], wrt[0]] + wrt[2:]
    ds = e.rollout_vjp_params(T, sw, **cot)[2]
    assert torch.equal(ds[0], dp[1]) and torch.equal(ds[1], dp[0]) and torch.equal(ds[2:], dp[2:])
    d2 = e.rollout_vjp_params(T, wrt[1::-1], **cot)[2]
    assert torch.equal(d2[0], e.rollout_vjp_params(T, wrt[:2], **cot)[2][1])
    # ---- NaN in every cotangent row behind a lane's end and in the lanes >= n changes nothing
    nan = {k: v.clone() for k, v in cot.items()}
    ln = torch.as_tensor(length, device="cuda")
    t = torch.arange(T + 1, device="cuda")
    nan["g_rew"][:, :N][t[:T, None] >= ln[None, :]] = float("nan")
    behind = (t[:, None] > ln[None, :])[:, None, :].expand(T + 1, c["ref"].O, N)
    nan["g_obs"][:, :, :N][behind] = float("nan")
    for v in nan.values():
        v[..., N:] = float("nan")
    assert bool(torch.isnan(nan["g_rew"][:, :N]).any()) and bool(torch.isnan(nan["g_obs"][:, :, :N]).any())
    assert all(torch.equal(a, b) for a, b in zip(e.rollout_vjp_params(T, wrt, **nan), (da, di, dp)))
    # ---- a cotangent on the rewards alone reaches the parameters through the states; one on observation row 0 alone does not
    gr = e.rollout_vjp_params(T, wrt, g_rew=cot["g_rew"])[2]
    assert bool(gr[:, :N][:, torch.as_tensor(length > 1, device="cuda")].any(dim=0).all())
    g0 = torch.zeros_like(cot["g_obs"])
    g0[0] = cot["g_obs"][0]
    assert not e.rollout_vjp_params(T, wrt, g_obs=g0)[2].any()
    # ---- no cotangent at all: zeros
    assert not any(x.any() for x in e.rollout_vjp_params(T, wrt))
    e.close()


# ---------------------------------------------------------------------------------------------------------- 5. refusals
def test_refusals_leave_the_outputs_untouched(vs):
    L = vs._lib
    lib = L.load()
    name = "qq-su"
    d = vs.env_dims(name)
    e = recorded(vs, name)
    d_act = torch.full((T, d["A"], e.ld), 7.0, device="cuda")
    d_init = torch.full((d["S"] + d["H"], e.ld), 7.0, device="cuda")
    d_par = torch.full((L.VS_SENS_MAX_PARAMS + 1, e.ld), 7.0, device="cuda")
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    i32 = lambda *x: np.array(x, dtype=np.int32)  # noqa: E731

    def call(handle, t_steps=T, idx=i32(1, 2), n_params=None, out=(d_act, d_init, d_par)):
        rc = lib.vs_rollout_vjp_params(handle._h if handle is not None else None, t_steps, None, None, None,
                                       None if idx is None else idx.ctypes.data_as(C.c_void_p),
                                       (0 if idx is None else len(idx)) if n_params is None else n_params, *[ptr(o) for o in out])
        torch.cuda.synchronize()
        return rc

    def refused(code, *args, **kw):
        assert call(*args, **kw) == code, (args, kw)
        assert bool((d_act == 7.0).all()) and bool((d_init == 7.0).all()) and bool((d_par == 7.0).all())  # the sentinels

    # ---- what vs_rollout_vjp refuses
    refused(L.VS_ERR_ARG, None)
    refused(L.VS_ERR_ARG, e, out=(None, d_init, d_par))
    refused(L.VS_ERR_ARG, e, out=(d_act, None, d_par))
    for t_steps in (0, -3, T + 1):
        refused(L.VS_ERR_ARG, e, t_steps)
    # ---- the index errors of vs_set_rollout_sens
    refused(L.VS_ERR_ARG, e, out=(d_act, d_init, None))
    refused(L.VS_ERR_ARG, e, idx=None, n_params=2)
    refused(L.VS_ERR_ARG, e, idx=i32(1, 2), n_params=0)
    refused(L.VS_ERR_ARG, e, idx=i32(1, 2), n_params=-1)
    for idx in (i32(1, 2, 3, 4, 5), i32(1, d["P"]), i32(-1, 2), i32(2, 2), i32(1, 2, 3, 1)):
        refused(L.VS_ERR_ARG, e, idx=idx)
    with pytest.raises(vs.ValueErr):
        e.rollout_vjp_params(T, ["motor_resistance", "no_such_parameter"])
    with pytest.raises(vs.ValueErr, match="n_params"):  # the Python face raises
        e.rollout_vjp_params(T, [])
    # ---- the handle's state
    e.set_traj_offset(3)
    refused(L.VS_ERR_STATE, e)
    with pytest.raises(RuntimeError):
        e.rollout_vjp_params(T, [1, 2])
    e.set_traj_offset(0)
    e.set_auto_reset(True)
    refused(L.VS_ERR_STATE, e)
    e.set_auto_reset(False)
    e.set_policy_playback(None)
    e.set_obs_pipeline(scale=np.full(d["O"], 2.0))
    refused(L.VS_ERR_STATE, e)
    e.set_obs_pipeline()
    e.set_act_pipeline(delay=2)
    refused(L.VS_ERR_STATE, e)
    e.set_act_pipeline()
    # ---- after the refusals the very same handle still serves: the bits of a handle that was never refused
    cot = cotangents(vs, name, e)
    fresh = recorded(vs, name)
    assert all(torch.equal(a, b) for a, b in zip(e.rollout_vjp_params(T, [1, 2], **cot), fresh.rollout_vjp_params(T, [1, 2], **cot)))
    fresh.close()
    assert call(e) == L.VS_OK and not bool((d_act == 7.0).any()) and not bool((d_init == 7.0).any())
    assert not bool((d_par[:2] == 7.0).any()) and bool((d_par[2:] == 7.0).all())  # n_params rows are written, no more
    d_act.fill_(7.0), d_init.fill_(7.0), d_par.fill_(7.0)
    e.set_record_mode(1)
    e.set_traj_capacity(T)
    refused(L.VS_ERR_STATE, e)
    e.close()
    disc = vs.VecSimEnv("bob-d", 64, dt=0.01, max_steps=MAX_STEPS)
    disc.set_record_mode(2)
    disc.set_traj_capacity(T)
    o1, o2 = torch.full((T, 1, disc.ld), 7.0, device="cuda"), torch.full((4, disc.ld), 7.0, device="cuda")
    o3 = torch.full((1, disc.ld), 7.0, device="cuda")
    assert lib.vs_rollout_vjp_params(disc._h, T, None, None, None, i32(1).ctypes.data_as(C.c_void_p), 1, ptr(o1), ptr(o2), ptr(o3)) == L.VS_ERR_STATE
    torch.cuda.synchronize()
    assert bool((o1 == 7.0).all()) and bool((o2 == 7.0).all()) and bool((o3 == 7.0).all())
    disc.close()


# ----------------------------------------------------------------------------------------------------------- 6. autograd
ENVS = {"qq-su": "QQubeSwingUpSim", "qcp-su": "QCartPoleSwingUpSim"}
SIX = {"qq-su": [1, 2, 6, 8, 3, 7], "qcp-su": [1, 8, 12, 13, 9, 10]}  # WRT and two more: two passes


@pytest.mark.parametrize("name", ["qq-su", "qcp-su"])
def test_autograd(vs, name):
    n, gamma, lanes = 70, 0.97, 32
    c = case(name)
    env = getattr(vs, ENVS[name])(max_steps=MAX_STEPS, **KW[name])
    names = [vs.param_names(name)[k] for k in SIX[name]]
    acts, init = dev(c["acts"][:n]), dev(c["init"][:n])
    theta0 = dev(c["params"][:n][:, SIX[name]])
    w_obs = dev(c["g_obs"][:n])

    def loss_of(obs, rew, lengths):
        return vs.discounted_return(rew, lengths, gamma).sum() + (w_obs * obs).sum() + 0.5 * (obs ** 2).sum()

    roll = vs.DifferentiableRollout(env, batch_lanes=lanes)
    a, s, th = acts.clone().requires_grad_(True), init.clone().requires_grad_(True), theta0.clone().requires_grad_(True)
    obs, rew, lengths = roll(a, s, domain_params=th, names=names)
    assert len(roll._vecs) == 3 and obs.requires_grad and rew.requires_grad
    g_obs, g_rew = torch.autograd.grad(loss_of(obs, rew, lengths), (obs, rew), retain_graph=True)
    loss_of(obs, rew, lengths).backward()
    assert tuple(th.grad.shape) == (n, 6) and bool(torch.isfinite(th.grad).all()) and bool(th.grad.any(dim=1).all())
    # ---- the raw entry point on the very handles, re-laid to [N, 6]: the same kernel, the same bits
    want = torch.empty(n, 6, device="cuda")
    for b, (n0, n1) in enumerate(roll._batches(n)):
        v = roll._vecs[b][0]
        cot = dict(g_rew=vs.lanes_last(g_rew[n0:n1], v.ld), g_obs=vs.lanes_last(g_obs[n0:n1], v.ld))
        want[n0:n1, :4] = vs.lanes_first(v.rollout_vjp_params(T, SIX[name][:4], **cot)[2], n1 - n0)
        want[n0:n1, 4:] = vs.lanes_first(v.rollout_vjp_params(T, SIX[name][4:], **cot)[2], n1 - n0)
    assert torch.equal(th.grad, want)
    # ---- the parameters as a plain array: the same outputs, the same action and initial-state gradients, bit for bit
    a2, s2 = acts.clone().requires_grad_(True), init.clone().requires_grad_(True)
    obs2, rew2, lengths2 = roll(a2, s2, domain_params=c["params"][:n][:, SIX[name]], names=names)
    assert torch.equal(obs2, obs) and torch.equal(rew2, rew) and torch.equal(lengths2, lengths)
    loss_of(obs2, rew2, lengths2).backward()
    assert torch.equal(a2.grad, a.grad) and torch.equal(s2.grad, s.grad)
    # ---- a tensor that does not require grad takes the old path: vs_rollout_vjp_params is not called
    calls = []
    for v, _ in roll._vecs.values():
        v.rollout_vjp_params = (lambda f: lambda *args, **kw: (calls.append(1), f(*args, **kw))[1])(v.rollout_vjp_params)
    a3, s3 = acts.clone().requires_grad_(True), init.clone().requires_grad_(True)
    obs3, rew3, lengths3 = roll(a3, s3, domain_params=theta0, names=names)
    loss_of(obs3, rew3, lengths3).backward()
    assert not calls and torch.equal(a3.grad, a.grad) and torch.equal(s3.grad, s.grad)
    # (the wrapper counts: a tensor that requires grad goes through it, two passes per batch)
    th4 = theta0.clone().requires_grad_(True)
    obs4, rew4, lengths4 = roll(acts, init, domain_params=th4, names=names)
    loss_of(obs4, rew4, lengths4).backward()
    assert len(calls) == 6 and torch.equal(th4.grad, th.grad)
    # ---- a name the family does not have
    with pytest.raises(vs.ValueErr, match="no_such"):
        roll(acts, init, domain_params=theta0[:, :1].clone().requires_grad_(True), names=["no_such"])
    roll.close()
