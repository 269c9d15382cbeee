"""
vs_rollout_vjp / k_rollout_vjp: the reverse-mode sweep over recorded rollouts, VecSimEnv.rollout_vjp and DifferentiableRollout.

Shapes follow test_gpu_trajectory_grad.py: 150 lanes (three waves, the last one partial), T = 24 steps, max_steps = 50, one recording
per lane with actions strictly inside the box and outside the dead zones, lanes 0 .. 9 start at the edge of the state space and end
early, +-5 % per-lane parameters, random cotangents for all three cotangent inputs.

Gradients are compared per unit change of an input in its own scale (d_act times the action scale ACT_IN, d_init times INIT_SCALE),
which puts the entries of one lane in one unit, so that the project's tolerance of test_step_jacobians_against_finite_differences
applies per lane: 3e-3 |g| + 3e-4 max |g_smooth| of the lane, at most a 2e-3 share of bad entries, entries smooth where central
differences of the fp64 oracle at relative steps 1e-6 and 1e-5 agree to 1e-4.

The hidden rows S .. S + H - 1 of d_init (cartpole, ball balancer) are not columns of that per-lane array: they are compared per column,
each per HIDDEN_SCALE, from the hidden state that reset leaves and from a non-trivial one (test_hidden_adjoint_against_the_fp64_oracle;
derivative_cases.py says why).
"""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from derivative_cases import (ACT_IN, FAMILIES, HIDDEN_FAMILIES, INIT_SCALE, KW, MAX_STEPS, N, N_EDGE, SPLITS, STARTS, STATE_BUFFERS, T,  # noqa: E402
                              case_cotangents, check_hidden_block, check_hidden_start, dev, frozen, hidden_conditions, hidden_start, lengths_of,
                              open_loop_hidden_reference, oracle_rollout, playback_case, record_mode2, scaled_hidden, smooth_per_lane,
                              start_hidden, within_per_lane)


@pytest.fixture(scope="module")
def vs():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import simurlacra_amd

    return simurlacra_amd


@functools.lru_cache(maxsize=None)
def case(name):
    """the inputs of a family, all float32 and left unchanged by the tests: params [N, P], init [N, S], acts [N, T, A] and the
    cotangents g_rew [N, T], g_obs [N, T + 1, O], g_last [N, S + H]"""
    return frozen(playback_case(name)[0])


def phi(c, state0, hidden0, acts, length):
    """[N]: sum g_rew r + sum g_obs . obs + g_last . (s_L, h_L) of every lane over its first length[n] steps (fp64 oracle)"""
    states, hiddens, obs, rew, _ = oracle_rollout(c["ref"], c["params"].astype(np.float64), state0, hidden0, acts)
    k = np.arange(T + 1)[:, None]
    n = np.arange(state0.shape[0])
    out = (np.where(k[:T] < length[None, :], c["g_rew"].T.astype(np.float64) * rew, 0.0)).sum(axis=0)
    out += np.where((k <= length[None, :])[:, :, None], c["g_obs"].transpose(1, 0, 2).astype(np.float64) * obs, 0.0).sum(axis=(0, 2))
    last = np.concatenate([states[length, n], hiddens[length, n]], axis=1)
    return out + (c["g_last"].astype(np.float64) * last).sum(axis=1)


@functools.lru_cache(maxsize=None)
def oracle_reference(name, start="reset"):
    """central differences of Phi at relative steps 1e-6 and 1e-5 with respect to every action entry and every initial-state entry,
    per unit of the input's scale: two arrays [N, T * A + S] (actions first, step-major), and the oracle's lane lengths.  The hidden
    state starts from the oracle's reset (start = "perturbed": from hidden_start()); a lane's length is held at its unperturbed value
    (the branch taken)."""
    c = case(name)
    ref = c["ref"]
    s0, a0 = c["init"].astype(np.float64), c["acts"].astype(np.float64)
    h0 = start_hidden(name, c, start)
    length = lengths_of(oracle_rollout(ref, c["params"].astype(np.float64), s0, h0, a0).done)
    out = []
    for h in (1e-6, 1e-5):
        g = np.zeros((N, T * ref.A + ref.S))
        for t in range(T):
            for j in range(ref.A):
                d = np.zeros_like(a0)
                d[:, t, j] = h * ACT_IN[name]
                g[:, t * ref.A + j] = (phi(c, s0, h0, a0 + d, length) - phi(c, s0, h0, a0 - d, length)) / (2.0 * h)
        for j in range(ref.S):
            d = np.zeros_like(s0)
            d[:, j] = h * INIT_SCALE[name][j]
            g[:, T * ref.A + j] = (phi(c, s0 + d, h0, a0, length) - phi(c, s0 - d, h0, a0, length)) / (2.0 * h)
        out.append(g)
    return out[0], out[1], length


def recorded(vs, name, splits=(T,), acts=None, n=N, hidden=None):
    """a handle whose rows 0 .. T - 1 hold the playback rollouts of the case, recorded in mode 2 by step_policy in the given launches;
    hidden [N, H]: the initial hidden state in place of reset's"""
    c = case(name)
    e = vs.VecSimEnv(name, n, max_steps=MAX_STEPS, **KW[name])
    return record_mode2(e, T, c["params"][:n], lambda e: e.set_policy_playback(c["acts"][:n] if acts is None else acts), c["init"][:n], splits,
                        hidden=None if hidden is None else hidden[:n])


def cotangents(vs, name, e, t_steps=T):
    return case_cotangents(vs, case(name), e, t_steps)


def host(vs, d_act, d_init, n=N):
    return vs.lanes_first(d_act, n).cpu().numpy(), vs.lanes_first(d_init, n).cpu().numpy()


# ----------------------------------------------------------------------------------------- 1. against the fp64 oracle
@pytest.mark.parametrize("name", FAMILIES)
def test_against_the_fp64_oracle(vs, name):
    """Worst error / tolerance measured on the MI355X (printed with -s): 0.002 (ball-on-beam, pendulum), 0.001
    (oscillator, QQube, cartpole), below 0.0005 (ball balancer); every entry smooth, no bad entry."""
    L = vs._lib
    c = case(name)
    ref = c["ref"]
    f1, f2, length = oracle_reference(name)
    smooth = smooth_per_lane(f1, f2)
    assert (~smooth).mean() <= 0.01, (name, float((~smooth).mean()))  # from the oracle alone
    e = recorded(vs, name)
    assert np.array_equal(e.rollout_lengths(N, T)[0].cpu().numpy(), length)
    assert (length[:N_EDGE] < T).any() and (length[N_EDGE:] == T).mean() > 0.9  # lanes that end early, lanes that run through
    d_act, d_init = host(vs, *e.rollout_vjp(T, **cotangents(vs, name, e)))
    assert e.error_count() == 0
    e.close()
    # (the hidden rows of d_init have a unit and a test of their own: test_hidden_adjoint_against_the_fp64_oracle)
    got = np.concatenate([d_act.reshape(N, T * ref.A) * ACT_IN[name], d_init[:, :ref.S] * np.array(INIT_SCALE[name])], axis=1)
    assert np.isfinite(got).all()
    bad, worst = within_per_lane(got.astype(np.float64), f1, smooth)
    print(f"{name}: not smooth {(~smooth).mean():.4f}, bad share {bad:.2e}, worst error / tolerance {worst:.3f}")
    assert bad <= 2e-3, (name, bad, worst)


@pytest.mark.parametrize("start", STARTS)
@pytest.mark.parametrize("name", HIDDEN_FAMILIES)
def test_hidden_adjoint_against_the_fp64_oracle(vs, name, start):
    """Rows S .. S + H - 1 of d_init, d Phi / d h_0, against central differences of the same Phi at HIDDEN_STEPS x HIDDEN_SCALE, per column
    and per HIDDEN_SCALE, from the hidden state that reset leaves and from hidden_start(); edge lanes like any other, lanes >= n exactly
    0.  From hidden_start() the action and state columns go through test_against_the_fp64_oracle's per-lane check as well.  vs_step_jac
    has no h in its x, so nothing else sees this column (test_against_chained_one_step_jacobians leaves both families out).
    Worst error / tolerance per column measured on the MI355X (printed with -s): DESIGN.md section 8d."""
    c = case(name)
    ref = c["ref"]
    g1, g2, length, _ = open_loop_hidden_reference(name, start)
    hidden_conditions(name, g1, g2)  # from the oracle alone, before the device is asked
    hidden = hidden_start(name, c) if start == "perturbed" else None
    e = recorded(vs, name, hidden=hidden)
    if hidden is None:
        assert np.array_equal(e.rollout_lengths(N, T)[0].cpu().numpy(), length)
    else:
        check_hidden_start(e, hidden, length)
    da, di = e.rollout_vjp(T, **cotangents(vs, name, e))
    assert e.error_count() == 0 and e.ld > N and not da[..., N:].any() and not di[..., N:].any()
    e.close()
    check_hidden_block(f"{name} vs_rollout_vjp from {start}", scaled_hidden(vs, c, di), g1, g2)
    if start == "perturbed":
        f1, f2, length2 = oracle_reference(name, start)
        smooth = smooth_per_lane(f1, f2)
        assert np.array_equal(length2, length) and (~smooth).mean() <= 0.01, (name, float((~smooth).mean()))  # from the oracle alone
        d_act, d_init = host(vs, da, di)
        got = np.concatenate([d_act.reshape(N, T * ref.A) * ACT_IN[name], d_init[:, :ref.S] * np.array(INIT_SCALE[name])], axis=1)
        assert np.isfinite(got).all()
        bad, worst = within_per_lane(got.astype(np.float64), f1, smooth)
        print(f"{name} from {start}: actions and states: not smooth {(~smooth).mean():.4f}, bad share {bad:.2e}, worst error / tolerance {worst:.3f}")
        assert bad <= 2e-3, (name, bad, worst)


# ------------------------------------------------------------------------------------ 2. against the one-step Jacobians
@pytest.mark.parametrize("name", [f for f in FAMILIES if f not in ("qcp-su", "qbb")])
def test_against_chained_one_step_jacobians(vs, name):
    """Families without hidden state (vs_step_jac's x = (s, a) has no h, so its Jacobians cannot be chained for the other two; their hidden
    column is held to the oracle in test_hidden_adjoint_against_the_fp64_oracle), the first K = 12 steps: a second handle steps along
    the same actions with vs_step_jac and its fp32 Jacobians are chained transposed in fp64 on the host.  (g_obs row 0 is 0 here: vs_step_jac has no Jacobian of the initial
    observation.)  Both sides differentiate the same dual-number step code, so the difference is the kernel's fp32 summation alone.
    Bound: one output of one step is an fma chain of M = S + 1 + O terms from 0, its rounding error at most M u times the sum of the
    absolute terms, u = 2^-24 (Higham, gamma_M, first order).  With abs_t = |J_t|^T abs_{t+1} + |g_rew[t]| |J_r| + |J_o|^T |g_obs[t+1]|
    (abs_L = |g_state_last|) the error e_t of lambda_t obeys e_t <= |J_t|^T e_{t+1} + M u abs_t, hence e_t <= (L - t) M u abs_t; the
    same for d_act[t].  The test allows 1.01 times that for the terms of second order.  Worst measured ratio to the bound on the MI355X
    (DESIGN.md section 8d): oscillator 0.28, ball-on-beam 0.18, QQube 0.31, pendulum 0.35."""
    K = 12
    c = case(name)
    ref = c["ref"]
    S, A, O = ref.S, ref.A, ref.O
    e = recorded(vs, name)
    cot = cotangents(vs, name, e, K)
    cot["g_obs"][0] = 0.0
    d_act, d_init = host(vs, *e.rollout_vjp(K, **cot))
    length = e.rollout_lengths(N, K)[0].cpu().numpy()
    e.close()
    j = vs.VecSimEnv(name, N, max_steps=MAX_STEPS, **KW[name])
    j.set_auto_reset(False)
    j.set_params(c["params"])
    j.reset(init_state=c["init"])
    jac = [j.step_jac(dev(c["acts"][:, t])) for t in range(K)]
    j.close()
    g_rew, g_obs, g_last = (c[k].astype(np.float64) for k in ("g_rew", "g_obs", "g_last"))
    lam, ab = g_last.copy(), np.abs(g_last)
    want_act, abs_act = np.zeros((N, K, A)), np.zeros((N, K, A))
    for t in range(K - 1, -1, -1):
        js, jr, jo = (jac[t][k].astype(np.float64) for k in ("state", "rew", "obs"))
        new = np.einsum("nj,njk->nk", lam, js) + g_rew[:, t, None] * jr + np.einsum("nq,nqk->nk", g_obs[:, t + 1], jo)
        nab = np.einsum("nj,njk->nk", ab, np.abs(js)) + np.abs(g_rew[:, t, None] * jr) + np.einsum("nq,nqk->nk", np.abs(g_obs[:, t + 1]), np.abs(jo))
        on = (t < length)[:, None]  # a lane that ended before step t keeps lambda = g_state_last
        want_act[:, t], abs_act[:, t] = np.where(on, new[:, S:], 0.0), np.where(on, nab[:, S:], 0.0)
        lam, ab = np.where(on, new[:, :S], lam), np.where(on, nab[:, :S], ab)
    u, M = 2.0 ** -24, S + 1 + O
    steps_left = np.maximum(length[:, None] - np.arange(K)[None, :], 0)[:, :, None]
    r_act = np.abs(d_act - want_act) / np.maximum(1.01 * steps_left * M * u * abs_act, 1e-300)
    r_init = np.abs(d_init - lam) / np.maximum(1.01 * length[:, None] * M * u * ab, 1e-300)
    assert not d_act[steps_left[:, :, 0] == 0].any()
    worst = max(float(r_act[steps_left[:, :, 0] > 0].max()), float(r_init.max()))
    print(f"{name}: worst error / bound {worst:.3f}")
    assert worst <= 1.0, (name, worst)


# ------------------------------------------------------------------------------------------------- 3. exact structure
@pytest.mark.parametrize("name", ["qq-su", "qcp-su"])
def test_exact_structure(vs, name):
    L = vs._lib
    c = case(name)
    e = recorded(vs, name, SPLITS)
    cot = cotangents(vs, name, e)
    before = [e.get(getattr(L, b)).copy() for b in STATE_BUFFERS]
    da, di = e.rollout_vjp(T, **cot)
    # ---- the handle's state, step counter and flags are untouched
    for b, x in zip(STATE_BUFFERS, before):
        assert np.array_equal(e.get(getattr(L, b)), x), b
    # ---- lanes >= n hold zeros, rows behind a lane's end are 0, the rows before it are not
    assert e.ld > N and not da[..., N:].any() and not di[..., N:].any()
    d_act, d_init = host(vs, da, di)
    length = e.rollout_lengths(N, T)[0].cpu().numpy()
    early = np.flatnonzero(length < T)
    assert early.size > 0 and (early < N_EDGE).all()
    for n in early:
        assert not d_act[n, length[n]:].any() and d_act[n, :length[n]].all()
    assert d_act[length == T].all() and d_init.any(axis=1).all()
    # ---- all-zero cotangents (and none at all) give all-zero outputs
    zero = {k: torch.zeros_like(v) for k, v in cot.items()}
    for kw in (zero, {}):
        za, zi = e.rollout_vjp(T, **kw)
        assert not za.any() and not zi.any()
    # ---- records made in launches of 7 + 1 + 16 and records made by 24 step_record calls give the same bits
    one = recorded(vs, name)
    assert all(torch.equal(a, b) for a, b in zip(one.rollout_vjp(T, **cot), (da, di)))
    one.close()
    by_step = vs.VecSimEnv(name, N, max_steps=MAX_STEPS, **KW[name])
    by_step.set_auto_reset(False)
    by_step.set_record_mode(2)
    by_step.set_traj_capacity(T)
    by_step.set_params(c["params"])
    by_step.reset(init_state=c["init"])
    for t in range(T):
        by_step.step_record(dev(c["acts"][:, t]), row=t)
    assert all(torch.equal(a, b) for a, b in zip(by_step.rollout_vjp(T, **cot), (da, di)))
    by_step.close()
    # ---- a cotangent on observation row k alone leaves d_act[t >= k] at 0
    for k in (0, 5, T):
        g = torch.zeros_like(cot["g_obs"])
        g[k] = cot["g_obs"][k]
        ka, ki = e.rollout_vjp(T, g_obs=g)
        assert not ka[k:].any()
        reach = torch.as_tensor(length >= k, device=ki.device)
        assert ki[:, :N][:, reach].any(dim=0).all() and (k == 0 or ka[:k, :, :N][..., reach].any())
    # ---- changing one lane's cotangents leaves every other lane's bits unchanged
    other = {k: v.clone() for k, v in cot.items()}
    for v in other.values():
        v[..., 70] += 1.0
    oa, oi = e.rollout_vjp(T, **other)
    keep = torch.arange(e.ld, device=oa.device) != 70
    assert torch.equal(oa[..., keep], da[..., keep]) and torch.equal(oi[..., keep], di[..., keep])
    assert not torch.equal(oa[..., 70], da[..., 70]) and not torch.equal(oi[..., 70], di[..., 70])
    e.close()
    # ---- an action beyond the clip bound: nothing reaches the dynamics through it, d_act of that step is exactly 0 for cotangents
    # on observations and states while earlier rows stay non-zero.  (The reward's action cost is a function of the UNCLIPPED action,
    # P/environments/pysim/base.py: its own term -2 R a g_rew[t] stays; it is part of the oracle comparison above.)
    acts = c["acts"].copy()
    acts[N_EDGE:, 9] = 40.0 * np.sign(acts[N_EDGE:, 9])
    clip = recorded(vs, name, acts=acts)
    ca, _ = clip.rollout_vjp(T, g_obs=cot["g_obs"], g_state_last=cot["g_state_last"])
    ca = vs.lanes_first(ca, N).cpu().numpy()
    ran = clip.rollout_lengths(N, T)[0].cpu().numpy() > 9
    ran[:N_EDGE] = False
    assert ran.sum() > 100 and not ca[ran, 9].any() and ca[ran, :9].all()
    ra, _ = clip.rollout_vjp(T, **cot)
    assert vs.lanes_first(ra, N).cpu().numpy()[ran, 9].all()  # the reward's own term
    clip.close()


# ---------------------------------------------------------------------------------------------------------- 4. refusals
def test_refusals_leave_the_outputs_untouched(vs):
    L = vs._lib
    lib = L.load()
    name = "qq-su"
    d = vs.env_dims(name)
    e = recorded(vs, name)
    d_act = torch.full((T, d["A"], e.ld), 7.0, device="cuda")
    d_init = torch.full((d["S"] + d["H"], e.ld), 7.0, device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def call(handle, t_steps=T, out=(d_act, d_init)):
        rc = lib.vs_rollout_vjp(handle._h if handle is not None else None, t_steps, None, None, None,
                                ptr(out[0]) if out[0] is not None else None, ptr(out[1]) if out[1] is not None else None)
        torch.cuda.synchronize()
        return rc

    def refused(code, *args, **kw):
        assert call(*args, **kw) == code
        assert bool((d_act == 7.0).all()) and bool((d_init == 7.0).all())  # the sentinels

    refused(L.VS_ERR_ARG, None)
    refused(L.VS_ERR_ARG, e, out=(None, d_init))
    refused(L.VS_ERR_ARG, e, out=(d_act, None))
    for t_steps in (0, -3, T + 1):
        refused(L.VS_ERR_ARG, e, t_steps)
    e.set_traj_offset(3)
    refused(L.VS_ERR_STATE, e)
    with pytest.raises(RuntimeError):  # the Python face raises
        e.rollout_vjp(T)
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
    # after the refusals the very same handle still serves
    assert call(e) == L.VS_OK and not bool((d_act == 7.0).any()) and not bool((d_init == 7.0).any())
    d_act.fill_(7.0), d_init.fill_(7.0)
    e.set_record_mode(1)
    e.set_traj_capacity(T)
    refused(L.VS_ERR_STATE, e)
    e.close()
    disc = vs.VecSimEnv("bob-d", 64, dt=0.01, max_steps=MAX_STEPS)
    disc.set_record_mode(2)
    disc.set_traj_capacity(T)
    o1, o2 = torch.full((T, 1, disc.ld), 7.0, device="cuda"), torch.full((4, disc.ld), 7.0, device="cuda")
    assert lib.vs_rollout_vjp(disc._h, T, None, None, None, ptr(o1), ptr(o2)) == L.VS_ERR_STATE
    torch.cuda.synchronize()
    assert bool((o1 == 7.0).all()) and bool((o2 == 7.0).all())
    disc.close()


# ----------------------------------------------------------------------------------------------------------- 5. autograd
ENVS = {"qq-su": "QQubeSwingUpSim", "qcp-su": "QCartPoleSwingUpSim"}


def torch_case(name, n):
    rng = np.random.default_rng(31)
    scale = np.array(INIT_SCALE[name])
    A = case(name)["ref"].A
    init = (rng.uniform(-1.0, 1.0, (n, scale.size)) * scale).astype(np.float32)
    acts = (ACT_IN[name] * rng.uniform(0.3, 0.6, (n, T, A)) * rng.choice([-1.0, 1.0], (n, T, A))).astype(np.float32)
    return dev(acts), dev(init), scale


@pytest.mark.parametrize("name", ["qq-su", "qcp-su"])
def test_autograd(vs, name):
    n, gamma = 128, 0.97
    env = getattr(vs, ENVS[name])(max_steps=MAX_STEPS, **KW[name])
    roll = vs.DifferentiableRollout(env)
    acts, init, scale = torch_case(name, n)
    S = init.shape[1]
    # ---- the gradient of the discounted return is rollout_vjp with g_rew[t] = gamma^t, bit for bit
    a, s = acts.clone().requires_grad_(True), init.clone().requires_grad_(True)
    obs, rew, lengths = roll(a, s)
    assert tuple(obs.shape) == (n, T + 1, obs.shape[2]) and tuple(rew.shape) == (n, T) and float((lengths == T).float().mean()) > 0.9
    assert obs.requires_grad and rew.requires_grad and not lengths.requires_grad
    ga, gs = torch.autograd.grad(vs.discounted_return(rew, lengths, gamma).sum(), (a, s))
    v = roll._vecs[0][0]
    disc = torch.pow(torch.tensor(gamma, dtype=torch.float32, device="cuda"), torch.arange(T, dtype=torch.float32, device="cuda"))
    da, di = v.rollout_vjp(T, g_rew=vs.lanes_last(disc[None, :].expand(n, T), v.ld))
    assert torch.equal(ga, vs.lanes_first(da, n)) and torch.equal(gs, vs.lanes_first(di[:S], n))
    assert bool(ga[lengths == T].any(dim=2).all()) and bool(gs.any(dim=1).all())
    # ---- a trajectory-matching loss on the observations reaches the initial states; every lane has a descent step along -grad
    with torch.no_grad():
        target = roll(acts, init)[0]
    delta = torch.as_tensor((0.05 * scale * np.random.default_rng(2).choice([-1.0, 1.0], (n, S))).astype(np.float32), device="cuda")

    def lane_loss(s0):
        return ((roll(acts, s0)[0] - target) ** 2).sum(dim=(1, 2))

    s1 = (init + delta).requires_grad_(True)
    loss0 = lane_loss(s1)
    (g,) = torch.autograd.grad(loss0.sum(), s1)
    assert bool(torch.isfinite(g).all()) and bool(g.any(dim=1).all())
    better = torch.zeros(n, dtype=torch.bool, device="cuda")
    with torch.no_grad():
        for k in range(1, 6):
            step = 10.0 ** -k * s1.norm(dim=1, keepdim=True) / g.norm(dim=1, keepdim=True)
            better |= lane_loss(s1 - step * g) < loss0
    assert bool(better.all()), int((~better).sum())
    roll.close()
    # ---- 200 lanes in batches of 128 give the bits of one batch
    acts2, init2, _ = torch_case(name, 200)
    res = []
    for batch_lanes in (128, 65536):
        r = vs.DifferentiableRollout(env, batch_lanes=batch_lanes)
        a, s = acts2.clone().requires_grad_(True), init2.clone().requires_grad_(True)
        obs, rew, lengths = r(a, s)
        ((obs ** 2).sum() + vs.discounted_return(rew, lengths, gamma).sum()).backward()
        res.append((obs.detach(), rew.detach(), lengths, a.grad, s.grad))
        assert len(r._vecs) == (2 if batch_lanes == 128 else 1)
        r.close()
    assert all(torch.equal(x, y) for x, y in zip(*res))
