"""
vs_rollout_vjp_policy / k_rollout_vjp_lin: the reverse-mode sweep over CLOSED-LOOP recorded rollouts (a linear policy on a feature stack
in the loop), VecSimEnv.rollout_vjp_policy and DifferentiablePolicyRollout.

Shapes are those of test_gpu_rollout_vjp.py: 150 lanes (three waves, the last one partial), T = 24 steps, max_steps = 50, +-5 % per-lane
parameters, lanes 0 .. 9 start at the edge of the state space and end early, random cotangents on all four cotangent inputs.

The reference is a closed-loop fp64 rollout (closed_loop_cases.py): oracle.cpu_ref for the step, the NumPy feature stack for the policy,
a_t = W phi(obs_t) + n_t with an additive per-step offset n_t (0 unless a test says otherwise).  Central differences of Phi at relative
steps 1e-6 and 1e-5 with respect to every n_t entry (-> d_act, the total adjoint of a_t) and every initial-state entry (-> d_init), the
lane's length held at its unperturbed value, per unit of the input's scale (ACT_IN, INIT_SCALE).  Tolerance, per lane, the project's:
3e-3 |g| + 3e-4 max |g_smooth|, at most a 2e-3 share of bad entries, entries smooth where the two step sizes agree to 1e-4, at most 1 %
not smooth (asserted from the oracle alone).

The weights keep every lane inside the action box and outside the dead zones for all 24 steps: the const feature is a bias of
+-0.45 ACT_IN, every other feature f has the weight +-0.12 ACT_IN / (F max |phi_f|), the maximum taken over a rollout under the bias
alone, so that their sum stays within +-0.15 ACT_IN (asserted on the oracle's closed loop).
"""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import closed_loop_cases as clc  # noqa: E402
from closed_loop_cases import (ENVS, GAMMA, LINEAR_ORACLE_CASES as ORACLE_CASES, NT, TT, case, check_policy_keeps_the_box, cotangents,  # noqa: E402
                               features, feedback_seen, hidden_reference, linear_policy, oracle_reference, recorded, reference)
from derivative_cases import (ACT_IN, HIDDEN_FAMILIES, INIT_SCALE, KW, MAX_STEPS, N, N_EDGE, SPLITS, STARTS, STATE_BUFFERS, T,  # noqa: E402
                              check_hidden_block, check_hidden_start, dev, hidden_conditions, hidden_start, scaled, scaled_hidden,
                              smooth_per_lane, within_per_lane)


@pytest.fixture(scope="module")
def vs():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import simurlacra_amd

    return simurlacra_amd


# ----------------------------------------------------------------------------------- 1. + 2. against the fp64 oracle
@pytest.mark.parametrize("key", ORACLE_CASES)
def test_against_the_closed_loop_fp64_oracle(vs, key):
    """Worst error / tolerance measured on the MI355X (printed with -s): 0.012 (QQube, full stack), 0.001
    (oscillator with either stack, cartpole, pendulum through obs_idx), below 0.0005 (ball-on-beam, ball balancer); every entry smooth,
    no bad entry; the feedback is seen on 0.55 (cartpole) to 0.96 (ball balancer) of the full-length lanes."""
    c = case(key)
    r = oracle_reference(key)
    f1, length = r.f1, r.length
    smooth = smooth_per_lane(f1, r.f2)
    assert (~smooth).mean() <= 0.01, (key, float((~smooth).mean()))  # from the oracle alone
    check_policy_keeps_the_box(c, r.acts, length)
    assert (length[:N_EDGE] < T).any() and (length[N_EDGE:] == T).mean() > 0.9  # lanes that end early, lanes that run through
    # ---- the test can see the feedback (oracle alone): closed- and open-loop d_init differ by more than 10 x the tolerance on at
    # least half of the full-length lanes
    seen = feedback_seen(c, f1, smooth, r.open_init, length)
    assert seen >= 0.5, (key, seen)
    e = recorded(vs, key)
    assert np.array_equal(e.rollout_lengths(N, T)[0].cpu().numpy(), length)
    got = scaled(vs, c, *e.rollout_vjp_policy(T, **cotangents(vs, key, e)))
    assert e.error_count() == 0
    e.close()
    bad, worst = within_per_lane(got, f1, smooth)
    print(f"{key}: not smooth {(~smooth).mean():.4f}, feedback seen on {seen:.2f} of the full lanes, bad share {bad:.2e}, "
          f"worst error / tolerance {worst:.3f}")
    assert bad <= 2e-3, (key, bad, worst)


@pytest.mark.parametrize("start", STARTS)
@pytest.mark.parametrize("key", HIDDEN_FAMILIES)
def test_hidden_adjoint_against_the_closed_loop_fp64_oracle(vs, key, start):
    """Rows S .. S + H - 1 of d_init (scaled() cuts them off: they have another unit and another rule) against central differences of the
    closed loop's Phi at HIDDEN_STEPS x HIDDEN_SCALE, per column and per HIDDEN_SCALE, from the hidden state that reset leaves and from
    hidden_start(); edge lanes like any other, lanes >= n exactly 0.  From hidden_start() the offset and state columns go through test
    1's per-lane check as well, and the policy still keeps the box.  Worst error / tolerance per column as measured on the MI355X
    (printed with -s): DESIGN.md section 8d."""
    c = case(key)
    g1, g2, length = hidden_reference(key, start)
    hidden_conditions(key, g1, g2)  # from the oracle alone, before the device is asked
    hidden = hidden_start(c["name"], c) if start == "perturbed" else None
    e = recorded(vs, key, hidden=hidden)
    if hidden is None:
        assert np.array_equal(e.rollout_lengths(N, T)[0].cpu().numpy(), length)
    else:
        check_hidden_start(e, hidden, length)
    da, di = e.rollout_vjp_policy(T, **cotangents(vs, key, e))
    assert e.error_count() == 0 and e.ld > N and not da[..., N:].any() and not di[..., N:].any()
    e.close()
    check_hidden_block(f"{key} vs_rollout_vjp_policy from {start}", scaled_hidden(vs, c, di), g1, g2)
    if start == "perturbed":
        r = oracle_reference(key, start)
        f1, smooth = r.f1, smooth_per_lane(r.f1, r.f2)
        assert np.array_equal(r.length, length) and (~smooth).mean() <= 0.01, (key, float((~smooth).mean()))  # from the oracle alone
        check_policy_keeps_the_box(c, r.acts, length)
        bad, worst = within_per_lane(scaled(vs, c, da, di), f1, smooth)
        print(f"{key} from {start}: offsets and states: not smooth {(~smooth).mean():.4f}, bad share {bad:.2e}, worst error / tolerance {worst:.3f}")
        assert bad <= 2e-3, (key, bad, worst)


# ------------------------------------------------------------------------------------ 3. reduction to the open-loop sweep
@pytest.mark.parametrize("key", ["omo-const", "bob-const", "qq-su-const", "qcp-su-const", "pend-const", "qbb-const"])
def test_a_constant_policy_reduces_to_the_open_loop_sweep(vs, key):
    e = recorded(vs, key)
    cot = cotangents(vs, key, e, with_act=False)
    oa, oi = e.rollout_vjp(T, **cot)
    pa, pi = e.rollout_vjp_policy(T, **cot)
    assert torch.equal(pa, oa) and torch.equal(pi, oi) and bool(oa.any()) and bool(oi.any())
    g_act = cotangents(vs, key, e)["g_act"]
    ga, gi = e.rollout_vjp_policy(T, g_act=g_act, **cot)
    length = e.rollout_lengths(N, T)[0]
    inside = torch.zeros(T, 1, e.ld, device="cuda")
    inside[:, 0, :N] = (torch.arange(T, device="cuda")[:, None] < length[None, :]).float()
    assert torch.equal(ga, oa + g_act * inside) and torch.equal(gi, oi)
    assert e.error_count() == 0
    e.close()


# ------------------------------------------------------------------------------------------------- 4. exact structure
@pytest.mark.parametrize("key", ["qq-su", "qcp-su"])
def test_exact_structure(vs, key):
    L = vs._lib
    e = recorded(vs, key, SPLITS)
    cot = cotangents(vs, key, e)
    before = [e.get(getattr(L, b)).copy() for b in STATE_BUFFERS]
    da, di = e.rollout_vjp_policy(T, **cot)
    for b, x in zip(STATE_BUFFERS, before):  # the handle's state, step counter and flags are untouched
        assert np.array_equal(e.get(getattr(L, b)), x), b
    assert e.ld > N and not da[..., N:].any() and not di[..., N:].any()
    d_act = vs.lanes_first(da, N).cpu().numpy()
    length = e.rollout_lengths(N, T)[0].cpu().numpy()
    early = np.flatnonzero(length < T)
    assert early.size > 0 and (early < N_EDGE).all()
    for n in early:
        assert not d_act[n, length[n]:].any() and d_act[n, :length[n]].all()
    assert d_act[length == T].all() and bool(di[:, :N].any(dim=0).all())
    for kw in ({k: torch.zeros_like(v) for k, v in cot.items()}, {}):  # zero cotangents, and none at all
        za, zi = e.rollout_vjp_policy(T, **kw)
        assert not za.any() and not zi.any()
    one = recorded(vs, key)  # records made in one launch: the same bits
    assert all(torch.equal(a, b) for a, b in zip(one.rollout_vjp_policy(T, **cot), (da, di)))
    assert e.error_count() == 0 and one.error_count() == 0
    one.close()
    e.close()


# ----------------------------------------------------------------------------------------------------------- 5. noise
def test_exploration_noise_is_an_additive_constant(vs):
    """The recorded raw action contains the noise: n_t = a_recorded - W phi(obs_recorded), taken from the records in fp64, is fed to
    the oracle as a constant offset; the comparison is test 1's."""
    key = "pend-view"
    c = case(key)
    ref = c["ref"]
    e = recorded(vs, key, noise_std=np.full(ref.A, 0.02 * ACT_IN[c["name"]]), noise_seed=77)
    tt = e.traj_tensors(T, N)
    obs, act = tt["obs"].cpu().numpy().astype(np.float64), tt["act"].cpu().numpy().astype(np.float64)  # [T, N, .]
    x = obs.reshape(T * N, ref.O)[:, list(c["obs_idx"])]
    offs = (act - (features(c["terms"], x) @ c["W"].astype(np.float64).T).reshape(T, N, ref.A)).transpose(1, 0, 2)
    assert 0.5 < offs[N_EDGE:].std() / (0.02 * ACT_IN[c["name"]]) < 1.5  # the noise is there
    r = reference(c, np.ascontiguousarray(offs))
    f1, length, smooth = r.f1, r.length, smooth_per_lane(r.f1, r.f2)
    assert (~smooth).mean() <= 0.01
    assert np.array_equal(e.rollout_lengths(N, T)[0].cpu().numpy(), length)
    got = scaled(vs, c, *e.rollout_vjp_policy(T, **cotangents(vs, key, e)))
    assert e.error_count() == 0
    e.close()
    bad, worst = within_per_lane(got, f1, smooth)
    print(f"{key} + noise: not smooth {(~smooth).mean():.4f}, bad share {bad:.2e}, worst error / tolerance {worst:.3f}")
    assert bad <= 2e-3, (bad, worst)


# ---------------------------------------------------------------------------------------------------------- 6. refusals
def test_refusals_leave_the_outputs_untouched(vs):
    L = vs._lib
    lib = L.load()
    key = "qq-su"
    c = case(key)
    d = vs.env_dims(c["name"])
    e = recorded(vs, key)
    d_act = torch.full((T, d["A"], e.ld), 7.0, device="cuda")
    d_init = torch.full((d["S"] + d["H"], e.ld), 7.0, device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def call(handle, t_steps=T, out=(d_act, d_init)):
        rc = lib.vs_rollout_vjp_policy(handle._h if handle is not None else None, t_steps, None, None, None, None,
                                       ptr(out[0]) if out[0] is not None else None, ptr(out[1]) if out[1] is not None else None)
        torch.cuda.synchronize()
        return rc

    def refused(code, *args, **kw):
        assert call(*args, **kw) == code
        assert bool((d_act == 7.0).all()) and bool((d_init == 7.0).all())  # the sentinels

    def linear():
        e.set_policy_linear(c["W"].reshape(-1), list(c["terms"]))

    refused(L.VS_ERR_ARG, None)
    refused(L.VS_ERR_ARG, e, out=(None, d_init))
    refused(L.VS_ERR_ARG, e, out=(d_act, None))
    for t_steps in (0, -3, T + 1):
        refused(L.VS_ERR_ARG, e, t_steps)
    e.set_traj_offset(3)
    refused(L.VS_ERR_STATE, e)
    with pytest.raises(RuntimeError):  # the Python face raises
        e.rollout_vjp_policy(T)
    e.set_traj_offset(0)
    e.set_auto_reset(True)
    refused(L.VS_ERR_STATE, e)
    e.set_auto_reset(False)
    e.set_policy_population(np.tile(c["W"].reshape(1, -1), (3, 1)), lane_set=np.arange(N) // 64)
    refused(L.VS_ERR_STATE, e)
    e.set_policy_population(None)
    assert call(e) == L.VS_OK and not bool((d_act == 7.0).any()) and not bool((d_init == 7.0).any())  # the same handle still serves
    d_act.fill_(7.0), d_init.fill_(7.0)
    e.set_policy_linear(None, None)                             # no policy
    refused(L.VS_ERR_STATE, e)
    n_fnn = (d["O"] + 1) * 8 + (8 + 1) * d["A"]
    e.set_policy_fnn(np.zeros(n_fnn, dtype=np.float32), [8])    # an FNN policy
    refused(L.VS_ERR_STATE, e)
    e.set_policy_playback(np.zeros((N, T, d["A"]), dtype=np.float32))  # a playback policy
    refused(L.VS_ERR_STATE, e)
    linear()
    assert call(e) == L.VS_OK
    d_act.fill_(7.0), d_init.fill_(7.0)
    e.set_record_mode(1)
    e.set_traj_capacity(T)
    refused(L.VS_ERR_STATE, e)
    assert e.error_count() == 0
    e.close()
    disc = vs.VecSimEnv("bob-d", 64, dt=0.01, max_steps=MAX_STEPS)
    disc.set_record_mode(2)
    disc.set_traj_capacity(T)
    o1, o2 = torch.full((T, 1, disc.ld), 7.0, device="cuda"), torch.full((4, disc.ld), 7.0, device="cuda")
    assert lib.vs_rollout_vjp_policy(disc._h, T, None, None, None, None, ptr(o1), ptr(o2)) == L.VS_ERR_STATE
    torch.cuda.synchronize()
    assert bool((o1 == 7.0).all()) and bool((o2 == 7.0).all())
    disc.close()


# ----------------------------------------------------------------------------------------------------------- 7. autograd
def torch_case(name):
    return clc.torch_case("linear", name)


def oracle_loss(name, W, s0, length=None):
    """[NT] per-lane loss -discounted return + 1e-3 sum a^2 of the fp64 closed loop under the weights W [A, F], and the lane lengths"""
    return clc.oracle_loss(torch_case(name), linear_policy(clc.SMALL, None, W), s0, length)


@functools.lru_cache(maxsize=None)
def oracle_loss_gradients(name):
    """central differences at relative steps 1e-6 and 1e-5 per unit of |W| (the whole weight vector: [1, A F]) and of INIT_SCALE
    ([NT, S])"""
    tc = torch_case(name)
    W0, s0 = tc["W"].astype(np.float64), tc["init"].astype(np.float64)
    length = oracle_loss(name, W0, s0)[1]
    gw, gs = [], []
    for h in (1e-6, 1e-5):
        g = np.zeros(W0.shape)
        for idx in np.ndindex(*W0.shape):
            d = np.zeros_like(W0)
            d[idx] = h * abs(W0[idx])
            g[idx] = (oracle_loss(name, W0 + d, s0, length)[0].sum() - oracle_loss(name, W0 - d, s0, length)[0].sum()) / (2.0 * h)
        gw.append(g.reshape(1, -1))
        g = np.zeros(s0.shape)
        for j in range(s0.shape[1]):
            d = np.zeros_like(s0)
            d[:, j] = h * INIT_SCALE[name][j]
            g[:, j] = (oracle_loss(name, W0, s0 + d, length)[0] - oracle_loss(name, W0, s0 - d, length)[0]) / (2.0 * h)
        gs.append(g)
    return gw, gs, length


@pytest.mark.parametrize("name", ["qq-su", "qcp-su"])
def test_autograd(vs, name):
    tc = torch_case(name)
    gw, gs, length = oracle_loss_gradients(name)
    for pair in (gw, gs):
        assert (~smooth_per_lane(*pair)).mean() <= 0.01
    env = getattr(vs, ENVS[name])(max_steps=MAX_STEPS, **KW[name])
    policy = vs.LinearPolicy(env.spec, vs.FeatureStack(vs.identity_feat, vs.sin_feat, vs.const_feat, vs.MultFeat((0, 1))))
    roll = vs.DifferentiablePolicyRollout(env, policy)
    wscale = np.abs(tc["W"].astype(np.float64))

    def loss_of(init):
        obs, rew, act, lengths = roll(init, TT)
        assert tuple(obs.shape) == (NT, TT + 1, tc["ref"].O) and tuple(rew.shape) == (NT, TT) and tuple(act.shape) == (NT, TT, tc["ref"].A)
        assert not lengths.requires_grad and np.array_equal(lengths.cpu().numpy(), length)
        return -vs.discounted_return(rew, lengths, GAMMA).sum() + 1e-3 * act.pow(2).sum()

    with torch.no_grad():
        policy.net.weight.copy_(torch.as_tensor(tc["W"]))
    init = dev(tc["init"]).requires_grad_(True)
    loss = loss_of(init)
    g1 = torch.autograd.grad(loss, (policy.net.weight, init), retain_graph=True)
    with torch.no_grad():
        roll(dev(tc["init"]) * 0.5, TT)  # another forward call overwrites the records
    g2 = torch.autograd.grad(loss, (policy.net.weight, init))  # the re-record path
    assert all(torch.equal(a, b) for a, b in zip(g1, g2))
    got_w = (g1[0].detach().cpu().numpy().astype(np.float64) * wscale).reshape(1, -1)
    got_s = g1[1].cpu().numpy().astype(np.float64) * np.array(INIT_SCALE[name])
    for what, got, (f1, f2) in (("weights", got_w, gw), ("init_states", got_s, gs)):
        bad, worst = within_per_lane(got, f1, smooth_per_lane(f1, f2))
        print(f"{name} {what}: bad share {bad:.2e}, worst error / tolerance {worst:.3f}")
        assert bad <= 2e-3, (name, what, bad, worst)
    # ---- two steps of plain gradient descent on the weights (in units of |W|) lower the oracle's loss
    s0 = tc["init"].astype(np.float64)
    eta = 0.02 * np.sqrt(wscale.size) / np.linalg.norm(gw[0])
    losses = [oracle_loss(name, tc["W"].astype(np.float64), s0, length)[0].sum()]
    for _ in range(2):
        policy.net.weight.grad = None
        loss_of(dev(tc["init"])).backward()
        with torch.no_grad():
            policy.net.weight -= eta * policy.net.weight.grad * torch.as_tensor(wscale ** 2, dtype=torch.float32)
        losses.append(oracle_loss(name, policy.net.weight.detach().numpy().astype(np.float64), s0, length)[0].sum())
    print(f"{name}: oracle loss {losses[0]:.6f} -> {losses[1]:.6f} -> {losses[2]:.6f}")
    assert losses[2] < losses[1] < losses[0], losses
    roll.close()
