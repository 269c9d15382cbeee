"""
vs_rollout_vjp_fnn / k_rollout_vjp_fnn: the reverse-mode sweep over CLOSED-LOOP recorded rollouts with a feed-forward network of one or
two hidden layers in the loop, VecSimEnv.rollout_vjp_fnn and DifferentiableNetRollout.

Shapes, cotangents, scales and the per-lane tolerance rule are those of test_gpu_policy_vjp.py, both from derivative_cases.py: 150 lanes
(64 + 64 + 22: a partial last workgroup), T = 24, max_steps = 50, +-5 % per-lane parameters, lanes 0 .. 9 start at the edge of the state space and
end early, random cotangents on all four inputs; per lane 3e-3 |g| + 3e-4 max |g| against central differences of the fp64 closed loop at
relative steps 1e-6 and 1e-5 (oracle.cpu_ref for the step, the NumPy network of closed_loop_cases.py for the policy).  Here EVERY entry must be smooth (the
two step sizes agree; asserted from the oracle alone) and every entry is held to the tolerance: none is excluded.

The weights (closed_loop_cases.make_net) keep every lane inside the action box and outside the dead zones, and no unit near a kink:
  * every layer's input is measured on a rollout under the bias action alone: mid and dev = half its range per row;
  * a hidden pre-activation is b + W (x - mid) with |b| drawn from the case's range with a random sign and
    |W (x - mid)| <= amp on that rollout (relu: |b| in [0.5, 1.5], amp 0.3, rows scaled by 1 / fan-in, so that no unit comes near 0 --
    asserted at 1e-3 on the fp64 closed loop before the GPU is asked; tanh / sigmoid: |b| <= 0.7, amp 1, rows scaled by 1 / sqrt(fan-in));
  * the output layer adds at most +-gain x 0.12 ACT_IN to a bias of +-0.45 ACT_IN on that rollout (its rows are scaled by 1 / fan-in,
    so the sum uses a fraction of the bound; what is asserted on the closed loop is section 8e's box, |a| in [0.30, 0.60] ACT_IN); under
    a tanh output nonlinearity the same in the pre-activation: +-0.24 around +-atanh(0.7), |a| in [0.51, 0.83] asserted -- beyond the
    ball balancer's dead zone (up to 0.28 V x 1.05) and inside its box;
  * seed and gain of a case are chosen on the CPU, from the oracle alone: gain 1 to 3 until the closed-loop and open-loop differences
    part on at least half of the full-length lanes, the seed so that every entry is smooth and (relu) the lone unit of [1] is alive.
"""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import closed_loop_cases as clc  # noqa: E402
from closed_loop_cases import (ENVS, FNN_AUTOGRAD as AUTOGRAD, FNN_ORACLE_CASES as ORACLE_CASES, GAMMA, NT, TT, case,  # noqa: E402
                               check_no_unit_near_a_kink, cotangents, feedback_seen, flat_params, fnn_policy, hidden_reference, mlp,
                               oracle_reference, recorded, reference, set_net)
from derivative_cases import (ACT_IN, HIDDEN_FAMILIES, INIT_SCALE, KW, MAX_STEPS, N, N_EDGE, STARTS, STATE_BUFFERS, T,  # noqa: E402
                              check_hidden_block, check_hidden_start, check_net_keeps_the_box, dev, hidden_conditions, hidden_start, scaled,
                              scaled_hidden, smooth_per_lane, tolerance_per_lane, worst_of)

DEGENERATE = {"omo": "omo-63x7-relu", "bob": "bob-8", "qq-su": "qq-su-64x64-feat", "qcp-su": "qcp-su-32x33", "pend": "pend-8",
              "qbb": "qbb-31x64-tanh-out"}


@pytest.fixture(scope="module")
def vs():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import simurlacra_amd

    return simurlacra_amd


# ----------------------------------------------------------------------------------- 1. + 2. against the fp64 closed loop
@pytest.mark.parametrize("key", ORACLE_CASES)
def test_against_the_closed_loop_fp64_oracle(vs, key):
    """Worst error / tolerance over all entries, measured on the MI355X (printed with -s): 0.001 (QQube [16],
    cartpole, both oscillator networks), 0.002 (QQube [64, 64] with feat, pendulum through obs_idx), below 0.0005 (ball balancer); the
    feedback is seen on 0.61 (pendulum) to 0.98 (oscillator [1]) of the full-length lanes, by the oracle and by the device alike."""
    c = case(key)
    ref = c["ref"]
    r = oracle_reference(key)
    f1, length = r.f1, r.length
    smooth = smooth_per_lane(f1, r.f2)
    assert smooth.all(), (key, float((~smooth).mean()))  # from the oracle alone: every entry, none excluded
    check_net_keeps_the_box(c, r.acts, length)
    check_no_unit_near_a_kink(c, r.pres, length)
    assert (length[:N_EDGE] < T).any() and (length[N_EDGE:] == T).mean() > 0.9  # lanes that end early, lanes that run through
    seen = feedback_seen(c, f1, smooth, r.open_init, length)
    assert seen >= 0.5, (key, seen)  # from the oracle alone: the test can see the feedback
    e = recorded(vs, key)
    assert np.array_equal(e.rollout_lengths(N, T)[0].cpu().numpy(), length)
    cot = cotangents(vs, key, e)
    got = scaled(vs, c, *e.rollout_vjp_fnn(T, **cot))
    # ---- 2. the feedback is there: along the same records the open-loop sweep's d_init is off where the oracle says it must be
    # (state columns only: the feedback enters through the observations, which no hidden state reaches; the hidden rows of both sweeps
    # have their own tests, test_hidden_adjoint_against_the_closed_loop_fp64_oracle here and in test_gpu_rollout_vjp.py)
    _, oi = e.rollout_vjp(T, **{k: v for k, v in cot.items() if k != "g_act"})
    open_got = vs.lanes_first(oi, N).cpu().numpy()[:, :ref.S].astype(np.float64) * np.array(INIT_SCALE[c["name"]])
    init_cols = slice(T * ref.A, None)
    differs = (np.abs(got[:, init_cols] - open_got) > 10.0 * tolerance_per_lane(f1, smooth)[:, init_cols]).any(axis=1)
    assert e.error_count() == 0
    e.close()
    worst = worst_of(got, f1, smooth)
    print(f"{key}: feedback seen on {seen:.2f} (oracle) / {differs[length == T].mean():.2f} (device) of the full lanes, "
          f"worst error / tolerance {worst:.3f}")
    assert differs[length == T].mean() >= 0.5, (key, float(differs[length == T].mean()))
    assert worst <= 1.0, (key, worst)


HIDDEN_CASES = {"qcp-su": "qcp-su-32x33", "qbb": "qbb-31x64-tanh-out"}


@pytest.mark.parametrize("start", STARTS)
@pytest.mark.parametrize("name", HIDDEN_FAMILIES)
def test_hidden_adjoint_against_the_closed_loop_fp64_oracle(vs, name, start):
    """Rows S .. S + H - 1 of d_init (scaled() cuts them off: they have another unit and another rule) against central differences of the
    closed loop's Phi at HIDDEN_STEPS x HIDDEN_SCALE, per column and per HIDDEN_SCALE, from the hidden state that reset leaves and from
    hidden_start(); edge lanes like any other, lanes >= n exactly 0.  From hidden_start() the offset and state columns go through test
    1's check as well (every entry smooth, every entry held), the network keeps the box and stays off its kinks.  Worst error /
    tolerance per column as measured on the MI355X (printed with -s): DESIGN.md section 8d."""
    key = HIDDEN_CASES[name]
    c = case(key)
    g1, g2, length = hidden_reference(key, start)
    hidden_conditions(key, g1, g2)  # from the oracle alone, before the device is asked
    hidden = hidden_start(name, c) if start == "perturbed" else None
    e = recorded(vs, key, hidden=hidden)
    if hidden is None:
        assert np.array_equal(e.rollout_lengths(N, T)[0].cpu().numpy(), length)
    else:
        check_hidden_start(e, hidden, length)
    da, di = e.rollout_vjp_fnn(T, **cotangents(vs, key, e))
    assert e.error_count() == 0 and e.ld > N and not da[..., N:].any() and not di[..., N:].any()
    e.close()
    check_hidden_block(f"{key} vs_rollout_vjp_fnn from {start}", scaled_hidden(vs, c, di), g1, g2)
    if start == "perturbed":
        r = oracle_reference(key, start)
        f1, smooth = r.f1, smooth_per_lane(r.f1, r.f2)
        assert np.array_equal(r.length, length) and smooth.all(), (key, float((~smooth).mean()))  # from the oracle alone
        check_net_keeps_the_box(c, r.acts, length)
        check_no_unit_near_a_kink(c, r.pres, length)
        worst = worst_of(scaled(vs, c, da, di), f1, smooth)
        print(f"{key} from {start}: offsets and states: worst error / tolerance {worst:.3f}")
        assert worst <= 1.0, (key, worst)


def test_exploration_noise_is_an_additive_constant(vs):
    """The network inside a NormalActNoiseExplStrat, handed over as fnn_kernel_spec describes it.  The recorded raw action contains the
    noise: n_t = a_recorded - net(obs_recorded), taken from the records in fp64, is fed to the oracle as a constant offset; the comparison
    is test 1's."""
    key = "pend-8"
    c = case(key)
    ref = c["ref"]
    env = vs.PendulumSim(max_steps=MAX_STEPS, **KW[c["name"]])
    policy = vs.NormalActNoiseExplStrat(vs.FNNPolicy(env.spec, list(c["net"]["hidden"]), torch.tanh, featurize=False),
                                        std_init=0.02 * ACT_IN[c["name"]])
    policy.policy.param_values = torch.as_tensor(flat_params(c["net"]))
    e = recorded(vs, key, spec=vs.fnn_kernel_spec(policy), noise_seed=77)
    tt = e.traj_tensors(T, N)
    obs, act = tt["obs"].cpu().numpy().astype(np.float64), tt["act"].cpu().numpy().astype(np.float64)  # [T, N, .]
    offs = (act - mlp(c["net"], obs.reshape(T * N, ref.O))[0].reshape(T, N, ref.A)).transpose(1, 0, 2)
    assert 0.5 < offs[N_EDGE:].std() / (0.02 * ACT_IN[c["name"]]) < 1.5  # the noise is there
    r = reference(c, np.ascontiguousarray(offs))
    f1, length, smooth = r.f1, r.length, smooth_per_lane(r.f1, r.f2)
    assert smooth.all()
    assert np.array_equal(e.rollout_lengths(N, T)[0].cpu().numpy(), length)
    got = scaled(vs, c, *e.rollout_vjp_fnn(T, **cotangents(vs, key, e)))
    assert e.error_count() == 0
    e.close()
    worst = worst_of(got, f1, smooth)
    print(f"{key} + noise: worst error / tolerance {worst:.3f}")
    assert worst <= 1.0, worst


# ------------------------------------------------------------------------------------------------- 3. degenerate network
@pytest.mark.parametrize("name", sorted(DEGENERATE))
def test_a_constant_network_reduces_to_the_open_loop_sweep(vs, name):
    """a first layer of all-zero weights: the policy is a constant, gpol is 0 and the two sweeps agree by value"""
    key = DEGENERATE[name]
    net = dict(case(key)["net"])
    net["W"] = [np.zeros_like(net["W"][0])] + list(net["W"][1:])
    e = recorded(vs, key, net=net)
    cot = cotangents(vs, key, e, with_act=False)
    oa, oi = e.rollout_vjp(T, **cot)
    pa, pi = e.rollout_vjp_fnn(T, **cot)
    assert not torch.isnan(pa).any() and not torch.isnan(pi).any()
    assert bool((pa == oa).all()) and bool((pi == oi).all()) and bool(oa.any()) and bool(oi.any())
    assert e.error_count() == 0
    e.close()


# ------------------------------------------------------------------------------------------------------------- 4. edges
@pytest.mark.parametrize("key", ["qq-su-64x64-feat", "qcp-su-32x33"])
def test_edges(vs, key):
    L = vs._lib
    e = recorded(vs, key)
    cot = cotangents(vs, key, e)
    before = [e.get(getattr(L, b)).copy() for b in STATE_BUFFERS]
    planes, words = e.traj_planes()
    rows = [p.clone() for p, _ in planes] + [words.clone()]
    da, di = e.rollout_vjp_fnn(T, **cot)
    for b, x in zip(STATE_BUFFERS, before):  # the handle's state, step counter and flags are untouched
        assert np.array_equal(e.get(getattr(L, b)), x), b
    planes, words = e.traj_planes()
    assert all(torch.equal(a, b) for a, b in zip([p for p, _ in planes] + [words], rows)) and e.error_count() == 0  # the record rows
    assert e.ld > N and not da[..., N:].any() and not di[..., N:].any()  # lanes >= n up to ld: exactly 0
    d_act = vs.lanes_first(da, N).cpu().numpy()
    length = e.rollout_lengths(N, T)[0].cpu().numpy()
    early = np.flatnonzero(length < T)
    assert early.size > 0 and (early < N_EDGE).all()
    for n in early:
        assert not d_act[n, length[n]:].any() and d_act[n, :length[n]].all()
    assert d_act[length == T].all() and bool(di[:, :N].any(dim=0).all())
    for kw in ({k: torch.zeros_like(v) for k, v in cot.items()}, {}):  # zero cotangents, and none at all
        za, zi = e.rollout_vjp_fnn(T, **kw)
        assert not za.any() and not zi.any()
    # ---- t_steps below the capacity: the sweep over the first 17 rows is the sweep of a 17-step rollout
    short = {k: v[:17 + (k == "g_obs")].contiguous() if k != "g_state_last" else v for k, v in cot.items()}
    sa, si = e.rollout_vjp_fnn(17, **short)
    assert tuple(sa.shape) == (17, da.shape[1], e.ld) and bool(sa[..., :N].any()) and bool(torch.isfinite(sa).all())
    f = recorded(vs, key, splits=(17,))
    fa, fi = f.rollout_vjp_fnn(17, **short)
    assert torch.equal(fa, sa) and torch.equal(fi, si)
    assert e.error_count() == 0 and f.error_count() == 0
    f.close()
    e.close()


# ------------------------------------------------------------------------------------ 5. records from both forward shapes
def test_records_from_both_forward_shapes(vs):
    key, n = "qq-su-64x64-feat", 320
    c = case(key)
    f1, f2 = oracle_reference(key).f1, oracle_reference(key).f2
    res = []
    for shape in ("64", "mfma"):
        e = recorded(vs, key, n=n, shape=shape)
        res.append(scaled(vs, c, *e.rollout_vjp_fnn(T, **cotangents(vs, key, e, n=n)), n=n))
        assert e.error_count() == 0
        e.close()
    rep = lambda x: np.resize(x, (n,) + x.shape[1:])  # noqa: E731  (lane k repeats lane k % N of the case)
    tol = tolerance_per_lane(rep(f1), rep(smooth_per_lane(f1, f2)))
    worst = float((np.abs(res[0] - res[1]) / tol).max())
    print(f"{key}: 64-env against matrix-core records, worst difference / tolerance {worst:.3f}")
    assert worst <= 1.0, worst


# ---------------------------------------------------------------------------------------------------------- 6. refusals
def test_refusals_leave_the_outputs_untouched(vs):
    L = vs._lib
    lib = L.load()
    key = "qq-su-16"
    c = case(key)
    d = vs.env_dims(c["name"])
    e = recorded(vs, key)
    d_act = torch.full((T, d["A"], e.ld), 7.0, device="cuda")
    d_init = torch.full((d["S"] + d["H"], e.ld), 7.0, device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def call(handle, t_steps=T, out=(d_act, d_init)):
        rc = lib.vs_rollout_vjp_fnn(handle._h if handle is not None else None, t_steps, None, None, None, None,
                                    ptr(out[0]) if out[0] is not None else None, ptr(out[1]) if out[1] is not None else None)
        torch.cuda.synchronize()
        return rc

    def refused(code, *args, **kw):
        assert call(*args, **kw) == code
        assert bool((d_act == 7.0).all()) and bool((d_init == 7.0).all())  # the sentinels

    def served():
        assert call(e) == L.VS_OK and not bool((d_act == 7.0).any()) and not bool((d_init == 7.0).any())
        d_act.fill_(7.0), d_init.fill_(7.0)

    refused(L.VS_ERR_ARG, None)
    refused(L.VS_ERR_ARG, e, out=(None, d_init))
    refused(L.VS_ERR_ARG, e, out=(d_act, None))
    for t_steps in (0, -3, T + 1):
        refused(L.VS_ERR_ARG, e, t_steps)
    e.set_traj_offset(3)
    refused(L.VS_ERR_STATE, e)
    with pytest.raises(RuntimeError):  # the Python face raises
        e.rollout_vjp_fnn(T)
    e.set_traj_offset(0)
    e.set_auto_reset(True)
    refused(L.VS_ERR_STATE, e)
    e.set_auto_reset(False)
    e.set_policy_population(np.tile(flat_params(c["net"])[None, :], (3, 1)), lane_set=np.arange(N) // 64)
    refused(L.VS_ERR_STATE, e)
    e.set_policy_population(None)
    served()                                                    # the same handle still serves
    e.set_policy_fnn(None, None)                                # no policy
    refused(L.VS_ERR_STATE, e)
    e.set_policy_linear(np.zeros(d["A"], dtype=np.float32), ["const"])  # a linear policy
    refused(L.VS_ERR_STATE, e)
    n_gru = 3 * 8 * (d["O"] + 8 + 2) + (8 + 1) * d["A"]
    e.set_policy_rnn(np.zeros(n_gru, dtype=np.float32), cell="gru", n_layers=1, hidden_size=8)  # a recurrent policy
    refused(L.VS_ERR_STATE, e)
    e.set_policy_playback(np.zeros((N, T, d["A"]), dtype=np.float32))  # a playback policy
    refused(L.VS_ERR_STATE, e)
    n3 = (d["O"] + 1) * 8 + 2 * (8 + 1) * 8 + (8 + 1) * d["A"]
    e.set_policy_fnn(np.zeros(n3, dtype=np.float32), [8, 8, 8])  # three hidden layers
    refused(L.VS_ERR_STATE, e)
    set_net(e, c["net"])
    served()
    e.set_record_mode(1)
    e.set_traj_capacity(T)
    refused(L.VS_ERR_STATE, e)
    e.set_record_mode(2)
    e.set_traj_capacity(T)
    served()                                                    # after the refusals the same handle serves a good call
    assert e.error_count() == 0
    e.close()
    disc = vs.VecSimEnv("bob-d", 64, dt=0.01, max_steps=MAX_STEPS)
    disc.set_record_mode(2)
    disc.set_traj_capacity(T)
    o1, o2 = torch.full((T, 1, disc.ld), 7.0, device="cuda"), torch.full((4, disc.ld), 7.0, device="cuda")
    assert lib.vs_rollout_vjp_fnn(disc._h, T, None, None, None, None, ptr(o1), ptr(o2)) == L.VS_ERR_STATE
    torch.cuda.synchronize()
    assert bool((o1 == 7.0).all()) and bool((o2 == 7.0).all())
    disc.close()


# ----------------------------------------------------------------------------------------------------------- 7. autograd
def torch_case(name):
    return clc.torch_case("fnn", name)


def with_params(net, flat):
    """the network with the flat parameter vector (torch's order, fp64) in place of its own"""
    out, at = dict(net), 0
    out["W"], out["b"] = [], []
    for W, b in zip(net["W"], net["b"]):
        out["W"].append(flat[at:at + W.size].reshape(W.shape))
        out["b"].append(flat[at + W.size:at + W.size + b.size])
        at += W.size + b.size
    return out


def oracle_loss(name, flat, s0, length=None):
    """[NT] per-lane loss -discounted return + 1e-3 sum a^2 of the fp64 closed loop under the flat parameters, and the lane lengths"""
    tc = torch_case(name)
    return clc.oracle_loss(tc, fnn_policy(with_params(tc["net"], flat)), s0, length)


def chosen_entries(name, n_params):
    """every parameter of the small network, a fixed random 200 of the large one"""
    return np.arange(n_params) if n_params <= 200 else np.sort(np.random.default_rng(41).choice(n_params, 200, replace=False))


@functools.lru_cache(maxsize=None)
def oracle_loss_gradients(name):
    """central differences at relative steps 1e-6 and 1e-5 per unit of |theta| (the chosen entries: [1, n]) and of INIT_SCALE ([NT, S])"""
    tc = torch_case(name)
    th0, s0 = flat_params(tc["net"]).astype(np.float64), tc["init"].astype(np.float64)
    length = oracle_loss(name, th0, s0)[1]
    which = chosen_entries(name, th0.size)
    gw, gs = [], []
    for h in (1e-6, 1e-5):
        g = np.zeros(which.size)
        for q, idx in enumerate(which):
            d = np.zeros_like(th0)
            d[idx] = h * abs(th0[idx])
            g[q] = (oracle_loss(name, th0 + d, s0, length)[0].sum() - oracle_loss(name, th0 - d, s0, length)[0].sum()) / (2.0 * h)
        gw.append(g.reshape(1, -1))
        g = np.zeros(s0.shape)
        for j in range(s0.shape[1]):
            d = np.zeros_like(s0)
            d[:, j] = h * INIT_SCALE[name][j]
            g[:, j] = (oracle_loss(name, th0, s0 + d, length)[0] - oracle_loss(name, th0, s0 - d, length)[0]) / (2.0 * h)
        gs.append(g)
    return gw, gs, length


@pytest.mark.parametrize("name", ["qq-su", "qcp-su"])
def test_autograd(vs, name):
    tc = torch_case(name)
    gw, gs, length = oracle_loss_gradients(name)
    for pair in (gw, gs):
        assert smooth_per_lane(*pair).all()
    env = getattr(vs, ENVS[name])(max_steps=MAX_STEPS, **KW[name])
    policy = vs.FNNPolicy(env.spec, hidden_sizes=list(AUTOGRAD[name]), hidden_nonlin=torch.tanh, featurize=False)
    roll = vs.DifferentiableNetRollout(env, policy)
    th0 = flat_params(tc["net"])
    which = chosen_entries(name, th0.size)
    scale = np.abs(th0.astype(np.float64))

    def loss_of(init):
        obs, rew, act, lengths = roll(init, TT)
        assert tuple(obs.shape) == (NT, TT + 1, tc["ref"].O) and tuple(rew.shape) == (NT, TT) and tuple(act.shape) == (NT, TT, tc["ref"].A)
        assert not lengths.requires_grad and np.array_equal(lengths.cpu().numpy(), length)
        return -vs.discounted_return(rew, lengths, GAMMA).sum() + 1e-3 * act.pow(2).sum()

    def flat_grad(grads):
        return torch.cat([g.reshape(-1) for g in grads]).detach().cpu().numpy().astype(np.float64)

    policy.param_values = torch.as_tensor(th0)
    weights = list(policy.parameters())
    init = dev(tc["init"]).requires_grad_(True)
    loss = loss_of(init)
    g1 = torch.autograd.grad(loss, weights + [init], retain_graph=True)
    with torch.no_grad():
        roll(dev(tc["init"]) * 0.5, TT)  # another forward call overwrites the records
    g2 = torch.autograd.grad(loss, weights + [init])  # the re-record path
    assert all(torch.equal(a, b) for a, b in zip(g1, g2))
    got_w = (flat_grad(g1[:-1]) * scale)[which].reshape(1, -1)
    got_s = g1[-1].cpu().numpy().astype(np.float64) * np.array(INIT_SCALE[name])
    for what, got, (f1, f2) in (("parameters", got_w, gw), ("init_states", got_s, gs)):
        worst = worst_of(got, f1, smooth_per_lane(f1, f2))
        print(f"{name} {what}: worst error / tolerance {worst:.3f}")
        assert worst <= 1.0, (name, what, worst)
    # ---- two steps of plain gradient descent on the parameters (in units of |theta|) lower the oracle's loss; the step size moves no
    # parameter by more than 2 % of its magnitude in the first step (thousands of parameters: a rule on the norm would let the few
    # entries that carry it move by more than their size)
    s0 = tc["init"].astype(np.float64)
    eta = 0.02 / np.abs(flat_grad(g1[:-1]) * scale).max()
    losses = [oracle_loss(name, th0.astype(np.float64), s0, length)[0].sum()]
    for _ in range(2):
        for p in weights:
            p.grad = None
        loss_of(dev(tc["init"])).backward()
        with torch.no_grad():
            step = eta * flat_grad([p.grad for p in weights]) * scale ** 2
            policy.param_values = policy.param_values - torch.as_tensor(step, dtype=torch.float32)
        losses.append(oracle_loss(name, policy.param_values.detach().cpu().numpy().astype(np.float64), s0, length)[0].sum())
    print(f"{name}: oracle loss {losses[0]:.6f} -> {losses[1]:.6f} -> {losses[2]:.6f}")
    assert losses[2] < losses[1] < losses[0], losses
    roll.close()
