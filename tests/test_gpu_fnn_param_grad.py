"""
vs_fnn_param_grad / k_fnn_param_grad + k_fnn_param_reduce: the parameter gradient of a feed-forward network policy over the recorded
rows of a handle, VecSimEnv.fnn_param_grad and DifferentiableNetRollout(param_pass="kernel").

Shapes, networks and seeds are those of test_gpu_fnn_vjp.py (closed_loop_cases.py has the cases): 150 lanes (64 + 64 + 22), T = 24, +-5 % per-lane
parameters, lanes 0 .. 9 end early.  abar is random and dense and is fed directly.

Reference: test_fnn_param_grad_host.param_grad_fp64 -- the sum restated in fp64 over the RECORDED observations and lengths (held to
torch.autograd.grad of the .double() module at 1e-12 in that file, without a device).

Tolerance, per parameter p: the first-order bound of test_fnn_param_grad_host.error_bound (derived in its docstring),
    bound_p = sum_rows (|delta| e(y) + |y| e(delta)) + gamma(acc + 3 + wg + 1) sum_rows |term_p|,      gamma(m) = m 2^-24,
where e(.) carries tanh_fast's 2e-7, the sigmoid's 4e-7, sincos_fast's 4e-7 and the rounding of every fp32 chain the kernel runs
(12 / 19 / 8 operations per forward layer, A or 19 per pull-back) through the fp64 reference's own values, and the accumulation chain is
read off the launch: acc = the rows one wave sums in its registers (64 per tile of its run), 3 adds across the four waves, wg = the adds
of k_fnn_param_reduce across the workgroups (n_wg / 4 per partial sum, 2 to join them), 1 for accumulate.  The grid is mirrored from the
documented rule (grid_of).  The kernel is held to the fp64 reference within bound_p and to the fp32 torch pass of the same rows within
twice it.  The bound is not tuned to the measurement; the worst measured ratio per case is printed (-s) and recorded in DESIGN.md 8h.

Which assertion catches which kernel mistake:
  * a missing L select                  test_nan_behind_the_rows_changes_no_bit (NaN at t >= L, at lanes >= n and behind t_steps), and every
                                        table case (lanes 0 .. 9 end early: the reference leaves their tails out)
  * padding leaking into d_params       omo-1-relu (63 padding units) and qbb-31x64-tanh-out (33 padding units in layer 1): the flat
                                        vector has exactly the network's entries and each is compared
  * a transposed dW_2                   qcp-su-32x33 (unequal widths: [33, 32] against [32, 33])
  * a dropped g'                        qbb-31x64-tanh-out (tanh output nonlinearity)
  * a nondeterministic reduction        test_two_calls_and_accumulate_are_exact, test_nan_behind_the_rows_changes_no_bit, the autograd test's
                                        backward-twice assertion
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import closed_loop_cases as clc  # noqa: E402  (cases, networks, seeds)
import test_fnn_param_grad_host as host  # noqa: E402  (the fp64 reference and its error bound)
from derivative_cases import ACT_IN, KW, MAX_STEPS, N, N_EDGE, STATE_BUFFERS, T, dev, record_mode2  # noqa: E402

TABLE = ["omo-1-relu", "omo-63x7-relu", "qq-su-16", "qq-su-64x64-feat", "qcp-su-32x33", "qbb-31x64-tanh-out", "pend-view-8-sigmoid"]


@pytest.fixture(scope="module")
def vs():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import simurlacra_amd

    return simurlacra_amd


def grid_of(ld, t_steps):
    """(workgroups, rows a wave accumulates at most) of the launch: a wave per tile while there are fewer tiles than wave slots, else two
    workgroups of four waves per compute unit, each wave a contiguous run of tiles"""
    tiles = (ld // 64) * t_steps
    n_wg = min(-(-tiles // 4), 2 * torch.cuda.get_device_properties(0).multi_processor_count)
    return n_wg, 64 * -(-tiles // (4 * n_wg))


def recorded(vs, key, n=N, t=T, lanes=None, spec=None, noise_seed=0, cap=None):
    """closed_loop_cases.recorded with the number of steps free: rows 0 .. t - 1 hold the closed-loop rollouts of the case (lane k repeats lane k % N,
    or the case's lanes `lanes`)"""
    c = clc.case(key)
    name = c["name"]
    pick = (lambda x: np.resize(x, (n,) + x.shape[1:])) if lanes is None else (lambda x: np.resize(x[lanes], (n,) + x.shape[1:]))
    e = vs.VecSimEnv(name, n, max_steps=MAX_STEPS, **KW[name])

    def policy(e):
        if spec is None:
            clc.set_net(e, c["net"])
        else:
            e.set_policy_fnn(**spec)

    return record_mode2(e, t if cap is None else cap, pick(c["params"]), policy, pick(c["init"]), (t,), noise_seed=noise_seed)


def abar_of(key, n, t, seed=0):
    A = clc.case(key)["ref"].A
    return np.random.default_rng(1000 + seed).normal(size=(n, t, A)).astype(np.float32)


def rows_of(e, n, t):
    """(obs [t n, O], inside [t n], lengths [n]) of the handle's records, step-major"""
    obs = e.traj_tensors(t, n)["obs"].cpu().numpy()  # [t, n, O]
    length = e.rollout_lengths(n, t)[0].cpu().numpy()
    inside = np.arange(t)[:, None] < length[None, :]
    return obs.reshape(t * n, -1), inside.reshape(-1), length


def reference(e, net, n, t, abar, more_adds=0):
    """(fp64 gradient, bound, hidden pre-activations, lengths, obs rows, inside) for the handle's records"""
    obs, inside, length = rows_of(e, n, t)
    n_wg, acc = grid_of(e.ld, t)
    want, _, pre, bound = host.param_grad_fp64(net, obs, abar.transpose(1, 0, 2).reshape(t * n, -1), inside,
                                               chains=dict(acc=acc, wg=-(-n_wg // 4) + 2 + more_adds))
    return want, bound, pre, length, obs, inside


def torch_pass(net, obs, abar_rows, inside):
    """the fp32 torch.autograd.grad of the same rows, flat"""
    layers, forward = host.torch_module(net)
    layers.float()
    out = forward(torch.as_tensor(obs[inside]))
    g = torch.autograd.grad(out, list(layers.parameters()), grad_outputs=torch.as_tensor(abar_rows[inside]))
    return torch.cat([x.reshape(-1) for x in g]).numpy().astype(np.float64)


def check_kinks_and_ranges(net, pre):
    """relu: no hidden pre-activation of the fp64 forward within 1e-3 of 0; sigmoid: |z| <= 8 (the bound's assumption)"""
    for kind, z in zip(net["hidden_nonlin"], pre):
        if kind == "relu":
            assert (np.abs(z) >= 1e-3).all()
        if kind == "sigmoid":
            assert (np.abs(z) <= 8.0).all()


def worst_ratio(err, bound):
    """max err / bound; an entry whose bound is 0 (every term of it is 0: a dead relu unit) must be met exactly"""
    return float(np.where(bound > 0.0, err / np.where(bound > 0.0, bound, 1.0), np.where(err == 0.0, 0.0, np.inf)).max())


def held(vs, e, key, net, n, t, abar, what):
    want, bound, pre, length, obs, inside = reference(e, net, n, t, abar)
    check_kinks_and_ranges(net, pre)
    got = e.fnn_param_grad(t, vs.lanes_last(dev(abar), e.ld))
    assert got.dtype == torch.float32 and tuple(got.shape) == (host.flat_of(net["W"], net["b"]).size,) and got.is_cuda
    got = got.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all() and e.error_count() == 0
    tp = torch_pass(net, obs, abar.transpose(1, 0, 2).reshape(t * n, -1), inside)
    r64, r32 = worst_ratio(np.abs(got - want), bound), worst_ratio(np.abs(got - tp), 2.0 * bound)
    print(f"{what}: worst |kernel - fp64| / bound {r64:.3f}, worst |kernel - torch fp32| / (2 bound) {r32:.3f}, "
          f"bound / max |g| {float((bound / np.abs(want).max()).max()):.1e}")
    assert np.abs(want).max() > 0.0 and r64 <= 1.0 and r32 <= 1.0, (what, r64, r32)
    return got, length


# ------------------------------------------------------------------------------------------------------- 1. the table
@pytest.mark.parametrize("key", TABLE)
def test_against_the_fp64_reference(vs, key):
    """Worst |kernel - fp64| / bound and |kernel - torch fp32| / (2 bound) measured on the MI355X (printed with -s):
    oscillator [1] 0.000 / 0.001, [63, 7] 0.002 / 0.005; QQube [16] 0.002 / 0.002, [64, 64] with feat 0.001 / 0.001; cartpole 0.001 /
    0.002; ball balancer 0.001 / 0.003; pendulum through obs_idx 0.002 / 0.003."""
    e = recorded(vs, key)
    _, length = held(vs, e, key, clc.case(key)["net"], N, T, abar_of(key, N, T), key)
    assert (length[:N_EDGE] < T).any() and (length[N_EDGE:] == T).mean() > 0.9  # lanes that end early, lanes that run through
    e.close()


def test_exploration_noise(vs):
    """the network inside a NormalActNoiseExplStrat: the records hold the noisy rollout, the gradient is the mean network's"""
    key = "pend-8"
    c = clc.case(key)
    env = vs.PendulumSim(max_steps=MAX_STEPS, **KW[c["name"]])
    policy = vs.NormalActNoiseExplStrat(vs.FNNPolicy(env.spec, list(c["net"]["hidden"]), torch.tanh, featurize=False),
                                        std_init=0.02 * ACT_IN[c["name"]])
    policy.policy.param_values = torch.as_tensor(clc.flat_params(c["net"]))
    e = recorded(vs, key, spec=vs.fnn_kernel_spec(policy), noise_seed=77)
    quiet = recorded(vs, key)
    assert not torch.equal(e.traj_tensors(T, N)["act"], quiet.traj_tensors(T, N)["act"])  # the noise is there
    quiet.close()
    held(vs, e, key, c["net"], N, T, abar_of(key, N, T), key + " + noise")
    e.close()


# ------------------------------------------------------------------------------------------------------- 2. edges
@pytest.mark.parametrize("n,t", [(1, T), (65, T), (N, 1)])
def test_small_batches(vs, n, t):
    key = "qcp-su-32x33"
    e = recorded(vs, key, n=n, t=t)
    held(vs, e, key, clc.case(key)["net"], n, t, abar_of(key, n, t), f"{key} n={n} T={t}")
    e.close()


def test_t_steps_below_the_capacity(vs):
    key = "qq-su-64x64-feat"
    e = recorded(vs, key)
    short, _ = held(vs, e, key, clc.case(key)["net"], N, 17, abar_of(key, N, 17), key + " 17 of 24 rows")
    f = recorded(vs, key, t=17)
    assert np.array_equal(f.fnn_param_grad(17, vs.lanes_last(dev(abar_of(key, N, 17)), f.ld)).cpu().numpy().astype(np.float64), short)
    f.close()
    e.close()


def test_every_rollout_runs_to_the_end(vs):
    key = "qq-su-16"
    lanes = np.arange(N_EDGE, N)
    e = recorded(vs, key, lanes=lanes)
    full = np.flatnonzero(e.rollout_lengths(N, T)[0].cpu().numpy() == T)
    e.close()
    lanes = lanes[full % lanes.size]  # the case's lanes that run through
    e = recorded(vs, key, lanes=lanes)
    _, length = held(vs, e, key, clc.case(key)["net"], N, T, abar_of(key, N, T), key + " all lanes full")
    assert (length == T).all()
    e.close()


def test_tiles_outnumber_the_waves(vs):
    """2 x 256 workgroups of four waves are 2048 wave slots, and ld is the lane count rounded up to 256.  The issue's 2112 lanes x 40 steps
    are ld = 2304, 1440 tiles: a wave each, the tile loop does not iterate.  The smallest batch that iterates at about that horizon is
    3073 lanes (ld = 3328, 52 lane groups), and with T = 41 -- odd, so that the runs of two tiles do not line up with the lane groups --
    2132 tiles: a wave's run is two tiles, every other group boundary falls INSIDE a run (tiles 40 | 41: the wave re-derives the lanes'
    lengths in mid-run), lane group 48 holds one lane and groups 49 .. 51 none."""
    key, n, t = "qbb-31x64-tanh-out", 3073, 41
    e = recorded(vs, key, n=n, t=t)
    n_wg, acc = grid_of(e.ld, t)
    assert e.ld == 3328 and (e.ld // 64) * t > 4 * n_wg and acc == 128 and t % (acc // 64) != 0
    held(vs, e, key, clc.case(key)["net"], n, t, abar_of(key, n, t), f"{key} n={n} T={t}")
    e.close()


def test_zero_adjoints_give_zeros(vs):
    key = "qcp-su-32x33"
    e = recorded(vs, key)
    out = torch.full((e._fnn_n_params,), 7.0, device="cuda")
    assert e.fnn_param_grad(T, torch.zeros(T, clc.case(key)["ref"].A, e.ld, device="cuda"), out=out) is out
    assert not out.any()
    e.close()


@pytest.mark.parametrize("key", ["qq-su-64x64-feat", "omo-1-relu"])
def test_nan_behind_the_rows_changes_no_bit(vs, key):
    """NaN in abar at every row t >= L, at lanes n .. ld - 1 and in rows t_steps .. of a larger buffer: the same bits as with zeros there"""
    e = recorded(vs, key)
    A = clc.case(key)["ref"].A
    length = e.rollout_lengths(N, T)[0]
    assert e.ld > N and bool((length < T).any())
    big = torch.zeros(T + 5, A, e.ld, device="cuda")
    big[:T, :, :N] = vs.lanes_last(dev(abar_of(key, N, T)), e.ld)[:, :, :N]
    behind = torch.arange(T, device="cuda")[:, None] >= length[None, :]          # [T, N]
    big[:T, :, :N] = torch.where(behind[:, None, :], torch.zeros((), device="cuda"), big[:T, :, :N])
    clean = e.fnn_param_grad(T, big[:T])
    dirty = big.clone()
    dirty[:T, :, :N] = torch.where(behind[:, None, :], torch.full((), float("nan"), device="cuda"), dirty[:T, :, :N])
    dirty[:, :, N:] = float("nan")
    dirty[T:] = float("nan")
    assert bool(torch.isnan(dirty[:T, :, :N]).any())
    got = e.fnn_param_grad(T, dirty[:T])
    assert bool(clean.any()) and bool(torch.isfinite(got).all()) and torch.equal(got, clean)
    e.close()


def test_two_calls_and_accumulate_are_exact(vs):
    key = "qbb-31x64-tanh-out"
    e = recorded(vs, key)
    ab = vs.lanes_last(dev(abar_of(key, N, T)), e.ld)
    g = e.fnn_param_grad(T, ab)
    assert torch.equal(e.fnn_param_grad(T, ab), g) and bool(g.all())
    twice = e.fnn_param_grad(T, ab)
    e.fnn_param_grad(T, ab, out=twice, accumulate=True)
    assert torch.equal(twice, 2.0 * g)
    r = torch.randn(g.shape, device="cuda", generator=torch.Generator("cuda").manual_seed(3))
    out = r.clone()
    e.fnn_param_grad(T, ab, out=out, accumulate=True)
    assert torch.equal(out, r + g)
    with pytest.raises(vs.ValueErr):
        e.fnn_param_grad(T, ab, accumulate=True)
    with pytest.raises(vs.ShapeErr):
        e.fnn_param_grad(T, ab[:, :, :64].contiguous())
    e.close()


def test_the_handle_is_untouched_and_goes_on_serving(vs):
    L = vs._lib
    key = "qq-su-64x64-feat"
    e = recorded(vs, key)
    cot = clc.cotangents(vs, key, e)
    da0, di0 = e.rollout_vjp_fnn(T, **cot)
    before = [e.get(getattr(L, b)).copy() for b in STATE_BUFFERS]
    planes, words = e.traj_planes()
    rows = [p.clone() for p, _ in planes] + [words.clone()]
    g = e.fnn_param_grad(T, da0)  # straight on the sweep's d_act
    for b, x in zip(STATE_BUFFERS, before):
        assert np.array_equal(e.get(getattr(L, b)), x), b
    planes, words = e.traj_planes()
    assert all(torch.equal(a, b) for a, b in zip([p for p, _ in planes] + [words], rows)) and e.error_count() == 0
    da1, di1 = e.rollout_vjp_fnn(T, **cot)
    assert torch.equal(da1, da0) and torch.equal(di1, di0)
    # ---- another policy, then the network again: the workspace went with the first network and comes back
    d = vs.env_dims(clc.case(key)["name"])
    e.set_policy_linear(np.zeros(d["A"], dtype=np.float32), ["const"])
    with pytest.raises(RuntimeError, match="vs_fnn_param_grad"):
        e.fnn_param_grad(T, da0)
    clc.set_net(e, clc.case(key)["net"])
    assert torch.equal(e.fnn_param_grad(T, da0), g)
    # ---- and the handle still steps: the same launch from the same state gives the same records
    f = recorded(vs, key)
    for h in (e, f):
        h.reset(init_state=np.resize(clc.case(key)["init"], (N, clc.case(key)["init"].shape[1])))
        h.set_traj_offset(0)
        h.step_policy(T, record=True)
    assert torch.equal(e.traj_tensors(T, N)["act"], f.traj_tensors(T, N)["act"]) and e.error_count() == 0
    f.close()
    e.close()


# ------------------------------------------------------------------------------------------------------- 3. refusals
def test_refusals_leave_the_output_untouched(vs):
    L = vs._lib
    lib = L.load()
    key = "qq-su-16"
    c = clc.case(key)
    d = vs.env_dims(c["name"])
    e = recorded(vs, key)
    n_params = e._fnn_n_params
    abar = vs.lanes_last(dev(abar_of(key, N, T)), e.ld)
    out = torch.full((n_params + 1,), 7.0, device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731

    def call(handle, t_steps=T, ab=abar, dp=out, n=None):
        rc = lib.vs_fnn_param_grad(handle._h if handle is not None else None, t_steps, ptr(ab), ptr(dp), n_params if n is None else n, 0)
        torch.cuda.synchronize()
        return rc

    def refused(code, handle, **kw):
        assert call(handle, **kw) == code
        assert bool((out == 7.0).all())  # the sentinels
        if handle is not None:
            assert "vs_fnn_param_grad" in lib.vs_last_error(handle._h).decode()

    def served():
        assert call(e) == L.VS_OK and not bool((out[:n_params] == 7.0).any()) and float(out[n_params]) == 7.0
        out.fill_(7.0)

    refused(L.VS_ERR_ARG, None)
    refused(L.VS_ERR_ARG, e, ab=None)
    refused(L.VS_ERR_ARG, e, dp=None)
    for t_steps in (0, -3, T + 1):
        refused(L.VS_ERR_ARG, e, t_steps=t_steps)
    for n in (n_params - 1, n_params + 1):
        refused(L.VS_ERR_ARG, e, n=n)
    e.set_policy_population(np.tile(clc.flat_params(c["net"])[None, :], (3, 1)), lane_set=np.arange(N) // 64)
    refused(L.VS_ERR_STATE, e)
    e.set_policy_population(None)
    served()
    e.set_policy_fnn(None, None)                                # no policy
    refused(L.VS_ERR_STATE, e)
    e.set_policy_linear(np.zeros(d["A"], dtype=np.float32), ["const"])
    refused(L.VS_ERR_STATE, e)
    n_gru = 3 * 8 * (d["O"] + 8 + 2) + (8 + 1) * d["A"]
    e.set_policy_rnn(np.zeros(n_gru, dtype=np.float32), cell="gru", n_layers=1, hidden_size=8)
    refused(L.VS_ERR_STATE, e)
    e.set_policy_playback(np.zeros((N, T, d["A"]), dtype=np.float32))
    refused(L.VS_ERR_STATE, e)
    n3 = (d["O"] + 1) * 8 + 2 * (8 + 1) * 8 + (8 + 1) * d["A"]
    e.set_policy_fnn(np.zeros(n3, dtype=np.float32), [8, 8, 8])  # three hidden layers
    refused(L.VS_ERR_STATE, e, n=n3)
    clc.set_net(e, c["net"])
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
    ab = torch.zeros(T, 1, disc.ld, device="cuda")
    assert lib.vs_fnn_param_grad(disc._h, T, ptr(ab), ptr(out), n_params, 0) == L.VS_ERR_STATE
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and "vs_fnn_param_grad" in lib.vs_last_error(disc._h).decode()
    disc.close()


# ------------------------------------------------------------------------------------------------------- 4. autograd
@pytest.mark.parametrize("name", ["qq-su", "qcp-su"])
def test_autograd_kernel_against_torch(vs, name, monkeypatch):
    from simurlacra_amd import diffsim

    tc = clc.torch_case("fnn", name)
    NT, TT = clc.NT, clc.TT
    env = getattr(vs, clc.ENVS[name])(max_steps=MAX_STEPS, **KW[name])
    policy = vs.FNNPolicy(env.spec, hidden_sizes=list(clc.FNN_AUTOGRAD[name]), hidden_nonlin=torch.tanh, featurize=False)
    policy.param_values = torch.as_tensor(clc.flat_params(tc["net"]))
    weights = list(policy.parameters())

    def grads(roll):
        init = dev(tc["init"]).requires_grad_(True)
        obs, rew, act, lengths = roll(init, TT)
        loss = -vs.discounted_return(rew, lengths, clc.GAMMA).sum() + 1e-3 * act.pow(2).sum()
        g = torch.autograd.grad(loss, weights + [init], retain_graph=True)
        return g, loss, init

    by_torch = vs.DifferentiableNetRollout(env, policy, batch_lanes=32, param_pass="torch")
    g_torch, _, _ = grads(by_torch)
    by_torch.close()
    # ---- through the kernel: the torch pass is not entered; what every batch's call saw is kept for the bound
    seen = []
    plain = vs.VecSimEnv.fnn_param_grad

    def spy(self, t_steps, abar, out=None, accumulate=False):
        obs, inside, _ = rows_of(self, self.n_envs, t_steps)
        seen.append((obs, inside, vs.lanes_first(abar, self.n_envs).cpu().numpy(), self.ld, bool(accumulate)))
        return plain(self, t_steps, abar, out=out, accumulate=accumulate)

    def no_torch_pass(*a, **k):
        raise AssertionError("the torch parameter pass was entered")

    monkeypatch.setattr(vs.VecSimEnv, "fnn_param_grad", spy)
    monkeypatch.setattr(diffsim._ClosedLoopRollout, "_param_grads", no_torch_pass)
    roll = vs.DifferentiableNetRollout(env, policy, batch_lanes=32)
    assert roll.param_pass == "kernel"
    g_kernel, loss, _ = grads(roll)
    assert [s[4] for s in seen] == [False, True, True] and [s[2].shape[0] for s in seen] == [32, 32, 6]  # three batches accumulate
    again = torch.autograd.grad(loss, weights, retain_graph=True)
    assert all(torch.equal(a, b) for a, b in zip(again, g_kernel[:-1]))                # backward() twice: the same bits
    assert torch.equal(g_kernel[-1], g_torch[-1]) and bool(g_kernel[-1].any())         # d init_states: the same sweep
    bound = 0.0
    for obs, inside, abar, ld, _ in seen[:3]:
        n_wg, acc = grid_of(ld, TT)
        bound = bound + host.param_grad_fp64(tc["net"], obs, abar.transpose(1, 0, 2).reshape(TT * abar.shape[0], -1), inside,
                                             chains=dict(acc=acc, wg=-(-n_wg // 4) + 2))[3]
    flat = lambda g: torch.cat([x.reshape(-1) for x in g[:-1]]).cpu().numpy().astype(np.float64)  # noqa: E731
    assert all(a.shape == w.shape for a, w in zip(g_kernel, weights))
    worst = worst_ratio(np.abs(flat(g_kernel) - flat(g_torch)), 2.0 * bound)
    print(f"{name}: kernel against torch parameter pass, worst difference / (2 bound) {worst:.3f}")
    assert np.abs(flat(g_torch)).max() > 0.0 and worst <= 1.0, (name, worst)
    roll.close()


def test_autograd_fp64_parameters_take_the_torch_pass(vs):
    name = "qq-su"
    tc = clc.torch_case("fnn", name)
    env = getattr(vs, clc.ENVS[name])(max_steps=MAX_STEPS, **KW[name])
    policy = vs.FNNPolicy(env.spec, hidden_sizes=list(clc.FNN_AUTOGRAD[name]), hidden_nonlin=torch.tanh, featurize=False)
    policy.param_values = torch.as_tensor(clc.flat_params(tc["net"]))
    policy.double()
    roll = vs.DifferentiableNetRollout(env, policy, batch_lanes=32)
    assert roll.param_pass == "torch"
    obs, rew, act, lengths = roll(dev(tc["init"]), clc.TT)
    g = torch.autograd.grad(-vs.discounted_return(rew, lengths, clc.GAMMA).sum() + 1e-3 * act.pow(2).sum(), list(policy.parameters()))
    assert all(x.dtype == torch.float64 and bool(torch.isfinite(x).all()) for x in g) and any(bool(x.any()) for x in g)
    with pytest.raises(vs.ValueErr, match="param_pass"):
        vs.DifferentiableNetRollout(env, policy, param_pass="triton")
    roll.close()
