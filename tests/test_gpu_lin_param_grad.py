"""
vs_lin_param_grad / k_lin_param_grad (+ k_fnn_param_reduce): the weight gradient of a linear policy on a feature stack over the recorded
rows of a handle, VecSimEnv.lin_param_grad and DifferentiablePolicyRollout(param_pass="kernel").

Shapes, stacks, weights and seeds are those of test_gpu_policy_vjp.py (closed_loop_cases.py; 150 lanes = 64 + 64 + 22, T = 24, +-5 % per-lane parameters,
lanes 0 .. 9 end early) plus the two stacks of test_lin_param_grad_host.EXTRA (all 128 features; a stack in a non-slot order).  abar is
dense, fed directly, and not zero-mean (test_lin_param_grad_host's docstring says why).

Reference: test_lin_param_grad_host.lin_param_grad_fp64 -- sum_rows abar (x) phi(x) in fp64 over the RECORDED observations and
lengths, with the NumPy feature stack of closed_loop_cases (held to torch.autograd.grad of the .double() LinearPolicy at 1e-12 in
that file, without a device).  Tolerance, per parameter: test_lin_param_grad_host.error_bound, derived in its docstring,
    bound = sum_rows |abar| e(phi_q) + gamma(chain) sum_rows |abar phi_q|,
the chain read off the launch's grid rule (grid_of / chain_of there, mirrored from the documented rule with the device's compute-unit
count).  The kernel is held to the fp64 reference within the bound.  The bound is not tuned to the kernel: the worst measured ratio
per case is printed (-s) and recorded in DESIGN.md 8n.

Which assertion catches which kernel mistake:
  * a missing L select / mask          test_nan_behind_the_rows_changes_no_bit, and every table case (lanes 0 .. 9 end early)
  * a slot landing at the wrong index  test_wiring_of_a_single_row (a stack in a non-slot order, and all 128 slots)
  * a wrong obs_idx view               pend-view
  * a stale LDS row between tiles      test_runs_of_two_tiles (lengths change inside a run), test_small_batches
  * a nondeterministic reduction       test_two_calls_and_accumulate_are_exact, the autograd test's backward-twice assertion
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import closed_loop_cases as clc  # noqa: E402  (features, torch_case, the autograd shapes; a network for the policy-switch tests)
import test_lin_param_grad_host as host  # noqa: E402  (cases, the fp64 reference and its error bound)
from derivative_cases import ACT_IN, KW, MAX_STEPS, N, N_EDGE, STATE_BUFFERS, T, dev, record_mode2  # noqa: E402


@pytest.fixture(scope="module")
def vs():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import simurlacra_amd

    return simurlacra_amd


def n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def recorded(vs, key, n=N, t=T, lanes=None, noise_std=None, noise_seed=0, cap=None):
    """a handle whose rows 0 .. t - 1 hold the closed-loop rollouts of the case (lane k repeats lane k % N, or the case's `lanes`)"""
    c = host.case(key)
    name = c["name"]
    pick = (lambda x: np.resize(x, (n,) + x.shape[1:])) if lanes is None else (lambda x: np.resize(x[lanes], (n,) + x.shape[1:]))
    e = vs.VecSimEnv(name, n, max_steps=MAX_STEPS, **KW[name])

    def linear(e):
        e.set_policy_linear(c["W"].reshape(-1), list(c["terms"]), obs_idx=c["obs_idx"], noise_std=noise_std)

    return record_mode2(e, t if cap is None else cap, pick(c["params"]), linear, pick(c["init"]), (t,), noise_seed=noise_seed)


def rows_of(e, n, t):
    """(obs [t n, O], inside [t n], lengths [n]) of the handle's records, step-major"""
    obs = e.traj_tensors(t, n)["obs"].cpu().numpy()  # [t, n, O]
    length = e.rollout_lengths(n, t)[0].cpu().numpy()
    inside = np.arange(t)[:, None] < length[None, :]
    return obs.reshape(t * n, -1), inside.reshape(-1), length


def reference(e, key, n, t, abar, more_adds=0):
    """(fp64 gradient, bound) [A, F] for the handle's records and abar [n, t, A]"""
    c = host.case(key)
    obs, inside, _ = rows_of(e, n, t)
    want, _, bound = host.lin_param_grad_fp64(c["terms"], c["obs_idx"], obs, abar.transpose(1, 0, 2).reshape(t * n, -1), inside,
                                              chain=host.chain_of(e.ld, t, n_cu(), more_adds))
    return want, bound


def worst_ratio(err, bound):
    """max err / bound; an entry whose bound is 0 (every term of it is 0) must be met exactly"""
    return float(np.where(bound > 0.0, err / np.where(bound > 0.0, bound, 1.0), np.where(err == 0.0, 0.0, np.inf)).max())


def held(vs, e, key, n, t, abar, what):
    want, bound = reference(e, key, n, t, abar)
    got = e.lin_param_grad(t, vs.lanes_last(dev(abar), e.ld))
    assert got.dtype == torch.float32 and tuple(got.shape) == (want.size,) and got.is_cuda
    got = got.cpu().numpy().astype(np.float64).reshape(want.shape)
    assert np.isfinite(got).all() and e.error_count() == 0
    r = worst_ratio(np.abs(got - want), bound)
    print(f"{what}: worst |kernel - fp64| / bound {r:.3f}, bound / max |g| {float((bound / np.abs(want).max()).max()):.1e}")
    assert np.abs(want).max() > 0.0 and r <= 1.0, (what, r)
    return got


# ------------------------------------------------------------------------------------------------------- 1. the table
@pytest.mark.parametrize("key", host.TABLE)
def test_against_the_fp64_reference(vs, key):
    """Worst |kernel - fp64| / bound measured on the MI355X (printed with -s): DESIGN.md section 8n."""
    e = recorded(vs, key)
    held(vs, e, key, N, T, host.abar_of(key), key)
    length = e.rollout_lengths(N, T)[0].cpu().numpy()
    assert (length[:N_EDGE] < T).any() and (length[N_EDGE:] == T).mean() > 0.9  # lanes that end early, lanes that run through
    e.close()


def test_exploration_noise(vs):
    """the policy inside a NormalActNoiseExplStrat: the records hold the noisy rollout, the gradient is the mean policy's"""
    key = "pend-view"
    c = host.case(key)
    e = recorded(vs, key, noise_std=np.full(c["ref"].A, 0.02 * ACT_IN[c["name"]]), noise_seed=77)
    quiet = recorded(vs, key)
    assert not torch.equal(e.traj_tensors(T, N)["act"], quiet.traj_tensors(T, N)["act"])  # the noise is there
    quiet.close()
    held(vs, e, key, N, T, host.abar_of(key), key + " + noise")
    e.close()


# ------------------------------------------------------------------------------------------------------- 2. the wiring
@pytest.mark.parametrize("key", ["qq-su-shuffled", "qbb-full", "pend-view"])
def test_wiring_of_a_single_row(vs, key):
    """n = 1, T = 1, abar = 1: d_params of action row j IS phi(obs_0), in the stack's order whatever the kernel's slot order"""
    c = host.case(key)
    e = recorded(vs, key, n=1, t=1)
    A = c["ref"].A
    got = e.lin_param_grad(1, torch.ones(1, A, e.ld, device="cuda")).cpu().numpy().astype(np.float64).reshape(A, -1)
    obs = e.traj_tensors(1, 1)["obs"].cpu().numpy().astype(np.float64).reshape(1, -1)
    x = obs if c["obs_idx"] is None else obs[:, list(c["obs_idx"])]
    phi, err = clc.features(c["terms"], x)[0], host.feature_errors(c["terms"], x)[0]
    assert got.shape == (A, phi.size) and np.unique(np.round(phi, 6)).size >= min(phi.size, 4) - 1  # (the entries can be told apart)
    for j in range(A):
        assert (np.abs(got[j] - phi) <= err + 4.0 * host.U * np.abs(phi)).all(), (key, j, np.abs(got[j] - phi).max())
    e.close()


# ------------------------------------------------------------------------------------------------------- 3. edges
@pytest.mark.parametrize("n,t", [(1, T), (65, T), (N, 1)])
def test_small_batches(vs, n, t):
    key = "qq-su"
    e = recorded(vs, key, n=n, t=t)
    held(vs, e, key, n, t, host.abar_of(key, n, t), f"{key} n={n} T={t}")
    e.close()


def test_t_steps_below_the_capacity(vs):
    key = "qbb"
    e = recorded(vs, key)
    ab = host.abar_of(key, N, 17)
    short = held(vs, e, key, N, 17, ab, key + " 17 of 24 rows")
    f = recorded(vs, key, t=17)
    assert np.array_equal(f.lin_param_grad(17, vs.lanes_last(dev(ab), f.ld)).cpu().numpy().astype(np.float64).reshape(short.shape), short)
    f.close()
    e.close()


def test_every_rollout_runs_to_the_end(vs):
    key = "qcp-su"
    lanes = np.arange(N_EDGE, N)
    e = recorded(vs, key, lanes=lanes)
    full = np.flatnonzero(e.rollout_lengths(N, T)[0].cpu().numpy() == T)
    e.close()
    lanes = lanes[full % lanes.size]  # the case's lanes that run through
    e = recorded(vs, key, lanes=lanes)
    held(vs, e, key, N, T, host.abar_of(key), key + " all lanes full")
    assert (e.rollout_lengths(N, T)[0].cpu().numpy() == T).all()
    e.close()


def test_runs_of_two_tiles(vs):
    """The grid is one wave per tile up to 4 x 256 = 1024 wave slots, and ld is the lane count rounded up to 256, i.e. a multiple of four
    lane groups.  With T = 41 (odd, so that runs of two tiles do not line up with the lane groups) 24 lane groups are 984 tiles -- a wave
    each, the tile loop does not iterate -- and 28 are 1148: runs of two.  The smallest batch with 28 lane groups is 1537 lanes
    (ld = 1792): every other group boundary falls INSIDE a run (tiles 40 | 41: the wave re-derives the lanes' lengths in mid-run),
    lane group 24 holds one lane and groups 25 .. 27 none."""
    key, n, t = "qbb", 1537, 41
    e = recorded(vs, key, n=n, t=t)
    n_wg, acc = host.grid_of(e.ld, t, n_cu())
    if n_cu() == 256:
        assert e.ld == 1792 and (e.ld // 64) * t > n_wg and acc == 128 and t % 2 == 1
    held(vs, e, key, n, t, host.abar_of(key, n, t), f"{key} n={n} T={t}")
    e.close()


def test_zero_adjoints_give_zeros(vs):
    key = "qcp-su"
    e = recorded(vs, key)
    out = torch.full((e._lin_n_params,), 7.0, device="cuda")
    assert e.lin_param_grad(T, torch.zeros(T, host.case(key)["ref"].A, e.ld, device="cuda"), out=out) is out
    assert not out.any()
    e.close()


# ------------------------------------------------------------------------------------------------------- 4. bit-exact
@pytest.mark.parametrize("key", ["qq-su", "qbb-full"])
def test_nan_behind_the_rows_changes_no_bit(vs, key):
    """NaN in abar at every row t >= L, at lanes n .. ld - 1 and in rows t_steps .. of a larger buffer: the same bits as with zeros there"""
    e = recorded(vs, key)
    A = host.case(key)["ref"].A
    length = e.rollout_lengths(N, T)[0]
    assert e.ld > N and bool((length < T).any())
    big = torch.zeros(T + 5, A, e.ld, device="cuda")
    big[:T, :, :N] = vs.lanes_last(dev(host.abar_of(key)), e.ld)[:, :, :N]
    behind = torch.arange(T, device="cuda")[:, None] >= length[None, :]          # [T, N]
    big[:T, :, :N] = torch.where(behind[:, None, :], torch.zeros((), device="cuda"), big[:T, :, :N])
    clean = e.lin_param_grad(T, big[:T])
    dirty = big.clone()
    dirty[:T, :, :N] = torch.where(behind[:, None, :], torch.full((), float("nan"), device="cuda"), dirty[:T, :, :N])
    dirty[:, :, N:] = float("nan")
    dirty[T:] = float("nan")
    assert bool(torch.isnan(dirty[:T, :, :N]).any())
    got = e.lin_param_grad(T, dirty[:T])
    assert bool(clean.any()) and bool(torch.isfinite(got).all()) and torch.equal(got, clean)
    e.close()


def test_two_calls_and_accumulate_are_exact(vs):
    key = "qbb-full"
    e = recorded(vs, key)
    ab = vs.lanes_last(dev(host.abar_of(key)), e.ld)
    g = e.lin_param_grad(T, ab)
    assert torch.equal(e.lin_param_grad(T, ab), g) and bool(g.any())
    twice = e.lin_param_grad(T, ab)
    e.lin_param_grad(T, ab, out=twice, accumulate=True)
    assert torch.equal(twice, 2.0 * g)
    r = torch.randn(g.shape, device="cuda", generator=torch.Generator("cuda").manual_seed(3))
    out = r.clone()
    e.lin_param_grad(T, ab, out=out, accumulate=True)
    assert torch.equal(out, r + g)
    with pytest.raises(vs.ValueErr):
        e.lin_param_grad(T, ab, accumulate=True)
    with pytest.raises(vs.ShapeErr):
        e.lin_param_grad(T, ab[:, :, :64].contiguous())
    e.close()


def test_the_handle_is_untouched_and_goes_on_serving(vs):
    L = vs._lib
    key = "qq-su"
    e = recorded(vs, key)
    cot = clc.cotangents(vs, key, e)
    da0, di0 = e.rollout_vjp_policy(T, **cot)
    before = [e.get(getattr(L, b)).copy() for b in STATE_BUFFERS]
    planes, words = e.traj_planes()
    rows = [p.clone() for p, _ in planes] + [words.clone()]
    g = e.lin_param_grad(T, da0)  # straight on the sweep's d_act
    assert bool(torch.isfinite(g).all()) and bool(g.any())
    for b, x in zip(STATE_BUFFERS, before):
        assert np.array_equal(e.get(getattr(L, b)), x), b
    planes, words = e.traj_planes()
    assert all(torch.equal(a, b) for a, b in zip([p for p, _ in planes] + [words], rows)) and e.error_count() == 0
    da1, di1 = e.rollout_vjp_policy(T, **cot)
    assert torch.equal(da1, da0) and torch.equal(di1, di0)
    e.close()


def test_one_workspace_serves_linear_fnn_linear_in_turn(vs):
    """The workspace of the parameter-gradient pass belongs to the handle's policy slot, whichever kind is in it.  ONE pendulum handle of
    65 lanes runs the pend-view linear policy (T = 3: 12 tiles, a partial vector of 128 floats), the [8] tanh network (T = 40: another
    grid, another packed size and map; rows 3 .. 39 of the first step were stale), the linear policy again (T = 40: the linear grid of
    160 workgroups in a buffer sized for the network's 40), and each result equals BIT FOR BIT that of the same call on a fresh handle."""
    n, long = 65, 40
    fc, lc = clc.case("pend-8"), host.case("pend-view")
    params, init, A = fc["params"][:n], fc["init"][:n], fc["ref"].A

    def dense(e, t, seed):
        return torch.randn(t, A, e.ld, device="cuda", generator=torch.Generator("cuda").manual_seed(seed))

    def linear(e, t, seed):
        record_mode2(e, long, params, lambda e: e.set_policy_linear(lc["W"].reshape(-1), list(lc["terms"]), obs_idx=lc["obs_idx"]), init, (t,))
        return e.lin_param_grad(t, dense(e, t, seed))

    def network(e, t, seed):
        record_mode2(e, long, params, lambda e: clc.set_net(e, fc["net"]), init, (t,))
        return e.fnn_param_grad(t, dense(e, t, seed))

    steps = ((linear, 3, 4), (network, long, 5), (linear, long, 6))
    e = vs.VecSimEnv("pend", n, max_steps=MAX_STEPS, **KW["pend"])
    got = [f(e, t, seed).clone() for f, t, seed in steps]
    assert e.error_count() == 0
    e.close()
    for k, (f, t, seed) in enumerate(steps):
        fresh = vs.VecSimEnv("pend", n, max_steps=MAX_STEPS, **KW["pend"])
        want = f(fresh, t, seed)
        assert bool(torch.isfinite(want).all()) and bool(want.any()) and torch.equal(got[k], want), k
        fresh.close()
    assert got[0].shape == got[2].shape != got[1].shape and not torch.equal(got[0], got[2])


# ------------------------------------------------------------------------------------------------------- 5. refusals
def test_refusals_leave_the_output_untouched(vs):
    L = vs._lib
    lib = L.load()
    key = "qq-su"
    c = host.case(key)
    d = vs.env_dims(c["name"])
    e = recorded(vs, key)
    n_params = e._lin_n_params
    assert n_params == c["W"].size
    abar = vs.lanes_last(dev(host.abar_of(key)), e.ld)
    out = torch.full((n_params + 1,), 7.0, device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731

    def call(handle, t_steps=T, ab=abar, dp=out, n=None):
        rc = lib.vs_lin_param_grad(handle._h if handle is not None else None, t_steps, ptr(ab), ptr(dp), n_params if n is None else n, 0)
        torch.cuda.synchronize()
        return rc

    def refused(code, handle, **kw):
        assert call(handle, **kw) == code
        assert bool((out == 7.0).all())  # the sentinels
        if handle is not None:
            assert "vs_lin_param_grad" in lib.vs_last_error(handle._h).decode()

    def served():
        assert call(e) == L.VS_OK and not bool((out[:n_params] == 7.0).any()) and float(out[n_params]) == 7.0
        out.fill_(7.0)

    def linear():
        e.set_policy_linear(c["W"].reshape(-1), list(c["terms"]))

    refused(L.VS_ERR_ARG, None)
    refused(L.VS_ERR_ARG, e, ab=None)
    refused(L.VS_ERR_ARG, e, dp=None)
    for t_steps in (0, -3, T + 1):
        refused(L.VS_ERR_ARG, e, t_steps=t_steps)
    for n in (n_params - 1, n_params + 1):
        refused(L.VS_ERR_ARG, e, n=n)
    e.set_traj_offset(3)
    refused(L.VS_ERR_STATE, e)
    e.set_traj_offset(0)
    e.set_auto_reset(True)
    refused(L.VS_ERR_STATE, e)
    e.set_auto_reset(False)
    e.set_policy_population(np.tile(c["W"].reshape(1, -1), (3, 1)), lane_set=np.arange(N) // 64)
    refused(L.VS_ERR_STATE, e)
    e.set_policy_population(None)
    served()
    e.set_policy_linear(None, None)                             # no policy
    refused(L.VS_ERR_STATE, e)
    with pytest.raises(vs.ValueErr, match="set_policy_linear"):  # the Python face
        e.lin_param_grad(T, abar)
    n_fnn = (d["O"] + 1) * 8 + (8 + 1) * d["A"]
    e.set_policy_fnn(np.zeros(n_fnn, dtype=np.float32), [8])    # an FNN policy
    refused(L.VS_ERR_STATE, e)
    n_gru = 3 * 8 * (d["O"] + 8 + 2) + (8 + 1) * d["A"]
    e.set_policy_rnn(np.zeros(n_gru, dtype=np.float32), cell="gru", n_layers=1, hidden_size=8)
    refused(L.VS_ERR_STATE, e)
    e.set_policy_playback(np.zeros((N, T, d["A"]), dtype=np.float32))
    refused(L.VS_ERR_STATE, e)
    linear()
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
    assert lib.vs_lin_param_grad(disc._h, T, ptr(ab), ptr(out), n_params, 0) == L.VS_ERR_STATE
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and "vs_lin_param_grad" in lib.vs_last_error(disc._h).decode()
    disc.close()


# ------------------------------------------------------------------------------------------------------- 6. autograd
@pytest.mark.parametrize("name", ["qq-su", "qcp-su"])
def test_autograd_kernel_against_torch(vs, name, monkeypatch):
    tc = clc.torch_case("linear", name)
    NT, TT = clc.NT, clc.TT
    env = getattr(vs, clc.ENVS[name])(max_steps=MAX_STEPS, **KW[name])
    policy = vs.LinearPolicy(env.spec, vs.FeatureStack(vs.identity_feat, vs.sin_feat, vs.const_feat, vs.MultFeat((0, 1))))
    with torch.no_grad():
        policy.net.weight.copy_(torch.as_tensor(tc["W"]))
    weight = policy.net.weight

    def grads(roll):
        init = dev(tc["init"]).requires_grad_(True)
        obs, rew, act, lengths = roll(init, TT)
        loss = -vs.discounted_return(rew, lengths, clc.GAMMA).sum() + 1e-3 * act.pow(2).sum()
        return torch.autograd.grad(loss, [weight, init], retain_graph=True), loss, (obs, rew, act)

    by_torch = vs.DifferentiablePolicyRollout(env, policy, batch_lanes=32, param_pass="torch")
    g_torch, _, out_torch = grads(by_torch)
    by_torch.close()
    # ---- through the kernel: no [N, T, .] copy is made; what every batch's call saw is kept for the bound
    seen = []
    plain = vs.VecSimEnv.lin_param_grad

    def spy(self, t_steps, abar, out=None, accumulate=False):
        obs, inside, _ = rows_of(self, self.n_envs, t_steps)
        seen.append((obs, inside, vs.lanes_first(abar, self.n_envs).cpu().numpy(), self.ld, bool(accumulate)))
        return plain(self, t_steps, abar, out=out, accumulate=accumulate)

    roll = vs.DifferentiablePolicyRollout(env, policy, batch_lanes=32, param_pass="kernel")
    assert roll.param_pass == "kernel" and not roll._needs_rows
    init = dev(tc["init"]).requires_grad_(True)
    obs, rew, act, lengths = roll(init, TT)                      # the forward pass reads the records; the backward pass must not
    loss = -vs.discounted_return(rew, lengths, clc.GAMMA).sum() + 1e-3 * act.pow(2).sum()
    assert all(torch.equal(a, b) for a, b in zip((obs, rew, act), out_torch))

    def no_rows(*a, **k):
        raise AssertionError("traj_tensors was called in backward")

    real_tt = vs.VecSimEnv.traj_tensors
    monkeypatch.setattr(vs.VecSimEnv, "traj_tensors", no_rows)
    g_kernel = torch.autograd.grad(loss, [weight, init], retain_graph=True)
    again = torch.autograd.grad(loss, [weight], retain_graph=True)
    monkeypatch.setattr(vs.VecSimEnv, "traj_tensors", real_tt)
    assert torch.equal(again[0], g_kernel[0])                                          # backward() twice: the same bits
    assert torch.equal(g_kernel[1], g_torch[1]) and bool(g_kernel[1].any())            # d init_states: the same sweep
    # ---- once more with the spy, for the rows and adjoints of every batch
    monkeypatch.setattr(vs.VecSimEnv, "lin_param_grad", spy)
    spied = torch.autograd.grad(loss, [weight], retain_graph=True)
    assert torch.equal(spied[0], g_kernel[0])
    assert [s[4] for s in seen] == [False, True, True] and [s[2].shape[0] for s in seen] == [32, 32, 6]  # three batches accumulate
    bound = 0.0
    for ob, inside, abar, ld, _ in seen:
        bound = bound + host.lin_param_grad_fp64(clc.SMALL, None, ob, abar.transpose(1, 0, 2).reshape(TT * abar.shape[0], -1), inside,
                                                 chain=host.chain_of(ld, TT, n_cu()))[2]
    assert g_kernel[0].shape == weight.shape
    flat = lambda g: g.detach().cpu().numpy().astype(np.float64)  # noqa: E731
    worst = worst_ratio(np.abs(flat(g_kernel[0]) - flat(g_torch[0])), 2.0 * bound)
    print(f"{name}: kernel against torch parameter pass, worst difference / (2 bound) {worst:.3f}")
    assert np.abs(flat(g_torch[0])).max() > 0.0 and worst <= 1.0, (name, worst)
    roll.close()


def test_autograd_fp64_weights_take_the_torch_pass(vs):
    name = "qq-su"
    tc = clc.torch_case("linear", name)
    env = getattr(vs, clc.ENVS[name])(max_steps=MAX_STEPS, **KW[name])
    policy = vs.LinearPolicy(env.spec, vs.FeatureStack(vs.identity_feat, vs.sin_feat, vs.const_feat, vs.MultFeat((0, 1))))
    with torch.no_grad():
        policy.net.weight.copy_(torch.as_tensor(tc["W"]))
    policy.double()
    roll = vs.DifferentiablePolicyRollout(env, policy, batch_lanes=32, param_pass="kernel")
    assert roll.param_pass == "torch"
    obs, rew, act, lengths = roll(dev(tc["init"]), clc.TT)
    g, = torch.autograd.grad(-vs.discounted_return(rew, lengths, clc.GAMMA).sum() + 1e-3 * act.pow(2).sum(), [policy.net.weight])
    assert g.dtype == torch.float64 and bool(torch.isfinite(g).all()) and bool(g.any())
    roll.close()
