"""
vs_lin_param_grad / k_lin_param_grad (+ k_fnn_param_reduce): the weight gradient of a linear policy on a feature stack over the recorded
rows of a handle, VecSimEnv.lin_param_grad and DifferentiablePolicyRollout(param_pass="kernel").

Shapes, stacks, weights and seeds are those of test_gpu_policy_vjp.py (closed_loop_cases.py; 150 lanes = 64 + 64 + 22, T = 24, +-5 % per-lane parameters,
lanes 0 .. 9 end early) plus the two stacks of lin_param_grad_fp64.EXTRA (all 128 features; a stack in a non-slot order).  abar is
dense, fed directly, and not zero-mean (lin_param_grad_fp64's docstring says why).

Reference: lin_param_grad_fp64.lin_param_grad_fp64 -- sum_rows abar (x) phi(x) in fp64 over the RECORDED observations and
lengths, with the NumPy feature stack of closed_loop_cases (held to torch.autograd.grad of the .double() LinearPolicy at 1e-12 by
test_lin_param_grad_host, without a device).  Tolerance, per parameter: lin_param_grad_fp64.error_bound, derived in its docstring,
    bound = sum_rows |abar| e(phi_q) + gamma(chain) sum_rows |abar phi_q|,
the chain read off the launch's grid rule (param_grad_cases.lin_grid_of / chain_of, mirrored from the documented rule with the
device's compute-unit count).  The kernel is held to the fp64 reference within the bound.  The bound is not tuned to the kernel: the
worst measured ratio per case is printed (-s) and recorded in DESIGN.md 8n.

The checks that the three parameter-gradient passes share are bodies in param_grad_cases.py; the tests here hand them this family.

Which assertion catches which kernel mistake:
  * a missing L select / mask          test_nan_behind_the_rows_changes_no_bit, and every table case (lanes 0 .. 9 end early)
  * a slot landing at the wrong index  test_wiring_of_a_single_row (a stack in a non-slot order, and all 128 slots)
  * a wrong obs_idx view               pend-view
  * a stale LDS row between tiles      test_runs_of_two_tiles (lengths change inside a run), test_small_batches
  * a nondeterministic reduction       test_two_calls_and_accumulate_are_exact, the autograd test's backward-twice assertion
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import closed_loop_cases as clc  # noqa: E402  (features, torch_case, the autograd shapes; a network for the policy-switch tests)
import lin_param_grad_fp64 as host  # noqa: E402  (cases, the fp64 reference and its error bound)
import param_grad_cases as pgc  # noqa: E402
from derivative_cases import ACT_IN, KW, MAX_STEPS, N, N_EDGE, T, dev, record_mode2  # noqa: E402
from param_grad_cases import LIN, n_cu, vs, worst_ratio  # noqa: E402,F401  (vs: the fixture)


def set_linear(e, c, noise_std=None):
    e.set_policy_linear(c["W"].reshape(-1), list(c["terms"]), obs_idx=c["obs_idx"], noise_std=noise_std)


def recorded(vs, key, noise_std=None, **kw):
    """param_grad_cases.recorded of the case under its linear policy"""
    c = host.case(key)
    return pgc.recorded(vs, c, lambda e: set_linear(e, c, noise_std), **kw)


def on_device(vs, e, key):
    return vs.lanes_last(dev(host.abar_of(key)), e.ld)


def reference(e, key, n, t, abar):
    """(fp64 gradient, bound) [A, F] for the handle's records and abar [n, t, A]"""
    c = host.case(key)
    obs, inside, _ = pgc.rows_of(e, n, t)
    want, _, bound = host.lin_param_grad_fp64(c["terms"], c["obs_idx"], obs, abar.transpose(1, 0, 2).reshape(t * n, -1), inside,
                                              chain=pgc.chain_of(e.ld, t, n_cu()))
    return want, bound


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
    n_wg, acc = pgc.lin_grid_of(e.ld, t, n_cu())
    if n_cu() == 256:
        assert e.ld == 1792 and (e.ld // 64) * t > n_wg and acc == 128 and t % 2 == 1
    held(vs, e, key, n, t, host.abar_of(key, n, t), f"{key} n={n} T={t}")
    e.close()


def test_zero_adjoints_give_zeros(vs):
    key = "qcp-su"
    e = recorded(vs, key)
    pgc.check_zero_adjoints_give_zeros(e, LIN, T, [host.case(key)["ref"].A])
    e.close()


# ------------------------------------------------------------------------------------------------------- 4. bit-exact
@pytest.mark.parametrize("key", ["qq-su", "qbb-full"])
def test_nan_behind_the_rows_changes_no_bit(vs, key):
    """NaN in abar at every row t >= L, at lanes n .. ld - 1 and in rows t_steps .. of a larger buffer: the same bits as with zeros there"""
    e = recorded(vs, key)
    pgc.check_nan_behind_the_rows(e, LIN, N, T, [on_device(vs, e, key)])
    e.close()


def test_two_calls_and_accumulate_are_exact(vs):
    key = "qbb-full"
    e = recorded(vs, key)
    ab = on_device(vs, e, key)
    pgc.check_two_calls_and_accumulate(vs, e, LIN, T, [ab], [ab[:, :, :64].contiguous()], dense=False)
    e.close()


def test_the_handle_is_untouched_and_goes_on_serving(vs):
    key = "qq-su"
    e = recorded(vs, key)
    cot = clc.cotangents(vs, key, e)
    pgc.check_the_handle_is_untouched(vs, e, LIN, T, lambda: e.rollout_vjp_policy(T, **cot))  # straight on the sweep's d_act
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
        record_mode2(e, long, params, lambda e: set_linear(e, lc), init, (t,))
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
    key = "qq-su"
    c = host.case(key)
    e = recorded(vs, key)
    r = pgc.Refusals(vs, e, LIN, T, [on_device(vs, e, key)])
    assert r.n_params == c["W"].size
    r.arguments()
    r.policies(vs.env_dims(c["name"]), c["W"], lambda: e.set_policy_linear(None, None),
               lambda: e.set_policy_linear(c["W"].reshape(-1), list(c["terms"])), dict(fnn={}, gru={}, playback={}))
    e.set_policy_linear(None, None)
    with pytest.raises(vs.ValueErr, match="set_policy_linear"):  # the Python face
        e.lin_param_grad(T, r.bufs[0])
    e.close()
    r.discrete_family()


# ------------------------------------------------------------------------------------------------------- 6. autograd
def autograd_policy(vs, name):
    tc = clc.torch_case("linear", name)
    env = getattr(vs, clc.ENVS[name])(max_steps=MAX_STEPS, **KW[name])
    policy = vs.LinearPolicy(env.spec, vs.FeatureStack(vs.identity_feat, vs.sin_feat, vs.const_feat, vs.MultFeat((0, 1))))
    with torch.no_grad():
        policy.net.weight.copy_(torch.as_tensor(tc["W"]))
    return tc, env, policy


@pytest.mark.parametrize("name", ["qq-su", "qcp-su"])
def test_autograd_kernel_against_torch(vs, name, monkeypatch):
    tc, env, policy = autograd_policy(vs, name)
    weight = policy.net.weight
    by_torch = vs.DifferentiablePolicyRollout(env, policy, batch_lanes=32, param_pass="torch")
    g_torch, _, out_torch = pgc.autograd_grads(vs, by_torch, tc, [weight])
    by_torch.close()
    # ---- through the kernel: no [N, T, .] copy is made
    roll = vs.DifferentiablePolicyRollout(env, policy, batch_lanes=32, param_pass="kernel")
    assert roll.param_pass == "kernel" and not roll._needs_rows
    init = dev(tc["init"]).requires_grad_(True)
    loss, out_kernel = pgc.autograd_loss(vs, roll, init)         # the forward pass reads the records; the backward pass must not
    assert all(torch.equal(a, b) for a, b in zip(out_kernel, out_torch))

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
    seen = []
    pgc.spy_on(vs, monkeypatch, LIN, seen)
    spied = torch.autograd.grad(loss, [weight], retain_graph=True)
    assert torch.equal(spied[0], g_kernel[0])
    pgc.check_three_batches_accumulate(seen)
    assert g_kernel[0].shape == weight.shape

    def bound_of(s):
        return host.lin_param_grad_fp64(clc.SMALL, None, s.obs, s.bufs[0], s.inside, chain=pgc.chain_of(s.ld, clc.TT, n_cu()))[2]

    pgc.check_kernel_against_torch_pass(name, seen, bound_of, pgc.flat_grads(g_kernel[:1]), pgc.flat_grads(g_torch[:1]), 2.0, "2 bound")
    roll.close()


def test_autograd_fp64_weights_take_the_torch_pass(vs):
    tc, env, policy = autograd_policy(vs, "qq-su")
    policy.double()
    roll = vs.DifferentiablePolicyRollout(env, policy, batch_lanes=32, param_pass="kernel")
    pgc.check_fp64_takes_the_torch_pass(vs, roll, tc, [policy.net.weight])
    roll.close()
