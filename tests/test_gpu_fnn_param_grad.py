"""
vs_fnn_param_grad / k_fnn_param_grad + k_fnn_param_reduce: the parameter gradient of a feed-forward network policy over the recorded
rows of a handle, VecSimEnv.fnn_param_grad and DifferentiableNetRollout(param_pass="kernel").

Shapes, networks and seeds are those of test_gpu_fnn_vjp.py (closed_loop_cases.py has the cases): 150 lanes (64 + 64 + 22), T = 24, +-5 % per-lane
parameters, lanes 0 .. 9 end early.  abar is random and dense and is fed directly.

Reference: fnn_param_grad_fp64.param_grad_fp64 -- the sum restated in fp64 over the RECORDED observations and lengths (held to
torch.autograd.grad of the .double() module at 1e-12 by test_fnn_param_grad_host, without a device).

Tolerance, per parameter p: the first-order bound of fnn_param_grad_fp64.error_bound (derived in its docstring),
    bound_p = sum_rows (|delta| e(y) + |y| e(delta)) + gamma(acc + 3 + wg + 1) sum_rows |term_p|,      gamma(m) = m 2^-24,
where e(.) carries tanh_fast's 2e-7, the sigmoid's 4e-7, sincos_fast's 4e-7 and the rounding of every fp32 chain the kernel runs
(12 / 19 / 8 operations per forward layer, A or 19 per pull-back) through the fp64 reference's own values, and the accumulation chain is
read off the launch: acc = the rows one wave sums in its registers (64 per tile of its run), 3 adds across the four waves, wg = the adds
of k_fnn_param_reduce across the workgroups (n_wg / 4 per partial sum, 2 to join them), 1 for accumulate.  The grid is mirrored from the
documented rule (param_grad_cases.fnn_grid_of).  The kernel is held to the fp64 reference within bound_p and to the fp32 torch pass of the same rows within
twice it.  The bound is not tuned to the measurement; the worst measured ratio per case is printed (-s) and recorded in DESIGN.md 8h.

The checks that the three parameter-gradient passes share are bodies in param_grad_cases.py; the tests here hand them this family.

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
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import closed_loop_cases as clc  # noqa: E402  (cases, networks, seeds)
import fnn_param_grad_fp64 as host  # noqa: E402  (the fp64 reference and its error bound)
import param_grad_cases as pgc  # noqa: E402
from derivative_cases import ACT_IN, KW, MAX_STEPS, N, N_EDGE, T, dev  # noqa: E402
from fnn_param_grad_fp64 import abar_of  # noqa: E402
from param_grad_cases import FNN, vs, worst_ratio  # noqa: E402,F401  (vs: the fixture)

TABLE = host.GPU_TABLE


def grid_of(ld, t_steps):
    return pgc.fnn_grid_of(ld, t_steps, pgc.n_cu())


def recorded(vs, key, spec=None, **kw):
    """param_grad_cases.recorded of the case under its network, or under what fnn_kernel_spec made of a torch policy"""
    c = clc.case(key)
    return pgc.recorded(vs, c, (lambda e: clc.set_net(e, c["net"])) if spec is None else (lambda e: e.set_policy_fnn(**spec)), **kw)


def on_device(vs, e, key, t=T):
    return vs.lanes_last(dev(abar_of(key, N, t)), e.ld)


def reference(e, net, n, t, abar):
    """(fp64 gradient, bound, hidden pre-activations, lengths, obs rows, inside) for the handle's records"""
    obs, inside, length = pgc.rows_of(e, n, t)
    want, _, pre, bound = host.param_grad_fp64(net, obs, abar.transpose(1, 0, 2).reshape(t * n, -1), inside,
                                               chains=pgc.chains_of(grid_of(e.ld, t)))
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
    assert np.array_equal(f.fnn_param_grad(17, on_device(vs, f, key, 17)).cpu().numpy().astype(np.float64), short)
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
    pgc.check_zero_adjoints_give_zeros(e, FNN, T, [clc.case(key)["ref"].A])
    e.close()


@pytest.mark.parametrize("key", ["qq-su-64x64-feat", "omo-1-relu"])
def test_nan_behind_the_rows_changes_no_bit(vs, key):
    """NaN in abar at every row t >= L, at lanes n .. ld - 1 and in rows t_steps .. of a larger buffer: the same bits as with zeros there"""
    e = recorded(vs, key)
    pgc.check_nan_behind_the_rows(e, FNN, N, T, [on_device(vs, e, key)])
    e.close()


def test_two_calls_and_accumulate_are_exact(vs):
    key = "qbb-31x64-tanh-out"
    e = recorded(vs, key)
    ab = on_device(vs, e, key)
    pgc.check_two_calls_and_accumulate(vs, e, FNN, T, [ab], [ab[:, :, :64].contiguous()], dense=True)
    e.close()


def test_the_handle_is_untouched_and_goes_on_serving(vs):
    key = "qq-su-64x64-feat"
    e = recorded(vs, key)
    cot = clc.cotangents(vs, key, e)
    da0, _ = e.rollout_vjp_fnn(T, **cot)
    g = pgc.check_the_handle_is_untouched(vs, e, FNN, T, lambda: e.rollout_vjp_fnn(T, **cot))  # straight on the sweep's d_act
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
    key = "qq-su-16"
    c = clc.case(key)
    d = vs.env_dims(c["name"])
    e = recorded(vs, key)
    r = pgc.Refusals(vs, e, FNN, T, [on_device(vs, e, key)])
    r.arguments()
    n3 = (d["O"] + 1) * 8 + 2 * (8 + 1) * 8 + (8 + 1) * d["A"]  # three hidden layers: refused whatever n_params says
    r.policies(d, clc.flat_params(c["net"]), lambda: e.set_policy_fnn(None, None), lambda: clc.set_net(e, c["net"]),
               dict(linear={}, gru={}, playback={}, fnn3=dict(n=n3)))
    e.close()
    r.discrete_family()


# ------------------------------------------------------------------------------------------------------- 4. autograd
def autograd_policy(vs, name):
    tc = clc.torch_case("fnn", name)
    env = getattr(vs, clc.ENVS[name])(max_steps=MAX_STEPS, **KW[name])
    policy = vs.FNNPolicy(env.spec, hidden_sizes=list(clc.FNN_AUTOGRAD[name]), hidden_nonlin=torch.tanh, featurize=False)
    policy.param_values = torch.as_tensor(clc.flat_params(tc["net"]))
    return tc, env, policy


@pytest.mark.parametrize("name", ["qq-su", "qcp-su"])
def test_autograd_kernel_against_torch(vs, name, monkeypatch):
    from simurlacra_amd import diffsim

    tc, env, policy = autograd_policy(vs, name)
    weights = list(policy.parameters())
    by_torch = vs.DifferentiableNetRollout(env, policy, batch_lanes=32, param_pass="torch")
    g_torch = pgc.autograd_grads(vs, by_torch, tc, weights)[0]
    by_torch.close()
    # ---- through the kernel: the torch pass is not entered; what every batch's call saw is kept for the bound
    seen = []

    def no_torch_pass(*a, **k):
        raise AssertionError("the torch parameter pass was entered")

    pgc.spy_on(vs, monkeypatch, FNN, seen)
    monkeypatch.setattr(diffsim._ClosedLoopRollout, "_param_grads", no_torch_pass)
    roll = vs.DifferentiableNetRollout(env, policy, batch_lanes=32)
    assert roll.param_pass == "kernel"
    g_kernel, loss, _ = pgc.autograd_grads(vs, roll, tc, weights)
    pgc.check_three_batches_accumulate(seen)
    pgc.check_backward_twice_and_the_sweep(loss, weights, g_kernel, g_torch)

    def bound_of(s):
        return host.param_grad_fp64(tc["net"], s.obs, s.bufs[0], s.inside, chains=pgc.chains_of(grid_of(s.ld, clc.TT)))[3]

    pgc.check_kernel_against_torch_pass(name, seen, bound_of, pgc.flat_grads(g_kernel[:-1]), pgc.flat_grads(g_torch[:-1]), 2.0, "2 bound")
    roll.close()


def test_autograd_fp64_parameters_take_the_torch_pass(vs):
    tc, env, policy = autograd_policy(vs, "qq-su")
    policy.double()
    roll = vs.DifferentiableNetRollout(env, policy, batch_lanes=32)
    pgc.check_fp64_takes_the_torch_pass(vs, roll, tc, list(policy.parameters()))
    with pytest.raises(vs.ValueErr, match="param_pass"):
        vs.DifferentiableNetRollout(env, policy, param_pass="triton")
    roll.close()
