"""
vs_rnn_param_grad / k_rnn_param_grad (+ k_fnn_param_reduce): the parameter gradient of a recurrent policy over the recorded rows of a
handle, VecSimEnv.rnn_param_grad and DifferentiableRecurrentRollout(param_pass="kernel").

Shapes: 70 lanes (ld = 128: one full lane group and one of six lanes), T = 12.  The policies are closed_loop_cases.make_rnn's; the records
come from a recording step_policy launch, abar and d_hid from vs_rollout_vjp_rnn under random cotangents (g_act and g_hid_last
included).  Lanes 0 .. 9 start at the edge of the state space and so do lanes 64 .. 69 -- the whole second lane group --, so that some
rollouts of the first group and, where the family's edge is close enough, all of the second end before T.

The cotangents are those of a MEAN over the N T rows: standard normal / (N T).  With unit cotangents the gradients are sums of 840 terms of
size 1 and reach several hundred, and the absolute floor of the condition `bound <= 1e-3 sum |term| + 1e-4` (checked for every case
before the kernel is looked at) means nothing at that size: parameters whose terms nearly cancel in a unit of two layers of 64 (a GRU's
W_hn h + b_hn near 0, whose error is gamma(131) of 64 products) then exceed it by their rounding alone.  As a mean the gradients are of
size 0.1 .. 1 and the floor is 1e-4 .. 1e-3 of the largest entry, of the size of the relative term.

Reference: rnn_param_grad_fp64.param_grad_fp64 on the RECORDED observations, hidden states and lengths; tolerance: twice its bound
(derived in that module's docstring), the chains read off the launch by param_grad_cases.rnn_grid_of.  The worst measured ratio per
case is printed (-s).  The cases (CASES, ELMAN_AS_FNN, case) and the checks that the three parameter-gradient passes share are in
param_grad_cases.py; the tests here hand them this family.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import closed_loop_cases as clc  # noqa: E402  (flat_params, set_rnn, the autograd cases; the [8] tanh network of the pendulum)
import fnn_param_grad_fp64 as fnn_host  # noqa: E402  (the FNN pass's fp64 reference and bound)
import param_grad_cases as pgc  # noqa: E402
import rnn_param_grad_fp64 as ref64  # noqa: E402
from derivative_cases import ACT_IN, KW, MAX_STEPS, dev, record_mode2  # noqa: E402
from param_grad_cases import CASES, ELMAN_AS_FNN, RNN, case, vs, worst_ratio  # noqa: E402,F401  (vs: the fixture)

N, T = pgc.RNN_N, pgc.RNN_T


def recorded(vs, key, t=T, cap=T):
    c = case(key)
    std = [0.02 * ACT_IN[c["name"]]] * c["ref"].A if c["noisy"] else None
    return pgc.recorded(vs, c, lambda e: clc.set_rnn(e, c["net"], std), n=N, t=t, cap=cap, noise_seed=91)


def sweep(vs, key, e, t=T):
    """(abar [t, A, ld], d_hid [t, Hs, ld]) of vs_rollout_vjp_rnn under the case's cotangents"""
    c = case(key)
    ll = lambda x: vs.lanes_last(dev(x), e.ld)  # noqa: E731
    da, _, dh, _ = e.rollout_vjp_rnn(t, g_rew=ll(c["g_rew"][:, :t]), g_obs=ll(c["g_obs"][:, :t + 1]), g_act=ll(c["g_act"][:, :t]),
                                     g_state_last=ll(c["g_last"]), g_hid_last=ll(c["g_hid"]))
    return da, dh


def rows_of(vs, key, e, t, abar, d_hid):
    """the handle's records and the two cotangents as step-major rows, and the lengths"""
    obs, inside, length = pgc.rows_of(e, N, t, case(key)["net"]["obs_idx"])
    return obs, pgc.hidden_rows(vs, e, N, t), pgc.device_rows(vs, abar, N), pgc.device_rows(vs, d_hid, N), inside, length


def reference(vs, key, e, t, abar, d_hid):
    c = case(key)
    x, p, ab, dh, inside, length = rows_of(vs, key, e, t, abar, d_hid)
    ab, dh = np.where(inside[:, None], ab, 0.0), np.where(inside[:, None], dh, 0.0)  # (the caller may have put NaN behind the rows)
    want, mag, bound, info = ref64.param_grad_fp64(c["net"]["cell"], x, p, ab, dh, inside, c["net"]["output_nonlin"],
                                                   chains=pgc.chains_of(pgc.rnn_grid_of(e.ld, t, pgc.n_cu())))
    assert info["zmax"] <= 8.0 and info["kink"] >= 1e-3 and (bound <= 1e-3 * mag + 1e-4).all()
    return want, bound, length


# ------------------------------------------------------------------------------------------------------- 1. the table
@pytest.mark.parametrize("key", list(CASES))
def test_against_the_fp64_reference(vs, key):
    e = recorded(vs, key)
    abar, d_hid = sweep(vs, key, e)
    want, bound, length = reference(vs, key, e, T, abar, d_hid)
    got = e.rnn_param_grad(T, abar, d_hid)
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == (clc.flat_params(case(key)["net"]).size,)
    got = got.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all() and e.error_count() == 0
    worst = worst_ratio(np.abs(got - want), 2.0 * bound)
    print(f"{key}: worst |kernel - fp64| / (2 bound) {worst:.3f}; lengths {np.bincount(length, minlength=T + 1).tolist()}, "
          f"second lane group {length[64:].tolist()}")
    assert np.abs(want).max() > 0.0 and worst <= 1.0, (key, worst)
    assert (length[:64] < T).any() and (length[:64] == T).any()  # lanes that end early, lanes that run through
    e.close()


def test_every_lane_of_a_group_ends_before_the_last_rows(vs):
    """the second lane group of every case but the cartpole's (whose rail is long): its six lanes all end within the first rows, so
    the tiles of that group behind them are skipped before their loads -- the table cases above run through that path"""
    for key in CASES:
        if key == "qcp-su-lstm-64":
            continue
        e = recorded(vs, key)
        assert (e.rollout_lengths(N, T)[0].cpu().numpy()[64:] <= 4).all(), key
        e.close()


# ------------------------------------------------------------------------------------------------------- 2. edges
@pytest.mark.parametrize("key", ["qbb-lstm-2x33-tanh-out", "qq-su-gru-2x64"])
def test_nan_behind_the_rows_changes_no_bit(vs, key):
    """NaN in abar, d_hid and the hidden-state record at every row t >= L and at lanes n .. ld - 1: the same bits, and finite"""
    e = recorded(vs, key)
    pgc.check_nan_behind_the_rows(e, RNN, N, T, sweep(vs, key, e), records=[e.hidden_record_tensor()])
    e.close()


def test_two_calls_and_accumulate_are_exact(vs):
    key = "qcp-su-lstm-64"
    e = recorded(vs, key)
    abar, d_hid = sweep(vs, key, e)
    pgc.check_two_calls_and_accumulate(vs, e, RNN, T, [abar, d_hid], [abar, d_hid[:, :-1].contiguous()], dense=False)
    e.close()


def test_the_handle_is_untouched(vs):
    key = "qq-su-gru-2x64"
    e = recorded(vs, key)
    pgc.check_the_handle_is_untouched(vs, e, RNN, T, lambda: sweep(vs, key, e), lambda: [e.hidden_record_tensor(), e.policy_hidden()])
    e.close()


# ------------------------------------------------------------------------------------------- 3. against the FNN pass
@pytest.mark.parametrize("key", sorted(ELMAN_AS_FNN))
def test_an_elman_cell_without_recurrence_is_the_fnn_pass(vs, key):
    """one set of records, one abar: vs_rnn_param_grad with the Elman cell (W_hh = 0, d_hid = 0) on the handle, then the network [H]
    tanh with bias b_ih + b_hh in its place and vs_fnn_param_grad -- two kernels with nothing in common but the reduction"""
    c = case(key)
    cn = c["net"]["cell"]
    w, H, A = cn["layers"][0], cn["hidden"], c["ref"].A
    O = w["w_ih"].shape[1]
    assert not w["w_hh"].any()
    e = recorded(vs, key)
    abar = torch.zeros(T, A, e.ld, device="cuda")
    abar[:, :, :N] = vs.lanes_last(dev(c["g_act"]), e.ld)[:, :, :N]
    d_hid = torch.zeros(T, c["Hs"], e.ld, device="cuda")
    want, bound, _ = reference(vs, key, e, T, abar, d_hid)
    rnn = e.rnn_param_grad(T, abar, d_hid).cpu().numpy().astype(np.float64)
    net = dict(W=[w["w_ih"], cn["w_out"]], b=[w["b_ih"] + w["b_hh"], cn["b_out"]], hidden=[H], hidden_nonlin=["tanh"], output_nonlin=None,
               feat=False, obs_idx=None)
    e.set_policy_fnn(fnn_host.flat_of(net["W"], net["b"]).astype(np.float32), [H], hidden_nonlin="tanh")
    fnn = e.fnn_param_grad(T, abar).cpu().numpy().astype(np.float64)
    x, _, ab, _, inside, _ = rows_of(vs, key, e, T, abar, d_hid)
    fb = fnn_host.param_grad_fp64(net, x, ab, inside, chains=pgc.chains_of(pgc.fnn_grid_of(e.ld, T, pgc.n_cu())))[3]
    # rnn order: w_ih [H, O], w_hh [H, H], b_ih [H], b_hh [H], w_out, b_out;  fnn order: W_1 [H, O], b_1 [H], W_out, b_out
    n1, nh = H * O, H * H
    pick = np.concatenate([np.arange(n1), n1 + nh + np.arange(H), n1 + nh + 2 * H + np.arange(A * H + A)])
    assert worst_ratio(np.abs(rnn - want), 2.0 * bound) <= 1.0                                  # (dW_hh = delta h_t^T included: h_t is not 0)
    assert np.array_equal(rnn[n1 + nh:n1 + nh + H], rnn[n1 + nh + H:n1 + nh + 2 * H])                 # db_ih and db_hh: the same sums
    worst = worst_ratio(np.abs(rnn[pick] - fnn), 2.0 * bound[pick] + 2.0 * fb)
    print(f"{key}: worst |rnn pass - fnn pass| / (sum of the doubled bounds) {worst:.3f}")
    assert np.abs(fnn).max() > 0.0 and worst <= 1.0, (key, worst)
    e.close()


# ------------------------------------------------------------------------------------------------------- 4. refusals
def test_refusals_leave_the_output_untouched(vs):
    L = vs._lib
    key = "pend-gru-8"
    c = case(key)
    e = recorded(vs, key)
    r = pgc.Refusals(vs, e, RNN, T, sweep(vs, key, e))
    r.arguments()
    e.set_policy_hidden_record(c["Hs"] + 1)                     # a record plane of another width
    r.refused(L.VS_ERR_STATE, e)
    e.set_policy_hidden_record(0)
    r.refused(L.VS_ERR_STATE, e)
    e.set_policy_hidden_record(c["Hs"])
    r.policies(vs.env_dims(c["name"]), clc.flat_params(c["net"]), lambda: e.set_policy_rnn(None), lambda: clc.set_rnn(e, c["net"]),
               dict(linear={}, fnn={}, playback={}))
    e.close()
    r.discrete_family()


# ------------------------------------------------------------------------------------------------------- 5. autograd
@pytest.mark.parametrize("name", ["pend", "qcp-su"])
def test_autograd_kernel_against_torch(vs, name, monkeypatch):
    tc = clc.torch_case("rnn", name)
    NT, TT = clc.NT, clc.TT
    cell, n_layers, H = clc.RNN_AUTOGRAD[name][:3]
    env = getattr(vs, clc.ENVS[name])(max_steps=MAX_STEPS, **KW[name])
    policy = clc.torch_policy(env.spec, cell, n_layers, H)
    th0 = clc.flat_params(tc["net"])
    policy.param_values = torch.as_tensor(th0)
    weights = list(policy.parameters())
    grads = lambda roll: pgc.autograd_grads(vs, roll, tc, weights)[:2]  # noqa: E731
    flat = lambda g: pgc.flat_grads(g[:-1])  # noqa: E731
    by_torch = vs.DifferentiableRecurrentRollout(env, policy, batch_lanes=32, param_pass="torch")
    g_torch, _ = grads(by_torch)
    by_torch.close()
    seen = []
    pgc.spy_on(vs, monkeypatch, RNN, seen)
    roll = vs.DifferentiableRecurrentRollout(env, policy, batch_lanes=32, param_pass="kernel")
    assert roll.param_pass == "kernel"
    g_kernel, loss = grads(roll)
    pgc.check_three_batches_accumulate(seen)
    pgc.check_backward_twice_and_the_sweep(loss, weights, g_kernel, g_torch)

    def bound_of(s):  # (one more add: accumulate)
        return ref64.param_grad_fp64(tc["net"]["cell"], s.obs, s.hid, *s.bufs, s.inside, None,
                                     chains=pgc.chains_of(pgc.rnn_grid_of(s.ld, TT, pgc.n_cu()), 1))[2]

    # each side within the doubled bound of the reference
    pgc.check_kernel_against_torch_pass(name, seen, bound_of, flat(g_kernel), flat(g_torch), 4.0, "2 x 2 bound")
    # ---- two plain gradient steps (in units of |theta|) lower the loss
    scale = np.abs(th0.astype(np.float64))
    eta = 0.02 / np.abs(flat(g_kernel) * scale).max()
    losses = [float(loss.detach())]
    for _ in range(2):
        g, _ = grads(roll)
        with torch.no_grad():
            policy.param_values = policy.param_values - torch.as_tensor(eta * flat(g) * scale ** 2, dtype=torch.float32)
        losses.append(float(grads(roll)[1].detach()))
    print(f"{name}: loss {losses[0]:.6f} -> {losses[1]:.6f} -> {losses[2]:.6f}")
    assert losses[2] < losses[1] < losses[0], losses
    roll.close()


# ------------------------------------------------------------------------------------------------------- 6. one workspace
def test_one_workspace_serves_both_policy_kinds_in_turn(vs):
    """The workspace of the parameter-gradient pass (index map, partial vectors) belongs to the handle's policy slot, whichever kind is
    in it.  ONE pendulum handle of 65 lanes (two lane groups, the second 1/64 full) runs, in this order,
      1. the [8] tanh network: record T = 3, sweep, fnn_param_grad           (3 ld / 64 tiles)
      2. the GRU of pend-gru-8 with its hidden record: record T = 40, rnn_param_grad
                                                                              (40 ld / 64 tiles: the buffer regrows, another packed size and map; 40 rows
                                                                              cross the 32-row done word; rows 3 .. 39 of step 1 were stale)
      3. the network again: record T = 40, fnn_param_grad                    (again another packed size and map)
      4. the same network, not set again: record T = 3, sweep, fnn_param_grad (a smaller grid in the larger buffer)
    and each result equals BIT FOR BIT that of the same call on a fresh handle: the grid is a function of (ld, t_steps, device) and the
    kernels are deterministic (test_two_calls_and_accumulate_are_exact), so a stale map, a buffer of another width or a regrow under
    a running launch would show, and nothing else can differ."""
    n, long = 65, 40
    fc, gc = clc.case("pend-8"), case("pend-gru-8")
    params, init, A = fc["params"][:n], fc["init"][:n], fc["ref"].A

    def record(e, t, set_policy):
        return record_mode2(e, long, params, set_policy, init, (t,))

    def dense(e, t, width, seed):
        return torch.randn(t, width, e.ld, device="cuda", generator=torch.Generator("cuda").manual_seed(seed))

    def fnn_short(e, set_policy=lambda e: clc.set_net(e, fc["net"])):
        record(e, 3, set_policy)
        ll = lambda x: vs.lanes_last(dev(x), e.ld)  # noqa: E731
        da, _ = e.rollout_vjp_fnn(3, g_rew=ll(fc["g_rew"][:n, :3]), g_obs=ll(fc["g_obs"][:n, :4]), g_act=ll(fc["g_act"][:n, :3]),
                                  g_state_last=ll(fc["g_last"][:n]))
        return e.fnn_param_grad(3, da)

    def gru_long(e):
        record(e, long, lambda e: clc.set_rnn(e, gc["net"]))
        return e.rnn_param_grad(long, dense(e, long, A, 6), dense(e, long, gc["Hs"], 7))

    def fnn_long(e):
        record(e, long, lambda e: clc.set_net(e, fc["net"]))
        return e.fnn_param_grad(long, dense(e, long, A, 5))

    def handle():
        return vs.VecSimEnv("pend", n, max_steps=MAX_STEPS, **KW["pend"])

    e = handle()
    got = [fnn_short(e).clone(), gru_long(e).clone(), fnn_long(e).clone()]
    length = e.rollout_lengths(n, long)[0].cpu().numpy()
    got.append(fnn_short(e, lambda e: None).clone())
    assert e.error_count() == 0
    e.close()
    for k, step in ((0, fnn_short), (1, gru_long), (2, fnn_long)):
        f = handle()
        want = step(f)
        assert bool(torch.isfinite(want).all()) and bool(want.any()) and f.error_count() == 0, k
        assert torch.equal(got[k], want), k
        if k == 0:
            assert torch.equal(got[3], want), 3
        f.close()
    assert got[0].shape == got[2].shape and got[1].shape != got[0].shape and not torch.equal(got[0], got[2])
    print(f"lengths of the network's {long}-row record: {np.bincount(length, minlength=long + 1).tolist()}")
    assert (length < long).any() and (length > 32).any()  # lanes that end early, lanes that live into the second done word
