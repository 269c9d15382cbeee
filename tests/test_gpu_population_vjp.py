"""
vs_rollout_vjp_pop / vs_pop_param_grad / DifferentiablePopulationRollout on the device (population_vjp_cases.py has the standard table,
the members and the mirror of the partition):

  * the sweep of a population against the single-policy sweep of every member on a plain handle of the same lanes, bit for bit (same
    states, parameters, T = 33, noise off, forward shape 0), exact zeros on inert lanes and lanes >= n, NaN behind the rows changes nothing;
  * the parameter pass, row by row, against the fp64 references of the single-policy passes on the recorded rows of the set's lanes,
    within their error bound with the reduction chain of the set's workgroups; the unnamed set's row is exact zeros / keeps a sentinel;
  * the check sees a wrong member (two rows swapped; two members' weights swapped);
  * determinism, accumulate, another t_steps in between; T = 1; 1 100 sets; one set over all groups against the single-policy pass;
  * the refusals; autograd against per-member runs of the single-policy classes.

The sweep against fp64 runs at closed_loop_cases.reference's own shape, 150 lanes x 24 steps, with a table over the three groups of those
lanes (sets [1, 2, 0]): d_act and d_init on a member's lanes against reference(member) within block_tolerance, the project's criterion
(at most a 2e-3 share of the smooth entries off, at most 1 % not smooth), every lane compared, lane lengths equal to the oracle's.
"""
import ctypes as C

import numpy as np
import pytest

import closed_loop_cases as clc
import param_grad_cases as pgc
import population_vjp_cases as pvc
from derivative_cases import KW, MAX_STEPS, dev
from param_grad_cases import vs  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu
CASES = pvc.LINEAR + pvc.NETS
GROUPS, N, NS, T = pvc.GROUPS_STD, pvc.N_STD, pvc.N_SETS_STD, pvc.T_STD


def _single_sweep(key, e, **cot):
    return (e.rollout_vjp_policy if pvc.is_linear(key) else e.rollout_vjp_fnn)(T, **cot)


def _rows(vs, e, da, n, t):
    """(obs [t n, O], abar [t n, A], inside [t n], lengths) of the handle, step-major"""
    obs, inside, length = pgc.rows_of(e, n, t)
    return obs, pgc.device_rows(vs, da, n), inside, length


def _check_rows(vs, key, mem, e, da, got, groups, n, t, n_sets, label):
    """every named set's row within the fp64 bound of its own lanes' rows; -> worst ratio"""
    obs, abar, inside, _ = _rows(vs, e, da, n, t)
    table = pvc.groups_of(pvc.lane_set_of(groups, n), n, e.ld)
    lane_of_row = np.tile(np.arange(n), t)
    worst = 0.0
    for s in range(n_sets):
        lanes = pvc.lanes_of_set(groups, n, s)
        if lanes.size == 0:
            assert not got[s].any(), (key, s)
            continue
        chain = (pvc.lin_chain_of_set if pvc.is_linear(key) else pvc.fnn_chains_of_set)(table, n_sets, t, s, pgc.n_cu())
        want, bound = pvc.reference_row(key, mem[s], obs, abar, inside & np.isin(lane_of_row, lanes), chain)
        assert np.abs(want).max() > 0.0
        worst = max(worst, pgc.worst_ratio(np.abs(got[s].astype(np.float64) - want), bound))
    print(f"{key} {label}: worst |kernel - fp64| / bound {worst:.3f}")
    return worst


@pytest.fixture(scope="module", params=CASES)
def pop(request, vs):
    key = request.param
    mem = pvc.members(key)
    e = pvc.population_handle(vs, key, mem)
    cot = pvc.cotangents(vs, key, e)
    da, di = e.rollout_vjp_population(T, **cot)
    yield key, mem, e, cot, da, di
    e.close()


def test_sweep_equals_the_single_policy_sweep_bit_for_bit(vs, pop):
    import torch

    key, mem, e, cot, da, di = pop
    length = e.rollout_lengths(N, T)[0].cpu().numpy()
    for s in range(3):
        lanes = torch.as_tensor(pvc.lanes_of_set(GROUPS, N, s), device="cuda")
        single = pvc.member_handle(vs, key, mem[s])
        a, b = e.traj_tensors(T, N), single.traj_tensors(T, N)
        assert all(torch.equal(a[k][:, lanes], b[k][:, lanes]) for k in ("obs", "act", "rew")), (key, s)
        sa, si = _single_sweep(key, single, **cot)
        assert torch.equal(da[:, :, lanes], sa[:, :, lanes]) and torch.equal(di[:, lanes], si[:, lanes]), (key, s)
        assert bool(sa[:, :, lanes].any()) and bool(si[:, lanes].any())
        single.close()
    inert = torch.as_tensor(pvc.lanes_of_set(GROUPS, N, -1), device="cuda")
    assert inert.numel() == 64 and not bool(da[:, :, inert].any()) and not bool(di[:, inert].any())
    assert not bool(da[:, :, N:].any()) and not bool(di[:, N:].any())
    live = pvc.lane_set_of(GROUPS, N) >= 0
    assert (length[~live] == 0).all() and (length[live] < T).any() and (length[live] == T).any()
    assert (length[live] == 1).any()   # a lane that ends at step 1: the one-row run (the cases' edge lanes, in groups 0 and 4)


@pytest.mark.parametrize("key", CASES)
def test_sweep_against_the_fp64_closed_loop_of_every_member(vs, key):
    from derivative_cases import N as N0, T as T0, scaled, smooth_per_lane

    groups = (1, 2, 0)
    mem = pvc.members(key)
    e = pvc.population_handle(vs, key, mem, groups=groups, n=N0, t=T0)
    da, di = e.rollout_vjp_population(T0, **pvc.cotangents(vs, key, e, n=N0, t=T0))
    got = scaled(vs, mem[0], da, di)                                                   # [150, T A + S] per ACT_IN / INIT_SCALE
    length = e.rollout_lengths(N0, T0)[0].cpu().numpy()
    assert e.error_count() == 0
    e.close()
    for s in range(3):
        lanes = pvc.lanes_of_set(groups, N0, s)
        r = pvc.member_reference(key, s)
        f1, smooth = r.f1[lanes], smooth_per_lane(r.f1, r.f2)[lanes]
        assert lanes.size > 0 and (~smooth).mean() <= 0.01 and np.array_equal(length[lanes], r.length[lanes]), (key, s)
        tol = clc.block_tolerance(mem[s], f1, smooth)
        err = np.abs(got[lanes] - f1)
        bad = float((smooth & (err > tol)).mean())
        print(f"{key} member {s}: {lanes.size} lanes, not smooth {(~smooth).mean():.4f}, bad share {bad:.2e}, worst error / tolerance "
              f"{float((err[smooth] / tol[smooth]).max()):.3f}")
        assert bad <= 2e-3, (key, s, bad)


def test_nan_behind_the_rows_changes_nothing(vs, pop):
    """check_nan_behind_the_rows' method on both calls: NaN in the cotangents at every row t >= L (inert groups: every row) and at lanes
    >= n gives the same bits, and so does NaN in abar there for the parameter pass"""
    import torch

    key, mem, e, cot, da, di = pop
    length = e.rollout_lengths(N, T)[0]
    nan = torch.full((), float("nan"), device="cuda")

    def poison(x, steps, shift=0):  # x [steps, W, ld] or [steps, ld]
        y = x.clone()
        behind = torch.arange(steps, device="cuda")[:, None] >= (length[None, :] + shift)
        view = y if y.dim() == 3 else y[:, None, :]
        view[:, :, :N] = torch.where(behind[:, None, :], nan, view[:, :, :N])
        view[:, :, N:] = nan
        return y

    dirty = dict(g_rew=poison(cot["g_rew"], T), g_act=poison(cot["g_act"], T), g_obs=poison(cot["g_obs"], T + 1, 1),
                 g_state_last=cot["g_state_last"].clone())
    inert = torch.as_tensor(pvc.lanes_of_set(GROUPS, N, -1), device="cuda")
    dirty["g_state_last"][:, inert] = nan
    dirty["g_state_last"][:, N:] = nan
    assert all(bool(torch.isnan(x).any()) for x in dirty.values())
    da2, di2 = e.rollout_vjp_population(T, **dirty)
    assert torch.equal(da2, da) and torch.equal(di2, di)
    clean = e.population_param_grad(T, da)
    got = e.population_param_grad(T, poison(da, T))
    assert bool(torch.isfinite(got).all()) and torch.equal(got, clean) and bool(clean.any())


def test_parameter_pass_against_fp64_and_the_check_sees_a_wrong_member(vs, pop):
    import torch

    key, mem, e, cot, da, di = pop
    got = e.population_param_grad(T, da)
    assert tuple(got.shape) == (NS, pvc.theta_of(key, mem).shape[1]) and not bool(got[3].any())   # nobody names set 3
    g = got.cpu().numpy()
    assert _check_rows(vs, key, mem, e, da, g, GROUPS, N, T, NS, "standard table") <= 1.0
    assert _check_rows(vs, key, mem, e, da, g[[1, 0, 2, 3]], GROUPS, N, T, NS, "rows 0 and 1 swapped") > 1.0
    if not pvc.is_linear(key):  # (a linear policy's parameter pass does not read the weights)
        swapped = (mem[1], mem[0]) + tuple(mem[2:])
        assert _check_rows(vs, key, swapped, e, da, g, GROUPS, N, T, NS, "members 0 and 1 swapped") > 1.0
    out = torch.full_like(got, 7.0)
    assert e.population_param_grad(T, da, out=out, accumulate=True) is out
    assert bool((out[3] == 7.0).all()) and torch.equal(out[:3], 7.0 + got[:3])                     # one fp32 add per entry; the sentinel


def test_two_calls_accumulate_and_another_t_steps_in_between(vs, pop):
    import torch

    key, mem, e, cot, da, di = pop
    g = e.population_param_grad(T, da)
    assert torch.equal(e.population_param_grad(T, da), g)
    short = e.population_param_grad(T - 5, da[:T - 5].contiguous())                                # another partition in between
    assert torch.equal(e.population_param_grad(T, da), g) and not torch.equal(short, g)
    fresh = pvc.population_handle(vs, key, mem)
    fa, fi = fresh.rollout_vjp_population(T, **cot)
    assert torch.equal(fa, da) and torch.equal(fresh.population_param_grad(T, fa), g)              # the bits of a fresh handle
    fresh.close()
    r = torch.randn(g.shape, device="cuda", generator=torch.Generator("cuda").manual_seed(3))
    out = r.clone()
    e.population_param_grad(T, da, out=out, accumulate=True)
    assert torch.equal(out[:3], (r + g)[:3]) and torch.equal(out[3], r[3])
    with pytest.raises(vs.ValueErr):
        e.population_param_grad(T, da, accumulate=True)
    with pytest.raises(vs.ShapeErr):
        e.population_param_grad(T, da[:, :, :-1].contiguous())
    g1 = e.population_param_grad(1, da[:1].contiguous())                                           # T = 1
    assert _check_rows(vs, key, mem, e, da[:1].contiguous(), g1.cpu().numpy(), GROUPS, N, 1, NS, "T = 1") <= 1.0


@pytest.mark.parametrize("key", ["qq-su", "qq-su-16"])
def test_more_sets_than_any_grid_cap(vs, key):
    """1 100 sets x 64 lanes at T = 3: every set still gets a workgroup; rows against fp64 (members cycle through the four drawn)"""
    n_sets, t = 1100, 3
    four = pvc.members(key)
    mem = tuple(four[s % 4] for s in range(n_sets))
    groups = tuple(range(n_sets))
    e = pvc.population_handle(vs, key, mem, groups=groups, n=64 * n_sets, t=t)
    da, _ = e.rollout_vjp_population(t, **pvc.cotangents(vs, key, e, n=64 * n_sets, t=t))
    got = e.population_param_grad(t, da).cpu().numpy()
    assert np.abs(got).max(axis=1).min() > 0.0
    assert _check_rows(vs, key, mem, e, da, got, groups, 64 * n_sets, t, n_sets, "1100 sets") <= 1.0
    e.close()


@pytest.mark.parametrize("key", ["qq-su", "qcp-su-32x33"])
def test_one_set_over_all_groups_against_the_single_policy_pass(vs, key):
    import torch

    mem = pvc.members(key)[:1]
    groups = (0,) * 6
    e = pvc.population_handle(vs, key, mem, groups=groups)
    cot = pvc.cotangents(vs, key, e)
    da, di = e.rollout_vjp_population(T, **cot)
    got = e.population_param_grad(T, da)
    single = pvc.member_handle(vs, key, mem[0])
    sa, si = _single_sweep(key, single, **cot)
    assert torch.equal(sa, da) and torch.equal(si, di)
    want = (single.lin_param_grad if pvc.is_linear(key) else single.fnn_param_grad)(T, sa).cpu().numpy().astype(np.float64)
    obs, abar, inside, _ = _rows(vs, single, sa, N, T)
    table = pvc.groups_of(pvc.lane_set_of(groups, N), N, e.ld)
    if pvc.is_linear(key):
        chains = [pvc.lin_chain_of_set(table, 1, T, 0, pgc.n_cu()), pgc.chain_of(e.ld, T, pgc.n_cu())]
    else:
        chains = [pvc.fnn_chains_of_set(table, 1, T, 0, pgc.n_cu()), pgc.chains_of(pgc.fnn_grid_of(e.ld, T, pgc.n_cu()))]
    bound = sum(pvc.reference_row(key, mem[0], obs, abar, inside, c)[1] for c in chains)           # each within its own bound of fp64
    worst = pgc.worst_ratio(np.abs(got[0].cpu().numpy() - want), bound)
    print(f"{key}: one set over all groups against the single-policy pass, worst difference / (sum of both bounds) {worst:.3f}")
    assert worst <= 1.0
    e.close(), single.close()


def test_refusals_leave_the_outputs_untouched(vs):
    import torch

    key = "qq-su"
    L, lib = vs._lib, vs._lib.load()
    mem = pvc.members(key)
    e = pvc.population_handle(vs, key, mem)
    theta, lane_set = pvc.theta_of(key, mem), pvc.lane_set_of(GROUPS, N)
    A, SH, n_params = e.dims["A"], e.dims["S"] + e.dims["H"], theta.shape[1]
    o1, o2 = torch.full((T, A, e.ld), 7.0, device="cuda"), torch.full((SH, e.ld), 7.0, device="cuda")
    gp = torch.full((NS, n_params), 7.0, device="cuda")
    ab = torch.zeros(T, A, e.ld, device="cuda")
    ptr = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731

    def refused(code, n_sets=NS, n=n_params, t=T, which=(0, 1)):
        for k in which:
            name = ("vs_rollout_vjp_pop", "vs_pop_param_grad")[k]
            rc = (lib.vs_rollout_vjp_pop(e._h, t, None, None, None, None, ptr(o1), ptr(o2)) if k == 0 else
                  lib.vs_pop_param_grad(e._h, t, ptr(ab), ptr(gp), n_sets, n, 0))
            torch.cuda.synchronize()
            assert rc == code and name in lib.vs_last_error(e._h).decode(), (name, rc)
            assert bool((o1 == 7.0).all()) and bool((o2 == 7.0).all()) and bool((gp == 7.0).all())

    def population():
        e.set_policy_population(theta, lane_set=lane_set)

    refused(L.VS_ERR_ARG, n_sets=NS + 1, which=(1,))
    refused(L.VS_ERR_ARG, n_sets=NS - 1, which=(1,))
    refused(L.VS_ERR_ARG, n=n_params + 1, which=(1,))
    refused(L.VS_ERR_ARG, t=0)
    refused(L.VS_ERR_ARG, t=T + 1)
    e.set_policy_population(None)
    refused(L.VS_ERR_STATE)                                                                        # no population
    population()
    e.set_traj_offset(3)
    refused(L.VS_ERR_STATE)
    e.set_traj_offset(0)
    e.set_auto_reset(True)
    refused(L.VS_ERR_STATE)
    e.set_auto_reset(False)
    d = e.dims
    kinds = pgc.other_kinds(e, d, T)
    kinds["playback"]()
    refused(L.VS_ERR_STATE)                                                                        # a playback policy
    kinds["gru"]()
    gru = np.zeros((NS, 3 * 8 * (d["O"] + 8 + 2) + 9 * d["A"]), dtype=np.float32)
    e.set_policy_population(gru, lane_set=lane_set)
    refused(L.VS_ERR_STATE, n=gru.shape[1])                                                        # a recurrent policy with a population
    kinds["fnn3"]()
    fnn3 = np.zeros((NS, (d["O"] + 1) * 8 + 2 * 9 * 8 + 9 * d["A"]), dtype=np.float32)
    e.set_policy_population(fnn3, lane_set=lane_set)
    refused(L.VS_ERR_STATE, n=fnn3.shape[1])                                                       # three hidden layers
    clc.policy_of(mem[0]).install(e)
    population()
    e.set_record_mode(1)
    e.set_traj_capacity(T)
    refused(L.VS_ERR_STATE)
    e.set_record_mode(2)
    e.set_traj_capacity(T)
    # after the refusals the same handle serves both calls
    assert lib.vs_rollout_vjp_pop(e._h, T, None, None, None, None, ptr(o1), ptr(o2)) == L.VS_OK
    assert lib.vs_pop_param_grad(e._h, T, ptr(ab), ptr(gp), NS, n_params, 0) == L.VS_OK
    torch.cuda.synchronize()
    assert not bool((gp == 7.0).any()) and e.error_count() == 0
    e.close()


def test_the_handle_is_untouched(vs, pop):
    key, mem, e, cot, da, di = pop
    fam = pgc.Family("population", (), 321)  # (its method: population_param_grad)
    pgc.check_the_handle_is_untouched(vs, e, fam, T, lambda: list(e.rollout_vjp_population(T, **cot)))


# ------------------------------------------------------------------------------------------------------------ autograd
def _torch_policy(vs, kind, name, env, tc):
    import torch

    if kind == "linear":
        policy = vs.LinearPolicy(env.spec, vs.FeatureStack(vs.identity_feat, vs.sin_feat, vs.const_feat, vs.MultFeat((0, 1))))
        with torch.no_grad():
            policy.net.weight.copy_(torch.as_tensor(tc["W"]))
        return policy
    policy = vs.FNNPolicy(env.spec, list(clc.FNN_AUTOGRAD[name]), torch.tanh, featurize=False)
    with torch.no_grad():
        torch.nn.utils.vector_to_parameters(torch.as_tensor(clc.flat_params(tc["net"])), policy.parameters())
    return policy


def _member_of(kind, tc, theta_row):
    """the fp64 form of a member from its flat float32 parameters (what reference_row takes)"""
    flat = np.asarray(theta_row, dtype=np.float32)
    if kind == "linear":
        return dict(terms=clc.SMALL, obs_idx=None, W=flat.reshape(tc["W"].shape))
    net, at, W, b = tc["net"], 0, [], []
    for w0, b0 in zip(net["W"], net["b"]):
        W.append(flat[at:at + w0.size].reshape(w0.shape))
        b.append(flat[at + w0.size:at + w0.size + b0.size])
        at += w0.size + b0.size
    assert at == flat.size
    return dict(net=dict(net, W=W, b=b))


def _pass_bounds(kind, tc, theta, seen, lanes_of_call):
    """per member the fp64 gradient and the summed error bound of the calls in `seen` (param_grad_cases.Seen); lanes_of_call(k) -> the
    lane table of call k ([n] member per lane) or None for a single-policy call (its one member: theta[0]).  Every later call adds
    onto the earlier ones: one more add in its chain."""
    P = len(theta)
    want, bound = [0.0] * P, [0.0] * P
    for k, sn in enumerate(seen):
        table = lanes_of_call(k)
        t = sn.obs.shape[0] // sn.n
        lane_of_row = np.tile(np.arange(sn.n), t)
        more = 1 if k else 0
        for m in range(P):
            if table is None:
                inside = sn.inside
                chain = (pgc.chain_of(sn.ld, t, pgc.n_cu(), more) if kind == "linear"
                         else pgc.chains_of(pgc.fnn_grid_of(sn.ld, t, pgc.n_cu()), more))
            else:
                lanes = np.flatnonzero(table == m)
                if lanes.size == 0:
                    continue
                inside = sn.inside & np.isin(lane_of_row, lanes)
                groups = pvc.groups_of(table, sn.n, sn.ld)
                chain = (pvc.lin_chain_of_set(groups, P, t, m, pgc.n_cu()) + more if kind == "linear"
                         else pvc.fnn_chains_of_set(groups, P, t, m, pgc.n_cu(), more))
            g, b = pvc.reference_row(None, _member_of(kind, tc, theta[m]), sn.obs, sn.bufs[0], inside, chain)
            want[m], bound[m] = want[m] + g, bound[m] + b
    return want, bound


@pytest.mark.parametrize("kind, name", [("linear", "qq-su"), ("fnn", "qcp-su")])
def test_autograd_against_per_member_rollouts(vs, kind, name, monkeypatch):
    """P = 3 members x M = 65 rollouts x T = 24.  Every parameter pass that runs is recorded (param_grad_cases.spy_on) and given its
    fp64 sum and first-order error bound on the rows it saw, with its own chains: the partition mirror for a population call, the
    single-policy grid rule for a per-member call, one more add for a call that accumulates.  params.grad[s] against the per-member
    class (kernel parameter pass): within the SUM of the two passes' bounds, entry by entry -- both are within their own bound of the
    same fp64 sum.  Three batches of 128 lanes against one batch: within the sum of the one call's and the three calls' bounds (their
    reduction chains).  Each result is also held to its own bound of fp64.  d init_states: the same bits; backward() twice: the same
    bits."""
    import torch

    from simurlacra_amd.diffsim import population_lanes

    P, M, TT = 3, 65, 24
    tc = clc.torch_case(kind, name)
    env = getattr(vs, clc.ENVS[name])(max_steps=MAX_STEPS, **KW[name])
    rng = np.random.default_rng(5)
    base = _torch_policy(vs, kind, name, env, tc)
    flat0 = torch.nn.utils.parameters_to_vector(base.parameters()).detach()
    theta = (flat0[None, :] * torch.as_tensor(1.0 + 0.05 * rng.uniform(-1, 1, (P, flat0.numel())), dtype=torch.float32)).cuda()
    theta_np = theta.cpu().numpy()
    init = dev(tc["init"][:M]).repeat(P, 1, 1)
    lane_set = population_lanes(P, M)[2]
    seen_pop, seen_one = [], []
    pgc.spy_on(vs, monkeypatch, pgc.Family("population", (), 321), seen_pop)
    pgc.spy_on(vs, monkeypatch, pgc.LIN if kind == "linear" else pgc.FNN, seen_one)

    def loss_of(rew, act, lengths):
        return -vs.discounted_return(rew, lengths, clc.GAMMA).sum() + 1e-3 * act.pow(2).sum()

    def run(batch_lanes):
        roll = vs.DifferentiablePopulationRollout(env, base, batch_lanes=batch_lanes)
        th, s0 = theta.clone().requires_grad_(True), init.clone().requires_grad_(True)
        obs, rew, act, lengths = roll.roll(th, s0, TT)
        assert tuple(obs.shape) == (P, M, TT + 1, env.obs_space.flat_dim) and tuple(lengths.shape) == (P, M)
        loss = loss_of(rew.reshape(P * M, TT), act.reshape(P * M, TT, -1), lengths.reshape(-1))
        del seen_pop[:]
        g = torch.autograd.grad(loss, [th, s0], retain_graph=True)
        calls = list(seen_pop)
        again = torch.autograd.grad(loss, [th, s0])
        assert all(torch.equal(a, b) for a, b in zip(g, again))                                    # backward() twice
        n_batches = len(roll._vecs)
        roll.close()
        starts = np.cumsum([0] + [c.n for c in calls])
        want, bound = _pass_bounds(kind, tc, theta_np, calls, lambda k: lane_set[starts[k]:starts[k + 1]])
        return g, n_batches, calls, want, bound

    (g_th, g_s0), nb, calls1, want1, bound1 = run(65536)
    (b_th, b_s0), nb3, calls3, want3, bound3 = run(128)
    assert (nb, nb3) == (1, 3) and [c.accumulate for c in calls1] == [False] and [c.accumulate for c in calls3] == [False, True, True]
    assert torch.equal(b_s0, g_s0) and bool(g_s0.any())
    g1, g3 = g_th.cpu().numpy().astype(np.float64), b_th.cpu().numpy().astype(np.float64)
    Single = vs.DifferentiablePolicyRollout if kind == "linear" else vs.DifferentiableNetRollout
    for s in range(P):
        assert np.abs(want1[s]).max() > 0.0
        own1, own3 = pgc.worst_ratio(np.abs(g1[s] - want1[s]), bound1[s]), pgc.worst_ratio(np.abs(g3[s] - want3[s]), bound3[s])
        split = pgc.worst_ratio(np.abs(g3[s] - g1[s]), bound1[s] + bound3[s])
        member = _torch_policy(vs, kind, name, env, tc)
        with torch.no_grad():
            torch.nn.utils.vector_to_parameters(theta[s].cpu(), member.parameters())
        roll = Single(env, member, param_pass="kernel")
        s0 = init[s].clone().requires_grad_(True)
        obs, rew, act, lengths = roll(s0, TT)
        del seen_one[:]
        g = torch.autograd.grad(loss_of(rew, act, lengths), list(member.parameters()) + [s0])
        assert len(seen_one) == 1 and torch.equal(g[-1], g_s0[s]), (kind, s)                        # the same sweep
        _, bound_one = _pass_bounds(kind, tc, theta_np[s:s + 1], seen_one, lambda k: None)
        got_one = torch.cat([x.reshape(-1) for x in g[:-1]]).cpu().numpy().astype(np.float64)
        against = pgc.worst_ratio(np.abs(g1[s] - got_one), bound1[s] + bound_one[0])
        print(f"{kind} {name} member {s}: |population - fp64| / bound {own1:.3f} (three batches {own3:.3f}); three batches against one / "
              f"(sum of their bounds) {split:.3f}; against the single-policy class / (sum of both bounds) {against:.3f}")
        assert max(own1, own3, split, against) <= 1.0, (kind, s, own1, own3, split, against)
        roll.close()
