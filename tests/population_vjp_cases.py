"""
What the tests of the population sweep and its parameter pass share (test_population_vjp_host, test_gpu_population_vjp): the Python mirror
of the partition of the tile space by set (pop_partition of simurlacra_amd/csrc/vecsim.hip, line by line), the chains of a set's sum, the
standard lane table, the members' weights and the recording of a population handle.  Not a test module: import it by bare name.

The standard table: 5 groups of 64 lanes + 17 lanes (N = 337, the last group partial), sets [0, 1, -1, 2, 0, 1] -- sets 0 and 1 are named by
non-adjacent groups, group 2 is inert, set 3 of n_sets = 4 is named by nobody.  Lane k runs the case's lane k % 150, so every group but
the partial one holds some of the case's edge lanes (they end early).  The members' weights are independent draws of
closed_loop_cases.make_weights / make_net (seed 900 + member).

T_STD = 33 steps cross a done word; the case's cotangents have 24 steps, so the tests repeat them cyclically in time (np.resize) -- the
same values on every handle that is compared.  closed_loop_cases.reference is tied to 150 lanes x 24 steps: what is compared against it
runs at those.
"""
import functools

import numpy as np

import closed_loop_cases as clc
import param_grad_cases as pgc
from derivative_cases import KW, MAX_STEPS, N, T, dev, record_mode2

GROUPS_STD = (0, 1, -1, 2, 0, 1)
N_STD, N_SETS_STD, T_STD = 5 * 64 + 17, 4, 33
LINEAR = ("qq-su", "qbb")
NETS = ("qq-su-16", "qcp-su-32x33")


# ------------------------------------------------------------------------------------------------- the partition, mirrored
def partition(groups, n_sets, t_steps, per_wg, cap):
    """pop_partition: groups[g] the set of lane group g (-1: inert or past n_envs) -> (ent, wg, seg): the groups that name a set in stable
    order by (set, group); per workgroup (first entry of its set, entries of its set, rank among the set's workgroups, workgroups of the
    set); per set (first workgroup, workgroups).  A set WANTS ceil(tiles / per_wg) workgroups (tiles = its groups x t_steps); while all
    wants fit under cap every set gets what it wants, beyond that floor(cap tiles_s / tiles), at least 1 and at most what it wants."""
    cnt = [0] * n_sets
    for s in groups:
        if s >= 0:
            cnt[s] += 1
    first, n_ent = [], 0
    for s in range(n_sets):
        first.append(n_ent)
        n_ent += cnt[s]
    ent, at = [0] * n_ent, list(first)
    for g, s in enumerate(groups):
        if s >= 0:
            ent[at[s]] = g
            at[s] += 1
    tiles = n_ent * t_steps
    want = sum(-(-cnt[s] * t_steps // per_wg) for s in range(n_sets))
    wg, seg = [], []
    for s in range(n_sets):
        ts = cnt[s] * t_steps
        k = ws = -(-ts // per_wg)
        if want > cap and ts > 0:
            k = min(ws, max(1, cap * ts // tiles))
        seg.append((len(wg), k))
        wg += [(first[s], cnt[s], r, k) for r in range(k)]
    return ent, wg, seg


@functools.lru_cache(maxsize=8)
def _partition_of(groups, n_sets, t_steps, per_wg, cap):
    return partition(groups, n_sets, t_steps, per_wg, cap)


def runs_of(row, t_steps, waves):
    """the kernels' run of tiles per wave of one workgroup `row` of wg: [(tile0, tile1)] in its set's tile space (entry major)"""
    _, cnt, r, k = row
    tiles, n_runs = cnt * t_steps, k * waves
    chunk = -(-tiles // n_runs)
    out = []
    for w in range(waves):
        t0 = min((r * waves + w) * chunk, tiles)
        out.append((t0, min(t0 + chunk, tiles)))
    return out


def grid_of_set(groups, n_sets, t_steps, s, kind, n_cu):
    """(workgroups of set s, rows a wave accumulates at most) -- what param_grad_cases.chains_of / reduce_chain take; kind: "lin" | "fnn" """
    waves, cap = (1, 4 * n_cu) if kind == "lin" else (4, 2 * n_cu)
    _, wg, seg = _partition_of(tuple(groups), n_sets, t_steps, waves, cap)
    k = seg[s][1]
    if k == 0:
        return 0, 0
    cnt = wg[seg[s][0]][1]
    return k, 64 * -(-cnt * t_steps // (k * waves))


def lin_chain_of_set(groups, n_sets, t_steps, s, n_cu):
    """param_grad_cases.chain_of for set s: the FMAs of a wave's run, the reduce chain over the set's workgroups, 1 for accumulate"""
    k, acc = grid_of_set(groups, n_sets, t_steps, s, "lin", n_cu)
    return acc + pgc.reduce_chain(k) + 1


def fnn_chains_of_set(groups, n_sets, t_steps, s, n_cu, more_adds=0):
    return pgc.chains_of(grid_of_set(groups, n_sets, t_steps, s, "fnn", n_cu), more_adds)


def library_partition(groups, n_sets, t_steps, per_wg, cap):
    """the same from pop_partition itself (vs_pop_partition: host only, no device) -> (ent, wg, seg) in the mirror's form"""
    import ctypes as C

    from simurlacra_amd import _lib as L

    g = (C.c_int32 * len(groups))(*groups)
    seg = (C.c_int32 * (2 * n_sets))()
    ent = (C.c_int32 * len(groups))()
    n_wg = L.load().vs_pop_partition(g, len(groups), n_sets, t_steps, per_wg, cap, seg, None, 0, ent)
    assert n_wg >= 0, n_wg
    wg = (C.c_int32 * (4 * max(n_wg, 1)))()
    assert L.load().vs_pop_partition(g, len(groups), n_sets, t_steps, per_wg, cap, seg, wg, n_wg, ent) == n_wg
    n_ent = sum(1 for s in groups if s >= 0)
    return list(ent[:n_ent]), [tuple(wg[4 * k:4 * k + 4]) for k in range(n_wg)], [tuple(seg[2 * s:2 * s + 2]) for s in range(n_sets)]


def groups_of(lane_set, n, ld):
    """the table's groups as the library derives them: the set of every aligned group of 64 lanes, -1 past n"""
    return [int(lane_set[g * 64]) if g * 64 < n else -1 for g in range(ld // 64)]


# ------------------------------------------------------------------------------------------------- the members
def is_linear(key):
    return key in LINEAR


@functools.lru_cache(maxsize=None)
def members(key, n_sets=N_SETS_STD, t=T):
    """n_sets independent policies of the case's architecture -> tuple of case dicts (the case with W or net replaced)"""
    c = clc.case(key)
    ref, name = c["ref"], c["name"]
    p64, s64 = c["params"].astype(np.float64), c["init"].astype(np.float64)
    out = []
    for s in range(n_sets):
        rng = np.random.default_rng(900 + s)
        if is_linear(key):
            out.append(dict(c, W=clc.make_weights(ref, name, c["terms"], c["obs_idx"], p64, s64, c["h0"], rng, t)))
        else:
            _, hidden, hn, on, feat, obs_idx, _, gain = clc.FNN_CASES[key]
            out.append(dict(c, net=clc.make_net(ref, name, hidden, hn, on, feat, obs_idx, p64, s64, c["h0"], rng, t, gain)))
    return tuple(out)


def theta_of(key, mem):
    """[n_sets, n_params] float32: the members' flat parameters in the order of the policy's setter"""
    return np.stack([m["W"].astype(np.float32).reshape(-1) if is_linear(key) else clc.flat_params(m["net"]) for m in mem])


def lane_set_of(groups, n):
    return np.repeat(np.asarray(groups, dtype=np.int32), 64)[:n]


def _record(vs, c, n, t, install):
    name = c["name"]
    rs = lambda x: np.resize(x, (n,) + x.shape[1:])  # noqa: E731
    e = vs.VecSimEnv(name, n, max_steps=MAX_STEPS, **KW[name])
    return record_mode2(e, t, rs(c["params"]), install, rs(c["init"]), (t,))


def population_handle(vs, key, mem, groups=GROUPS_STD, n=N_STD, t=T_STD):
    """a handle of n lanes whose rows 0 .. t - 1 hold the rollouts of the population (lane k: the case's lane k % 150, forward shape 0)"""
    def install(e):
        clc.policy_of(mem[0]).install(e)
        if not is_linear(key):
            e.set_policy_shape("64")   # (forward shape 0: 64-env workgroups on both handles)
        e.set_policy_population(theta_of(key, mem), lane_set=lane_set_of(groups, n))

    return _record(vs, mem[0], n, t, install)


def member_handle(vs, key, m, n=N_STD, t=T_STD):
    """a plain handle of the same n lanes with the member m as an ordinary policy"""
    def install(e):
        clc.policy_of(m).install(e)
        if not is_linear(key):
            e.set_policy_shape("64")   # (forward shape 0: 64-env workgroups on both handles)

    return _record(vs, m, n, t, install)


def cotangents(vs, key, e, n=N_STD, t=T_STD):
    """the case's cotangents repeated over the lanes (lane k: k % 150) and cyclically in time, lanes last, under the sweep's keywords"""
    c = clc.case(key)

    def up(x, steps):
        x = x[np.arange(n) % N]
        if steps is not None:
            x = x[:, np.arange(steps) % x.shape[1]]
        return vs.lanes_last(dev(np.ascontiguousarray(x)), e.ld)

    return dict(g_rew=up(c["g_rew"], t), g_obs=up(c["g_obs"], t + 1), g_act=up(c["g_act"], t), g_state_last=up(c["g_last"], None))


def lanes_of_set(groups, n, s):
    """the lanes < n whose group names set s (s = -1: the inert groups)"""
    return np.flatnonzero(lane_set_of(groups, n) == s)


@functools.lru_cache(maxsize=None)
def member_reference(key, s):
    """closed_loop_cases.reference of member s of the case (its 150 lanes x 24 steps, no noise): the action-offset and initial-state
    columns"""
    m = members(key)[s]
    return clc.reference(m, np.zeros((N, T, m["ref"].A)), first_block_only=True)


def reference_row(key, m, obs, abar, inside, chain):
    """(fp64 gradient of member m over the rows inside, its error bound), flat in the setter's order; key: unused where m says what it
    is (a member with "terms" is linear)"""
    from fnn_param_grad_fp64 import param_grad_fp64
    from lin_param_grad_fp64 import lin_param_grad_fp64

    if "terms" in m:
        g, _, bound = lin_param_grad_fp64(m["terms"], m["obs_idx"], obs, abar, inside, chain=chain)
        return g.reshape(-1), bound.reshape(-1)
    g, _, _, bound = param_grad_fp64(m["net"], obs, abar, inside, chains=chain)
    return g, bound
