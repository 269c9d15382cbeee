"""
vs_rollout_vjp_pop / vs_pop_param_grad / DifferentiablePopulationRollout, the parts that need no GPU: the C-ABI declarations, export and
binding, the refusals before any device call, the Python argument checks, the partition of the tile space by set (the mirror in
population_vjp_cases.py of pop_partition in vecsim.hip) over random lane tables, and the padding-lane bookkeeping of the rollout class.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import simurlacra_amd as vs

torch = pytest.importorskip("torch")

import population_vjp_cases as pvc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------- the C-ABI
def test_header_declares_both_signatures():
    header = open(os.path.join(ROOT, "include", "vecsim.h")).read()
    assert re.search(r"int\s+vs_rollout_vjp_pop\(vs_handle h, int t_steps, const float\* g_rew, const float\* g_obs, const float\* g_act,"
                     r"\s*const float\* g_state_last, float\* d_act, float\* d_init\);", header)
    assert re.search(r"int\s+vs_pop_param_grad\(vs_handle h, int t_steps, const float\* abar, float\* d_params, int n_sets, "
                     r"int64_t n_params, int accumulate\);", header)


def test_symbols_are_exported_and_bound():
    from simurlacra_amd import _lib as L

    lib = C.CDLL(L.LIB_PATH)
    for name, argtypes in (("vs_rollout_vjp_pop", [C.c_void_p, C.c_int] + [C.c_void_p] * 6),
                           ("vs_pop_param_grad", [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int])):
        assert hasattr(lib, name) and name in L.exported_symbols()
        fn = getattr(L.load(), name)
        assert fn.restype is C.c_int and list(fn.argtypes) == argtypes
    assert L.load().vs_version() >= 321
    assert callable(vs.VecSimEnv.rollout_vjp_population) and callable(vs.VecSimEnv.population_param_grad)
    assert vs.DifferentiablePopulationRollout.__name__ == "DifferentiablePopulationRollout"


def test_null_handle_and_null_pointers_are_refused_before_a_device_is_touched():
    from simurlacra_amd import _lib as L

    lib, buf = L.load(), (C.c_float * 4)()
    assert lib.vs_rollout_vjp_pop(None, 1, None, None, None, None, buf, buf) == L.VS_ERR_ARG
    assert lib.vs_rollout_vjp_pop(None, 1, None, None, None, None, None, buf) == L.VS_ERR_ARG
    assert lib.vs_rollout_vjp_pop(None, 1, None, None, None, None, buf, None) == L.VS_ERR_ARG
    assert lib.vs_pop_param_grad(None, 1, buf, buf, 1, 4, 0) == L.VS_ERR_ARG
    assert lib.vs_pop_param_grad(None, 1, None, buf, 1, 4, 0) == L.VS_ERR_ARG
    assert lib.vs_pop_param_grad(None, 1, buf, None, 1, 4, 1) == L.VS_ERR_ARG
    assert all(x == 0.0 for x in buf)


# ----------------------------------------------------------------------------------------------- the Python surface
def _env_and_policies():
    env = vs.QQubeSwingUpSim(dt=0.004, max_steps=30)
    lin = vs.LinearPolicy(env.spec, vs.FeatureStack(vs.identity_feat, vs.sin_feat, vs.const_feat, vs.MultFeat((0, 1))))
    return env, lin


def test_argument_checks_of_the_rollout_class():
    env, lin = _env_and_policies()
    roll = vs.DifferentiablePopulationRollout(env, lin)
    S, n_params = env.state_space.flat_dim, sum(p.numel() for p in lin.parameters())
    assert roll.n_params == n_params and not roll._vecs                                   # nothing touched a device
    assert vs.DifferentiablePopulationRollout(env, vs.NormalActNoiseExplStrat(lin, std_init=0.1)).n_params == n_params
    ok_p, ok_s = torch.zeros(3, n_params), torch.zeros(3, 5, S)
    for params, init in ((torch.zeros(3, n_params + 1), ok_s), (torch.zeros(n_params), ok_s), (ok_p, torch.zeros(2, 5, S)),
                         (ok_p, torch.zeros(3, 5, S + 1)), (ok_p, torch.zeros(3, S)), (ok_p, torch.zeros(3, 0, S))):
        with pytest.raises(vs.ShapeErr):
            roll.roll(params, init, 4)
    with pytest.raises(vs.ValueErr):
        roll.roll(ok_p, ok_s, 0)
    with pytest.raises(vs.TypeErr):
        roll.roll(ok_p, ok_s, 4)                                                          # host tensors
    with pytest.raises(vs.TypeErr):
        roll.roll(ok_p.numpy(), ok_s, 4)
    with pytest.raises(vs.ValueErr):
        vs.DifferentiablePopulationRollout(env, lin, batch_lanes=63)
    assert not roll._vecs


def test_an_unsupported_policy_is_refused():
    env, _ = _env_and_policies()
    with pytest.raises(vs.TypeErr, match="DifferentiablePopulationRollout"):
        vs.DifferentiablePopulationRollout(env, vs.GRUPolicy(env.spec, 8, 1))
    with pytest.raises(vs.TypeErr):
        vs.DifferentiablePopulationRollout(env, torch.nn.Linear(env.obs_space.flat_dim, 1))
    with pytest.raises(vs.ValueErr, match="one or two hidden layers"):
        vs.DifferentiablePopulationRollout(env, vs.FNNPolicy(env.spec, [8, 8, 8], torch.tanh, featurize=False))
    two = vs.DifferentiablePopulationRollout(env, vs.FNNPolicy(env.spec, [8, 8], torch.tanh, featurize=False))
    assert two.n_params == (env.obs_space.flat_dim + 1) * 8 + 9 * 8 + 9


def test_population_param_grad_without_a_population_raises():
    e = object.__new__(vs.VecSimEnv)
    with pytest.raises(vs.ValueErr, match="set_policy_population"):
        e.population_param_grad(4, None)


# ------------------------------------------------------------------------------------------------------ the partition
def _random_table(rng):
    n_sets = int(rng.integers(1, 40))
    groups = [int(x) for x in rng.integers(-1, n_sets, size=int(rng.integers(1, 200)))]
    if rng.random() < 0.2:
        groups = [s if s < n_sets - 1 else -1 for s in groups]                            # the last set named by nobody
    return groups, n_sets, int(rng.integers(1, 60))


@pytest.mark.parametrize("waves, cap", [(1, 1024), (4, 512), (4, 7), (1, 3)])
def test_the_partition_covers_every_tile_of_a_named_set_exactly_once(waves, cap):
    rng = np.random.default_rng(11)
    for _ in range(300):
        groups, n_sets, t = _random_table(rng)
        ent, wg, seg = pvc.partition(groups, n_sets, t, waves, cap)
        assert (ent, wg, seg) == pvc.partition(list(groups), n_sets, t, waves, cap)       # the same inputs: the same partition
        assert [groups[g] for g in ent] == sorted(s for s in groups if s >= 0)            # by set ...
        assert all(a < b for a, b in zip(ent, ent[1:]) if groups[a] == groups[b])         # ... and stable by group
        assert len(wg) == sum(k for _, k in seg)
        for s, (w0, k) in enumerate(seg):
            cnt = sum(1 for x in groups if x == s)
            assert (k == 0) == (cnt == 0)                                                 # every named set is served, no other
            seen = np.zeros(cnt * t, dtype=int)
            for r in range(k):
                first, n_ent, rank, of = wg[w0 + r]
                assert (n_ent, rank, of) == (cnt, r, k) and {groups[g] for g in ent[first:first + n_ent]} == {s}  # one set per workgroup
                for t0, t1 in pvc.runs_of(wg[w0 + r], t, waves):
                    seen[t0:t1] += 1
            assert (seen == 1).all(), (groups, n_sets, t, s)
        want = sum(-(-sum(1 for x in groups if x == s) * t // waves) for s in range(n_sets))
        assert len(wg) <= max(min(want, cap) + n_sets, 0) and (want > cap or len(wg) == want)


@pytest.mark.parametrize("waves, cap", [(1, 1024), (4, 512), (4, 7), (1, 3)])
def test_the_mirror_is_the_library_partition(waves, cap):
    """pop_partition of vecsim.hip itself (vs_pop_partition, host only) gives the mirror's tables, entry for entry"""
    from simurlacra_amd import _lib as L

    rng = np.random.default_rng(12)
    for _ in range(200):
        groups, n_sets, t = _random_table(rng)
        assert pvc.library_partition(groups, n_sets, t, waves, cap) == pvc.partition(groups, n_sets, t, waves, cap), (groups, n_sets, t)
    groups = list(pvc.GROUPS_STD) + [-1, -1]
    assert pvc.library_partition(groups, 4, 33, waves, cap) == pvc.partition(groups, 4, 33, waves, cap)
    assert pvc.library_partition(list(range(1100)), 1100, 3, waves, cap) == pvc.partition(list(range(1100)), 1100, 3, waves, cap)
    lib, seg = L.load(), (C.c_int32 * 8)()
    g = (C.c_int32 * 3)(0, 5, -2)
    assert lib.vs_pop_partition(None, 3, 4, 2, 1, 8, seg, None, 0, None) == L.VS_ERR_ARG
    assert lib.vs_pop_partition(g, 3, 4, 2, 1, 8, seg, None, 0, None) == L.VS_ERR_ARG      # a set id outside the range
    assert lib.vs_pop_partition(g, 1, 4, 0, 1, 8, seg, None, 0, None) == L.VS_ERR_ARG
    assert lib.vs_pop_partition(g, 1, 4, 2, 1, 8, None, None, 0, None) == L.VS_ERR_ARG


def test_the_partition_by_hand():
    """the standard table at T = 33 on 256 compute units, and more sets than the cap"""
    groups = list(pvc.GROUPS_STD) + [-1, -1]                                              # ld = 512: two groups past n
    ent, wg, seg = pvc.partition(groups, 4, 33, 1, 1024)
    assert ent == [0, 4, 1, 5, 3] and seg == [(0, 66), (66, 66), (132, 33), (165, 0)]      # a wave per tile
    assert wg[0] == (0, 2, 0, 66) and wg[66] == (2, 2, 0, 66) and wg[-1] == (4, 1, 32, 33)
    assert pvc.lin_chain_of_set(groups, 4, 33, 0, 256) == 64 + 17 + 2 + 1
    _, wg, seg = pvc.partition(groups, 4, 33, 4, 512)
    assert seg == [(0, 17), (17, 17), (34, 9), (43, 0)]                                   # 66 tiles on four waves per workgroup
    assert pvc.fnn_chains_of_set(groups, 4, 33, 2, 256) == dict(acc=64, wg=3 + 2)
    _, wg, seg = pvc.partition(list(range(1100)), 1100, 3, 4, 512)                         # 1100 sets want one workgroup each: 1100 > 512
    assert len(wg) == 1100 and all(k == 1 for _, k in seg)
    _, wg, seg = pvc.partition([0] * 1000 + [1], 2, 40, 1, 1024)                           # unequal sets beyond the cap: shares by tiles
    assert seg == [(0, 1022), (1022, 1)]


# ------------------------------------------------------------------------------------------ the lanes of the rollout class
@pytest.mark.parametrize("M", [1, 64, 65])
def test_padding_lane_bookkeeping(M):
    from simurlacra_amd.diffsim import population_lanes

    P = 3
    src, real, lane_set = population_lanes(P, M)
    per = -(-M // 64) * 64
    assert len(src) == len(real) == len(lane_set) == P * per and per % 64 == 0
    assert int(real.sum()) == P * M and sorted(src[real]) == list(range(P * M))            # every rollout on exactly one real lane
    for s in range(P):
        block = slice(s * per, (s + 1) * per)
        assert (lane_set[block] == s).all()                                                # whole groups of 64 per member
        assert (src[block][:M] == s * M + np.arange(M)).all() and real[block][:M].all()
        assert (src[block][M:] == s * M + M - 1).all() and not real[block][M:].any()       # padding repeats the member's last rollout
