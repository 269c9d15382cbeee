"""
vs_step_policy with an open-loop policy (vs_set_policy_playback, k_rollout_play) and the on-device trajectory discrepancy
(vs_set_rollout_target): PlaybackPolicy / TimePolicy of upstream Pyrado, the samplers that take them, TrajectoryMatchSampler.

Shapes: 200 lanes (ld = 256: ragged), 3 recordings of a 40-row table with 37 / 40 / 12 steps, max_steps = 50, 45 steps per run
cut into launches of 7 + 1 + 32 + 5.  One lane map is a fixed scramble, the other run uses the modulo rule with an index offset.

The discrepancy bound: every term w e^2 is non-negative, so sequential fp32 summation of L * O terms of three roundings each
(e, w * e, the fma) is off by at most (L * O + 3) * 2^-24 relative; asserted with a factor 2 of margin against a float64 sum of
the lane's own recorded fp32 observations and the fp32 target, in the kernel's order.  The worst ratio is printed with -s.
"""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from derivative_cases import edge_states  # noqa: E402
from simurlacra_amd.policies import PlaybackPolicy, TimePolicy  # noqa: E402

FAMILIES = ["omo", "qq-su", "qcp-su", "qbb"]
KW = {"omo": dict(dt=0.02), "qq-su": dict(dt=0.004), "qcp-su": dict(dt=0.002), "qbb": dict(dt=0.01), "bob": dict(dt=0.01)}
ACT_MAX = {"omo": 30.0, "qq-su": 4.5, "qcp-su": 12.0, "qbb": 3.0, "bob": 20.0}  # rough sizes of the action boxes
N, N_REC, T_LEN, REC_LEN, MAX_STEPS, T, SPLITS = 200, 3, 40, np.array([37, 40, 12], dtype=np.int32), 50, 45, (7, 1, 32, 5)
LANE_REC = np.random.default_rng(5).integers(0, N_REC, N).astype(np.int32)  # a fixed scrambled map
OFFSET = 5


@pytest.fixture(scope="module")
def vs():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import simurlacra_amd

    return simurlacra_amd


def dev(x):
    return torch.as_tensor(np.asarray(x, dtype=np.float32)).cuda()


def table_of(vs, name, seed=0):
    """[N_REC, T_LEN, A]: normal draws around the size of the action box, so that actions fall inside and outside it; rows
    beyond a recording's length are NOT zero (the kernel's select has to make them so)"""
    A = vs.env_dims(name)["A"]
    return (ACT_MAX[name] * np.random.default_rng(seed).normal(size=(N_REC, T_LEN, A))).astype(np.float32)


def lane_recs(mode):
    return LANE_REC if mode == "map" else ((OFFSET + np.arange(N)) % N_REC).astype(np.int32)


def handle(vs, name, mode, table, max_steps=MAX_STEPS, auto_reset=False, rec_mode=2, seed=3, n=N):
    e = vs.VecSimEnv(name, n, max_steps=max_steps, **KW[name])
    e.set_index_offset(OFFSET if mode == "modulo" else 0)
    e.set_auto_reset(auto_reset, seed=11)
    e.reset(seed=seed)
    if table is not None:
        e.set_policy_playback(table, REC_LEN, LANE_REC if mode == "map" else None)
    e.set_record_mode(rec_mode)
    e.set_traj_capacity(T)
    return e


def run(e, splits, record=True):
    t = 0
    for k in splits:
        e.set_traj_offset(t)
        e.step_policy(k, record=record)
        t += k
    return e.traj(t) if record else None


def expected_actions(table, recs, curr_step):
    """table row curr_step of every lane's recording, exactly 0 from rec_len on; curr_step [N]"""
    row = table[recs, np.minimum(curr_step, T_LEN - 1)]
    return np.where((curr_step < REC_LEN[recs])[:, None], row, np.float32(0))


# ------------------------------------------------------------------------------------------------ 1. actions and records
@pytest.mark.parametrize("mode,rec_mode", [("map", 2), ("modulo", 1)])
@pytest.mark.parametrize("name", FAMILIES)
def test_actions_records_and_the_step_kernel(vs, name, mode, rec_mode):
    L = vs._lib
    table, recs = table_of(vs, name), lane_recs(mode)
    fused = handle(vs, name, mode, table, rec_mode=rec_mode)
    tr = run(fused, SPLITS)
    ref = handle(vs, name, mode, None, rec_mode=rec_mode)
    alive = np.ones(N, dtype=bool)
    seen_inside = seen_outside = False
    for t in range(T):
        want = expected_actions(table, recs, np.full(N, t))
        assert np.array_equal(tr["act"][t][alive], want[alive]), (name, t)       # the table row, bit for bit
        assert not tr["act"][t][~alive].any()                                    # a frozen lane reads nothing
        assert not tr["act"][t][alive & (t >= REC_LEN[recs])].any()              # exactly 0 from rec_len on
        assert np.array_equal(ref.get(L.VS_OBS)[alive], tr["obs"][t][alive]), (name, t)
        if rec_mode == 2:
            assert np.array_equal(ref.get(L.VS_STATE)[alive], tr["state"][t][alive]), (name, t)
            if vs.env_dims(name)["H"]:
                assert np.array_equal(ref.get(L.VS_HIDDEN)[alive], tr["hidden"][t][alive]), (name, t)
            clipped = (tr["act_app"][t] != tr["act"][t]).any(axis=1)[alive]
            seen_inside |= bool((~clipped).any())
            seen_outside |= bool(clipped.any())
        ref.step(dev(tr["act"][t]))
        assert np.array_equal(ref.get(L.VS_REW)[alive], tr["rew"][t][alive]), (name, t)
        assert np.array_equal(ref.get(L.VS_DONE).astype(bool)[alive], tr["done"][t].astype(bool)[alive]), (name, t)
        alive &= ~tr["done"][t].astype(bool)
    if rec_mode == 2:
        assert seen_inside and seen_outside  # actions inside and outside the action box
    for which in (L.VS_STATE, L.VS_HIDDEN, L.VS_STEPCOUNT, L.VS_RETURNS):
        assert np.array_equal(ref.get(which)[alive], fused.get(which)[alive]), (name, which)
    assert fused.error_count() == 0
    # one uncut launch: the same bits
    whole = handle(vs, name, mode, table, rec_mode=rec_mode)
    tr_w = run(whole, (T,))
    assert set(tr_w) == set(tr)
    for k in tr:
        assert np.array_equal(tr_w[k], tr[k]), (name, k)
    for which in (L.VS_STATE, L.VS_OBS, L.VS_HIDDEN, L.VS_REW, L.VS_DONE, L.VS_STEPCOUNT, L.VS_RETURNS, L.VS_FAILED):
        assert np.array_equal(whole.get(which), fused.get(which)), (name, which)
    for e in (fused, ref, whole):
        e.close()


# ------------------------------------------------------------------------------------------------------- 2. auto-reset
@pytest.mark.parametrize("name,mode", [("qq-su", "map"), ("qbb", "modulo")])
def test_auto_reset_restarts_the_recording(vs, name, mode):
    table, recs = table_of(vs, name, seed=1), lane_recs(mode)
    e = handle(vs, name, mode, table, max_steps=16, auto_reset=True, rec_mode=1)
    tr = run(e, SPLITS)
    curr = np.zeros(N, dtype=np.int64)  # curr_step before recorded step t, rebuilt from the done bits
    restarts = 0
    for t in range(T):
        assert np.array_equal(tr["act"][t], expected_actions(table, recs, curr)), (name, t)
        done = tr["done"][t].astype(bool)
        restarts += int(done.sum())
        curr = np.where(done, 0, curr + 1)
    assert restarts >= 2 * N and curr.max() < 16  # every lane ran at least two episodes
    assert np.array_equal(e.get(vs._lib.VS_STEPCOUNT), curr)
    e.close()


# ------------------------------------------------------------------------------------------------------- 3. discrepancy
@pytest.mark.parametrize("name", ["qq-su", "qbb", "bob"])
def test_discrepancy(vs, name):
    L = vs._lib
    O = vs.env_dims(name)["O"]
    table = (0.3 * table_of(vs, name, seed=2)).astype(np.float32)
    nominal = vs.nominal_params(name)
    scaled = (1.1 * nominal).astype(np.float32)
    weights = np.linspace(0.5, 2.0, O).astype(np.float32)
    # ---- the target: the playback kernel itself, with records, under the scaled parameters
    gen = handle(vs, name, "map", table)
    init = edge_states(name, gen.get(L.VS_STATE), n_edge=20)  # lanes 0 .. 19 start at the edge of the state space and end early
    gen.set_params(np.tile(scaled, (N, 1)))
    gen.reset(init_state=init)
    tr_g = run(gen, (T,))
    len_g = gen.get(L.VS_STEPCOUNT)
    src = [int(np.flatnonzero((LANE_REC == r) & (len_g == T))[0]) for r in range(N_REC)]  # a lane per recording that ran through
    target = np.stack([tr_g["obs"][: T_LEN + 1, j] for j in src])  # [N_REC, T_LEN + 1, O]: row k = the observation after k steps
    gen.close()
    # ---- the lanes: every fourth one carries the target's parameters and initial state, the others the nominal parameters
    same = np.arange(N) % 4 == 0
    params = np.where(same[:, None], scaled, nominal).astype(np.float32)
    init_b = np.where(same[:, None], init[np.array(src)[LANE_REC]], init).astype(np.float32)

    def fresh(e):
        e.set_params(params)
        e.reset(init_state=init_b)

    e = handle(vs, name, "map", table)
    e.set_rollout_target(target, weights)
    fresh(e)
    assert not e.rollout_loss().any()
    tr = run(e, SPLITS)
    loss = e.rollout_loss().cpu().numpy().copy()
    steps = e.get(L.VS_STEPCOUNT)
    summed = np.minimum(steps, REC_LEN[LANE_REC])
    assert not loss[same].any()                     # the same parameters and initial state: exactly 0
    through, early = steps == T, steps < REC_LEN[LANE_REC]
    assert through[~same].any() and early[~same].any()  # both cases occur
    worst = 0.0
    for i in np.flatnonzero(~same):
        ref = 0.0
        for k in range(1, summed[i] + 1):  # an early lane's sum stops at its last step
            err = tr["obs"][k, i].astype(np.float64) - target[LANE_REC[i], k].astype(np.float64)
            for d in range(O):
                ref += float(weights[d]) * err[d] * err[d]
        bound = 2.0 * (summed[i] * O + 3) * 2.0 ** -24 * ref
        worst = max(worst, abs(float(loss[i]) - ref) / bound if bound > 0 else 0.0)
        assert abs(float(loss[i]) - ref) <= bound, (name, i, loss[i], ref, summed[i])
        assert ref > 0
    print(f"{name}: worst |loss - ref| / bound = {worst:.3f}; {int(through.sum())} lanes ran through, {int(early.sum())} ended early, "
          f"loss up to {loss.max():.3g}")
    # ---- records off, and one uncut launch with records: the same bits
    fresh(e)
    assert not e.rollout_loss().any()  # vs_reset zeroed the sums
    run(e, SPLITS, record=False)
    assert np.array_equal(e.rollout_loss().cpu().numpy(), loss)
    fresh(e)
    run(e, (T,))
    assert np.array_equal(e.rollout_loss().cpu().numpy(), loss)
    # ---- vs_reset with a mask zeroes only the masked lanes' sums
    mask = np.arange(N) % 3 == 0
    e.reset(mask=mask, seed=1)
    after = e.rollout_loss().cpu().numpy()
    assert not after[mask].any() and np.array_equal(after[~mask], loss[~mask]) and loss[mask & ~same].all()
    e.close()


# --------------------------------------------------------------------------------------------------------- 4. refusals
def test_refusals_leave_the_previous_policy_working(vs):
    L = vs._lib
    lib = L.load()
    name, n = "qq-su", 128
    table = table_of(vs, name, seed=3)
    e = vs.VecSimEnv(name, n, max_steps=MAX_STEPS, **KW[name])
    e.reset(seed=1)
    with pytest.raises(RuntimeError):
        e.step_policy(1)  # no policy yet
    lane_rec = (np.arange(n) % N_REC).astype(np.int32)
    e.set_policy_playback(table, REC_LEN, lane_rec)
    e.set_traj_capacity(8)

    def rollout():
        e.reset(seed=1)
        e.set_traj_offset(0)
        e.step_policy(6, record=True)
        tr = e.traj(6)
        return tr["act"].copy(), tr["obs"].copy()

    first = rollout()

    def still_there():
        now = rollout()
        assert np.array_equal(now[0], first[0]) and np.array_equal(now[1], first[1])

    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def play(tab, n_rec, t_len, rec_len=None, lanes=None):
        return lib.vs_set_policy_playback(e._h, ptr(tab), n_rec, t_len, ptr(rec_len), ptr(lanes))

    i32 = lambda *x: np.array(x, dtype=np.int32)
    bad_lane = lane_rec.copy()
    bad_lane[77] = N_REC
    neg_lane = lane_rec.copy()
    neg_lane[0] = -1
    for args in ((table, 0, T_LEN), (table, N_REC, 0), (table, N_REC, T_LEN, i32(37, 41, 12)), (table, N_REC, T_LEN, i32(-1, 40, 12)),
                 (table, N_REC, T_LEN, REC_LEN, bad_lane), (table, N_REC, T_LEN, None, neg_lane)):
        assert play(*args) == L.VS_ERR_ARG, args[1:3]
        still_there()
    with pytest.raises(vs.ValueErr):
        e.set_policy_playback(table, i32(37, 41, 12))
    # a wrapper pipeline on the handle: a state error at the setter and at the step
    e.set_act_pipeline(delay=1)
    assert play(table, N_REC, T_LEN) == L.VS_ERR_STATE
    with pytest.raises(RuntimeError, match=r"\(-3\)"):
        e.step_policy(1)
    e.set_act_pipeline(delay=0)
    still_there()
    # no population on a playback policy
    sets = np.zeros((1, 4), dtype=np.float32)
    assert lib.vs_set_policy_population(e._h, ptr(sets), 4, 1, ptr(np.zeros(n, dtype=np.int32))) == L.VS_ERR_STATE
    still_there()
    # the target: sizes of the playback policy, weights >= 0, no auto-reset
    O = vs.env_dims(name)["O"]
    tgt = np.zeros((N_REC, T_LEN + 1, O), dtype=np.float32)
    w = np.ones(O, dtype=np.float32)
    target = lambda n_rec, t_len, wts: lib.vs_set_rollout_target(e._h, ptr(tgt), n_rec, t_len, ptr(wts))
    assert target(N_REC + 1, T_LEN, w) == L.VS_ERR_ARG and target(N_REC, T_LEN - 1, w) == L.VS_ERR_ARG
    for bad in (-1.0, float("nan")):
        wb = w.copy()
        wb[2] = bad
        assert target(N_REC, T_LEN, wb) == L.VS_ERR_ARG
    assert not lib.vs_get(e._h, L.VS_ROLLOUT_LOSS)
    still_there()
    assert target(N_REC, T_LEN, None) == L.VS_OK and lib.vs_get(e._h, L.VS_ROLLOUT_LOSS)
    still_there()  # (a target changes no rollout)
    e.set_auto_reset(True, seed=2)
    with pytest.raises(RuntimeError, match=r"\(-3\)"):
        e.step_policy(1)
    e.set_auto_reset(False)
    # replacing the playback policy removes the target; another policy removes the playback policy, and the other way round
    e.set_policy_playback(table, REC_LEN, lane_rec)
    assert not lib.vs_get(e._h, L.VS_ROLLOUT_LOSS)
    with pytest.raises(vs.ValueErr):
        e.rollout_loss()
    e.set_policy_fnn(np.zeros(6 * 8 + 8 + 8 + 1), [8], "tanh")
    assert target(N_REC, T_LEN, w) == L.VS_ERR_STATE  # no playback policy on the handle
    e.step_policy(2)
    e.set_policy_playback(table, REC_LEN, lane_rec)
    still_there()
    e.set_policy_playback(None)
    with pytest.raises(RuntimeError):
        e.step_policy(1)
    e.close()
    d = vs.VecSimEnv("bob-d", 64, dt=0.01, max_steps=10)
    with pytest.raises(vs.ValueErr):
        d.set_policy_playback(np.zeros((1, 4, 1), dtype=np.float32))  # discrete actions
    d.close()


# ----------------------------------------------------------------------------------------------------------- 5. sampler
FIELDS = ("observations", "actions", "rewards", "states", "actions_applied")


def assert_same_rollouts(a, b):
    assert len(a) == len(b)
    for j, (x, y) in enumerate(zip(a, b)):
        assert len(x) == len(y), j
        for f in FIELDS:
            assert np.array_equal(np.asarray(getattr(x, f), dtype=np.float32), np.asarray(getattr(y, f), dtype=np.float32)), (j, f)


def test_sampler_replays_recordings_in_rollout_order(vs, monkeypatch):
    env = vs.QQubeSwingUpSim(dt=0.004, max_steps=30)
    rng = np.random.default_rng(7)
    recs = [(6.0 * rng.normal(size=(t, 1))).astype(np.float32) for t in (30, 17, 25)]
    policy = PlaybackPolicy(env.spec, recs)
    np.random.seed(2)
    inits = [env.init_space.sample_uniform() for _ in range(7)]
    calls = []
    orig = vs.VecSimEnv.set_policy_playback
    monkeypatch.setattr(vs.VecSimEnv, "set_policy_playback", lambda self, *a, **k: (calls.append(1), orig(self, *a, **k))[1])
    fused = vs.ParallelRolloutSampler(env, policy, 1, min_rollouts=7, seed=4)
    ros_f = fused.sample(init_states=inits)
    assert calls and len(ros_f) == 7
    calls.clear()
    loop = vs.ParallelRolloutSampler(env, policy, 1, min_rollouts=7, seed=4, fuse_policy=False)
    ros_l = loop.sample(init_states=inits)
    assert not calls
    assert_same_rollouts(ros_f, ros_l)
    small = vs.ParallelRolloutSampler(env, policy, 1, min_rollouts=7, seed=4, batch_lanes=4)
    assert_same_rollouts(ros_f, small.sample(init_states=inits))
    for j, ro in enumerate(ros_f):  # rollout j replays recording j % 3 ...
        rec = recs[j % 3]
        k = min(len(ro), len(rec))
        assert np.array_equal(ro.actions[:k], rec[:k]) and not np.asarray(ro.actions[k:]).any()
    assert policy.curr_rec == -1  # (the samplers left the policy object's own position alone)
    for j, ro in enumerate(ros_f):  # ... like rollout() of one env object with the same policy object, reset in sequence
        one = vs.rollout(env, policy, eval=True, reset_kwargs=dict(init_state=inits[j]))
        assert policy.curr_rec == j % 3
        assert_same_rollouts([ro], [one])
    # a wrapper pipeline keeps the policy usable: the recording step path
    calls.clear()
    delayed = vs.ParallelRolloutSampler(vs.ActDelayWrapper(env, delay=2), policy, 1, min_rollouts=7, seed=4)
    ros_d = delayed.sample(init_states=inits)
    assert not calls and len(ros_d) == 7
    k = min(len(ros_d[1]), 17)
    assert np.array_equal(ros_d[1].actions[:k], recs[1][:k])
    for s in (fused, loop, small, delayed):
        s.close()


def test_sampler_time_policy_fused_equals_unfused(vs, monkeypatch):
    env = vs.QQubeSwingUpSim(dt=0.004, max_steps=30)
    policy = TimePolicy(env.spec, lambda t: [3.0 * math.sin(60.0 * t)], env.dt)
    calls = []
    orig = vs.VecSimEnv.set_policy_playback
    monkeypatch.setattr(vs.VecSimEnv, "set_policy_playback", lambda self, *a, **k: (calls.append(1), orig(self, *a, **k))[1])
    fused = vs.ParallelRolloutSampler(env, policy, 1, min_rollouts=5, seed=9)
    ros_f = fused.sample()
    assert calls
    calls.clear()
    loop = vs.ParallelRolloutSampler(env, policy, 1, min_rollouts=5, seed=9, fuse_policy=False)
    ros_l = loop.sample()
    assert not calls
    assert_same_rollouts(ros_f, ros_l)
    tab = policy.tabulate(30).numpy()
    for ro in ros_f:
        assert np.array_equal(ro.actions, tab[: len(ro)])
    fused.close()
    loop.close()


# ------------------------------------------------------------------------------------------- 6. TrajectoryMatchSampler
def test_trajectory_match_sampler(vs):
    L = vs._lib
    env = vs.QQubeSwingUpSim(dt=0.004, max_steps=60)
    name, R, P = "qq-su", 3, 5
    rng = np.random.default_rng(11)
    lens = (40, 25, 33)
    acts = [(2.0 * rng.normal(size=(t, 1))).astype(np.float32) for t in lens]
    np.random.seed(3)
    inits = np.stack([env.init_space.sample_uniform() for _ in range(R)]).astype(np.float32)
    names = vs.param_names(name)
    nominal = vs.nominal_params(name)
    cands = [dict(), dict(mass_pend_pole=0.03, length_pend_pole=0.14), dict(mass_rot_pole=0.11),
             dict(motor_resistance=9.0, motor_back_emf=0.05), dict(damping_rot_pole=1e-3)]
    truth = 1
    mat = np.tile(nominal, (P, 1))
    for p, d in enumerate(cands):
        for k, val in d.items():
            mat[p, names.index(k)] = np.float32(val)
    # ---- the recorded observations: the playback kernel under the true candidate
    act_tab = np.zeros((R, max(lens), 1), dtype=np.float32)
    for r, a in enumerate(acts):
        act_tab[r, : len(a)] = a
    g = vs.VecSimEnv(name, R, dt=0.004, max_steps=60)
    g.set_params(np.tile(mat[truth], (R, 1)))
    g.reset(init_state=inits)
    g.set_policy_playback(act_tab, np.array(lens, dtype=np.int32), np.arange(R, dtype=np.int32))
    g.set_traj_capacity(max(lens) + 1)
    g.step_policy(max(lens) + 1, record=True)
    obs_g = g.traj(max(lens) + 1)["obs"]
    obs_recs = [obs_g[: lens[r] + 1, r] for r in range(R)]
    g.close()
    w = np.array([1.0, 1.0, 1.0, 1.0, 0.1, 0.1], dtype=np.float32)
    smp = vs.TrajectoryMatchSampler(env, acts, obs_recs, inits, obs_weights=w, batch_lanes=6, chunk=16)
    res = smp.evaluate(cands)
    assert tuple(res.loss.shape) == (P, R) and tuple(res.steps.shape) == (P, R) and res.loss.is_cuda
    loss = res.loss.cpu().numpy()
    assert np.array_equal(res.steps.cpu().numpy(), np.tile(np.array(lens), (P, 1)))
    # ---- the same through direct VecSimEnv calls: one handle of P * R lanes, one launch
    obs_tab = np.zeros((R, max(lens) + 1, 6), dtype=np.float32)
    for r, o in enumerate(obs_recs):
        obs_tab[r, : len(o)] = o
    d = vs.VecSimEnv(name, P * R, dt=0.004, max_steps=60)
    d.set_params(np.repeat(mat, R, axis=0))
    d.reset(init_state=np.tile(inits, (P, 1)))
    d.set_policy_playback(act_tab, np.array(lens, dtype=np.int32), np.tile(np.arange(R, dtype=np.int32), P))
    d.set_rollout_target(obs_tab, w)
    d.step_policy(max(lens), record=False)
    assert np.array_equal(d.rollout_loss().cpu().numpy().reshape(P, R), loss)
    d.close()
    # ---- the candidate that generated the target has loss 0 and is the argmin
    assert not loss[truth].any() and (loss[np.arange(P) != truth] > 0).all()
    mean = res.mean_loss().cpu().numpy()
    assert int(mean.argmin()) == truth and mean[truth] == 0.0
    np.testing.assert_allclose(mean, loss.sum(1) / sum(lens), rtol=1e-6)
    # the array form of the candidates
    res2 = smp.evaluate(mat[:, [names.index("mass_pend_pole"), names.index("length_pend_pole")]][:2],
                        names=["mass_pend_pole", "length_pend_pole"])
    assert np.array_equal(res2.loss.cpu().numpy(), loss[:2])
    smp.close()
    with pytest.raises(vs.ValueErr, match="ActDelayWrapper"):
        vs.TrajectoryMatchSampler(vs.ActDelayWrapper(env, delay=1), acts, obs_recs, inits)
    ok = vs.TrajectoryMatchSampler(vs.ActNormWrapper(env), acts, obs_recs, inits)
    assert ok.num_segments == R
    ok.close()
