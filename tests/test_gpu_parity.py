"""
GPU parity tests proper: the HIP path, called through the C-ABI (ctypes -> libvecsim.so), against
  (1) the committed golden vectors the reference produced (tests/golden/*.npz),
  (2) the oracle (oracle/cpu_ref.py, fp64) on identical seeded inputs,
  (3) size-independent properties at BASELINE.json's full sizes.

Tolerances (north_star: "done masks bit-exact, state trajectories within 1e-5 relative fp32"), set from what the kernels
achieve on the reference's golden step cases (scratch/r2_errors.py on MI355X; every test prints its worst case with -s):
  states  : |got - ref| <= 1e-5 |ref| + ATOL_FRAC * (half-width of the state box in that dimension), ATOL_FRAC = 1e-6
            (2e-6 for the oscillator); achieved: <= 6.6e-6 relative where |ref| > 1 % of the box, <= 9.6e-7 of the box overall
  rewards : |got - ref| <= 3e-5 |ref| (5e-5 for the two QQube tasks: exp of costs up to a few hundred); achieved <= 2.1e-5
  hidden  : qcp th_ddot 1e-4 relative + 5e-5 (achieved 3.1e-5 relative), qbb plate angles 2e-6
  done / failed masks : bit-exact wherever the fp64 next state is further than 1e-5 (relative) from a bound,
                        and ALWAYS bit-exact w.r.t. the kernel's own fp32 next state.
"""
import ctypes as C
import os

import numpy as np
import pytest

import step_jacobian_cases as sj
from oracle import cpu_ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ENVS = ["omo", "bob", "qq-su", "qcp-su", "qbb", "qq-st", "qcp-st", "pend", "bob-d"]
KW = {"omo": dict(dt=0.02, max_steps=300), "bob": dict(dt=0.01, max_steps=500), "qq-su": dict(dt=0.004, max_steps=4000),
      "qcp-su": dict(dt=0.002, max_steps=8000), "qbb": dict(dt=0.01, max_steps=500),
      "qq-st": dict(dt=0.01, max_steps=500), "qcp-st": dict(dt=0.01, max_steps=300),
      "pend": dict(dt=0.02, max_steps=400, init_state=np.array([0.1, 0.2])), "bob-d": dict(dt=0.01, max_steps=500)}
RTOL_S, ATOL_S = 1e-5, 2e-6  # (ATOL_S: absolute floor of the secondary checks on O(1) quantities)
RTOL_R_ANY = 5e-5  # the loosest per-family reward tolerance, for the tests that are not per family
ATOL_FRAC = {"omo": 2e-6}  # fraction of the state box's half-width; default 1e-6
RTOL_R = {"qq-su": 5e-5, "qq-st": 5e-5}  # default 3e-5
ATOL_R = 1e-12
WORST = {}  # family -> worst observed (state error / tolerance, reward relative error): printed by the tests


@pytest.fixture(scope="module")
def vs():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import simurlacra_amd

    return simurlacra_amd

# the families that also run the three-role shapes of k_rollout_ws (E::WS_G3: a generator wave beside the physics and the
# reward wave); pinning those shapes for another family falls back to the two-role shape of the same workgroup size
G3_FAMILIES = {"qq-su", "qq-st", "omo", "pend", "qcp-su", "bob", "bob-d", "qbb"}


def ws_variants(name):
    base = ("k_rollout_ws", "k_rollout_ws64")
    return base + (("k_rollout_ws64g", "k_rollout_ws256g") if name in G3_FAMILIES else ())



def load(golden_dir, kind, name):
    return np.load(os.path.join(golden_dir, f"{kind}_{name.replace('-', '_')}.npz"))


def f32(x):
    return np.asarray(x, dtype=np.float32)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(f32(x))).cuda()


def assert_state_close(ref, got, exp, params):
    """|got - exp| <= 1e-5 |exp| + ATOL_FRAC * (half-width of the state space in that dimension)"""
    _, shi, _, _ = ref.bounds(np.asarray(params, dtype=np.float64))
    tol = RTOL_S * np.abs(exp) + ATOL_FRAC.get(ref.name, 1e-6) * np.abs(shi)
    err = np.abs(np.asarray(got, dtype=np.float64) - exp)
    w = WORST.setdefault(ref.name, [0.0, 0.0])
    w[0] = max(w[0], float((err / tol).max()))
    bad = err > tol
    assert not bad.any(), f"{bad.sum()} state elements out of tolerance, worst {err[bad].max()} (x{(err / tol).max():.2f} the bound)"


def assert_rew_close(name, got, exp):
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    big = np.abs(exp) > 1e-30
    if big.any():
        w = WORST.setdefault(name, [0.0, 0.0])
        w[1] = max(w[1], float((np.abs(got - exp)[big] / np.abs(exp)[big]).max()))
    np.testing.assert_allclose(got, exp, rtol=RTOL_R.get(name, 3e-5), atol=ATOL_R)


def bound_margin(ref, nstate, params):
    slo, shi, _, _ = ref.bounds(params)
    scale = np.maximum(np.abs(shi), 1e-12)
    return np.minimum(np.abs(nstate - slo), np.abs(nstate - shi)) / scale


def check_step(env, L, ref, params, state, hidden, act, curr_step, exp, yielded=None, ref32=None):
    """exp: dict with state/obs/rew/done(/hidden) from the reference or the oracle (fp64)"""
    assert_state_close(ref, env.get(L.VS_STATE), exp["state"], params)
    # observe(): tight against the oracle's observe of the kernel's OWN next state (tests the trig), and against the
    # reference within what the state tolerance allows (an angle of 4 pi known to 1e-5 relative moves its sine by 1e-4)
    own = ref.observe(env.get(L.VS_STATE).astype(np.float64))
    np.testing.assert_allclose(env.get(L.VS_OBS), own, rtol=1e-6, atol=5e-7)
    np.testing.assert_allclose(env.get(L.VS_OBS), exp["obs"], rtol=RTOL_S, atol=1e-5)
    assert_rew_close(ref.name, env.get(L.VS_REW), exp["rew"])
    if ref.H:
        np.testing.assert_allclose(env.get(L.VS_HIDDEN), exp["hidden"], rtol=1e-4, atol=5e-5 if ref.name.startswith("qcp") else 2e-6)
    print(f"[{ref.name}] worst so far: state error {WORST[ref.name][0]:.2f} x its bound, reward {WORST[ref.name][1]:.1e} relative")
    got_done = env.get(L.VS_DONE).astype(bool)
    margin = bound_margin(ref, exp["state"], params).min(axis=1)
    far = margin > 1e-5
    assert np.array_equal(got_done[far], np.asarray(exp["done"], dtype=bool)[far])
    assert (~far).sum() <= max(2, 0.01 * far.size)
    # bit-exact w.r.t. the kernel's own fp32 state: done == any(s' < lo32 | s' > hi32) | timeout
    slo, shi, _, _ = ref.bounds(f32(env.get(L.VS_PARAMS)).astype(np.float64))
    s32 = env.get(L.VS_STATE)
    ref32 = ref32 or cpu_ref.make_ref(ref.name, ref.dt, ref.max_steps, dtype=np.float32)
    lo32, hi32 = ref32.bounds(env.get(L.VS_PARAMS))[:2]
    failed = ((s32 < lo32) | (s32 > hi32)).any(axis=1)
    timeout = (np.asarray(curr_step) + 1) >= ref.max_steps
    assert np.array_equal(env.get(L.VS_FAILED).astype(bool), failed)
    assert np.array_equal(got_done, failed | timeout)
    assert np.array_equal(env.get(L.VS_STEPCOUNT), np.asarray(curr_step) + 1)


def setup_lanes(env, L, params, state, hidden, curr_step):
    env.set_params(f32(params))
    env.reset(init_state=f32(state))  # full-state shape -> copied verbatim
    if hidden.shape[1]:
        env.put(L.VS_HIDDEN, f32(hidden))
    env.put(L.VS_STEPCOUNT, np.asarray(curr_step, dtype=np.int32))


@pytest.mark.parametrize("name", ENVS)
def test_step_golden_cases(vs, golden_dir, name):
    """single-step cases the reference produced, pushed through vs_set_params / vs_reset / vs_step"""
    L = vs._lib
    g = load(golden_dir, "step", name)
    n = g["state"].shape[0]
    env = vs.VecSimEnv(name, n, **KW[name])
    ref = cpu_ref.make_ref(name, **KW[name])
    setup_lanes(env, L, g["params"], g["state"], g["hidden"], g["curr_step"])
    env.step(dev(g["act"]))
    exp = dict(state=g["nstate"], obs=g["obs"], rew=g["rew"], done=g["done"], hidden=g["nhidden"])
    check_step(env, L, ref, g["params"], g["state"], g["hidden"], g["act"], g["curr_step"], exp)
    assert env.error_count() == 0
    env.close()


@pytest.mark.parametrize("name", ENVS)
def test_step_along_golden_trajectories(vs, golden_dir, name):
    """every (state_t, act_t) of the reference's trajectories as one lane: one-step parity on naturally reached states"""
    L = vs._lib
    g = load(golden_dir, "traj", name)
    ref = cpu_ref.make_ref(name, **KW[name])
    idx = [(i, t) for i in range(g["params"].shape[0]) for t in range(int(g["length"][i]))
           if not g["done"][i, :t].any()]  # steps after the first done carry the once-only final-reward flag
    ii, tt = np.array(idx).T
    env = vs.VecSimEnv(name, len(idx), **KW[name])
    setup_lanes(env, L, g["params"][ii], g["state"][ii, tt], g["hidden"][ii, tt], tt)
    env.step(dev(g["act"][ii, tt]))
    exp = dict(state=g["state"][ii, tt + 1], obs=g["obs"][ii, tt], rew=g["rew"][ii, tt], done=g["done"][ii, tt],
               hidden=g["hidden"][ii, tt + 1])
    check_step(env, L, ref, g["params"][ii], None, None, None, tt, exp)
    env.close()


@pytest.mark.parametrize("name", ENVS)
def test_closed_loop_short_horizon(vs, golden_dir, name):
    """reset -> 30 steps on the device without host intervention vs the reference trajectory (chaos-limited tolerance)"""
    L = vs._lib
    g = load(golden_dir, "traj", name)
    ref = cpu_ref.make_ref(name, **KW[name])
    n = g["params"].shape[0]
    env = vs.VecSimEnv(name, n, **KW[name])
    env.set_params(f32(g["params"]))
    env.reset(init_state=f32(g["init"]))
    np.testing.assert_allclose(env.get(L.VS_STATE), g["state"][:, 0], rtol=RTOL_S, atol=ATOL_S)
    if ref.H:
        np.testing.assert_allclose(env.get(L.VS_HIDDEN), g["hidden"][:, 0], rtol=0, atol=5e-6)
    T = int(min(30, g["length"].min()))
    for t in range(T):
        env.step(dev(g["act"][:, t]))
        np.testing.assert_allclose(env.get(L.VS_REW), g["rew"][:, t], rtol=5e-3, atol=1e-9)
    np.testing.assert_allclose(env.get(L.VS_STATE), g["state"][:, T], rtol=2e-4, atol=2e-5)
    assert np.array_equal(env.get(L.VS_STEPCOUNT), np.full(n, T))
    env.close()


def test_omo_final_reward_once_and_stepping_after_done(vs, golden_dir):
    """rollout(stop_on_done=False): the failure malus is paid once (final_reward.py:130-135); golden OMO trajectories
    keep stepping after done"""
    L = vs._lib
    g = load(golden_dir, "traj", "omo")
    n = g["params"].shape[0]
    env = vs.VecSimEnv("omo", n, **KW["omo"])
    env.set_params(f32(g["params"]))
    env.reset(init_state=f32(g["init"]))
    Lmin = int(g["length"].min())
    saw_malus = False
    for t in range(Lmin):
        env.put(L.VS_STATE, f32(g["state"][:, t]))  # follow the reference states, keep the device's episode flags
        env.step(dev(g["act"][:, t]))
        np.testing.assert_allclose(env.get(L.VS_REW), g["rew"][:, t], rtol=RTOL_R_ANY, atol=1e-6)
        assert np.array_equal(env.get(L.VS_DONE).astype(bool), g["done"][:, t])
        saw_malus |= bool((g["rew"][:, t] < -900).any())
    assert saw_malus
    env.close()


@pytest.mark.parametrize("name", ENVS)
def test_reset_golden_cases(vs, golden_dir, name):
    L = vs._lib
    g = load(golden_dir, "reset", name)
    ref = cpu_ref.make_ref(name, **KW[name])
    for full in (False, True):
        sel = np.where(g["full"] == full)[0]
        env = vs.VecSimEnv(name, len(sel), **KW[name])
        env.set_params(f32(g["params"][sel]))
        init = g["init"][sel] if full else g["init"][sel][:, :ref.I]
        env.reset(init_state=f32(init))
        np.testing.assert_allclose(env.get(L.VS_STATE), g["state"][sel], rtol=1e-6, atol=1e-7)
        obs = env.get(L.VS_OBS)
        exp_obs = ref.observe(g["state"][sel])  # QCartPoleSim.reset returns the state (Q5); the device buffer holds observe()
        np.testing.assert_allclose(obs, exp_obs, rtol=RTOL_S, atol=ATOL_S)
        if ref.H:
            np.testing.assert_allclose(env.get(L.VS_HIDDEN), g["hidden"][sel], rtol=0, atol=5e-6)
        assert (env.get(L.VS_STEPCOUNT) == 0).all() and not env.get(L.VS_DONE).any()
        # derived constants: bounds and c_max per env (Q11) -- checked through their effect below and directly here
        if name in ("bob", "qbb", "bob-d"):
            K = env.get(L.VS_CONSTS)
            cmax_col = {"bob": 8, "qbb": 16, "bob-d": 8}[name]
            np.testing.assert_allclose(K[:, cmax_col], g["c_max"][sel], rtol=2e-6)
        env.close()


@pytest.mark.parametrize("name", ENVS)
def test_oracle_parity_seeded_batch(vs, name):
    """4096 seeded lanes (config-2 size), randomised params, random states/actions: HIP vs the fp64 oracle on the
    SAME fp32-rounded inputs"""
    L = vs._lib
    n = 4096
    rng = np.random.default_rng(42)
    ref = cpu_ref.make_ref(name, **KW[name])
    params = ref.nominal_params(n)
    params *= 1 + 0.15 * rng.standard_normal(params.shape) * (params != 0)
    for j, pn in enumerate(ref.param_names):
        if pn.startswith("voltage_thold") and name != "qbb":  # noqa: E501
            params[:, j] = np.where("neg" in pn, -1, 1) * rng.uniform(0, 0.4, n)
        if pn.startswith("offset") or pn == "ang_offset":
            params[:, j] = rng.uniform(-0.05, 0.05, n)
    params = f32(params).astype(np.float64)
    slo, shi, alo, ahi = ref.bounds(params)
    mid, half = 0.5 * (slo + shi), 0.5 * (shi - slo)
    state = f32(mid + rng.uniform(-1, 1, slo.shape) * half * np.where(rng.random(slo.shape) < 0.03, 1.001, 0.98)).astype(np.float64)
    hidden = f32(rng.uniform(-1, 1, (n, ref.H)) * (100 if name.startswith("qcp") else 0.3)).astype(np.float64)
    act = f32(rng.uniform(-1.4, 1.4, alo.shape) * ahi).astype(np.float64)
    curr = rng.integers(0, KW[name]["max_steps"], n)
    curr[::17] = KW[name]["max_steps"] - 1
    env = vs.VecSimEnv(name, n, **KW[name])
    setup_lanes(env, L, params, state, hidden, curr)
    env.step(dev(act))
    exp = ref.step(state, hidden, act, params, curr)
    check_step(env, L, ref, params, state, hidden, act, curr, exp)
    env.close()


def test_nan_action_sets_error_flag(vs):
    """the reference raises pyrado.ValueErr on NaN (box.py:142-146); the kernel sets a sticky per-env flag instead"""
    L = vs._lib
    env = vs.VecSimEnv("qq-su", 300, **KW["qq-su"])
    act = np.zeros((300, 1), dtype=np.float32)
    act[[3, 77, 299]] = np.nan
    env.step(dev(act))
    flags = env.get(L.VS_ERRFLAG)
    assert flags.sum() == 3 and flags[[3, 77, 299]].all()
    assert env.error_count() == 3
    with pytest.raises(vs.ValueErr):
        env.raise_on_error()
    env.step(dev(np.zeros((300, 1))))
    assert env.error_count() == 3  # sticky until reset
    env.reset()
    assert env.error_count() == 0
    env.close()


@pytest.mark.parametrize("name", ENVS)
def test_init_space_sampling(vs, name):
    """vs_reset(init_state=NULL): device-side init_space.sample_uniform; test_init_spaces of the reference
    (Pyrado/tests/test_environments.py:140-148): samples lie in the init space, states in the state space"""
    L = vs._lib
    n = 20000
    env = vs.VecSimEnv(name, n, **KW[name])
    ref = cpu_ref.make_ref(name, **KW[name])
    params = ref.nominal_params(n)
    env.reset(seed=5)
    s = env.get(L.VS_STATE).astype(np.float64)
    slo, shi, _, _ = ref.bounds(params)
    assert ((s >= slo) & (s <= shi)).all()
    eps = 1e-6
    if name in ("bob", "bob-d"):
        lo0, hi0 = ref.init_bounds(params, 0)
        lo1, hi1 = ref.init_bounds(params, 1)
        in0 = ((s >= lo0 - eps) & (s <= hi0 + eps)).all(axis=1)
        in1 = ((s >= lo1 - eps) & (s <= hi1 + eps)).all(axis=1)
        assert (in0 ^ in1).all() and 0.45 < in0.mean() < 0.55
    elif name == "qbb":
        lo, hi = ref.init_bounds(params)
        r = np.hypot(s[:, 2], s[:, 3])
        assert (r >= lo[:, 0] - eps).all() and (r <= hi[:, 0] + eps).all()
        phi = np.arctan2(s[:, 3], s[:, 2])
        assert abs(phi.mean()) < 0.06 and abs(phi.std() - np.pi / np.sqrt(3)) < 0.05
        assert (np.abs(s[:, 6:]) <= 0.025 + eps).all() and (s[:, [0, 1, 4, 5]] == 0).all()
    else:
        lo, hi = ref.init_bounds(params)
        assert ((s >= lo - eps) & (s <= hi + eps)).all()
        span = (hi - lo)[0]
        ok = span > 0
        assert (np.abs(s.mean(axis=0) - ((lo + hi) / 2)[0])[ok] < 0.03 * span[ok]).all()
        assert (np.abs(s.std(axis=0)[ok] - span[ok] / np.sqrt(12)) < 0.03 * span[ok]).all()
    # same seed -> same states; another seed -> different ones; test_reset (test_environments.py:192-214)
    env.reset(seed=5)
    assert np.array_equal(env.get(L.VS_STATE), f32(s))
    env.reset(seed=6)
    assert np.array_equal(env.get(L.VS_STATE), f32(s)) == (name == "pend")  # SingularStateSpace: always the same state
    env.close()


@pytest.mark.parametrize("name", ENVS)
def test_domain_randomization_on_device(vs, golden_dir, name):
    """vs_sample_params with the reference's default randomizer table: moments, clipping, untouched params, and the
    derived constants follow (checked by stepping against the oracle with the sampled params)"""
    import json

    L = vs._lib
    tab = json.load(open(os.path.join(golden_dir, "randomizers.json")))[name]
    specs = [(r["name"], "normal" if r["kind"] == "NormalDomainParam" else "uniform", r["mean"], r["spread"],
              r["clip_lo"], r["clip_up"]) for r in tab["randomizer"]]
    n = 50000
    env = vs.VecSimEnv(name, n, **KW[name])
    ref = cpu_ref.make_ref(name, **KW[name])
    env.sample_params(specs, seed=11)
    P = env.get(L.VS_PARAMS).astype(np.float64)
    nominal = ref.nominal_params(1)[0]
    touched = set()
    for (pn, kind, mean, spread, lo, hi) in specs:
        col = P[:, ref.param_names.index(pn)]
        touched.add(pn)
        assert (col >= np.float32(lo)).all() and (col <= np.float32(hi)).all()
        if spread == 0:
            continue
        clipped = ((col <= np.float32(lo)) | (col >= np.float32(hi))).mean()
        if clipped < 1e-3:
            assert abs(col.mean() - mean) < 0.02 * spread + 1e-12
            std = spread if kind == "normal" else spread / np.sqrt(3)
            assert abs(col.std() - std) < 0.02 * std
        if kind == "uniform":
            assert col.min() >= mean - spread - 1e-6 * abs(mean) - 1e-9 and col.max() <= mean + spread + 1e-6 * abs(mean) + 1e-9
    for j, pn in enumerate(ref.param_names):
        if pn not in touched:
            assert (P[:, j] == np.float32(nominal[j])).all()
    # different lanes got different draws; same seed reproduces
    assert np.unique(P[:, ref.param_names.index(specs[0][0])]).size > 0.99 * n
    env2 = vs.VecSimEnv(name, n, **KW[name])
    env2.sample_params(specs, seed=11)
    assert np.array_equal(env2.get(L.VS_PARAMS), env.get(L.VS_PARAMS))
    env2.close()
    # constants follow the sampled params
    rng = np.random.default_rng(1)
    slo, shi, alo, ahi = ref.bounds(P)
    state = f32(0.5 * (slo + shi) + rng.uniform(-0.9, 0.9, slo.shape) * 0.5 * (shi - slo)).astype(np.float64)
    hidden = np.zeros((n, ref.H))
    act = f32(rng.uniform(-1.2, 1.2, alo.shape) * ahi).astype(np.float64)
    env.reset(init_state=f32(state))
    if ref.H:
        env.put(L.VS_HIDDEN, f32(hidden))
    env.step(dev(act))
    exp = ref.step(state, hidden, act, P, np.zeros(n, dtype=np.int64))
    assert_state_close(ref, env.get(L.VS_STATE), exp["state"], P)
    np.testing.assert_allclose(env.get(L.VS_REW), exp["rew"], rtol=RTOL_R_ANY, atol=ATOL_R)
    env.close()


@pytest.mark.parametrize("name", ["omo", "bob", "qbb", "bob-d"])
def test_random_rollout_kernel_with_auto_reset(vs, name):
    """vs_step_random (k fused steps, on-device uniform policy, auto-reset) recorded and replayed
    through the oracle lane by lane; completed-episode returns/lengths (ballot-compacted) must match the records"""
    import json

    L = vs._lib
    n, T = 512, 700 if name == "omo" else 520
    kw = dict(KW[name])
    env = vs.VecSimEnv(name, n, **kw)
    ref = cpu_ref.make_ref(name, **kw)
    env.set_auto_reset(True, seed=3)
    env.set_episode_log(True)
    env.reset(seed=9)
    env.step_random(T, seed=21, record=True)
    tr = env.traj(T)
    obs, act, rew, done = tr["obs"].astype(np.float64), tr["act"].astype(np.float64), tr["rew"], tr["done"].astype(bool)
    params = ref.nominal_params(n)
    _, _, alo, ahi = ref.bounds(params)
    assert (act >= alo[None] - 1e-6).all() and (act <= ahi[None] + 1e-6).all()
    if name == "bob-d":  # DiscreteSpace.sample_uniform: the three torques, a third each
        vals, counts = np.unique(act, return_counts=True)
        np.testing.assert_allclose(vals, [alo[0, 0], 0.0, ahi[0, 0]], rtol=1e-6, atol=1e-6)
        assert (np.abs(counts / act.size - 1 / 3) < 0.01).all()
    else:
        assert abs(act.mean()) < 0.02 * ahi.max() and abs(act.std() - (ahi - alo).mean() / np.sqrt(12)) < 0.02 * ahi.max()
    # replay: obs == state for these envs (qbb: the hidden plate angles are re-derived by carrying them along)
    steps = np.zeros(n, dtype=np.int64)
    hidden = ref.reset(params, obs[0], init_is_full_state=True)["hidden"]
    ret = np.zeros(n)
    ep_ret, ep_len = [], []
    for t in range(T - 1):
        out = ref.step(obs[t], hidden, act[t], params, steps)
        np.testing.assert_allclose(rew[t], out["rew"], rtol=RTOL_R_ANY, atol=1e-6 if name == "omo" else ATOL_R)  # noqa: E501
        margin = bound_margin(ref, out["state"], params).min(axis=1)
        far = margin > 1e-5
        assert np.array_equal(done[t][far], out["done"][far])
        cont = ~done[t]
        np.testing.assert_allclose(obs[t + 1][cont], out["state"][cont], rtol=RTOL_S, atol=ATOL_S)
        ret += rew[t]
        steps = steps + 1
        for i in np.where(done[t])[0]:
            ep_ret.append(ret[i])
            ep_len.append(steps[i])
        ret[done[t]] = 0
        steps[done[t]] = 0
        hidden = out["hidden"]
        if done[t].any():  # fresh lanes: new init state from the init space, hidden re-initialised
            fresh = ref.reset(params[done[t]], obs[t + 1][done[t]], init_is_full_state=True)
            hidden[done[t]] = fresh["hidden"]
    cnt, rsum, lsum = env.episode_stats()
    r, ln, ix = env.episodes()
    # the per-env accumulators (no atomics) and the ballot-compacted log describe the same episodes
    assert cnt.sum() == len(r) and lsum.sum() == ln.sum()
    np.testing.assert_allclose(rsum.sum(dtype=np.float64), r.sum(dtype=np.float64), rtol=1e-5)
    assert np.array_equal(np.bincount(ix, minlength=n), cnt)
    # every episode that ended before the last step is in the device's episode buffer
    assert len(r) >= len(ep_ret) > n // 2
    got = sorted(zip(ln.tolist(), np.round(r, 3).tolist()))
    exp = sorted(zip([int(x) for x in ep_len], np.round(np.asarray(ep_ret, dtype=np.float32), 3).tolist()))
    assert len(got) - len(exp) == int(done[T - 1].sum())
    matched = sum(1 for e in exp if any(abs(e[1] - g_[1]) <= 2e-3 * max(1, abs(e[1])) for g_ in got if g_[0] == e[0]))
    assert matched == len(exp)
    env.close()


@pytest.mark.parametrize("auto_reset", [False, True])
@pytest.mark.parametrize("name", ["qq-su", "qcp-su", "bob", "qcp-st", "pend", "bob-d"])
def test_rollout_kernel_equals_step_kernel(vs, name, auto_reset):
    """k fused steps == k single-step launches fed with the recorded actions: bit-exact.  Without auto-reset a lane
    that finished freezes in the fused kernel (rollout() stops at done) while vs_step keeps stepping, so lanes are
    compared up to their first done; with auto-reset both kernels draw the same fresh episodes (same Philox counters)."""
    L = vs._lib
    n, T = 2048, 64
    kw = dict(KW[name])
    if name in ("qq-su", "pend"):
        kw["max_steps"] = 40  # time-outs inside the window
    a = vs.VecSimEnv(name, n, **kw)
    b = vs.VecSimEnv(name, n, **kw)
    for e in (a, b):
        e.set_auto_reset(auto_reset, seed=17)
        e.set_episode_log(True)
        e.reset(seed=1)
    assert np.array_equal(a.get(L.VS_STATE), b.get(L.VS_STATE))
    a.step_random(T, seed=4, record=True)
    tr = a.traj(T)
    alive = np.ones(n, dtype=bool)
    for t in range(T):
        assert np.array_equal(b.get(L.VS_OBS)[alive], tr["obs"][t][alive])
        b.step(dev(tr["act"][t]))
        assert np.array_equal(b.get(L.VS_REW)[alive], tr["rew"][t][alive])
        assert np.array_equal(b.get(L.VS_DONE).astype(bool)[alive], tr["done"][t].astype(bool)[alive])
        if not auto_reset:
            alive &= ~tr["done"][t].astype(bool)
    assert tr["done"].any() and (auto_reset or not alive.all())
    for which in (L.VS_STATE, L.VS_OBS, L.VS_HIDDEN, L.VS_STEPCOUNT, L.VS_RETURNS):
        assert np.array_equal(a.get(which)[alive], b.get(which)[alive])
    if auto_reset:
        ra, la, ia = a.episodes()
        rb, lb, ib = b.episodes()
        assert len(ra) == len(rb) > 0
        assert sorted(zip(ia.tolist(), la.tolist(), ra.tolist())) == sorted(zip(ib.tolist(), lb.tolist(), rb.tolist()))
        for x, y in zip(a.episode_stats(), b.episode_stats()):
            assert np.array_equal(x, y)
    a.close()
    b.close()


def test_full_size_properties_qq_65536(vs):
    """BASELINE metric config: 65 536 QQubeSwingUpSim envs.  Size-independent properties: determinism, lane independence
    (env i in a batch of 65 536 == env i in a batch of 4 096), broadcast-constant kernel == per-env-constant kernel"""
    L = vs._lib
    n, m = 65536, 4096
    big = vs.VecSimEnv("qq-su", n, **KW["qq-su"])
    big2 = vs.VecSimEnv("qq-su", n, **KW["qq-su"])
    small = vs.VecSimEnv("qq-su", m, **KW["qq-su"])
    ref = cpu_ref.make_ref("qq-su", **KW["qq-su"])
    big2.set_params(np.tile(vs.nominal_params("qq-su"), (n, 1)))  # per-env constants, same values
    rng = np.random.default_rng(7)
    lo, hi = ref.init_bounds(ref.nominal_params(n))
    init = f32(rng.uniform(lo, hi))
    for e, k in ((big, n), (big2, n), (small, m)):
        e.reset(init_state=init[:k])
    for t in range(50):
        act = f32(rng.uniform(-5, 5, (n, 1)))
        for e, k in ((big, n), (big2, n), (small, m)):
            e.step(dev(act[:k]))
    sb = big.get(L.VS_STATE)
    assert np.array_equal(sb, big2.get(L.VS_STATE))
    assert np.array_equal(sb[:m], small.get(L.VS_STATE))
    assert np.array_equal(big.get(L.VS_RETURNS)[:m], small.get(L.VS_RETURNS))
    assert np.isfinite(sb).all() and big.error_count() == 0
    # spot-check 512 lanes of the big batch against the oracle for the last step
    prev = big.get(L.VS_STATE)[:512].astype(np.float64)
    act = f32(rng.uniform(-5, 5, (n, 1)))
    big.step(dev(act))
    exp = ref.step(prev, np.zeros((512, 0)), act[:512].astype(np.float64), ref.nominal_params(512), np.full(512, 50))
    np.testing.assert_allclose(big.get(L.VS_STATE)[:512], exp["state"], rtol=RTOL_S, atol=ATOL_S)
    for e in (big, big2, small):
        e.close()


def test_full_size_qcp_65536_live_dr(vs, golden_dir):
    """BASELINE config 3: QCartPoleSwingUpSim + DomainRandWrapperLive over the first 7 default-randomizer params,
    65 536 envs: params are redrawn at every (auto-)reset, stay inside their clip range, constants stay consistent"""
    import json

    L = vs._lib
    tab = json.load(open(os.path.join(golden_dir, "randomizers.json")))["qcp-su"]["randomizer"][:7]
    specs = [(r["name"], "normal" if r["kind"] == "NormalDomainParam" else "uniform", r["mean"], r["spread"],
              r["clip_lo"], r["clip_up"]) for r in tab]
    assert [s[0] for s in specs] == ["gravity_const", "cart_mass", "pole_mass", "rail_length", "pole_length",
                                     "motor_efficiency", "gear_efficiency"]
    n = 65536
    env = vs.VecSimEnv("qcp-su", n, **KW["qcp-su"])
    ref = cpu_ref.make_ref("qcp-su", **KW["qcp-su"])
    env.set_randomizer(specs)
    env.set_auto_reset(True, seed=2)
    env.set_episode_log(True)
    env.reset(seed=1)
    p0 = env.get(L.VS_PARAMS)
    assert np.unique(p0[:, 0]).size > 0.9 * n  # every env drew its own gravity at reset
    env.step_random(400, seed=8)
    r, ln, ix = env.episodes()
    assert len(r) > 1000  # wild init + random actions: many carts hit the rail end
    p1 = env.get(L.VS_PARAMS)
    changed = (p1[:, 0] != p0[:, 0])
    assert np.array_equal(np.unique(ix), np.where(changed)[0])  # exactly the envs that finished an episode were redrawn
    for (pn, kind, mean, spread, lo, hi) in specs:
        col = p1[:, ref.param_names.index(pn)]
        assert (col >= np.float32(lo)).all() and (col <= np.float32(hi)).all()
    # constants consistent with the (redrawn) params: one checked step on 2048 lanes
    sel = slice(0, 2048)
    P = p1[sel].astype(np.float64)
    s = env.get(L.VS_STATE)[sel].astype(np.float64)
    h = env.get(L.VS_HIDDEN)[sel].astype(np.float64)
    c = env.get(L.VS_STEPCOUNT)[sel]
    env.set_auto_reset(False)
    env.set_randomizer([])
    act = f32(np.random.default_rng(0).uniform(-6, 6, (n, 1)))
    env.step(dev(act))
    exp = ref.step(s, h, act[sel].astype(np.float64), P, c)
    np.testing.assert_allclose(env.get(L.VS_STATE)[sel], exp["state"], rtol=RTOL_S, atol=ATOL_S)
    np.testing.assert_allclose(env.get(L.VS_REW)[sel], exp["rew"], rtol=RTOL_R_ANY, atol=ATOL_R)
    env.close()


def test_edge_sizes(vs):
    """N = 1 (reference-sized), ragged N (not a multiple of the 64-lane wave / 256-thread block)"""
    L = vs._lib
    ref = cpu_ref.make_ref("bob", **KW["bob"])
    for n in (1, 63, 257, 1000):
        env = vs.VecSimEnv("bob", n, **KW["bob"])
        rng = np.random.default_rng(n)
        state = f32(rng.uniform(-0.5, 0.5, (n, 4)))
        act = f32(rng.uniform(-10, 10, (n, 1)))
        env.reset(init_state=state)
        env.step(dev(act))
        exp = ref.step(state.astype(np.float64), np.zeros((n, 0)), act.astype(np.float64), ref.nominal_params(n),
                       np.zeros(n, dtype=np.int64))
        np.testing.assert_allclose(env.get(L.VS_STATE), exp["state"], rtol=RTOL_S, atol=ATOL_S)
        env.step_random(3, seed=1)
        assert env.get(L.VS_STEPCOUNT).tolist() == [4] * n
        env.close()


def test_fast_sincos_accuracy_through_observe(vs):
    """the sincos of the hot path (vecsim_envs.h: sincos_fast) against fp64 over |angle| <= 100 rad, read back through
    QQubeSim.observe.  Since the end of round 3 it is the hardware's v_sin_f32 / v_cos_f32 behind an exact two-term reduction:
    3.5e-7 maximum absolute error measured here (3.8e-7 in scratch/ubench/hw_sincos_err.hip), where the polynomial form it
    replaced reached 9e-8 and this bound stood at 2e-7 -- a deliberate trade: three ulp of a value near 1,
    a thirtieth of the 1e-5 relative the trajectories are held to, for 10 % on the headline and 37 % on BASELINE config 4."""
    L = vs._lib
    n = 1 << 16
    env = vs.VecSimEnv("qq-su", n, **KW["qq-su"])
    rng = np.random.default_rng(0)
    s = np.zeros((n, 4), dtype=np.float32)
    s[:, 0] = rng.uniform(-100, 100, n)
    s[:, 1] = np.concatenate([rng.uniform(-13, 13, n // 2), np.linspace(-4 * np.pi, 4 * np.pi, n // 2)])
    s[:16, 0] = np.arange(16) * np.float32(np.pi / 4)  # multiples of pi/4: quadrant boundaries
    env.reset(init_state=s)
    o = env.get(L.VS_OBS).astype(np.float64)
    s64 = s.astype(np.float64)
    exp = np.stack([np.sin(s64[:, 0]), np.cos(s64[:, 0]), np.sin(s64[:, 1]), np.cos(s64[:, 1])], axis=1)
    err = np.abs(o[:, :4] - exp).max()
    assert err < 4.0e-7, err
    env.close()


@pytest.mark.parametrize("auto_reset", [False, True])
def test_mixed_batch_equals_separate_handles(vs, auto_reset):
    """BASELINE config 5 (QQube + QCartPole + BallOnBeam in one launch, lanes sorted by type): the mixed launch runs the
    same per-type bodies, so every member ends bit-identical to a stand-alone handle stepped on its own"""
    L = vs._lib
    names, sizes = ["qq-su", "qcp-su", "bob"], [3000, 1111, 2048]  # ragged: segments end inside a workgroup
    mixed_members = [vs.VecSimEnv(nm, n, **KW[nm]) for nm, n in zip(names, sizes)]
    solo = [vs.VecSimEnv(nm, n, **KW[nm]) for nm, n in zip(names, sizes)]
    mixed = vs.MixedVecSimEnv(mixed_members)
    off = 0
    for a, b in zip(mixed_members, solo):
        b.set_index_offset(off)
        off += b.n_envs
        for e in (a, b):
            e.set_params(np.tile(vs.nominal_params(e.name), (e.n_envs, 1)))
            e.set_auto_reset(auto_reset, seed=21)
            e.set_record_mode(2 if auto_reset else 1)  # the mixed launch records in the members' mode
            e.reset(seed=5)
    mixed.step_random(150, seed=9, record=True)
    for b in solo:
        b.step_random(150, seed=9, record=True)
    for a, b in zip(mixed_members, solo):
        for which in (L.VS_STATE, L.VS_OBS, L.VS_HIDDEN, L.VS_REW, L.VS_DONE, L.VS_STEPCOUNT, L.VS_RETURNS, L.VS_EPSTAT_COUNT):
            assert np.array_equal(a.get(which), b.get(which)), (a.name, which)
        ta, tb = a.traj(150), b.traj(150)
        for k in ta:
            assert np.array_equal(ta[k], tb[k])
    # policy-in-the-loop variant: one launch for three action tensors
    rng = np.random.default_rng(3)
    acts = [dev(rng.uniform(-5, 5, (n, 1))) for n in sizes]
    mixed.step(acts)
    for b, act in zip(solo, acts):
        b.step(act)
    for a, b in zip(mixed_members, solo):
        assert np.array_equal(a.get(L.VS_STATE), b.get(L.VS_STATE)) and np.array_equal(a.get(L.VS_REW), b.get(L.VS_REW))
    # and against the oracle for the QCartPole segment
    ref = cpu_ref.make_ref("qcp-su", **KW["qcp-su"])
    m = mixed_members[1]
    s0, h0, c0 = m.get(L.VS_STATE).astype(np.float64), m.get(L.VS_HIDDEN).astype(np.float64), m.get(L.VS_STEPCOUNT)
    act = f32(rng.uniform(-7, 7, (sizes[1], 1)))
    m.set_auto_reset(False)
    mixed_members[0].set_auto_reset(False)
    mixed_members[2].set_auto_reset(False)
    mixed.step([dev(np.zeros((sizes[0], 1))), dev(act), dev(np.zeros((sizes[2], 1)))])
    exp = ref.step(s0, h0, act.astype(np.float64), ref.nominal_params(sizes[1]).astype(np.float32).astype(np.float64), c0)
    assert_state_close(ref, m.get(L.VS_STATE), exp["state"], ref.nominal_params(sizes[1]))
    mixed.close()


def test_full_size_qbb_config4_rank_shard(vs):
    """BASELINE config 4: QBallBalancerSim, 262 144 envs over 8 GPUs = 32 768 per rank.  One rank's shard on this GPU:
    polar init on the device, fused rollout with auto-reset, per-env return accumulators (what the RCCL gather reads),
    shard invariance (global lane index) and a spot check of the last step against the oracle"""
    L = vs._lib
    n, rank = 32768, 3
    env = vs.VecSimEnv("qbb", n, **KW["qbb"])
    ref = cpu_ref.make_ref("qbb", **KW["qbb"])
    env.set_index_offset(rank * n)
    env.set_auto_reset(True, seed=1)
    env.reset(seed=2)
    env.step_random(600, seed=3)
    cnt, rs, ls = env.episode_stats()
    assert cnt.min() >= 1 and cnt.sum() == (ls > 0).sum() + (cnt - 1).sum()  # every env finished at least one episode (<= 500 steps)
    assert (ls <= 500 * cnt).all() and np.isfinite(rs).all() and env.error_count() == 0
    mean_ret = rs.sum(dtype=np.float64) / cnt.sum()
    assert 0.0 < mean_ret < 500.0
    # the same global lanes inside a differently cut handle behave identically
    sub = vs.VecSimEnv("qbb", 4096, **KW["qbb"])
    sub.set_index_offset(rank * n + 8192)
    sub.set_auto_reset(True, seed=1)
    sub.reset(seed=2)
    sub.step_random(600, seed=3)
    assert np.array_equal(sub.get(L.VS_STATE), env.get(L.VS_STATE)[8192:8192 + 4096])
    assert np.array_equal(sub.get(L.VS_EPSTAT_RETSUM), rs[8192:8192 + 4096])
    # last step against the oracle on 1024 lanes
    env.set_auto_reset(False)
    s0 = env.get(L.VS_STATE)[:1024].astype(np.float64)
    h0 = env.get(L.VS_HIDDEN)[:1024].astype(np.float64)
    c0 = env.get(L.VS_STEPCOUNT)[:1024]
    act = f32(np.random.default_rng(0).uniform(-3.5, 3.5, (n, 2)))
    env.step(dev(act))
    P = ref.nominal_params(1024).astype(np.float32).astype(np.float64)
    exp = ref.step(s0, h0, act[:1024].astype(np.float64), P, c0)
    assert_state_close(ref, env.get(L.VS_STATE)[:1024], exp["state"], P)
    np.testing.assert_allclose(env.get(L.VS_REW)[:1024], exp["rew"], rtol=RTOL_R_ANY, atol=ATOL_R)
    np.testing.assert_allclose(env.get(L.VS_HIDDEN)[:1024], exp["hidden"], rtol=1e-4, atol=2e-6)


def test_full_size_mixed_config5_rank_shard(vs):
    """BASELINE config 5: 1 M mixed envs over 8 GPUs = 131 072 per rank, a third each of QQube / QCartPole / BallOnBeam,
    lanes sorted by type, one launch.  Determinism and agreement with stand-alone handles at full per-rank size."""
    L = vs._lib
    per = 43520  # 3 * 43 520 = 130 560 <= 131 072, multiple of 256
    names = ["qq-su", "qcp-su", "bob"]

    def build():
        ms = [vs.VecSimEnv(nm, per, **KW[nm]) for nm in names]
        mx = vs.MixedVecSimEnv(ms)
        for m in ms:
            m.set_auto_reset(True, seed=7)
            m.reset(seed=8)
        return ms, mx

    a_m, a = build()
    b_m, b = build()
    a.step_random(120, seed=5)
    b.step_random(60, seed=5)
    b.step_random(60, seed=5)  # chunking does not matter: the action stream is keyed by the absolute step index
    for x, y in zip(a_m, b_m):
        assert np.array_equal(x.get(L.VS_STATE), y.get(L.VS_STATE))
        assert np.array_equal(x.get(L.VS_EPSTAT_COUNT), y.get(L.VS_EPSTAT_COUNT))
        assert x.error_count() == 0
    solo = vs.VecSimEnv("qcp-su", per, **KW["qcp-su"])
    solo.set_index_offset(per)
    solo.set_auto_reset(True, seed=7)
    solo.reset(seed=8)
    solo.step_random(120, seed=5)
    assert np.array_equal(solo.get(L.VS_STATE), a_m[1].get(L.VS_STATE))
    assert a_m[2].get(L.VS_EPSTAT_COUNT).sum() > per // 2  # ball-on-beam episodes are short under a random policy


def setup_jac_lanes(env, L, c):
    """the lanes of a step_jacobian_cases.Case on a handle; in the "uniform" layout without set_params: the handle keeps the uniform
    constants of its constructor, and k_step_jac<E, true> runs"""
    if c.set_params:
        env.set_params(c.params)
    env.reset(init_state=c.state)  # full-state shape -> copied verbatim
    if c.hidden.shape[1]:
        env.put(L.VS_HIDDEN, c.hidden)
    env.put(L.VS_STEPCOUNT, c.curr.astype(np.int32))
    assert np.array_equal(env.get(L.VS_PARAMS), c.params)  # (the oracle's parameters are the device's, in every layout)


def jac_at_full_pitch(env, L):
    """the three Jacobian buffers of the last vs_step_jac as the device holds them, padding lanes included: [rows (S + A), ld] each"""
    S, A, O = (env.dims[k] for k in "SAO")
    out = {}
    for key, which, rows in (("state", L.VS_JAC_STATE, S), ("rew", L.VS_JAC_REW, 1), ("obs", L.VS_JAC_OBS, O)):
        buf = np.empty((rows * (S + A), env.ld), dtype=np.float32)
        env._check(env._lib.vs_copy_to_host(env._h, which, buf.ctypes.data_as(C.c_void_p)), "vs_copy_to_host")
        out[key] = buf
    return out


VALUE_BUFFERS = ("VS_STATE", "VS_OBS", "VS_REW", "VS_DONE", "VS_HIDDEN", "VS_STEPCOUNT")


@pytest.mark.parametrize("name,layout", [pytest.param(name, layout, id=name if layout == "nominal" else f"{name}-{layout}")
                                         for layout in sj.LAYOUTS for name in ENVS])
def test_step_jacobians_against_finite_differences(vs, name, layout):
    """vs_step_jac (forward-mode differentiation of the step code in the kernel) against central finite differences of the
    fp64 oracle, position by position under the rule of step_jacobian_cases.py, in its three parameter layouts: not one bad entry,
    every entry of every live position being smooth on these draws, and exact zeros where the oracle has them; the step VALUES must
    equal vs_step bit for bit"""
    L = vs._lib
    assert sj.ENVS == ENVS
    c, o, rs = sj.case(name, layout), sj.oracle(name, layout), sj.rules(name, layout)
    ref, n = c.ref, c.n
    a = vs.VecSimEnv(name, n, **sj.KW[name])
    b = vs.VecSimEnv(name, n, **sj.KW[name])
    for e in (a, b):
        setup_jac_lanes(e, L, c)
    act = dev(np.array(c.act))  # (a copy: the case arrays are read-only)
    J = a.step_jac(act)
    b.step(act)
    for which in VALUE_BUFFERS:
        assert np.array_equal(a.get(getattr(L, which)), b.get(getattr(L, which))), which
    S, A, O = ref.S, ref.A, ref.O
    assert J["state"].shape == (n, S, S + A) and J["rew"].shape == (n, S + A) and J["obs"].shape == (n, O, S + A)
    checked, failures = 0, []
    for tag, r in zip(sj.ARRAYS, rs):
        got = J[tag].reshape(n, -1).astype(np.float64)
        assert np.isfinite(got).all(), tag
        bad, worst = sj.within(got, r)
        beyond = sj.ulps_beyond(got, r)
        print(f"[{name} {layout}] d {tag}: {bad} bad, worst ratio {worst.max():.3g} at position "
              f"{sj.position(worst.argmax(), S + A)}, {beyond.max():.3g} ulp of the row maximum beyond the relative terms")
        if bad:
            failures.append(f"{bad} bad; " + sj.report(name, layout, tag, worst, S + A))
        assert r.smooth[:, r.live].all() and r.smooth.mean() > 0.9, (tag, float(r.smooth.mean()))
        assert not got[:, r.exact].any(), (tag, "an exact-zero position is not 0.0")
        checked += int(sj.checked(r).sum())
    assert not failures, "\n".join(failures)
    # structure: clipped actions have zero action-gradient of the next state (of the 1.5 x lanes, n // 8, those whose draw lies above
    # 2 / 3 of the bound in every action dimension clip: more than 10 of 96, at least 3 of 18)
    if name != "bob-d":
        assert o.clipped.sum() > (10 if layout == "nominal" else 2) and np.abs(J["state"][o.clipped][:, :, S:]).max() == 0.0
    assert checked > 0.9 * n * (S + 1 + O) * (S + A)
    # the padding lanes n .. ld - 1 of the three buffers hold numbers (768 lanes fill their blocks, 150 do not)
    full = jac_at_full_pitch(a, L)
    assert a.ld >= n and (a.ld > n) == (layout != "nominal")
    for tag in sj.ARRAYS:
        assert full[tag].shape[1] == a.ld and np.isfinite(full[tag]).all(), tag
        assert np.array_equal(full[tag][:, :n].T, J[tag].reshape(n, -1)), tag
    # the lanes at curr = max_steps - 1 take the time-limit branch of done, under the same rule as the others (checked above:
    # every entry of theirs is smooth)
    assert np.array_equal(a.get(L.VS_DONE).astype(bool), o.done)
    if layout != "nominal":
        limit = slice(n - sj.N_LIMIT, n)
        assert o.done[limit].all() and not a.get(L.VS_FAILED)[limit].any() and o.done.sum() == sj.N_LIMIT
        assert (a.get(L.VS_STEPCOUNT)[limit] == sj.KW[name]["max_steps"]).all()
        assert all(sj.checked(r)[limit].all() for r in rs)
    if name == "omo":
        # a lane that has already yielded its final reward has the d r of one that has not: a third handle pays the malus first
        # (a step from outside the box), then steps from the case's lanes
        y = vs.VecSimEnv(name, n, **sj.KW[name])
        setup_jac_lanes(y, L, c)
        y.put(L.VS_STATE, (1.5 * ref.bounds(c.params.astype(np.float64))[1]).astype(np.float32))
        y.step(act)
        assert y.get(L.VS_FAILED).all() and (y.get(L.VS_REW) < -900).all()
        y.put(L.VS_STATE, c.state)
        y.put(L.VS_STEPCOUNT, c.curr.astype(np.int32))
        Jy = y.step_jac(act)
        for tag in sj.ARRAYS:
            assert np.array_equal(Jy[tag], J[tag]), tag
        assert np.array_equal(y.get(L.VS_REW), a.get(L.VS_REW))  # (no lane of the case fails: none has a malus to pay)
        y.close()
    with pytest.raises(RuntimeError):
        a.set_auto_reset(True)
        a.step_jac(act)
    a.close()
    b.close()


@pytest.mark.parametrize("name", ENVS)
def test_step_jacobians_uniform_constants_equal_per_lane_nominal(vs, name):
    """k_step_jac<E, true> (a handle that keeps its uniform constants) against k_step_jac<E, false> (the nominal parameters set per
    lane): the three Jacobians and the step values agree bit for bit, on the first 64 lanes of the "uniform" case"""
    L = vs._lib
    c = sj.case(name, "uniform")
    n = 64
    cut = c._replace(n=n, params=c.params[:n], state=c.state[:n], hidden=c.hidden[:n], act=c.act[:n], curr=c.curr[:n])
    uni = vs.VecSimEnv(name, n, **sj.KW[name])
    per = vs.VecSimEnv(name, n, **sj.KW[name])
    setup_jac_lanes(uni, L, cut)
    setup_jac_lanes(per, L, cut._replace(set_params=True))
    act = dev(np.array(cut.act))  # (a copy: the case arrays are read-only)
    Ju, Jp = uni.step_jac(act), per.step_jac(act)
    for tag in sj.ARRAYS:
        assert np.isfinite(Ju[tag]).all() and np.abs(Ju[tag]).max() > 0.0 and np.array_equal(Ju[tag], Jp[tag]), tag
    for which in VALUE_BUFFERS:
        assert np.array_equal(uni.get(getattr(L, which)), per.get(getattr(L, which))), which
    uni.close()
    per.close()


def test_maximum_size_batch_4m_lanes(vs):
    """a batch far beyond the caches (4 194 304 QQube envs, ~0.8 GB of per-env buffers, 0.5 GB per step of traffic):
    the first lanes behave exactly like the same lanes in a small handle; every lane advances; no error flags"""
    L = vs._lib
    n, m = 1 << 22, 4096
    big = vs.VecSimEnv("qq-su", n, **KW["qq-su"])
    small = vs.VecSimEnv("qq-su", m, **KW["qq-su"])
    for e in (big, small):
        e.set_params(np.tile(vs.nominal_params("qq-su"), (e.n_envs, 1)))
        e.set_auto_reset(True, seed=3)
        e.reset(seed=4)
        e.step_random(24, seed=5)
    act = torch.rand(n, 1, device="cuda") * 9 - 4.5
    big.step(act)
    small.step(act[:m].contiguous())
    assert np.array_equal(big.get(L.VS_STATE)[:m], small.get(L.VS_STATE))
    assert (big.get(L.VS_STEPCOUNT) == 25).all() and big.error_count() == 0
    tail = big.get(L.VS_STATE)[-m:]
    assert np.isfinite(tail).all() and np.abs(tail).max() > 0
    big.close()
    small.close()


def test_ctor_and_task_variants(vs, golden_dir):
    """constructor / task options of the reference classes pushed through vs_task_cfg: simple_dynamics, long, wild_init,
    task_args (state_des, Q, R), max_steps=inf, the short-pole stabilisation task (tests/golden/variants.npz)"""
    from test_oracle_golden import VARIANTS

    L = vs._lib
    g = np.load(os.path.join(golden_dir, "variants.npz"))
    for tag, (name, kw) in VARIANTS.items():
        n = g[f"{tag}__state"].shape[0]
        env = vs.VecSimEnv(name, n, **kw)
        ref = cpu_ref.make_ref(name, **kw)
        ref32 = cpu_ref.make_ref(name, dtype=np.float32, **kw)
        P = np.tile(g[f"{tag}__params"], (n, 1))
        np.testing.assert_allclose(env.get(L.VS_PARAMS)[0], g[f"{tag}__params"], rtol=1e-6, err_msg=tag)  # nominal set
        setup_lanes(env, L, P, g[f"{tag}__state"], g[f"{tag}__hidden"], g[f"{tag}__curr_step"])
        env.step(dev(g[f"{tag}__act"]))
        exp = {k: g[f"{tag}__{v}"] for k, v in dict(state="nstate", obs="obs", rew="rew", done="done", hidden="nhidden").items()}
        check_step(env, L, ref, P, None, None, None, g[f"{tag}__curr_step"], exp, ref32=ref32)
        if f"{tag}__init_lo" in g.files:  # the init space the ctor flags select (wild_init, long)
            env.reset(seed=5)
            s0 = env.get(L.VS_STATE).astype(np.float64)
            lo, hi = g[f"{tag}__init_lo"], g[f"{tag}__init_hi"]
            eps = 1e-6 * np.maximum(1.0, np.abs(hi))
            assert ((s0 >= lo - eps) & (s0 <= hi + eps)).all(), tag
        assert env.error_count() == 0
        env.close()


def test_bernoulli_rounded_and_1d_multivariate_params_on_device(vs):
    """vs_sample_params with the remaining DomainParam kinds (domain_parameter.py:206-311): Bernoulli(val_0, val_1, prob_1),
    roundint, MultivariateNormal of dimension 1; the live randomizer redraws them at auto-resets"""
    L = vs._lib
    n = 65536
    env = vs.VecSimEnv("omo", n, dt=0.02, max_steps=8)
    rz = vs.DomainRandomizer(
        vs.BernoulliDomainParam(name="mass", val_0=1.0, val_1=3.0, prob_1=0.3, clip_up=2.5),
        vs.NormalDomainParam(name="stiffness", mean=30.0, std=4.0, roundint=True),
        vs.MultivariateNormalDomainParam(name="damping", mean=[0.5], cov=[[0.04]], clip_lo=0.3))
    env.sample_params(rz.device_specs(), seed=21)
    P = env.get(L.VS_PARAMS).astype(np.float64)
    assert set(np.unique(P[:, 0])) == {1.0, 2.5}  # val_1 = 3 clipped to 2.5
    assert abs((P[:, 0] == 2.5).mean() - 0.3) < 0.01
    assert np.array_equal(P[:, 1], np.rint(P[:, 1])) and abs(P[:, 1].mean() - 30.0) < 0.1
    assert abs(P[:, 1].std() - np.sqrt(16.0 + 1.0 / 12.0)) < 0.1  # rounding adds the variance of U(-1/2, 1/2)
    free = P[:, 2] > np.float64(np.float32(0.3))
    assert (P[:, 2] >= np.float32(0.3)).all() and abs(free.mean() - 0.8413) < 0.01  # P(z > -1)
    assert abs(np.median(P[:, 2]) - 0.5) < 0.005
    # derived constants and spaces follow (act bound = stiffness)
    ref = cpu_ref.make_ref("omo", dt=0.02, max_steps=8)
    _, _, alo, ahi = ref.bounds(P)
    assert np.array_equal(ahi[:, 0], P[:, 1])
    # same seed -> same draw; objects are accepted in place of tuples
    env2 = vs.VecSimEnv("omo", n, dt=0.02, max_steps=8)
    env2.sample_params(rz.domain_params, seed=21)
    assert np.array_equal(env2.get(L.VS_PARAMS), env.get(L.VS_PARAMS))
    # live randomisation: every auto-reset redraws
    env.set_randomizer(rz.device_specs())
    env.set_auto_reset(True, seed=5)
    env.reset(seed=1)
    p0 = env.get(L.VS_PARAMS).copy()
    env.step_random(8, seed=2)  # every lane times out once
    p1 = env.get(L.VS_PARAMS)
    assert (env.episode_stats()[0] == 1).all()
    assert 0.3 < (p0[:, 0] != p1[:, 0]).mean() < 0.55  # 2 * 0.3 * 0.7 = 0.42 of the Bernoulli draws flip
    assert set(np.unique(p1[:, 0])) == {1.0, 2.5} and np.array_equal(p1[:, 1], np.rint(p1[:, 1]))
    with pytest.raises(vs.ValueErr):
        env.sample_params([("mass", "bernoulli", 1.0, 2.0, -np.inf, np.inf, 1.5, False)])
    with pytest.raises(vs.ValueErr):
        env.sample_params([("mass", "poisson", 1.0, 2.0, -np.inf, np.inf)])
    env.close()
    env2.close()


@pytest.mark.parametrize("auto_reset", [False, True])
@pytest.mark.parametrize("name", ["qq-su", "qcp-su", "bob", "omo", "qbb", "pend", "bob-d", "qq-st"])
def test_wave_specialised_rollout_kernel_equals_plain_kernel(vs, name, auto_reset):
    """k_rollout_ws (a physics wave + a reward/record wave per 64 envs, exchanging through LDS; for QQube, the oscillator and
    the pendulum also with a third, generator wave: actions a batch ahead, reset stock, first record plane) against k_rollout: records,
    final buffers, episode statistics and the episode log bit for bit; launches of 7, 1 and 30 steps (batches of 4 with a
    ragged tail), per-env and broadcast constants, n not a multiple of the 256-env workgroup"""
    L = vs._lib
    n = 1000
    kw = dict(KW[name])
    kw["max_steps"] = 25  # time-outs inside the window
    live_dr = {"qq-su": ("mass_pend_pole", 0.024), "qcp-su": ("pole_length", 0.16825), "qq-st": ("length_pend_pole", 0.129)}
    for per_env, mode in ((False, 1), (True, 2), ("live-dr", 1), ("live-dr", 2)):
        if per_env == "live-dr" and not (auto_reset and name in live_dr):
            continue
        trio = []
        for variant in ("k_rollout",) + ws_variants(name):
            e = vs.VecSimEnv(name, n, **kw)
            e.set_record_mode(mode)
            if per_env is True:
                e.set_params(np.tile(vs.nominal_params(name), (n, 1)))
            if per_env == "live-dr":  # parameters redrawn at every auto-reset inside the launches
                pname, nominal = live_dr[name]
                e.set_randomizer([(pname, "normal", nominal, nominal / 5, 1e-3, np.inf)])
            e.set_rollout_variant(variant)
            assert e.rollout_variant() == variant
            e.set_auto_reset(auto_reset, seed=17)
            e.set_episode_log(True)
            e.reset(seed=1)
            e.set_traj_capacity(38)
            t = 0
            for k in (7, 1, 30):
                e.set_traj_offset(t)
                e.step_random(k, seed=4, record=True)
                t += k
            e.set_traj_offset(0)
            e.step_random(5, seed=9, record=False)  # the variant without records (no observation in the message)
            trio.append(e)
        a = trio[0]
        ta = a.traj(38)
        assert set(ta) == ({"obs", "act", "rew", "done"} | ({"state", "act_app", "hidden"} if mode == 2 else set()))
        assert ta["done"].any()
        stats_a = a.episode_stats()
        ra, la, ia = a.episodes()  # (clears the accumulators)
        for b in trio[1:]:
            tb = b.traj(38)
            for key in ta:
                assert np.array_equal(ta[key], tb[key]), (name, key, b.rollout_variant())
            for which in (L.VS_STATE, L.VS_OBS, L.VS_HIDDEN, L.VS_STEPCOUNT, L.VS_RETURNS, L.VS_REW, L.VS_DONE, L.VS_FAILED,
                          L.VS_PARAMS, L.VS_CONSTS):
                assert np.array_equal(a.get(which), b.get(which)), (name, which)
            for x, y in zip(stats_a, b.episode_stats()):
                assert np.array_equal(x, y)
            assert stats_a[0].sum() > 0
            rb, lb, ib = b.episodes()
            assert sorted(zip(ia.tolist(), la.tolist(), ra.tolist())) == sorted(zip(ib.tolist(), lb.tolist(), rb.tolist()))
            assert b.error_count() == 0
        if per_env == "live-dr":
            assert len(np.unique(a.get(L.VS_PARAMS)[:, vs.param_names(name).index(live_dr[name][0])])) > n // 2
        assert len(ra) > 0 and a.error_count() == 0
        for e in trio:
            e.close()


@pytest.mark.parametrize("name", ["qq-su", "qcp-su", "qq-st"])
def test_live_randomizer_stock_equals_plain_kernel(vs, name):
    """DomainRandWrapperLive on the device with the reference's default randomizer (its first seven parameters: Normal and
    Uniform draws, clipped) in every shape of k_rollout_ws against k_rollout.  In the wave-specialised kernel a resetting lane
    takes the next episode's parameters and constants from the reset stock its reward / generator wave pre-draws into LDS, or
    -- a second reset before the refill: episodes of a few steps make that common here -- draws them itself; either way the
    parameters, constants, records and episode statistics are those of the plain kernel, bit for bit, across launches that
    start with an empty stock (1-, 9- and 64-step launches) and with a ragged last workgroup."""
    L = vs._lib
    n = 1000
    kw = dict(KW[name])
    kw["max_steps"] = 11  # a time-out every 11 steps: several resets per lane and launch, refills every 32 steps
    specs = vs.create_default_randomizer(vs.ENV_CLASSES[name](**KW[name])).device_specs()[:7]
    if name != "qcp-su":  # the QQube table is all Normal: make the stream mix one- and two-word draws here too
        specs[2] = (specs[2][0], "uniform") + tuple(specs[2][2:])
    assert {sp[1] for sp in specs} >= {"normal", "uniform"}
    envs = []
    for variant in ("k_rollout",) + ws_variants(name):
        e = vs.VecSimEnv(name, n, **kw)
        e.set_record_mode(2)
        e.set_params(np.tile(vs.nominal_params(name), (n, 1)))
        e.set_randomizer(specs)
        e.set_rollout_variant(variant)
        assert e.rollout_variant() == variant
        e.set_auto_reset(True, seed=23)
        e.reset(seed=5)
        e.set_traj_capacity(74)
        t = 0
        for k in (1, 9, 64):
            e.set_traj_offset(t)
            e.step_random(k, seed=6, record=True)
            t += k
        envs.append(e)
    a = envs[0]
    ta = a.traj(74)
    pa = a.get(L.VS_PARAMS)
    rnd = [vs.param_names(name).index(sp[0]) for sp in specs]
    assert all(len(np.unique(pa[:, k])) > n // 2 for k in rnd)          # every lane drew its own values ...
    fixed = [k for k in range(pa.shape[1]) if k not in rnd]
    assert np.array_equal(pa[:, fixed], np.tile(vs.nominal_params(name), (n, 1))[:, fixed].astype(np.float32))  # ... of those only
    assert a.episode_stats()[0].min() >= 5
    for b in envs[1:]:
        tb = b.traj(74)
        for key in ta:
            assert np.array_equal(ta[key], tb[key]), (name, key, b.rollout_variant())
        for which in (L.VS_STATE, L.VS_OBS, L.VS_HIDDEN, L.VS_STEPCOUNT, L.VS_RETURNS, L.VS_REW, L.VS_DONE, L.VS_FAILED,
                      L.VS_PARAMS, L.VS_CONSTS):
            assert np.array_equal(a.get(which), b.get(which)), (name, which, b.rollout_variant())
        for x, y in zip(a.episode_stats(), b.episode_stats()):
            assert np.array_equal(x, y)
        assert b.error_count() == 0
    for e in envs:
        e.close()


def test_step_jacobians_against_the_forks_autograd(vs, golden_dir):
    """vs_step_jac against tests/golden/jac_qcp_su.npz: d(s', r) / d(s, a) of QCartPoleSwingUpSim as the fork computes them
    with torch.autograd.grad through its step_diff_state (P/sampling/rollout.py:832-837, quanser_cartpole.py:257-431), float64,
    inside the region where that differentiable restatement and the NumPy step agree.  Forward-mode
    fp32 on the device: the tolerance is relative to the largest entry of a Jacobian row's scale."""
    L = vs._lib
    g = np.load(os.path.join(golden_dir, "jac_qcp_su.npz"))
    n = g["state"].shape[0]
    env = vs.VecSimEnv("qcp-su", n, **KW["qcp-su"])
    setup_lanes(env, L, g["params"], g["state"], g["hidden"], np.full(n, 10))
    J = env.step_jac(dev(g["act"]))
    ref = cpu_ref.make_ref("qcp-su", **KW["qcp-su"])
    assert_state_close(ref, env.get(L.VS_STATE), g["nstate"], g["params"])
    np.testing.assert_allclose(env.get(L.VS_REW), g["rew"], rtol=2e-5, atol=1e-9)
    js, jr = g["jac_state"], g["jac_rew"]
    # per output row: entries are compared relative to the row's largest magnitude (a row mixes 1.0 and 1e-5 entries)
    scale_s = np.abs(js).max(axis=2, keepdims=True)
    err_s = np.abs(J["state"] - js) / scale_s
    scale_r = np.maximum(np.abs(jr).max(axis=1, keepdims=True), 1e-12)
    err_r = np.abs(J["rew"] - jr) / scale_r
    print(f"jacobian vs fork autograd: max row-relative error state {err_s.max():.2e}, reward {err_r.max():.2e}")
    assert err_s.max() < 1e-6 and err_r.max() < 5e-6  # measured: 5.6e-8 / 7.0e-7
    # structure the fork's clamp / dead-zone masks imply: no action gradient where the action was clipped or swallowed
    clipped = np.abs(g["act"][:, 0]) > 6.0
    tn, tp = (list(g["param_names"]).index(k) for k in ("voltage_thold_neg", "voltage_thold_pos"))
    dead = (g["params"][:, tn] <= g["act"][:, 0]) & (g["act"][:, 0] <= g["params"][:, tp]) & (g["params"][:, tp] > 0)
    assert clipped.sum() >= 10 and dead.sum() >= 10
    assert np.abs(js[clipped | dead][:, :, 4]).max() == 0.0 and np.abs(J["state"][clipped | dead][:, :, 4]).max() == 0.0
    assert np.abs(J["rew"][~clipped, 4] - jr[~clipped, 4]).max() < 1e-6  # the reward sees the unclipped action
    env.close()


@pytest.mark.parametrize("mode", [1, 2])
def test_headline_launch_values_at_65536(vs, mode):
    """The exact launch bench.py times -- 65 536 QQubeSwingUpSim envs, per-env constants, auto-reset, every step recorded in
    record mode 1 (`mode` = 1: the very template instantiation of the timed region, k_rollout_ws<QQT<0>, false, true, 1, 4, 256,
    false, 3>) or 2, bench.py's default steps per launch, the records of consecutive launches ROTATING through three slots of the
    record buffer as in bench.py (four launches: the fourth overwrites the first slot), the three-role k_rollout_ws in 256-env
    workgroups (one per compute unit) -- checked for VALUES: records, done bits, final buffers and episode statistics equal the
    plain kernel's bit for bit (and every other shape's); mode 2: 512 lanes of the last recorded step are re-stepped by the fp64
    oracle and the record planes hold what rollout() keeps; mode 1: its [obs | act | rew] planes are the first planes of the
    oracle-checked mode-2 records of the same launches, bit for bit."""
    L = vs._lib
    import bench

    n, T, slots, launches = 65536, bench.DEFAULT_CHUNK, 3, 4

    def run(variant, rec_mode):
        e = vs.VecSimEnv("qq-su", n, **KW["qq-su"])
        e.set_params(np.tile(vs.nominal_params("qq-su"), (n, 1)))
        e.set_rollout_variant(variant)
        assert e.rollout_variant() == variant
        e.set_auto_reset(True, seed=1)
        e.reset(seed=2)
        e.set_record_mode(rec_mode)
        e.set_traj_capacity(slots * T)
        for l in range(launches):  # bench.py's run(): slot l % slots, the streams continue from launch to launch
            e.set_traj_offset((l % slots) * T)
            e.step_random(T, seed=3, record=True)
        return e

    auto = vs.VecSimEnv("qq-su", n, **KW["qq-su"])
    assert auto.rollout_variant() == "k_rollout_ws256g"  # what the automatic choice (and bench.py) launches at this size
    auto.close()
    a = run("k_rollout", mode)
    tt_a = a.traj_tensors(slots * T)
    for variant in ws_variants("qq-su"):
        b = run(variant, mode)
        tt_b = b.traj_tensors(slots * T)
        for key in ("rec", "done"):
            assert torch.equal(tt_a[key], tt_b[key]), (variant, key)
        for which in (L.VS_STATE, L.VS_OBS, L.VS_STEPCOUNT, L.VS_RETURNS, L.VS_REW, L.VS_DONE, L.VS_FAILED,
                      L.VS_EPSTAT_COUNT, L.VS_EPSTAT_RETSUM, L.VS_EPSTAT_LENSUM):
            assert np.array_equal(a.get(which), b.get(which)), (variant, which)
        assert b.error_count() == 0
        del tt_b
        b.close()
    assert int(tt_a["done"].sum()) > 100  # episodes ended (and restarted) inside the window
    if mode == 1:
        # the lean records are the leading planes of the full ones: the same launches in record mode 2 (the oracle-checked form)
        full = run("k_rollout_ws256g", 2)
        tt_f = full.traj_tensors(slots * T)
        for key in ("obs", "act", "rew", "done"):
            assert torch.equal(tt_a[key], tt_f[key]), key
        for which in (L.VS_STATE, L.VS_RETURNS, L.VS_EPSTAT_COUNT, L.VS_EPSTAT_RETSUM):
            assert np.array_equal(a.get(which), full.get(which)), which
        full.close()
        a.close()
        return
    # 512 lanes of the last recorded step (launch 4 wrote slot 0: rows 0 .. T-1) against the fp64 oracle: recorded state +
    # action -> reward, next state
    ref = cpu_ref.make_ref("qq-su", **KW["qq-su"])
    lanes = np.arange(0, n, n // 512)
    row = ((launches - 1) % slots) * T + T - 1
    last = {k: v[row][torch.from_numpy(lanes).cuda()].cpu().numpy().astype(np.float64) for k, v in tt_a.items()
            if k in ("state", "act", "rew", "obs", "act_app")}
    done_last = tt_a["done"][row].cpu().numpy().astype(bool)[lanes]
    P = ref.nominal_params(len(lanes)).astype(np.float32).astype(np.float64)
    out = ref.step(last["state"], np.zeros((len(lanes), 0)), last["act"], P, np.zeros(len(lanes), dtype=np.int64))
    np.testing.assert_allclose(last["rew"], out["rew"], rtol=2e-5, atol=1e-12)
    np.testing.assert_allclose(last["obs"], ref.observe(last["state"]), rtol=1e-6, atol=5e-7)
    np.testing.assert_array_equal(last["act_app"], np.clip(last["act"], -4.5, 4.5))
    keep = ~done_last  # lanes that did not reset: VS_STATE is the successor of the recorded state
    got_next = a.get(L.VS_STATE)[lanes].astype(np.float64)
    assert keep.sum() > 400
    assert_state_close(ref, got_next[keep], out["state"][keep], P[keep])
    a.close()


def test_config3_launch_values_at_65536(vs):
    """BASELINE config 3 as bench.py's `roofline.configs.config3` leg launches it -- 65 536 QCartPoleSwingUpSim envs, the first
    seven parameters of the reference's default randomizer (default_randomizers.py:322-342) redrawn at every reset
    (DomainRandWrapperLive), record mode 1, bench.py's steps per launch, records rotating through three slots -- in the
    automatic kernel (k_rollout_ws, three roles in 64-env workgroups: the generator wave keeps the reset stock with the pre-drawn
    parameters in LDS), in the two-role 64-env shape and in 256-env workgroups against the plain kernel: records, done bits, VS_PARAMS, VS_CONSTS, final buffers and episode statistics bit
    for bit.  (Values against the reference: the golden step / reset cases and the randomizer tables, at small n.)"""
    L = vs._lib
    import bench

    n, T, slots, launches = 65536, bench.DEFAULT_CHUNK, 3, 4
    kw = KW["qcp-su"]
    specs = vs.create_default_randomizer(vs.ENV_CLASSES["qcp-su"](**kw)).device_specs()[:7]
    assert [sp[0] for sp in specs] == ["gravity_const", "cart_mass", "pole_mass", "rail_length", "pole_length",
                                       "motor_efficiency", "gear_efficiency"]

    def run(variant):
        e = vs.VecSimEnv("qcp-su", n, **kw)
        e.set_params(np.tile(vs.nominal_params("qcp-su"), (n, 1)))
        e.set_randomizer(specs)
        if variant:
            e.set_rollout_variant(variant)
        e.set_auto_reset(True, seed=11)
        e.reset(seed=12)
        e.set_record_mode(1)
        e.set_traj_capacity(slots * T)
        for l in range(launches):
            e.set_traj_offset((l % slots) * T)
            e.step_random(T, seed=13, record=True)
        return e

    auto = run(None)
    assert auto.rollout_variant() == "k_rollout_ws64g"  # the automatic choice at this size under a live randomizer
    a = run("k_rollout")
    tt_a = a.traj_tensors(slots * T)
    cnt = a.episode_stats()[0]
    assert cnt.sum() > n // 4 and int(tt_a["done"].sum()) > 1000  # the randomised rail length ends many episodes early
    pa = a.get(L.VS_PARAMS)
    rnd = [vs.param_names("qcp-su").index(sp[0]) for sp in specs]
    reset_lanes = cnt > 0
    assert all(len(np.unique(pa[reset_lanes][:, k])) > reset_lanes.sum() // 2 for k in rnd)
    for b in (auto, run("k_rollout_ws64"), run("k_rollout_ws")):
        tt_b = b.traj_tensors(slots * T)
        for key in ("rec", "done"):
            assert torch.equal(tt_a[key], tt_b[key]), (b.rollout_variant(), key)
        for which in (L.VS_STATE, L.VS_OBS, L.VS_HIDDEN, L.VS_STEPCOUNT, L.VS_RETURNS, L.VS_REW, L.VS_DONE, L.VS_FAILED,
                      L.VS_PARAMS, L.VS_CONSTS, L.VS_EPSTAT_COUNT, L.VS_EPSTAT_RETSUM, L.VS_EPSTAT_LENSUM):
            assert np.array_equal(a.get(which), b.get(which)), (b.rollout_variant(), which)
        assert b.error_count() == 0
        del tt_b
        b.close()
    a.close()


def test_lean_step_is_the_step_without_the_bookkeeping(vs):
    """vs_set_lean_step: vs_step returns what SimPyEnv.step returns (obs, rew, done: pysim/base.py:217-241) -- state,
    observation, reward, done flag and step counter bit for bit those of the default kernel, with and without auto-reset;
    VS_RETURNS and VS_FAILED are left alone, episodes still count (with a return of 0)"""
    L = vs._lib
    n = 3000
    for ar in (False, True):
        pair = []
        for lean in (False, True):
            e = vs.VecSimEnv("qq-st", n, dt=0.01, max_steps=20)
            e.set_params(np.tile(vs.nominal_params("qq-st"), (n, 1)))
            e.set_auto_reset(ar, seed=3)
            e.reset(seed=4)
            e.set_lean_step(lean)
            torch.manual_seed(0)
            for _ in range(45):
                e.step((torch.rand(n, 1, device="cuda") * 2 - 1) * 6.0)
            pair.append(e)
        a, b = pair
        for which in (L.VS_STATE, L.VS_OBS, L.VS_REW, L.VS_DONE, L.VS_STEPCOUNT, L.VS_EPSTAT_COUNT, L.VS_EPSTAT_LENSUM):
            assert np.array_equal(a.get(which), b.get(which)), (ar, which)
        assert np.abs(a.get(L.VS_RETURNS)).max() > 0 and np.abs(b.get(L.VS_RETURNS)).max() == 0  # untouched since the reset
        assert (b.get(L.VS_FAILED) == 0).all() and (b.get(L.VS_EPSTAT_RETSUM) == 0).all()
        if ar:
            assert a.episode_stats()[0].sum() > n and np.abs(a.get(L.VS_EPSTAT_RETSUM)).max() > 0
        a.close(), b.close()


def test_rollout_variant_selection(vs):
    """automatic choice (Launch<E>::variant): the wave-specialised kernel while k_rollout would leave SIMDs with a single
    wave -- in 64-env workgroups up to 128 envs per compute unit (every family) and between 256 and 384, in the family's
    faster shape at 256 -- and never with a wrapper pipeline, the state-and-time dependent final reward, or live
    randomisation of constants its reward wave reads"""
    e = vs.VecSimEnv("qq-su", 65536, **KW["qq-su"])
    assert e.rollout_variant() == "k_rollout_ws256g"  # three waves per 64 envs, one workgroup per compute unit
    e.set_randomizer([("gravity_const", "normal", 9.81, 1.0, 1e-4, np.inf)])
    assert e.rollout_variant() == "k_rollout_ws64g"  # (a redraw stalls one trio of waves instead of four)
    e.set_rollout_variant("k_rollout_ws")
    assert e.rollout_variant() == "k_rollout_ws"
    e.set_rollout_variant(None)
    e.set_randomizer([])
    q = vs.VecSimEnv("qcp-su", 4096, **KW["qcp-su"])
    q.set_randomizer([("gravity_const", "normal", 9.81, 1.0, 1e-4, np.inf)])
    assert q.rollout_variant() == "k_rollout_ws64g"  # BASELINE config 3 at small size
    q.close()
    b = vs.VecSimEnv("bob", 4096, **KW["bob"])
    b.set_randomizer([("gravity_const", "normal", 9.81, 1.0, 1e-4, np.inf)])
    assert b.rollout_variant() == "k_rollout"  # act bound and c_max follow the redrawn parameters
    b.close()
    e.set_act_pipeline(delay=1)
    assert e.rollout_variant() == "k_rollout"
    e.set_rollout_variant("k_rollout_ws")
    assert e.rollout_variant() == "k_rollout"  # the pipeline still wins over the pin
    e.set_act_pipeline(delay=0)
    assert e.rollout_variant() == "k_rollout_ws"  # the pin holds again
    e.set_rollout_variant(None)
    assert e.rollout_variant() == "k_rollout_ws256g"
    e.close()
    for n_big, expect in ((65537, "k_rollout_ws64"), (81920, "k_rollout_ws64"), (82176, "k_rollout_ws64g"), (98304, "k_rollout_ws64g"),
                          (98305, "k_rollout"), (131072, "k_rollout")):
        big = vs.VecSimEnv("qq-su", n_big, **KW["qq-su"])
        assert big.rollout_variant() == expect, n_big
        big.close()
    for name, n, expect in (("omo", 4096, "k_rollout_ws64g"), ("qbb", 4096, "k_rollout_ws64g"), ("qbb", 32768, "k_rollout_ws64g"),
                            ("qbb", 65536, "k_rollout_ws64g"), ("qbb", 98304, "k_rollout"), ("qcp-st", 4096, "k_rollout"), ("bob", 65536, "k_rollout_ws64g"),
                            ("bob-d", 65536, "k_rollout_ws64g"), ("bob", 98304, "k_rollout_ws64g"), ("pend", 98304, "k_rollout_ws64g"), ("qq-st", 98304, "k_rollout_ws64g"), ("qq-st", 73728, "k_rollout_ws64"), ("qcp-su", 65536, "k_rollout_ws64g"),
                            ("qcp-su", 98304, "k_rollout"), ("qq-su", 4096, "k_rollout_ws64g"), ("qq-su", 32768, "k_rollout_ws64g"),
                            ("qq-su", 32769, "k_rollout_ws256g"), ("omo", 65536, "k_rollout_ws256g"), ("pend", 16384, "k_rollout_ws64g"),
                            ("qq-st", 65536, "k_rollout_ws256g")):
        x = vs.VecSimEnv(name, n, **KW[name])
        assert x.rollout_variant() == expect, (name, n)
        x.set_rollout_variant("k_rollout_ws")
        assert x.rollout_variant() == ("k_rollout" if name == "qcp-st" else "k_rollout_ws")
        x.set_rollout_variant("k_rollout_ws64g")  # the three-role shape only where the family has it
        assert x.rollout_variant() == ("k_rollout" if name == "qcp-st" else "k_rollout_ws64g" if name in G3_FAMILIES else "k_rollout_ws64")
        x.close()


def test_baseline_config1_omo_single_env_500_steps(vs, golden_dir):
    """BASELINE.json configs[0] on the device: ONE OneMassOscillatorSim, reset(init_state=[-0.7, 0]), the reference's 500
    actions, forward Euler; the whole closed-loop trajectory against the reference's (a stable linear system: fp32 rounding
    does not amplify), rewards, the once-only failure malus and the done mask; through vs_step and through the env object"""
    L = vs._lib
    g = np.load(os.path.join(golden_dir, "cfg1_omo_500.npz"))
    env = vs.VecSimEnv("omo", 1, dt=0.02, max_steps=500)
    env.reset(init_state=f32([[-0.7, 0.0]]))
    np.testing.assert_allclose(env.get(L.VS_OBS)[0], g["obs0"], rtol=1e-6)
    obj = vs.OneMassOscillatorSim(dt=0.02, max_steps=500)
    obs = obj.reset(init_state=np.array([-0.7, 0.0]))
    np.testing.assert_allclose(obs, g["obs0"], rtol=1e-6)
    for t in range(500):
        env.step(dev(g["act"][t][None, :]))
        s = env.get(L.VS_STATE)[0]
        np.testing.assert_allclose(s, g["state"][t + 1], rtol=2e-4, atol=2e-4, err_msg=f"t={t}")
        np.testing.assert_allclose(env.get(L.VS_REW)[0], g["rew"][t], rtol=5e-4, atol=1e-5, err_msg=f"t={t}")
        assert bool(env.get(L.VS_DONE)[0]) == bool(g["done"][t]), t
        if t < 80:  # the env object: the same values through the reference-shaped surface
            o2, r2, d2, _ = obj.step(g["act"][t].copy())
            assert np.array_equal(o2.astype(np.float32), s) and d2 == bool(g["done"][t])
            assert np.float32(r2) == env.get(L.VS_REW)[0]
    assert int(env.get(L.VS_STEPCOUNT)[0]) == 500 and env.error_count() == 0
    env.close()


def test_fused_kernels_fuzz_against_step_kernel(vs):
    """seeded sweep over families, sizes, launch splits, constructor flags, ActNorm, per-env parameters and auto-reset:
    k_rollout and k_rollout_ws must both reproduce the single-step kernel fed with their recorded actions, bit for bit"""
    L = vs._lib
    rng = np.random.default_rng(20260104)
    names = ["omo", "bob", "qq-su", "qcp-su", "qbb", "qq-st", "pend", "bob-d"]
    for case in range(24):
        name = names[case % len(names)]
        n = int(rng.choice([1, 63, 64, 257, 700, 1536]))
        kw = dict(KW[name], max_steps=int(rng.integers(5, 40)))
        extra = {}
        if name == "qcp-su":
            extra = dict(simple_dynamics=bool(rng.integers(2)), long=bool(rng.integers(2)),
                         wild_init=str(rng.choice(["True", "False", "other"])))
        if name == "qbb":
            extra = dict(simple_dynamics=bool(rng.integers(2)))
        auto_reset, act_norm, per_env = bool(rng.integers(2)), bool(rng.integers(2)), bool(rng.integers(2))
        splits = [int(x) for x in rng.integers(1, 13, size=4)]
        mode = int(rng.integers(1, 3))
        T = sum(splits)
        ref = vs.VecSimEnv(name, n, **kw, **extra)
        envs = {v: vs.VecSimEnv(name, n, **kw, **extra) for v in ("k_rollout",) + ws_variants(name)}
        params = None
        if per_env:
            params = np.tile(vs.nominal_params(name, **({"long": extra["long"]} if "long" in extra else {})), (n, 1))
            params *= 1.0 + 0.02 * rng.standard_normal(params.shape).astype(np.float32) * (params != 0)
        for e in [ref, *envs.values()]:
            if per_env:
                e.set_params(params)
            e.set_act_norm(act_norm)
            e.set_auto_reset(auto_reset, seed=99)
            e.reset(seed=case)
        trajs = {}
        for v, e in envs.items():
            e.set_rollout_variant(v)
            e.set_record_mode(mode)
            e.set_traj_capacity(T)
            t = 0
            for k in splits:
                e.set_traj_offset(t)
                e.step_random(k, seed=5, record=True)
                t += k
            trajs[v] = e.traj(T)
        a = trajs["k_rollout"]
        for v in ws_variants(name):
            for key in a:
                assert np.array_equal(a[key], trajs[v][key]), (case, name, key, v)
        alive = np.ones(n, dtype=bool)
        for t in range(T):
            assert np.array_equal(ref.get(L.VS_OBS)[alive], a["obs"][t][alive]), (case, name, t)
            if mode == 2:  # what rollout() keeps besides obs / act / rew: state and hidden state before the step ...
                assert np.array_equal(ref.get(L.VS_STATE)[alive], a["state"][t][alive]), (case, name, t)
                if ref.dims["H"]:
                    assert np.array_equal(ref.get(L.VS_HIDDEN)[alive], a["hidden"][t][alive]), (case, name, t)
                if name != "bob-d":  # ... and env.limit_act(act): the projection onto the action box the policy sees
                    if act_norm:
                        lo_, hi_ = -np.ones_like(a["act"][t]), np.ones_like(a["act"][t])
                    else:
                        cst = ref.get(L.VS_CONSTS)
                        amax = {"omo": cst[:, 3:4], "bob": cst[:, 7:8], "pend": cst[:, 3:4]}.get(
                            name, np.float32({"qq-su": 4.5, "qq-st": 4.5, "qcp-su": 6.0, "qbb": 3.0}.get(name, 0.0)))
                        lo_, hi_ = -amax * np.ones_like(a["act"][t]), amax * np.ones_like(a["act"][t])
                    assert np.array_equal(np.clip(a["act"][t], lo_, hi_)[alive], a["act_app"][t][alive]), (case, name, t)
            ref.step(dev(a["act"][t]))
            assert np.array_equal(ref.get(L.VS_REW)[alive], a["rew"][t][alive]), (case, name, t)
            assert np.array_equal(ref.get(L.VS_DONE).astype(bool)[alive], a["done"][t].astype(bool)[alive])
            if not auto_reset:
                alive &= ~a["done"][t].astype(bool)
        for which in (L.VS_STATE, L.VS_HIDDEN, L.VS_STEPCOUNT, L.VS_RETURNS):
            x, y = ref.get(which), envs["k_rollout"].get(which)
            assert np.array_equal(x[alive], y[alive]), (case, name, which)
            for v in ws_variants(name):
                assert np.array_equal(y, envs[v].get(which)), (case, name, which, v)
        for e in [ref, *envs.values()]:
            assert e.error_count() == 0
            e.close()


def test_freeze_done_and_event_timer(vs):
    """vs_set_freeze_done: with it on, vs_step leaves finished lanes alone (state, observation, counters, flags; reward 0;
    a NaN fed to such a lane raises no flag) -- rollout() stops at done -- and off (default) env.step() keeps stepping as in
    the reference; vs_timer_start / vs_timer_stop bracket launches on the handle's stream"""
    L = vs._lib
    n = 512
    kw = dict(KW["bob"], max_steps=6)
    a, b = vs.VecSimEnv("bob", n, **kw), vs.VecSimEnv("bob", n, **kw)
    a.set_freeze_done(True)
    for e in (a, b):
        e.reset(seed=3)
    rng = np.random.default_rng(0)
    for t in range(6):
        act = dev(rng.uniform(-20, 20, (n, 1)))
        a.step(act), b.step(act)
    assert a.get(L.VS_DONE).all() and np.array_equal(a.get(L.VS_STATE), b.get(L.VS_STATE))  # time-out at step 6 for everyone
    frozen = {w: a.get(w).copy() for w in (L.VS_STATE, L.VS_OBS, L.VS_STEPCOUNT, L.VS_DONE, L.VS_RETURNS)}
    bad = dev(np.full((n, 1), np.nan))
    a.timer_start()
    a.step(bad), b.step(bad)
    ms = a.timer_stop()
    assert 0.0 < ms < 50.0
    for w, v in frozen.items():
        assert np.array_equal(a.get(w), v), w
    assert (a.get(L.VS_REW) == 0).all() and a.error_count() == 0
    assert b.error_count() == n and (b.get(L.VS_STEPCOUNT) == 7).all()  # the unfrozen handle stepped on and saw the NaN
    a.set_freeze_done(False)
    a.step(dev(np.zeros((n, 1))))
    assert (a.get(L.VS_STEPCOUNT) == 7).all()
    a.close(), b.close()


@pytest.mark.parametrize("auto_reset", [False, True])
def test_nan_flag_is_the_same_in_every_fused_kernel(vs, auto_reset):
    """a lane whose state turns NaN (here: a NaN domain parameter) raises the sticky error flag in k_rollout (tested per
    step) and in both shapes of k_rollout_ws (tested where a NaN state must surface: at the lane's time-out reset and at
    the end of the launch) -- the same lanes, nothing else"""
    L = vs._lib
    n = 700
    flags = {}
    for variant in ("k_rollout",) + ws_variants("qq-su"):
        e = vs.VecSimEnv("qq-su", n, **dict(KW["qq-su"], max_steps=20))
        P = np.tile(vs.nominal_params("qq-su"), (n, 1))
        P[[5, 64, 699], 0] = np.nan
        e.set_params(P)
        e.set_rollout_variant(variant)
        e.set_auto_reset(auto_reset, seed=3)
        e.reset(seed=4)
        e.set_traj_capacity(30)
        e.step_random(30, seed=5, record=True)  # crosses the time-out at step 20
        flags[variant] = e.get(L.VS_ERRFLAG).copy()
        assert e.error_count() == 3
        with pytest.raises(vs.ValueErr):
            e.raise_on_error()
        e.close()
    expect = np.zeros(n, dtype=np.uint8)
    expect[[5, 64, 699]] = 1
    for variant, f in flags.items():
        assert np.array_equal(f, expect), variant


@pytest.mark.parametrize("name", ["bob", "omo", "qbb"])
def test_long_launches_with_many_resets_equal_the_plain_kernel(vs, name):
    """one launch of 300 recorded steps with auto-reset for the families with short episodes (ball-on-beam: 73 steps on
    average): every lane resets several times inside the launch, through the reset stock of k_rollout_ws (refilled every 32
    steps) and, where a lane resets twice between refills, through its own draw -- records, final buffers and episode
    statistics must equal k_rollout's bit for bit in both workgroup shapes"""
    L = vs._lib
    n, T = 2048, 300
    out = {}
    for variant in ("k_rollout",) + ws_variants(name):
        e = vs.VecSimEnv(name, n, **dict(KW[name], max_steps=90))
        e.set_params(np.tile(vs.nominal_params(name), (n, 1)))
        e.set_rollout_variant(variant)
        e.set_auto_reset(True, seed=11)
        e.reset(seed=12)
        e.set_record_mode(2)
        e.set_traj_capacity(T)
        e.step_random(T, seed=13, record=True)
        tt = e.traj_tensors(T)
        out[variant] = (tt["rec"].clone(), tt["done"].clone(), {w: e.get(w) for w in (L.VS_STATE, L.VS_HIDDEN, L.VS_STEPCOUNT,
                        L.VS_RETURNS, L.VS_EPSTAT_COUNT, L.VS_EPSTAT_RETSUM, L.VS_EPSTAT_LENSUM)})
        assert e.error_count() == 0
        e.close()
    rec_a, done_a, fin_a = out["k_rollout"]
    assert int(done_a.sum()) >= 3 * n  # every lane finished (and restarted) several episodes
    gaps = torch.diff(torch.nonzero(done_a[:, 0]).flatten())
    for variant in ws_variants(name):
        rec_b, done_b, fin_b = out[variant]
        assert torch.equal(rec_a, rec_b) and torch.equal(done_a, done_b), variant
        for w in fin_a:
            assert np.array_equal(fin_a[w], fin_b[w]), (variant, w)
    assert len(gaps) >= 2
