"""
The checks of random_draw_checks.py, on the host:
  (1) an ideal generator -- NumPy's, pushed through the fp64 forward maps of every family's init space, action space and every
      domain-parameter kind, rounded to float32 -- passes every check at the sample sizes test_gpu_random_draws.py uses, and
  (2) every planted fault fails the check named for it at the size the GPU test gives that check.
If (1) failed, an inverse map would be wrong; if (2) failed, the GPU test's sample would be too small for the fault.
"""
import numpy as np
import pytest

import random_draw_checks as rc
from oracle import cpu_ref

pytest.importorskip("torch")

ENVS = ["omo", "bob", "qq-su", "qcp-su", "qbb", "qq-st", "qcp-st", "pend", "bob-d"]
KW = {n: dict(dt=0.01, max_steps=100) for n in ENVS}
KW["pend"]["init_state"] = np.array([0.1, 0.2])
# the GPU tests' sizes: lanes per handle, recorded steps, rows of init draws (reset + 8 episodes), live redraws, shards of sample_params
N, T, EPISODES, REDRAWS, SHARDS = 16384, 64, 9, 8, 4
BOOK = rc.Book()


def f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def lane_params(ref, rng, n=N):
    """+-15 % around nominal, per lane, as float32 holds them"""
    p = ref.nominal_params(n)
    return f32(p * rng.uniform(0.85, 1.15, p.shape))


def draw_init(ref, params, rng, rows):
    """rows of init states [rows, n, S] by the reference's definition of the init space"""
    n = params.shape[0]
    if ref.name in ("bob", "bob-d"):
        side = rng.integers(2, size=(rows, n))
        b0, b1 = ref.init_bounds(params, 0), ref.init_bounds(params, 1)
        lo, hi = np.where(side[..., None] == 1, b1[0], b0[0]), np.where(side[..., None] == 1, b1[1], b0[1])
        return f32(lo + (hi - lo) * rng.random((rows, n, 4)))
    lo, hi = ref.init_bounds(params)
    init = lo + (hi - lo) * rng.random((rows, n, lo.shape[1]))
    if ref.name == "qbb":
        init = np.stack([ref.polar_to_init(x) for x in init])
    return np.stack([ref.state_from_init(f32(x)) for x in init])


def draw_actions(ref, params, rng, rows, normed=False):
    _, _, alo, ahi = ref.bounds(params)
    if normed:
        alo, ahi = -np.ones_like(alo), np.ones_like(ahi)
    n = params.shape[0]
    if ref.name == "bob-d":
        eles = np.stack([alo[:, 0], 0.5 * (alo[:, 0] + ahi[:, 0]), ahi[:, 0]], axis=1)
        k = rng.integers(3, size=(rows, n))
        return f32(eles[np.arange(n)[None], k])[..., None]
    return f32(alo + (ahi - alo) * rng.random((rows, n, ref.A)))


SPECS = rc.PARAM_SPECS


def draw_params(specs, names, rng, rows, n):
    P = np.zeros((rows, n, len(names)))
    for s in specs:
        name, kind, mean, spread, lo, hi = s[:6]
        if kind == "uniform":
            x = rng.uniform(mean - spread, mean + spread, (rows, n))
        elif kind == "bernoulli":
            x = np.where(rng.random((rows, n)) < s[6], spread, mean)
        else:
            x = np.clip(mean + spread * rng.standard_normal((rows, n)), lo, hi)
            if len(s) > 7 and s[7]:
                x = np.rint(x)
        P[..., names.index(name)] = x
    return f32(P)


# ------------------------------------------------------------------------------------------------- an ideal generator passes
@pytest.mark.parametrize("normed", [False, True])
@pytest.mark.parametrize("name", ENVS)
def test_ideal_actions_pass(name, normed):
    rng = np.random.default_rng(ENVS.index(name) + 100 * normed)
    ref = cpu_ref.make_ref(name, **KW[name])
    params = lane_params(ref, rng)
    vs = rc.action_variates(ref, draw_actions(ref, params, rng, T, normed), params, normed)
    assert len(vs) == (1 if ref.A == 1 else 2) and vs[0].u.shape == (T, N)
    rc.battery(BOOK, "host actions", vs, step_lags=(1, 4 // ref.A), what=name)


@pytest.mark.parametrize("name", [n for n in ENVS if n != "pend"])
def test_ideal_init_states_pass(name):
    rng = np.random.default_rng(20 + ENVS.index(name))
    ref = cpu_ref.make_ref(name, **KW[name])
    params = lane_params(ref, rng)
    vs = rc.init_variates(ref, draw_init(ref, params, rng, EPISODES), params)
    assert len(vs) == {"omo": 2, "bob": 5, "bob-d": 5, "qq-st": 2}.get(name, 4)
    rc.battery(BOOK, "host init", vs, what=name)
    if name in ("bob", "bob-d"):
        rc.hold_lagged(BOOK, "host init", vs[:1], 0, 1, f"{name} side bit, row t x t + 1")


def test_singular_init_space_has_no_variates():
    ref = cpu_ref.make_ref("pend", **KW["pend"])
    params = ref.nominal_params(8)
    assert rc.init_variates(ref, np.tile(f32(KW["pend"]["init_state"]), (2, 8, 1)), params) == []


@pytest.mark.parametrize("rows", [SHARDS, REDRAWS])
def test_ideal_domain_parameters_pass(rows):
    rng = np.random.default_rng(40 + rows)
    names = list(cpu_ref.ENV_REFS["qq-su"].param_names)
    vs = rc.param_variates(SPECS, names, draw_params(SPECS, names, rng, rows, N))
    assert [v.probs is None for v in vs] == [True, True, True, True, False, False, False, True, True]
    rc.battery(BOOK, "host params", vs, what=f"{rows} rows")
    rc.hold_lagged(BOOK, "host params", [v for v, s in zip(vs, SPECS) if s[1] == "bernoulli"], 0, 1, "Bernoulli, row t x t + 1")
    pool = np.concatenate([v.u.ravel() for v in vs if v.probs is None])
    BOOK.hold("host params", "marginal", rc.marginal(pool, max(v.q for v in vs if v.probs is None)), "all continuous parameters")
    k = rng.integers(6, size=(rows, N))
    rc.battery(BOOK, "host params", [rc.set_index_variate(k, 6)], what="buffer set")


def test_ideal_normal_noise_passes():
    rng = np.random.default_rng(60)
    b, std = np.array([0.25, -0.5]), np.array([0.5, 0.25])
    act = np.float32(b) + np.float32(std) * rng.standard_normal((T, N, 2)).astype(np.float32)  # what the kernel's fmaf leaves
    vs = [rc.normal_variate(f"z{j}", act[..., j], np.float32(b[j]), np.float32(std[j])) for j in range(2)]
    rc.battery(BOOK, "host noise", vs)


def test_bare_uniforms_and_the_budget():
    rng = np.random.default_rng(7)
    worst = {}
    for n in (16384, 65536, 1048576):
        u, v = rng.random(n), rng.random(n)
        for k, r in (("marginal", rc.marginal(u)), ("correlation", rc.correlation(u, v)), ("joint_cells", rc.joint_cells(u, v))):
            worst[k] = max(worst.get(k, 0.0), BOOK.hold("host bare", k, r, f"n = {n}"))
    print("bare uniforms, worst ratios:", {k: round(v, 3) for k, v in worst.items()})
    print(BOOK.report())
    BOOK.assert_budget()


# ----------------------------------------------------------------------------------------------------- planted faults fail
def test_planted_faults_fail_the_check_named_for_them():
    rng = np.random.default_rng(1)
    ratios = {}
    # one draw shared by two dimensions, at the smallest sample a pair of dimensions gets (one row of 16 384 lanes)
    u = rng.random(N)
    ratios["shared draw"] = rc.correlation(u, u)
    # the same, 10 % of the time: needs the 65 536 samples every pair of dimensions has on the GPU (sample_params: four shards)
    u, v = rng.random(SHARDS * N), rng.random(SHARDS * N)
    ratios["shared draw, 10 %"] = rc.correlation(u, np.where(rng.random(u.size) < 0.1, u, v))
    ratios["v = frac(2 u)"] = rc.joint_cells(u[:N], (2 * u[:N]) % 1.0)
    # ... and dependence without any linear part, which `correlation` cannot see: v = |2 u - 1| (uniform, uncorrelated with u)
    assert rc.correlation(u, np.abs(2 * u - 1)) <= 1.0
    ratios["v = |2 u - 1|"] = rc.joint_cells(u[:N], np.abs(2 * u[:N] - 1))
    # distribution faults: the pooled sizes (2^20) only
    u = rng.random(1 << 20)
    ratios["range shrunk by 3 %"] = rc.marginal(0.015 + 0.97 * u)
    ratios["normal of std 1.03"] = rc.marginal(rc.Phi(1.03 * rng.standard_normal(1 << 20)))
    # lane i and lane i + 64 on one stream (every second group of 64), at one row of lanes
    x = rng.random((1, N))
    y = x.reshape(1, -1, 2, 64).copy()
    y[:, :, 1] = y[:, :, 0]
    ratios["lanes i, i + 64 on one stream"] = rc.correlation(y.reshape(1, N)[:, :-64], y.reshape(1, N)[:, 64:])
    # the draws of episode e + 1 equal to those of episode e, at the init test's 9 rows
    x = np.repeat(rng.random((1, N)), EPISODES, axis=0)
    ratios["episode e + 1 = episode e"] = rc.correlation(x[:-1], x[1:])
    # a block reused across SPB steps: step t + SPB repeats step t, seen at lag SPB and not at lag 1
    for spb in (2, 4):
        x = rng.random((T, N))
        for t in range(spb, T):
            if (t // spb) % 2:
                x[t] = x[t - spb]
        ratios[f"block reused, SPB = {spb}"] = rc.correlation(x[:-spb], x[spb:])
        assert rc.correlation(x[:-1], x[1:]) <= 1.0
    # the high word of the step counter dropped: after a seek to 8 steps before the boundary, row t + 8 repeats row t of the run from
    # step 0.  The aligned rows see nothing; rows 8 .. against rows 0 .. do (hold_shifted, at the seek test's 64 x 16 384)
    base = [rc.Var("a0", rng.random((T, N)))]
    seeked = [rc.Var("a0", np.concatenate([rng.random((8, N)), base[0].u[:-8]]))]
    quiet, loud = rc.Book(), rc.Book()
    rc.hold_against(quiet, "fault", seeked, base, "aligned rows")
    with pytest.raises(AssertionError):
        rc.hold_shifted(loud, "fault", seeked, base, 8, "rows 8 .. x rows 0 ..")
    ratios["counter high word dropped"] = loud.worst[("fault", "correlation")]
    # an atom repeated from episode to episode (the Bernoulli redraw, the side bit), at the live redraw's 8 rows
    stuck = [rc.Var("b", np.repeat(np.where(rng.random((1, N)) < 0.3, 0.85, 0.35), REDRAWS, axis=0),
                    probs=rc._atom_probs([0.35, 0.85], [0.7, 0.3]))]
    with pytest.raises(AssertionError):
        rc.hold_lagged(loud, "atom", stuck, 0, 1, "row t x t + 1")
    ratios["Bernoulli repeated from episode to episode"] = loud.worst[("atom", "correlation")]
    print({k: round(v, 2) for k, v in ratios.items()})
    for k, v in ratios.items():
        assert v > 1.0, (k, v)


def test_a_wrong_inverse_map_is_caught():
    """the lane's own bounds matter: nominal bounds under per-lane parameters fail `marginal` or the in-space assertion"""
    rng = np.random.default_rng(3)
    ref = cpu_ref.make_ref("bob", **KW["bob"])
    params = lane_params(ref, rng)
    st = draw_init(ref, params, rng, EPISODES)
    with pytest.raises(AssertionError):
        vs = rc.init_variates(ref, st, ref.nominal_params(N))
        assert rc.marginal(vs[1].u, vs[1].q) <= 1.0


def test_frequency_bounds():
    assert not rc.frequency_usable(16384, rc.TAIL3) and rc.frequency_usable(1 << 20, rc.TAIL3)
    rng = np.random.default_rng(5)
    n = 1 << 20
    assert rc.frequency(int((np.abs(rng.standard_normal(n)) > 3).sum()), n, rc.TAIL3) <= 1.0
    assert rc.frequency(int((np.abs(1.1 * rng.standard_normal(n)) > 3).sum()), n, rc.TAIL3) > 1.0
