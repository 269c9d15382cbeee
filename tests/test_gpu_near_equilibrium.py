"""
Near-equilibrium parity: the trig of the hot path (vecsim_envs.h: sincos_fast) and one step from rest at the equilibria.

The golden and oracle parity tests (tests/test_gpu_parity.py) hold every state to 1e-5 relative plus an absolute floor of
1e-6 of the state box's half-width.  Where the dynamics are quiet -- a pendulum at rest next to k pi -- that floor is far
above fp32 resolution, and a sine that is wrong by 2e-7 absolute (26 % relative at |x - pi| ~ 1e-6) passes it.  This file
closes that gap:

  1. (gpu) sin(x) near every k pi, read back through observe(), to 2e-6 RELATIVE; cos near pi/2 + k pi is printed and held
     to the absolute bound of test_fast_sincos_accuracy_through_observe (no equilibrium sits there).
  2. (gpu) one vs_step at the equilibria of every family against the fp64 oracle, with a tolerance derived from a plain fp32
     evaluation of the oracle's own expression tree on the same inputs:
         tol[i, j] = 10 * B32[j, band(i)] + 2 ulp32(s'_64[i, j])
     B32[j, band] is the worst |s'_32 - s'_64| of cpu_ref.make_ref(..., dtype=np.float32) over the lanes of one band, a band
     being the lanes of one multiple k of pi and one decade of their angle's offset |d| from it.  The kernel may be at most
     10x worse than fp32 arithmetic; the existing check_step runs on the same lanes, so nothing is held to less than before.
  3. (cpu) that tolerance has teeth: the fp32 restatement passes it, while an emulation of library 304's sincos (a 2 pi
     reduction to [-pi, pi] before the transcendental unit) and a 1e-5 relative error in gravity_const do not.
"""
import sys

import numpy as np
import pytest

from oracle import cpu_ref

N = 4096
FACTOR = 10.0
SIN_RTOL = 2e-6  # ~16 ulp
COS_ATOL = 4e-7  # test_fast_sincos_accuracy_through_observe

# family -> stepping arguments, the multiples k of pi its angle sits next to, and the roles of its state / hidden slots:
# "ang" (the angle near k pi), "ang0" (a second angle near 0), "small" (a position near 0), "vel" (a rate near 0)
CASES = {
    "qq-su": dict(dt=0.004, max_steps=4000, ks=(0, 1, -1, 3, -3), state=("small", "ang", "vel", "vel"), hidden=()),
    "qq-st": dict(dt=0.01, max_steps=500, ks=(1,), state=("small", "ang", "vel", "vel"), hidden=()),
    "pend": dict(dt=0.02, max_steps=400, ks=(0, 1, -1, 2, -2, 3, -3), state=("ang", "vel"), hidden=()),
    # dt = 2 ms: the addition-theorem branch (rk_tail<true>) for the stage angles
    "qcp-su": dict(dt=0.002, max_steps=8000, ks=(0, 1, -1), state=("small", "ang", "vel", "vel"), hidden=("vel",)),
    # dt = 10 ms: a fresh sincos per RK stage
    "qcp-st": dict(dt=0.01, max_steps=300, ks=(1,), state=("small", "ang", "vel", "vel"), hidden=("vel",)),
    "bob": dict(dt=0.01, max_steps=500, ks=(0,), state=("small", "ang", "vel", "vel"), hidden=()),
    "qbb": dict(dt=0.01, max_steps=500, ks=(0,), state=("ang", "ang0", "small", "small", "vel", "vel", "vel", "vel"),
                hidden=("small", "small")),
    "omo": dict(dt=0.02, max_steps=300, ks=(0,), state=("ang", "vel"), hidden=()),
}
# the action dead zones [neg, pos] the kernels test (qbb: per action dimension); the others' thresholds are nominally 0
DEAD_ZONE = {"qbb": ((-0.10, 0.28), (-0.074, 0.28))}
# check_step holds rewards to 3e-5 relative.  The cartpole stabiliser's reward is minus a quadratic cost that is ~1e-13 .. 1e-6
# at its equilibrium, and the fp32 rounding of its desired angle pi alone moves that cost by O(1) relative (the fp32
# restatement: up to 1.5): there the relative bound is widened by the fp32-derived band tolerance of the states, not replaced.
REW_FROM_FP32 = {"qcp-st"}
WORST = {}  # (family, check) -> worst error / tolerance, printed by the tests


def f32(x):
    return np.asarray(x, dtype=np.float32)


def ulp32(v):
    """fp32 spacing at |v| (float64)"""
    return np.spacing(np.abs(np.asarray(v, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def log_uniform(rng, lo, hi, n, signed=True):
    v = np.exp(rng.uniform(np.log(lo), np.log(hi), n))
    return v * rng.choice([-1.0, 1.0], n) if signed else v


def near_zero(rng, n):
    """exactly 0 for a third of the lanes, +-1e-6 .. 1e-3 log-uniform for the rest"""
    v = log_uniform(rng, 1e-6, 1e-3, n)
    v[rng.random(n) < 1 / 3] = 0.0
    return v


def angles_near(rng, ks, n):
    """-> (x [n] fp32 values as float64, k [n]): x = fp32(k pi + d), d log-uniform in +-1e-6 .. 1e-2, plus lanes at fp32(k pi)
    and at its two fp32 neighbours (for k = 0: +-1e-6 .. 1e-2 only, and 0 itself)"""
    k = rng.choice(np.asarray(ks), n)
    x = f32(k * np.pi + log_uniform(rng, 1e-6, 1e-2, n))
    at = f32(k * np.pi)
    pick = rng.random(n)
    x = np.where(pick < 0.05, at, x)
    x = np.where((pick >= 0.05) & (pick < 0.10), np.nextafter(at, np.float32(np.inf)), x)
    x = np.where((pick >= 0.10) & (pick < 0.15), np.nextafter(at, np.float32(-np.inf)), x)
    x = np.where((k == 0) & (pick < 0.15) & (pick >= 0.05), f32(log_uniform(rng, 1e-6, 1e-2, n)), x)
    return x.astype(np.float64), k


def bands(x, k):
    """band of each lane: (k, decade of |x - k pi|); offsets below 1e-7 (fp32(k pi) itself) share the 1e-8 decade, 0 is its own"""
    d = np.abs(x - k * np.pi)
    dec = np.where(d > 0, np.clip(np.floor(np.log10(np.maximum(d, 1e-300))), -8, -2), -9).astype(np.int64)
    return k.astype(np.int64) * 100 + dec


def case_inputs(name, n=N, seed=0):
    """the lanes of one family's case: fp32-representable inputs as float64 arrays, and each lane's band"""
    c = CASES[name]
    ref = cpu_ref.make_ref(name, c["dt"], c["max_steps"])
    rng = np.random.default_rng([seed, sum(map(ord, name))])
    x, k = angles_near(rng, c["ks"], n)
    slot = {"ang": lambda: x, "ang0": lambda: f32(angles_near(rng, (0,), n)[0]).astype(np.float64),
            "small": lambda: near_zero(rng, n), "vel": lambda: near_zero(rng, n)}
    state = np.stack([slot[r]() for r in c["state"]], axis=1) if c["state"] else np.zeros((n, 0))
    hidden = np.stack([slot[r]() for r in c["hidden"]], axis=1) if c["hidden"] else np.zeros((n, 0))
    params = ref.nominal_params(n)
    _, _, alo, ahi = ref.bounds(params)
    act = np.zeros((n, ref.A))
    pick = rng.integers(0, 3, size=(n, ref.A))
    small = ahi * rng.uniform(-1e-3, 1e-3, size=(n, ref.A))  # +-1e-3 of the box
    act = np.where(pick == 1, small, act)
    if name in DEAD_ZONE:
        dz = np.array(DEAD_ZONE[name])
        inside = rng.uniform(dz[:, 0], dz[:, 1], size=(n, ref.A))
        act = np.where(pick == 2, inside, act)
    else:
        act = np.where(pick == 2, -small, act)
    rd = lambda a: f32(a).astype(np.float64)  # noqa: E731
    return dict(params=rd(params), state=rd(state), hidden=rd(hidden), act=rd(act), curr_step=np.zeros(n, dtype=np.int64),
                band=bands(rd(x), k), k=k)


def step_ref(name, inp, dtype=np.float64, params=None):
    c = CASES[name]
    ref = cpu_ref.make_ref(name, c["dt"], c["max_steps"], dtype=dtype)
    p = inp["params"] if params is None else params
    return ref.step(inp["state"], inp["hidden"], inp["act"], p, inp["curr_step"])


def tolerance(inp, s64, s32):
    """tol[i, j] = FACTOR * B32[j, band(i)] + 2 ulp32(s'_64[i, j])"""
    err32 = np.abs(np.asarray(s32, dtype=np.float64) - s64)
    tol = 2.0 * ulp32(s64)
    for b in np.unique(inp["band"]):
        m = inp["band"] == b
        tol[m] += FACTOR * err32[m].max(axis=0)
    return tol


def ratio(got, s64, tol):
    """|got - s'_64| / tol, elementwise"""
    return np.abs(np.asarray(got, dtype=np.float64) - s64) / tol


def report(name, check, r, inp, extra=""):
    worst = float(r.max())
    WORST[(name, check)] = max(WORST.get((name, check), 0.0), worst)
    i, j = np.unravel_index(np.argmax(r), r.shape)
    print(f"[{name}] {check}: worst error / tol {worst:.3g} (lane {i}, component {j}, k = {inp['k'][i]}, "
          f"band {inp['band'][i] % 100 if inp['band'][i] % 100 < 50 else inp['band'][i] % 100 - 100}){extra}")
    return worst


# ------------------------------------------------------------------------------------------------ section 3 (cpu)
# library 304's sincos_fast restated in numpy, assuming an ideal v_sin_f32 / v_cos_f32: q = rint(x / 2pi) in fp32, a two-term
# FMA reduction to [-pi, pi] (each FMA exact in float64, then rounded once), r / 2pi rounded to fp32, sin / cos of 2 pi rev
_TWOPI_HI, _TWOPI_LO, _INV_2PI = np.float32(6.28318548202514648), np.float32(-1.74845553146951715e-07), np.float32(0.159154943091895336)


def _rev_lib304(x):
    x = f32(x)
    q = np.rint(x * _INV_2PI).astype(np.float64)
    r = f32(-q * np.float64(_TWOPI_HI) + x.astype(np.float64))
    r = f32(-q * np.float64(_TWOPI_LO) + r.astype(np.float64))
    return (r * _INV_2PI).astype(np.float64)


class _Lib304Trig:
    """numpy with sin / cos replaced by the emulation (for cpu_ref's module global ``np``)"""

    def __getattr__(self, attr):
        return getattr(np, attr)

    @staticmethod
    def sin(x):
        return np.sin(2 * np.pi * _rev_lib304(x))

    @staticmethod
    def cos(x):
        return np.cos(2 * np.pi * _rev_lib304(x))


def test_lib304_emulation_reproduces_its_error_floor():
    """the emulation shows library 304's floor: percent-level relative sin error next to +-pi, none next to 0 or 2 pi"""
    d = np.geomspace(1e-6, 1e-2, 200)
    for k, worst in ((1, 1e-2), (-1, 1e-2), (0, 2e-7), (2, 2e-7)):
        x = f32(k * np.pi + d).astype(np.float64)
        rel = np.abs(_Lib304Trig.sin(x) - np.sin(x)) / np.abs(np.sin(x))
        assert (rel.max() > worst) if k % 2 else (rel.max() < worst), (k, rel.max())
    xs = f32(np.linspace(-4 * np.pi, 4 * np.pi, 10001)).astype(np.float64)
    assert np.abs(_Lib304Trig.sin(xs) - np.sin(xs)).max() < 4e-7


@pytest.mark.parametrize("name", sorted(CASES))
def test_fp32_restatement_passes_the_tolerance(name):
    inp = case_inputs(name)
    s64 = step_ref(name, inp)["state"]
    s32 = step_ref(name, inp, dtype=np.float32)["state"]
    r = ratio(s32, s64, tolerance(inp, s64, s32))
    assert report(name, "fp32 restatement", r, inp) <= 1.0 / FACTOR + 1e-12


@pytest.mark.parametrize("name", ["qq-su", "qq-st", "pend"])
def test_lib304_sincos_fails_the_tolerance_near_odd_k_pi(name, monkeypatch):
    inp = case_inputs(name)
    s64 = step_ref(name, inp)["state"]
    tol = tolerance(inp, s64, step_ref(name, inp, dtype=np.float32)["state"])
    monkeypatch.setattr(cpu_ref, "np", _Lib304Trig())
    emu = step_ref(name, inp)["state"]
    monkeypatch.undo()
    r = ratio(emu, s64, tol)
    for k in sorted(set(CASES[name]["ks"])):
        m = inp["k"] == k
        w = report(name, f"lib304 sincos at k = {k:+d}", r[m], {key: v[m] for key, v in inp.items()})
        if k % 2:
            assert w > 1.0, (k, w)


@pytest.mark.parametrize("name", ["qq-su", "qq-st", "pend", "qcp-su"])
def test_gravity_error_of_1e5_fails_the_tolerance(name):
    inp = case_inputs(name)
    s64 = step_ref(name, inp)["state"]
    tol = tolerance(inp, s64, step_ref(name, inp, dtype=np.float32)["state"])
    ref = cpu_ref.make_ref(name, CASES[name]["dt"], CASES[name]["max_steps"])
    p = inp["params"].copy()
    p[:, ref.param_names.index("gravity_const")] *= 1.0 + 1e-5
    r = ratio(step_ref(name, inp, params=p)["state"], s64, tol)
    for near, m in (("0", inp["k"] == 0), ("odd k pi", inp["k"] % 2 == 1)):
        if m.any():
            w = report(name, f"gravity +1e-5 near {near}", r[m], {key: v[m] for key, v in inp.items()})
            assert w > 1.0, (near, w)


# ------------------------------------------------------------------------------------------------ sections 1 and 2 (gpu)
@pytest.fixture(scope="module")
def vs():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import simurlacra_amd

    return simurlacra_amd


def _parity():
    """check_step / setup_lanes of tests/test_gpu_parity.py (imported here so that the cpu tests above need no torch)"""
    import importlib
    import os

    here = os.path.dirname(os.path.abspath(__file__))
    if here not in sys.path:
        sys.path.insert(0, here)
    return importlib.import_module("test_gpu_parity")


def sincos_lanes(rng):
    """-> (x near k pi, y near pi/2 + k pi), k = -4..4, both fp32 values as float64"""
    ks = tuple(range(-4, 5))
    x, _ = angles_near(rng, ks, N)
    tiny = log_uniform(rng, 1e-30, 1e-6, 64)  # k = 0: the same relative bound for every |x| < 1e-2
    x = np.concatenate([x, f32(tiny).astype(np.float64), [0.0]])
    kk = rng.choice(np.asarray(ks), x.size)
    y = f32((kk + 0.5) * np.pi + log_uniform(rng, 1e-6, 1e-2, x.size)).astype(np.float64)
    return x, y


def _sin_rel(got, x):
    exp = np.sin(x)
    err = np.abs(np.asarray(got, dtype=np.float64) - exp)
    rel = np.where(exp != 0, err / np.maximum(np.abs(exp), 1e-300), np.where(err == 0, 0.0, np.inf))
    return rel


@pytest.mark.gpu
def test_sincos_relative_error_near_multiples_of_pi(vs):
    """sin(x) near every k pi (k = -4..4) to 2e-6 relative, through QQubeSim.observe (alpha: obs 2, 3; theta: obs 0, 1) and
    PendulumSim.observe (theta: obs 0, 1); cos near pi/2 + k pi is printed and held to the absolute bound"""
    L = vs._lib
    x, y = sincos_lanes(np.random.default_rng(1))
    n = x.size
    q = vs.VecSimEnv("qq-su", n, dt=0.004, max_steps=4000)
    s = np.zeros((n, 4))
    s[:, 0], s[:, 1] = y, x
    q.reset(init_state=f32(s))
    oq = q.get(L.VS_OBS).astype(np.float64)
    q.close()
    p = vs.VecSimEnv("pend", n, dt=0.02, max_steps=400, init_state=np.array([0.1, 0.2]))
    p.reset(init_state=f32(np.stack([x, np.zeros(n)], axis=1)))
    op = p.get(L.VS_OBS).astype(np.float64)
    p.close()
    k = np.rint(x / np.pi).astype(int)
    for label, got in (("qq alpha", oq[:, 2]), ("pend theta", op[:, 0])):
        rel = _sin_rel(got, x)
        worst = {kk: float(rel[k == kk].max()) for kk in range(-4, 5)}
        print(f"[sincos] {label}: worst relative sin error per k: " + ", ".join(f"{kk:+d}: {w:.2e}" for kk, w in worst.items()))
        bad = rel > SIN_RTOL
        assert not bad.any(), f"{bad.sum()} lanes over {SIN_RTOL} relative, worst {rel.max():.3g} at x = {x[np.argmax(rel)]!r}"
    np.testing.assert_allclose(oq[:, 3], np.cos(x), rtol=0, atol=COS_ATOL)
    np.testing.assert_allclose(op[:, 1], np.cos(x), rtol=0, atol=COS_ATOL)
    cos_y = oq[:, 1]
    rel = np.abs(cos_y - np.cos(y)) / np.abs(np.cos(y))
    print(f"[sincos] qq theta: cos near pi/2 + k pi: worst relative error {rel.max():.2e}, "
          f"absolute {np.abs(cos_y - np.cos(y)).max():.2e}")
    np.testing.assert_allclose(cos_y, np.cos(y), rtol=0, atol=COS_ATOL)
    np.testing.assert_allclose(oq[:, 0], np.sin(y), rtol=0, atol=COS_ATOL)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_step_at_equilibria_against_fp32_derived_tolerance(vs, name, monkeypatch):
    """one vs_step at the equilibria vs the fp64 oracle; tolerance: FACTOR x what fp32 evaluation of the oracle's expression
    tree loses in the same band, plus 2 ulp.  Then check_step on the same lanes (state / obs / reward / hidden / done masks)."""
    par = _parity()
    L = vs._lib
    c = CASES[name]
    inp = case_inputs(name)
    kw = dict(dt=c["dt"], max_steps=c["max_steps"])
    ref = cpu_ref.make_ref(name, **kw)
    exp = ref.step(inp["state"], inp["hidden"], inp["act"], inp["params"], inp["curr_step"])
    s32 = step_ref(name, inp, dtype=np.float32)["state"]
    tol = tolerance(inp, exp["state"], s32)
    env = vs.VecSimEnv(name, N, **kw)
    par.setup_lanes(env, L, inp["params"], inp["state"], inp["hidden"], inp["curr_step"])
    env.step(par.dev(inp["act"]))
    got = env.get(L.VS_STATE).astype(np.float64)
    r = ratio(got, exp["state"], tol)
    for k in sorted(set(c["ks"])):
        m = inp["k"] == k
        report(name, f"step at k = {k:+d}", r[m], {key: v[m] for key, v in inp.items()})
    bad = r > 1.0
    assert not bad.any(), (f"{bad.sum()} state elements over {FACTOR:g}x the fp32 restatement's error, worst x{r.max():.3g} "
                           f"(lane {np.unravel_index(np.argmax(r), r.shape)})")
    if name in REW_FROM_FP32:
        rew32 = step_ref(name, inp, dtype=np.float32)["rew"][:, None]

        def rew_close(fam, got_r, exp_r):
            exp_r = np.asarray(exp_r, dtype=np.float64)[:, None]
            tol_r = tolerance(inp, exp_r, rew32) + 3e-5 * np.abs(exp_r)
            rr = ratio(np.asarray(got_r, dtype=np.float64)[:, None], exp_r, tol_r)
            assert report(fam, "reward", rr, inp) <= 1.0

        monkeypatch.setattr(par, "assert_rew_close", rew_close)
    par.check_step(env, L, ref, inp["params"], inp["state"], inp["hidden"], inp["act"], inp["curr_step"], exp)
    assert env.error_count() == 0
    env.close()
