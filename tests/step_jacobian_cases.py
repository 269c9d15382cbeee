"""
What the tests of the one-step Jacobians share (test_gpu_parity.test_step_jacobians_against_finite_differences,
test_step_jacobian_positions_host): the inputs of a case, the fp64 oracle and the tolerance, one Jacobian POSITION (i, k) -- output i,
input k -- at a time.  Not a test module: import it by bare name.

vs_step_jac returns d(s', r, obs') / d(s, a) in raw units, [n, S, S + A], [n, S + A] and [n, O, S + A].  The positions of one array
differ by five orders of magnitude (a diagonal of 1 and d alpha_dot' / d alpha of 15 .. 37 beside entries of order dt and dt^2), so one
floor over the whole array -- 3e-4 max |g_smooth|, the rule this module replaces -- lets a small position be zero or of the wrong sign
in every lane.  The rule here is the per-column rule of derivative_cases.py with one position per column, the lanes of a position being
of one size, plus one term for what fp32 tangents cannot resolve.  For the entry (lane, i, k) of an array g:

    tol = 3e-3 |g| + 3e-4 top(i, k) + K_FP32 2^-23 rowmax(lane, i) / scale[lane, k]

top(i, k) is the largest smooth |g| of the position over the lanes; rowmax(lane, i) = max_k' |g(lane, i, k')| scale[lane, k'] is the
largest entry of the row once every column is expressed in the unit of output i, `scale` being the state half-width or the action bound,
floored at 1e-3 (the unit the finite differences step by).  A forward-mode tangent of output i is a sum over the inputs whose terms are
as large as rowmax, so its entries carry rounding of that size whatever their own; the fork's own fixture is met to 5.6e-8 of the row
maximum, half an fp32 ulp of a row whose smallest live entry is 1e-5.  On the cases of this module the device
turned out not to need the term (K_FP32 below).  The result is the smaller of this and of the rule replaced, entry by entry: no entry
is held more loosely than before.

Positions the oracle holds (almost) at zero (derivative_cases.null_columns) have no unit of their own.  Where the oracle is 0.0 in
every lane at both step sizes the device entry must be 0.0; where it holds rounding noise the device stays under the third term alone.
"""
import functools
from typing import NamedTuple

import numpy as np

import derivative_cases as dc
from oracle import cpu_ref

ENVS = ["omo", "bob", "qq-su", "qcp-su", "qbb", "qq-st", "qcp-st", "pend", "bob-d"]
KW = {"omo": dict(dt=0.02, max_steps=300), "bob": dict(dt=0.01, max_steps=500), "qq-su": dict(dt=0.004, max_steps=4000),
      "qcp-su": dict(dt=0.002, max_steps=8000), "qbb": dict(dt=0.01, max_steps=500),
      "qq-st": dict(dt=0.01, max_steps=500), "qcp-st": dict(dt=0.01, max_steps=300),
      "pend": dict(dt=0.02, max_steps=400, init_state=np.array([0.1, 0.2])), "bob-d": dict(dt=0.01, max_steps=500)}
# "nominal": nominal parameters set per lane (k_step_jac<E, false>), 12 full waves; "per_lane": every parameter of every lane at
# nominal x (1 +- 5 %), two full waves and a partial one; "uniform": no set_params at all, the handle keeps its uniform constants
# (k_step_jac<E, true>)
LAYOUTS = ("nominal", "per_lane", "uniform")
N_LANES = {"nominal": 768, "per_lane": 150, "uniform": 150}
SEED = 11
N_LIMIT = 4  # the last lanes of the 150-lane layouts are at curr = max_steps - 1: the time-limit branch of done
ARRAYS = ("state", "rew", "obs")
ULP = 2.0 ** -23
# The multiple of an fp32 ulp of the row maximum that the third term allows: twice the largest (err - 3e-3 |g| - 3e-4 top) / third
# measured on the device over all families, layouts and arrays, rounded up to an integer.  Measured on MI355X (DESIGN.md section 2,
# next to the 5.6e-8 / 7.0e-7 line, has the figure of every family): the largest is -0.027 (qcp-su, d obs') -- the first two terms
# cover the device's error in every entry, which is at most 6.8e-3 of them -- so K_FP32 = ceil(2 x -0.027) = 0 and the third term is
# not drawn on.  It stays in the rule for a kernel change that needs it: raising K_FP32 takes a new measurement.
K_FP32 = 0


# ------------------------------------------------------------------------------------------------------------ the inputs
class Case(NamedTuple):
    ref: object
    n: int
    params: np.ndarray  # [n, P] float32
    state: np.ndarray   # [n, S] float32
    hidden: np.ndarray  # [n, H] float32
    act: np.ndarray     # [n, A] float32
    curr: np.ndarray    # [n] int64
    set_params: bool    # whether the handle gets `params` through set_params (False: it keeps its uniform constants)


@functools.lru_cache(maxsize=None)
def case(name, layout):
    """the inputs of a family's step-Jacobian test in one of LAYOUTS, all float32 and read-only: states within +-0.6 of the box
    half-width, hidden +-20 (qcp) or +-0.1, actions 0.35 .. 0.9 of the bound, the first eighth x 1.5 so that they clip, curr in 0 .. 49"""
    n = N_LANES[layout]
    rng = np.random.default_rng(SEED)
    ref = cpu_ref.make_ref(name, **KW[name])
    params = ref.nominal_params(n).astype(np.float32)
    if layout == "per_lane":  # (a generator of its own: the draws below are those of "uniform")
        params = (params * (1.0 + 0.05 * np.random.default_rng([SEED, 1]).uniform(-1.0, 1.0, params.shape))).astype(np.float32)
    slo, shi, alo, ahi = ref.bounds(params.astype(np.float64))
    state = (0.5 * (slo + shi) + rng.uniform(-0.6, 0.6, slo.shape) * 0.5 * (shi - slo)).astype(np.float32)
    hidden = (rng.uniform(-1, 1, (n, ref.H)) * (20 if name.startswith("qcp") else 0.1)).astype(np.float32)
    act = (rng.uniform(0.35, 0.9, alo.shape) * ahi * rng.choice([-1, 1], alo.shape)).astype(np.float32).astype(np.float64)
    act[: n // 8] *= 1.5  # some clipped actions: zero action gradient
    act = act.astype(np.float32)
    curr = rng.integers(0, 50, n)
    if layout != "nominal":
        curr[n - N_LIMIT:] = KW[name]["max_steps"] - 1
    c = Case(ref, n, params, state, hidden, act, curr, layout != "uniform")
    dc.frozen(c._asdict())
    return c


# ------------------------------------------------------------------------------------------------------- the fp64 oracle
class Oracle(NamedTuple):
    f1: tuple          # (state [n, S (S + A)], rew [n, S + A], obs [n, O (S + A)]): central differences at relative step 1e-6 of scale
    f2: tuple          # the same at 1e-5
    scale: np.ndarray  # [n, S + A]: the state half-width or the action bound, floored at 1e-3
    done: np.ndarray   # [n] bool: the oracle's done flag of the unperturbed step
    clipped: np.ndarray  # [n] bool: every action of the lane lies outside its box


@functools.lru_cache(maxsize=None)
def oracle(name, layout):
    """central differences of cpu_ref.step in fp64 with respect to (s, a), the hidden state held, every array flattened to
    [n, positions] with position = i (S + A) + k"""
    c = case(name, layout)
    ref, n = c.ref, c.n
    S, A, O = ref.S, ref.A, ref.O
    P, hidden = c.params.astype(np.float64), c.hidden.astype(np.float64)
    _, shi, _, ahi = ref.bounds(P)
    x0 = np.concatenate([c.state, c.act], axis=1).astype(np.float64)
    scale = np.concatenate([np.maximum(np.abs(shi), 1e-3), np.maximum(np.abs(ahi), 1e-3)], axis=1)

    def fd(eps_rel):
        js, jr, jo = np.zeros((n, S, S + A)), np.zeros((n, S + A)), np.zeros((n, O, S + A))
        for k in range(S + A):
            h_ = eps_rel * scale[:, k]
            outs = []
            for sgn in (+1, -1):
                x = x0.copy()
                x[:, k] += sgn * h_
                outs.append(ref.step(x[:, :S], hidden, x[:, S:], P, c.curr))
            js[:, :, k] = (outs[0]["state"] - outs[1]["state"]) / (2 * h_[:, None])
            jr[:, k] = (outs[0]["rew"] - outs[1]["rew"]) / (2 * h_)
            jo[:, :, k] = (outs[0]["obs"] - outs[1]["obs"]) / (2 * h_[:, None])
        return js.reshape(n, -1), jr, jo.reshape(n, -1)

    done = np.asarray(ref.step(x0[:, :S], hidden, x0[:, S:], P, c.curr)["done"], dtype=bool)
    o = Oracle(fd(1e-6), fd(1e-5), scale, done, (np.abs(c.act.astype(np.float64)) > ahi).all(axis=1))
    dc.frozen({}, *o.f1, *o.f2, o.scale, o.done, o.clipped)
    return o


# --------------------------------------------------------------------------------------- the tolerance, one unit per position
class Rule(NamedTuple):
    want: np.ndarray     # [n, R NI]: the oracle at the smaller step
    smooth: np.ndarray   # [n, R NI] bool: the two step sizes agree (per position)
    live: np.ndarray     # [R NI] bool: not a null position
    exact: np.ndarray    # [R NI] bool: null, and 0.0 in every lane at both step sizes
    top: np.ndarray      # [R NI]: the largest smooth |g| of a live position, 0 for a null one
    third: np.ndarray    # [n, R NI]: 2^-23 rowmax / scale, WITHOUT K
    present: np.ndarray  # [n, R NI]: the tolerance of the rule replaced, 3e-3 |g| + 3e-4 x the largest smooth entry of the array
    present_smooth: np.ndarray  # [n, R NI] bool: the smooth mask of the rule replaced (one maximum over the array)
    tol: np.ndarray      # [n, R NI]: the tolerance; 0 on exact positions, K x third on the other null ones


def third_term(want, scale):
    """[n, R NI]: 2^-23 rowmax(lane, i) / scale[lane, k], rowmax the row's largest |g| scale"""
    n, NI = scale.shape
    g = np.abs(want).reshape(n, -1, NI)
    rowmax = (g * scale[:, None, :]).max(axis=2, keepdims=True)
    return (ULP * rowmax / scale[:, None, :]).reshape(n, -1)


def rule(g1, g2, scale, k_fp32=None):
    """the rule of the module's docstring for one array: g1, g2 [n, R NI] at the two step sizes, scale [n, NI]"""
    k_fp32 = K_FP32 if k_fp32 is None else k_fp32
    smooth = dc.smooth_per_column(g1, g2)
    null = dc.null_columns(g1, g2)
    live = ~null
    exact = null & ~g1.any(axis=0) & ~g2.any(axis=0)
    third = third_term(g1, scale)
    present_smooth = dc.smooth_global(g1, g2)
    present = 3e-3 * np.abs(g1) + 3e-4 * (np.abs(g1[present_smooth]).max() if present_smooth.any() else 1.0)
    top = np.zeros(g1.shape[1])
    tol = k_fp32 * third
    top[live] = np.where(smooth[:, live], np.abs(g1[:, live]), 0.0).max(axis=0)
    tol[:, live] += dc.tolerance_per_column(g1[:, live], smooth[:, live])
    tol[:, exact] = 0.0
    return Rule(g1, smooth, live, exact, top, third, present, present_smooth, np.minimum(tol, present))


@functools.lru_cache(maxsize=None)
def rules(name, layout, k_fp32=None):
    """(Rule of d s', of d r, of d obs') of a case"""
    o = oracle(name, layout)
    out = tuple(rule(g1, g2, o.scale, k_fp32) for g1, g2 in zip(o.f1, o.f2))
    dc.frozen({}, *[a for r in out for a in r])
    return out


def checked(r):
    """[n, R NI] bool: the entries a comparison covers: the smooth ones of a live position, every one of a null position"""
    return np.where(r.live[None, :], r.smooth, True)


def within(got, r):
    """got [n, R NI] under the rule -> (number of bad entries, [R NI]: worst error / tolerance of every position; an exact position
    is 0.0 where the entry is 0.0 and inf where it is not)"""
    err = np.abs(got - r.want)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err > 0.0, err / r.tol, 0.0)
    ratio = np.where(checked(r), ratio, 0.0)
    return int((ratio > 1.0).sum()), ratio.max(axis=0)


def within_present(got, r):
    """the rule replaced: share of bad entries among all (the test allowed 2e-3)"""
    return float((r.present_smooth & (np.abs(got - r.want) > r.present)).mean())


def ulps_beyond(got, r):
    """[n, R NI]: (err - 3e-3 |g| - 3e-4 top) / third on the checked entries, what K_FP32 has to cover: negative where the first two
    terms cover the error by themselves (exact positions left out; a row of zeros, third = 0, gives -inf or inf)"""
    err = np.abs(got - r.want) - 3e-3 * np.abs(r.want) - 3e-4 * r.top[None, :]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        u = np.where(r.third > 0.0, err / r.third, np.where(err > 0.0, np.inf, -np.inf))
    return np.where(checked(r) & ~r.exact[None, :], u, -np.inf)


def position(p, NI):
    """(i, k) of the flat position p"""
    return divmod(int(p), NI)


def report(name, layout, tag, worst, NI):
    """the worst ratio of every position, for a failure message"""
    return f"{name} {layout} d {tag}: " + ", ".join(f"{position(p, NI)} {w:.3g}" for p, w in enumerate(worst))
