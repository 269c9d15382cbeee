"""
The fp64 reference of vs_lin_param_grad (lin_param_grad_fp64), its error bound (error_bound, feature_errors), the cases and their
cotangents.  Not a test module: import it by bare name.

The reference is sum_rows abar (x) phi(x) with the NumPy feature stack closed_loop_cases.features (imported, not copied); test_lin_param_grad_host
holds it to torch.autograd.grad of the .double() LinearPolicy at 1e-12 for every case stack.

Cases: the stacks of closed_loop_cases.LINEAR_CASES that the sweep's oracle test runs (between them all 14 kinds, an obs_idx view, A = 2), plus
  qbb-full       11 elementwise kinds x 8 rows + const + 39 MultFeat / ATan2Feat terms = 128 features: both slot halves of an action
                 row and the last extra-term slot
  qq-su-shuffled a stack given in an order that is not the kernel's slot order (const, a product, sin, identity)
The rows of a case here are the fp64 oracle's closed loop of that case (closed_loop_cases.closed_loop: 150 lanes x 24 steps, lanes
0 .. 9 ending early), rounded to float32; the GPU test runs the same stacks, weights and cotangents on the handle's own records.

Cotangents: abar = (0.6 + 0.25 xi) / (N T) with xi standard normal, fixed seed -- NOT zero-mean.  With zero-mean cotangents the
gradient of a column is a random walk over the rows and a column may cancel to within twenty bounds of zero, where the 1.05 mutation
cannot be told from rounding; a mean away from zero keeps most columns' sums at the size of their terms (the bound is 5e-6 to 8e-6 of
an action row's largest gradient here, 5e-5 to 8e-4 with zero-mean draws of the same seed, which happen to pass the rule too).  The
choice was made on the reference alone, before any kernel result; the rule of test_the_bound_resolves_a_mutated_column is the issue's,
unchanged.  The 1 / (N T) is the recurrent tests' scaling (gradients of order one).
"""
import functools
import types

import numpy as np
import torch

import simurlacra_amd as vs
import closed_loop_cases as clc  # (the linear cases, features, closed_loop)
from derivative_cases import N, T, frozen, lengths_of

U = 2.0 ** -24            # unit roundoff of fp32
EPS_SINCOS = 4e-7         # sincos_fast's stated absolute error
EPS_SIG = 4e-7            # the sigmoid's (v_exp_f32 + bare v_rcp_f32), see error_bound
# The project states no figure for the two below: each is TWICE the worst absolute error measured on the MI355X against fp64 over the
# cases' observations (profiles/lin_feature_errors.py -> profiles/lin_feature_errors.txt)
EPS_BELL = 2.0 * 5.75e-8  # exp2f(-0.72134752 (v v)): measured 5.747e-08
EPS_ATAN2 = 2.0 * 3.02e-7  # the device library's atan2f: measured 3.015e-07

ELEM11 = ("identity", "sign", "abs", "squared", "cubic", "sig", "bell", "sin", "cos", "sinsin", "sincos")
# 39 extra terms on the 8 rows of the ball balancer: products of 2, 3 and 4 rows and angles, the last slot (89 + 38) an ATan2Feat
FULL_X = tuple(("mult", (i, (i + 1) % 8)) for i in range(8)) + tuple(("mult", (i, (i + 2) % 8, (i + 5) % 8)) for i in range(8)) + \
    tuple(("mult", (i, (i + 3) % 8, i, (i + 4) % 8)) for i in range(8)) + tuple(("atan2", (i, (i + 4) % 8)) for i in range(8)) + \
    tuple(("mult", (i, i)) for i in range(6)) + (("atan2", (6, 1)),)
EXTRA = {
    "qbb-full": ("qbb", ELEM11 + ("const",) + FULL_X, None),
    "qq-su-shuffled": ("qq-su", ("const", ("mult", (4, 5)), "sin", "identity"), None),
}
TABLE = list(clc.LINEAR_ORACLE_CASES) + ["qbb-full"]
ALL_CASES = TABLE + ["qq-su-shuffled"]


@functools.lru_cache(maxsize=None)
def case(key):
    """the linear sweep's case for its own keys; the same draws (seed 29) and the same weight rule for the stacks of EXTRA (no cotangents)"""
    return clc.case(key) if key in clc.LINEAR_CASES else clc.linear_case(*EXTRA[key], cotangents=False)


def abar_of(key, n=N, t=T, seed=0):
    """[n, t, A] float32 (module docstring: not zero-mean, of order 1 / (n t))"""
    A = case(key)["ref"].A
    return ((0.6 + 0.25 * np.random.default_rng(2000 + seed).normal(size=(n, t, A))) / (n * t)).astype(np.float32)


def ld_of(n):
    """the handle's leading dimension: the lane count rounded up to 256"""
    return -(-n // 256) * 256


# ------------------------------------------------------------------------------------------------- the fp64 reference
def feature_errors(terms, x):
    """e(phi) [n, F]: absolute error bound of every feature of features(terms, x) as the kernel evaluates it (see error_bound)"""
    s, c = np.sin(x), np.cos(x)
    zero = np.zeros_like(x)
    elem = {"identity": zero, "sign": zero, "abs": zero, "squared": U * x ** 2, "cubic": 2.0 * U * np.abs(x) ** 3,
            "sig": zero + EPS_SIG, "bell": zero + EPS_BELL, "sin": zero + EPS_SINCOS, "cos": zero + EPS_SINCOS,
            "sinsin": 2.0 * np.abs(s) * EPS_SINCOS + EPS_SINCOS ** 2 + U * s * s,
            "sincos": (np.abs(s) + np.abs(c)) * EPS_SINCOS + EPS_SINCOS ** 2 + U * np.abs(s * c)}
    cols = []
    for t in terms:
        if t == "const":
            cols.append(np.zeros((x.shape[0], 1)))
        elif isinstance(t, str):
            cols.append(elem[t])
        elif t[0] == "mult":
            cols.append((len(t[1]) - 1) * U * np.abs(np.prod(x[:, list(t[1])], axis=1, keepdims=True)))
        else:
            cols.append(np.full((x.shape[0], 1), EPS_ATAN2))
    return np.concatenate(cols, axis=1)


def error_bound(terms, x, ab, abs_sum, chain):
    """First-order bound of |kernel - fp64| per parameter, [A, F]; u = 2^-24, gamma(m) = m u:

        bound[j][q] = sum_rows |abar_j| e(phi_q) + gamma(chain) sum_rows |abar_j phi_q|

    The recorded observation and abar are the kernel's own fp32 inputs: exact.  A row's term abar phi is formed INSIDE the
    accumulating FMA, so it has no rounding of its own: it errs by |abar| e(phi_q), e the absolute error of the feature as
    k_lin_param_grad (= k_rollout_lin) evaluates it:
      identity, sign, abs, const   exact
      squared   v v: one rounding, u x^2;   cubic  (v v) v: two, 2 u |x|^3
      sin, cos  sincos_fast's stated 4e-7
      sinsin    s s of the computed sine: 2 |s| 4e-7 + (4e-7)^2 and one rounding u s^2;  sincos likewise (|s| + |c|) 4e-7 + .. + u |s c|
      sig       4e-7 for every finite x: v_exp_f32 and v_rcp_f32 are 1 ulp each and the argument's rounding adds |x| log2(e) u relative to
                the exponential t, so the error is y (1 - y) (1.44 |x| + 3) u + 2 u y, and y (1 - y) (1.44 |x| + 3) < 0.9 on the whole axis
                (its maximum is near |x| = 1): below 3 u = 1.8e-7
      mult      a product of m rows: m - 1 roundings, (m - 1) u |product|
      bell, atan2  no stated figure: EPS_BELL and EPS_ATAN2 above, twice the worst measured error
    The sum of a parameter's terms is one FMA per live row in a wave's register (at most 64 rows per tile of the wave's run), then
    k_fnn_param_reduce's adds across the workgroups' rows and one more under accumulate: `chain` operations (param_grad_cases.chain_of, read off the
    launch's grid rule), each rounding a partial sum that is at most sum |term|."""
    return np.abs(ab).T @ feature_errors(terms, x) + chain * U * abs_sum


def lin_param_grad_fp64(terms, obs_idx, obs, abar, inside, chain=None):
    """The sum the kernel computes, restated in fp64: obs [R, O] recorded observations, abar [R, A], inside [R] bool (t < L of the row's
    lane).  Returns (gradient [A, F] -- torch's net.weight layout, stack order --, sum over the rows of |term| [A, F]) and, with
    chain, the bound of error_bound [A, F]."""
    rows = np.flatnonzero(inside)
    x = obs[rows].astype(np.float64)
    x = x if obs_idx is None else x[:, list(obs_idx)]
    ab = abar[rows].astype(np.float64)
    phi = clc.features(terms, x)
    abs_sum = np.abs(ab).T @ np.abs(phi)
    out = (ab.T @ phi, abs_sum)
    return out if chain is None else out + (error_bound(terms, x, ab, abs_sum, chain),)


@functools.lru_cache(maxsize=None)
def oracle_rows(key):
    """(obs [T N, O] float32, inside [T N], abar [T N, A] float32) of the case's fp64 closed loop, step-major: the rows of the host
    tests (the GPU test takes the handle's own records instead)"""
    c = case(key)
    A = c["ref"].A
    roll = clc.closed_loop(c["ref"], c["params"].astype(np.float64), c["init"].astype(np.float64), c["h0"], clc.policy_of(c), np.zeros((N, T, A)))
    length = lengths_of(roll.done)
    inside = np.arange(T)[:, None] < length[None, :]
    obs = roll.obs[:T].astype(np.float32)
    return frozen(dict(obs=obs.reshape(T * N, -1), inside=inside.reshape(-1), abar=abar_of(key).transpose(1, 0, 2).reshape(T * N, A)))


_FEATS = {"identity": "identity_feat", "sign": "sign_feat", "abs": "abs_feat", "squared": "squared_feat", "cubic": "cubic_feat",
          "sig": "sig_feat", "bell": "bell_feat", "sin": "sin_feat", "cos": "cos_feat", "sinsin": "sinsin_feat", "sincos": "sincos_feat",
          "const": "const_feat"}


def feature_stack(terms):
    return vs.FeatureStack(*[getattr(vs, _FEATS[t]) if isinstance(t, str) else vs.MultFeat(tuple(t[1])) if t[0] == "mult"
                             else vs.ATan2Feat(*t[1]) for t in terms])


def linear_policy(key, dtype=torch.float64):
    """the case's LinearPolicy on the rows it sees (under obs_idx the spec of the view)"""
    c = case(key)
    n_vis = c["ref"].O if c["obs_idx"] is None else len(c["obs_idx"])
    spec = types.SimpleNamespace(obs_space=types.SimpleNamespace(flat_dim=n_vis), act_space=types.SimpleNamespace(flat_dim=c["ref"].A))
    policy = vs.LinearPolicy(spec, feature_stack(c["terms"])).to(dtype)
    with torch.no_grad():
        policy.net.weight.copy_(torch.as_tensor(np.array(c["W"])).to(dtype))
    return policy


def mutations(phi, ab, q):
    """the reference with feature column q of phi [R, F] scaled by 1.05, zeroed, swapped with its neighbour -> three gradients [A, F]"""
    nb = q + 1 if q + 1 < phi.shape[1] else q - 1
    out = []
    for kind in ("scaled", "zeroed", "swapped"):
        m = phi.copy()
        if kind == "scaled":
            m[:, q] *= 1.05
        elif kind == "zeroed":
            m[:, q] = 0.0
        else:
            m[:, [q, nb]] = m[:, [nb, q]]
        out.append(ab.T @ m)
    return out
