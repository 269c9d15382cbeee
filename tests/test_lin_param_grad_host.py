"""
vs_lin_param_grad / DifferentiablePolicyRollout(param_pass=...), the parts that need no GPU: the C-ABI declaration, export and binding,
the refusals before any device call, the param_pass argument and the fp64 fallback decision -- and the fp64 NumPy reference of
tests/test_gpu_lin_param_grad.py (lin_param_grad_fp64, defined here) with its error bound (error_bound).

The reference is sum_rows abar (x) phi(x) with the NumPy feature stack closed_loop_cases.features (imported, not copied); it is held
to torch.autograd.grad of the .double() LinearPolicy at 1e-12 for every case stack.

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
import ctypes as C
import functools
import os
import re
import types

import numpy as np
import pytest

import simurlacra_amd as vs
from simurlacra_amd import _lib as L

torch = pytest.importorskip("torch")

import closed_loop_cases as clc  # noqa: E402  (the linear cases, features, closed_loop)
from derivative_cases import N, T, frozen, lengths_of  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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


# ------------------------------------------------------------------------------------------------- the launch's grid rule
def ld_of(n):
    """the handle's leading dimension: the lane count rounded up to 256"""
    return -(-n // 256) * 256


def grid_of(ld, t_steps, n_cu):
    """(workgroups, rows a wave accumulates at most) of vs_lin_param_grad's launch: workgroups of ONE wave; a wave per tile (64 lanes x
    one step) while there are fewer tiles than wave slots, else four waves per compute unit, each a contiguous run of tiles"""
    tiles = (ld // 64) * t_steps
    n_wg = min(tiles, 4 * n_cu)
    return n_wg, 64 * -(-tiles // n_wg)


def chain_of(ld, t_steps, n_cu=256, more_adds=0):
    """length of the accumulation chain of one parameter: the FMAs of a wave's run, the adds of k_fnn_param_reduce across the
    workgroups' rows (n_wg / 4 per partial sum, 2 to join the four), 1 for accumulate"""
    n_wg, acc = grid_of(ld, t_steps, n_cu)
    return acc + -(-n_wg // 4) + 2 + 1 + more_adds


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
    k_fnn_param_reduce's adds across the workgroups' rows and one more under accumulate: `chain` operations (chain_of, read off the
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


@pytest.mark.parametrize("key", ALL_CASES)
def test_the_fp64_reference_is_torch_autograd_of_the_double_policy(key):
    c, r = case(key), oracle_rows(key)
    got, abs_sum = lin_param_grad_fp64(c["terms"], c["obs_idx"], r["obs"], r["abar"], r["inside"])
    policy = linear_policy(key)
    x = r["obs"][r["inside"]].astype(np.float64)
    x = x if c["obs_idx"] is None else x[:, list(c["obs_idx"])]
    want, = torch.autograd.grad(policy(torch.as_tensor(x)), [policy.net.weight],
                                grad_outputs=torch.as_tensor(r["abar"][r["inside"]].astype(np.float64)))
    assert got.shape == tuple(want.shape) == c["W"].shape
    assert np.abs(got - want.numpy()).max() <= 1e-12 * max(1.0, np.abs(want.numpy()).max())
    assert (abs_sum >= np.abs(got) - 1e-12).all()
    if key == "qbb-full":
        assert got.shape == (2, 128)


# ------------------------------------------------------------------------------------------- the bound resolves something
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


@pytest.mark.parametrize("key", ALL_CASES)
def test_the_bound_resolves_a_mutated_column(key):
    """On the reference alone: every parameter's bound is at most 1e-2 of the largest |gradient| of its action row, and a feature
    column scaled by 1.05, zeroed or swapped with its neighbour moves its entries out of the bound -- for every entry whose gradient
    is not itself below its bound (a stack of one feature has no neighbour: the swap is skipped)."""
    c, r = case(key), oracle_rows(key)
    g, _, bound = lin_param_grad_fp64(c["terms"], c["obs_idx"], r["obs"], r["abar"], r["inside"], chain=chain_of(ld_of(N), T))
    assert (bound >= 0.0).all() and (bound <= 1e-2 * np.abs(g).max(axis=1, keepdims=True)).all(), float((bound / np.abs(g).max(axis=1, keepdims=True)).max())
    x = r["obs"][r["inside"]].astype(np.float64)
    phi = clc.features(c["terms"], x if c["obs_idx"] is None else x[:, list(c["obs_idx"])])
    ab = r["abar"][r["inside"]].astype(np.float64)
    seen = 0
    for q in range(g.shape[1]):
        for kind, m in zip(("scaled", "zeroed", "swapped"), mutations(phi, ab, q)):
            if kind == "swapped" and g.shape[1] == 1:
                continue
            for j in range(g.shape[0]):
                if np.abs(g[j, q]) < bound[j, q]:
                    continue
                seen += 1
                assert np.abs(m[j, q] - g[j, q]) > bound[j, q], (key, kind, j, q, g[j, q], m[j, q], bound[j, q])
    assert seen >= 2 * g.size  # (at most a third of the entries may be exempt)


# ------------------------------------------------------------------------------------------------------- the C-ABI
def test_header_declares_the_exact_signature():
    header = open(os.path.join(ROOT, "include", "vecsim.h")).read()
    sig = (r"int\s+vs_lin_param_grad\(vs_handle h, int t_steps, const float\* abar, float\* d_params, int64_t n_params, "
           r"int accumulate\);")
    assert re.search(sig, header)
    assert "vs_lin_param_grad" in header.split("int vs_rollout_vjp_policy(")[0].split("vs_rollout_vjp_params(")[-1]  # the sweep points to it


def test_symbol_is_exported_and_bound():
    lib = C.CDLL(L.LIB_PATH)
    assert hasattr(lib, "vs_lin_param_grad")
    assert "vs_lin_param_grad" in L.exported_symbols()
    fn = L.load().vs_lin_param_grad
    assert fn.restype is C.c_int
    assert list(fn.argtypes) == [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int]
    assert L.load().vs_version() >= 318
    assert callable(vs.VecSimEnv.lin_param_grad)


def test_null_handle_and_null_pointers_are_refused_before_a_device_is_touched():
    buf = (C.c_float * 4)()
    fn = L.load().vs_lin_param_grad
    assert fn(None, 1, buf, buf, 4, 0) == L.VS_ERR_ARG
    assert fn(None, 1, None, buf, 4, 0) == L.VS_ERR_ARG
    assert fn(None, 1, buf, None, 4, 1) == L.VS_ERR_ARG
    assert all(x == 0.0 for x in buf)


# ----------------------------------------------------------------------------------------------- the Python surface
def test_param_pass_argument_and_the_fp64_fallback():
    env = vs.QQubeSwingUpSim(dt=0.004, max_steps=30)
    stack = lambda: vs.FeatureStack(vs.identity_feat, vs.sin_feat, vs.const_feat, vs.MultFeat((0, 1)))  # noqa: E731
    policy = vs.LinearPolicy(env.spec, stack())
    roll = vs.DifferentiablePolicyRollout(env, policy)
    assert roll.param_pass == "torch" and roll._needs_rows                           # the default stays the torch pass
    roll = vs.DifferentiablePolicyRollout(env, policy, param_pass="kernel")
    assert roll.param_pass == "kernel" and not roll._needs_rows and not roll._vecs   # nothing touched a device
    for bad in ("hip", "", None, 1):
        with pytest.raises(vs.ValueErr, match="param_pass"):
            vs.DifferentiablePolicyRollout(env, policy, param_pass=bad)
    noisy = vs.NormalActNoiseExplStrat(policy, std_init=0.1)
    assert vs.DifferentiablePolicyRollout(env, noisy, param_pass="kernel").param_pass == "kernel"
    double = vs.LinearPolicy(env.spec, stack()).double()
    for asked in ("kernel", "torch"):
        roll = vs.DifferentiablePolicyRollout(env, double, param_pass=asked)        # silently: no error, no warning
        assert roll.param_pass == "torch" and roll._needs_rows and not roll._vecs


def test_lin_param_grad_without_a_linear_policy_raises():
    """as far as it is reachable without a device: the check comes before the handle is touched, so an object that has never had
    set_policy_linear called on it -- or on which another kind was set since -- raises ValueErr"""
    e = object.__new__(vs.VecSimEnv)
    with pytest.raises(vs.ValueErr, match="set_policy_linear"):
        e.lin_param_grad(4, None)
    e._lin_n_params = 0
    with pytest.raises(vs.ValueErr, match="set_policy_linear"):
        e.lin_param_grad(4, None)


def test_the_grid_rule():
    assert grid_of(256, 24, 256) == (96, 64)         # 150 lanes x 24 steps: a wave per tile
    assert grid_of(256, 1, 256) == (4, 64)
    assert grid_of(1792, 41, 256) == (1024, 128)     # 1148 tiles on 1024 waves: runs of two
    assert grid_of(1536, 41, 256) == (984, 64)       # one lane group fewer: a wave per tile
    assert chain_of(256, 24) == 64 + 24 + 2 + 1
