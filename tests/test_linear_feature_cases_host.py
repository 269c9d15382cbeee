"""
tests/linear_feature_cases.py on the CPU alone: the rule that tests/test_gpu_linear_features.py applies to the kernels is applied here to
a float32 restatement of the kernels' expressions (emulate_value: k_rollout_lin; emulate_derivative: k_rollout_vjp_lin with one-hot
weights), every operation rounded to float32, np.exp2 for v_exp_f32, an IEEE division for v_rcp_f32, and for sincos_fast the rounded sine
and cosine of the float64 argument.  The restatement stays inside the value bound and the derivative bound at EVERY grid point (so the
reference and the stated errors alone satisfy the rule), and every listed mutant of it is refused at one grid point or more.  The
hand-written fp64 derivatives are held to torch float64 autograd at 1e-12 away from the named exclusion.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import linear_feature_cases as lc  # noqa: E402
import lin_param_grad_fp64 as host  # noqa: E402

f32 = np.float32
SCALAR_TERMS = lc.ELEM + ("const",)
# (terms, states [n, n_vis]) of every grid
GRIDS = [(SCALAR_TERMS, lc.SCALAR_STATES), (lc.PAIR_TERMS, lc.PAIRS), (lc.MULT_TERMS, lc.MULT_STATES),
         (host.EXTRA["qbb-full"][1], lc.qbb_states())]


# ------------------------------------------------------------------------------------ the kernels' expressions in float32
def _sigmoid(v):
    with np.errstate(all="ignore"):
        return f32(1.0) / (f32(1.0) + np.exp2(f32(-1.4426950408889634) * v))


def _bell(v):
    return np.exp2(f32(-0.7213475204444817) * (v * v))


def _sincos(v):
    return np.sin(v.astype(np.float64)).astype(f32), np.cos(v.astype(np.float64)).astype(f32)


def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def emulate_value(term, x, mutant=None):
    """[n, F] float32 of one term on x [n, n_vis] float32, in k_rollout_lin's expressions"""
    x = np.asarray(x, dtype=f32)
    with np.errstate(all="ignore"):
        if term == "const":
            return np.ones((x.shape[0], 1), dtype=f32)
        if isinstance(term, str):
            if term in ("sin", "cos", "sinsin", "sincos"):
                s, c = _sincos(x)
                return {"sin": s, "cos": c, "sinsin": s * s, "sincos": s * c}[term]
            if term == "sign":
                zero = f32(1.0) if mutant == "sign(0) = 1" else x
                return np.where(x > 0, f32(1.0), np.where(x < 0, f32(-1.0), zero)).astype(f32)
            if term == "sig":
                out = _sigmoid(x)
                return np.where(x == f32(-104.5), f32(np.nan), out) if mutant == "sig(-104.5) = NaN" else out
            return {"identity": lambda v: v, "abs": np.abs, "squared": lambda v: v * v, "cubic": lambda v: v * v * v, "bell": _bell}[term](x)
        v = [x[:, r] for r in term[1]]
        if term[0] == "atan2":
            return np.arctan2(v[0].astype(np.float64), v[1].astype(np.float64)).astype(f32)[:, None]
        p = v[0] * v[1]
        for u in v[2:]:
            p = p * u
        return p[:, None]


def emulate_derivative(term, x, mutant=None):
    """[n, F, n_vis] float32 of one term, in k_rollout_vjp_lin's expressions with wbar = 1"""
    x = np.asarray(x, dtype=f32)
    n, n_vis = x.shape
    with np.errstate(all="ignore"):
        if term in ("const", "sign"):
            return np.zeros((n, lc.n_features(term, n_vis), n_vis), dtype=f32)
        if isinstance(term, str):
            if term in ("sin", "cos", "sinsin", "sincos"):
                s, c = _sincos(x)
                d = {"sin": c, "cos": s if mutant == "cos' sign" else -s,
                     "sinsin": s * c if mutant == "sinsin' factor 2" else f32(2.0) * (s * c), "sincos": c * c - s * s}[term]
            elif term == "sig":
                sg = _sigmoid(x)
                d = sg * (f32(1.0) - sg)
            elif term == "bell":
                d = (x if mutant == "bell' sign" else -x) * _bell(x)
            elif term == "cubic":
                d = f32(3.0) * (x * x)
                d = (d * f32(1.001)) if mutant == "cubic' 1.001" else d
            elif term == "abs":
                zero = f32(1.0) if mutant == "|v|'(0) = 1" else f32(0.0)
                d = np.where(x > 0, f32(1.0), np.where(x < 0, f32(-1.0), zero)).astype(f32)
            else:
                d = {"identity": np.ones_like(x), "squared": f32(2.0) * x}[term]
            out = np.zeros((n, n_vis, n_vis), dtype=f32)
            for k in range(n_vis):
                out[:, k, k] = d[:, k]
            return out
        out = np.zeros((n, 1, n_vis), dtype=f32)
        idx = list(term[1])
        v = [x[:, r] for r in idx]
        if term[0] == "mult":
            seen = set()
            for r, row in enumerate(idx):
                if mutant == "mult repeated row dropped" and row in seen:
                    continue
                seen.add(row)
                p = np.ones(n, dtype=f32)
                for r2 in range(len(idx)):
                    if r2 != r or mutant == "mult includes the row":
                        p = p * v[r2]
                out[:, 0, row] = out[:, 0, row] + p
            return out
        # the scaling by one power of two, then (x, -y) / (x^2 + y^2)
        _, ex = np.frexp(np.maximum(np.abs(v[0]), np.abs(v[1])))
        ys, xs = np.ldexp(v[0], -ex).astype(f32), np.ldexp(v[1], -ex).astype(f32)
        if mutant == "atan2 unscaled":  # the kernel before library 319: wbar / (x^2 + y^2) on the rows as they are
            ex, ys, xs = 0 * ex, v[0], v[1]
        q = f32(1.0) / _fma(xs, xs, ys * ys)
        g0, g1 = np.ldexp(xs * q, -ex).astype(f32), np.ldexp(-ys * q, -ex).astype(f32)
        if mutant == "atan2 rows swapped":
            g0, g1 = g1, g0
        if mutant == "atan2 sign":
            g0, g1 = -g0, -g1
        out[:, 0, idx[0]] += g0
        out[:, 0, idx[1]] += g1
        return out


def _inside(got, ref, bound):
    """got within bound of ref entry by entry; a NaN or an infinity where the reference is finite is outside"""
    with np.errstate(all="ignore"):
        return np.abs(got.astype(np.float64) - ref) <= bound


# ----------------------------------------------------------------------------------------- the rule holds for the restatement
@pytest.mark.parametrize("g", range(len(GRIDS)), ids=["scalar", "pairs", "mult", "qbb-full"])
def test_the_float32_restatement_is_inside_both_bounds_at_every_grid_point(g):
    terms, x = GRIDS[g]
    n_excluded = 0
    for term in terms:
        ref, bound = lc.value(term, x), lc.value_errors(term, x)
        got = emulate_value(term, x)
        assert np.isfinite(ref).all() and (bound >= 0.0).all()
        assert _inside(got, ref, bound).all(), (term, x[np.argwhere(~_inside(got, ref, bound))[0][0]])
        if term in lc.EXACT_VALUE:
            assert np.array_equal(got.astype(np.float64), ref)
        dref, dbound = lc.derivative(term, x), lc.derivative_errors(term, x)
        keep = ~lc.excluded(term, x)
        n_excluded += int((~keep).sum())
        dgot = emulate_derivative(term, x)
        assert np.isfinite(dref[keep]).all() and (dbound[keep] >= 0.0).all()
        assert _inside(dgot, dref, dbound)[keep].all(), (term, x[keep][np.argwhere(~_inside(dgot, dref, dbound)[keep])[0][0]])
    assert n_excluded == (4 * len(lc.PAIR_TERMS) if g == 1 else 0)  # the ONE exclusion: atan2' at the four (+-0, +-0) pairs


def test_required_points():
    """the values the issue requires, not merely bounds: of the reference (so a kernel inside the bound has them too where the bound
    is TINY-sized) and of the restatement"""
    x = np.array([[-150.0], [-104.5], [17.5], [150.0], [20.0], [-20.0], [0.0], [-0.0]], dtype=f32)
    sg, dsg = emulate_value("sig", x)[:, 0], emulate_derivative("sig", x)[:, 0, 0]
    assert (sg[:2] == 0.0).all() and (dsg[:2] == 0.0).all() and (sg[2:4] == 1.0).all() and (dsg[2:4] == 0.0).all()
    assert (emulate_value("bell", x)[4:6, 0] == 0.0).all() and (emulate_derivative("bell", x)[4:6, 0, 0] == 0.0).all()
    assert (emulate_value("sign", x)[6:, 0] == 0.0).all() and (emulate_derivative("abs", x)[6:, 0, 0] == 0.0).all()
    assert (lc.value("sign", x)[6:, 0] == 0.0).all() and (lc.derivative("abs", x)[6:, 0, 0] == 0.0).all()
    assert np.isfinite(emulate_value("sig", lc.SCALAR_STATES)).all()


# ------------------------------------------------------------------------------------------------- the fp64 derivatives
def _torch_feature(term, t):
    if term == "const":
        return torch.ones(t.shape[0], 1, dtype=t.dtype) + 0.0 * t[:, :1]
    if isinstance(term, str):
        return {"identity": lambda v: v, "sign": torch.sign, "abs": torch.abs, "squared": lambda v: v ** 2, "cubic": lambda v: v ** 3,
                "sig": torch.sigmoid, "bell": lambda v: torch.exp(-v ** 2 / 2.0), "sin": torch.sin, "cos": torch.cos,
                "sinsin": lambda v: torch.sin(v) ** 2, "sincos": lambda v: torch.sin(v) * torch.cos(v)}[term](t)
    if term[0] == "mult":
        return torch.prod(t[:, list(term[1])], dim=1, keepdim=True)
    return torch.atan2(t[:, term[1][0]], t[:, term[1][1]])[:, None]


@pytest.mark.parametrize("g", range(len(GRIDS)), ids=["scalar", "pairs", "mult", "qbb-full"])
def test_the_fp64_derivatives_are_torch_autograd(g):
    terms, x = GRIDS[g]
    for term in terms:
        t = torch.tensor(np.asarray(x, dtype=np.float64), requires_grad=True)
        phi = _torch_feature(term, t)
        ref = lc.derivative(term, x)
        keep = ~lc.excluded(term, x)
        assert np.abs(phi.detach().numpy() - lc.value(term, x)).max() <= 1e-12 * max(1.0, float(phi.detach().abs().max()))
        for f in range(phi.shape[1]):
            want, = torch.autograd.grad(phi[:, f].sum(), t, retain_graph=True)
            want = want.numpy()
            assert want.shape == ref[:, f].shape
            assert (np.abs(ref[:, f] - want)[keep] <= 1e-12 * np.maximum(1.0, np.abs(want[keep]))).all(), (term, f)
            # 0 / 0 in the definition: no value to hold a kernel to (torch's backward gives NaN or a masked 0 there, by version)
            assert np.isnan(ref[:, f][~keep]).any(axis=1).all() and (np.isnan(want[~keep]) | (want[~keep] == 0.0)).all()


# --------------------------------------------------------------------------------------------------------- the mutants
def _refused_somewhere(terms_and_x, mutant, of_value):
    hits = 0
    for terms, x in terms_and_x:
        for term in terms:
            if of_value:
                ref, bound, got = lc.value(term, x), lc.value_errors(term, x), emulate_value(term, x, mutant)
                keep = np.ones(ref.shape, dtype=bool)
            else:
                ref, bound, got = lc.derivative(term, x), lc.derivative_errors(term, x), emulate_derivative(term, x, mutant)
                keep = np.broadcast_to(~lc.excluded(term, x)[:, None, None], ref.shape)
            hits += int((~_inside(got, ref, bound) & keep).sum())
    return hits


@pytest.mark.parametrize("g", range(len(GRIDS)), ids=["scalar", "pairs", "mult", "qbb-full"])
def test_a_value_scaled_by_1_plus_1e_5_is_refused(g):
    """for EVERY term: among the points where |phi| is above 10 times its bound there is one, and the scaled value is refused at one
    of them or more"""
    terms, x = GRIDS[g]
    for term in terms:
        ref, bound = lc.value(term, x), lc.value_errors(term, x)
        at = np.abs(ref) > 10.0 * bound
        got = emulate_value(term, x).astype(np.float64) * (1.0 + 1e-5)
        for f in range(ref.shape[1]):
            assert at[:, f].any(), (term, f)
            assert (~_inside(got, ref, bound) & at)[:, f].any(), (term, f)


@pytest.mark.parametrize("mutant", ["sign(0) = 1", "sig(-104.5) = NaN"])
def test_value_mutants_are_refused(mutant):
    assert _refused_somewhere(GRIDS[:1], None, True) == 0
    assert _refused_somewhere(GRIDS[:1], mutant, True) >= 1


@pytest.mark.parametrize("mutant", ["cos' sign", "sinsin' factor 2", "bell' sign", "cubic' 1.001", "|v|'(0) = 1"])
def test_elementwise_derivative_mutants_are_refused(mutant):
    assert _refused_somewhere(GRIDS[:1], mutant, False) >= 1


@pytest.mark.parametrize("mutant", ["mult repeated row dropped", "mult includes the row", "atan2 rows swapped", "atan2 sign"])
def test_extra_term_derivative_mutants_are_refused(mutant):
    """on the grid of the kind, and on the ball balancer's 128-slot stack"""
    at = GRIDS[2:3] if mutant.startswith("mult") else GRIDS[1:2]
    assert _refused_somewhere(at, None, False) == 0
    assert _refused_somewhere(at, mutant, False) >= 1
    assert _refused_somewhere(GRIDS[3:], mutant, False) >= 1


def test_the_unscaled_atan2_gradient_is_refused_at_the_small_magnitudes():
    """what k_rollout_vjp_lin computed before library 319: at (y, x) = (1e-20, 0) x^2 + y^2 = 1e-40 is below the normal range and
    1 / 1e-40 overflows, (NaN, -inf) for the gradient (0, -1e20); it is refused at the pairs of magnitude 1e-20 and nowhere else"""
    term, x = lc.PAIR_TERMS[0], lc.PAIRS
    bad = ~_inside(emulate_derivative(term, x, "atan2 unscaled"), lc.derivative(term, x), lc.derivative_errors(term, x))[:, 0]
    bad = bad.any(axis=1) & ~lc.excluded(term, x)
    at = np.flatnonzero((x[:, 0] == f32(1e-20)) & (x[:, 1] == 0.0))
    assert bad[at].all() and at.size == 2 and bad.sum() >= 2
    assert (np.abs(x[bad]).max(axis=1) == f32(1e-20)).all()


# ----------------------------------------------------------------------------------------------------------- the grids
def test_the_grids_hold_every_edge_by_value():
    g = lc.SCALAR
    assert g.dtype == np.float32 and lc.SCALAR_STATES.shape == (g.size, 2) and 5000 <= g.size <= 12000
    has = lambda v: bool((g == f32(v)).any())  # noqa: E731
    assert (g == 0.0).sum() == 2 and np.signbit(g[g == 0.0]).sum() == 1                      # 0.0 and -0.0
    assert has(1e-30) and has(-1e-30)
    assert ((g == 0.0) | (np.abs(g) >= np.finfo(f32).tiny)).all()                            # no subnormal observation
    uni = np.linspace(-8.0, 8.0, 4096).astype(f32)
    assert np.isin(uni, g).all()
    assert has(1e-6) and has(-1e-6) and has(1e3) and has(-1e3) and (np.abs(g) <= f32(318.5 * np.pi) + 1.0).all()
    for lo in 10.0 ** np.arange(-6, 3):                                                      # every decade, both signs
        assert ((g > lo) & (g < 10 * lo)).sum() >= 30 and ((g < -lo) & (g > -10 * lo)).sum() >= 30
    for k in lc.PI_KS:
        for c in (k * np.pi, (k + 0.5) * np.pi):
            for sgn in (1.0, -1.0):
                if c == 0.0:
                    continue
                mid = f32(sgn * c)
                p = mid
                q = mid
                assert has(mid)
                for _ in range(3):
                    p, q = np.nextafter(p, f32(np.inf)), np.nextafter(q, f32(-np.inf))
                    assert has(p) and has(q), (k, c)
    for v in lc.SIG_TAILS + lc.BELL_TAILS:
        assert has(v) and has(-v)
    assert lc.SIG_TAILS == (16.5, 17.5, 87.0, 88.5, 89.0, 103.0, 104.5, 150.0) and lc.BELL_TAILS == (13.0, 14.3, 14.6, 20.0)
    assert lc.PI_KS == (0, 1, 2, 3, 4, 20, 318)
    # ---- pairs: eight directions x independent magnitudes, the signed zeros, the division probes
    p = lc.PAIRS
    pairs = {(float(a), float(b)) for a, b in p}
    mags = [float(f32(m)) for m in (1e-20, 1e-3, 1.0, 1e3)]
    for my in mags:
        for mx in mags:
            for sy in (1.0, -1.0):
                for sx in (1.0, -1.0):
                    assert (sy * my, sx * mx) in pairs
        for sgn in (1.0, -1.0):
            assert (sgn * my, 0.0) in pairs and (0.0, sgn * my) in pairs
    zero = p[lc.ZERO_PAIRS]
    assert zero.shape == (4, 2) and {(bool(np.signbit(a)), bool(np.signbit(b))) for a, b in zero} == {(False, False), (False, True),
                                                                                                       (True, False), (True, True)}
    want = np.arctan2(zero[:, 0].astype(np.float64), zero[:, 1].astype(np.float64))
    assert np.array_equal(lc.value(("atan2", (0, 1)), zero)[:, 0], want) and set(np.round(want, 6)) == {0.0, 3.141593, -3.141593}
    assert lc.DIV_PROBES.sum() == 64 and (p[lc.DIV_PROBES, 0] == 1.0).all()
    # ---- mult: products of 2, 3 and 4 rows, a row named twice and three times, magnitudes in [1e-6, 1e2], an exact zero
    sizes = {len(t[1]) for t in lc.MULT_TERMS}
    counts = {max(t[1].count(r) for r in set(t[1])) for t in lc.MULT_TERMS}
    assert sizes == {2, 3, 4} and {2, 3} <= counts
    m = np.abs(lc.MULT_STATES[:512])
    assert (m >= 1e-6).all() and (m <= 1e2).all() and (lc.MULT_STATES[512:] == 0.0).any(axis=1).all()
    for t in lc.MULT_TERMS:
        prod = np.abs(lc.value(t, lc.MULT_STATES[:512]))
        assert (prod >= np.finfo(f32).tiny).all()                                            # no product underflows
    # ---- the ball balancer's lanes: inside the box, no (0, 0) pair in any atan2 term of the full stack
    q = lc.qbb_states()
    assert q.shape == (256, 8) and (np.abs(q) <= 0.9 * lc.QBB_BOX).all() and ((q == 0.0).sum(axis=1) <= 1).all()
    assert (q == 0.0).any(axis=0).all() and len(host.EXTRA["qbb-full"][1]) == 51
