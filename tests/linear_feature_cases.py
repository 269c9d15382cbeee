"""
The linear policy's 14 feature kinds, point by point: the grids, the fp64 definitions of every feature and of its derivative with respect
to every observation row, and the error bounds that tests/test_gpu_linear_features.py holds k_rollout_lin (values) and k_rollout_vjp_lin
(derivatives) to.  tests/test_linear_feature_cases_host.py shows on the CPU alone that a float32 restatement of the kernels' expressions
stays inside the bounds at every grid point and that the listed mutants do not.  Not a test module: import it by bare name.

Grids (float32 values; every reference is fp64 ON exactly those values):
  SCALAR   0.0, -0.0, +-1e-30; 4096 points uniform on [-8, 8]; 40 magnitudes per decade from 1e-6 to 1e3, both signs (1e3 is the range
           the kernel comment states for sincos_fast); the fp32 neighbours at 0, +-1, +-2, +-3 ulp of +-k pi and +-(k + 1/2) pi for
           k in {0 .. 4, 20, 318}; the sigmoid tails +-{16.5, 17.5, 87, 88.5, 89, 103, 104.5, 150}; the bell tails +-{13, 14.3, 14.6, 20}.
           NO subnormal observation: whether the device flushes subnormals is not part of the contract (so 0 pi has no ulp neighbours
           here: they are subnormal).  On the oscillator row 0 holds the grid and row 1 the grid reversed.
  PAIRS    (y, x) for atan2: the eight directions (four axes, each with the other coordinate +0 and -0; four diagonals) with the
           magnitudes {1e-20, 1e-3, 1, 1e3} chosen independently per coordinate; the four sign combinations of (+-0, +-0), where the
           reference is np.arctan2 (IEEE: +-pi against -0, +-0 against +0); and DIV_PROBES, (1, m) for m = 2 .. 65: x^2 + y^2 = 1 + m^2 is
           exact in fp32 and d atan2 / d x = -1 / (1 + m^2) is then ONE fp32 division and nothing else, which is how the division of the
           project's compile flags is measured through the kernel.
  MULT     MULT_TERMS: products of 2, 3 and 4 rows of the oscillator's two, with rows named twice and three times; 512 lanes of
           magnitudes log-uniform in [1e-6, 1e2] with random signs (no product of four underflows), then lanes with an exact zero in
           row 0, in row 1 and in both.

Exclusions: exactly one -- the atan2 DERIVATIVE at the four (+-0, +-0) pairs (0 / 0 in the definition; torch's backward gives NaN or a
masked 0 there, by version); excluded() names them and the tests count them.  No other entry is left out and no share of bad entries
is allowed.

Bounds.  Values: lin_param_grad_fp64.feature_errors as it stands for identity, sign, abs, squared, cubic, sig, sin, cos, sinsin,
sincos, mult and const; the bell and atan2 from the figures measured on THIS grid (below).  Derivatives: derivative_errors, derived in
its docstring.  Both get one term feature_errors does not have: a result below the normal range is rounded to a subnormal or flushed,
either way an absolute error of at most TINY = 2^-126 per operation (squared(1e-30) = 1e-60 is 0 in fp32 in either mode); it is added to
every bound that is not 0, and is 1.2e-38.

The three figures the project does not state: worst |device - fp64| over this grid on the MI355X, library
version MEASURED["library"]; the bounds use TWICE each (the margin EPS_BELL and EPS_ATAN2 of lin_param_grad_fp64 were given: one
measurement on a finite grid).
  bell    exp2f(-0.72134752 (v v)): BELL_ABS absolute, BELL_ULPS in ulps of |reference|.  The bound is the absolute figure: in the tail the
          rounding of the exponent's argument alone is |arg| u ln 2 relative (hundreds of ulps at |v| = 13), so the ulps figure is a
          record, not a bound.
  atan2f  the device library's: ATAN2_ABS absolute, ATAN2_ULPS in ulps of |reference|; the bound is the smaller of twice each, so a
          reference of 1e-23 (y = 1e-20, x = 1e3) is held relatively and atan2(+0, x > 0) = 0 exactly.  6 ulp is the OpenCL limit; a figure
          above it would be a finding, not a constant (asserted).
  a / b   the fp32 division: DIV_ULPS, over DIV_PROBES.
"""
import numpy as np

from closed_loop_cases import features  # (the fp64 values)
import lin_param_grad_fp64 as host  # (feature_errors, U, EPS_SIG, EPS_SINCOS, EXTRA)

U, EPS_SIG, EPS_SINCOS = host.U, host.EPS_SIG, host.EPS_SINCOS
TINY = 2.0 ** -126
ELEM = host.ELEM11
EXACT_VALUE = ("identity", "sign", "abs", "const")  # bit-equal, not merely inside a bound

# worst |device - fp64| on the MI355X over the grids of this module (tests/test_gpu_linear_features.py -s prints them)
MEASURED = dict(library=319, n_scalar=None, n_pairs=None, n_div_probes=64)
BELL_ABS, BELL_ULPS = 4.99e-8, 77.0      # measured 4.983e-08, 77.0
ATAN2_ABS, ATAN2_ULPS = 1.60e-7, 1.11    # measured 1.596e-07, 1.10
DIV_ULPS = 0.5                           # measured 0.50: the division is IEEE's under the project's flags
ATAN2_ULPS_LIMIT = 6.0  # OpenCL's

SIG_TAILS = (16.5, 17.5, 87.0, 88.5, 89.0, 103.0, 104.5, 150.0)
BELL_TAILS = (13.0, 14.3, 14.6, 20.0)
PI_KS = (0, 1, 2, 3, 4, 20, 318)
PAIR_MAGS = (1e-20, 1e-3, 1.0, 1e3)


# --------------------------------------------------------------------------------------------------------------- the grids
def _frozen(a):
    a.setflags(write=False)
    return a


def pi_neighbours():
    """the fp32 neighbours at 0, +-1, +-2, +-3 ulp of +-k pi and +-(k + 1/2) pi, k in PI_KS (not of 0: its neighbours are subnormal)"""
    out = []
    for k in PI_KS:
        for c in (k * np.pi, (k + 0.5) * np.pi):
            if c == 0.0:
                continue
            for sgn in (1.0, -1.0):
                mid = np.float32(sgn * c)
                up, dn = [mid], [mid]
                for _ in range(3):
                    up.append(np.nextafter(up[-1], np.float32(np.inf)))
                    dn.append(np.nextafter(dn[-1], np.float32(-np.inf)))
                out += up + dn[1:]
    return np.array(out, dtype=np.float32)


def scalar_grid():
    mags = (10.0 ** np.linspace(-6.0, 3.0, 361)).astype(np.float32)
    mags[-1] = np.float32(1e3)
    tails = np.array(SIG_TAILS + BELL_TAILS, dtype=np.float32)
    g = np.concatenate([np.array([0.0, -0.0, 1e-30, -1e-30], dtype=np.float32), np.linspace(-8.0, 8.0, 4096).astype(np.float32),
                        mags, -mags, pi_neighbours(), tails, -tails])
    assert g.dtype == np.float32 and ((g == 0.0) | (np.abs(g) >= np.finfo(np.float32).tiny)).all()  # no subnormal
    return _frozen(g)


SCALAR = scalar_grid()
SCALAR_STATES = _frozen(np.stack([SCALAR, SCALAR[::-1]], axis=1))  # the oscillator's lanes: [n, 2]


def pair_grid():
    """-> (pairs [n, 2] float32 as (y, x), zero pairs [n] bool, division probes [n] bool)"""
    rows = []
    for my in PAIR_MAGS:
        for mx in PAIR_MAGS:
            rows += [(sy * my, sx * mx) for sy in (1.0, -1.0) for sx in (1.0, -1.0)]  # the four diagonals
    for m in PAIR_MAGS:
        for z in (0.0, -0.0):
            rows += [(m, z), (-m, z), (z, m), (z, -m)]                                 # the four axes
    rows += [(0.0, 0.0), (0.0, -0.0), (-0.0, 0.0), (-0.0, -0.0)]
    n_grid = len(rows)
    rows += [(1.0, float(m)) for m in range(2, 66)]
    p = np.array(rows, dtype=np.float32)
    zero = (p[:, 0] == 0.0) & (p[:, 1] == 0.0)
    return _frozen(p), _frozen(zero), _frozen(np.arange(len(rows)) >= n_grid)


PAIRS, ZERO_PAIRS, DIV_PROBES = pair_grid()
PAIR_TERMS = (("atan2", (0, 1)), ("atan2", (1, 0)))

MULT_TERMS = (("mult", (0, 1)), ("mult", (1, 1)), ("mult", (0, 1, 0)), ("mult", (1, 0, 1)), ("mult", (1, 0, 0)), ("mult", (0, 1, 1, 0)),
              ("mult", (0, 0, 1, 0)), ("mult", (1, 0, 1, 1)))


def mult_grid():
    rng = np.random.default_rng(61)
    x = (10.0 ** rng.uniform(-6.0, 2.0, (512, 2)) * rng.choice([-1.0, 1.0], (512, 2))).astype(np.float32)
    edge = np.array([(0.0, 3.5), (0.0, -1e-6), (-0.0, 1e2), (7.25, 0.0), (-1e2, -0.0), (0.0, 0.0)], dtype=np.float32)
    return _frozen(np.concatenate([x, edge]))


MULT_STATES = mult_grid()
MEASURED.update(n_scalar=int(SCALAR.size), n_pairs=int(PAIRS.shape[0]))

# the ball balancer's state box (observe(s) = s): +-pi/4, +-pi/4, +-l/2, +-l/2, +-5 pi, +-5 pi, +-0.5, +-0.5 at the nominal plate length
QBB_BOX = np.array([np.pi / 4, np.pi / 4, 0.1375, 0.1375, 5 * np.pi, 5 * np.pi, 0.5, 0.5])
QBB_LANES = 256


def qbb_states(n=QBB_LANES):
    """[n, 8] float32: per row the part of SCALAR inside 0.9 of the row's box, n of its points spread evenly over it (the zeros and
    +-1e-30 among them), in a different rotation per row so that no lane holds two zeros (no atan2 pair of the stack is (0, 0))"""
    cols = []
    for k, b in enumerate(QBB_BOX):
        part = SCALAR[np.abs(SCALAR) <= 0.9 * b]
        pick = np.concatenate([part[:4], part[4:][np.linspace(0, part.size - 5, n - 4).astype(int)]])
        cols.append(np.roll(pick, 29 * k))
    return _frozen(np.stack(cols, axis=1).astype(np.float32))


# ------------------------------------------------------------------------------------------------- the fp64 definitions
def n_features(term, n_vis):
    return n_vis if isinstance(term, str) and term != "const" else 1


def value(term, x):
    """phi [n, F] of ONE term on the visible rows x [n, n_vis] (fp64): closed_loop_cases.features"""
    with np.errstate(all="ignore"):
        return features((term,), np.asarray(x, dtype=np.float64))


def derivative(term, x):
    """d phi_f / d x_k [n, F, n_vis] of one term, by hand in fp64 (held to torch float64 autograd at 1e-12 by the host test).
    |v|' and sign' are 0 at 0 as torch has them; atan2 at (0, 0) is NaN (0 / 0): excluded()."""
    x = np.asarray(x, dtype=np.float64)
    n, n_vis = x.shape
    if term == "const":
        return np.zeros((n, 1, n_vis))
    with np.errstate(all="ignore"):
        if isinstance(term, str):
            sg = 1.0 / (1.0 + np.exp(-x))
            s, c = np.sin(x), np.cos(x)
            d = {"identity": np.ones_like(x), "sign": np.zeros_like(x), "abs": np.sign(x), "squared": 2.0 * x, "cubic": 3.0 * x * x,
                 "sig": sg * (1.0 - sg), "bell": -x * np.exp(-x * x / 2.0), "sin": c, "cos": -s, "sinsin": 2.0 * s * c,
                 "sincos": c * c - s * s}[term]
            out = np.zeros((n, n_vis, n_vis))
            for k in range(n_vis):
                out[:, k, k] = d[:, k]
            return out
        out = np.zeros((n, 1, n_vis))
        idx = list(term[1])
        if term[0] == "mult":
            for r, row in enumerate(idx):
                out[:, 0, row] += np.prod(x[:, idx[:r] + idx[r + 1:]], axis=1)
            return out
        y, xx = x[:, idx[0]], x[:, idx[1]]
        den = xx * xx + y * y
        gy, gx = xx / den, -y / den
        if idx[0] == idx[1]:
            out[:, 0, idx[0]] = gy + gx
        else:
            out[:, 0, idx[0]], out[:, 0, idx[1]] = gy, gx
        return out


def excluded(term, x):
    """[n] bool: the points of the ONE exclusion -- the derivative of atan2 where both of its rows are (+-) 0"""
    x = np.asarray(x)
    if isinstance(term, str) or term[0] != "atan2":
        return np.zeros(x.shape[0], dtype=bool)
    return (x[:, term[1][0]] == 0.0) & (x[:, term[1][1]] == 0.0)


def ulps_of(err, ref):
    """err in units of the fp32 spacing at |ref|"""
    return np.abs(err) / np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)


# ----------------------------------------------------------------------------------------------------------- the bounds
def value_errors(term, x):
    """[n, F]: absolute error bound of one term's value as k_rollout_lin evaluates it (module docstring)"""
    x = np.asarray(x, dtype=np.float64)
    if term == "bell":
        return np.full(x.shape, 2.0 * BELL_ABS + TINY)
    if not isinstance(term, str) and term[0] == "atan2":
        ref = value(term, x)
        return np.minimum(2.0 * ATAN2_ABS, 2.0 * ATAN2_ULPS * np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64))
    with np.errstate(all="ignore"):
        e = host.feature_errors((term,), x)
    return e if term in EXACT_VALUE else e + TINY


def derivative_errors(term, x):
    """[n, F, n_vis]: first-order bound of |k_rollout_vjp_lin's derivative - fp64| per entry, with one-hot weights and the cotangent e_j,
    so that wbar = fmaf(1, 1, 0) = 1 and gx = fmaf(1, phi', 0) = phi' exactly: the error is that of the kernel's expression for phi'.
    u = 2^-24, E = EPS_SINCOS, y the sigmoid, s / c the sine / cosine, every entry + TINY unless it is 0 (module docstring):
      identity' = 1 + 0 v, sign' = const' = 0 (not computed), |v|' = +-1 or 0, squared' = 2 v          exact: 0
      cubic'    3 (v v): two roundings                                                                2 u 3 v^2
      sig'      sg (1 - sg) of the computed sigmoid, |sg - y| <= EPS_SIG: the function's slope |1 - 2 y| EPS_SIG + EPS_SIG^2, the
                subtraction's rounding u (1 - y) times y and the product's u y (1 - y)                |1 - 2y| EPS_SIG + EPS_SIG^2 + 2 u y (1 - y)
      bell'     -v bell(v), the negation exact, |bell error| <= 2 BELL_ABS, one product                |v| 2 BELL_ABS + u |v bell|
      sin'      cs: E;   cos'  -sn: E
      sinsin'   2 (s c), the doubling exact: the product of two values of error E, one rounding        2 ((|s| + |c|) E + E^2 + u |s c|)
      sincos'   c c - s s: two squares of values of error E, a rounding each, and the subtraction's     2 (|c| + |s|) E + 2 E^2 + u (c^2 + s^2) + u |c^2 - s^2|
      mult      d / d row j = the sum over the positions r that name j of prod_{r2 != r} v[r2].  The kernel forms each term as
                wbar v .. v, one rounding per multiplication (m - 1 of them for a product of m rows), and adds a row's n_j terms with
                n_j - 1 roundings of partial sums of at most sum |term|                                ((m - 1) + (n_j - 1)) u sum_r |term_r|
                A row the term does not name gets nothing added: exactly 0.
      atan2     (y, x) -> (x, -y) / (x^2 + y^2).  The kernel scales both rows by ONE power of two 2^-e, 2^e within a factor 2 of
                max(|x|, |y|) (exact, and x^2 + y^2 then lies in [1/4, 2): no underflow), den = fmaf(x, x, y y): the product's and the
                FMA's rounding, 2 u relative; q = wbar / den: the division, at most 2 DIV_ULPS ulps = 4 DIV_ULPS u relative; x q or -y q:
                one product; the scaling back exact                                                    |g| (3 + 4 DIV_ULPS) u
    """
    x = np.asarray(x, dtype=np.float64)
    n, n_vis = x.shape
    ref = derivative(term, x)
    if term in ("identity", "sign", "abs", "squared", "const"):
        return np.zeros(ref.shape)
    with np.errstate(all="ignore"):
        if isinstance(term, str):
            y = 1.0 / (1.0 + np.exp(-x))
            s, c = np.abs(np.sin(x)), np.abs(np.cos(x))
            E = EPS_SINCOS
            d = {"cubic": 2.0 * U * 3.0 * x * x,
                 "sig": np.abs(1.0 - 2.0 * y) * EPS_SIG + EPS_SIG ** 2 + 2.0 * U * y * (1.0 - y),
                 "bell": np.abs(x) * 2.0 * BELL_ABS + U * np.abs(x) * np.exp(-x * x / 2.0),
                 "sin": np.full(x.shape, E), "cos": np.full(x.shape, E),
                 "sinsin": 2.0 * ((s + c) * E + E ** 2 + U * s * c),
                 "sincos": 2.0 * (c + s) * E + 2.0 * E ** 2 + U * (c * c + s * s) + U * np.abs(c * c - s * s)}[term]
            out = np.zeros(ref.shape)
            for k in range(n_vis):
                out[:, k, k] = d[:, k] + TINY
            return out
        out = np.zeros(ref.shape)
        idx = list(term[1])
        if term[0] == "mult":
            m = len(idx)
            for j in set(idx):
                terms = [np.abs(np.prod(x[:, idx[:r] + idx[r + 1:]], axis=1)) for r, row in enumerate(idx) if row == j]
                out[:, 0, j] = ((m - 1) + (len(terms) - 1)) * U * np.sum(terms, axis=0) + m * TINY
            return out
        for j in set(idx):
            out[:, 0, j] = np.abs(ref[:, 0, j]) * (3.0 + 4.0 * DIV_ULPS) * U + TINY
        return out
