"""
What a device random draw is held to: its distribution and its independence.  Not a test module: the host
tests (test_random_draw_checks_host.py) and the GPU tests (test_gpu_random_draws.py) import it by bare name.

The reference draws from NumPy's global generator, so no device sample equals a reference sample; the distribution is the
specification.  A draw is first mapped back to its STANDARD VARIATE -- a number that is U(0, 1) if the draw has the distribution
the reference's space or domain parameter defines -- by the fp64 inverse maps below, written from oracle.cpu_ref (bounds,
init_bounds) and from the definitions of the parameter kinds, not from the kernels' arithmetic.  Four checks then apply, each
returning  statistic / threshold  (a ratio of at most 1 passes).  Every threshold is a non-asymptotic bound that a correct
generator exceeds with probability at most ALPHA, whatever the seed; none is tuned against a device.
"""
import math

import numpy as np

ALPHA = 1e-9  # per check
MAX_CHECKS = 1000  # checks * ALPHA <= 1e-6 per test module
_LN2A = math.log(2.0 / ALPHA)


# ------------------------------------------------------------------------------------------------------------- the four checks
def marginal(u, q=0.0):
    """Kolmogorov distance of u to U(0, 1) over the Dvoretzky-Kiefer-Wolfowitz bound sqrt(ln(2 / ALPHA) / (2 n)) + q;
    q: the quantum of the recovered variate (float32 spacing of the drawn value over the span it was recovered over)"""
    u = np.sort(np.asarray(u, dtype=np.float64).ravel())
    n = u.size
    i = np.arange(1, n + 1, dtype=np.float64)
    d = max(float((i / n - u).max()), float((u - (i - 1) / n).max()))
    return d / (math.sqrt(_LN2A / (2.0 * n)) + float(q))


def correlation(u, v):
    """|mean((u - 1/2)(v - 1/2))| over sqrt(ln(2 / ALPHA) / (8 n)): Hoeffding, terms in [-1/4, 1/4].  Holds for independent
    variates in [0, 1] of which at least one has mean 1/2."""
    u, v = np.asarray(u, dtype=np.float64).ravel(), np.asarray(v, dtype=np.float64).ravel()
    assert u.size == v.size
    return abs(float(((u - 0.5) * (v - 0.5)).mean())) / math.sqrt(_LN2A / (8.0 * u.size))


def cells_of(u, K=8):
    return np.minimum((np.asarray(u, dtype=np.float64) * K).astype(np.int64), K - 1)


def joint_cells(u, v, K=8, pu=None, pv=None):
    """every cell frequency of the K x K grid against its probability (1 / K^2; pu[a] pv[b] for variates that are not
    uniform, such as atoms) over sqrt(ln(2 K^2 / ALPHA) / (2 n)): Hoeffding per cell, union bound over the cells"""
    u, v = np.asarray(u, dtype=np.float64).ravel(), np.asarray(v, dtype=np.float64).ravel()
    assert u.size == v.size
    n = u.size
    freq = np.bincount(cells_of(u, K) * K + cells_of(v, K), minlength=K * K) / n
    pu = np.full(K, 1.0 / K) if pu is None else np.asarray(pu, dtype=np.float64)
    pv = np.full(K, 1.0 / K) if pv is None else np.asarray(pv, dtype=np.float64)
    dev = float(np.abs(freq - np.outer(pu, pv).ravel()).max())
    return dev / math.sqrt(math.log(2.0 * K * K / ALPHA) / (2.0 * n))


def frequency_usable(n, p):
    return n * p > 0 and 3.0 * _LN2A / (n * p) <= 1.0


def frequency(count, n, p):
    """|count / (n p) - 1| over the multiplicative Chernoff bound sqrt(3 ln(2 / ALPHA) / (n p)), used only where that is <= 1"""
    assert frequency_usable(n, p), (n, p)
    return abs(count / (n * p) - 1.0) / math.sqrt(3.0 * _LN2A / (n * p))


def Phi(z):
    import torch

    z = torch.as_tensor(np.asarray(z, dtype=np.float64))
    return (0.5 * (1.0 + torch.erf(z / math.sqrt(2.0)))).numpy()


TAIL3 = 2.0 * (1.0 - 0.5 * (1.0 + math.erf(3.0 / math.sqrt(2.0))))  # P(|z| > 3)


# --------------------------------------------------------------------------------------------------------------- bookkeeping
class Book:
    """counts the checks of a test module and keeps the worst ratio per (purpose, check)"""

    def __init__(self):
        self.n = 0
        self.worst = {}

    def hold(self, purpose, check, ratio, what=""):
        self.n += 1
        key = (purpose, check)
        self.worst[key] = max(self.worst.get(key, 0.0), float(ratio))
        assert ratio <= 1.0, f"{purpose} / {check} {what}: {ratio:.3f} x its bound"
        return ratio

    def assert_budget(self):
        assert self.n <= MAX_CHECKS and self.n * ALPHA <= 1e-6, self.n

    def report(self):
        rows = [f"{p:<14s} {c:<12s} worst ratio {r:.3f}" for (p, c), r in sorted(self.worst.items())]
        return "\n".join(rows + [f"checks: {self.n} (x ALPHA = {self.n * ALPHA:.2e})"])


def digest_header(version):
    """first line of profiles/random_draw_digest.txt: the library version and the commit of the tree under test (VS_COMMIT where
    the tree travels without its history)"""
    import os
    import subprocess

    commit = os.environ.get("VS_COMMIT")
    if not commit:
        try:
            commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=os.path.dirname(os.path.abspath(__file__)),
                                    capture_output=True, text=True, timeout=10).stdout.strip()
        except OSError:
            commit = ""
    return (f"random-draw digest: vs_version() = {version}, commit {commit or 'unknown'}; worst ratio statistic / bound per "
            "(purpose, check) of tests/test_gpu_random_draws.py")


class Var:
    """One recovered variate per (step or episode, lane): u [T, n] in [0, 1].
    probs None: continuous, U(0, 1) under the specification, known to the quantum q.  Otherwise u sits on atoms and probs [8] are
    the probabilities of the eight cells of [0, 1) (the variate keeps mean 1/2, which `correlation` needs of one partner).
    atoms: [(label, indicator [T, n], probability)] for `frequency`; cont: (mask, u_cond, q) the continuous part of a mixed draw,
    conditional on not being at an atom; z [T, n]: the standard normal behind u, for the tail frequency."""

    def __init__(self, name, u, q=0.0, probs=None, atoms=(), cont=None, z=None):
        self.name, self.u, self.q, self.probs, self.atoms, self.cont, self.z = name, np.asarray(u, dtype=np.float64), q, probs, atoms, cont, z
        assert self.u.ndim == 2 and (self.u >= 0).all() and (self.u <= 1).all(), name

    def rows(self, sl):
        return Var(self.name, self.u[sl], self.q, self.probs, [(a, i[sl], p) for a, i, p in self.atoms],
                   None if self.cont is None else (self.cont[0][sl], self.cont[1][sl], self.cont[2]),
                   None if self.z is None else self.z[sl])


def hold_marginal(book, purpose, v, what):
    if v.probs is None:
        book.hold(purpose, "marginal", marginal(v.u, v.q), f"{v.name} {what}")
    for label, ind, p in v.atoms:
        if frequency_usable(ind.size, p):
            book.hold(purpose, "frequency", frequency(int(ind.sum()), ind.size, p), f"{v.name} {label} {what}")
    if v.cont is not None:
        mask, uc, q = v.cont
        book.hold(purpose, "marginal", marginal(uc[mask], q), f"{v.name} inside the clip {what}")
    if v.z is not None and frequency_usable(v.z.size, TAIL3):
        book.hold(purpose, "frequency", frequency(int((np.abs(v.z) > 3.0).sum()), v.z.size, TAIL3), f"{v.name} |z| > 3 {what}")


def hold_pair(book, purpose, a, b, ua, ub, what):
    """correlation and joint_cells of two aligned samples ua, ub of the variates a, b (lists of variates: pooled, when all of
    a list share one cell structure)"""
    book.hold(purpose, "correlation", correlation(ua, ub), what)
    book.hold(purpose, "joint_cells", joint_cells(ua, ub, 8, a.probs, b.probs), what)


def _groups(vs):
    """the variates of a draw that stand for it between lanes, rows, seeds and shards: the continuous ones, pooled into one sample;
    where a draw has none (a category, a set index), every atomic one by itself.  (The atoms of a mixed draw are held by their
    marginals and by the pairs of dimensions; leaving them out here keeps the module inside its budget of checks.)"""
    cont = [v for v in vs if v.probs is None]
    return [cont] if cont else [[v] for v in vs]


def hold_lagged(book, purpose, vs, axis, lag, what):
    """the draw at index k against the one at k + lag along axis (0: step or episode, 1: lane).
    The pairs (k, k + lag) and (k + lag, k + 2 lag) share a variate.  `correlation` takes them all: ordered by k its terms are
    bounded martingale differences, for which Azuma's inequality gives Hoeffding's bound unchanged.  The cell indicators of
    `joint_cells` are no martingale differences, so it takes the disjoint pairs only -- k in every second block of `lag` indices --
    whose terms are independent, and evaluates its bound at their number."""
    for g in _groups(vs):
        k = np.arange(g[0].u.shape[axis] - lag)
        take = (lambda x, idx: (x[idx] if axis == 0 else x[:, idx]).ravel())
        both = lambda idx: (np.concatenate([take(v.u, idx) for v in g]), np.concatenate([take(v.u, idx + lag) for v in g]))  # noqa: E731
        tag = f"{'+'.join(v.name for v in g)} {what}"
        book.hold(purpose, "correlation", correlation(*both(k)), tag)
        book.hold(purpose, "joint_cells", joint_cells(*both(k[(k // lag) % 2 == 0]), 8, g[0].probs, g[0].probs), tag)


def hold_shifted(book, purpose, vs, ws, shift, what):
    """rows shift .. of the draws vs against rows 0 .. of the draws ws of the same lanes: two runs of one stream that should not
    overlap (a run after a seek against the run from step 0)"""
    for g, h in zip(_groups(vs), _groups(ws)):
        hold_pair(book, purpose, g[0], h[0], np.concatenate([v.u[shift:].ravel() for v in g]),
                  np.concatenate([w.u[:-shift].ravel() for w in h]), f"{'+'.join(v.name for v in g)} {what}")


def hold_against(book, purpose, vs, ws, what):
    """the draws vs against the draws ws of the same lanes and steps (another seed, another shard)"""
    for g, h in zip(_groups(vs), _groups(ws)):
        hold_pair(book, purpose, g[0], h[0], np.concatenate([v.u.ravel() for v in g]), np.concatenate([w.u.ravel() for w in h]),
                  f"{'+'.join(v.name for v in g)} {what}")


LANE_LAGS = (1, 64, 256)


def battery(book, purpose, vs, step_lags=(1,), what=""):
    """everything one handle's draws are held to: marginals (pooled and on the first row), every pair of dimensions, lanes
    against lanes, steps or episodes against later ones.  vs: the variates of one draw, each [T, n]."""
    for v in vs:
        hold_marginal(book, purpose, v, f"pooled {what}")
        hold_marginal(book, purpose, v.rows(slice(0, 1)), f"first row {what}")
    for k, a in enumerate(vs):
        for b in vs[k + 1:]:
            hold_pair(book, purpose, a, b, a.u, b.u, f"{a.name} x {b.name} {what}")
    for lag in LANE_LAGS:
        hold_lagged(book, purpose, vs, 1, lag, f"lane i x i + {lag} {what}")
    if vs[0].u.shape[0] > 1:
        for lag in sorted(set(step_lags)):
            hold_lagged(book, purpose, vs, 0, lag, f"row t x t + {lag} {what}")


# ------------------------------------------------------------------------------------------------------------ inverse maps
def spacing32(x):
    return float(np.spacing(np.float32(np.max(np.abs(x)))))


def box_variate(x, lo, hi, roundings=1):
    """x [T, n] drawn from the box [lo, hi] [n] of each lane -> (u, q).  A value may leave the box by the roundings of the
    float32 draw (asserted: that licenses reading it as a draw); q = roundings * spacing of the bound / span."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    span = hi - lo
    assert (span > 0).all()
    slack = 2.0 * roundings * np.spacing(np.maximum(np.abs(lo), np.abs(hi)).astype(np.float32)).astype(np.float64)
    assert (x >= lo - slack).all() and (x <= hi + slack).all(), "a value outside its lane's space"
    q = float((0.5 * slack / span).max())
    return np.clip((x - lo) / span, 0.0, 1.0), q


def init_variates(ref, state, params):
    """state [T, n, S]: rows of init states of the lanes with domain parameters params [n, P] (fp64) -> [Var]"""
    state = np.asarray(state, dtype=np.float64)
    if ref.name in ("bob", "bob-d"):  # CompoundSpace of two boxes that differ in the side of the ball: the side bit and u of |x|
        lo, hi = ref.init_bounds(params, 1)
        lo0, hi0 = ref.init_bounds(params, 0)
        assert np.array_equal(lo0[:, 1:], lo[:, 1:]) and np.array_equal(hi0[:, 1:], hi[:, 1:]) and np.array_equal(-hi0[:, 0], lo[:, 0])
        right = state[..., 0] > 0
        out = [Var("side", np.where(right, 0.75, 0.25), probs=_atom_probs([0.25, 0.75], [0.5, 0.5]), atoms=[("right", right, 0.5)])]
        u, q = box_variate(np.abs(state[..., 0]), lo[:, 0], hi[:, 0])
        out.append(Var("|x|", u, q))
        for j in range(1, 4):
            u, q = box_variate(state[..., j], lo[:, j], hi[:, j])
            out.append(Var(f"s{j}", u, q))
        return out
    lo, hi = ref.init_bounds(params)
    if ref.name == "qbb":  # Polar2DPosVelSpace: [r, phi, x_dot, y_dot]; the state holds r cos phi, r sin phi at 2, 3
        assert (state[..., [0, 1, 4, 5]] == 0).all()
        r, phi = np.hypot(state[..., 2], state[..., 3]), np.arctan2(state[..., 3], state[..., 2])
        # r comes back from two products r cos, r sin of rounded factors: four roundings
        ur, qr = box_variate(r, lo[:, 0], hi[:, 0], roundings=4)
        up, qp = box_variate(phi, lo[:, 1], hi[:, 1], roundings=4)
        out = [Var("r", ur, qr), Var("phi", up, qp)]
        for j, k in ((2, 6), (3, 7)):
            u, q = box_variate(state[..., k], lo[:, j], hi[:, j])
            out.append(Var(f"s{k}", u, q))
        return out
    out = []
    for j in range(ref.I):
        if (hi[:, j] > lo[:, j]).all():
            u, q = box_variate(state[..., j], lo[:, j], hi[:, j])
            out.append(Var(f"s{j}", u, q))
        else:
            assert (state[..., j] == np.float32(lo[:, j])).all()
    return out


def _atom_probs(us, ps):
    probs = np.zeros(8)
    np.add.at(probs, cells_of(np.asarray(us), 8), np.asarray(ps, dtype=np.float64))
    return probs


def action_variates(ref, act, params, normed=False):
    """act [T, n, A] drawn from the lanes' action spaces (the wrapper's [-1, 1] when normed) -> [Var]"""
    act = np.asarray(act, dtype=np.float64)
    _, _, alo, ahi = ref.bounds(params)
    if normed:
        alo, ahi = -np.ones_like(alo), np.ones_like(ahi)
    if ref.name == "bob-d":  # DiscreteSpace of three elements: the category
        eles = np.stack([alo[:, 0], 0.5 * (alo[:, 0] + ahi[:, 0]), ahi[:, 0]], axis=1)  # [n, 3]
        dist = np.abs(act[..., 0][..., None] - eles[None])
        k = dist.argmin(axis=-1)
        assert (dist.min(axis=-1) <= 2.0 * np.spacing(np.abs(ahi[:, 0]).astype(np.float32))).all(), "an action that is no element"
        us = (np.arange(3) + 0.5) / 3.0
        return [Var("category", us[k], probs=_atom_probs(us, [1 / 3.0] * 3), atoms=[(f"= {c}", k == c, 1 / 3.0) for c in range(3)])]
    out = []
    for j in range(ref.A):
        u, q = box_variate(act[..., j], alo[:, j], ahi[:, j])
        out.append(Var(f"a{j}", u, q))
    return out


def normal_variate(name, x, mean, std):
    """x [T, n] = mean + std z in float32 (mean, std scalars or [n]) -> Var of Phi(z)"""
    z = (np.asarray(x, dtype=np.float64) - mean) / std
    q = float(np.max(spacing32(x) / np.asarray(std, dtype=np.float64)))  # (the density of Phi is below 1: q bounds the quantum of u)
    return Var(name, Phi(z), q, z=z)


# the randomizer both test modules draw domain parameters with (QQube): uniform, normal, normal, uniform, normal clipped at -1 sigma, Bernoulli, rounded normal, normal, normal
PARAM_SPECS = [("motor_resistance", "uniform", 8.4, 1.0, -np.inf, np.inf),
               ("motor_back_emf", "normal", 0.042, 0.004, -np.inf, np.inf),
               ("mass_rot_pole", "normal", 0.095, 0.005, -np.inf, np.inf),
               ("length_rot_pole", "uniform", 0.085, 0.01, -np.inf, np.inf),
               ("mass_pend_pole", "normal", 0.024, 0.002, 0.022, np.inf),
               ("voltage_thold_pos", "bernoulli", 0.0, 0.1, -np.inf, np.inf, 0.3, False),
               ("gravity_const", "normal", 10.0, 2.0, -np.inf, np.inf, 0.0, True),
               ("length_pend_pole", "normal", 0.129, 0.01, -np.inf, np.inf),
               ("damping_rot_pole", "normal", 5e-6, 5e-7, -np.inf, np.inf)]


def param_variates(specs, names, P):
    """P [T, n, n_params] drawn by the randomizer `specs` (tuples as VecSimEnv._specs takes them) -> one Var per spec"""
    P = np.asarray(P, dtype=np.float64)
    out = []
    for s in specs:
        name, kind, mean, spread, lo, hi = s[:6]
        aux = float(s[6]) if len(s) > 6 else 0.0
        rnd = bool(s[7]) if len(s) > 7 else False
        x = P[..., names.index(name)]
        if kind == "uniform":
            u, q = box_variate(x, np.full(x.shape[1], mean - spread), np.full(x.shape[1], mean + spread))
            out.append(Var(name, u, q))
        elif kind == "bernoulli":  # mean = val_0, spread = val_1, aux = prob_1
            one = x == np.float32(spread)
            assert (one | (x == np.float32(mean))).all()
            us = [0.5 - aux / 2.0, 0.5 + (1.0 - aux) / 2.0]  # (indicator - prob_1) / 2 around 1/2: mean 1/2
            out.append(Var(name, np.where(one, us[1], us[0]), probs=_atom_probs(us, [1.0 - aux, aux]), atoms=[("= val_1", one, aux)]))
        elif rnd:  # rounded normal: the integer cells; symmetric about an integer mean, so Phi((k - mean) / std) keeps mean 1/2
            assert float(mean).is_integer() and np.array_equal(x, np.rint(x)) and np.isinf(lo) and np.isinf(hi)
            ks = np.arange(math.floor(mean - 8 * spread), math.ceil(mean + 8 * spread) + 1)
            pk = Phi((ks + 0.5 - mean) / spread) - Phi((ks - 0.5 - mean) / spread)
            uk = Phi((ks - mean) / spread)
            assert (x >= ks[0]).all() and (x <= ks[-1]).all()
            out.append(Var(name, Phi((x - mean) / spread), probs=_atom_probs(uk, pk), atoms=[(f"= {k}", x == k, p) for k, p in zip(ks, pk)]))
        elif np.isfinite(lo) or np.isfinite(hi):  # normal clipped from below: the mass at the clip and the truncated rest
            assert np.isfinite(lo) and np.isinf(hi)
            c = float(Phi((lo - mean) / spread))
            at = x <= np.float32(lo)
            assert (x >= np.float32(lo)).all()
            nv = normal_variate(name, x, mean, spread)
            # for the pair checks: the atom sits at c / 2, the mean of Phi(z) below the clip, so the variate keeps mean 1/2
            edges = np.arange(9) / 8.0
            probs = np.clip(edges[1:], c, 1.0) - np.clip(edges[:-1], c, 1.0) + _atom_probs([c / 2.0], [c])
            out.append(Var(name, np.where(at, c / 2.0, nv.u), probs=probs, atoms=[("at the clip", at, c)],
                           cont=(~at, np.clip((nv.u - c) / (1.0 - c), 0.0, 1.0), nv.q / (1.0 - c))))
        else:
            out.append(normal_variate(name, x, mean, spread))
    return out


def set_index_variate(k, B):
    """k [T, n]: the set of a buffer of B <= 8 sets a lane took, uniform over the buffer"""
    us = (np.arange(B) + 0.5) / B
    assert ((k >= 0) & (k < B)).all()
    return Var("set", us[k], probs=_atom_probs(us, [1.0 / B] * B), atoms=[(f"= {c}", k == c, 1.0 / B) for c in range(B)])
