"""
k_rollout_lin and k_rollout_vjp_lin, feature by feature and point by point: every feature kind of the linear policy is read out of the
kernels through ONE-HOT weights (fmaf(1, phi, 0) is phi exactly) on the grids of tests/linear_feature_cases.py and held to the fp64
definitions there, within value_errors / derivative_errors -- at every lane, with no share of bad entries and one named exclusion
(the derivative of atan2 at the four (+-0, +-0) pairs).

The families are those whose observation is the state (asserted on the oracle): the oscillator (2 rows, linear dynamics: any finite state
steps without a non-finite Jacobian) carries the whole grids, the ball balancer (8 rows = MAXO, A = 2) the wiring of all 128 slots with
the part of the grid inside its state box.  The grid goes into the lanes with reset(init_state=...); step_policy(1, record=True) in
record mode 2 leaves the raw action of row 0, formed BEFORE the step (so a lane that leaves its box at that step does not matter);
rollout_vjp_policy(1, g_act=e_j) on that one-row record, every other cotangent NULL, has lambda = g_rew = g_obs = 0, so
d_init[:, k] = sum_slot W[j][slot] d phi_slot / d obs_k, a single derivative under one-hot weights.  Rows the feature does not depend on
must be exactly 0 and d_act[0] must be g_act.

Each test prints (-s) the worst error / bound per feature kind, and test_the_three_measured_figures the raw figures behind BELL_ABS,
ATAN2_ABS / _ULPS and DIV_ULPS: DESIGN.md section 8o.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import linear_feature_cases as lc  # noqa: E402
import lin_param_grad_fp64 as host  # noqa: E402
from derivative_cases import KW, MAX_STEPS  # noqa: E402
from oracle import cpu_ref  # noqa: E402


@pytest.fixture(scope="module")
def vs():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import simurlacra_amd

    return simurlacra_amd


class Probe:
    """a handle of one family whose lanes hold `states` [n, S] float32 (observe(s) = s, asserted on the oracle)"""

    def __init__(self, vs, name, states):
        ref = cpu_ref.make_ref(name, max_steps=MAX_STEPS, **KW[name])
        probe = np.arange(1.0, 1.0 + 3 * ref.S).reshape(3, ref.S) / 7.0
        assert ref.O == ref.S and np.array_equal(ref.observe(probe), probe)
        self.vs, self.name, self.S, self.H, self.A = vs, name, ref.S, ref.H, ref.A
        self.states = np.ascontiguousarray(states, dtype=np.float32)
        self.n = self.states.shape[0]
        assert self.states.shape == (self.n, ref.S)
        self.e = vs.VecSimEnv(name, self.n, max_steps=MAX_STEPS, **KW[name])
        self.e.set_auto_reset(False)
        self.e.set_record_mode(2)
        self.e.set_traj_capacity(1)

    def seen(self, obs_idx):
        """[n, n_vis] float32: what the policy sees of the lanes"""
        return self.states if obs_idx is None else self.states[:, list(obs_idx)]

    def run(self, terms, hot, j, obs_idx=None, sweep=True):
        """one-hot weight at (action row j, feature `hot` of the stack) -> (act [n, A] float32 of record row 0, d_init [n, S + H] float32
        and d_act [n, A] float32 of the sweep with g_act = e_j, or None without the sweep)"""
        e, n = self.e, self.n
        n_vis = self.S if obs_idx is None else len(obs_idx)
        F = sum(lc.n_features(t, n_vis) for t in terms)
        W = np.zeros((self.A, F), dtype=np.float32)
        W[j, hot] = 1.0
        e.set_policy_linear(W.reshape(-1), list(terms), obs_idx=obs_idx)
        e.reset(init_state=self.states)
        e.set_traj_offset(0)
        e.step_policy(1, record=True)
        tt = e.traj_tensors(1, n)
        obs, act = tt["obs"][0].cpu().numpy(), tt["act"][0].cpu().numpy()
        assert obs.dtype == np.float32 and obs.tobytes() == self.states.tobytes()  # the lanes hold the grid, bit for bit
        if not sweep:
            return act, None, None
        g = torch.zeros(1, self.A, e.ld, device="cuda")
        g[0, j, :n] = 1.0
        d_act, d_init = e.rollout_vjp_policy(1, g_act=g)
        assert torch.equal(d_act, g)                                                  # d_act[0] IS g_act (lanes >= n: 0)
        return act, self.vs.lanes_first(d_init, n).cpu().numpy(), self.vs.lanes_first(d_act, n).cpu().numpy()

    def close(self):
        self.e.close()


def ratio(err, bound):
    """err / bound per entry; an entry whose bound is 0 must be met exactly (inf otherwise); NaN counts as inf"""
    with np.errstate(all="ignore"):
        r = np.where(bound > 0.0, err / np.where(bound > 0.0, bound, 1.0), np.where(err == 0.0, 0.0, np.inf))
    return np.where(np.isnan(r), np.inf, r)


def check_feature(p, terms, t, hot0, j, obs_idx, worst):
    """every feature of term t (the stack's features hot0 ..) through the one-hot weight of action row j: the value at every lane, the
    derivative at every lane and row; -> the number of excluded lanes.  `worst` collects error / bound per kind."""
    x = p.seen(obs_idx)
    n_vis = x.shape[1]
    vref, vbound = lc.value(t, x), lc.value_errors(t, x)
    dref, dbound = lc.derivative(t, x), lc.derivative_errors(t, x)
    out = lc.excluded(t, x)
    kind = t if isinstance(t, str) else t[0]
    rows = list(range(n_vis)) if obs_idx is None else list(obs_idx)        # visible row k is state row rows[k]
    for f in range(vref.shape[1]):
        act, d_init, _ = p.run(terms, hot0 + f, j, obs_idx)
        got = act.astype(np.float64)
        rv = ratio(np.abs(got[:, j] - vref[:, f]), vbound[:, f])
        assert (rv <= 1.0).all(), (p.name, t, f, j, x[np.argmax(rv)], got[np.argmax(rv), j], vref[np.argmax(rv), f], float(rv.max()))
        if kind in lc.EXACT_VALUE:
            assert np.array_equal(got[:, j], vref[:, f])                   # bit-equal (zeros by value)
        assert (np.delete(got, j, axis=1) == 0.0).all()                    # the other action row: exactly 0
        want = np.zeros((p.n, p.S + p.H))
        bound = np.zeros((p.n, p.S + p.H))
        want[:, rows], bound[:, rows] = dref[:, f], dbound[:, f]
        keep = ~out
        rd = ratio(np.abs(d_init.astype(np.float64) - want), bound)[keep]
        at = np.unravel_index(np.argmax(rd), rd.shape)
        assert (rd <= 1.0).all(), (p.name, t, f, j, x[keep][at[0]], at[1], d_init[keep][at], want[keep][at], float(rd.max()))
        w = worst.setdefault(kind, [0.0, 0.0])
        w[0], w[1] = max(w[0], float(rv.max())), max(w[1], float(rd.max()))
    return int(out.sum())


def report(what, worst):
    print(f"{what}: worst error / bound per kind (value, derivative): " + ", ".join(f"{k} {v[0]:.3f} {v[1]:.3f}" for k, v in worst.items()))


# ------------------------------------------------------------------------------------------- the whole grid, the oscillator
@pytest.mark.parametrize("obs_idx", [None, (1, 0)], ids=["ident", "obs_idx=(1,0)"])
def test_every_elementwise_kind_at_every_grid_point(vs, obs_idx):
    """the 11 elementwise kinds and const, each a stack of its own, on both oscillator rows (row 1 holds the grid reversed); (1, 0)
    takes the select path instead of ident"""
    p = Probe(vs, "omo", lc.SCALAR_STATES)
    worst = {}
    for t in lc.ELEM + ("const",):
        assert check_feature(p, (t,), t, 0, 0, obs_idx, worst) == 0
    # the required points, by value: both rows hold every grid point
    x = p.seen(obs_idx)
    sig = p.run(("sig",), 0, 0, obs_idx)
    bell = p.run(("bell",), 0, 0, obs_idx)
    row = 0 if obs_idx is None else obs_idx[0]
    v = x[:, 0]
    assert np.isfinite(sig[0]).all()
    assert (sig[0][v <= -104.5, 0] == 0.0).all() and (sig[1][v <= -104.5, row] == 0.0).all() and (v <= -104.5).sum() >= 2
    assert (sig[0][v >= 17.5, 0] == 1.0).all() and (sig[1][v >= 17.5, row] == 0.0).all() and (v >= 17.5).sum() >= 7
    assert (bell[0][np.abs(v) >= 20.0, 0] == 0.0).all() and (bell[1][np.abs(v) >= 20.0, row] == 0.0).all() and (np.abs(v) >= 20.0).sum() >= 16
    assert (p.run(("sign",), 0, 0, obs_idx, sweep=False)[0][v == 0.0, 0] == 0.0).all()
    assert (p.run(("abs",), 0, 0, obs_idx)[1][v == 0.0, row] == 0.0).all() and (v == 0.0).sum() == 2
    assert p.e.error_count() == 0
    p.close()
    report(f"oscillator, {lc.SCALAR.size} lanes, obs_idx {obs_idx}", worst)


@pytest.mark.parametrize("obs_idx", [None, (1, 0)], ids=["ident", "obs_idx=(1,0)"])
def test_atan2_and_mult_on_their_grids(vs, obs_idx):
    worst = {}
    p = Probe(vs, "omo", lc.PAIRS)
    n_out = sum(check_feature(p, lc.PAIR_TERMS, t, q, 0, obs_idx, worst) for q, t in enumerate(lc.PAIR_TERMS))
    assert n_out == 4 * len(lc.PAIR_TERMS)                                  # the ONE exclusion, counted
    assert p.e.error_count() == 0
    p.close()
    p = Probe(vs, "omo", lc.MULT_STATES)
    assert sum(check_feature(p, lc.MULT_TERMS, t, q, 0, obs_idx, worst) for q, t in enumerate(lc.MULT_TERMS)) == 0
    assert p.e.error_count() == 0
    p.close()
    report(f"oscillator, {lc.PAIRS.shape[0]} pairs and {lc.MULT_STATES.shape[0]} product lanes, obs_idx {obs_idx}", worst)


def test_the_three_measured_figures(vs):
    """worst |device - fp64| of the bell, atan2f and the fp32 division over the grids: the bounds use twice the module's constants, which
    are these figures as measured on the MI355X; here they are printed and held to the constants' margin.  atan2f above 6 ulp (the
    OpenCL limit) or a sigmoid that is not finite on the grid would be findings, not constants."""
    p = Probe(vs, "omo", lc.SCALAR_STATES)
    got = p.run(("bell",), 0, 0, sweep=False)[0][:, 0].astype(np.float64)
    ref = lc.value("bell", lc.SCALAR_STATES)[:, 0]
    normal = ref >= np.finfo(np.float32).tiny
    bell_abs, bell_ulps = float(np.abs(got - ref).max()), float(lc.ulps_of(got - ref, ref)[normal].max())
    assert np.isfinite(p.run(("sig",), 0, 0, sweep=False)[0]).all()
    p.close()
    p = Probe(vs, "omo", lc.PAIRS)
    a_abs = a_ulps = d_ulps = 0.0
    for q, t in enumerate(lc.PAIR_TERMS):
        act, d_init, _ = p.run(lc.PAIR_TERMS, q, 0)
        got, ref = act[:, 0].astype(np.float64), lc.value(t, lc.PAIRS)[:, 0]
        nz = ref != 0.0
        assert (got[~nz] == 0.0).all()
        a_abs, a_ulps = max(a_abs, float(np.abs(got - ref).max())), max(a_ulps, float(lc.ulps_of(got - ref, ref)[nz].max()))
        if t[1] == (0, 1):  # (y, x) = (1, m): d / d x = -1 / (1 + m^2), one division
            pr = lc.DIV_PROBES
            dref = lc.derivative(t, lc.PAIRS)[pr, 0, 1]
            d_ulps = float(lc.ulps_of(d_init[pr, 1].astype(np.float64) - dref, dref).max())
    p.close()
    print(f"library {vs._lib.load().vs_version()}, {lc.SCALAR.size} scalar points, {lc.PAIRS.shape[0]} pairs of which "
          f"{int(lc.DIV_PROBES.sum())} division probes: bell {bell_abs:.3e} abs, {bell_ulps:.1f} ulps (normal references); "
          f"atan2f {a_abs:.3e} abs, {a_ulps:.2f} ulps; division {d_ulps:.2f} ulps")
    assert a_ulps <= lc.ATAN2_ULPS_LIMIT
    assert bell_abs <= 2.0 * lc.BELL_ABS and a_abs <= 2.0 * lc.ATAN2_ABS and a_ulps <= 2.0 * lc.ATAN2_ULPS and d_ulps <= 2.0 * lc.DIV_ULPS


# ------------------------------------------------------------------------------------- the wiring, the ball balancer's 128 slots
def slots_of(terms, n_vis):
    """[(term, first feature of the term in the stack)]"""
    out, q = [], 0
    for t in terms:
        out.append((t, q))
        q += lc.n_features(t, n_vis)
    return out, q


@pytest.mark.parametrize("j", [0, 1])
def test_wiring_of_all_128_slots_on_the_ball_balancer(vs, j):
    """qbb-full of lin_param_grad_fp64.EXTRA: each of the 128 slots one-hot in action row j (128 one-step launches of 256 lanes and
    as many sweeps): the hot action row holds that slot's feature, the other one exactly 0, d_init that slot's derivative"""
    terms = host.EXTRA["qbb-full"][1]
    p = Probe(vs, "qbb", lc.qbb_states())
    slots, F = slots_of(terms, 8)
    assert F == 128
    worst = {}
    assert sum(check_feature(p, terms, t, q, j, None, worst) for t, q in slots) == 0
    assert p.e.error_count() == 0
    p.close()
    report(f"ball balancer, 128 slots x 256 lanes, action row {j}", worst)


def test_wiring_through_obs_idx_on_the_ball_balancer(vs):
    """a permuted strict subset of the rows: the stack's indices count VISIBLE rows, d_init goes back to state rows"""
    obs_idx = (6, 1, 4, 3, 0)
    terms = lc.ELEM + ("const", ("mult", (0, 4)), ("mult", (2, 1, 2)), ("mult", (4, 3, 4, 4)), ("atan2", (1, 3)), ("atan2", (4, 0)))
    p = Probe(vs, "qbb", lc.qbb_states())
    slots, F = slots_of(terms, len(obs_idx))
    assert F == 11 * 5 + 6
    worst = {}
    assert sum(check_feature(p, terms, t, q, q % 2, obs_idx, worst) for t, q in slots) == 0
    assert p.e.error_count() == 0
    p.close()
    report(f"ball balancer through obs_idx {obs_idx}", worst)
