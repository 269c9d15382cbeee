"""
The per-position rule of step_jacobian_cases.py on the fp64 oracle alone, no device: what the rule accepts (the oracle at the other
step size), what it must refuse (a position off by 5 %, zeroed, or swapped with its neighbour -- for EVERY live position of every
family, array and parameter layout), the gap the rule it replaces leaves, and the table of null positions.

The arrays are oracle(name, layout): central differences of cpu_ref.step with respect to (s, a), flattened to [n, positions].
"""
import numpy as np
import pytest

import derivative_cases as dc
import step_jacobian_cases as sj

CASES = [(name, layout) for layout in sj.LAYOUTS for name in sj.ENVS]
# the null positions of d s', d r and d obs', the same in the three layouts; every one of them is 0.0 in every lane at both step sizes
# (the oscillator's d x' / d a, the first rows' action columns of the others, the ball balancer's uncoupled axes, the snapped action
# of bob-d): none holds rounding noise, so the device has to return 0.0 in all of them
NULLS = {"omo": (1, 0, 1), "bob": (2, 0, 2), "qq-su": (3, 0, 4), "qcp-su": (3, 0, 4), "qbb": (50, 0, 50), "qq-st": (3, 0, 4),
         "qcp-st": (3, 0, 4), "pend": (0, 0, 0), "bob-d": (4, 0, 4)}
# On the "nominal" draw, per array: live positions, the floor of the rule replaced (3e-4 x the array's largest smooth entry) over
# the largest entry of the smallest live position, the positions that rule lets be 5 % off, and those it lets be ZERO in every
# lane, each without exceeding the 2e-3 bad share it allowed.
GAP = {("qbb", "state"): (30, 46.7, 14, 6), ("qbb", "rew"): (10, 1.28, 8, 2),
       ("qcp-su", "state"): (17, 29.7, 9, 4), ("qcp-su", "obs"): (21, 29.7, 12, 6),
       ("qcp-st", "state"): (17, 17.1, 6, 2), ("qcp-st", "obs"): (21, 17.1, 9, 3),
       ("qq-su", "state"): (17, 11.5, 7, 6), ("qq-su", "obs"): (26, 31.9, 14, 12),
       ("qq-st", "state"): (17, 4.61, 7, 6), ("qq-st", "obs"): (26, 9.02, 14, 12),
       ("bob", "state"): (18, 3.52, 5, 3), ("bob-d", "state"): (16, 3.52, 4, 2),
       ("omo", "rew"): (3, 44.7, 1, 1),
       ("pend", "state"): (6, 0.251, 1, 0), ("pend", "obs"): (9, 0.251, 2, 0)}
# the live positions whose 5 % the third term of the rule would hide at K_FP32, by (family, layout, array, i, k): with K_FP32 = 0
# there is none
UNRESOLVABLE = []


def mutations(f, live, j):
    """live position live[j] multiplied by 1.05, zeroed, swapped with its right neighbour among the live ones (the last with the
    first)"""
    p, q = live[j], live[(j + 1) % live.size]
    scaled, zeroed, swapped = f.copy(), f.copy(), f.copy()
    scaled[:, p] *= 1.05
    zeroed[:, p] = 0.0
    swapped[:, [p, q]] = f[:, [q, p]]
    return dict(scaled=scaled, zeroed=zeroed, swapped=swapped)


def test_the_cases():
    """the inputs: float32, read-only, the lanes of every layout, the time-limit lanes, the parameters of every layout"""
    for name, layout in CASES:
        c = sj.case(name, layout)
        ref, n = c.ref, sj.N_LANES[layout]
        assert c.n == n and c.params.shape == (n, len(ref.param_names)) and c.state.shape == (n, ref.S)
        assert c.hidden.shape == (n, ref.H) and c.act.shape == (n, ref.A) and c.curr.shape == (n,)
        for a in (c.params, c.state, c.hidden, c.act):
            assert a.dtype == np.float32 and not a.flags.writeable
        assert not c.curr.flags.writeable and c.set_params == (layout != "uniform")
        nominal = ref.nominal_params(n).astype(np.float32)
        if layout == "per_lane":
            moved = nominal != 0
            assert (c.params[:, moved[0]] != nominal[:, moved[0]]).mean() > 0.99
            assert (np.abs(c.params - nominal) <= 0.0501 * np.abs(nominal)).all()
        else:
            assert np.array_equal(c.params, nominal)
        limit = c.curr == sj.KW[name]["max_steps"] - 1
        assert limit.sum() == (0 if layout == "nominal" else sj.N_LIMIT) and (c.curr[~limit] < 50).all()
        o = sj.oracle(name, layout)
        assert np.array_equal(o.done, limit)  # (no lane leaves its box in this step: done is the time limit alone)
        assert o.clipped[: n // 8].sum() == o.clipped.sum() > (10 if layout == "nominal" else 2)
    assert sj.N_LANES == {"nominal": 768, "per_lane": 150, "uniform": 150}  # 12 full waves; two full waves and a partial one


@pytest.mark.parametrize("name,layout", CASES)
def test_every_entry_of_every_position_is_smooth(name, layout):
    """(a) the two step sizes agree in every entry of every position, the mask taken per position: no entry is left out of the
    comparison, and the device test needs no allowance for bad entries"""
    o = sj.oracle(name, layout)
    ref, n = sj.case(name, layout).ref, sj.N_LANES[layout]
    NI = ref.S + ref.A
    assert [g.shape for g in o.f1] == [(n, ref.S * NI), (n, NI), (n, ref.O * NI)] and o.scale.shape == (n, NI)
    assert (o.scale >= 1e-3).all()
    for r in sj.rules(name, layout):
        assert r.smooth.all() and sj.checked(r).all()


@pytest.mark.parametrize("name,layout", CASES)
def test_the_other_step_size_lies_inside_the_rule(name, layout):
    """(b) h = 1e-5 against h = 1e-6: no bad entry, the worst ratio under 1e-2, in the three arrays"""
    o = sj.oracle(name, layout)
    for g2, r in zip(o.f2, sj.rules(name, layout)):
        bad, worst = sj.within(g2, r)
        assert bad == 0 and worst.shape == r.live.shape and worst.max() < 1e-2, (name, layout, worst)


@pytest.mark.parametrize("name,layout", CASES)
def test_a_wrong_position_lies_outside_the_rule(name, layout):
    """(c) every live position, every mutation, K_FP32 at its recorded value.  A position zeroed or swapped is refused without
    exception; one off by 5 % is refused wherever 5 % of the position's own maximum exceeds twice the third term (at the lane of that
    maximum), and the others are those of UNRESOLVABLE"""
    NI = sj.case(name, layout).ref.S + sj.case(name, layout).ref.A
    unresolvable = []
    for tag, r in zip(sj.ARRAYS, sj.rules(name, layout)):
        live = np.flatnonzero(r.live)
        at_top = np.where(r.smooth, np.abs(r.want), 0.0).argmax(axis=0)
        for j, p in enumerate(live):
            resolvable = 0.05 * r.top[p] > 2.0 * sj.K_FP32 * r.third[at_top[p], p]
            if not resolvable:
                unresolvable.append((name, layout, tag) + sj.position(p, NI))
            for what, got in mutations(r.want, live, j).items():
                bad, worst = sj.within(got, r)
                if what == "scaled" and not resolvable:
                    continue
                assert bad > 0 and worst[p] > 1.0, (name, layout, tag, sj.position(p, NI), what, worst[p])
                assert what == "swapped" or not np.delete(worst, p).any()  # (the other positions are untouched)
    assert unresolvable == [u for u in UNRESOLVABLE if u[:2] == (name, layout)]


def test_no_position_is_unresolvable():
    assert sj.K_FP32 == 0 and len(UNRESOLVABLE) == 0


@pytest.mark.parametrize("name,tag", sorted(GAP))
def test_the_gap_of_the_rule_replaced(name, tag):
    """(d) 3e-3 |g| + 3e-4 max |g_smooth| over the whole array, fewer than 2e-3 of the entries bad: the positions it lets be 5 % off
    or zero in every lane, counted; the per-position rule refuses every one of them"""
    r = sj.rules(name, "nominal")[sj.ARRAYS.index(tag)]
    n_live, ratio, n_off, n_zero = GAP[name, tag]
    live = np.flatnonzero(r.live)
    assert live.size == n_live and r.present_smooth.all()
    floor = 3e-4 * np.abs(r.want).max()
    assert floor / r.top[live].min() == pytest.approx(ratio, rel=1e-2)
    off, zero = 0, 0
    for j, p in enumerate(live):
        m = mutations(r.want, live, j)
        passes_off, passes_zero = sj.within_present(m["scaled"], r) < 2e-3, sj.within_present(m["zeroed"], r) < 2e-3
        off, zero = off + passes_off, zero + passes_zero
        assert floor / r.top[p] < 1.0 or passes_zero  # (a floor above the position's maximum: zero in every lane passes)
        for got in (m["scaled"], m["zeroed"]):
            assert sj.within(got, r)[1][p] > 1.0
    assert (off, zero) == (n_off, n_zero)


def test_the_named_positions_pass_the_rule_replaced_when_zeroed():
    """the ball balancer's d (x, y)' / d (theta_x, theta_y), the cart-pole's d x' / d x_dot, the QQube's d theta' / d theta_dot and the
    oscillator's d r / d a are among them"""
    for name, tag, i, k in (("qbb", "state", 2, 0), ("qbb", "state", 3, 1), ("qcp-su", "state", 0, 3), ("qq-su", "state", 0, 2),
                            ("omo", "rew", 0, 2)):
        r = sj.rules(name, "nominal")[sj.ARRAYS.index(tag)]
        p = i * (sj.case(name, "nominal").ref.S + sj.case(name, "nominal").ref.A) + k
        got = r.want.copy()
        got[:, p] = 0.0
        assert r.live[p] and sj.within_present(got, r) < 2e-3 and sj.within(got, r)[0] > 0.9 * got.shape[0], (name, tag, i, k)


@pytest.mark.parametrize("name,layout", CASES)
def test_no_entry_is_held_more_loosely_than_before(name, layout):
    """(e) the tolerance is at most that of the rule replaced in every entry, whatever K_FP32; and far below it where it matters"""
    for k in (None, 1, 16):
        for r in sj.rules(name, layout, k):
            assert (r.tol <= r.present).all()
            assert (r.tol[:, r.exact] == 0.0).all() and (r.tol[:, r.live] > 0.0).all()


@pytest.mark.parametrize("name,layout", CASES)
def test_the_null_positions_are_those_of_the_table(name, layout):
    """(f) NULLS from the oracle: every null position is exactly 0.0 at both step sizes, and a device entry other than 0.0 in one of
    them is refused"""
    o = sj.oracle(name, layout)
    rs = sj.rules(name, layout)
    assert tuple(int((~r.live).sum()) for r in rs) == NULLS[name]
    for g1, g2, r in zip(o.f1, o.f2, rs):
        null = ~r.live
        assert np.array_equal(null, dc.null_columns(g1, g2)) and np.array_equal(r.exact, null)
        assert not g1[:, null].any() and not g2[:, null].any() and not r.top[null].any()
        if null.any():
            got = r.want.copy()
            got[3, np.flatnonzero(null)[0]] = 1e-30
            bad, worst = sj.within(got, r)
            assert bad == 1 and np.isinf(worst[np.flatnonzero(null)[0]])


def test_the_rule_itself():
    """two outputs and two inputs, positions four orders apart: the floor is the position's own, the third term is 2^-23 of the row's
    largest entry in the unit of the output over the input's scale, the smaller of the two rules holds, an exact zero admits nothing"""
    scale = np.array([[2.0, 0.5], [2.0, 0.5], [2.0, 0.5]])
    want = np.array([[1.0, 1e-4, 0.0, 40.0], [0.5, 2e-4, 0.0, 20.0], [0.25, 4e-4, 0.0, 10.0]])
    third = sj.third_term(want, scale)
    assert np.array_equal(third[0], sj.ULP * np.array([2.0 / 2.0, 2.0 / 0.5, 20.0 / 2.0, 20.0 / 0.5]))
    r0, r4 = sj.rule(want, want, scale, 0), sj.rule(want, want, scale, 4)
    assert np.array_equal(r0.live, [True, True, False, True]) and np.array_equal(r0.exact, ~r0.live) and r0.smooth.all()
    assert np.array_equal(r0.top, [1.0, 4e-4, 0.0, 40.0])
    assert np.array_equal(r0.present, 3e-3 * want + 3e-4 * 40.0)
    assert np.array_equal(r0.tol[:, [0, 1, 3]], (3e-3 * want + 3e-4 * r0.top)[:, [0, 1, 3]]) and not r0.tol[:, 2].any()
    with_third = 3e-3 * want + 3e-4 * r0.top + 4 * third
    assert np.array_equal(r4.tol[:, :2], with_third[:, :2]) and not r4.tol[:, 2].any()
    assert (with_third[:, 3] > r4.present[:, 3]).all() and np.array_equal(r4.tol[:, 3], r4.present[:, 3])  # (the smaller of the two)
    got = want.copy()
    got[1, 1] = 0.0  # 2e-4 off: the position's own floor is 1.2e-7, the array's 1.2e-2
    assert sj.within(got, r0)[0] == 1 and sj.within_present(got, r0) == 0.0
    assert sj.within(got, r0)[1][1] == pytest.approx(2e-4 / (3e-3 * 2e-4 + 3e-4 * 4e-4), rel=1e-12)
    got = want.copy()
    got[2, 2] = 1e-12
    bad, worst = sj.within(got, r0)
    assert bad == 1 and np.array_equal(worst, [0.0, 0.0, np.inf, 0.0])
    noise = want.copy()
    noise[0, 2] = 1e-9  # a null position that holds noise is not exact: it gets K x the third term alone
    rn = sj.rule(noise, want, scale, 4)
    assert not rn.live[2] and not rn.exact[2] and np.array_equal(rn.tol[:, 2], 4 * sj.third_term(noise, scale)[:, 2])
    assert sj.position(7, 5) == (1, 2)
    u = sj.ulps_beyond(want + 2.0 * third, r4)  # an error of two third terms: 2 less what the first two terms cover, in ulps
    live = [0, 1, 3]
    np.testing.assert_allclose(u[:, live], 2.0 - ((3e-3 * want + 3e-4 * r0.top) / third)[:, live], rtol=1e-9)
    assert u[0, 1] == pytest.approx(2.0 - 4.2e-7 / (4 * sj.ULP), rel=1e-9) and (u[:, [0, 3]] < 0.0).all() and np.isneginf(u[:, 2]).all()
