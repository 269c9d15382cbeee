"""
The per-column rule of derivative_cases.py on the fp64 oracle alone, no device: what the rule accepts (the oracle at the other step
size), what it must refuse (a column off by 5 %, zeroed, or swapped with its neighbour -- for EVERY non-null column of every family),
the gap the per-family rule leaves over an all-parameter array, and the table of null columns.

The arrays are all_param_oracle(name): central differences of Phi with respect to every domain parameter, [150, P], per PARAM_UNIT.
"""
import numpy as np
import pytest

import derivative_cases as dc

# the three small columns of the issue's table and the largest relative error in them that the per-family rule lets through
# without one bad entry (its floor, 3e-4 x the family's largest column, over the column's own largest entry)
SMALL = {"qq-su": ("damping_pend_pole", 1.45), "bob": ("beam_thickness", 1.13), "qbb": ("ball_radius", 1.26)}


def live_arrays(name):
    """the oracle's two arrays cut to the non-null columns, their smooth mask, and those columns' indices"""
    o = dc.all_param_oracle(name)
    live = np.flatnonzero(~dc.null_columns(o.f1, o.f2))
    f1, f2 = o.f1[:, live], o.f2[:, live]
    return f1, f2, dc.smooth_per_column(f1, f2), live


def mutations(f, j):
    """column j multiplied by 1.05, zeroed, swapped with its right neighbour (the last column with the first)"""
    scaled, zeroed, swapped = f.copy(), f.copy(), f.copy()
    scaled[:, j] *= 1.05
    zeroed[:, j] = 0.0
    nb = (j + 1) % f.shape[1]
    swapped[:, [j, nb]] = f[:, [nb, j]]
    return dict(scaled=scaled, zeroed=zeroed, swapped=swapped)


@pytest.mark.parametrize("name", dc.FAMILIES)
def test_every_entry_of_every_column_is_smooth(name):
    """(a) the two step sizes agree in every entry of all P columns (null columns included: 0 against 0, or 4e-10 against the like):
    the suite's condition `smooth share > 0.9` holds with room to spare"""
    o = dc.all_param_oracle(name)
    assert o.f1.shape == (dc.N, len(dc.params_case(name)["ref"].param_names))
    assert dc.smooth_per_column(o.f1, o.f2).all() and dc.smooth_per_column(o.gn1, o.gn2).all()
    assert (o.unit > 0).all() and np.array_equal(o.unit == 0.1, dc.params_case(name)["params"] == 0)


@pytest.mark.parametrize("name", dc.FAMILIES)
def test_the_other_step_size_lies_inside_the_rule(name):
    """(b) h = 1e-5 against h = 1e-6: no bad entry, in the gradient and in the Gauss-Newton diagonal"""
    f1, f2, smooth, live = live_arrays(name)
    bad, worst = dc.within_per_column(f2, f1, smooth)
    assert bad == 0.0 and worst.shape == (live.size,) and worst.max() < 1e-2, (name, worst)
    o = dc.all_param_oracle(name)
    bad, worst = dc.within_per_column(o.gn2[:, live], o.gn1[:, live], dc.smooth_per_column(o.gn1[:, live], o.gn2[:, live]))
    assert bad == 0.0 and worst.max() < 1e-2, (name, worst)


@pytest.mark.parametrize("name", dc.FAMILIES)
def test_a_wrong_column_lies_outside_the_rule(name):
    """(c) every non-null column, every mutation: a bad share above the 2e-3 the GPU tests allow, and the worst ratio of the
    mutated column above 1"""
    f1, _, smooth, live = live_arrays(name)
    for j in range(live.size):
        for what, got in mutations(f1, j).items():
            bad, worst = dc.within_per_column(got, f1, smooth)
            assert bad > 2e-3 and worst[j] > 1.0, (name, int(live[j]), what, bad, worst[j])
            assert what == "swapped" or (np.delete(worst, j) == 0.0).all()  # (the other columns are untouched)


@pytest.mark.parametrize("name", sorted(SMALL))
def test_the_gap_of_the_per_family_rule(name):
    """(d) within_global over the all-parameter array, its one maximum the family's largest column.  A small column off by 5 %, and
    off by as much as 45 % (damping_pend_pole), 13 % (beam_thickness), 26 % (ball_radius), passes it without one bad entry; the
    per-column rule refuses each.  (Zeroing such a column, or swapping it with a neighbour hundreds of times its size, is still
    caught by the per-family rule: the gap is a scale error of tens of per cent, not a missing column.)"""
    o = dc.all_param_oracle(name)
    ref = dc.params_case(name)["ref"]
    col, most = SMALL[name]
    j = ref.param_names.index(col)
    everywhere = dc.smooth_global(o.f1, o.f2)
    assert everywhere.all()
    f1, _, smooth, live = live_arrays(name)
    jl = int(np.flatnonzero(live == j)[0])
    for factor in (1.05, most):
        got = o.f1.copy()
        got[:, j] *= factor
        bad, worst = dc.within_global(got, o.f1, everywhere)
        assert bad == 0.0 and worst < 1.0, (name, col, factor, bad, worst)
        bad, worst = dc.within_per_column(got[:, live], f1, smooth)
        assert bad > 2e-3 and worst[jl] > 1.0, (name, col, factor, bad, worst[jl])
    for what in ("zeroed", "swapped"):
        got = mutations(o.f1, j)[what]
        assert dc.within_global(got, o.f1, everywhere)[0] > 2e-3, (name, col, what)


@pytest.mark.parametrize("name", dc.FAMILIES)
def test_the_null_columns_are_those_of_the_table(name):
    """(e) NULL_COLUMNS from the oracle: the "exact" columns are 0.0 in every lane at both step sizes (gradient and Gauss-Newton
    diagonal); the ball-on-beam's ball_radius, which cancels analytically, is fp64 rounding (below 1e-9, 99 % of it zeros) next to
    a smallest real column, beam_thickness, of 1.86e-2"""
    o = dc.all_param_oracle(name)
    null = dc.null_columns(o.f1, o.f2)
    assert np.flatnonzero(null).tolist() == sorted(dc.NULL_COLUMNS[name])
    for j, (kind, why) in dc.NULL_COLUMNS[name].items():
        assert why.startswith(dc.params_case(name)["ref"].param_names[j] + ":")
        if kind == "exact":
            assert not o.f1[:, j].any() and not o.f2[:, j].any() and not o.gn1[:, j].any() and not o.gn2[:, j].any(), (name, j)
        else:
            assert kind == "cancels" and (name, j) == ("bob", 2)
            assert 0.0 < np.abs(o.f1[:, j]).max() < 1e-9 and (o.f1[:, j] == 0.0).mean() >= 0.98
            smallest = np.abs(o.f1[:, ~null]).max(axis=0)
            assert dc.params_case(name)["ref"].param_names[int(np.flatnonzero(~null)[smallest.argmin()])] == "beam_thickness"
            assert smallest.min() == pytest.approx(1.856e-2, rel=1e-3)


def test_the_rule_itself():
    """two columns whose sizes differ by 1e3: the tolerance's floor is the column's own, a column without a smooth entry is an error,
    the bad share counts the whole array"""
    want = np.array([[1000.0, 1.0], [500.0, 0.5], [250.0, 0.25]])
    every = np.ones(want.shape, dtype=bool)
    assert np.array_equal(dc.tolerance_per_column(want, every), 3e-3 * want + 3e-4 * want[:1])
    got = want.copy()
    got[1, 1] += 0.01  # tolerance 3e-3 * 0.5 + 3e-4 * 1 = 0.0018; the per-family rule gives it 0.3015
    bad, worst = dc.within_per_column(got, want, every)
    assert bad == 1.0 / 6.0 and worst[0] == 0.0 and worst[1] == pytest.approx(0.01 / 0.0018, rel=1e-9)
    assert dc.within_global(got, want, every)[0] == 0.0
    other = want.copy()
    other[2, 1] += 5e-5  # 1e-4 * 0.25 does not cover that, 1e-7 (1 + 1) of the column neither; 1e-7 (1 + 1000) of the array would
    assert np.array_equal(dc.smooth_per_column(want, other), [[True, True], [True, True], [True, False]]) and dc.smooth_global(want, other).all()
    masked = every.copy()
    masked[0, 1] = False  # the column's maximum is now 0.5, and the unmasked entry is not counted
    assert np.array_equal(dc.tolerance_per_column(want, masked)[:, 1], 3e-3 * want[:, 1] + 3e-4 * 0.5)
    masked[:, 1] = False
    with pytest.raises(ValueError, match=r"\[1\]"):
        dc.within_per_column(got, want, masked)
    assert np.array_equal(dc.null_columns(np.array([[1.0, 1e-9, 0.0]]), np.array([[1.0, 0.0, 2e-8]])), [False, True, False])
    assert np.array_equal(dc.PARAM_UNIT("bob", np.array([[-2.0, 0.0, 0.05]], dtype=np.float32)), [[2.0, 0.1, np.float64(np.float32(0.05))]])
