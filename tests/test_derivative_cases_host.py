"""
derivative_cases.py without a device: what tells its two tolerance rules apart, and the small helpers every derivative test leans on.
"""
import numpy as np
import pytest

import derivative_cases as dc

# two lanes whose gradients differ by 1e3; both central differences agree, so every entry is smooth
WANT = np.array([[1000.0, 500.0, 250.0], [1.0, 0.5, 0.25]])
EVERY = np.ones(WANT.shape, dtype=bool)


def test_an_error_in_the_small_lane_passes_globally_and_fails_per_lane():
    """0.01 off on the entry 0.5 of the small lane: its tolerance is 3e-3 * 0.5 + 3e-4 * 1000 = 0.3015 in the unit of the whole array
    and 3e-3 * 0.5 + 3e-4 * 1 = 0.0018 in the lane's own"""
    got = WANT.copy()
    got[1, 1] += 0.01
    bad, worst = dc.within_global(got, WANT, EVERY)
    assert bad == 0.0 and worst == pytest.approx(0.01 / 0.3015, rel=1e-12)
    bad, worst = dc.within_per_lane(got, WANT, EVERY)
    assert bad == 1.0 / 6.0 and worst == pytest.approx(0.01 / 0.0018, rel=1e-9)
    assert dc.worst_of(got, WANT, EVERY) == worst
    assert np.array_equal(dc.tolerance_per_lane(WANT, EVERY), 3e-3 * WANT + 3e-4 * WANT[:, :1])


def test_the_smooth_masks_differ_in_the_same_way():
    """the two step sizes part by 5e-5 on the small lane's last entry, 0.25: 1e-4 |g| = 2.5e-5 does not cover that, with 1e-7 (1 + 1000)
    of the whole array on top it does, with 1e-7 (1 + 1) of the lane it does not"""
    other = WANT.copy()
    other[1, 2] += 5e-5
    assert dc.smooth_global(WANT, other).all()
    assert np.array_equal(dc.smooth_per_lane(WANT, other), [[True, True, True], [True, True, False]])


def test_a_lane_without_a_smooth_entry_has_the_floor_one():
    smooth = np.array([[True, True, True], [False, False, False]])
    tol = dc.tolerance_per_lane(WANT, smooth)
    assert np.array_equal(tol[1], 3e-3 * WANT[1] + 3e-4 * 1.0) and np.array_equal(tol[0], 3e-3 * WANT[0] + 3e-4 * 1000.0)
    got = WANT.copy()
    got[1] += 100.0  # not smooth: not counted
    assert dc.within_per_lane(got, WANT, smooth) == (0.0, 0.0)
    assert dc.worst_of(got, WANT, smooth) > 1.0  # ... but worst_of holds every entry


def test_per_lane_with_nothing_smooth_is_an_error_and_global_returns_zero():
    none = np.zeros(WANT.shape, dtype=bool)
    with pytest.raises(ValueError):
        dc.within_per_lane(WANT + 1.0, WANT, none)
    assert dc.within_global(WANT + 1.0, WANT, none) == (0.0, 0.0)


def test_global_without_a_mask_counts_every_entry():
    got = WANT.copy()
    got[0, 0] += 10.0  # tolerance 3e-3 * 1000 + 3e-4 * 1000 = 3.3
    assert dc.within_global(got, WANT) == dc.within_global(got, WANT, EVERY)
    bad, worst = dc.within_global(got, WANT)
    assert bad == 1.0 / 6.0 and worst == pytest.approx(10.0 / 3.3, rel=1e-12)
    masked = EVERY.copy()
    masked[0, 0] = False  # the maximum is now 500 and the entry is not counted
    assert dc.within_global(got, WANT, masked) == (0.0, 0.0)


def test_lengths_of():
    done = np.zeros((4, 3), dtype=bool)  # [T, N]
    done[0, 0] = done[2, 0] = True       # lane 0: done in the first row (and again later)
    done[3, 1] = True                    # lane 1: done in the last row; lane 2: never
    assert np.array_equal(dc.lengths_of(done), [1, 4, 4])


@pytest.mark.parametrize("name", dc.FAMILIES)
def test_edge_states_touches_the_first_lanes_only(name):
    S = len(dc.INIT_SCALE[name])
    init = np.arange(30.0 * S, dtype=np.float32).reshape(30, S) / 1000.0
    kept = init.copy()
    for kw, n_edge in (({}, dc.N_EDGE), (dict(n_edge=20), 20)):
        out = dc.edge_states(name, init, **kw)
        assert np.array_equal(init, kept) and out is not init       # the input is unmodified
        assert np.array_equal(out[n_edge:], kept[n_edge:])          # lanes >= n_edge are untouched
        changed = (out[:n_edge] != kept[:n_edge]).any(axis=0)
        assert changed.sum() == 2 and (out[:n_edge] == out[0]).all(axis=0)[changed].all()  # a position and a velocity, one value each
