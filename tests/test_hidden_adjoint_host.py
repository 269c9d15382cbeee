"""
The hidden-state adjoint and the carried tangents without a device: what the GPU tests of d_init[S:] and VS_ROLLOUT_SENS take from
derivative_cases.py holds from the fp64 oracle alone, so that a failure on the device is never the oracle's fault -- and the checks can
fail: a hidden block that is negated, zeroed or 2 % off does not pass the per-column rule, while the per-lane rule over
[state | hidden] columns, which is what the hidden rows would get as further columns of the existing arrays, accepts a zeroed one.
"""
import numpy as np
import pytest

import derivative_cases as dc


@pytest.mark.parametrize("name", dc.HIDDEN_FAMILIES)
def test_hidden_start_is_deterministic_float32_read_only_and_keeps_the_lane_lengths(name):
    c = dc.params_case(name)
    h = dc.hidden_start(name, c)
    assert h.dtype == np.float32 and h.shape == (dc.N, c["ref"].H) and not h.flags.writeable
    assert np.array_equal(h, dc.hidden_start(name, c)) and np.array_equal(h, dc.hidden_start(name, dc.playback_case(name)[0]))
    off = (h.astype(np.float64) - dc.reset_hidden(c)) / np.array(dc.HIDDEN_SCALE[name])
    assert (np.abs(off) <= 1.0 + 1e-6).all() and np.abs(off).mean() > 0.4 and (off > 0).any(axis=0).all() and (off < 0).any(axis=0).all()
    with pytest.raises(ValueError):
        h[0, 0] = 0.0
    at_reset, at_start = (dc.open_loop_hidden_reference(name, s) for s in dc.STARTS)
    assert np.array_equal(at_reset[2], at_start[2])                      # no lane changes its length
    assert (at_reset[2][:dc.N_EDGE] < dc.T).any() and (at_reset[2][dc.N_EDGE:] == dc.T).mean() > 0.9
    assert np.array_equal(at_start[3], h.astype(np.float64)) and np.array_equal(at_reset[3], dc.reset_hidden(c))


@pytest.mark.parametrize("start", dc.STARTS)
@pytest.mark.parametrize("name", dc.HIDDEN_FAMILIES)
def test_the_hidden_block_is_smooth_and_the_check_can_fail(name, start):
    """from the oracle alone: at most 1 % of the block not smooth (measured: none) and no column without a smooth entry; then three
    wrong blocks -- negated, zeroed, the h = 1e-3 differences scaled by 1.02 -- each beyond the 2e-3 cap on the share of bad entries"""
    g1, g2 = dc.open_loop_hidden_reference(name, start)[:2]
    smooth = dc.hidden_conditions(name, g1, g2)
    assert g1.shape == (dc.N, len(dc.HIDDEN_SCALE[name])) and smooth.all()
    assert dc.within_per_column(g2, g1, smooth)[0] == 0.0 and dc.check_hidden_block(name, g2, g1, g2).max() < 0.1  # the other step size passes
    for tag, wrong in (("negated", -g1), ("zeroed", np.zeros_like(g1)), ("2 % off", 1.02 * g2)):
        bad = dc.within_per_column(wrong, g1, smooth)[0]
        assert bad > 2e-3, (name, start, tag, bad)
        with pytest.raises(AssertionError):
            dc.check_hidden_block(f"{name} {tag}", wrong, g1, g2)
    # most entries are held to less than half their own size (the cartpole: 93 %, the ball balancer: all of them)
    tight = (dc.tolerance_per_column(g1, smooth) < 0.5 * np.abs(g1)).mean()
    assert tight > (0.9 if name == "qcp-su" else 0.999), (name, tight)


def state_columns(name, start):
    """d Phi / d s_0 of params_case per INIT_SCALE at relative steps 1e-6 and 1e-5: two arrays [N, S]"""
    c = dc.params_case(name)
    P0, s0, a0 = (c[k].astype(np.float64) for k in ("params", "init", "acts"))
    _, _, length, h0 = dc.open_loop_hidden_reference(name, start)
    out = []
    for h in (1e-6, 1e-5):
        g = np.zeros(s0.shape)
        for j in range(s0.shape[1]):
            d = np.zeros_like(s0)
            d[:, j] = h * dc.INIT_SCALE[name][j]
            g[:, j] = (dc.phi(c, P0, P0, s0 + d, h0, a0, length) - dc.phi(c, P0, P0, s0 - d, h0, a0, length)) / (2.0 * h)
        out.append(g)
    return out


@pytest.mark.parametrize("start", dc.STARTS)
def test_the_per_lane_rule_accepts_a_zeroed_hidden_column_of_the_cartpole(start):
    """The gap, pinned: as one more column of a lane's [state | hidden] row the cartpole's hidden column lies below the lane's floor
    3e-4 max |g_smooth| in EVERY lane, so a sweep that returned 0 there passes the per-lane rule with no bad entry -- and fails the
    per-column one (above).  The ball balancer's is large enough to be seen per lane in most lanes."""
    name = "qcp-su"
    g1, g2 = dc.open_loop_hidden_reference(name, start)[:2]
    s1, s2 = state_columns(name, start)
    want, other = np.concatenate([s1, g1], axis=1), np.concatenate([s2, g2], axis=1)
    smooth = dc.smooth_per_lane(want, other)
    assert smooth[:, :s1.shape[1]].mean() > 0.99
    ratio = np.abs(g1[:, 0]) / np.abs(s1).max(axis=1)
    assert ratio.max() < 3e-4 and 1e-7 < np.median(ratio) < 1e-5, (ratio.min(), np.median(ratio), ratio.max())
    zeroed = want.copy()
    zeroed[:, s1.shape[1]:] = 0.0
    bad, worst = dc.within_per_lane(zeroed, want, smooth)
    assert bad == 0.0 and dc.worst_of(zeroed, want, smooth) < 1.0, (bad, worst)
    b1, b2 = dc.open_loop_hidden_reference("qbb", start)[:2]
    q1 = state_columns("qbb", start)[0]
    assert (np.abs(b1).max(axis=1) / np.abs(q1).max(axis=1) > 3e-4).mean() > 0.9 and dc.hidden_conditions("qbb", b1, b2).all()


@pytest.mark.parametrize("name", dc.FAMILIES)
def test_the_tangent_oracle_is_smooth_and_its_null_columns_are_the_listed_ones(name):
    """from the oracle alone: the columns it holds at 0 are NULL_TANGENTS (asserted inside), at most 1 % of the live entries not smooth
    (measured: at most 0.003), no live column without a smooth entry; a negated, a zeroed and a 2 % off array do not pass"""
    o, null, smooth = dc.tangents_conditions(name)
    c = dc.params_case(name)
    G = len(dc.WRT[name])
    assert o.f1.shape == (dc.N, (c["ref"].S + c["ref"].H) * G) and o.theta.shape == (dc.N, G) and (o.theta != 0).all()
    assert np.array_equal(o.length, dc.all_param_oracle(name).length)
    assert not o.f1[:, null].any() and null.sum() == len(dc.NULL_TANGENTS[name])
    assert dc.check_tangents(name, o.f2).max() < 0.1  # the other step size passes
    for wrong in (-o.f1, np.zeros_like(o.f1), 1.02 * o.f2):
        with pytest.raises(AssertionError):
            dc.check_tangents(name, wrong)
    if null.any():  # rounding noise of the size of the floor in a null column does not pass either
        noisy = o.f1.copy()
        noisy[3, np.flatnonzero(null)[0]] = dc.CANCEL_FLOOR * np.abs(o.f1[:, ~null]).max(axis=0).min()
        with pytest.raises(AssertionError):
            dc.check_tangents(name, noisy)


def test_the_all_parameter_oracle_from_hidden_start_keeps_lengths_and_null_columns():
    for name in dc.HIDDEN_FAMILIES:
        a, b = dc.all_param_oracle(name), dc.all_param_oracle(name, "perturbed")
        assert np.array_equal(a.length, b.length) and np.array_equal(a.unit, b.unit) and not np.array_equal(a.f1, b.f1)
        assert np.flatnonzero(dc.null_columns(b.f1, b.f2)).tolist() == sorted(dc.NULL_COLUMNS[name])
        live = ~dc.null_columns(b.f1, b.f2)
        assert dc.smooth_per_column(b.f1[:, live], b.f2[:, live]).mean() > 0.9


def test_scaled_hidden_reads_the_hidden_rows_and_refuses_a_written_lane_beyond_the_batch():
    torch = pytest.importorskip("torch")

    class Face:  # what scaled_hidden uses of the package
        @staticmethod
        def lanes_first(x, n):
            return x[:, :n].t().contiguous()

    c = dc.params_case("qbb")
    S, H, ld = c["ref"].S, c["ref"].H, 192
    d_init = torch.zeros(S + H, ld)
    d_init[:, :dc.N] = torch.arange((S + H) * dc.N, dtype=torch.float32).reshape(S + H, dc.N)
    got = dc.scaled_hidden(Face, c, d_init)
    assert got.dtype == np.float64 and got.shape == (dc.N, H)
    assert np.array_equal(got, d_init[S:, :dc.N].t().numpy().astype(np.float64) * np.array(dc.HIDDEN_SCALE["qbb"]))
    d_init[S + 1, dc.N + 3] = 1e-30
    with pytest.raises(AssertionError):
        dc.scaled_hidden(Face, c, d_init)
