"""Host side of the open-loop policies (no GPU): PlaybackPolicy / TimePolicy of upstream Pyrado policies/feed_forward/playback.py
and time.py, the table the fused kernel replays (playback_kernel_spec), and the lane arithmetic of TrajectoryMatchSampler."""
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from simurlacra_amd import sysid  # noqa: E402
from simurlacra_amd.policies import (IdlePolicy, PlaybackPolicy, TimePolicy, playback_kernel_spec)  # noqa: E402
from simurlacra_amd.spaces import BoxSpace, EnvSpec  # noqa: E402


def spec_of(O=3, A=2):
    return EnvSpec(BoxSpace(-np.ones(O), np.ones(O)), BoxSpace(-np.ones(A), np.ones(A)))


def recordings(lengths=(4, 2, 5), A=2, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.normal(size=(t, A)).astype(np.float32) for t in lengths]


def test_playback_cycles_recordings_and_returns_zeros_past_the_end():
    recs = recordings()
    pol = PlaybackPolicy(spec_of(), recs)
    for cycle in range(2):
        for r, rec in enumerate(recs):
            pol.reset()
            assert pol.curr_rec == r and pol.curr_step == 0  # the first reset() selects recording 0
            for k in range(len(rec) + 3):
                act = pol(torch.zeros(3))
                want = rec[k] if k < len(rec) else np.zeros(2, dtype=np.float32)
                assert act.dtype == torch.float32 and np.array_equal(act.numpy(), want), (cycle, r, k)


def test_playback_no_reset_holds():
    recs = recordings()
    pol = PlaybackPolicy(spec_of(), recs, no_reset=True)
    pol.reset()
    assert np.array_equal(pol().numpy(), recs[0][0])
    pol.reset()  # does nothing: neither the recording nor the step moves
    assert np.array_equal(pol().numpy(), recs[0][1])
    pol.no_reset = False
    pol.reset()
    assert pol.curr_rec == 0 and np.array_equal(pol().numpy(), recs[0][0])
    pol.reset()
    assert pol.curr_rec == 1


def test_actions_at_agrees_with_forward():
    recs = recordings()
    pol = PlaybackPolicy(spec_of(), recs)
    T = 8
    seq = np.zeros((len(recs), T, 2), dtype=np.float32)
    for r in range(len(recs)):
        pol.reset()
        for k in range(T):
            seq[r, k] = pol().numpy()
    steps, rr = np.meshgrid(np.arange(T), np.arange(len(recs)))
    got = pol.actions_at(steps.reshape(-1), rr.reshape(-1))
    assert tuple(got.shape) == (len(recs) * T, 2)
    assert np.array_equal(got.numpy().reshape(len(recs), T, 2), seq)
    assert np.array_equal(pol.actions_at(torch.tensor([1, 7]), torch.tensor([2, 1])).numpy(), np.stack([recs[2][1], np.zeros(2)]))


def test_time_policy_tabulation_equals_forward_bit_for_bit():
    dt = 0.004
    pol = TimePolicy(spec_of(A=2), lambda t: [math.sin(37.0 * t), 2.0 * t * t - 0.1], dt)
    pol.reset()
    seq = np.stack([pol().numpy() for _ in range(50)])
    tab = pol.tabulate(50).numpy()
    assert tab.dtype == np.float32 and np.array_equal(tab, seq)
    # t is accumulated, not k * dt: row 49 is the function at the accumulated float
    t = 0.0
    for _ in range(49):
        t += dt
    assert t != 49 * dt and seq[49, 0] == np.float32(math.sin(37.0 * t))
    pol.reset()
    assert np.array_equal(pol().numpy(), seq[0])
    spec = playback_kernel_spec(pol, max_steps=50)
    assert spec["actions"].shape == (1, 50, 2) and np.array_equal(spec["actions"][0], seq) and list(spec["rec_len"]) == [50]
    assert playback_kernel_spec(pol) is None  # no horizon, no table


def test_kernel_spec_pads_ragged_recordings_and_reports_lengths():
    recs = recordings((4, 2, 5))
    spec = playback_kernel_spec(PlaybackPolicy(spec_of(), recs))
    assert spec["actions"].shape == (3, 5, 2) and spec["actions"].dtype == np.float32
    assert spec["rec_len"].dtype == np.int32 and list(spec["rec_len"]) == [4, 2, 5]
    for r, rec in enumerate(recs):
        assert np.array_equal(spec["actions"][r, : len(rec)], rec) and not spec["actions"][r, len(rec):].any()
    assert playback_kernel_spec(IdlePolicy(spec_of())) is None
    assert playback_kernel_spec(None) is None


def test_package_exports():
    import simurlacra_amd as vs

    assert vs.PlaybackPolicy is PlaybackPolicy and vs.TimePolicy is TimePolicy and vs.playback_kernel_spec is playback_kernel_spec
    assert vs.TrajectoryMatchSampler is sysid.TrajectoryMatchSampler


def test_trajectory_match_lane_arithmetic():
    R = 3
    for p in range(5):
        for r in range(R):
            lane = sysid.lane_of(p, r, R)
            assert lane == p * R + r and sysid.pair_of(lane, R) == (p, r)
    assert list(sysid.batch_lane_rec(2, R)) == [0, 1, 2, 0, 1, 2]
    # 5 candidates x 3 segments in batches of at most 6 lanes: whole candidates only
    assert sysid.candidate_batches(5, 3, 6) == [(0, 2), (2, 4), (4, 5)]
    assert sysid.candidate_batches(5, 3, 65536) == [(0, 5)]
    assert sysid.candidate_batches(4, 3, 2) == [(0, 1), (1, 2), (2, 3), (3, 4)]  # a candidate is never split
    assert sysid.candidate_batches(0, 3, 6) == []
    for P, batch in ((1024, 65536), (1025, 65536), (7, 13)):
        cuts = sysid.candidate_batches(P, 64 if batch > 100 else 3, batch)
        assert cuts[0][0] == 0 and cuts[-1][1] == P and all(a[1] == b[0] for a, b in zip(cuts, cuts[1:]))
    tab, lens = sysid.pad_recordings([np.ones((3, 2)), np.ones((5, 2))], 2, extra_rows=1)
    assert tab.shape == (2, 5, 2) and list(lens) == [2, 4] and not tab[0, 3:].any()
    with pytest.raises(Exception):
        sysid.pad_recordings([np.ones((3, 3))], 2)
