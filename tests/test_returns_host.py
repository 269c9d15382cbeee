"""vs_returns_scan without a GPU: the semantics of the entry point restated as a sequential fp64 NumPy function (the reference
of tests/test_gpu_returns.py) against hand-computed cases, the packed-row layout helper, and the argument refusals, all of which
return before the first device call."""
import ctypes as C

import numpy as np
import pytest

from simurlacra_amd import _lib as L

RETURN, GAE = L.VS_RETURNS_RETURN, L.VS_RETURNS_GAE


def returns_reference(lengths, rew, gamma, lam=1.0, mode=RETURN, values=None, done_last=None):
    """include/vecsim.h, vs_returns_scan, step by step in fp64.  rew / values: one entry per packed row (dense).
    Returns (out [rows], out_first [n], S [rows]); S_t = sum_k c^k D_{t+k} is the magnitude the error bound of the GPU test scales
    with: D = |rew| (RETURN), |rew_t| + gamma |V_{t+1}| + |V_t| (GAE), and the bootstrap value in the final-entry row."""
    lengths = np.asarray(lengths, dtype=np.int64)
    rew = np.asarray(rew, dtype=np.float64)
    vals = None if values is None else np.asarray(values, dtype=np.float64)
    gamma, lam = float(gamma), float(lam)
    if mode == GAE and vals is None:
        raise ValueError("GAE needs values")
    n = len(lengths)
    rows = int(lengths.sum()) + n
    out, S, first = np.zeros(rows), np.zeros(rows), np.zeros(n)
    b = 0
    for j in range(n):
        Lj = int(lengths[j])
        keep = 0.0 if (done_last is not None and done_last[j]) else 1.0
        v_last = 0.0 if vals is None else vals[b + Lj] * keep
        if mode == RETURN:
            c = gamma
            y = v_last
        else:
            c = gamma * lam
            y = 0.0
        s = abs(y)
        out[b + Lj], S[b + Lj] = y, s
        for t in range(Lj - 1, -1, -1):
            if mode == RETURN:
                x, d = rew[b + t], abs(rew[b + t])
            else:
                v_next = v_last if t == Lj - 1 else vals[b + t + 1]
                x = rew[b + t] + gamma * v_next - vals[b + t]
                d = abs(rew[b + t]) + gamma * abs(v_next) + abs(vals[b + t])
            y = x + c * y
            s = d + c * s
            out[b + t], S[b + t] = y, s
        first[j] = y
        b += Lj + 1
    return out, first, S


def returns_reference_batched(lengths, rew, gamma, lam=1.0, mode=RETURN, values=None, done_last=None):
    """returns_reference with the rollouts side by side: the same fp64 operations in the same order per rollout (sequential
    backwards in time), one NumPy operation per time step over all rollouts that have that step -- for the large batches"""
    from simurlacra_amd.sampling import packed_row_layout

    lengths = np.asarray(lengths, dtype=np.int64)
    rew = np.asarray(rew, dtype=np.float64)
    vals = None if values is None else np.asarray(values, dtype=np.float64)
    gamma, lam = float(gamma), float(lam)
    _, base, final, rows = packed_row_layout(lengths)
    order = np.argsort(-lengths, kind="stable")  # the rollouts that have step t are a prefix of this order
    base_o, len_o = base[order], lengths[order]
    keep = np.ones(len(lengths)) if done_last is None else np.where(np.asarray(done_last, dtype=bool), 0.0, 1.0)
    v_last = np.zeros(len(lengths)) if vals is None else vals[final] * keep
    c = gamma if mode == RETURN else gamma * lam
    y = (v_last if mode == RETURN else np.zeros(len(lengths)))[order].copy()
    v_last = v_last[order]
    s = np.abs(y)
    out, S = np.zeros(rows), np.zeros(rows)
    out[final[order]], S[final[order]] = y, s
    for t in range(int(lengths.max()) - 1, -1, -1):
        k = int(np.searchsorted(-len_o, -t, side="left"))  # rollouts with length > t
        r = base_o[:k] + t
        if mode == RETURN:
            x, d = rew[r], np.abs(rew[r])
        else:
            v_next = np.where(len_o[:k] - 1 == t, v_last[:k], vals[np.minimum(r + 1, rows - 1)])
            x = rew[r] + gamma * v_next - vals[r]
            d = np.abs(rew[r]) + gamma * np.abs(v_next) + np.abs(vals[r])
        y[:k] = x + c * y[:k]
        s[:k] = d + c * s[:k]
        out[r], S[r] = y[:k], s[:k]
    first = np.empty(len(lengths))
    first[order] = y
    return out, first, S


def test_batched_reference_is_the_sequential_one():
    rng = np.random.default_rng(5)
    lengths = np.concatenate([rng.integers(0, 9, 40), [0, 0, 1, 37, 1, 0]])
    rows = int(lengths.sum()) + len(lengths)
    rew, vals, done = rng.normal(size=rows), rng.normal(size=rows), rng.random(len(lengths)) < 0.5
    for mode in (RETURN, GAE):
        for v, dl in ((vals, done), (vals, None), (None, None)):
            if mode == GAE and v is None:
                continue
            a = returns_reference(lengths, rew, 0.9, 0.8, mode, v, dl)
            b = returns_reference_batched(lengths, rew, 0.9, 0.8, mode, v, dl)
            for x, y in zip(a, b):
                assert np.array_equal(x, y)


def test_reference_length_one_and_zero():
    out, first, S = returns_reference([1, 0, 1], [2.0, 9.0, 9.0, -3.0, 9.0], 0.5)
    assert out.tolist() == [2.0, 0.0, 0.0, -3.0, 0.0] and first.tolist() == [2.0, 0.0, -3.0]  # the final-entry rewards are not read
    assert S.tolist() == [2.0, 0.0, 0.0, 3.0, 0.0]
    # with values: a length-1 rollout bootstraps, an L = 0 rollout is its bootstrap value
    vals = [10.0, 4.0, 7.0, 20.0, 8.0]
    out, first, _ = returns_reference([1, 0, 1], [2.0, 9.0, 9.0, -3.0, 9.0], 0.5, values=vals)
    assert out.tolist() == [2.0 + 0.5 * 4.0, 4.0, 7.0, -3.0 + 0.5 * 8.0, 8.0] and first.tolist() == [4.0, 7.0, 1.0]


def test_reference_gamma_zero_and_one():
    rew = [1.0, 2.0, 3.0, 99.0, 4.0, 5.0, 99.0]
    out, first, _ = returns_reference([3, 2], rew, 0.0)
    assert out.tolist() == [1.0, 2.0, 3.0, 0.0, 4.0, 5.0, 0.0] and first.tolist() == [1.0, 4.0]
    out, first, S = returns_reference([3, 2], rew, 1.0)
    assert out.tolist() == [6.0, 5.0, 3.0, 0.0, 9.0, 5.0, 0.0] and first.tolist() == [6.0, 9.0]
    assert S.tolist() == out.tolist()  # (positive rewards)
    out, _, _ = returns_reference([3], [1.0, 2.0, 3.0, 0.0], 0.5)
    assert out.tolist() == [1.0 + 0.5 * (2.0 + 0.5 * 3.0), 2.0 + 0.5 * 3.0, 3.0, 0.0]


def test_reference_done_last_zeroes_the_bootstrap():
    rew, vals = [1.0, 1.0, 0.0, 1.0, 1.0, 0.0], [0.5, 0.25, 8.0, 0.5, 0.25, 8.0]
    out, first, _ = returns_reference([2, 2], rew, 0.5, values=vals, done_last=[True, False])
    assert out.tolist() == [1.5, 1.0, 0.0, 1.0 + 0.5 * 5.0, 1.0 + 0.5 * 8.0, 8.0]
    assert first.tolist() == [1.5, 3.5]
    # GAE: the final value is zeroed in delta_{L-1} as well, and the final-entry row holds A_L = 0
    out, first, S = returns_reference([2, 2], rew, 0.5, 1.0, GAE, values=vals, done_last=[True, False])
    d = [1.0 + 0.5 * 0.25 - 0.5, 1.0 + 0.5 * 0.0 - 0.25, 1.0 + 0.5 * 0.25 - 0.5, 1.0 + 0.5 * 8.0 - 0.25]
    assert out.tolist() == [d[0] + 0.5 * d[1], d[1], 0.0, d[2] + 0.5 * d[3], d[3], 0.0]
    assert S[1] == 1.0 + 0.25 and S[4] == 1.0 + 0.5 * 8.0 + 0.25 and S[2] == 0.0


def test_reference_lambda_zero_and_one():
    rng = np.random.default_rng(0)
    lengths = [4, 1, 0, 3]
    rows = sum(lengths) + len(lengths)
    rew, vals = rng.normal(size=rows), rng.normal(size=rows)
    gamma = 0.9
    # lam = 0: the one-step TD error
    out, _, _ = returns_reference(lengths, rew, gamma, 0.0, GAE, values=vals)
    b = 0
    for Lj in lengths:
        for t in range(Lj):
            assert out[b + t] == rew[b + t] + gamma * vals[b + t + 1] - vals[b + t]
        assert out[b + Lj] == 0.0
        b += Lj + 1
    # lam = 1: the bootstrapped reward-to-go minus the value
    out, first, _ = returns_reference(lengths, rew, gamma, 1.0, GAE, values=vals)
    rtg, _, _ = returns_reference(lengths, rew, gamma, values=vals)
    b = 0
    for j, Lj in enumerate(lengths):
        np.testing.assert_allclose(out[b:b + Lj], rtg[b:b + Lj] - vals[b:b + Lj], rtol=0, atol=1e-14)
        assert first[j] == (out[b] if Lj else 0.0)
        b += Lj + 1
    with pytest.raises(ValueError):
        returns_reference(lengths, rew, gamma, 1.0, GAE)


def test_reference_matches_step_sequence_discounted_return():
    from simurlacra_amd.sampling import StepSequence

    rng = np.random.default_rng(1)
    rew = rng.normal(size=37)
    ro = StepSequence(observations=np.zeros((38, 1)), actions=np.zeros((37, 1)), rewards=rew)
    _, first, _ = returns_reference([37], np.append(rew, 0.0), 0.97)
    assert first[0] == pytest.approx(ro.discounted_return(0.97), rel=1e-13)


def test_packed_row_layout():
    from simurlacra_amd.sampling import packed_row_layout

    starts, base, final, rows = packed_row_layout([3, 0, 1, 2])
    assert starts.tolist() == [0, 3, 3, 4] and base.tolist() == [0, 4, 5, 7] and final.tolist() == [3, 4, 6, 9] and rows == 10
    assert starts.dtype == base.dtype == final.dtype == np.int64
    starts, base, final, rows = packed_row_layout([5])
    assert (starts.tolist(), base.tolist(), final.tolist(), rows) == ([0], [0], [5], 6)


@pytest.fixture(scope="module")
def lib():
    from simurlacra_amd.csrc import build

    build.build()
    return L.load()


def test_argument_refusals_come_before_any_device_call(lib):
    """every refusal of vs_returns_scan is VS_ERR_ARG with its reason in vs_last_error(NULL) -- also on a machine without a GPU,
    where the first device call would answer VS_ERR_HIP; the pointers are never followed"""
    assert lib.vs_version() >= 306
    p = C.c_void_p(256)  # stands for device memory

    def call(n=4, lengths=p, starts=p, rew=p, rs=1, values=None, vs_=1, done=None, gamma=0.9, lam=0.9, mode=RETURN, out=p, first=None):
        return lib.vs_returns_scan(0, None, n, lengths, starts, rew, rs, values, vs_, done, gamma, lam, mode, out, first)

    def refused(match, **kw):
        assert call(**kw) == L.VS_ERR_ARG, kw
        assert match in lib.vs_last_error(None).decode(), (kw, lib.vs_last_error(None))

    refused("n must", n=0)
    refused("n must", n=-3)
    for k in ("lengths", "starts", "rew", "out"):
        refused("must not be NULL", **{k: None})
    refused("needs values", mode=GAE)
    refused("unknown mode", mode=2)
    refused("unknown mode", mode=-1)
    refused("stride", rs=0)
    refused("stride", values=p, vs_=0)
    refused("stride", rs=-13)
    refused("gamma", gamma=1.5)
    refused("gamma", gamma=-0.1)
    refused("gamma", gamma=float("nan"))
    refused("lam", lam=1.0001)
    refused("lam", lam=-1.0, mode=GAE, values=p)
