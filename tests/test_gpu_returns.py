"""vs_returns_scan on the GPU: the segmented scan against the fp64 restatement of tests/test_returns_host.py on synthetic ragged
batches, through PackedRollouts on the sampler's rollouts, and ParameterExploringSampler.sample_returns against sample().

The tolerance is derived, not tuned: with u = 2^-24 and S_t = sum_k c^k D_{t+k} (the same recurrence over magnitudes, the bootstrap
term included), |y_t - ref_t| <= 2 (L - t + 8) u S_t.  Every term reaches y_t through at most L - t multiply-add pairs in the
sequential order; the kernel's tree has fewer additions and its powers of c by squaring carry at most the same count of roundings;
the + 8 covers the rounding of delta_t and of the carries between waves and tiles.  The reference gets the float32 values of gamma
and lam that the entry point gets.  Run with -s to see the worst ratio to the bound of every test.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from test_returns_host import GAE, RETURN, returns_reference_batched  # noqa: E402

U = 2.0 ** -24
STRIDES, GAMMAS, LAMS = (1, 8, 13), (0.0, 0.9, 0.99, 1.0), (0.0, 0.95, 1.0)
KINDS = ("ones", "zero_one", "short", "geometric", "long")


@pytest.fixture(scope="module")
def vs():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import simurlacra_amd

    return simurlacra_amd


@pytest.fixture(scope="module")
def lib(vs):
    from simurlacra_amd import _lib

    return _lib.load()


def draw_lengths(kind, n, rng):
    if kind == "ones":
        return np.ones(n, dtype=np.int64)
    if kind == "zero_one":
        return rng.integers(0, 2, n).astype(np.int64)
    if kind == "short":
        return rng.integers(1, 9, n).astype(np.int64)
    if kind == "geometric":
        return np.minimum(rng.geometric(1.0 / 500.0, n), 4000).astype(np.int64)
    return np.full(n, 4000, dtype=np.int64)


def edge_batch():
    """a rollout boundary on every position of a 64-, a 256- and a 1024-row tile: rollouts of 65, 257 and 1025 rows, as many of each
    as the tile has rows, and a few that span several tiles"""
    return np.concatenate([np.full(64, 64), np.full(256, 256), np.full(1024, 1024), [4000, 3, 0, 2500, 1, 4000]]).astype(np.int64)


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def raw_scan(lib, lengths, starts, rew, values, done, gamma, lam, mode, out, first):
    """the C entry point as it is, on torch's current stream; rew / values are 1-D views with any stride"""
    rc = lib.vs_returns_scan(torch.cuda.current_device(), C.c_void_p(torch.cuda.current_stream().cuda_stream or 1), int(lengths.shape[0]),
                             ptr(lengths), ptr(starts), ptr(rew), int(rew.stride(0)), ptr(values),
                             1 if values is None else int(values.stride(0)), ptr(done), float(gamma), float(lam), int(mode), ptr(out),
                             ptr(first))
    assert rc == 0, lib.vs_last_error(None)


def row_bound(lengths, S):
    from simurlacra_amd.sampling import packed_row_layout

    _, _, final, rows = packed_row_layout(lengths)
    jr = np.repeat(np.arange(len(lengths)), lengths + 1)
    return 2.0 * (final[jr] - np.arange(rows) + 8) * U * S


def worst_ratio(err, bound):
    assert (err <= bound).all(), (float((err - bound).max()), int(np.argmax(err - bound)))
    pos = bound > 0
    return float((err[pos] / bound[pos]).max()) if pos.any() else 0.0


def check(lib, lengths, stride, gamma, lam, mode, with_values, with_done, seed):
    """one batch: kernel against reference at the bound, final-entry rows and out_first exact, two launches the same bits"""
    from simurlacra_amd.sampling import packed_row_layout

    n = len(lengths)
    starts, base, final, rows = packed_row_layout(lengths)
    g = torch.Generator(device="cuda").manual_seed(seed)
    rew = torch.randn(rows, stride, generator=g, device="cuda")[:, stride - 1]  # a column of a wider matrix, read where it lies
    values = torch.randn(rows, 2, generator=g, device="cuda")[:, 0] if (with_values or mode == GAE) else None
    done = (torch.rand(n, generator=g, device="cuda") < 0.5).to(torch.uint8) if (with_done and values is not None) else None
    len_d, sta_d = torch.from_numpy(lengths).cuda(), torch.from_numpy(starts).cuda()
    outs = []
    for _ in range(2):
        out = torch.full((rows,), float("nan"), device="cuda")
        first = torch.full((n,), float("nan"), device="cuda")
        raw_scan(lib, len_d, sta_d, rew, values, done, gamma, lam, mode, out, first)
        outs.append((out, first))
    (out, first), (out2, first2) = outs
    assert torch.equal(out.view(torch.int32), out2.view(torch.int32)) and torch.equal(first.view(torch.int32), first2.view(torch.int32))
    ref, ref_first, S = returns_reference_batched(lengths, rew.cpu().numpy(), np.float32(gamma), np.float32(lam), mode,
                                                  None if values is None else values.cpu().numpy(),
                                                  None if done is None else done.cpu().numpy())
    got, got_first = out.cpu().numpy(), first.cpu().numpy()
    assert np.isfinite(got).all()
    ratio = worst_ratio(np.abs(got.astype(np.float64) - ref), row_bound(lengths, S))
    assert np.array_equal(got[final].astype(np.float64), ref[final])          # the bootstrap value or 0: no arithmetic
    assert np.array_equal(got_first.view(np.int32), got[base].view(np.int32))  # out_first is out's first row of the rollout
    # ... and against the reference: exact where no arithmetic happens (L = 0: the bootstrap value or 0), else at the row's bound
    assert np.array_equal(got_first[lengths == 0].astype(np.float64), ref_first[lengths == 0])
    worst_ratio(np.abs(got_first.astype(np.float64) - ref_first), 2.0 * (lengths + 8) * U * S[base])
    return ratio


def test_kernel_against_reference_on_ragged_batches(lib):
    """every n with every length distribution (all 4 000 at the small n); strides, gamma, lam, mode, values and done_last cycle so
    that every value of each meets every batch size"""
    rng = np.random.default_rng(0)
    i, worst = 0, {}
    for n in (1, 63, 257, 4096, 65536):
        for kind in KINDS:
            if kind == "long" and n > 257:
                continue
            lengths = draw_lengths(kind, n, rng)
            reps = 1 if (n == 65536 and kind == "geometric") else 2
            for _ in range(reps):
                mode = (RETURN, GAE)[i % 2]
                r = check(lib, lengths, STRIDES[i % 3], GAMMAS[(i // 2) % 4], LAMS[(i // 3) % 3], mode, (i // 5) % 2 == 0, (i // 4) % 2 == 0,
                          seed=i)
                worst[(n, kind, "GAE" if mode == GAE else "RETURN")] = r
                i += 1
    print("\nworst |err| / bound per case:", {k: round(v, 4) for k, v in worst.items()})
    print("worst ratio to the bound, ragged batches:", max(worst.values()))


def test_kernel_every_gamma_lam_mode_and_stride(lib):
    """the full cross of gamma x lam x mode x done_last (strides cycling) on short rollouts (1 .. 8) and on 0 / 1 mixed"""
    rng = np.random.default_rng(1)
    worst, i = 0.0, 0
    for kind in ("short", "zero_one"):
        lengths = draw_lengths(kind, 257, rng)
        for gamma in GAMMAS:
            for lam in LAMS:
                for mode in (RETURN, GAE):
                    for with_done in (False, True):
                        worst = max(worst, check(lib, lengths, STRIDES[i % 3], gamma, lam, mode, True, with_done, seed=100 + i))
                        i += 1
        worst = max(worst, check(lib, lengths, 13, 0.99, 1.0, RETURN, False, False, seed=99))  # no values: y_L = 0
    print("\nworst ratio to the bound, full cross:", worst)


def test_kernel_rollout_boundaries_on_every_tile_position(lib):
    from simurlacra_amd.sampling import packed_row_layout

    lengths = edge_batch()
    _, base, final, _ = packed_row_layout(lengths)
    for tile in (64, 256, 1024):
        assert len(set((base % tile).tolist())) == tile and len(set((final % tile).tolist())) == tile
    worst, i = 0.0, 0
    for gamma in GAMMAS:
        for mode in (RETURN, GAE):
            for with_done in (False, True):
                worst = max(worst, check(lib, lengths, STRIDES[i % 3], gamma, LAMS[i % 3], mode, True, with_done, seed=200 + i))
                i += 1
    print("\nworst ratio to the bound, tile edges:", worst)


def test_kernel_sub_range_leaves_the_other_rows_alone(lib):
    """rollouts j0 .. j1 - 1 of a batch: lengths + j0, starts + j0 and the row pointers advanced by j0 rows (include/vecsim.h)"""
    from simurlacra_amd.sampling import packed_row_layout

    rng = np.random.default_rng(2)
    lengths = np.concatenate([draw_lengths("short", 300, rng), draw_lengths("geometric", 40, rng), draw_lengths("zero_one", 100, rng)])
    rng.shuffle(lengths)
    n = len(lengths)
    starts, base, final, rows = packed_row_layout(lengths)
    g = torch.Generator(device="cuda").manual_seed(7)
    rew = torch.randn(rows, 8, generator=g, device="cuda")[:, 7]
    values = torch.randn(rows, generator=g, device="cuda")
    done = (torch.rand(n, generator=g, device="cuda") < 0.5).to(torch.uint8)
    len_d, sta_d = torch.from_numpy(lengths).cuda(), torch.from_numpy(starts).cuda()
    for mode in (RETURN, GAE):
        ref, ref_first, S = returns_reference_batched(lengths, rew.cpu().numpy(), np.float32(0.99), np.float32(0.95), mode,
                                                      values.cpu().numpy(), done.cpu().numpy())
        bound = row_bound(lengths, S)
        for j0, j1 in ((0, n), (17, 230), (n - 1, n), (5, 6), (200, n)):
            marker = -12345.0
            out = torch.full((rows,), marker, device="cuda")
            first = torch.full((n,), marker, device="cuda")
            raw_scan(lib, len_d[j0:j1], sta_d[j0:j1], rew[j0:], values[j0:], done[j0:j1], 0.99, 0.95, mode, out[j0:], first[j0:j1])
            got, got_first = out.cpu().numpy(), first.cpu().numpy()
            a, b = int(base[j0]), int(final[j1 - 1]) + 1
            assert (got[:a] == marker).all() and (got[b:] == marker).all()
            assert (got_first[:j0] == marker).all() and (got_first[j1:] == marker).all()
            worst_ratio(np.abs(got[a:b].astype(np.float64) - ref[a:b]), bound[a:b])
            assert np.array_equal(got_first[j0:j1], got[base[j0:j1]])
            worst_ratio(np.abs(got_first[j0:j1].astype(np.float64) - ref_first[j0:j1]), bound[base[j0:j1]])


def test_kernel_keeps_a_non_finite_rollout_to_itself(lib):
    """the final-entry row cuts the carry by a select, not by a multiplication with 0: a NaN or Inf reward or value in one rollout
    reaches the rows of that rollout only (as in the sequential recurrence), whatever tile, wave or chunk its neighbours share"""
    from simurlacra_amd.sampling import packed_row_layout

    rng = np.random.default_rng(3)
    lengths = np.concatenate([draw_lengths("short", 200, rng), [1500, 3, 2600, 0, 5], draw_lengths("zero_one", 60, rng),
                              draw_lengths("short", 200, rng)]).astype(np.int64)
    n = len(lengths)
    starts, base, final, rows = packed_row_layout(lengths)
    g = torch.Generator(device="cuda").manual_seed(9)
    rew0 = torch.randn(rows, generator=g, device="cuda")
    val0 = torch.randn(rows, generator=g, device="cuda")
    len_d, sta_d = torch.from_numpy(lengths).cuda(), torch.from_numpy(starts).cuda()
    poisoned = [5, 199, 200, 201, 202, 204, 230, n - 1]  # short ones, both tile-crossing ones, their neighbours, the last
    poisoned = [j for j in poisoned if lengths[j] > 0]
    own = np.zeros(rows, dtype=bool)
    for j in poisoned:
        own[base[j]:final[j] + 1] = True
    for mode in (RETURN, GAE):
        clean = torch.empty(rows, device="cuda")
        clean_first = torch.empty(n, device="cuda")
        raw_scan(lib, len_d, sta_d, rew0, val0, None, 0.99, 0.95, mode, clean, clean_first)
        for bad, in_values in ((float("nan"), False), (float("inf"), False), (float("nan"), True), (float("-inf"), True)):
            rew, val = rew0.clone(), val0.clone()
            for j in poisoned:
                if in_values:
                    val[int(final[j])] = bad  # the value of the final observation (no done_last: it bootstraps)
                else:
                    rew[int(base[j]) + int(lengths[j]) // 2] = bad  # a step in the middle of the rollout
            out = torch.empty(rows, device="cuda")
            first = torch.empty(n, device="cuda")
            raw_scan(lib, len_d, sta_d, rew, val, None, 0.99, 0.95, mode, out, first)
            got, want = out.cpu().numpy(), clean.cpu().numpy()
            assert np.array_equal(got[~own].view(np.int32), want[~own].view(np.int32)), (mode, bad, in_values)
            keep = np.ones(n, dtype=bool)
            keep[poisoned] = False
            assert np.array_equal(first.cpu().numpy()[keep].view(np.int32), clean_first.cpu().numpy()[keep].view(np.int32))
            assert not np.isfinite(got[base[poisoned]]).any()  # ... and it does reach the first row of its own rollout


# ------------------------------------------------------------------------------------------------ through the sampler
def rollout_bound(ros, gamma):
    """(reference discounted returns, the bound on them) of host rollouts"""
    ref = np.array([ro.discounted_return(gamma) for ro in ros])
    S = np.array([float(np.sum(np.abs(ro.rewards) * gamma ** np.arange(len(ro)))) for ro in ros])
    return ref, 2.0 * (np.array([len(ro) for ro in ros]) + 8) * U * S


def close_pairs(ref, bound):
    """sorted by the reference: which neighbouring pairs differ by no more than the bound (of either)"""
    order = np.argsort(ref, kind="stable")
    gap = np.diff(ref[order])
    return order, gap <= np.maximum(bound[order][:-1], bound[order][1:])


SAMPLER_CASES = {"qq-su": dict(cls="QQubeSwingUpSim", dt=0.004, n=4096, pilot=1000, seeds=(11,), assert_close=False),
                 "qcp-su": dict(cls="QCartPoleSwingUpSim", dt=0.002, n=256, pilot=60, seeds=(11, 12, 13, 14), assert_close=True)}


@pytest.mark.parametrize("name", list(SAMPLER_CASES))
def test_packed_rollouts_against_the_host_rollouts(vs, name):
    """sample_packed() against sample() of the same seed and call count, rollout for rollout.

    Both ends occur: max_steps is put between the shortest and the longest rollout of a pilot run, so some rollouts fail before the
    step limit and some run into it.  `done_last` is StepSequence.done[-1], and the env's done flag is set at the step limit too (as
    the reference's), so it is True for both ends (asserted equal to the host rollouts' done[-1]).  The flag that tells the ends
    apart is `failed_last` (Task.has_failed of the last step): both of its values are asserted to be present, it is checked against
    the lengths, and it is what gae / rewards_to_go zero the bootstrap with.  The entry point is also run with `done_last` itself.

    select_cvar.  The issue's form: the index lists are equal wherever neighbouring reference returns differ by more than the bound,
    and at most 1 % of the pairs are that close, the seed being the first of a short list whose REFERENCE returns satisfy this.
    That holds and is asserted on the cartpole batch (256 rollouts of <= 60 steps).  On the 4 096 QQube rollouts the reference alone
    puts 14.4 % of the neighbouring pairs within the bound (measured, seed 11, max_steps 562; the bound is 2 (L + 8) u S ~ 7e-5 S at
    L ~ 560 and 4 096 returns lie ~ 2.4e-4 of their range apart on average), whatever the code under test computes, so no seed can
    meet 1 % there.  Both batches therefore also assert, with tol = 2 max(bound) (two values can only swap places in the order if
    their references are no further apart than the sum of their bounds, and then so is every gap between them):
      * the reference returns of the device's selection, position by position, are within tol of the host's k lowest (order
        statistics of two sequences that differ by at most max(bound) element-wise differ by at most that; one more bound from the
        device value back to its reference);
      * every position where the two index lists differ lies in a run of neighbouring pairs no further apart than tol;
      * the two selections are the same SET up to members of the run that straddles position k."""
    from simurlacra_amd.policies import DummyPolicy
    from simurlacra_amd.sampling import ParallelRolloutSampler, returns_scan, select_cvar

    case = SAMPLER_CASES[name]
    mk = lambda max_steps: getattr(vs, case["cls"])(dt=case["dt"], max_steps=max_steps)
    n, gamma, lam = case["n"], 0.99, 0.95
    env = mk(case["pilot"])
    smp = ParallelRolloutSampler(env, DummyPolicy(env.spec), 1, min_rollouts=n, seed=case["seeds"][0])
    pilot = smp.sample_packed()[0].lengths
    smp.close()
    lo, hi = int(pilot.min()), int(pilot.max())
    assert lo < hi, "the pilot run's rollouts all have one length"
    max_steps = (lo + hi) // 2 + 1
    env = mk(max_steps)
    pol = DummyPolicy(env.spec)
    for seed in case["seeds"]:
        smp = ParallelRolloutSampler(env, pol, 1, min_rollouts=n, seed=seed)
        ros = smp.sample()
        smp.close()
        ref, bound = rollout_bound(ros, gamma)
        order, close = close_pairs(ref, bound)
        if close.mean() <= 0.01 or not case["assert_close"]:
            break
    print(f"\n{name}: seed {seed}, max_steps {max_steps}, {close.mean():.4f} of the neighbouring pairs within the bound")
    if case["assert_close"]:
        assert close.mean() <= 0.01
    smp = ParallelRolloutSampler(env, pol, 1, min_rollouts=n, seed=seed)
    (p,) = smp.sample_packed()
    smp.close()
    lengths = p.lengths.cpu().numpy()
    assert np.array_equal(lengths, [len(ro) for ro in ros])
    timed_out = lengths == max_steps
    assert timed_out.any() and not timed_out.all()  # both ends
    assert np.array_equal(p.done_last.cpu().numpy(), [bool(ro.done[-1]) for ro in ros])  # the env's done: set at the step limit too
    failed = p.failed_last.cpu().numpy()
    assert p.failed_last.is_cuda and p.failed_last.dtype == torch.bool and failed.shape == (n,)
    assert failed.any() and not failed.all()                         # both values of the flag that zeroes the bootstrap
    assert failed[~timed_out].all() and timed_out[~failed].all()     # a rollout that stopped early failed; one that did not fail ran out
    print(f"{name}: {int(timed_out.sum())} of {n} rollouts ran into the step limit, {int(failed.sum())} failed; "
          f"done_last True for {int(p.done_last.sum())}")
    # discounted returns against StepSequence.discounted_return, and gamma = 1 against undiscounted_returns()
    got = p.discounted_returns(gamma)
    assert got.is_cuda and got.dtype == torch.float32 and got.shape == (n,)
    r1 = worst_ratio(np.abs(got.cpu().numpy().astype(np.float64) - ref), bound)
    ref1, bound1 = rollout_bound(ros, 1.0)
    one = p.discounted_returns(1.0).cpu().numpy().astype(np.float64)
    r2 = worst_ratio(np.abs(one - ref1), bound1)
    r3 = worst_ratio(np.abs(one - p.undiscounted_returns().cpu().numpy().astype(np.float64)), bound1)
    # GAE and the bootstrapped reward-to-go with a small value network on the packed observations, as the [:, 0] view of its output
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(p.observations.shape[1], 16), torch.nn.Tanh(), torch.nn.Linear(16, 2)).cuda()
    with torch.no_grad():
        values = net(p.observations)[:, 0]
    assert not values.is_contiguous() and values.shape == (p.total_steps + n,)
    rew_h, val_h = p.rewards.cpu().numpy(), values.cpu().numpy()
    rows = p.total_steps + n
    r4 = []
    for flag in ("failed_last", "done_last"):
        if flag == "failed_last":  # the methods: a failure zeroes the final value, a time-out bootstraps
            adv, rtg = p.gae(values, gamma, lam), p.rewards_to_go(gamma, values)
        else:                      # the entry point with the env's done flag: nothing bootstraps
            adv = returns_scan(p.lengths, p.offsets[:-1], p.rewards, rows, GAE, gamma, lam, values, p.done_last)[0]
            rtg = returns_scan(p.lengths, p.offsets[:-1], p.rewards, rows, RETURN, gamma, 1.0, values, p.done_last)[0]
        dl_h = getattr(p, flag).cpu().numpy()
        assert adv.shape == rtg.shape == (rows,) and adv.is_cuda
        for got_rows, mode, lam_ in ((adv, GAE, lam), (rtg, RETURN, 1.0)):
            ref_rows, _, S = returns_reference_batched(lengths, rew_h, np.float32(gamma), np.float32(lam_), mode, val_h, dl_h)
            r4.append(worst_ratio(np.abs(got_rows.cpu().numpy().astype(np.float64) - ref_rows), row_bound(lengths, S)))
    final = (p.offsets[1:] + torch.arange(n, device=p.offsets.device)).cpu().numpy()
    boot = p.rewards_to_go(gamma, values).cpu().numpy()[final]
    assert np.array_equal(boot, np.where(failed, np.float32(0), val_h[final]))  # the time-outs bootstrap, exactly
    plain = p.rewards_to_go(gamma)
    ref_rows, ref_first, S = returns_reference_batched(lengths, rew_h, np.float32(gamma))
    r4.append(worst_ratio(np.abs(plain.cpu().numpy().astype(np.float64) - ref_rows), row_bound(lengths, S)))
    print(f"{name}: worst ratio to the bound: discounted {r1:.4f}, gamma = 1 {r2:.4f}, against undiscounted_returns() {r3:.4f}, "
          f"gae / rewards_to_go {max(r4):.4f}")
    # refusals
    for bad in (values.double(), values[:-1], values.cpu(), val_h):
        with pytest.raises(vs.ValueErr):
            p.gae(bad, gamma, lam)
    with pytest.raises(vs.ValueErr):
        p.discounted_returns(1.5)
    # select_cvar on the device against the host's
    eps = 0.2
    idx = p.select_cvar(eps, gamma)
    assert idx.is_cuda and idx.dtype == torch.int64
    number = {id(ro): j for j, ro in enumerate(ros)}
    host = np.array([number[id(ro)] for ro in select_cvar(list(ros), eps, gamma)])
    idx = idx.cpu().numpy()
    assert idx.shape == host.shape == (round(n * eps),)
    k = len(host)
    assert np.array_equal(host, order[:k])  # (the host's selection is the reference order)
    near = np.zeros(n, dtype=bool)  # the issue's form: positions of the sorted order with a neighbour within the bound
    near[:-1] |= close
    near[1:] |= close
    assert np.array_equal(idx[~near[:k]], host[~near[:k]])
    tol = 2.0 * bound.max()
    assert (np.abs(ref[idx] - ref[host]) <= tol).all()  # the selected returns, position by position
    cut = np.diff(ref[order]) > tol                      # a gap that no pair of device values can cross
    run = np.concatenate([[0], np.cumsum(cut)])          # the run of close pairs every position of the order belongs to
    in_run = np.zeros(n, dtype=bool)                     # ... and whether that run has more than one member
    in_run[:-1] |= ~cut
    in_run[1:] |= ~cut
    differ = idx != host
    assert in_run[:k][differ].all()
    straddle = set(order[(run == run[k - 1]) | (run == run[min(k, n - 1)])].tolist())
    assert (set(idx.tolist()) ^ set(host.tolist())) <= straddle
    print(f"{name}: select_cvar: {int(differ.sum())} of {k} positions differ from the host's, all inside runs of close pairs; "
          f"{near[:k].mean():.4f} of the positions have a neighbour within the bound")
    with pytest.raises(vs.ValueErr):
        p.select_cvar(1e-6, gamma)


# ------------------------------------------------------------------------------------------------ populations
def make_policy(vs, kind, env):
    torch.manual_seed(0)
    return vs.FNNPolicy(env.spec, [64, 64], torch.tanh) if kind == "fnn" else vs.GRUPolicy(env.spec, 64, 1)


@pytest.mark.parametrize("kind", ["fnn", "gru"])
@pytest.mark.parametrize("P,R", [(3, 10), (3, 64), (40, 10), (40, 64)])
def test_sample_returns_against_sample(vs, kind, P, R):
    env = vs.QQubeSwingUpSim(dt=0.004, max_steps=100)
    policy = make_policy(vs, kind, env)
    before = policy.param_values.detach().clone()
    torch.manual_seed(1)
    params = torch.stack([before + 0.3 * torch.randn_like(before) for _ in range(P)])
    np.random.seed(R)
    inits = [env.init_space.sample_uniform() for _ in range(R)]
    batch_lanes = 64 * ((P + 1) // 2)  # stride 64: two batches of whole sets
    gamma = 0.97

    def sampler():
        return vs.ParameterExploringSampler(env, policy, R, 1, seed=2, batch_lanes=batch_lanes)

    smp = sampler()
    res = smp.sample(params, init_states=inits)
    smp.close()
    smp = sampler()
    got = smp.sample_returns(params, init_states=inits, gamma=gamma)
    smp.close()
    smp = sampler()
    got1 = smp.sample_returns(params, init_states=inits)  # gamma = 1
    smp.close()
    assert len(got.packed) == 2 and len(got) == P
    assert got.returns.is_cuda and got.returns.dtype == torch.float32 and got.returns.shape == (P, R)
    assert got.lengths.is_cuda and got.lengths.dtype == torch.int64 and got.mean_returns.is_cuda and got.mean_returns.shape == (P,)
    assert torch.equal(got.parameters.cpu(), params) and torch.equal(res.parameters, params)
    lengths = np.array([[len(ro) for ro in s.rollouts] for s in res])
    assert np.array_equal(got.lengths.cpu().numpy(), lengths) and np.array_equal(got1.lengths.cpu().numpy(), lengths)
    worst = 0.0
    for g, out in ((gamma, got), (1.0, got1)):
        ret = out.returns.cpu().numpy().astype(np.float64)
        for s in range(P):
            ref, bound = rollout_bound(res[s].rollouts, g)
            worst = max(worst, worst_ratio(np.abs(ret[s] - ref), bound))
            if g == 1.0:
                # the fp32 mean of R returns, summed in any order: (R + 2) u mean |return| on top of the returns' own bound
                slack = bound.mean() + (R + 2) * U * np.abs(ref).mean()
                assert abs(float(out.mean_returns[s]) - res.mean_returns[s]) <= slack
    print(f"\n{kind} P = {P} R = {R}: worst ratio to the bound {worst:.4f}")
    assert torch.equal(policy.param_values.detach(), before)


def test_sample_returns_needs_a_fused_policy(vs):
    env = vs.QQubeSwingUpSim(dt=0.004, max_steps=20)
    policy = make_policy(vs, "fnn", env)
    smp = vs.ParameterExploringSampler(env, policy, 4, 1, seed=2, fuse_policy=False)
    with pytest.raises(vs.ValueErr, match="population"):
        smp.sample_returns(policy.param_values.detach()[None])
    smp.close()
