"""Throughput of vs_returns_scan (PackedRollouts.discounted_returns / rewards_to_go / gae, ParameterExploringSampler.sample_returns).

  (a) the kernel on 65 536 rollouts with geometric lengths (mean ~545, capped at 4 000), reward read from full QQube record rows
      (F = 13), lean record rows (F = 8) and a dense vector; HIP events around ITERS calls after a warm-up.  Against
        * a torch baseline in this script: pad to [n, T_max], then T_max steps of y = r[:, t] + gamma * y (the padding included in
          its time, as a consumer pays it), and
        * the algorithmic bytes: every 128-byte line of the reward column that a row touches, once, plus 4 B per row written.
  (b) ParameterExploringSampler.sample_returns() against sample() followed by mean_returns, wall time of one call after a warm-up,
      at the P x R points of profiles/param_exploration_throughput.txt (QQube swing-up, rollouts of <= 100 steps).
Three alternating runs of every pair; the table gives the median and the spread (max / min) over the three.

    python profiles/bench_returns.py [out.txt]
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import simurlacra_amd as vs  # noqa: E402
from simurlacra_amd import _lib as L  # noqa: E402
from simurlacra_amd.sampling import packed_row_layout, returns_scan  # noqa: E402

N, ITERS, RUNS, GAMMA, T_SAMPLE = 65536, 20, 3, 0.99, 100
SETS, ROLLOUTS = (64, 256, 1024), (10, 64, 256)


def event_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def spread(xs):
    return f"{np.median(xs):9.3f} (x{max(xs) / min(xs):.2f})"


def torch_loop(rew, lengths_d, base_d, t_max):
    """the ragged recurrence in torch: a padded [n, T_max] copy and one small kernel pair per time step"""
    n = lengths_d.shape[0]
    t = torch.arange(t_max, device=rew.device)
    mask = t[None, :] < lengths_d[:, None]
    pad = torch.zeros(n, t_max, device=rew.device)
    pad[mask] = rew[(base_d[:, None] + t[None, :])[mask]]
    y = torch.zeros(n, device=rew.device)
    for k in range(t_max - 1, -1, -1):
        y = pad[:, k] + GAMMA * y
    return y


def kernel_table(out):
    rng = np.random.default_rng(0)
    lengths = np.minimum(rng.geometric(1.0 / 545.0, N), 4000).astype(np.int64)
    starts, base, _, rows = packed_row_layout(lengths)
    len_d, sta_d, base_d = (torch.from_numpy(x).cuda() for x in (lengths, starts, base))
    out.append(f"(a) vs_returns_scan, {N} rollouts, {int(lengths.sum())} steps (mean {lengths.mean():.0f}, max {lengths.max()}), RETURN "
               f"mode with out_first, {ITERS} calls per run, {RUNS} alternating runs: median (max / min)")
    out.append(f"{'reward column':22} {'kernel ms':>18} {'alg. MB':>9} {'GB/s':>8} {'torch loop ms':>18} {'loop / kernel':>13} {'max |diff|':>10}")
    for name, F in (("record rows, F = 13", 13), ("record rows, F = 8", 8), ("dense", 1)):
        rec = torch.randn(rows, F, device="cuda")
        rew = rec[:, F - 1]
        ker, loop = [], []
        for _ in range(RUNS):
            ker.append(event_ms(lambda: returns_scan(len_d, sta_d, rew, rows, L.VS_RETURNS_RETURN, GAMMA, want_first=True), ITERS))
            loop.append(event_ms(lambda: torch_loop(rew, len_d, base_d, int(lengths.max())), 1))
        first = returns_scan(len_d, sta_d, rew, rows, L.VS_RETURNS_RETURN, GAMMA, want_first=True)[1]
        ref = torch_loop(rew, len_d, base_d, int(lengths.max()))
        diff = float((first - ref).abs().max())  # (both fp32: the two orders of summation)
        # a 128-byte line holds 32 / F reward entries (F <= 32: every line of the rows is touched when F * 4 <= 128)
        read = rows * min(F * 4, 128) if F > 1 else rows * 4
        mb = (read + rows * 4) / 1e6
        out.append(f"{name:22} {spread(ker):>18} {mb:9.1f} {mb / 1e3 / (np.median(ker) * 1e-3):8.0f} {spread(loop):>18} "
                   f"{np.median(loop) / np.median(ker):13.0f} {diff:10.1e}")
        print(out[-1], flush=True)
        del rec, rew


def returns_and_means(smp, params):
    res = smp.sample_returns(params)
    res.mean_returns.cpu()  # (the [P] means on the host, as sample().mean_returns has them)
    return res


def sampler_table(out):
    env = vs.QQubeSwingUpSim(dt=0.004, max_steps=T_SAMPLE)
    out.append("")
    out.append(f"(b) ParameterExploringSampler on QQube swing-up, rollouts of <= {T_SAMPLE} steps, full_records=False: one call of "
               f"sample_returns() against sample() + mean_returns, wall ms, {RUNS} alternating runs: median (max / min); env-steps/s of "
               "real lanes from the medians")
    out.append(f"{'policy':10} {'P':>5} {'R':>4} {'sample() ms':>18} {'sample_returns() ms':>20} {'ratio':>6} {'steps/s sample':>15} "
               f"{'steps/s returns':>15}")
    for name in ("FNN-64x64", "GRU-64"):
        torch.manual_seed(0)
        pol = vs.FNNPolicy(env.spec, [64, 64], torch.tanh) if name.startswith("FNN") else vs.GRUPolicy(env.spec, 64, 1)
        p0 = pol.param_values.detach()
        for P in SETS:
            params = torch.stack([p0 + 0.1 * torch.randn_like(p0) for _ in range(P)])
            for R in ROLLOUTS:
                smp = vs.ParameterExploringSampler(env, pol, R, 1, seed=3, full_records=False)
                smp.sample(params).mean_returns  # warm-up (handles, allocator)
                smp.sample_returns(params).mean_returns.cpu()
                host, dev, steps = [], [], 0
                for _ in range(RUNS):
                    dt, res = wall(lambda: smp.sample(params).mean_returns)
                    host.append(dt * 1e3)
                    dt, res = wall(lambda: returns_and_means(smp, params))
                    dev.append(dt * 1e3)
                    steps = int(res.lengths.sum())
                smp.close()
                out.append(f"{name:10} {P:5d} {R:4d} {spread(host):>18} {spread(dev):>20} {np.median(host) / np.median(dev):6.1f} "
                           f"{steps / np.median(host) * 1e3:15.3e} {steps / np.median(dev) * 1e3:15.3e}")
                print(out[-1], flush=True)


def main():
    out = []
    kernel_table(out)
    sampler_table(out)
    text = "\n".join(out)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
