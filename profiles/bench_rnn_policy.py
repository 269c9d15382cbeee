"""Throughput of a recurrent policy in the loop on 65 536 QQube envs: the fused kernel (vs_step_policy with vs_set_policy_rnn,
record mode 1, hidden-state record off and on) against the sampler's torch-in-the-loop paths (eager and graph_policy=True) on
the same sample_packed() call.  GRU-64 and LSTM-64, one layer.  Prints a table (and writes it to the path given as argv[1]).

    python profiles/bench_rnn_policy.py [out.txt]
"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import simurlacra_amd as vs  # noqa: E402
from simurlacra_amd.policies import rnn_kernel_spec  # noqa: E402

N, K, LAUNCHES = 65536, 64, 10
FP32_PEAK = 157.3e12  # MI355X fp32 vector peak (FLOP/s), AMD's published figure


def fmas_per_step(cell, hidden, n_obs, n_act):
    g = {"gru": 3, "lstm": 4}[cell]
    hp = (hidden + 3) // 4 * 4
    return g * hidden * (8 + hp) + n_act * hidden  # the kernel's padded input row (8) and hidden rows


def kernel_rate(pol, cell, hrec):
    e = vs.VecSimEnv("qq-su", N, dt=0.004, max_steps=4000)
    e.set_auto_reset(True, seed=1)
    e.reset(seed=2)
    e.set_policy_rnn(**rnn_kernel_spec(pol))
    e.set_record_mode(1)
    e.set_traj_capacity(K)
    e.set_policy_hidden_record(pol.hidden_size if hrec else 0)
    e.step_policy(K, record=True)  # warm-up
    e.sync()
    t0 = time.perf_counter()
    for _ in range(LAUNCHES):
        e.step_policy(K, record=True)
    e.sync()
    dt = time.perf_counter() - t0
    e.close()
    return N * K * LAUNCHES / dt


def sampler_rate(pol, **kw):
    env = vs.QQubeSwingUpSim(dt=0.004, max_steps=K)
    smp = vs.ParallelRolloutSampler(env, pol, 1, min_rollouts=N, seed=3, full_records=False, **kw)
    smp.sample_packed()  # warm-up (handles, graph capture, allocator)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    (pk,) = smp.sample_packed()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    steps = pk.total
    smp.close()
    return steps / dt


def main():
    out = []
    env = vs.QQubeSwingUpSim(dt=0.004, max_steps=K)
    O, A = env.obs_space.flat_dim, env.act_space.flat_dim
    out.append(f"recurrent policy in the loop, {N} QQube envs, 1 layer of 64 units; fused kernel: {LAUNCHES} launches of {K} steps, "
               f"record mode 1, auto-reset on; sampler: one sample_packed() call of {N} rollouts of <= {K} steps")
    out.append(f"{'policy':8} {'path':34} {'env-steps/s':>12} {'GFLOP/s':>9} {'of fp32 peak':>12}")
    for cell, cls in (("gru", vs.GRUPolicy), ("lstm", vs.LSTMPolicy)):
        torch.manual_seed(0)
        pol = cls(env.spec, 64, 1)
        fl = 2 * fmas_per_step(cell, 64, O, A)
        rows = [("fused kernel, hidden record off", kernel_rate(pol, cell, False)),
                ("fused kernel, hidden record on", kernel_rate(pol, cell, True)),
                ("sampler, fused", sampler_rate(pol)),
                ("sampler, torch eager", sampler_rate(pol, fuse_policy=False)),
                ("sampler, torch graph_policy=True", sampler_rate(pol, fuse_policy=False, graph_policy=True))]
        for what, r in rows:
            out.append(f"{cell.upper() + '-64':8} {what:34} {r:12.3e} {r * fl / 1e9:9.0f} {r * fl / FP32_PEAK:12.3f}")
        pol.to("cpu")
    text = "\n".join(out)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
