"""Throughput of a policy population (ParameterExploringSampler / vs_set_policy_population) on QQube swing-up: FNN 64 x 64 tanh
and GRU-64, P parameter sets x R rollouts each.  Per row:
  * kernel: vs_set_policy_population + vs_step_policy (LAUNCHES launches of K recorded steps, record mode 1, auto-reset off),
    env-steps/s of the real lanes (P x R), and the single-policy kernel on the same handle (same lanes and shape, no
    population) with the ratio population / single counted over all lanes;
  * sampler: one ParameterExploringSampler.sample() call (rollouts of <= T_SAMPLE steps), recorded env-steps/s;
  * host loop (P = 64 and 256): one ParallelRolloutSampler.sample() per set with that set's vector, the same rollouts;
  * lane utilisation: real / padded lanes.
Prints a table (and writes it to the path given as argv[1]).

    python profiles/bench_param_exploration.py [out.txt]
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import simurlacra_amd as vs  # noqa: E402
from simurlacra_amd import parameter_exploration as pe  # noqa: E402
from simurlacra_amd.policies import fnn_kernel_spec, rnn_kernel_spec  # noqa: E402

K, LAUNCHES, T_SAMPLE = 64, 4, 100
SETS, ROLLOUTS, LOOP_SETS = (64, 256, 1024), (10, 64, 256), (64, 256)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def kernel_rates(pol, params, R):
    P = params.shape[0]
    stride, _ = pe.population_lane_layout(P, R, 1 << 30)
    n = P * stride
    e = vs.VecSimEnv("qq-su", n, dt=0.004, max_steps=4000)
    e.set_record_mode(1)
    e.set_traj_capacity(K)
    fnn = fnn_kernel_spec(pol)
    rates = []
    for population in (True, False):
        if fnn is not None:
            e.set_policy_fnn(**fnn)
        else:
            e.set_policy_rnn(**rnn_kernel_spec(pol))
        if population:
            e.set_policy_population(params.cuda(), pe.population_lane_set(P, stride))
        e.reset(seed=2)
        e.step_policy(K, record=True)  # warm-up
        e.reset(seed=2)

        def go():
            for _ in range(LAUNCHES):
                e.step_policy(K, record=True)
        rates.append(n * K * LAUNCHES / timed(go))
    e.close()
    pop_all, single = rates
    return pop_all * (P * R) / n, pop_all / single, (P * R) / n


def sampler_rate(pol, params, R):
    env = vs.QQubeSwingUpSim(dt=0.004, max_steps=T_SAMPLE)
    smp = vs.ParameterExploringSampler(env, pol, R, 1, seed=3, full_records=False)
    smp.sample(params)  # warm-up (handles, allocator)
    out = []
    dt = timed(lambda: out.append(smp.sample(params)))
    smp.close()
    return sum(len(ro) for s in out[0] for ro in s.rollouts) / dt


def loop_rate(pol, params, R):
    env = vs.QQubeSwingUpSim(dt=0.004, max_steps=T_SAMPLE)
    np.random.seed(0)
    inits = [env.init_space.sample_uniform() for _ in range(R)]
    keep = pol.param_values.detach().clone()
    smp = vs.ParallelRolloutSampler(env, pol, 1, min_rollouts=R, seed=3, full_records=False)
    smp.sample(init_states=inits)  # warm-up
    steps = []

    def go():
        for p in params:
            pol.param_values = p
            steps.append(sum(len(ro) for ro in smp.sample(init_states=inits)))
    dt = timed(go)
    pol.param_values = keep
    smp.close()
    return sum(steps) / dt


def main():
    env = vs.QQubeSwingUpSim(dt=0.004, max_steps=T_SAMPLE)
    out = [f"policy population on QQube swing-up: kernel = {LAUNCHES} launches of {K} recorded steps (record mode 1, auto-reset off), "
           f"sampler / host loop = one call of rollouts of <= {T_SAMPLE} steps (full_records=False); env-steps/s of real lanes",
           f"{'policy':8} {'P':>5} {'R':>4} {'lanes':>7} {'util':>5} {'kernel':>10} {'pop/single':>10} {'sampler':>10} "
           f"{'host loop':>10} {'smp/loop':>8}"]
    for name in ("FNN-64x64", "GRU-64"):
        torch.manual_seed(0)
        pol = vs.FNNPolicy(env.spec, [64, 64], torch.tanh) if name.startswith("FNN") else vs.GRUPolicy(env.spec, 64, 1)
        p0 = pol.param_values.detach()
        for P in SETS:
            params = torch.stack([p0 + 0.1 * torch.randn_like(p0) for _ in range(P)])
            for R in ROLLOUTS:
                stride, _ = pe.population_lane_layout(P, R, 1 << 30)
                kr, ratio, util = kernel_rates(pol, params, R)
                sr = sampler_rate(pol, params, R)
                lr = loop_rate(pol, params, R) if P in LOOP_SETS else float("nan")
                out.append(f"{name:8} {P:5d} {R:4d} {P * stride:7d} {util:5.2f} {kr:10.3e} {ratio:10.3f} {sr:10.3e} {lr:10.3e} "
                           f"{sr / lr:8.1f}")
                print(out[-1], flush=True)
    text = "\n".join(out)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
