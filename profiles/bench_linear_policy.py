"""Throughput of a linear policy on a feature stack in the loop (vs_set_policy_linear, k_rollout_lin) on QQube swing-up.

  * kernel: vs_step_policy against (a) vs_step_random pinned to the plain k_rollout, on the SAME handle, launch length and record
    mode (LAUNCHES launches of K recorded steps, record mode 1, auto-reset on) -- the uniform policy is the yardstick of a kernel
    in which nothing is matrix-shaped.  Device time between HIP events; the two kernels alternate, ROUNDS rounds, median and
    spread (min .. max) reported.
  * sampler: one ParallelRolloutSampler.sample_packed() call, the fused path against (b) the same LinearPolicy as a torch module
    in the loop (fuse_policy=False), alternating, wall time.
  * population: ParameterExploringSampler.sample_returns() against the host loop over the sets (one fused sample_packed() per
    set with that set's vector).
Prints a table (and writes it to the path given as argv[1]).

    python profiles/bench_linear_policy.py [out.txt]
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import simurlacra_amd as vs  # noqa: E402
from simurlacra_amd import features as F  # noqa: E402
from simurlacra_amd.policies import LinearPolicy, linear_kernel_spec  # noqa: E402

K, LAUNCHES, ROUNDS = 64, 10, 5
SIZES = (16384, 65536)
STACKS = {"identity+sin+cos": (F.identity_feat, F.sin_feat, F.cos_feat), "identity": (F.identity_feat,)}
POP_SETS, POP_ROLLOUTS, T_SAMPLE = 64, 256, 64


def spread(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2], xs[0], xs[-1]


def make_policy(env, stack, seed=0):
    pol = LinearPolicy(env.spec, F.FeatureStack(*stack))
    pol.param_values = 2.0 * torch.randn(pol.param_values.shape, generator=torch.Generator().manual_seed(seed))
    return pol


def kernel_rates(pol, n):
    """env-steps/s (median, min, max) of vs_step_policy and of vs_step_random / k_rollout on one handle, alternating"""
    e = vs.VecSimEnv("qq-su", n, dt=0.004, max_steps=4000)
    e.set_auto_reset(True, seed=1)
    e.reset(seed=2)
    e.set_policy_linear(**linear_kernel_spec(pol))
    e.set_rollout_variant("k_rollout")
    e.set_record_mode(1)
    e.set_traj_capacity(K)

    def lin():
        e.step_policy(K, record=True)

    def uni():
        e.step_random(K, seed=7, record=True)
    rates = {"lin": [], "uni": []}
    for name, fn in (("lin", lin), ("uni", uni)):  # warm-up
        fn()
    e.sync()
    for _ in range(ROUNDS):
        for name, fn in (("lin", lin), ("uni", uni)):
            e.timer_start()
            for _ in range(LAUNCHES):
                fn()
            rates[name].append(n * K * LAUNCHES / (e.timer_stop() * 1e-3))
    e.close()
    return spread(rates["lin"]), spread(rates["uni"])


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def sampler_rates(stack, n):
    env = vs.QQubeSwingUpSim(dt=0.004, max_steps=T_SAMPLE)
    pol = make_policy(env, stack)
    smps = {"fused": vs.ParallelRolloutSampler(env, pol, 1, min_rollouts=n, seed=3, full_records=False),
            "torch": vs.ParallelRolloutSampler(env, pol, 1, min_rollouts=n, seed=3, full_records=False, fuse_policy=False)}
    rates = {k: [] for k in smps}
    for s in smps.values():
        s.sample_packed()  # warm-up (handles, allocator)
    for _ in range(3):
        for k, s in smps.items():
            dt, (pk,) = timed(s.sample_packed)
            rates[k].append(pk.total / dt)
    for s in smps.values():
        s.close()
    pol.to("cpu")
    return spread(rates["fused"]), spread(rates["torch"])


def population_rates(stack):
    env = vs.QQubeSwingUpSim(dt=0.004, max_steps=T_SAMPLE)
    pol = make_policy(env, stack)
    p0 = pol.param_values.detach().clone()
    params = torch.stack([p0 + 0.3 * torch.randn_like(p0) for _ in range(POP_SETS)])
    np.random.seed(0)
    inits = [env.init_space.sample_uniform() for _ in range(POP_ROLLOUTS)]
    pes = vs.ParameterExploringSampler(env, pol, POP_ROLLOUTS, 1, seed=3, full_records=False)
    prs = vs.ParallelRolloutSampler(env, pol, 1, min_rollouts=POP_ROLLOUTS, seed=3, full_records=False)

    def fused():
        return int(pes.sample_returns(params, init_states=inits).lengths.sum())

    def loop():
        total = 0
        for p in params:
            pol.param_values = p
            (pk,) = prs.sample_packed(init_states=inits)
            total += pk.total
        return total
    fused(), loop()  # warm-up
    rates = {"fused": [], "loop": []}
    for _ in range(3):
        for k, fn in (("fused", fused), ("loop", loop)):
            dt, steps = timed(fn)
            rates[k].append(steps / dt)
    pol.param_values = p0
    pes.close()
    prs.close()
    return spread(rates["fused"]), spread(rates["loop"])


def fmt(s):
    return f"{s[0]:10.3e} ({s[1]:.2e} .. {s[2]:.2e})"


def main():
    env = vs.QQubeSwingUpSim(dt=0.004, max_steps=T_SAMPLE)
    out = [f"linear policy on a feature stack in the loop, QQube swing-up; env-steps/s, median (min .. max)",
           f"kernel: {ROUNDS} alternating rounds of {LAUNCHES} launches of {K} recorded steps (record mode 1, auto-reset on), device time",
           f"{'stack':18} {'envs':>6}  {'k_rollout_lin':34} {'(a) k_rollout, uniform policy':34} {'lin / (a)':>9}"]
    for name, stack in STACKS.items():
        pol = make_policy(env, stack)
        for n in SIZES:
            lin, uni = kernel_rates(pol, n)
            out.append(f"{name:18} {n:6d}  {fmt(lin):34} {fmt(uni):34} {lin[0] / uni[0]:9.3f}")
            print(out[-1], flush=True)
    out.append(f"sampler: sample_packed() of n rollouts of <= {T_SAMPLE} steps (full_records=False), 3 alternating calls, wall time")
    out.append(f"{'stack':18} {'envs':>6}  {'fused':34} {'(b) torch in the loop':34} {'fused / (b)':>11}")
    for name, stack in STACKS.items():
        for n in SIZES:
            fu, to = sampler_rates(stack, n)
            out.append(f"{name:18} {n:6d}  {fmt(fu):34} {fmt(to):34} {fu[0] / to[0]:11.1f}")
            print(out[-1], flush=True)
    out.append(f"population: {POP_SETS} sets x {POP_ROLLOUTS} rollouts of <= {T_SAMPLE} steps, ParameterExploringSampler.sample_returns() against "
               f"the host loop over the sets (one fused sample_packed() per set), 3 alternating calls, wall time")
    out.append(f"{'stack':18} {'sample_returns':34} {'host loop over sets':34} {'ratio':>6}")
    for name, stack in STACKS.items():
        fu, lo = population_rates(stack)
        out.append(f"{name:18} {fmt(fu):34} {fmt(lo):34} {fu[0] / lo[0]:6.1f}")
        print(out[-1], flush=True)
    text = "\n".join(out)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
