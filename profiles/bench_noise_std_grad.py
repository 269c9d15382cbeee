"""Cost of the gradient of the exploration noise's std (vs_noise_std_grad: k_noise_std_grad + k_fnn_param_reduce) against the torch route
it replaces, on the same records and adjoints: QQube swing-up, cartpole swing-up and the ball balancer, 16 384 lanes x 400 steps
recorded with a LinearPolicy (identity, sin, const, MultFeat((0, 1))) and noise_std = 0.05 in the loop, random cotangents.

Per family ROUNDS rounds, each timing one after the other (interleaved repeats):
  1. the closed-loop sweep: one vs_rollout_vjp_policy over the 400 recorded rows (HIP events on the handle's stream);
  2. the kernel pass: one vs_noise_std_grad on the sweep's d_act (HIP events on the handle's stream);
  3. the torch route in device time between torch events and in wall time: lanes_first of d_act, the gather of the recorded
     observations and actions, the policy's mean over the [N T] rows, (act - mean) / sigma, times the adjoints, masked by the
     lengths and summed.
The table gives the median (min .. max) of each in ms.  Prints it (and writes it to the path given as argv[1]).

    python profiles/bench_noise_std_grad.py [out.txt]
"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import simurlacra_amd as vs  # noqa: E402
from simurlacra_amd import _lib as L  # noqa: E402

N, T, ROUNDS, STD, SEED = 16384, 400, 5, 0.05, 77
FAMILIES = {"qq-su": (0.004, "QQubeSwingUpSim"), "qcp-su": (0.002, "QCartPoleSwingUpSim"), "qbb": (0.01, "QBallBalancerSim")}


def spread(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2], xs[0], xs[-1]


def main():
    lines = [f"vs_noise_std_grad against the torch route on the same records and adjoints and the closed-loop sweep: {N} lanes x {T} "
             f"steps, LinearPolicy, noise_std {STD}; library version {L.load().vs_version()}, {ROUNDS} interleaved rounds: ms, median "
             f"(min .. max)"]
    for name, (dt, cls) in FAMILIES.items():
        torch.manual_seed(0)
        d = vs.env_dims(name)
        S, A, O, H = (d[k] for k in "SAOH")
        env = getattr(vs, cls)(dt=dt, max_steps=4000)
        policy = vs.LinearPolicy(env.spec, vs.FeatureStack(vs.identity_feat, vs.sin_feat, vs.const_feat, vs.MultFeat((0, 1))))
        with torch.no_grad():
            policy.net.weight.mul_(0.05)
        spec = vs.linear_kernel_spec(policy)
        spec["noise_std"] = [STD] * A
        policy.to("cuda")
        e = vs.VecSimEnv(name, N, dt=dt, max_steps=4000)
        e.set_auto_reset(False)
        e.reset(seed=1)
        init = e.get(L.VS_STATE)
        e.set_record_mode(2)
        e.set_traj_capacity(T)
        e.set_policy_linear(**spec)
        e.reset(init_state=init)
        e.step_policy(T, record=True, noise_seed=SEED)
        g_rew = torch.randn(T, e.ld, device="cuda")
        g_obs = torch.randn(T + 1, O, e.ld, device="cuda")
        g_act = torch.randn(T, A, e.ld, device="cuda")
        g_last = torch.randn(S + H, e.ld, device="cuda")
        kept = {}
        out = torch.empty(A, device="cuda")
        sigma = torch.full((A,), STD, device="cuda")

        def sweep():
            e.timer_start()
            kept["abar"] = e.rollout_vjp_policy(T, g_rew=g_rew, g_obs=g_obs, g_act=g_act, g_state_last=g_last)[0]
            return e.timer_stop()

        def kernel_pass():
            e.timer_start()
            e.noise_std_grad(T, SEED, kept["abar"], out=out)
            return e.timer_stop()

        def torch_route():
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ev0.record()
            with torch.no_grad():
                abar = vs.lanes_first(kept["abar"], N)                               # [N, T, A]
                tt = e.traj_tensors(T, N)
                mean = policy(tt["obs"].reshape(T * N, O)).reshape(T, N, A)
                eps = (tt["act"] - mean) / sigma
                inside = torch.arange(T, device="cuda")[:, None] < e.rollout_lengths(N, T)[0][None, :]
                g = torch.where(inside[:, :, None], abar.transpose(0, 1) * eps, torch.zeros((), device="cuda")).sum(dim=(0, 1))
            ev1.record()
            torch.cuda.synchronize()
            kept["torch"] = g
            return ev0.elapsed_time(ev1), (time.perf_counter() - t0) * 1e3

        labels = ["closed-loop sweep (vs_rollout_vjp_policy)", "kernel pass (vs_noise_std_grad)", "torch route, device time",
                  "torch route, wall time"]
        ms = {label: [] for label in labels}
        for r in range(ROUNDS + 1):  # round 0 warms up (loads the kernels, torch's allocator)
            row = [sweep(), kernel_pass(), *torch_route()]
            if r:
                for label, x in zip(labels, row):
                    ms[label].append(x)
        mean_len = float(e.rollout_lengths(N, T)[0].float().mean())
        agree = float((out - kept["torch"]).abs().max() / kept["torch"].abs().max())
        for label in labels:
            m, lo, hi = spread(ms[label])
            lines.append(f"{name:8s} {label:44s} {m:10.3f} ({lo:.3f} .. {hi:.3f})")
        ratio = spread(ms[labels[2]])[0] / spread(ms[labels[1]])[0]
        lines.append(f"{name:8s} torch device time / kernel {ratio:.2f}; max |kernel - torch| / max |torch| {agree:.1e}; mean rollout length "
                     f"{mean_len:.1f} of {T} steps, errors {e.error_count()}")
        e.close()
    text = "\n".join(lines)
    print(text, flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
