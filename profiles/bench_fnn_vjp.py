"""Cost of the closed-loop reverse-mode sweep with a feed-forward network in the loop (vs_rollout_vjp_fnn, k_rollout_vjp_fnn) on QQube
swing-up, cartpole swing-up and the ball balancer: 16 384 lanes x 400 steps recorded with an FNNPolicy of [64] and of [64, 64] tanh units
(no featurisation) in the loop, random cotangents on rewards, observations, actions and the last state.

Per family ROUNDS rounds, each timing one after the other (interleaved repeats, so that clock and temperature drift hit every variant
alike); 1 - 3 are device times between HIP events on the handle's stream, 4 is wall time with a device synchronisation:
  1. the closed-loop sweep: one vs_rollout_vjp_fnn over the 400 recorded rows;
  2. the open-loop sweep of the same build over the same records: one vs_rollout_vjp (the policy's Jacobian dropped);
  3. the recording forward launch of the same rollouts: reset + one vs_step_policy of 400 steps in record mode 2;
  4. the parameter gradient: one batched torch pass of the network over the [N T] recorded observations on the device,
     torch.autograd.grad(policy(obs), parameters, grad_outputs=abar).
The table gives the median (min .. max) of each and the ratio of 1 to 2.  Prints it (and writes it to the path given as argv[1]).

    python profiles/bench_fnn_vjp.py [out.txt]
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import simurlacra_amd as vs  # noqa: E402
from simurlacra_amd import _lib as L  # noqa: E402

N, T, ROUNDS = 16384, 400, 5
FAMILIES = {"qq-su": (0.004, "QQubeSwingUpSim"), "qcp-su": (0.002, "QCartPoleSwingUpSim"), "qbb": (0.01, "QBallBalancerSim")}
NETWORKS = ([64], [64, 64])


def spread(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2], xs[0], xs[-1]


def main():
    lines = [f"vs_rollout_vjp_fnn against vs_rollout_vjp over the same records, the recording forward launch and the torch parameter-"
             f"gradient pass: {N} lanes x {T} steps, FNNPolicy of tanh units, output layer scaled by 0.2; library version "
             f"{L.load().vs_version()}, {ROUNDS} interleaved rounds: ms, median (min .. max); sweeps and forward launch between HIP events, "
             f"the torch pass in wall time"]
    for name, hidden, dt, cls in [(name, hidden, dt, cls) for name, (dt, cls) in FAMILIES.items() for hidden in NETWORKS]:
        torch.manual_seed(0)
        d = vs.env_dims(name)
        S, A, O, H = (d[k] for k in "SAOH")
        env = getattr(vs, cls)(dt=dt, max_steps=4000)
        policy = vs.FNNPolicy(env.spec, hidden_sizes=hidden, hidden_nonlin=torch.tanh, featurize=False)
        with torch.no_grad():
            policy.net.output_layer.weight.mul_(0.2)
        spec = vs.fnn_kernel_spec(policy)
        spec.pop("noise_std")
        tag = f"{name} {'x'.join(str(h) for h in hidden)}"
        policy.to("cuda")
        e = vs.VecSimEnv(name, N, dt=dt, max_steps=4000)
        e.set_auto_reset(False)
        e.reset(seed=1)
        init = e.get(L.VS_STATE)
        e.set_record_mode(2)
        e.set_traj_capacity(T)
        e.set_policy_fnn(**spec)
        g_rew = torch.randn(T, e.ld, device="cuda")
        g_obs = torch.randn(T + 1, O, e.ld, device="cuda")
        g_act = torch.randn(T, A, e.ld, device="cuda")
        g_last = torch.randn(S + H, e.ld, device="cuda")
        kept = {}

        def forward():
            e.reset(init_state=init)
            e.timer_start()
            e.step_policy(T, record=True)
            return e.timer_stop()

        def closed():
            e.timer_start()
            kept["abar"] = e.rollout_vjp_fnn(T, g_rew=g_rew, g_obs=g_obs, g_act=g_act, g_state_last=g_last)[0]
            return e.timer_stop()

        def opened():
            e.timer_start()
            e.rollout_vjp(T, g_rew=g_rew, g_obs=g_obs, g_state_last=g_last)
            return e.timer_stop()

        def param_grad():
            seen = e.traj_tensors(T, N)["obs"].reshape(T * N, O)
            abar = kept["abar"][..., :N].movedim(1, 2).reshape(T * N, A)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with torch.enable_grad():
                torch.autograd.grad(policy(seen), list(policy.parameters()), grad_outputs=abar)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        variants = [("closed-loop sweep (vs_rollout_vjp_fnn)", closed), ("open-loop sweep (vs_rollout_vjp)", opened),
                    ("recording forward launch", forward), ("torch parameter-gradient pass", param_grad)]
        forward()
        for _, f in variants:  # warm-up (loads the kernels)
            f()
        ms = {label: [] for label, _ in variants}
        for _ in range(ROUNDS):
            for label, f in variants:
                ms[label].append(f())
        mean_len = float(e.rollout_lengths(N, T)[0].float().mean())
        for label, _ in variants:
            m, lo, hi = spread(ms[label])
            lines.append(f"{tag:13s} {label:42s} {m:10.3f} ({lo:.3f} .. {hi:.3f})")
        ratio = spread(ms[variants[0][0]])[0] / spread(ms[variants[1][0]])[0]
        lines.append(f"{tag:13s} closed / open {ratio:.2f}; mean rollout length {mean_len:.1f} of {T} steps, errors {e.error_count()}")
        e.close()
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
