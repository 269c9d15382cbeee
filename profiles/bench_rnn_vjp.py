"""Cost of the closed-loop reverse-mode sweep with a recurrent policy in the loop (vs_rollout_vjp_rnn, k_rollout_vjp_rnn) on QQube
swing-up, cartpole swing-up and the ball balancer: 16 384 lanes x 400 steps recorded with a GRUPolicy and an LSTMPolicy of one layer of
64 units in the loop, random cotangents on rewards, observations, actions, the last state and the last hidden state.

Per family ROUNDS rounds, each timing one after the other (interleaved repeats, so that clock and temperature drift hit every variant
alike); all four are device times between events, 1 - 3 on the handle's stream, 4 between torch events on torch's current stream:
  1. the closed-loop sweep: one vs_rollout_vjp_rnn over the 400 recorded rows (d_hid and d_hid0 written);
  2. the open-loop sweep of the same build over the same records: one vs_rollout_vjp (the policy's Jacobian dropped);
  3. the recording forward launch of the same rollouts: reset + one vs_step_policy of 400 steps in record mode 2;
  4. the parameter gradient: one batched single-step torch pass of the policy over the [N T] recorded observations and hidden states on
     the device, torch.autograd.grad(policy(obs, hid), parameters, grad_outputs=(abar, d_hid)), 2^20 rows at a time.
The table gives the median (min .. max) of each and the ratio of 1 to 2.  Prints it (and writes it to the path given as argv[1]).

    python profiles/bench_rnn_vjp.py [out.txt]
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import simurlacra_amd as vs  # noqa: E402
from simurlacra_amd import _lib as L  # noqa: E402

N, T, ROUNDS, ROWS = 16384, 400, 5, 1 << 20
FAMILIES = {"qq-su": (0.004, "QQubeSwingUpSim"), "qcp-su": (0.002, "QCartPoleSwingUpSim"), "qbb": (0.01, "QBallBalancerSim")}
POLICIES = (("gru", "GRUPolicy"), ("lstm", "LSTMPolicy"))


def spread(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2], xs[0], xs[-1]


def main():
    lines = [f"vs_rollout_vjp_rnn against vs_rollout_vjp over the same records, the recording forward launch and the torch parameter-"
             f"gradient pass: {N} lanes x {T} steps, one recurrent layer of 64 units, output layer scaled by 0.2; library version "
             f"{L.load().vs_version()}, {ROUNDS} interleaved rounds: ms, median (min .. max); device time between events (the torch pass: torch "
             f"events on its stream)"]
    for name, cell, pcls, dt, cls in [(name, cell, pcls, dt, cls) for name, (dt, cls) in FAMILIES.items() for cell, pcls in POLICIES]:
        torch.manual_seed(0)
        d = vs.env_dims(name)
        S, A, O, H = (d[k] for k in "SAOH")
        env = getattr(vs, cls)(dt=dt, max_steps=4000)
        policy = getattr(vs, pcls)(env.spec, hidden_size=64, num_recurrent_layers=1)
        with torch.no_grad():
            policy.output_layer.weight.mul_(0.2)
        spec = vs.rnn_kernel_spec(policy)
        spec.pop("noise_std")
        Hs = policy.hidden_size
        tag = f"{name} {cell}-64"
        policy.to("cuda")
        e = vs.VecSimEnv(name, N, dt=dt, max_steps=4000)
        e.set_auto_reset(False)
        e.reset(seed=1)
        init = e.get(L.VS_STATE)
        e.set_record_mode(2)
        e.set_traj_capacity(T)
        e.set_policy_rnn(**spec)
        e.set_policy_hidden_record(Hs)
        g_rew = torch.randn(T, e.ld, device="cuda")
        g_obs = torch.randn(T + 1, O, e.ld, device="cuda")
        g_act = torch.randn(T, A, e.ld, device="cuda")
        g_last = torch.randn(S + H, e.ld, device="cuda")
        g_hid = torch.randn(Hs, e.ld, device="cuda")
        kept = {}

        def forward():
            e.reset(init_state=init)
            e.policy_hidden().zero_()  # every rollout starts from init_hidden()
            e.timer_start()
            e.step_policy(T, record=True)
            return e.timer_stop()

        def closed():
            e.timer_start()
            out = e.rollout_vjp_rnn(T, g_rew=g_rew, g_obs=g_obs, g_act=g_act, g_state_last=g_last, g_hid_last=g_hid)
            kept["abar"], kept["d_hid"] = out[0], out[2]
            return e.timer_stop()

        def opened():
            e.timer_start()
            e.rollout_vjp(T, g_rew=g_rew, g_obs=g_obs, g_state_last=g_last)
            return e.timer_stop()

        def param_grad():
            seen = e.traj_tensors(T, N)["obs"].reshape(T * N, O)
            hid = e.hidden_record_tensor()[:T, :, :N].movedim(1, 2).reshape(T * N, Hs)
            abar = kept["abar"][..., :N].movedim(1, 2).reshape(T * N, A)
            d_hid = kept["d_hid"][..., :N].movedim(1, 2).reshape(T * N, Hs)
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            start.record()
            for r0 in range(0, T * N, ROWS):  # as DifferentiableRecurrentRollout._param_grads: 2^20 rows at a time
                rows = slice(r0, min(r0 + ROWS, T * N))
                with torch.enable_grad():
                    torch.autograd.grad(policy(seen[rows], hid[rows]), list(policy.parameters()), grad_outputs=(abar[rows], d_hid[rows]))
            stop.record()
            stop.synchronize()
            return start.elapsed_time(stop)

        variants = [("closed-loop sweep (vs_rollout_vjp_rnn)", closed), ("open-loop sweep (vs_rollout_vjp)", opened),
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
