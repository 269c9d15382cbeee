"""Cost of the in-kernel parameter gradient of a recurrent policy (vs_rnn_param_grad: k_rnn_param_grad + k_fnn_param_reduce) against the
torch pass of the same build, on the shapes of bench_rnn_vjp.py: QQube swing-up, cartpole swing-up and the ball balancer, 16 384 lanes x
400 steps recorded with a GRUPolicy and an LSTMPolicy of one layer of 64 units in the loop, random cotangents.

Per family and cell ROUNDS rounds, each timing one after the other (interleaved repeats), device time in ms:
  1. the closed-loop sweep: one vs_rollout_vjp_rnn over the 400 recorded rows (HIP events on the handle's stream);
  2. the kernel parameter pass: one vs_rnn_param_grad on the sweep's d_act and d_hid (HIP events on the handle's stream);
  3. the torch parameter pass of the same records: DifferentiableRecurrentRollout's, torch.autograd.grad of the single-step policy
     over the [N T] rows, 2^20 rows at a time (torch events); the lanes-first copies that feed it are made before and not counted.
The table gives the median (min .. max) of each.  Prints it (and writes it to the path given as argv[1]).

    python profiles/bench_rnn_param_grad.py [out.txt]
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import simurlacra_amd as vs  # noqa: E402
from simurlacra_amd import _lib as L  # noqa: E402

N, T, ROUNDS, PASS_ROWS = 16384, 400, 5, 1 << 20
FAMILIES = {"qq-su": (0.004, "QQubeSwingUpSim"), "qcp-su": (0.002, "QCartPoleSwingUpSim"), "qbb": (0.01, "QBallBalancerSim")}
CELLS = {"gru": "GRUPolicy", "lstm": "LSTMPolicy"}


def spread(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2], xs[0], xs[-1]


def main():
    lines = [f"vs_rnn_param_grad against the torch parameter pass of the same records and the closed-loop sweep: {N} lanes x {T} steps, one "
             f"layer of 64 units, output layer scaled by 0.2; library version {L.load().vs_version()}, {ROUNDS} interleaved rounds: "
             f"device ms, median (min .. max)"]
    for name, cell, dt, cls in [(name, cell, dt, cls) for name, (dt, cls) in FAMILIES.items() for cell in CELLS]:
        torch.manual_seed(0)
        d = vs.env_dims(name)
        S, A, O, H = (d[k] for k in "SAOH")
        env = getattr(vs, cls)(dt=dt, max_steps=4000)
        policy = getattr(vs, CELLS[cell])(env.spec, 64, 1)
        with torch.no_grad():
            policy.output_layer.weight.mul_(0.2)
        spec = vs.rnn_kernel_spec(policy)
        spec.pop("noise_std")
        Hs = policy.hidden_size
        tag = f"{name} {cell}"
        policy.to("cuda")
        params = list(policy.parameters())
        e = vs.VecSimEnv(name, N, dt=dt, max_steps=4000)
        e.set_auto_reset(False)
        e.reset(seed=1)
        init = e.get(L.VS_STATE)
        e.set_record_mode(2)
        e.set_traj_capacity(T)
        e.set_policy_rnn(**spec)
        e.set_policy_hidden_record(Hs)
        e.reset(init_state=init)
        e.step_policy(T, record=True)
        g_rew = torch.randn(T, e.ld, device="cuda")
        g_obs = torch.randn(T + 1, O, e.ld, device="cuda")
        g_act = torch.randn(T, A, e.ld, device="cuda")
        g_last = torch.randn(S + H, e.ld, device="cuda")
        kept = {}
        flat = torch.empty(e._rnn_n_params, device="cuda")

        def sweep():
            e.timer_start()
            kept["abar"], _, kept["d_hid"], _ = e.rollout_vjp_rnn(T, g_rew=g_rew, g_obs=g_obs, g_act=g_act, g_state_last=g_last)
            return e.timer_stop()

        def kernel_pass():
            e.timer_start()
            e.rnn_param_grad(T, kept["abar"], kept["d_hid"], out=flat)
            return e.timer_stop()

        def torch_pass():
            seen = e.traj_tensors(T, N)["obs"].transpose(0, 1).reshape(N * T, O)
            abar, d_hid, hid = (vs.lanes_first(x, N).reshape(N * T, -1) for x in (kept["abar"], kept["d_hid"], e.hidden_record_tensor()[:T]))
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            ev0.record()
            total = None
            for r0 in range(0, N * T, PASS_ROWS):
                rows = slice(r0, min(r0 + PASS_ROWS, N * T))
                with torch.enable_grad():
                    act, p_new = policy(seen[rows], hid[rows])
                    g = torch.autograd.grad((act, p_new), params, grad_outputs=(abar[rows], d_hid[rows]))
                total = g if total is None else tuple(a + b for a, b in zip(total, g))
            ev1.record()
            torch.cuda.synchronize()
            kept["torch"] = torch.cat([x.reshape(-1) for x in total])
            return ev0.elapsed_time(ev1)

        labels = ["closed-loop sweep (vs_rollout_vjp_rnn)", "kernel parameter pass (vs_rnn_param_grad)", "torch parameter pass"]
        ms = {label: [] for label in labels}
        for r in range(ROUNDS + 1):  # round 0 warms up (loads the kernels, torch's allocator)
            row = [sweep(), kernel_pass(), torch_pass()]
            if r:
                for label, x in zip(labels, row):
                    ms[label].append(x)
        mean_len = float(e.rollout_lengths(N, T)[0].float().mean())
        agree = float((flat - kept["torch"]).abs().max() / kept["torch"].abs().max())
        for label in labels:
            m, lo, hi = spread(ms[label])
            lines.append(f"{tag:12s} {label:44s} {m:10.3f} ({lo:.3f} .. {hi:.3f})")
        ratio = spread(ms[labels[2]])[0] / spread(ms[labels[1]])[0]
        lines.append(f"{tag:12s} torch / kernel {ratio:.2f}; max |kernel - torch| / max |torch| {agree:.1e}; mean rollout length "
                     f"{mean_len:.1f} of {T} steps, errors {e.error_count()}")
        e.close()
    text = "\n".join(lines)
    print(text, flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
