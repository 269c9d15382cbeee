"""Cost of the in-kernel weight gradient of a linear policy on a feature stack (vs_lin_param_grad: k_lin_param_grad +
k_fnn_param_reduce) against the torch pass it replaces, on the shapes of bench_fnn_param_grad.py: QQube swing-up, cartpole swing-up
and the ball balancer, 16 384 lanes x 400 steps recorded with a LinearPolicy in the loop, random cotangents.  Two stacks per family:
  small  identity, sin, const, MultFeat((0, 1))
  full   the 11 elementwise kinds, const and 39 MultFeat / ATan2Feat terms: 11 O + 40 features (128 on the ball balancer's 8 rows)

Per family and stack ROUNDS rounds, each timing one after the other (interleaved repeats):
  1. the closed-loop sweep: one vs_rollout_vjp_policy over the 400 recorded rows (HIP events on the handle's stream);
  2. the kernel parameter pass: one vs_lin_param_grad on the sweep's d_act (HIP events on the handle's stream);
  3. the torch parameter pass of the same run: torch.autograd.grad(policy(obs), weight, grad_outputs=abar) over the [N T] rows, in
     device time between torch events and in wall time -- the copies that feed it (the gather of the record planes, lanes_first of
     abar) are NOT counted here, they are part of 4;
  4. DifferentiablePolicyRollout's whole backward() in wall time with a device synchronisation, param_pass="kernel" against "torch"
     (one batch of 16 384 lanes; loss = -discounted return + 1e-3 sum a^2).
The table gives the median (min .. max) of each in ms.  Prints it (and writes it to the path given as argv[1]).

    python profiles/bench_lin_param_grad.py [out.txt]
"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import simurlacra_amd as vs  # noqa: E402
from simurlacra_amd import _lib as L  # noqa: E402

N, T, ROUNDS = 16384, 400, 5
FAMILIES = {"qq-su": (0.004, "QQubeSwingUpSim"), "qcp-su": (0.002, "QCartPoleSwingUpSim"), "qbb": (0.01, "QBallBalancerSim")}
ELEM = (vs.identity_feat, vs.sign_feat, vs.abs_feat, vs.squared_feat, vs.cubic_feat, vs.sig_feat, vs.bell_feat, vs.sin_feat,
        vs.cos_feat, vs.sinsin_feat, vs.sincos_feat)


def stack(which, O):
    if which == "small":
        return vs.FeatureStack(vs.identity_feat, vs.sin_feat, vs.const_feat, vs.MultFeat((0, 1)))
    extra = [vs.MultFeat((i % O, (i + 1) % O)) for i in range(13)] + [vs.MultFeat((i % O, (i + 2) % O, (i + 3) % O)) for i in range(13)]
    extra += [vs.ATan2Feat(i % O, (i + 1) % O) for i in range(13)]
    return vs.FeatureStack(*ELEM, vs.const_feat, *extra)


def spread(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2], xs[0], xs[-1]


def main():
    lines = [f"vs_lin_param_grad against the torch parameter pass of the same run and the closed-loop sweep: {N} lanes x {T} steps, "
             f"LinearPolicy, default weights scaled by 0.05; library version {L.load().vs_version()}, {ROUNDS} interleaved rounds: "
             f"ms, median (min .. max)"]
    for name, which, dt, cls in [(name, which, dt, cls) for name, (dt, cls) in FAMILIES.items() for which in ("small", "full")]:
        torch.manual_seed(0)
        d = vs.env_dims(name)
        S, A, O, H = (d[k] for k in "SAOH")
        env = getattr(vs, cls)(dt=dt, max_steps=4000)
        policy = vs.LinearPolicy(env.spec, stack(which, O))
        with torch.no_grad():
            policy.net.weight.mul_(0.05)
        spec = vs.linear_kernel_spec(policy)
        spec.pop("noise_std")
        tag = f"{name} {which} F={policy.num_active_feat}"
        policy.to("cuda")
        e = vs.VecSimEnv(name, N, dt=dt, max_steps=4000)
        e.set_auto_reset(False)
        e.reset(seed=1)
        init = e.get(L.VS_STATE)
        e.set_record_mode(2)
        e.set_traj_capacity(T)
        e.set_policy_linear(**spec)
        e.reset(init_state=init)
        e.step_policy(T, record=True)
        g_rew = torch.randn(T, e.ld, device="cuda")
        g_obs = torch.randn(T + 1, O, e.ld, device="cuda")
        g_act = torch.randn(T, A, e.ld, device="cuda")
        g_last = torch.randn(S + H, e.ld, device="cuda")
        kept = {}
        flat = torch.empty(e._lin_n_params, device="cuda")

        def sweep():
            e.timer_start()
            kept["abar"] = e.rollout_vjp_policy(T, g_rew=g_rew, g_obs=g_obs, g_act=g_act, g_state_last=g_last)[0]
            return e.timer_stop()

        def kernel_pass():
            e.timer_start()
            e.lin_param_grad(T, kept["abar"], out=flat)
            return e.timer_stop()

        def torch_pass():
            seen = e.traj_tensors(T, N)["obs"].reshape(T * N, O)
            abar = kept["abar"][..., :N].movedim(1, 2).reshape(T * N, A)
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ev0.record()
            with torch.enable_grad():
                g, = torch.autograd.grad(policy(seen), [policy.net.weight], grad_outputs=abar)
            ev1.record()
            torch.cuda.synchronize()
            kept["torch"] = g.reshape(-1)
            return ev0.elapsed_time(ev1), (time.perf_counter() - t0) * 1e3

        rolls = {p: vs.DifferentiablePolicyRollout(env, policy, batch_lanes=N, param_pass=p) for p in ("kernel", "torch")}
        init_t = torch.as_tensor(init).cuda()

        def backward(which_pass):
            obs, rew, act, lengths = rolls[which_pass](init_t, T)
            loss = -vs.discounted_return(rew, lengths, 0.99).sum() + 1e-3 * act.pow(2).sum()
            policy.net.weight.grad = None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss.backward()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        labels = ["closed-loop sweep (vs_rollout_vjp_policy)", "kernel parameter pass (vs_lin_param_grad)",
                  "torch parameter pass, device time", "torch parameter pass, wall time",
                  "backward() wall time, param_pass=kernel", "backward() wall time, param_pass=torch"]
        ms = {label: [] for label in labels}
        for r in range(ROUNDS + 1):  # round 0 warms up (loads the kernels, torch's allocator)
            row = [sweep(), kernel_pass(), *torch_pass(), backward("kernel"), backward("torch")]
            if r:
                for label, x in zip(labels, row):
                    ms[label].append(x)
        mean_len = float(e.rollout_lengths(N, T)[0].float().mean())
        agree = float((flat - kept["torch"]).abs().max() / kept["torch"].abs().max())
        for label in labels:
            m, lo, hi = spread(ms[label])
            lines.append(f"{tag:18s} {label:44s} {m:10.3f} ({lo:.3f} .. {hi:.3f})")
        ratio = spread(ms[labels[2]])[0] / spread(ms[labels[1]])[0]
        lines.append(f"{tag:18s} torch device time / kernel {ratio:.2f}; max |kernel - torch| / max |torch| {agree:.1e}; mean rollout "
                     f"length {mean_len:.1f} of {T} steps, errors {e.error_count()}")
        for r in rolls.values():
            r.close()
        e.close()
    text = "\n".join(lines)
    print(text, flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
