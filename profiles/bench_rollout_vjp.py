"""Cost of the reverse-mode sweep over recorded rollouts (vs_rollout_vjp, k_rollout_vjp) on QQube swing-up, cartpole swing-up and the
ball balancer: 16 384 lanes x 400 steps, every lane its own recording, random cotangents on rewards, observations and the last state.

Per family ROUNDS rounds, each timing one after the other (interleaved repeats, so that clock and temperature drift hit every variant
alike); 1 and 2 are device times between HIP events on the handle's stream, 3 is wall time with a device synchronisation (it is
hundreds of launches and torch ops):
  1. the backward sweep: one vs_rollout_vjp over the 400 recorded rows;
  2. the recording forward launch of the same rollouts: reset + one vs_step_policy of 400 steps in record mode 2;
  3. the only route to the same numbers without the sweep: 400 calls of vs_step_jac along the same actions and the transposed chain
     of their Jacobians in torch on the device (fp32 einsum per step) -- note that it holds the hidden state constant, so for the
     cartpole and the ball balancer it does not even compute the same gradient.
The table gives the median (min .. max) of each.  Prints it (and writes it to the path given as argv[1]).

    python profiles/bench_rollout_vjp.py [out.txt]
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import simurlacra_amd as vs  # noqa: E402
from simurlacra_amd import _lib as L  # noqa: E402
from simurlacra_amd.vec_env import _DevArray  # noqa: E402

N, T, ROUNDS = 16384, 400, 5
FAMILIES = {"qq-su": (0.004, 1.5), "qcp-su": (0.002, 3.0), "qbb": (0.01, 1.0)}


def spread(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2], xs[0], xs[-1]


def jac_views(e):
    """zero-copy device views of the Jacobians of the last vs_step_jac: state [S, S + A, ld], rew [S + A, ld], obs [O, S + A, ld]"""
    S, A, O = e.dims["S"], e.dims["A"], e.dims["O"]
    out = []
    for which, shape in ((L.VS_JAC_STATE, (S, S + A, e.ld)), (L.VS_JAC_REW, (S + A, e.ld)), (L.VS_JAC_OBS, (O, S + A, e.ld))):
        out.append(torch.as_tensor(_DevArray(e._lib.vs_get(e._h, which), shape, "<f4", e), device=f"cuda:{e.device}"))
    return out


def main():
    lines = [f"vs_rollout_vjp against its forward launch and against chained vs_step_jac: {N} lanes x {T} steps; library version "
             f"{L.load().vs_version()}, {ROUNDS} interleaved rounds: ms, median (min .. max); sweep and forward launch between HIP events, "
             f"the chain in wall time"]
    for name, (dt, amp) in FAMILIES.items():
        rng = np.random.default_rng(0)
        d = vs.env_dims(name)
        S, A, O, H = (d[k] for k in "SAOH")
        t = np.arange(T)[None, :, None] * dt
        acts = (amp * np.sin(2 * np.pi * rng.uniform(0.5, 3.0, (N, 1, A)) * t + rng.uniform(0, 6.28, (N, 1, A)))).astype(np.float32)
        e = vs.VecSimEnv(name, N, dt=dt, max_steps=4000)
        e.set_auto_reset(False)
        e.reset(seed=1)
        init = e.get(L.VS_STATE)
        e.set_record_mode(2)
        e.set_traj_capacity(T)
        e.set_policy_playback(torch.as_tensor(acts).cuda())
        g_rew = torch.randn(T, e.ld, device="cuda")
        g_obs = torch.randn(T + 1, O, e.ld, device="cuda")
        g_last = torch.randn(S + H, e.ld, device="cuda")
        acts_soa = torch.as_tensor(np.ascontiguousarray(acts.transpose(1, 2, 0))).cuda()  # [T, A, N]
        j = vs.VecSimEnv(name, N, dt=dt, max_steps=4000)
        j.set_auto_reset(False)

        def forward():
            e.reset(init_state=init)
            e.timer_start()
            e.step_policy(T, record=True)
            return e.timer_stop()

        def backward():
            e.timer_start()
            e.rollout_vjp(T, g_rew=g_rew, g_obs=g_obs, g_state_last=g_last)
            return e.timer_stop()

        def chained():
            # forward: T launches of vs_step_jac, the Jacobians of every step copied aside; backward: the transposed chain
            j.reset(init_state=init)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            kept = []
            for k in range(T):
                j._check(j._lib.vs_step_jac(j._h, acts_soa[k].data_ptr(), 1, N), "vs_step_jac")
                kept.append([x.clone() for x in jac_views(j)])
            lam = g_last[:S]
            for k in range(T - 1, -1, -1):
                js, jr, jo = kept[k]
                new = torch.einsum("jn,jkn->kn", lam, js) + g_rew[k] * jr + torch.einsum("qn,qkn->kn", g_obs[k + 1], jo)
                lam = new[:S]
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        variants = [("backward sweep (vs_rollout_vjp)", backward), ("recording forward launch", forward),
                    ("T x vs_step_jac + torch chain", chained)]
        forward()
        for _, f in variants:  # warm-up (loads the kernels)
            f()
        ms = {label: [] for label, _ in variants}
        for _ in range(ROUNDS):
            for label, f in variants:
                ms[label].append(f())
        for label, _ in variants:
            m, lo, hi = spread(ms[label])
            lines.append(f"{name:7s} {label:34s} {m:10.3f} ({lo:.3f} .. {hi:.3f})")
        e.close()
        j.close()
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
