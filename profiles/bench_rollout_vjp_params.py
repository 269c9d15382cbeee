"""Cost of the reverse-mode sweep with domain-parameter gradients (vs_rollout_vjp_params, k_rollout_vjp_dp) on QQube swing-up, cartpole
swing-up and the ball balancer: 16 384 lanes x 400 steps, every lane its own recording, random cotangents on rewards, observations
and the last state.

Per family ROUNDS rounds, each timing one after the other (interleaved repeats, so that clock and temperature drift hit every variant
alike), device times between HIP events on the handle's stream:
  1. the plain sweep: one vs_rollout_vjp over the 400 recorded rows;
  2. the sweep with G = 1, 2 and 4 parameters: one vs_rollout_vjp_params over the same records and cotangents (G = 8 is two of them:
     what DifferentiableRollout runs for more than four names);
  3. the recording forward launch both need first: reset + one vs_step_policy of 400 steps in record mode 2;
  4. the forward-mode route to a parameter gradient (vs_set_rollout_sens, the launch under TrajectoryMatchSampler.evaluate_grad):
     reset + one non-recording vs_step_policy of 400 steps with G = 1, 2 and 4 tangents carried, on a second handle with the same
     rollouts and a target table.  It needs no records and no sweep, and serves one loss only: the weighted squared discrepancy.
The table gives the median (min .. max) of each and the ratio to the plain sweep.  Prints it (and writes it to the path given as
argv[1]).

    python profiles/bench_rollout_vjp_params.py [out.txt]
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import simurlacra_amd as vs  # noqa: E402
from simurlacra_amd import _lib as L  # noqa: E402

N, T, ROUNDS = 16384, 400, 5
FAMILIES = {
    "qq-su": (0.004, 1.5, ["motor_resistance", "motor_back_emf", "mass_pend_pole", "damping_pend_pole", "mass_rot_pole",
                           "length_rot_pole", "length_pend_pole", "damping_rot_pole"]),
    "qcp-su": (0.002, 3.0, ["cart_mass", "motor_resistance", "pole_mass", "pole_length", "motor_back_emf", "pole_damping",
                            "combined_damping", "pinion_radius"]),
    "qbb": (0.01, 1.0, ["ball_mass", "arm_radius", "motor_back_emf", "motor_resistance", "ball_radius", "gear_ratio", "load_inertia",
                        "motor_inertia"]),
}


def spread(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2], xs[0], xs[-1]


def main():
    lines = [f"vs_rollout_vjp_params against vs_rollout_vjp, the recording launch and the forward-mode launch of vs_set_rollout_sens: "
             f"{N} lanes x {T} steps; library version {L.load().vs_version()}, {ROUNDS} interleaved rounds: device ms between HIP "
             f"events, median (min .. max)"]
    for name, (dt, amp, names) in FAMILIES.items():
        rng = np.random.default_rng(0)
        d = vs.env_dims(name)
        S, A, O, H = (d[k] for k in "SAOH")
        all_names = vs.param_names(name)
        names = [k for k in names if k in all_names]
        assert len(names) == 8, (name, all_names)
        t = np.arange(T)[None, :, None] * dt
        acts = torch.as_tensor((amp * np.sin(2 * np.pi * rng.uniform(0.5, 3.0, (N, 1, A)) * t
                                             + rng.uniform(0, 6.28, (N, 1, A)))).astype(np.float32)).cuda()
        params = (vs.nominal_params(name)[None, :] * rng.uniform(0.95, 1.05, (N, d["P"]))).astype(np.float32)
        e = vs.VecSimEnv(name, N, dt=dt, max_steps=4000)
        e.set_auto_reset(False)
        e.set_params(params)
        e.reset(seed=1)
        init = e.get(L.VS_STATE)
        e.set_record_mode(2)
        e.set_traj_capacity(T)
        e.set_policy_playback(acts)
        g_rew = torch.randn(T, e.ld, device="cuda")
        g_obs = torch.randn(T + 1, O, e.ld, device="cuda")
        g_last = torch.randn(S + H, e.ld, device="cuda")
        f = vs.VecSimEnv(name, N, dt=dt, max_steps=4000)  # the forward-mode handle: the same rollouts against a target table
        f.set_auto_reset(False)
        f.set_params(params)
        f.set_policy_playback(acts)
        f.set_rollout_target(torch.zeros(N, T + 1, O, device="cuda"))

        def forward():
            e.reset(init_state=init)
            e.timer_start()
            e.step_policy(T, record=True)
            return e.timer_stop()

        def plain():
            e.timer_start()
            e.rollout_vjp(T, g_rew=g_rew, g_obs=g_obs, g_state_last=g_last)
            return e.timer_stop()

        def sweep(g):
            e.timer_start()
            for j0 in range(0, g, L.VS_SENS_MAX_PARAMS):
                e.rollout_vjp_params(T, names[j0:min(g, j0 + L.VS_SENS_MAX_PARAMS)], g_rew=g_rew, g_obs=g_obs, g_last=g_last)
            return e.timer_stop()

        def sens(g):
            f.set_rollout_sens(names[:g])
            f.reset(init_state=init)
            f.timer_start()
            f.step_policy(T)
            return f.timer_stop()

        variants = [("plain sweep (vs_rollout_vjp)", plain)]
        variants += [(f"sweep with G = {g} (vs_rollout_vjp_params)", lambda g=g: sweep(g)) for g in (1, 2, 4, 8)]
        variants += [("recording forward launch", forward)]
        variants += [(f"forward mode, G = {g} (vs_set_rollout_sens)", lambda g=g: sens(g)) for g in (1, 2, 4)]
        forward()
        for _, fn in variants:  # warm-up (loads the kernels)
            fn()
        ms = {label: [] for label, _ in variants}
        for _ in range(ROUNDS):
            for label, fn in variants:
                ms[label].append(fn())
        base = spread(ms[variants[0][0]])[0]
        for label, _ in variants:
            m, lo, hi = spread(ms[label])
            lines.append(f"{name:7s} {label:44s} {m:10.3f} ({lo:.3f} .. {hi:.3f})   ratio to the plain sweep: {m / base:5.2f}")
        e.close()
        f.close()
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as out:
            out.write(text + "\n")


if __name__ == "__main__":
    main()
