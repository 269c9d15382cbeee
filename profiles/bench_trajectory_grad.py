"""Cost of TrajectoryMatchSampler.evaluate_grad() (vs_set_rollout_sens, k_rollout_play_sens) relative to one evaluate() on QQube
swing-up, cartpole swing-up and the ball balancer: 16 384 lanes = 256 domain-parameter candidates x 64 recorded segments of 400
steps, G = 1, 2 and 4 differentiated parameters.

Per family ROUNDS rounds, each running evaluate() and evaluate_grad() for G = 1, 2, 4 one after the other (interleaved repeats, so
that clock and temperature drift hit every variant alike), wall time with a device synchronisation; the table gives the median
(min .. max) and the cost ratio to evaluate().  Central differences would cost 2 G evaluate() calls.
Prints a table (and writes it to the path given as argv[1]).

    python profiles/bench_trajectory_grad.py [out.txt]
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import simurlacra_amd as vs  # noqa: E402

P, R, T, CHUNK, ROUNDS = 256, 64, 400, 128, 5
FAMILIES = {
    "qq-su": (vs.QQubeSwingUpSim, 0.004, 1.5, ["motor_resistance", "motor_back_emf", "mass_pend_pole", "damping_pend_pole"]),
    "qcp-su": (vs.QCartPoleSwingUpSim, 0.002, 3.0, ["cart_mass", "motor_resistance", "pole_mass", "pole_length"]),
    "qbb": (vs.QBallBalancerSim, 0.01, 1.0, ["ball_mass", "arm_radius", "motor_back_emf", "motor_resistance"]),
}


def spread(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2], xs[0], xs[-1]


def recordings(name, env, amp):
    """R segments of T steps: smooth random actions, the observations of the nominal simulator replaying them"""
    rng = np.random.default_rng(0)
    A = env.act_space.flat_dim
    t = np.arange(T)[None, :, None] * env.dt
    acts = (amp * np.sin(2 * np.pi * rng.uniform(0.5, 3.0, (R, 1, A)) * t + rng.uniform(0, 6.28, (R, 1, A)))).astype(np.float32)
    g = vs.VecSimEnv(name, R, dt=env.dt, max_steps=4000)
    g.reset(seed=1)
    inits = g.get(vs._lib.VS_STATE)
    g.set_policy_playback(acts, None, np.arange(R, dtype=np.int32))
    g.set_traj_capacity(T + 1)
    g.step_policy(T + 1, record=True)
    obs = g.traj(T + 1)["obs"].transpose(1, 0, 2).copy()  # [R, T + 1, O]
    g.close()
    return [a for a in acts], [o for o in obs], inits


def main():
    lines = [f"evaluate_grad() against evaluate(): {P} candidates x {R} segments = {P * R} lanes, {T} steps, launches of {CHUNK}; "
             f"library version {vs._lib.load().vs_version()}, {ROUNDS} interleaved rounds: wall ms, median (min .. max)"]
    for name, (cls, dt, amp, names) in FAMILIES.items():
        env = cls(dt=dt, max_steps=4000)
        acts, obs, inits = recordings(name, env, amp)
        nominal = np.array([env.domain_param[k] for k in names])
        cands = (nominal * np.random.default_rng(2).uniform(0.95, 1.05, (P, len(names)))).astype(np.float32)
        smp = vs.TrajectoryMatchSampler(env, acts, obs, inits, batch_lanes=P * R, chunk=CHUNK)
        variants = [("evaluate()", lambda: smp.evaluate(cands, names=names))]
        for g in (1, 2, 4):
            variants.append((f"evaluate_grad(), G = {g}", lambda g=g: smp.evaluate_grad(cands, names=names, wrt=names[:g])))
        for _, f in variants:  # warm-up (creates the handle, loads the kernels)
            f()
        torch.cuda.synchronize()
        wall = {label: [] for label, _ in variants}
        for _ in range(ROUNDS):
            for label, f in variants:
                t0 = time.perf_counter()
                f()
                torch.cuda.synchronize()
                wall[label].append(time.perf_counter() - t0)
        base = spread(wall["evaluate()"])[0]
        for label, _ in variants:
            m, lo, hi = spread(wall[label])
            lines.append(f"{name:7s} {label:24s} {m * 1e3:9.3f} ({lo * 1e3:.3f} .. {hi * 1e3:.3f})   ratio to evaluate(): {m / base:5.2f}")
        smp.close()
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
