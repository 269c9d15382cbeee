"""Throughput of trajectory matching (TrajectoryMatchSampler, vs_set_policy_playback + vs_set_rollout_target, k_rollout_play) on
QQube swing-up: 65 536 lanes = 1 024 domain-parameter candidates x 64 recorded segments of 400 steps.

  * evaluate(): one whole TrajectoryMatchSampler.evaluate() call (parameters per lane, full-state reset, the launches, the
    result tensors), wall time with a device synchronisation, ROUNDS rounds, median and spread (min .. max);
  * launches: the bare vs_step_policy launches of the same work (record = 0, the discrepancy accumulated in the kernel), device
    time between HIP events;
  * yardstick: the same number of lanes and steps through vs_step_random with record = 0 and auto-reset off (the uniform
    policy: no table gathers, no accumulator), same launch length, device time between HIP events, alternating with the above.
Prints a table (and writes it to the path given as argv[1]).

    python profiles/bench_trajectory_match.py [out.txt]
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import simurlacra_amd as vs  # noqa: E402

P, R, T, CHUNK, ROUNDS = 1024, 64, 400, 128, 5


def spread(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2], xs[0], xs[-1]


def recordings(env):
    """R segments of T steps: smooth random voltages, the observations of the nominal simulator replaying them"""
    rng = np.random.default_rng(0)
    t = np.arange(T)[None, :, None] * env.dt
    acts = (1.5 * np.sin(2 * np.pi * rng.uniform(0.5, 3.0, (R, 1, 1)) * t + rng.uniform(0, 6.28, (R, 1, 1)))).astype(np.float32)
    np.random.seed(1)
    inits = np.stack([env.init_space.sample_uniform() for _ in range(R)]).astype(np.float32)
    g = vs.VecSimEnv("qq-su", R, dt=env.dt, max_steps=4000)
    g.reset(init_state=inits)
    g.set_policy_playback(acts, None, np.arange(R, dtype=np.int32))
    g.set_traj_capacity(T + 1)
    g.step_policy(T + 1, record=True)
    obs = g.traj(T + 1)["obs"].transpose(1, 0, 2).copy()  # [R, T + 1, O]
    g.close()
    return [a for a in acts], [o for o in obs], inits


def main():
    env = vs.QQubeSwingUpSim(dt=0.004, max_steps=4000)
    acts, obs, inits = recordings(env)
    names = ["mass_pend_pole", "length_pend_pole", "mass_rot_pole", "length_rot_pole"]
    nominal = np.array([env.domain_param[k] for k in names])
    cands = (nominal * np.random.default_rng(2).uniform(0.8, 1.2, (P, len(names)))).astype(np.float32)
    smp = vs.TrajectoryMatchSampler(env, acts, obs, inits, batch_lanes=P * R, chunk=CHUNK)
    res = smp.evaluate(cands, names=names)  # warm-up (creates the handle)
    torch.cuda.synchronize()
    v = smp._vec
    n = P * R
    launches = [min(CHUNK, T - t) for t in range(0, T, CHUNK)]
    wall, play, uni = [], [], []
    for _ in range(ROUNDS):
        t0 = time.perf_counter()
        res = smp.evaluate(cands, names=names)
        torch.cuda.synchronize()
        wall.append(time.perf_counter() - t0)
        v.reset(init_state=np.tile(inits, (P, 1)))
        v.timer_start()
        for k in launches:
            v.step_policy(k, record=False)
        play.append(v.timer_stop() * 1e-3)
        v.reset(init_state=np.tile(inits, (P, 1)))
        v.timer_start()
        for k in launches:
            v.step_random(k, seed=7, record=False)
        uni.append(v.timer_stop() * 1e-3)
    steps = int(res.steps.sum())
    lines = [f"trajectory matching on QQube swing-up: {P} candidates x {R} segments = {n} lanes, {T} steps, launches of {CHUNK}; "
             f"library version {vs._lib.load().vs_version()}, {ROUNDS} rounds: median (min .. max)",
             f"steps summed into the discrepancies: {steps} of {n * T}"]
    for label, xs in (("TrajectoryMatchSampler.evaluate(), wall", wall), ("vs_step_policy launches (playback + discrepancy, record 0), device", play),
                      ("vs_step_random launches (uniform policy, record 0), device", uni)):
        m, lo, hi = spread(xs)
        lines.append(f"{label:72s} {m * 1e3:8.3f} ms ({lo * 1e3:.3f} .. {hi * 1e3:.3f})   {n * T / m:.3e} env-steps/s")
    lines.append(f"ratio playback launches / uniform-policy launches: {spread(play)[0] / spread(uni)[0]:.3f}; "
                 f"evaluate() / playback launches: {spread(wall)[0] / spread(play)[0]:.2f}")
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")
    smp.close()


if __name__ == "__main__":
    main()
