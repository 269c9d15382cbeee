"""Cost of the reverse-mode sweep and parameter pass of a policy POPULATION on one handle (vs_rollout_vjp_pop + vs_pop_param_grad) against
the loop over members it replaces, each member on its own handle with the single-policy entry points (vs_rollout_vjp_policy +
vs_lin_param_grad, vs_rollout_vjp_fnn + vs_fnn_param_grad): QQube swing-up, 400 recorded steps, a LinearPolicy (identity, sin, const,
one product) and an FNNPolicy of [64, 64] tanh units, populations of 256 members x 64 lanes and of 64 members x 256 lanes (16 384 lanes
either way), random cotangents, every member its own weights (the base weights scaled by 1 +- 5 %).

Per policy and population ROUNDS rounds, each timing one after the other (interleaved repeats), all work on the current torch stream,
device time between two events:
  1. population: one vs_rollout_vjp_pop and one vs_pop_param_grad on the population handle;
  2. loop: for every member one sweep and one parameter pass on its own handle (2 P launches + 2 P reductions).
The table gives the median (min .. max) of each in ms and the ratio of the medians.  Prints it (and writes it to the path given as
argv[1]).

    python profiles/bench_population_vjp.py [out.txt]
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import simurlacra_amd as vs  # noqa: E402
from simurlacra_amd import _lib as L  # noqa: E402

T, ROUNDS, DT, NAME = 400, 5, 0.004, "qq-su"
POPULATIONS = ((256, 64), (64, 256))


def spread(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2], xs[0], xs[-1]


def recorded(n, install, init):
    e = vs.VecSimEnv(NAME, n, dt=DT, max_steps=4000)
    e.set_auto_reset(False)
    e.set_record_mode(2)
    e.set_traj_capacity(T)
    install(e)
    e.reset(init_state=init)
    e.step_policy(T, record=True)
    return e


def main():
    lines = [f"vs_rollout_vjp_pop + vs_pop_param_grad on one handle against the loop over members on their own handles: {NAME}, {T} steps; "
             f"library version {L.load().vs_version()}, {ROUNDS} interleaved rounds: device ms, median (min .. max)"]
    env = vs.QQubeSwingUpSim(dt=DT, max_steps=4000)
    d = vs.env_dims(NAME)
    S, A, O, H = (d[k] for k in "SAOH")
    torch.manual_seed(0)
    lin = vs.LinearPolicy(env.spec, vs.FeatureStack(vs.identity_feat, vs.sin_feat, vs.const_feat, vs.MultFeat((0, 1))))
    with torch.no_grad():
        lin.net.weight.normal_(0.0, 0.3)
    fnn = vs.FNNPolicy(env.spec, hidden_sizes=[64, 64], hidden_nonlin=torch.tanh, featurize=False)
    with torch.no_grad():
        fnn.net.output_layer.weight.mul_(0.2)
    for tag, policy in (("linear", lin), ("fnn 64x64", fnn)):
        linear = tag == "linear"
        spec = (vs.linear_kernel_spec if linear else vs.fnn_kernel_spec)(policy)
        spec.pop("noise_std")
        flat = torch.nn.utils.parameters_to_vector(policy.parameters()).detach().numpy()

        def install(e, theta):
            if linear:
                e.set_policy_linear(theta, spec["terms"])
            else:
                e.set_policy_fnn(**dict(spec, params=theta))

        for P, M in POPULATIONS:
            n = P * M
            rng = np.random.default_rng(P)
            theta = (flat[None, :] * (1.0 + 0.05 * rng.uniform(-1.0, 1.0, (P, flat.size)))).astype(np.float32)
            seed_env = vs.VecSimEnv(NAME, n, dt=DT, max_steps=4000)
            seed_env.reset(seed=1)
            init = seed_env.get(L.VS_STATE)
            seed_env.close()

            def install_pop(e):
                install(e, theta[0])
                e.set_policy_population(theta, lane_set=np.arange(n) // M)

            pop = recorded(n, install_pop, init)
            singles = [recorded(M, lambda e, s=s: install(e, theta[s]), init[s * M:(s + 1) * M]) for s in range(P)]
            cot = lambda ld: dict(g_rew=torch.randn(T, ld, device="cuda"), g_obs=torch.randn(T + 1, O, ld, device="cuda"),  # noqa: E731
                                  g_act=torch.randn(T, A, ld, device="cuda"), g_state_last=torch.randn(S + H, ld, device="cuda"))
            g_pop, g_one = cot(pop.ld), cot(singles[0].ld)
            out_pop = torch.empty(P, flat.size, device="cuda")
            out_one = torch.empty(P, flat.size, device="cuda")

            def timed(fn):
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                ev0.record()
                fn()
                ev1.record()
                torch.cuda.synchronize()
                return ev0.elapsed_time(ev1)

            def population():
                with pop.on_current_stream():
                    da, _ = pop.rollout_vjp_population(T, **g_pop)
                    pop.population_param_grad(T, da, out=out_pop)

            def loop():
                for s, e in enumerate(singles):
                    with e.on_current_stream():
                        if linear:
                            e.lin_param_grad(T, e.rollout_vjp_policy(T, **g_one)[0], out=out_one[s])
                        else:
                            e.fnn_param_grad(T, e.rollout_vjp_fnn(T, **g_one)[0], out=out_one[s])

            ms = {"population": [], "loop": []}
            for r in range(ROUNDS + 1):  # round 0 warms up
                row = timed(population), timed(loop)
                if r:
                    ms["population"].append(row[0]), ms["loop"].append(row[1])
            a, b = spread(ms["population"]), spread(ms["loop"])
            lines.append(f"{tag:10s} {P:4d} x {M:3d} lanes  population {a[0]:9.3f} ({a[1]:.3f} .. {a[2]:.3f})   loop over members "
                         f"{b[0]:9.3f} ({b[1]:.3f} .. {b[2]:.3f})   loop / population {b[0] / a[0]:.2f}; errors {pop.error_count()}")
            pop.close()
            for e in singles:
                e.close()
    text = "\n".join(lines)
    print(text, flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
