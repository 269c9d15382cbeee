"""Worst absolute error of the two feature functions of the linear policy for which the project states no figure -- the bell
exp2f(-0.72134752 (v v)) and the device library's atan2f -- against fp64, over the observations of the derivative test cases.

Per case of tests/lin_param_grad_fp64.TABLE the states of its recorded closed-loop rollout (150 lanes x 24 rows) become the
initial states of ONE handle of 3 600 lanes; a recording step_policy(1) with a single-feature linear policy of weight 1 then leaves
that feature of every lane's observation in the record's raw action, as k_rollout_lin evaluates it (fmaf(1, phi, 0) = phi exactly):
the bell of observation row k through obs_idx = (k,), atan2 of every ordered pair of rows.  k_lin_param_grad evaluates the same
expressions.  Prints the table (and writes it to the path given as argv[1]).

    python profiles/lin_feature_errors.py [out.txt]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import simurlacra_amd as vs  # noqa: E402
import param_grad_cases as pgc  # noqa: E402
import lin_param_grad_fp64 as host  # noqa: E402
from derivative_cases import KW, MAX_STEPS, N, T  # noqa: E402


def main():
    lines = [f"absolute error of the bell and atan2 features against fp64 over the recorded observations of the derivative cases; "
             f"library version {vs._lib.load().vs_version()}"]
    worst = {"bell": 0.0, "atan2": 0.0}
    for key in host.TABLE:
        c = host.case(key)
        name, O, A = c["name"], c["ref"].O, c["ref"].A
        e = pgc.recorded(vs, c, lambda e: e.set_policy_linear(c["W"].reshape(-1), list(c["terms"]), obs_idx=c["obs_idx"]))
        states = e.traj_tensors(T, N)["state"].cpu().numpy().reshape(T * N, -1)
        e.close()
        n = states.shape[0]
        h = vs.VecSimEnv(name, n, max_steps=MAX_STEPS, **KW[name])
        h.set_auto_reset(False)
        h.set_record_mode(2)
        h.set_traj_capacity(1)

        def feature(terms, obs_idx):
            h.set_policy_linear(np.ones(A, dtype=np.float32), terms, obs_idx=obs_idx)
            h.reset(init_state=states)
            h.set_traj_offset(0)
            h.step_policy(1, record=True)
            tt = h.traj_tensors(1, n)
            return tt["obs"][0].cpu().numpy().astype(np.float64), tt["act"][0, :, 0].cpu().numpy().astype(np.float64)

        eb = ea = 0.0
        for k in range(O):
            obs, got = feature(["bell"], (k,))
            eb = max(eb, float(np.abs(got - np.exp(-obs[:, k] ** 2 / 2.0)).max()))
        for i in range(O):
            for j in range(O):
                if i != j:
                    obs, got = feature([("atan2", (i, j))], None)
                    ea = max(ea, float(np.abs(got - np.arctan2(obs[:, i], obs[:, j])).max()))
        rng = float(np.abs(obs).max())
        h.close()
        worst["bell"], worst["atan2"] = max(worst["bell"], eb), max(worst["atan2"], ea)
        lines.append(f"{key:10s} {n} observations of {O} rows, max |obs| {rng:8.3f}: bell {eb:.3e}   atan2 {ea:.3e}")
    lines.append(f"worst: bell {worst['bell']:.3e}   atan2 {worst['atan2']:.3e}")
    text = "\n".join(lines)
    print(text, flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
