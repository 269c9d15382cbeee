"""SHA-256 of every input and every fp64 reference of the derivative tests, and the verdicts of their tolerance rules on those
references, to compare two versions of tests/ bit for bit.  No device is needed: oracle/cpu_ref.py and numpy only.

    python profiles/derivative_case_digest.py --tree OLD_TREE > old.txt
    python profiles/derivative_case_digest.py --tree . > new.txt  &&  diff old.txt new.txt

--tree: the checkout whose tests/ and oracle/ are imported (default: this one).  --only MODULE ...: a subset of the eight modules.
Per module: a line per case(key) / oracle_case(name) with the digest over every array in it; a line per oracle_reference(...) with the
digest over every output (lane lengths included) and over the smooth mask; and the (bad share, worst error / tolerance) pairs of the
module's rule, repr'd floats, for got = the reference itself and for a seeded perturbed copy.  A rule is looked up under its name from
before tests/derivative_cases.py (smooth_of, within) or after (smooth_per_lane / smooth_global, ...): one script reads both trees.
test_gpu_trajectory_grad's oracle_reference takes the device's initial hidden state and step counts; the oracle's own reset and the
recordings' lengths stand in.  derivative_case_digest.txt, next to this file, is the output: equal before and after that module.

The three closed-loop sweep modules (SWEEPS) are printed under their own names from either home of their cases and references: the
test modules themselves, or tests/closed_loop_cases.py, where one loop serves the three policy families (fields_of puts the two
forms of a reference into one).  Beyond case and oracle_reference they get a line per hidden_reference(key, start) for both starts
(hidden block and lane lengths), and for the keys of the hidden families a line for the action-offset and initial-state block from
hidden_start() with its actions and pre-activations -- oracle_reference(key, "perturbed"), or what the recurrent module's
hidden_reference returned next to the hidden block.  test_lin_param_grad_host: a line per case(key), its rows and its fp64
reference with the bound.
"""
import argparse
import hashlib
import importlib
import os
import sys

import numpy as np

MODULES = ("test_gpu_rollout_vjp", "test_gpu_rollout_vjp_params", "test_gpu_trajectory_grad", "test_gpu_policy_vjp", "test_gpu_fnn_vjp",
           "test_gpu_rnn_vjp", "test_gpu_fnn_param_grad", "test_lin_param_grad_host")
SWEEPS = {"test_gpu_policy_vjp": "LINEAR", "test_gpu_fnn_vjp": "FNN", "test_gpu_rnn_vjp": "RNN"}
GLOBAL = ("test_gpu_rollout_vjp_params", "test_gpu_trajectory_grad")  # one unit per family; the others: one unit per lane


def arrays(v):  # every array of a nested case, in order; strings and numbers as they are; other objects (the oracle) left out
    if isinstance(v, dict):
        for k in v:
            yield k
            yield from arrays(v[k])
    elif isinstance(v, (list, tuple)):
        for x in v:
            yield from arrays(x)
    elif isinstance(v, (np.ndarray, str, int, float, bool, type(None))):
        yield v


def sha(v):
    h = hashlib.sha256()
    for p in arrays(v):
        h.update((str((p.dtype, p.shape)).encode() + np.ascontiguousarray(p).tobytes()) if isinstance(p, np.ndarray) else repr(p).encode())
    return h.hexdigest()


def line(*words):
    print(*words, flush=True)


def verdicts(m, mod, label, f1, f2):
    kind = "global" if mod in GLOBAL else "per_lane"
    smooth = (getattr(m, "smooth_of", None) or getattr(m, "smooth_" + kind))(f1, f2)
    line(mod, label, "smooth", sha(smooth), repr(float(smooth.mean())))
    noisy = f1 * (1.0 + 4e-3 * np.random.default_rng(7).normal(size=f1.shape))
    for rule in ("within", "within_" + kind, "worst_of"):
        if hasattr(m, rule):
            line(mod, label, rule.split("_")[0], repr(getattr(m, rule)(f1, f1, smooth)), repr(getattr(m, rule)(noisy, f1, smooth)))
    if mod in GLOBAL:
        line(mod, label, "within no mask", repr((getattr(m, "within", None) or m.within_global)(noisy, f1)))


def fields_of(out):
    """a reference in the order every form of it has: f1, f2, lane lengths, actions, open-loop d_init, (cut d_init,) (pre-activations);
    a field that a family does not have is None in closed_loop_cases.Reference and absent from the old tuples"""
    return [x for x in out if x is not None]


def sweep(mod, m):
    """the lines of one closed-loop sweep module"""
    try:
        home = importlib.import_module("closed_loop_cases")
        cases = {**getattr(home, SWEEPS[mod] + "_CASES"), **(home.ELMAN_AS_FNN if SWEEPS[mod] == "RNN" else {})}
        oracle_cases = getattr(home, SWEEPS[mod] + "_ORACLE_CASES")
    except ImportError:
        home, cases, oracle_cases = m, {**m.CASES, **getattr(m, "ELMAN_AS_FNN", {})}, m.ORACLE_CASES
    dc = importlib.import_module("derivative_cases")
    hidden_keys = list(getattr(m, "HIDDEN_CASES", {}).values()) or list(dc.HIDDEN_FAMILIES)
    for key in cases:
        line(mod, key, "case", sha(home.case(key)))
    for key in oracle_cases:
        out = fields_of(home.oracle_reference(key))
        line(mod, key, "oracle_reference", sha(out))
        verdicts(m, mod, key, out[0], out[1])
    for key in hidden_keys:
        for start in dc.STARTS:
            g1, g2, length, *more = home.hidden_reference(key, start)
            line(mod, key, start, "hidden_reference", sha([g1, g2, length]))
            if start == "perturbed":
                if home is not m or SWEEPS[mod] != "RNN":
                    out = fields_of(home.oracle_reference(key, start))
                    f1, f2, length2, acts, pres = out[0], out[1], out[2], out[3], out[5:] if home is m else out[4:]
                else:
                    (f1, f2, acts, *pres), length2 = more[0], length
                line(mod, key, start, "offsets and states", sha([f1, f2, length2, acts, list(pres)]))
                verdicts(m, mod, f"{key} {start}", f1, f2)


def param_grad_host(mod, m):
    for key in m.ALL_CASES:
        c, r = m.case(key), m.oracle_rows(key)
        line(mod, key, "case", sha(c))
        line(mod, key, "oracle_rows", sha(r))
        ref = m.lin_param_grad_fp64(c["terms"], c["obs_idx"], r["obs"], r["abar"], r["inside"], chain=m.chain_of(m.ld_of(m.N), m.T))
        line(mod, key, "lin_param_grad_fp64", sha(list(ref)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--only", nargs="*", default=MODULES)
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    sys.path[:0] = [os.path.join(tree, "tests"), tree]
    for mod in args.only:
        m = importlib.import_module(mod)
        assert os.path.abspath(m.__file__).startswith(tree), m.__file__
        if mod in SWEEPS:
            sweep(mod, m)
        elif mod == "test_lin_param_grad_host":
            param_grad_host(mod, m)
        elif mod == "test_gpu_fnn_param_grad":  # its cases are test_gpu_fnn_vjp's; its own input is abar
            for key in m.TABLE:
                line(mod, key, "abar", sha(m.abar_of(key, m.N, m.T)))
        elif mod == "test_gpu_trajectory_grad":
            for name in m.FAMILIES:
                c = m.oracle_case(name)
                line(mod, name, "oracle_case", sha(c))
                s0 = c["init"].astype(np.float64)
                h0 = c["ref"].reset(c["params"].astype(np.float64), s0, True)["hidden"]
                n_sum = m.REC_LEN[m.LANE_REC]
                (g1, n1), (g2, n2) = m.oracle_reference(name, c["params"], s0, h0, c["table"], c["target"], c["weights"], n_sum, m.WRT[name])
                line(mod, name, "oracle_reference", sha([g1, n1, g2, n2, n_sum]))
                verdicts(m, mod, name + " grad", g1, g2)
                verdicts(m, mod, name + " gn", n1, n2)
        else:
            keys = getattr(m, "FAMILIES", None) or list({**m.CASES, **getattr(m, "ELMAN_AS_FNN", {})})
            for key in keys:
                line(mod, key, "case", sha(m.case(key)))
            short = [(k, 1) for k in ("qq-su", "qbb")] if mod == "test_gpu_rollout_vjp_params" else []  # its one-step references
            for key, *more in [(k,) for k in getattr(m, "ORACLE_CASES", keys)] + short:
                out = m.oracle_reference(key, *more)
                line(mod, key, *more, "oracle_reference", sha(list(out)))
                verdicts(m, mod, " ".join(map(str, (key, *more))), out[0], out[1])


if __name__ == "__main__":
    main()
