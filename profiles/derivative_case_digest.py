"""SHA-256 of every input and every fp64 reference of the derivative tests, and the verdicts of their tolerance rules on those
references, to compare two versions of tests/ bit for bit.  No device is needed: oracle/cpu_ref.py and numpy only.

    python profiles/derivative_case_digest.py --tree OLD_TREE > old.txt
    python profiles/derivative_case_digest.py --tree . > new.txt  &&  diff old.txt new.txt

--tree: the checkout whose tests/ and oracle/ are imported (default: this one).  --only MODULE ...: a subset of MODULES.
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

The parameter-gradient lines (PARAM_GRAD) keep the name of the test module they were first printed under, and home_of() reads every
object from the first module of the tree that has it: the reference modules fnn_param_grad_fp64, lin_param_grad_fp64,
rnn_param_grad_fp64 and param_grad_cases, or the test modules that held them before.  test_fnn_param_grad_host: per TABLE key the
seeded random_net and param_grad_fp64 with its bound on the host test's own rows.  test_gpu_rnn_param_grad: case(key) of CASES and
ELMAN_AS_FNN.  test_rnn_param_grad_host: rows_case(key) and its reference with the bound.  param_grad_grids: the three launch grid
rules and the linear pass's chain_of at the (ld, t_steps) pairs of the host test, for 256 and 304 compute units (the rules that used
to ask torch for the device's count are given a stand-in).
"""
import argparse
import hashlib
import importlib
import os
import sys
import types

import numpy as np

MODULES = ("test_gpu_rollout_vjp", "test_gpu_rollout_vjp_params", "test_gpu_trajectory_grad", "test_gpu_policy_vjp", "test_gpu_fnn_vjp",
           "test_gpu_rnn_vjp", "test_gpu_fnn_param_grad", "test_lin_param_grad_host", "test_fnn_param_grad_host", "test_gpu_rnn_param_grad",
           "test_rnn_param_grad_host", "param_grad_grids")
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


def home_of(name, *mods):
    """the first of the tree's modules `mods` that has `name`"""
    for mod in mods:
        try:
            m = importlib.import_module(mod)
        except ImportError:
            continue
        if hasattr(m, name):
            assert os.path.abspath(m.__file__).startswith(sys.path[0]), m.__file__
            return m
    raise LookupError(name)


def fnn_abar(mod):  # the cases are test_gpu_fnn_vjp's; the pass's own input is abar
    m = home_of("abar_of", "fnn_param_grad_fp64", "test_gpu_fnn_param_grad")
    dc = importlib.import_module("derivative_cases")
    for key in getattr(m, "GPU_TABLE", m.TABLE):  # (the GPU test's own TABLE was that list)
        line(mod, key, "abar", sha(m.abar_of(key, dc.N, dc.T)))


def lin_host(mod):
    m = home_of("lin_param_grad_fp64", "lin_param_grad_fp64", "test_lin_param_grad_host")
    chain_of = home_of("chain_of", "param_grad_cases", "test_lin_param_grad_host").chain_of
    dc = importlib.import_module("derivative_cases")
    for key in m.ALL_CASES:
        c, r = m.case(key), m.oracle_rows(key)
        line(mod, key, "case", sha(c))
        line(mod, key, "oracle_rows", sha(r))
        ref = m.lin_param_grad_fp64(c["terms"], c["obs_idx"], r["obs"], r["abar"], r["inside"], chain=chain_of(m.ld_of(dc.N), dc.T))
        line(mod, key, "lin_param_grad_fp64", sha(list(ref)))


def fnn_host(mod):
    """the rows of test_the_fp64_reference_is_torch_autograd_of_the_double_module, drawn as that test draws them"""
    m = home_of("param_grad_fp64", "fnn_param_grad_fp64", "test_fnn_param_grad_host")
    dc = importlib.import_module("derivative_cases")
    for key in sorted(m.TABLE):
        name = m.TABLE[key][0]
        ref = dc.cpu_ref.make_ref(name, max_steps=dc.MAX_STEPS, **dc.KW[name])
        rng = np.random.default_rng(sorted(m.TABLE).index(key))
        net = m.random_net(key, rng, ref.O, ref.A)
        line(mod, key, "random_net", sha(net))
        obs = rng.normal(size=(300, ref.O)).astype(np.float32)
        abar = rng.normal(size=(300, ref.A)).astype(np.float32)
        inside = rng.uniform(size=300) < 0.8
        line(mod, key, "param_grad_fp64", sha(list(m.param_grad_fp64(net, obs, abar, inside, chains=dict(acc=64, wg=8)))))


def rnn_cases(mod):
    m = home_of("ELMAN_AS_FNN", "param_grad_cases", "test_gpu_rnn_param_grad")
    for key in {**m.CASES, **m.ELMAN_AS_FNN}:
        line(mod, key, "case", sha(m.case(key)))


def rnn_host(mod):
    m = home_of("rows_case", "rnn_param_grad_fp64", "test_rnn_param_grad_host")
    ref64 = importlib.import_module("rnn_param_grad_fp64")
    for key in m.TABLE:
        _, net, x, p, abar, d_hid, inside, out = m.rows_case(key)
        line(mod, key, "rows_case", sha([net, x, p, abar, d_hid, inside, out]))
        line(mod, key, "param_grad_fp64", sha(list(ref64.param_grad_fp64(net, x, p, abar, d_hid, inside, out))))


GRID_PAIRS = ((256, 24), (256, 1), (2304, 40), (3328, 41), (128, 12), (128, 7), (1792, 41), (1536, 41))


def grid_rule(kind, n_cu):
    """(ld, t_steps) -> (n_wg, rows) of one family's rule, from either home"""
    try:
        rule = getattr(home_of(kind + "_grid_of", "param_grad_cases"), kind + "_grid_of")
        return lambda ld, t: rule(ld, t, n_cu)
    except LookupError:
        if kind == "lin":
            return lambda ld, t: importlib.import_module("test_lin_param_grad_host").grid_of(ld, t, n_cu)
    m = importlib.import_module(f"test_gpu_{kind}_param_grad")
    import torch

    def asked(ld, t):  # the rule asks torch for the device's compute units
        real = torch.cuda.get_device_properties
        torch.cuda.get_device_properties = lambda *a: types.SimpleNamespace(multi_processor_count=n_cu)
        try:
            return m.grid_of(ld, t)
        finally:
            torch.cuda.get_device_properties = real

    return asked


def grids(mod):
    chain_of = home_of("chain_of", "param_grad_cases", "test_lin_param_grad_host").chain_of
    for n_cu in (256, 304):
        for kind in ("fnn", "rnn", "lin"):
            rule = grid_rule(kind, n_cu)
            for ld, t in GRID_PAIRS:
                line(mod, kind, n_cu, ld, t, "grid", *map(int, rule(ld, t)))
        for ld, t in GRID_PAIRS:
            line(mod, "lin", n_cu, ld, t, "chain_of", int(chain_of(ld, t, n_cu)), int(chain_of(ld, t, n_cu, 1)))


PARAM_GRAD = {"test_gpu_fnn_param_grad": fnn_abar, "test_lin_param_grad_host": lin_host, "test_fnn_param_grad_host": fnn_host,
              "test_gpu_rnn_param_grad": rnn_cases, "test_rnn_param_grad_host": rnn_host, "param_grad_grids": grids}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--only", nargs="*", default=MODULES)
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    sys.path[:0] = [os.path.join(tree, "tests"), tree]
    for mod in args.only:
        if mod in PARAM_GRAD:
            PARAM_GRAD[mod](mod)
            continue
        m = importlib.import_module(mod)
        assert os.path.abspath(m.__file__).startswith(tree), m.__file__
        if mod in SWEEPS:
            sweep(mod, m)
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
