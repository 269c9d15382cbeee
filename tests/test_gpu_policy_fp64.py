"""k_rollout_fnn (vs_set_policy_fnn / vs_step_policy) against the policy's own torch module in DOUBLE precision, one step at a time on
the kernel's records, at a bound that is derived and not tuned -- at every hidden width where the kernel's padding is live, in all
three evaluation shapes: 64-env workgroups on the vector ALU ('64'), 256-env workgroups on the vector ALU ('256') and 256-env
workgroups with the hidden layers as v_mfma_f32_32x32x2_f32 tiles ('mfma').  tests/test_gpu_policy.py holds the same kernel to fp32
torch at a flat 1e-5 (1 + |ref|) and at widths that are multiples of 8 only; none of the following runs with live padding there:
the second 32-unit tile of a 33 .. 63 wide layer (whose padding rows lean on zero biases and on zero next-layer weights -- under
sigmoid a padding unit is 0.5, not 0), the skipped tile of a layer of at most 32, the first layer's K loop at an odd in_dim and at
in_dim = 1, the zero padding of the packed weights under the 64-lane output reduction, and the matrix-core form of tanh.

Reference.  copy.deepcopy(net).double() on the CPU (the fp32 weights are exact in fp64), fed the RECORDED fp32 observation of every
step (record mode 2, traj()["obs"], then obs_idx and the featurisation in fp64) and compared with the recorded action: the actions do
not feed back into the comparison, so the error of one step does not compound.  The magnitude sums the bound needs come from a NumPy
restatement of the network (tests/policy_fp64.py); every test asserts that it agrees with the .double() module to 1e-12 (1 + |module|).

Bound.  Per entry and first order, from reference quantities and the figures the kernel's comments state, times 2 (the only margin):
derived per layer and per shape in the docstring of tests/policy_fp64.py, held to torch's fp32 forward and to three wrong networks
without a device in tests/test_policy_fp64_host.py.  The flat 1e-5 (1 + |ref|) of test_gpu_policy.py is asserted against the fp64
reference too, so this file is nowhere weaker than that one.  Run with -s to see the worst ratio to the doubled bound of every test.

Conditions, all from the reference alone and all asserted: no unit of any layer is zero on every record (relu biases made positive, the
first of at most four seeds); zeroing any single hidden unit moves the reference's action by more than the doubled bound on some
record (a kernel that dropped unit 32 of a 33-wide layer cannot pass); the tanh test's pre-activations lie beyond 17 and below 1 in
shares of at least 5 % each.  n = 300 is two 256-env workgroups, the second with 44 live lanes; 12 steps run as launches of 5 + 7 and
once more uncut, to the same bits; auto-reset is off and no lane ends.

Measured on an MI355X (worst ratio to the doubled bound; '64' and '256' give the same figure wherever both run): every width
0.079 on the vector ALU and 0.049 on the matrix cores (both [32] with a sigmoid output; the next, [1] sigmoid, 0.040 / 0.010; every
two-layer case below 0.015 in every shape), worst max |act - ref| / (1 + |ref|) 1.0e-6 ([63, 63]); three and four hidden layers
0.004 / 0.014; population 0.003; the tanh forms at gain 24 (16 % of the pre-activations beyond 17, 7 % below 1, 21 below 1e-3)
0.0001 / 0.0002 with the flat figure the tighter one there (9.9e-7 '256', 8.5e-7 'mfma'), and 9.5e-7 between the two shapes'
actions on the same observations.  The bound is a worst case over K roundings of one sign plus the stated absolute errors of the
nonlinearities through sum |w|, so a kernel that is right sits well below 1; the hidden tanh of the matrix-core shape away from
saturation is held by the width cases ([33], [31, 33], [33, 31], [1, 64], [33, 33] in 'mfma'), not by the tanh test.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import policy_fp64 as pf  # noqa: E402
from policy_fp64 import Spec  # noqa: E402
from test_gpu_policy import KW, features, make_net  # noqa: E402

N, SPLITS = 300, (5, 7)
T = sum(SPLITS)
# the tanh test's ladder: layer 1 of [64, 64] sees 64 inputs of +-1 through weights uniform in +-gain / 8, a pre-activation of standard
# deviation ~ 0.58 gain, so the shares beyond 17 and below 1 trade places between gain 16 and gain 32: the steps are finer there
GAINS = (4.0, 8.0, 12.0, 16.0, 24.0, 32.0, 48.0, 64.0)


@pytest.fixture(scope="module")
def vs():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import simurlacra_amd

    return simurlacra_amd


def build_net(vs, spec, in_dim, A, seed):
    net = make_net(vs, in_dim, A, list(spec.hidden), list(spec.nonlin), spec.out_nonlin, pf.OUT_GAIN, seed)
    pf.positive_relu_biases(net, spec)
    return net


def run_kernel(vs, name, net, spec, n, splits, shape, population=None):
    """the records (mode 2) of sum(splits) steps in launches of `splits` from one seeded reset, auto-reset off; population:
    (params [P, n_params], lane_set) on top of the network.  Returns (traj, handle)."""
    e = vs.VecSimEnv(name, n, **KW[name])
    e.set_auto_reset(False, seed=31)
    e.reset(seed=5)
    e.set_policy_fnn(torch.nn.utils.parameters_to_vector(net.parameters()), list(spec.hidden), list(spec.nonlin), spec.out_nonlin,
                     feat=spec.feat, obs_idx=None if spec.idx is None else list(spec.idx))
    if population is not None:
        e.set_policy_population(*population)
    e.set_policy_shape(shape)
    e.set_record_mode(2)
    e.set_traj_capacity(sum(splits))
    t = 0
    for k in splits:
        e.set_traj_offset(t)
        e.step_policy(k, record=True)
        t += k
    return e.traj(sum(splits)), e


def reference(net, spec, obs, shape):
    """the fp64 restatement (action, bound, hidden layers) and the .double() module on the recorded observations obs [T, n, O]; the
    two agree to 1e-12"""
    rows = obs.reshape(-1, obs.shape[-1])
    x, bx = pf.input_rows(rows, spec)
    assert np.array_equal(x, features(rows.astype(np.float64), None if spec.idx is None else list(spec.idx), spec.feat))
    Ws, bs = pf.net_arrays(net)
    fw = pf.forward(Ws, bs, spec, x, bx, shape)
    mod = pf.module_forward(net, spec, rows)
    pf.assert_restates(fw.act, mod)
    return fw, mod, (Ws, bs, x, bx)


def alive_rows(done):
    """[T n] bool: a lane's actions count up to its first done step (auto-reset off: behind its end a lane is frozen)"""
    alive = np.ones(done.shape, dtype=bool)
    alive[1:] = np.cumsum(done.astype(bool), axis=0)[:-1] == 0
    return alive.ravel()


def check_records(net, spec, tr, shape, label, conditions=True):
    """the recorded actions against the fp64 reference at the doubled bound and at the flat 1e-5; with `conditions` the reference's
    own: every unit live, every unit visible.  Returns (worst ratio, the restatement's Forward)."""
    fw, mod, (Ws, bs, x, bx) = reference(net, spec, tr["obs"], shape)
    got = tr["act"].reshape(mod.shape).astype(np.float64)
    alive = alive_rows(tr["done"])
    assert np.isfinite(got).all() and alive.any()
    if conditions:
        assert pf.all_units_live(fw), label
        least = pf.least_unit_effect(Ws, bs, spec, x, bx, shape, fw)
        assert least > 1.0, (label, least)
    err = np.abs(got - mod)[alive]
    ratio, ok = pf.worst_ratio(err, 2.0 * fw.bound[alive])
    flat = float((err / (1 + np.abs(mod[alive]))).max())
    print(f"\n{label}: worst ratio to the doubled bound {ratio:.4f}; max |act - ref| / (1 + |ref|) = {flat:.2e}; |ref| up to "
          f"{np.abs(mod).max():.2f}" + (f"; the least visible unit moves the action by {least:.0f} doubled bounds" if conditions else ""))
    assert ok, (label, ratio)
    assert flat < 1e-5, (label, flat)
    return ratio, fw


def same_records(a, b):
    return set(a) == set(b) and all(a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes() for k in a)


def first_live_net(vs, name, spec, in_dim, A, shape, base_seed, n=N, runs_as=None):
    """the first of at most four seeds whose REFERENCE leaves no unit of any hidden layer zero on every record of the kernel's run
    (nothing the kernel's error enters decides it); returns (net, traj, handle)"""
    for attempt in range(4):
        net = build_net(vs, spec, in_dim, A, seed=base_seed + 1000 * attempt)
        tr, e = run_kernel(vs, name, net, spec, n, SPLITS, shape)
        if pf.all_units_live(reference(net, spec, tr["obs"], runs_as or shape)[0]) or attempt == 3:
            return net, tr, e
        e.close()


def check_widths(vs, case, hidden, shape):
    name, spec, in_dim, A = pf.case_spec(case, hidden)
    assert KW[name]["max_steps"] > T
    assert (vs.env_dims(name)["O"], vs.env_dims(name)["A"]) == pf.DIMS[name]
    net, tr, e = first_live_net(vs, name, spec, in_dim, A, shape, base_seed=case)
    assert tr["obs"].shape == (T, N, pf.DIMS[name][0]) and tr["act"].shape == (T, N, A)
    assert not tr["done"].any() and e.error_count() == 0  # no lane ends: every record counts
    label = f"{name} in {in_dim} {list(hidden)} {list(spec.nonlin)} out {spec.out_nonlin} shape {shape}"
    check_records(net, spec, tr, shape, label)
    # one uncut launch of 12 steps leaves the same bits
    tr1, e1 = run_kernel(vs, name, net, spec, N, (T,), shape)
    assert same_records(tr, tr1)
    e.close()
    e1.close()


# ------------------------------------------------------------------------------------------------ 1: every width, every shape
@pytest.mark.parametrize("shape", pf.SHAPES)
@pytest.mark.parametrize("case", range(len(pf.WIDTHS)), ids=["x".join(map(str, h)) for h in pf.WIDTHS])
def test_every_width_in_every_shape(vs, case, shape):
    """both sides of every edge of the 32-unit tiles and all four (wide0, wide1) combinations; the four nonlinearities rotate over the
    hidden layers and the output (sigmoid on 1, 31, 33 and 63 units: tests/test_policy_fp64_host.py holds the table to that), the
    inputs over in_dim = 1, 7, 9, 1, 5 with one action row (QQube) and two (ball balancer)"""
    check_widths(vs, case, pf.WIDTHS[case], shape)


# ------------------------------------------------------------------------------------------------ 2: three and four hidden layers
@pytest.mark.parametrize("shape", pf.SHAPES)
@pytest.mark.parametrize("k", range(len(pf.DEEP)), ids=["x".join(map(str, h)) for h in pf.DEEP])
def test_three_and_four_hidden_layers_at_padded_widths(vs, k, shape):
    """these run the 64-env shape with 4 waves and the rolled groups of two envs whatever shape is asked (fnn_shape): every pinned shape
    is held to the 64-env shape's bound"""
    case = len(pf.WIDTHS) + k
    name, spec, in_dim, A = pf.case_spec(case, pf.DEEP[k])
    net, tr, e = first_live_net(vs, name, spec, in_dim, A, shape, base_seed=case, runs_as="64")
    assert not tr["done"].any() and e.error_count() == 0
    check_records(net, spec, tr, "64", f"{name} in {in_dim} {list(spec.hidden)} {list(spec.nonlin)} out {spec.out_nonlin} asked {shape}")
    tr1, e1 = run_kernel(vs, name, net, spec, N, (T,), shape)
    assert same_records(tr, tr1)
    if shape != "64":  # the pinned shape changes nothing
        tr2, e2 = run_kernel(vs, name, net, spec, N, SPLITS, "64")
        assert same_records(tr, tr2)
        e2.close()
    e.close()
    e1.close()


# ------------------------------------------------------------------------------------------------ 3: a population, padded width
@pytest.mark.parametrize("shape", pf.SHAPES)
def test_population_at_a_padded_width(vs, shape):
    """three parameter sets of [33, 31] (sigmoid on the 33) in one launch over 192 lanes, packed on the device by
    vs_set_policy_population: every set's lanes are held to that set's own reference.  A table that names three sets in groups of 64
    lanes runs the 64-env shape only: a pinned 256-env shape is refused by vs_step_policy, and that refusal is asserted."""
    name, n, P = "qq-su", 192, 3
    spec = Spec((33, 31), ("sigmoid", "tanh"), None, True, None)
    O, A = pf.DIMS[name]
    nets = [build_net(vs, spec, O + 1, A, seed=60 + s) for s in range(P)]
    lane_set = np.repeat(np.array([2, 0, 1]), 64).astype(np.int32)
    table = torch.stack([torch.nn.utils.parameters_to_vector(m.parameters()) for m in nets])
    if shape != "64":
        with pytest.raises(RuntimeError, match="pinned 256-env shape"):
            run_kernel(vs, name, nets[0], spec, n, SPLITS, shape, population=(table, lane_set))
        return
    tr, e = run_kernel(vs, name, nets[0], spec, n, SPLITS, shape, population=(table, lane_set))
    assert not tr["done"].any() and e.error_count() == 0
    of = lambda lanes: {k: v[:, lanes] for k, v in tr.items()}
    for s in range(P):
        lanes = np.flatnonzero(lane_set == s)
        assert len(lanes) == 64
        check_records(nets[s], spec, of(lanes), shape, f"{name} [33, 31] population set {s}")
    # the sets differ: set 1's lanes are not what set 0's parameters give
    lanes = np.flatnonzero(lane_set == 1)
    other, _, _ = reference(nets[0], spec, tr["obs"][:, lanes], shape)
    assert (np.abs(other.act - tr["act"][:, lanes].reshape(other.act.shape)) > 2.0 * other.bound).mean() > 0.5
    tr1, e1 = run_kernel(vs, name, nets[0], spec, n, (T,), shape, population=(table, lane_set))
    assert same_records(tr, tr1)
    e.close()
    e1.close()


# ------------------------------------------------------------------------------------------------ 4: the two forms of tanh
def saturation_shares(fw):
    """shares of the hidden pre-activations of a run, from the reference alone"""
    v = np.abs(np.concatenate([a.ravel() for a in fw.pre]))
    return {"beyond 17": float((v > 17).mean()), "below 1": float((v < 1).mean()), "below 1e-3 (count)": int((v < 1e-3).sum())}


def test_tanh_forms_against_fp64(vs):
    """[64, 64] tanh with the hidden weights times a gain: tanh_fast ((1 - t) / (1 + t), t = exp(-2 |x|)) in the '256' shape and the
    matrix-core shape's 1 - 2 / (1 + exp(2 x)) on the same network and initial state, both held to the bound with tanh_fast's stated
    2e-7.  The gain is the smallest of GAINS at which the REFERENCE's pre-activations, on the records of that gain's run, lie beyond 17
    and below 1 in shares of at least 5 % each (nothing the kernel's error enters decides it); some lie below 1e-3 as well.  The
    bound takes tanh's largest slope, so far in the tails it is loose and the flat 1e-5 is the tighter figure: every unit is live,
    but a saturated unit's visibility is not asserted here."""
    name = "qq-su"
    O, A = pf.DIMS[name]
    spec = Spec((64, 64), ("tanh", "tanh"), None, False, None)
    ok = lambda s: s["beyond 17"] >= 0.05 and s["below 1"] >= 0.05 and s["below 1e-3 (count)"] > 0
    for gain in GAINS:
        net = build_net(vs, spec, O, A, seed=7)
        with torch.no_grad():
            for m in net.hidden_layers:
                m.weight.mul_(gain)
        tr, e = run_kernel(vs, name, net, spec, N, SPLITS, "256")
        shares = saturation_shares(reference(net, spec, tr["obs"], "256")[0])
        if ok(shares) or gain == GAINS[-1]:
            break
        e.close()
    acts = {}
    for shape in ("256", "mfma"):
        if shape != "256":
            e.close()
            tr, e = run_kernel(vs, name, net, spec, N, SPLITS, shape)
        assert not tr["done"].any() and e.error_count() == 0
        _, fw = check_records(net, spec, tr, shape, f"{name} [64, 64] tanh, hidden weights x {gain}, shape {shape}", conditions=False)
        shares = saturation_shares(fw)
        print("    shares of the pre-activations: " + ", ".join(f"{k} {v:.4g}" for k, v in shares.items()))
        assert ok(shares)
        assert pf.all_units_live(fw)
        acts[shape] = tr["act"]
    e.close()
    diff = np.abs(acts["256"].astype(np.float64) - acts["mfma"])
    print(f"    largest difference between the two shapes' actions: first step (same observations) {diff[0].max():.2e}, all steps {diff.max():.2e}")
