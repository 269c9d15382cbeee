"""
The reference and the bound of tests/test_gpu_policy_fp64.py (tests/policy_fp64.py) without a device, on observations drawn by NumPy:
  * the fp64 restatement is the .double() module (1e-12) at every width of the GPU test, in every featurisation it rotates over;
  * torch's own fp32 forward -- a correct fp32 evaluation in another summation order -- lies inside the doubled bound of every
    evaluation shape: the bound is not unreachably tight;
  * three wrong networks lie outside it: one hidden unit dropped, a padding unit's next-layer weight set to 1 under sigmoid, the two
    32-unit tiles of a 33-wide layer swapped: the bound is not vacuous.
"""
import numpy as np
import pytest

import policy_fp64 as pf

torch = pytest.importorskip("torch")

NL = {"tanh": torch.tanh, "relu": torch.relu, "sigmoid": torch.sigmoid, None: None}
ROWS = 600


def make_case(case, hidden, nonlin=None, out_nonlin=None):
    """the first of at most four seeds whose reference leaves no unit dead on the observations (as the GPU test picks its seed)"""
    for attempt in range(4):
        net, spec, obs = make_net(case, hidden, nonlin, out_nonlin, seed=case + 1000 * attempt)
        if pf.all_units_live(pf.forward(*pf.net_arrays(net), spec, *pf.input_rows(obs, spec), "64")):
            break
    return net, spec, obs


def make_net(case, hidden, nonlin, out_nonlin, seed):
    from simurlacra_amd.policies import FNN

    name, spec, in_dim, A = pf.case_spec(case, hidden)
    if nonlin is not None:
        spec = spec._replace(nonlin=tuple(nonlin), out_nonlin=out_nonlin)
    torch.manual_seed(seed)
    net = FNN(in_dim, A, list(hidden), [NL[f] for f in spec.nonlin], output_nonlin=NL[spec.out_nonlin])
    with torch.no_grad():
        net.output_layer.weight.mul_(pf.OUT_GAIN)
    pf.positive_relu_biases(net, spec)
    obs = np.random.default_rng(100 + case).uniform(-1.5, 1.5, (ROWS, pf.DIMS[name][0])).astype(np.float32)
    return net, spec, obs


ALL = list(pf.WIDTHS) + list(pf.DEEP)
IDS = ["x".join(map(str, h)) for h in ALL]


def shapes_of(hidden):
    return pf.SHAPES if len(hidden) <= 2 else ("64",)


@pytest.mark.parametrize("case", range(len(ALL)), ids=IDS)
def test_restatement_is_the_double_module(case):
    net, spec, obs = make_case(case, ALL[case])
    Ws, bs = pf.net_arrays(net)
    x, bx = pf.input_rows(obs, spec)
    assert x.shape[1] == Ws[0].shape[1] and [W.shape[0] for W in Ws[:-1]] == list(spec.hidden)
    mod = pf.module_forward(net, spec, obs)
    for shape in shapes_of(spec.hidden):
        pf.assert_restates(pf.forward(Ws, bs, spec, x, bx, shape).act, mod)
    # the kernel's zero-padded layout is the same network
    Wp, bp = pf.padded(Ws, bs)
    assert np.abs(pf.forward(Wp, bp, spec, x, bx, "64").act - mod).max() <= 1e-12 * (1 + np.abs(mod).max())


@pytest.mark.parametrize("case", range(len(ALL)), ids=IDS)
def test_torch_fp32_lies_inside_the_doubled_bound(case):
    net, spec, obs = make_case(case, ALL[case])
    Ws, bs = pf.net_arrays(net)
    x, bx = pf.input_rows(obs, spec)
    with torch.no_grad():
        x32 = torch.from_numpy(obs if spec.idx is None else obs[:, list(spec.idx)])
        if spec.feat:
            x32 = torch.cat([x32[:, 0:1], torch.sin(x32[:, 1:2]), torch.cos(x32[:, 1:2]), x32[:, 2:]], dim=1)
        got = net(x32).numpy().astype(np.float64)
    for shape in shapes_of(spec.hidden):
        fw = pf.forward(Ws, bs, spec, x, bx, shape)
        ratio, ok = pf.worst_ratio(np.abs(got - fw.act), 2.0 * fw.bound)
        print(f"{spec.hidden} {spec.nonlin} out {spec.out_nonlin} shape {shape}: torch fp32 at {ratio:.3f} of the doubled bound")
        assert ok, (shape, ratio)


@pytest.mark.parametrize("case", range(len(ALL)), ids=IDS)
def test_a_dropped_unit_leaves_the_doubled_bound(case):
    net, spec, obs = make_case(case, ALL[case])
    Ws, bs = pf.net_arrays(net)
    x, bx = pf.input_rows(obs, spec)
    for shape in shapes_of(spec.hidden):
        fw = pf.forward(Ws, bs, spec, x, bx, shape)
        assert pf.all_units_live(fw)
        least = pf.least_unit_effect(Ws, bs, spec, x, bx, shape, fw)
        print(f"{spec.hidden} shape {shape}: the least visible unit moves the action by {least:.1f} doubled bounds")
        assert least > 1.0, (shape, least)


def outside(ref, bound, mutant):
    """a mutant is caught where some entry leaves the doubled bound"""
    return bool((np.abs(mutant - ref) > 2.0 * bound).any())


@pytest.mark.parametrize("hidden,layer", [([33], 0), ([33, 31], 0), ([31, 33], 1), ([63, 63], 0), ([63, 63], 1)],
                         ids=["33", "33x31-first", "31x33-second", "63x63-first", "63x63-second"])
def test_a_live_padding_unit_under_sigmoid_leaves_the_doubled_bound(hidden, layer):
    """in the kernel's layout a sigmoid layer's padding units are 0.5; with a weight of 1 behind the first of them (instead of the
    packed 0) the action moves by far more than the bound"""
    nonlin = ["tanh"] * len(hidden)
    nonlin[layer] = "sigmoid"
    net, spec, obs = make_case(1, hidden, nonlin, None)
    Ws, bs = pf.net_arrays(net)
    x, bx = pf.input_rows(obs, spec)
    Wp, bp = pf.padded(Ws, bs)
    pad = hidden[layer]
    assert pad < pf.FNN_W and not Wp[layer + 1][:, pad].any() and not Wp[layer][pad].any() and bp[layer][pad] == 0.0
    for shape in pf.SHAPES:
        fw = pf.forward(Wp, bp, spec, x, bx, shape)
        assert (fw.hid[layer][:, pad] == 0.5).all()
        pf.assert_restates(fw.act, pf.module_forward(net, spec, obs))
        Wm = [W.copy() for W in Wp]
        Wm[layer + 1][0, pad] = 1.0
        assert outside(fw.act, fw.bound, pf.forward(Wm, bp, spec, x, bx, shape).act)


@pytest.mark.parametrize("hidden,layer", [([33], 0), ([33, 31], 0), ([31, 33], 1), ([33, 33], 0)],
                         ids=["33", "33x31-first", "31x33-second", "33x33-first"])
def test_swapped_tiles_leave_the_doubled_bound(hidden, layer):
    """units 0 .. 31 and 32 .. 63 of a 33-wide layer handed to the next layer in each other's place"""
    net, spec, obs = make_case(2, hidden)
    Ws, bs = pf.net_arrays(net)
    x, bx = pf.input_rows(obs, spec)
    Wp, bp = pf.padded(Ws, bs)
    swap = np.r_[32:64, 0:32]
    for shape in pf.SHAPES:
        fw = pf.forward(Wp, bp, spec, x, bx, shape)
        mutant = pf.forward(Wp, bp, spec, None, None, shape, start=layer + 1, h=fw.hid[layer][:, swap], hb=fw.hidb[layer][:, swap]).act
        assert outside(fw.act, fw.bound, mutant)


def test_the_rotation_puts_sigmoid_where_the_padding_is_live():
    """what the GPU test's case table promises, from the table alone"""
    sig = [(w, l, len(h)) for c, h in enumerate(pf.WIDTHS) for l, w in enumerate(h) if pf.rotated_nonlins(c, len(h))[0][l] == "sigmoid"]
    assert any(33 <= w <= 63 for w, _, _ in sig) and any(w < 32 for w, _, _ in sig)
    assert any(33 <= w <= 63 and l == n - 1 for w, l, n in sig)      # ... in front of the output layer
    assert any(33 <= w <= 63 and l == 0 and n == 2 for w, l, n in sig)  # ... and in front of a hidden layer
    kinds = {k for c, h in enumerate(pf.WIDTHS) for k in pf.rotated_nonlins(c, len(h))[0]}
    outs = {pf.rotated_nonlins(c, len(h))[1] for c, h in enumerate(pf.WIDTHS)}
    assert kinds == set(pf.NONLINS) and outs == set(pf.NONLINS)
    first, second = {h[0] > 32 for h in pf.WIDTHS}, {(h[0] > 32, h[1] > 32) for h in pf.WIDTHS if len(h) == 2}
    assert first == {False, True} and len(second) == 4
    assert sorted({pf.case_spec(c, h)[2] for c, h in enumerate(pf.WIDTHS)}) == [1, 5, 7, 9]
    assert {pf.case_spec(c, h)[3] for c, h in enumerate(pf.WIDTHS)} == {1, 2}
    assert [pf.roundings("mfma", 1, d)[0] for d in (1, 2, 7, 9)] == [2, 2, 8, 10] and pf.roundings("256", 2, 9) == [12, 64, 8]
