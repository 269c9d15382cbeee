"""
What tests/test_gpu_policy_fp64.py (on the device) and tests/test_policy_fp64_host.py (without one) share: the fp64 NumPy restatement
of the feed-forward policy network that k_rollout_fnn evaluates, and the first-order bound of the kernel's fp32 error that is built
from the restatement's magnitude sums.  Not a test module: import it by bare name.

The network.  x = the visible observation rows (obs_idx), with `feat` [o_0, sin o_1, cos o_1, o_2 ..]; per hidden layer
h = f(W h_prev + b), f one of tanh / sigmoid / relu / identity; action = g(W_out h + b_out).  Weights as torch keeps them, [out, in].

The bound.  u = 2^-24.  A pre-activation v = sum_k w_k x_k + b that the kernel builds with m roundings, every partial sum of which is
at most sum |w_k x_k| + |b| in size, from inputs x_k that are themselves off by at most B(x_k), is off by at most (first order)

    B(v) = m u (sum |w_k x_k| + |b|) + sum |w_k| B(x_k),        m = K + c below.

m per layer and evaluation shape, read from k_rollout_fnn (vecsim_kernels.h):
  * layer 0, vector ALU ('64', '256'): acc = b, then `for k < FNN_XS: acc = fmaf(w1[k], x[k], acc)`: K = FNN_XS = 12 fused multiply-adds
    of one rounding each (the bias is the start value: c = 0).  The steps behind in_dim add an exact 0; 12 is what the code runs.
  * layer 0, matrix cores ('mfma'): the accumulator starts at b; one v_mfma_f32_32x32x2_f32 per kk with 2 kk < in_dim, i.e.
    ceil(in_dim / 2) steps of two products each.  No guide this project follows states how the fp32 MFMA rounds inside a step, so a
    step counts as two roundings: K = 2 ceil(in_dim / 2), c = 0.
  * hidden to hidden, vector ALU: acc = b, then 64 FMAs over the zero-padded row of 64 inputs: K = 64, c = 0.
  * hidden to hidden, matrix cores: the accumulator starts at b; 16 K-steps per 32-unit tile of the previous layer, two tiles, two
    products per step: K = 64, c = 0 (a narrow previous layer skips its second tile; 64 is the most the code runs).
  * output, vector ALU: one product wo * h per lane (1), six DPP additions of wave_sum_to_lane63 on the way to lane 63 (6), then
    `l_a + bo` in the env wave (c = 1): K + c = 8.
  * output, matrix cores: part = 0, then 32 FMAs per half-wave (two tiles of 16 accumulator registers), `part + other` for the two
    half-waves and `+ bo`: K = 32, c = 2.
The nonlinearities, f(v) off by at most:
  * tanh: B(v) + 2e-7 -- Lipschitz constant 1 and the absolute error tanh_fast's comment states.  The matrix-core shape evaluates
    1 - 2 / (1 + exp2(..)) instead; the same figure is used for it.
  * sigmoid: sigmoid_bound of tests/test_gpu_recurrent_policy_fp64.py, restated here (a test module marked gpu is not imported by a
    host test): Lipschitz constant 1 / 4, 2 ulp (fp32) of the result for v_exp_f32 and v_rcp_f32, 2 |v| u s (1 - s) for the rounding
    of the scaled argument, 2^-126 for a flushed sub-normal result.
  * relu, identity: B(v) (Lipschitz constant 1, exact).
With `feat` the sine and cosine inputs carry B(x) = 4e-7, sincos_fast's bound asserted in test_fast_sincos_accuracy_through_observe; every
other input is the recorded fp32 observation itself: B(x) = 0.
Everything is first order; the caller doubles the bound, and that factor 2 is the only margin.
"""
import copy
from typing import NamedTuple, Optional, Tuple

import numpy as np

U = 2.0 ** -24
TANH_ABS = 2e-7      # tanh_fast's stated absolute error
SINCOS_ABS = 4e-7    # sincos_fast's asserted absolute error
FLUSH = 2.0 ** -126  # the smallest normal fp32: what a flushed sub-normal result is off by at most
FNN_XS, FNN_W = 12, 64  # the kernel's padded input row and padded layer width
SHAPES = ("64", "256", "mfma")
NONLINS = ("tanh", "sigmoid", "relu", None)

# the widths at which the padding of k_rollout_fnn is live: both sides of every edge of the 32-unit matrix-core tiles and all four
# (first layer wide, second layer wide) combinations -- and the deeper networks, which run the 64-env vector-ALU shape only
WIDTHS = ([1], [31], [32], [33], [63], [1, 1], [31, 33], [33, 31], [32, 64], [64, 1], [1, 64], [33, 33], [63, 63])
DEEP = ([1, 63, 2], [33, 5, 64, 3])
# the gain on the output weights (make_net of test_gpu_policy.py).  1: a larger one saturates a tanh or sigmoid output behind a relu
# layer, and there the bound, which takes the nonlinearity's largest slope, no longer tells a dropped unit from rounding
OUT_GAIN = 1.0


class Spec(NamedTuple):
    """a network as the kernel's setter takes it"""
    hidden: Tuple[int, ...]
    nonlin: Tuple[Optional[str], ...]  # one per hidden layer
    out_nonlin: Optional[str]
    feat: bool
    idx: Optional[Tuple[int, ...]]     # the visible observation rows; None: all of them


# what the policy sees, rotated over the cases (family, visible rows, featurisation): in_dim = 1 (one visible row), odd in_dim (7, 5: the
# first layer's K loop takes the inputs two at a time) and 9, the largest the setter accepts (all 8 rows of the ball balancer and the
# featurisation); the QQube has one action row, the ball balancer two
INPUTS = (("qq-su", (5,), False), ("qq-su", None, True), ("qbb", None, True), ("qbb", (2,), False), ("qbb", (0, 2, 5, 7), True))
DIMS = {"qq-su": (6, 1), "qbb": (8, 2)}  # (observation rows, action rows): the GPU test holds env_dims to it


def rotated_nonlins(case, n_hidden):
    """the four nonlinearities rotated over the cases: hidden layer l of case c takes NONLINS[(c + l + 1) % 4], the output
    NONLINS[(c + 3) % 4]"""
    return tuple(NONLINS[(case + l + 1) % 4] for l in range(n_hidden)), NONLINS[(case + 3) % 4]


def case_spec(case, hidden):
    """(family, Spec, in_dim, action rows) of case number `case` with the given hidden sizes"""
    name, idx, feat = INPUTS[case % len(INPUTS)]
    nonlin, out_nonlin = rotated_nonlins(case, len(hidden))
    O, A = DIMS[name]
    return name, Spec(tuple(hidden), nonlin, out_nonlin, feat, idx), (O if idx is None else len(idx)) + int(feat), A


# ------------------------------------------------------------------------------------------------ the reference
def sigmoid(v):
    """fp64, accurate in both tails (no 1 - tanh cancellation)"""
    with np.errstate(over="ignore"):
        e = np.exp(-np.abs(v))
    return np.where(v >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def sigmoid_bound(v, bv):
    s = sigmoid(v)
    ulp = np.spacing(s.astype(np.float32)).astype(np.float64)
    return 0.25 * bv + 2.0 * ulp + 2.0 * np.abs(v) * U * s * sigmoid(-v) + FLUSH


def apply_nonlin(kind, v, bv):
    """(f(v), its bound)"""
    if kind == "tanh":
        return np.tanh(v), bv + TANH_ABS
    if kind == "sigmoid":
        return sigmoid(v), sigmoid_bound(v, bv)
    if kind == "relu":
        return np.maximum(v, 0.0), bv
    assert kind is None, kind
    return v, bv


def input_rows(obs, spec):
    """the policy's input of the fp32 observations obs [R, O] in fp64, and the bound of what the kernel makes of it"""
    x = obs.astype(np.float64)
    if spec.idx is not None:
        x = x[:, list(spec.idx)]
    bx = np.zeros(x.shape)
    if spec.feat:
        x = np.concatenate([x[:, 0:1], np.sin(x[:, 1:2]), np.cos(x[:, 1:2]), x[:, 2:]], axis=1)
        bx = np.zeros(x.shape)
        bx[:, 1:3] = SINCOS_ABS
    return x, bx


def net_arrays(net):
    """([W_l [out, in]], [b_l]) of an FNN in fp64, hidden layers first, the output layer last"""
    f64 = lambda p: p.detach().double().numpy().copy()
    layers = list(net.hidden_layers) + [net.output_layer]
    return [f64(m.weight) for m in layers], [f64(m.bias) for m in layers]


def roundings(shape, n_hidden, in_dim):
    """m = K + c of every layer (hidden layers, then the output layer) in an evaluation shape: see the module docstring"""
    assert shape in SHAPES
    mf = shape == "mfma"
    assert not mf or n_hidden <= 2
    first = 2 * ((in_dim + 1) // 2) if mf else FNN_XS
    return [first] + [FNN_W] * (n_hidden - 1) + [32 + 2 if mf else 1 + 6 + 1]


class Forward(NamedTuple):
    act: np.ndarray     # [R, A]
    bound: np.ndarray   # [R, A] first order: the caller doubles it
    pre: list           # pre-activation of every hidden layer [R, width]
    hid: list           # activation of every hidden layer [R, width]
    hidb: list          # ... and its first-order bound


def forward(Ws, bs, spec, x, bx, shape, start=0, h=None, hb=None):
    """The network in fp64 on the input rows x [R, in_dim] with bounds bx, and the first-order bound of the kernel's action in `shape`.
    start > 0: from the given activations h (bounds hb) of hidden layer start - 1 on."""
    kinds = list(spec.nonlin) + [spec.out_nonlin]
    m = roundings(shape, len(spec.nonlin), Ws[0].shape[1])
    pre, hid, hidb = [], [], []
    if start == 0:
        h, hb = x, bx
    for l in range(start, len(kinds)):
        W, b = Ws[l], bs[l]
        v = h @ W.T + b
        bv = m[l] * U * (np.abs(h) @ np.abs(W).T + np.abs(b)) + hb @ np.abs(W).T
        h, hb = apply_nonlin(kinds[l], v, bv)
        if l < len(kinds) - 1:
            pre.append(v)
            hid.append(h)
            hidb.append(hb)
    return Forward(h, hb, pre, hid, hidb)


def module_forward(net, spec, obs):
    """copy.deepcopy(net).double() on the featurised observations: the reference itself"""
    import torch

    x, _ = input_rows(obs, spec)
    with torch.no_grad():
        out = copy.deepcopy(net).double()(torch.from_numpy(x)).numpy()
    assert out.dtype == np.float64
    return out


def assert_restates(ref, mod):
    assert ref.shape == mod.shape and (np.abs(ref - mod) <= 1e-12 * (1 + np.abs(mod))).all(), float(np.abs(ref - mod).max())


# ------------------------------------------------------------------------------------------------ the conditions on a case
def all_units_live(fw):
    """no dead layer, no dead unit: every unit of every hidden layer is non-zero on some row"""
    return all(bool((np.abs(h).max(axis=0) > 0).all()) for h in fw.hid)


def least_unit_effect(Ws, bs, spec, x, bx, shape, fw=None):
    """Zero one hidden unit at a time: the smallest, over the units of all hidden layers, of the largest over rows and action entries
    of |action change| / doubled bound.  Above 1: a kernel that dropped any single unit would leave the doubled bound somewhere."""
    fw = forward(Ws, bs, spec, x, bx, shape) if fw is None else fw
    least = np.inf
    for l, h in enumerate(fw.hid):
        for k in range(h.shape[1]):
            cut = h.copy()
            cut[:, k] = 0.0
            act = forward(Ws, bs, spec, None, None, shape, start=l + 1, h=cut, hb=fw.hidb[l]).act
            least = min(least, float((np.abs(act - fw.act) / (2.0 * fw.bound)).max()))
    return least


def positive_relu_biases(net, spec):
    """A relu layer (the output included) gets the biases |b_j| + sum_k |w_jk| / 2.  With |b_j| alone a unit whose weights are mostly
    negative is dead on every row behind a sigmoid layer, whose outputs are all near 0.5; half the weight mass in front of the unit
    outweighs that, and the unit still goes to zero where its inputs are large."""
    import torch

    layers = list(net.hidden_layers) + [net.output_layer]
    with torch.no_grad():
        for m, kind in zip(layers, list(spec.nonlin) + [spec.out_nonlin]):
            if kind == "relu":
                m.bias.copy_(m.bias.abs() + 0.5 * m.weight.abs().sum(dim=1))


def worst_ratio(err, bound):
    """(largest err / bound over the entries with a positive bound, whether every entry is within its bound)"""
    pos = bound > 0
    ratio = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    return ratio, bool((err <= bound).all())


# ------------------------------------------------------------------------------------------------ the kernel's padded layout
def padded(Ws, bs):
    """the network as the kernel holds it: every hidden layer 64 units wide, the rows, columns and biases of the padding zero.  Under
    sigmoid a padding unit is 0.5, and only the zero weight behind it keeps it out of the next layer."""
    Wp, bp = [], []
    for l, (W, b) in enumerate(zip(Ws, bs)):
        last = l == len(Ws) - 1
        P = np.zeros((W.shape[0] if last else FNN_W, W.shape[1] if l == 0 else FNN_W))
        P[:W.shape[0], :W.shape[1]] = W
        q = np.zeros(P.shape[0])
        q[:b.size] = b
        Wp.append(P)
        bp.append(q)
    return Wp, bp
