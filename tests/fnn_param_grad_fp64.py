"""
The fp64 reference of vs_fnn_param_grad (param_grad_fp64), its first-order error bound (error_bound), the table of the tests' networks
and their dense cotangents.  Not a test module: import it by bare name.  test_fnn_param_grad_host holds the reference to
torch.autograd.grad of the .double() module (torch_module) at 1e-12 for every case of the table: featurisation, obs_idx and the torch
order of the flat vector are pinned without a device.
"""
import numpy as np

import closed_loop_cases as clc

U = 2.0 ** -24                                   # unit roundoff of fp32
EPS_ACT = {"tanh": 2e-7, "sigmoid": 4e-7, "relu": 0.0, None: 0.0}  # absolute error of the kernel's activation functions (see error_bound)
EPS_SINCOS = 4e-7                                # sincos_fast's stated absolute error

# case -> (family, hidden sizes, hidden nonlinearities, output nonlinearity, feat, obs_idx): the table of the GPU test
TABLE = {
    "omo-1-relu": ("omo", (1,), ("relu",), None, False, None),
    "omo-63x7-relu": ("omo", (63, 7), ("relu", "relu"), None, False, None),
    "qq-su-16": ("qq-su", (16,), ("tanh",), None, False, None),
    "qq-su-64x64-feat": ("qq-su", (64, 64), ("tanh", "tanh"), None, True, None),
    "qcp-su-32x33": ("qcp-su", (32, 33), ("tanh", "sigmoid"), None, False, None),
    "qbb-31x64-tanh-out": ("qbb", (31, 64), ("tanh", "tanh"), "tanh", False, None),
    "pend-view-8-sigmoid": ("pend", (8,), ("sigmoid",), None, False, (2, 0)),
    "pend-8": ("pend", (8,), ("tanh",), None, False, None),
}
# the cases of the GPU test's table: pend-8 is the network of its noise test and of the one-workspace tests, not a table case
GPU_TABLE = [k for k in TABLE if k != "pend-8"]
FUNCS = {"tanh": np.tanh, "relu": lambda z: np.maximum(z, 0.0), "sigmoid": lambda z: 1.0 / (1.0 + np.exp(-z)), None: lambda z: z}
# derivative from the VALUE y = f(z), as the kernel takes it, and |d f' / d y|
GRADS = {"tanh": lambda y: 1.0 - y * y, "relu": lambda y: (y > 0.0).astype(np.float64), "sigmoid": lambda y: y * (1.0 - y),
         None: lambda y: np.ones_like(y)}
GRAD_SLOPES = {"tanh": lambda y: 2.0 * np.abs(y), "relu": lambda y: np.zeros_like(y), "sigmoid": lambda y: np.abs(1.0 - 2.0 * y),
               None: lambda y: np.zeros_like(y)}


# ------------------------------------------------------------------------------------------------- the fp64 reference
def net_input(net, ob):
    x = ob if net["obs_idx"] is None else ob[:, list(net["obs_idx"])]
    if net["feat"]:
        x = np.concatenate([x[:, 0:1], np.sin(x[:, 1:2]), np.cos(x[:, 1:2]), x[:, 2:]], axis=1)
    return x


def flat_of(dW, db):
    """torch's order: per Linear weight [out, in], then bias"""
    return np.concatenate([np.concatenate([W.reshape(-1), b]) for W, b in zip(dW, db)])


def param_grad_fp64(net, obs, abar, inside, chains=None):
    """The sum the kernel computes, restated in fp64: obs [R, O] recorded observations, abar [R, A], inside [R] bool (t < L of the
    row's lane).  net: W [out, in] and b per layer (hidden .., output), hidden_nonlin, output_nonlin, feat, obs_idx.
    Returns (flat gradient, flat sum over the rows of |term|, hidden pre-activations [[R', h]]) over the rows inside, in torch's order;
    with chains = dict(acc=.., wg=..) also the first-order error bound of error_bound()."""
    W = [w.astype(np.float64) for w in net["W"]]
    b = [v.astype(np.float64) for v in net["b"]]
    kinds = list(net["hidden_nonlin"]) + [net["output_nonlin"]]
    rows = np.flatnonzero(inside)
    ab = abar[rows].astype(np.float64)
    ys, zs = [net_input(net, obs[rows].astype(np.float64))], []
    for l, kind in enumerate(kinds):
        zs.append(ys[-1] @ W[l].T + b[l])
        ys.append(FUNCS[kind](zs[-1]))
    deltas = [None] * len(kinds)
    deltas[-1] = ab * GRADS[kinds[-1]](ys[-1])
    for l in range(len(kinds) - 2, -1, -1):
        deltas[l] = (deltas[l + 1] @ W[l + 1]) * GRADS[kinds[l]](ys[l + 1])
    dW = [deltas[l].T @ ys[l] for l in range(len(kinds))]
    db = [deltas[l].sum(axis=0) for l in range(len(kinds))]
    aW = [np.abs(deltas[l]).T @ np.abs(ys[l]) for l in range(len(kinds))]
    abs_b = [np.abs(deltas[l]).sum(axis=0) for l in range(len(kinds))]
    out = [flat_of(dW, db), flat_of(aW, abs_b), zs[:-1]]
    if chains is not None:
        out.append(error_bound(net, W, b, kinds, ys, ab, deltas, aW, abs_b, chains))
    return tuple(out)


def error_bound(net, W, b, kinds, ys, ab, deltas, aW, abs_b, chains):
    """First-order bound of |kernel - fp64| per parameter (flat, torch's order); u = 2^-24, gamma(m) = m u.

    Every quantity of a row carries an absolute error bound e(.) through the very chains k_fnn_param_grad runs:
      x      the recorded observation is exact; under feat the sine and cosine rows carry sincos_fast's 4e-7.
      z_1    b + 12 FMAs in sequence (the padded row):      e = gamma(12) (|b| + |W||x|) + |W| e(x)
      z_2    fnn_row_dot: four partial sums of 16 FMAs, two levels of adds, the bias: gamma(19) (..) + |W| e(y_1)
      z_out  a product, six DPP add levels, the bias:       gamma(8) (|b| + |W||y|) + |W| e(y)
      y      e = eps_f + |f'| e(z): tanh_fast's stated 2e-7; 0 for relu (no unit within 1e-3 of 0: asserted by the caller) and none;
             sigmoid 4e-7: v_exp_f32 and v_rcp_f32 are 1 ulp each and the argument's rounding adds |z| log2(e) u relative to the
             exponential, so with |z| <= 8 (asserted by the caller) y^2 t (2 + 12 + 1) u + 2 u y <= 0.25 x 15 u + 2 u < 6 u = 3.6e-7.
      f'(y)  from the value, one or two roundings:          e = |d f' / d y| e(y) + 2 u |f'|
      delta_out = abar f'(y_out):                           e = |abar| e(f') + u |delta_out|
      W^T delta: A FMAs (output layer) or fnn_row_dot's 19: e = gamma(.) |W|^T |delta| + |W|^T e(delta)
      delta_l = (W^T delta) f'(y_l):                        e = |f'| e(W^T delta) + |W^T delta| e(f') + u |delta_l|
    A term delta_j y_k then errs by |delta| e(y) + |y| e(delta), and the sum of the terms -- one FMA per row in a wave's register
    (chains['acc'] rows at most), three adds across the waves, chains['wg'] adds across the workgroups' partial sums, one more
    under accumulate -- by gamma(acc + 3 + wg + 1) sum |term|."""
    g = lambda m: m * U  # noqa: E731
    n_l = len(kinds)
    absW = [np.abs(w) for w in W]
    ey = [np.zeros_like(ys[0])]
    if net["feat"]:
        ey[0][:, 1:3] = EPS_SINCOS
    fwd_chain = [12] + [19] * (n_l - 2) + [8]
    for l, kind in enumerate(kinds):
        ez = g(fwd_chain[l]) * (np.abs(b[l]) + np.abs(ys[l]) @ absW[l].T) + ey[l] @ absW[l].T
        ey.append(EPS_ACT[kind] + np.abs(GRADS[kind](ys[l + 1])) * ez)
    efp = [GRAD_SLOPES[kinds[l]](ys[l + 1]) * ey[l + 1] + 2.0 * U * np.abs(GRADS[kinds[l]](ys[l + 1])) for l in range(n_l)]
    ed = [None] * n_l
    ed[-1] = np.abs(ab) * efp[-1] + U * np.abs(deltas[-1])
    for l in range(n_l - 2, -1, -1):
        chain = W[l + 1].shape[0] if l == n_l - 2 else 19
        pre = deltas[l + 1] @ W[l + 1]
        epre = g(chain) * (np.abs(deltas[l + 1]) @ absW[l + 1]) + ed[l + 1] @ absW[l + 1]
        ed[l] = np.abs(GRADS[kinds[l]](ys[l + 1])) * epre + np.abs(pre) * efp[l] + U * np.abs(deltas[l])
    total = g(chains["acc"] + 3 + chains["wg"] + 1)
    eW = [np.abs(deltas[l]).T @ ey[l] + ed[l].T @ np.abs(ys[l]) + total * aW[l] for l in range(n_l)]
    eb = [ed[l].sum(axis=0) + total * abs_b[l] for l in range(n_l)]
    return flat_of(eW, eb)


def random_net(key, rng, O, A):
    """float32 weights of the case's shape, scaled so that no unit saturates on unit-sized observations"""
    _, hidden, hidden_nonlin, output_nonlin, feat, obs_idx = TABLE[key]
    n_in = (O if obs_idx is None else len(obs_idx)) + (1 if feat else 0)
    sizes = (n_in,) + tuple(hidden) + (A,)
    return dict(W=[(rng.normal(size=(o, i)) / np.sqrt(i)).astype(np.float32) for i, o in zip(sizes[:-1], sizes[1:])],
                b=[(0.5 * rng.normal(size=o)).astype(np.float32) for o in sizes[1:]], hidden=tuple(hidden),
                hidden_nonlin=hidden_nonlin, output_nonlin=output_nonlin, feat=feat, obs_idx=obs_idx)


def torch_module(net):
    """the .double() torch restatement of the network: Linear layers in parameters_to_vector's order"""
    import torch

    layers = torch.nn.ModuleList([torch.nn.Linear(W.shape[1], W.shape[0]) for W in net["W"]]).double()
    with torch.no_grad():
        for lin, W, b in zip(layers, net["W"], net["b"]):
            lin.weight.copy_(torch.as_tensor(W.astype(np.float64)))
            lin.bias.copy_(torch.as_tensor(b.astype(np.float64)))
    acts = {"tanh": torch.tanh, "relu": torch.relu, "sigmoid": torch.sigmoid, None: lambda z: z}

    def forward(ob):
        x = ob if net["obs_idx"] is None else ob[:, list(net["obs_idx"])]
        if net["feat"]:
            x = torch.cat([x[:, 0:1], torch.sin(x[:, 1:2]), torch.cos(x[:, 1:2]), x[:, 2:]], dim=1)
        for l, lin in enumerate(layers):
            x = acts[(list(net["hidden_nonlin"]) + [net["output_nonlin"]])[l]](lin(x))
        return x

    return layers, forward


def abar_of(key, n, t, seed=0):
    """[n, t, A] float32, dense and standard normal: the cotangents the GPU test feeds directly"""
    A = clc.case(key)["ref"].A
    return np.random.default_rng(1000 + seed).normal(size=(n, t, A)).astype(np.float32)
