"""
The fp64 reference of vs_rnn_param_grad and its first-order error bound, and the synthetic rows the host test and the digest tool run
it on (TABLE, ROWS, rows_case).  Not a test module: import it by bare name.

param_grad_fp64 restates in NumPy fp64
    d_params[q] = sum over the rows (t < L_i, i < n) of (d F / d theta_q)(x_t, p_t)^T (abar_t, d_hid_t)
for the four cells (Elman tanh / relu, GRU, LSTM; torch's gate order) and one or two layers, on rows the caller hands over: x [R, in]
(what the policy saw), p [R, Hs] (h of layer 0, 1, .. then the LSTM's c), abar [R, A], d_hid [R, Hs], inside [R].  It returns the flat
gradient in parameters_to_vector's order, per parameter the sum of the magnitudes of its terms, the bound, and the largest gate
pre-activation (with a relu cell's distance from the kink).  test_rnn_param_grad_host holds it to torch.autograd.grad of the .double() modules at 1e-12.

The bound, per parameter q whose terms are delta y (delta: a gate's delta or delta_out; y: an input, a hidden state, h'_top or 1):
    bound_q = sum_rows (|delta| e(y) + |y| e(delta)) + gamma(acc + wg) sum_rows |delta y|,        gamma(m) = m 2^-24,  u = 2^-24
a first-order bound: every e(.) below is propagated through the fp64 reference's own values, products of errors are dropped (the tests
double the bound for them, the factor test_gpu_policy_fp64.py uses).  The chains are those k_rnn_param_grad runs:
  * x_t, p_t, abar_t and d_hid_t are read, not computed: e = 0.
  * a gate's pre-activation is rnn_unit_act's: one FMA chain over the `in` inputs (RNN_XP = 8 in layer 0, hp in layer 1), one over the hp
    state entries, then (ai + bi) + (ah + bh): e(s) = gamma(in + hp + 3) (sum |w| |v| + |b_ih| + |b_hh|) + sum |w| e(v).  The GRU's n
    gate adds r (W_hn h + b_hn): one product, one more add, and |hn| e(r).
  * tanh_fast: 2e-7 + (1 - y^2) e(s); the v_rcp_f32 sigmoid: 4e-7 + y (1 - y) e(s); relu: e(s) above the kink and 0 below it (the GPU tests keep every unit 1e-3 off the kink, `kink` below).
  * h' = (1 - z) n + z h (three roundings), c' = f c + i g and h' = o tanh_fast(c') likewise, term by term.
  * y_out (only under an output nonlinearity): one FMA chain over the H units of h'_top and the bias: gamma(H + 1); then the
    nonlinearity's stage error and its derivative from the value that ran.
  * every delta is a product of k factors, each a recomputed value or a derivative 1 - y^2 (e = 2 |y| e(y) + 2 u) or y (1 - y)
    (e = |1 - 2 y| e(y) + 2 u): e = sum_i |delta / f_i| e(f_i) + k u |delta|.  The adjoint of h' is a chain: d_hid's entry plus A FMAs
    (top layer, gamma(A + 1)) or plus G H FMAs over layer 1's deltas (layer 0 of two, gamma(G H + 1)), with the deltas' own errors
    through |w|.  The LSTM's cell adjoint is one FMA on d_hid's c entry.
  * the accumulation: a thread adds one term per row with one FMA (four envs per LDS read, still one rounding per row): acc = the
    rows of the workgroup's run of tiles; wg = the adds of k_fnn_param_reduce (n_wg / 4 per partial sum, 2 to join them, 1 with
    accumulate).  The caller reads both off the launch (chains=dict(acc=.., wg=..)).
"""
import numpy as np

from closed_loop_cases import sigmoid

U = 2.0 ** -24
TANH_ABS, SIGMOID_ABS = 2e-7, 4e-7
GATES = {"tanh": 1, "relu": 1, "gru": 3, "lstm": 4}
RNN_XP = 8


def _act(kind, s, e_s):
    """(value, error) of a nonlinearity from its pre-activation"""
    if kind == "tanh":
        y = np.tanh(s)
        return y, TANH_ABS + (1.0 - y * y) * e_s
    if kind == "sigmoid":
        y = sigmoid(s)
        return y, SIGMOID_ABS + y * (1.0 - y) * e_s
    if kind == "relu":  # (a unit below the kink by more than its error gives an exact 0: the callers keep 1e-3 away from the kink)
        return np.maximum(s, 0.0), np.where(s > 0.0, e_s, 0.0)
    return s, e_s


def _dact(kind, y, e_y):
    """(g'(z) from the value y = g(z) that ran, its error)"""
    if kind == "tanh":
        return 1.0 - y * y, 2.0 * np.abs(y) * e_y + 2.0 * U
    if kind == "sigmoid":
        return y * (1.0 - y), np.abs(1.0 - 2.0 * y) * e_y + 2.0 * U
    if kind == "relu":
        return (y > 0.0).astype(np.float64), np.zeros_like(y)
    return np.ones_like(y), np.zeros_like(y)


def _prod(*fe):
    """(product, first-order error) of factors given as (value, error) pairs"""
    v = np.ones_like(fe[0][0])
    for f, _ in fe:
        v = v * f
    e = len(fe) * U * np.abs(v)
    for k, (_, ek) in enumerate(fe):
        rest = np.ones_like(v)
        for j, (f, _) in enumerate(fe):
            if j != k:
                rest = rest * np.abs(f)
        e = e + rest * ek
    return v, e


def _pre(w, b_ih, b_hh, v_in, e_in, h, n_chain):
    """gate pre-activations, split into the input part (with b_ih) and the hidden part (with b_hh), and the error of each"""
    gi, gh = v_in @ w["w_ih"].T + b_ih, h @ w["w_hh"].T + b_hh
    mi = np.abs(v_in) @ np.abs(w["w_ih"]).T + np.abs(b_ih)
    mh = np.abs(h) @ np.abs(w["w_hh"]).T + np.abs(b_hh)
    ei = n_chain * U * mi + e_in @ np.abs(w["w_ih"]).T
    eh = n_chain * U * mh
    return gi, gh, ei, eh


def param_grad_fp64(net, x, p, abar, d_hid, inside, output_nonlin=None, chains=None, mistake=None):
    """net: closed_loop_cases.unpack_rnn's dict.  -> (flat gradient, flat sum of |terms|, flat bound, dict(zmax: max |gate
    pre-activation|, kink: min |pre-activation| of a relu cell, inf otherwise)).
    mistake: None, or one of the kernel mistakes the host test shows the bound to catch -- "no_r_scale" (W_hn, b_hn take delta_n),
    "drop_unit" (the last unit of every layer gets no delta), "ignore_c" (the c part of d_hid is not read)"""
    chains = chains or dict(acc=x.shape[0], wg=3)
    cell, nl, H = net["cell"], net["n_layers"], net["hidden"]
    G = GATES[cell]
    hp = (H + 3) // 4 * 4
    keep = np.asarray(inside, dtype=bool)
    x, p, abar, d_hid = (np.asarray(a, dtype=np.float64)[keep] for a in (x, p, abar, d_hid))
    R = x.shape[0]
    zero = np.zeros((R, H))
    # ---- forward: values and errors of everything the deltas need
    fwd, v_in, e_in, zmax, kink = [], x, np.zeros_like(x), 0.0, np.inf
    for l, w in enumerate(net["layers"]):
        h = p[:, l * H:(l + 1) * H]
        gi, gh, ei, eh = _pre(w, w["b_ih"], w["b_hh"], v_in, e_in, h, (RNN_XP if l == 0 else hp) + hp + 3)
        f = dict(inp=v_in, e_inp=e_in, h=h)
        if G == 1:
            zmax = max(zmax, float(np.abs(gi + gh).max()))
            if cell == "relu":
                kink = min(kink, float(np.abs(gi + gh).min()))
            f["y"], f["e_y"] = _act(cell, gi + gh, ei + eh)
            hn, e_hn = f["y"], f["e_y"]
        elif G == 3:
            s = gi[:, :2 * H] + gh[:, :2 * H]
            rz, e_rz = _act("sigmoid", s, ei[:, :2 * H] + eh[:, :2 * H])
            r, z, e_r, e_z = rz[:, :H], rz[:, H:], e_rz[:, :H], e_rz[:, H:]
            hn_, e_hn_ = gh[:, 2 * H:], eh[:, 2 * H:]
            rh, e_rh = _prod((r, e_r), (hn_, e_hn_))
            sn = gi[:, 2 * H:] + rh
            zmax = max(zmax, float(np.abs(s).max()), float(np.abs(sn).max()))
            n, e_n = _act("tanh", sn, ei[:, 2 * H:] + e_rh + U * np.abs(sn))
            hn = (1.0 - z) * n + z * h
            e_hn = np.abs(h - n) * e_z + (1.0 - z) * e_n + 3.0 * U * (np.abs((1.0 - z) * n) + np.abs(z * h))
            f.update(r=r, z=z, n=n, hn=hn_, e_r=e_r, e_z=e_z, e_n=e_n, e_hn=e_hn_)
        else:
            c = p[:, (nl + l) * H:(nl + l + 1) * H]
            s, es = gi + gh, ei + eh
            zmax = max(zmax, float(np.abs(s).max()))
            i, e_i = _act("sigmoid", s[:, :H], es[:, :H])
            fg, e_f = _act("sigmoid", s[:, H:2 * H], es[:, H:2 * H])
            g, e_g = _act("tanh", s[:, 2 * H:3 * H], es[:, 2 * H:3 * H])
            o, e_o = _act("sigmoid", s[:, 3 * H:], es[:, 3 * H:])
            (ig, e_ig), (fc, e_fc) = _prod((i, e_i), (g, e_g)), _prod((fg, e_f), (c, zero))
            cn = fc + ig
            tc, e_tc = _act("tanh", cn, e_ig + e_fc + U * np.abs(cn))
            hn, e_hn = _prod((o, e_o), (tc, e_tc))
            f.update(i=i, f=fg, g=g, o=o, c=c, tc=tc, e_i=e_i, e_f=e_f, e_g=e_g, e_o=e_o, e_tc=e_tc)
        f["hn_out"], f["e_hn_out"] = hn, e_hn
        fwd.append(f)
        v_in, e_in = hn, e_hn
    top, e_top = v_in, e_in
    # ---- delta_out
    if output_nonlin is None:
        dout, e_dout = abar, np.zeros_like(abar)
    else:
        yo = top @ net["w_out"].T + net["b_out"]
        e_yo = (H + 1) * U * (np.abs(top) @ np.abs(net["w_out"]).T + np.abs(net["b_out"])) + e_top @ np.abs(net["w_out"]).T
        a, e_a = _act(output_nonlin, yo, e_yo)
        dout, e_dout = _prod((abar, np.zeros_like(abar)), _dact(output_nonlin, a, e_a))
    m_acc = (chains["acc"] + chains["wg"]) * U
    grads, mags, bounds = [None] * nl, [None] * nl, [None] * nl

    def outer(d, e_d, y, e_y):
        """(sum_rows d y^T, sum |d y|, the bound) -- d [R, M], y [R, K]"""
        mag = np.abs(d).T @ np.abs(y)
        return d.T @ y, mag, np.abs(d).T @ e_y + e_d.T @ np.abs(y) + m_acc * mag

    A = net["w_out"].shape[0]
    out_w = outer(dout, e_dout, top, e_top)
    out_b = outer(dout, e_dout, np.ones((R, 1)), np.zeros((R, 1)))
    # ---- the adjoint of the top layer's h'
    wd = dout @ net["w_out"]
    dh = d_hid[:, (nl - 1) * H:nl * H] + wd
    e_dh = e_dout @ np.abs(net["w_out"]) + (A + 1) * U * (np.abs(d_hid[:, (nl - 1) * H:nl * H]) + np.abs(dout) @ np.abs(net["w_out"]))
    for l in range(nl - 1, -1, -1):
        f, w = fwd[l], net["layers"][l]
        D = (dh, e_dh)
        if G == 1:
            di = [_prod(D, _dact(cell, f["y"], f["e_y"]))]
            dg = di
        elif G == 3:
            r, z, n, h = (f["r"], f["e_r"]), (f["z"], f["e_z"]), (f["n"], f["e_n"]), f["h"]
            one_z = (1.0 - f["z"], f["e_z"] + U)
            dn = _prod(D, one_z, _dact("tanh", *n))
            h_n = (h - f["n"], f["e_n"] + U * np.abs(h - f["n"]))
            di = [_prod(dn, (f["hn"], f["e_hn"]), _dact("sigmoid", *r)), _prod(D, h_n, _dact("sigmoid", *z)), dn]
            dg = di[:2] + [dn if mistake == "no_r_scale" else _prod(dn, r)]
        else:
            i, fg, g, o = (f["i"], f["e_i"]), (f["f"], f["e_f"]), (f["g"], f["e_g"]), (f["o"], f["e_o"])
            tc = (f["tc"], f["e_tc"])
            t1 = _prod(D, o, _dact("tanh", *tc))
            ca = d_hid[:, (nl + l) * H:(nl + l + 1) * H] * (0.0 if mistake == "ignore_c" else 1.0)
            dc = (t1[0] + ca, t1[1] + U * np.abs(t1[0] + ca))
            di = [_prod(dc, g, _dact("sigmoid", *i)), _prod(dc, (f["c"], zero), _dact("sigmoid", *fg)), _prod(dc, i, _dact("tanh", *g)),
                  _prod(D, tc, _dact("sigmoid", *o))]
            dg = di
        if mistake == "drop_unit":
            di = [(np.concatenate([d[:, :-1], 0.0 * d[:, -1:]], axis=1), e) for d, e in di]
            dg = [(np.concatenate([d[:, :-1], 0.0 * d[:, -1:]], axis=1), e) for d, e in dg]
        Di, eDi = np.concatenate([d for d, _ in di], axis=1), np.concatenate([e for _, e in di], axis=1)
        Dg, eDg = np.concatenate([d for d, _ in dg], axis=1), np.concatenate([e for _, e in dg], axis=1)
        one, z1 = np.ones((R, 1)), np.zeros((R, 1))
        parts = [outer(Di, eDi, f["inp"], f["e_inp"]), outer(Dg, eDg, f["h"], zero), outer(Di, eDi, one, z1), outer(Dg, eDg, one, z1)]
        grads[l], mags[l], bounds[l] = ([q[k].reshape(-1) for q in parts] for k in range(3))
        if l > 0:
            below = d_hid[:, (l - 1) * H:l * H]
            dh = below + Di @ w["w_ih"]
            e_dh = eDi @ np.abs(w["w_ih"]) + (G * H + 1) * U * (np.abs(below) + np.abs(Di) @ np.abs(w["w_ih"]))
    cat = lambda per_layer, k: np.concatenate([v for layer in per_layer for v in layer] + [out_w[k].reshape(-1), out_b[k].reshape(-1)])  # noqa: E731
    return cat(grads, 0), cat(mags, 1), cat(bounds, 2), dict(zmax=zmax, kink=kink)


# ------------------------------------------------------------------------------------------------- the host test's rows
# Synthetic rows (normal inputs, hidden states, cotangents; every fourth row is outside) for the cells of test_gpu_rnn_param_grad's
# table: (env class, dt, cell, layers, units, output nonlinearity)
TABLE = {
    "omo-tanh-3": ("OneMassOscillatorSim", 0.02, "tanh", 1, 3, None),
    "pend-relu-8": ("PendulumSim", 0.01, "relu", 1, 8, None),
    "pend-gru-8": ("PendulumSim", 0.01, "gru", 1, 8, None),
    "qq-su-gru-2x64": ("QQubeSwingUpSim", 0.004, "gru", 2, 64, None),
    "qcp-su-lstm-64": ("QCartPoleSwingUpSim", 0.002, "lstm", 1, 64, None),
    "qbb-lstm-2x33-tanh-out": ("QBallBalancerSim", 0.01, "lstm", 2, 33, "tanh"),
    "bob-gru-63": ("BallOnBeamSim", 0.01, "gru", 1, 63, None),
}
ROWS = 240


def rows_case(key):
    """(torch fp64 policy, unpacked fp64 net, x, p, abar, d_hid, inside, output nonlinearity's name)"""
    import torch

    import closed_loop_cases as cells
    import simurlacra_amd as vs

    env_cls, dt, cell, nl, H, out = TABLE[key]
    env = getattr(vs, env_cls)(dt=dt, max_steps=30)
    O, A = env.obs_space.flat_dim, env.act_space.flat_dim
    torch.manual_seed(11)
    policy = cells.torch_policy(env.spec, cell, nl, H, {None: None, "tanh": torch.tanh}[out])
    with torch.no_grad():  # float32 values, so that the host test's float32 pass runs on the very same parameters
        flat = policy.param_values.detach().float()
    policy = policy.double()
    policy.param_values = flat.double()
    net = cells.unpack_rnn(flat.numpy(), cell, nl, H, O, A)
    rng = np.random.default_rng(17)
    f32 = lambda a: a.astype(np.float32).astype(np.float64)  # noqa: E731
    x, p = f32(rng.normal(size=(ROWS, O))), f32(0.5 * rng.normal(size=(ROWS, policy.hidden_size)))
    abar, d_hid = f32(rng.normal(size=(ROWS, A))), f32(rng.normal(size=(ROWS, policy.hidden_size)))
    inside = np.arange(ROWS) % 4 != 3
    return policy, net, x, p, abar, d_hid, inside, out
