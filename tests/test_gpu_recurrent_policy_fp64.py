"""k_rollout_rnn (vs_set_policy_rnn) against the policy's own torch module in DOUBLE precision, one step at a time on the kernel's
records, at a bound that is derived and not tuned -- at every hidden width where the padding to a multiple of 4 units is live,
with saturated gates and a 64 step old state, with the output nonlinearity far in both tails, and through a population.

Reference.  copy.deepcopy(pol).double() on the CPU: the fp32 weights are exact in fp64.  The recorded observation and the
recorded hidden state before step t go in; the recorded action and the recorded hidden state before step t + 1 are compared.
Teacher-forced in this way the error of one step does not compound over the horizon.  The per-gate pre-activations and the
magnitude sums the bound needs come from a NumPy restatement of the three cells in torch's gate order (GRU r, z, n; LSTM i, f,
g, o) with the same fp64 weights; every test asserts that it agrees with the .double() module to 1e-12 (1 + |module|).

Bound.  Per entry, from reference quantities only, u = 2^-24 (fp32 unit round-off), hp = H rounded up to a multiple of 4:
  * pre-activation v = (a_i + b_ih) + (a_h + b_hh), a_i and a_h chains of fused multiply-adds.  The kernel sums K terms:
    RNN_XP + hp in layer 0 (the padded observation row and the padded state rows), 2 hp in layer 1.  A chain of m FMAs is off by
    at most m u sum |w_k x_k| to first order, the three additions by u each of what they add:
        B(v) = (K + 4) u (sum |w_k x_k| + |b_ih| + |b_hh|)  [+ sum |w_k| B(x_k) in layer 1, whose input is layer 0's h'].
    The GRU's candidate v_n = (a_i + b_in) + r (a_h + b_hn): the same with r (sum |w h| + |b_hn|) for the second half (the one
    more rounding of the product is the fourth of the + 4), plus B(r) |a_h + b_hn|.
  * tanh_fast: Lipschitz constant 1, and the absolute error its comment in vecsim_kernels.h states: B(v) + 2e-7.
  * the gates' sigmoid s = rcp(1 + exp2(-v log2 e)): Lipschitz constant 1 / 4, B(v) / 4, plus an absolute term for the hardware
    exponential and reciprocal.  The MI355X guides this project follows give no accuracy figure for v_exp_f32 or v_rcp_f32, so
    the term is 2 ulp (fp32) of the result plus 2 |v| u s (1 - s) for the rounding of the scaled argument (d s / d v = s (1 - s);
    one rounding of the constant, one of the product); the hardware flushes a sub-normal result to 0: + 2^-126.
  * GRU h' = (1 - z) n + z h:   B = |n - h| B(z) + (1 - z) B(n) + 3 u (|(1 - z) n| + |z h|)
    LSTM c' = f c + i g:        B = |c| B(f) + |g| B(i) + i B(g) + 3 u (|f c| + |i g|)
         h' = o tanh(c'):       B = |tanh c'| B(o) + o (B(c') + 2e-7) + 3 u |o tanh c'|
    tanh cell B(v) + 2e-7, relu cell B(v) (Lipschitz 1, exact).
  * action o_j = sum_k Wo_jk h'_k + bo_j over hp FMAs:  sum |Wo_jk| B(h'_k) + (hp + 3) u (sum |Wo_jk h'_k| + |bo_j|), then the
    output nonlinearity as above (relu and identity: Lipschitz 1, no extra term).
  * everything above is first order; a factor 2 covers the second-order terms and is the only margin.
The flat 1e-5 (1 + |ref|) of test_gpu_recurrent_policy.py is asserted against the fp64 reference too, so this file is nowhere
weaker than that one.  Run with -s to see the worst ratio to the bound of every test.

Measured on an MI355X (worst ratio to the doubled bound, action / hidden): every width 0.10 / 0.08; saturated gates 0.003 / 0.15
(there the flat figure is the tighter one: hidden 8.1e-6 (1 + |ref|) for the GRU at gain 16); output tails 0.03 / 0.06;
population 0.03 / 0.06.  The bound is a worst case over K roundings of one sign, so a kernel that is right sits well below 1.
"""
import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import test_gpu_recurrent_policy as rp  # noqa: E402
from test_gpu_recurrent_policy import make_policy, run_kernel  # noqa: E402

U = 2.0 ** -24
TANH_ABS = 2e-7      # tanh_fast's stated absolute error
FLUSH = 2.0 ** -126  # the smallest normal fp32: what a flushed sub-normal result is off by at most
RNN_XP = 8           # the kernel's padded observation row


@pytest.fixture(scope="module")
def vs():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import simurlacra_amd

    return simurlacra_amd


# ------------------------------------------------------------------------------------------------ reference and bound
def sigmoid(v):
    """fp64, accurate in both tails (no 1 - tanh cancellation)"""
    with np.errstate(over="ignore"):
        e = np.exp(-np.abs(v))
    return np.where(v >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def sigmoid_bound(v, bv):
    s = sigmoid(v)
    ulp = np.spacing(s.astype(np.float32)).astype(np.float64)
    return 0.25 * bv + 2.0 * ulp + 2.0 * np.abs(v) * U * s * sigmoid(-v) + FLUSH


def policy_arrays(pol):
    """(cell, layers, H, [(W_ih, W_hh, b_ih, b_hh)] per layer, W_out, b_out, output nonlinearity) in fp64"""
    from simurlacra_amd.policies import rnn_kernel_spec

    spec = rnn_kernel_spec(pol)
    m = pol.rnn_layers
    f64 = lambda p: p.detach().double().numpy()
    layers = [tuple(f64(getattr(m, f"{k}_l{l}")) for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")) for l in range(m.num_layers)]
    return spec["cell"], m.num_layers, m.hidden_size, layers, f64(pol.output_layer.weight), f64(pol.output_layer.bias), spec["output_nonlin"]


def one_step(pol, obs, hid):
    """One step of the policy in fp64 on obs [N, O] and the packed hidden state hid [N, hs]: the action, the next packed hidden
    state, the FIRST-ORDER bound of either (see the module docstring; the caller doubles it), and the gates of every layer:
    {name: pre-activation [N, layers, H]} and {name: value}"""
    cell, L, H, layers, Wo, bo, out_nonlin = policy_arrays(pol)
    hp = (H + 3) // 4 * 4
    G = {"tanh": 1, "relu": 1, "gru": 3, "lstm": 4}[cell]
    N = obs.shape[0]
    x, xb = obs.astype(np.float64), np.zeros(obs.shape)
    h_all = hid[:, :L * H].reshape(N, L, H).astype(np.float64)
    c_all = hid[:, L * H:].reshape(N, L, H).astype(np.float64) if cell == "lstm" else None
    new_h, new_hb, new_c, new_cb = [], [], [], []
    pre, val = {}, {}

    def keep(name, v, s):
        pre.setdefault(name, []).append(v)
        val.setdefault(name, []).append(s)

    for l, (Wi, Wh, bi, bh) in enumerate(layers):
        K = (RNN_XP if l == 0 else hp) + hp
        h = h_all[:, l]
        split = lambda a: a.reshape(N, G, H)  # torch stacks the gates' rows: row g H + j is gate g of unit j
        ai, ah = split(x @ Wi.T), split(h @ Wh.T)
        si, sh = split(np.abs(x) @ np.abs(Wi).T), split(np.abs(h) @ np.abs(Wh).T)
        ein = split(xb @ np.abs(Wi).T)  # what the bound of the layer's input makes of the pre-activation
        bi, bh = bi.reshape(G, H), bh.reshape(G, H)
        v = (ai + bi) + (ah + bh)
        bv = (K + 4) * U * (si + sh + np.abs(bi) + np.abs(bh)) + ein
        if G == 1:
            keep("v", v[:, 0], np.tanh(v[:, 0]))
            hn, hb = (np.tanh(v[:, 0]), bv[:, 0] + TANH_ABS) if cell == "tanh" else (np.maximum(v[:, 0], 0.0), bv[:, 0])
        elif G == 3:
            r, z = sigmoid(v[:, 0]), sigmoid(v[:, 1])
            br, bz = sigmoid_bound(v[:, 0], bv[:, 0]), sigmoid_bound(v[:, 1], bv[:, 1])
            hpart = ah[:, 2] + bh[2]
            vn = (ai[:, 2] + bi[2]) + r * hpart
            bvn = (K + 4) * U * (si[:, 2] + np.abs(bi[2]) + r * (sh[:, 2] + np.abs(bh[2]))) + ein[:, 2] + br * np.abs(hpart)
            n, bn = np.tanh(vn), bvn + TANH_ABS
            hn = (1.0 - z) * n + z * h
            hb = np.abs(n - h) * bz + (1.0 - z) * bn + 3 * U * (np.abs((1.0 - z) * n) + np.abs(z * h))
            keep("r", v[:, 0], r)
            keep("z", v[:, 1], z)
        else:
            c = c_all[:, l]
            ig, fg, og = sigmoid(v[:, 0]), sigmoid(v[:, 1]), sigmoid(v[:, 3])
            big, bfg, bog = (sigmoid_bound(v[:, q], bv[:, q]) for q in (0, 1, 3))
            gg, bgg = np.tanh(v[:, 2]), bv[:, 2] + TANH_ABS
            cn = fg * c + ig * gg
            cb = np.abs(c) * bfg + np.abs(gg) * big + ig * bgg + 3 * U * (np.abs(fg * c) + np.abs(ig * gg))
            tc = np.tanh(cn)
            hn = og * tc
            hb = np.abs(tc) * bog + og * (cb + TANH_ABS) + 3 * U * np.abs(hn)
            new_c.append(cn)
            new_cb.append(cb)
            keep("i", v[:, 0], ig)
            keep("f", v[:, 1], fg)
            keep("o", v[:, 3], og)
        new_h.append(hn)
        new_hb.append(hb)
        x, xb = hn, hb
    o = x @ Wo.T + bo
    ob = xb @ np.abs(Wo).T + (hp + 3) * U * (np.abs(x) @ np.abs(Wo).T + np.abs(bo))
    if out_nonlin == "tanh":
        act, ab = np.tanh(o), ob + TANH_ABS
    elif out_nonlin == "sigmoid":
        act, ab = sigmoid(o), sigmoid_bound(o, ob)
    elif out_nonlin == "relu":
        act, ab = np.maximum(o, 0.0), ob
    else:
        act, ab = o, ob
    nxt, nb = np.concatenate(new_h + new_c, axis=1), np.concatenate(new_hb + new_cb, axis=1)
    stack = lambda d: {k: np.stack(a, axis=1) for k, a in d.items()}
    return act, ab, nxt, nb, stack(pre), stack(val)


def worst_ratio(err, bound):
    pos = bound > 0
    ratio = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    return ratio, bool((err <= bound).all())


def check_records(pol, obs, act, hrec, hfin, label, done=None):
    """the kernel's records (obs [T, n, O], act [T, n, A], hidden before every step [T, n, hs], hidden behind the last [n, hs])
    against the fp64 reference at the bound and at the flat 1e-5; returns the reference's gates (pre-activations, values) and the
    recorded states before and behind every step, entries [T n, ...].  done [T, n] (auto-reset off): a lane's actions count up to
    its first done step, its next states up to the step before (behind its end a lane is frozen); None: no lane ends"""
    T, n = obs.shape[:2]
    alive = np.ones((T, n), dtype=bool)
    if done is not None:
        alive[1:] = np.cumsum(done, axis=0)[:-1] == 0
    carry = (alive if done is None else alive & ~done).ravel()
    alive = alive.ravel()
    hs = hrec.shape[2]
    assert pol.hidden_size == hs and hfin.shape == (n, hs)
    x, h0 = obs.reshape(T * n, -1), hrec.reshape(T * n, hs)
    nxt = np.concatenate([hrec[1:], hfin[None]], axis=0).reshape(T * n, hs)
    got_a = act.reshape(T * n, -1)
    ref_a, ba, ref_h, bh, pre, val = one_step(pol, x, h0)
    # the restatement is the module
    with torch.no_grad():
        mod_a, mod_h = copy.deepcopy(pol).double()(torch.from_numpy(x.astype(np.float64)), torch.from_numpy(h0.astype(np.float64)))
    mod_a, mod_h = mod_a.numpy(), mod_h.numpy()
    assert mod_a.dtype == np.float64 and mod_h.dtype == np.float64
    assert (np.abs(ref_a - mod_a) <= 1e-12 * (1 + np.abs(mod_a))).all() and (np.abs(ref_h - mod_h) <= 1e-12 * (1 + np.abs(mod_h))).all()
    assert np.isfinite(got_a).all() and np.isfinite(nxt).all() and alive.any() and carry.any()
    err_a, err_h = np.abs(got_a - mod_a)[alive], np.abs(nxt - mod_h)[carry]
    ra, ok_a = worst_ratio(err_a, 2.0 * ba[alive])
    rh, ok_h = worst_ratio(err_h, 2.0 * bh[carry])
    fa, fh = float((err_a / (1 + np.abs(mod_a[alive]))).max()), float((err_h / (1 + np.abs(mod_h[carry]))).max())
    print(f"\n{label}: worst ratio to the bound: action {ra:.4f}, hidden {rh:.4f}; max |x - ref| / (1 + |ref|): action {fa:.2e}, "
          f"hidden {fh:.2e}")
    assert ok_a and ok_h, (label, ra, rh)
    assert fa < 1e-5 and fh < 1e-5, (label, fa, fh)
    return pre, val, h0, nxt


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


# ------------------------------------------------------------------------------------------------ 1: every hidden width
WIDTHS = (1, 2, 3, 4, 5, 61, 63, 64)
WIDTH_CASES = [(cell, layers, H) for cell in ("tanh", "relu", "gru", "lstm") for layers in (1, 2) for H in WIDTHS]


@pytest.mark.parametrize("case", range(len(WIDTH_CASES)), ids=["{}-x{}-{}".format(*c) for c in WIDTH_CASES])
def test_every_hidden_width(vs, case):
    """hp - H = 3, 2, 1, 0, 3 at the small widths, live padding at RNN_MAXW (61, 63 -> hp = 64): layer 1 reads layer 0's padded h'
    rows, the LSTM keeps padded cell rows, and VS_POLICY_HIDDEN carries H of every hp rows from launch to launch"""
    cell, layers, H = WIDTH_CASES[case]
    name = ("qq-su", "qbb")[case % 2]
    out_nonlin = (None, "tanh", "sigmoid", "relu")[(case // 2) % 4]
    n, splits = 130, (5, 7)
    T = sum(splits)
    assert rp.KW[name]["max_steps"] > T
    O, A = vs.env_dims(name)["O"], vs.env_dims(name)["A"]
    hs = layers * H * (2 if cell == "lstm" else 1)
    # no width is run with a layer dead: a relu cell's (and a relu output's) biases are made positive, and the policy is the first
    # of a few seeds whose REFERENCE leaves something in every layer's rows (h and c) on the records
    for attempt in range(4):
        pol = make_policy(vs, cell, H, layers, O, A, out_nonlin, seed=100 + case + 1000 * attempt)
        with torch.no_grad():
            for pname, p in pol.named_parameters():
                if "bias" in pname and (cell if pname.startswith("rnn_layers") else out_nonlin) == "relu":
                    p.abs_()
        tr, hrec, hfin, e = run_kernel(vs, name, pol, n, splits, False)
        ref_next = one_step(pol, tr["obs"].reshape(T * n, O), hrec.reshape(T * n, hs))[2]
        live = (np.abs(ref_next).reshape(T * n, hs // H, H).max(axis=(0, 2)) > 0).all()
        if live or attempt == 3:
            break
        e.close()
    assert live
    assert tuple(e.policy_hidden().shape) == (hs, e.ld) and tuple(e.hidden_record_tensor().shape[1:]) == (hs, e.ld)
    assert hrec.shape == (T, n, hs) and hfin.shape == (n, hs)
    assert not tr["done"].any() and e.error_count() == 0  # no lane ends: every step carries its state
    assert not hrec[0].any()
    check_records(pol, tr["obs"], tr["act"], hrec, hfin, f"{name} {cell} x{layers} H = {H} out {out_nonlin}")
    # one launch of 12 steps leaves the same bits (records, hidden records, VS_POLICY_HIDDEN)
    tr1, hrec1, hfin1, e1 = run_kernel(vs, name, pol, n, (T,), False)
    for key in tr:
        assert np.array_equal(tr[key], tr1[key]), key
    assert same_bits(hrec, hrec1) and same_bits(hfin, hfin1)
    assert same_bits(e.policy_hidden().cpu().numpy(), e1.policy_hidden().cpu().numpy())  # the lanes behind n too
    e.close()
    e1.close()


# ------------------------------------------------------------------------------------------------ 2: saturated gates, an old state
GAINS = (4.0, 8.0, 16.0, 32.0, 64.0)


def saturation_shares(cell, pre, val):
    """shares over the gate evaluations of a run, from the reference alone: the sigmoid gates of the GRU (r, z) and the LSTM
    (i, f, o), the tanh cell's own pre-activation"""
    v = np.abs(np.concatenate([a.ravel() for a in pre.values()]))
    s = {"beyond 17": float((v > 17).mean()), "below 1": float((v < 1).mean())}
    ok = s["beyond 17"] >= 0.05 and s["below 1"] >= 0.05
    if cell == "gru":
        s["z > 0.999"], s["z < 0.001"] = float((val["z"] > 0.999).mean()), float((val["z"] < 0.001).mean())
        ok = ok and s["z > 0.999"] >= 0.01 and s["z < 0.001"] >= 0.01
    return s, ok


@pytest.mark.parametrize("cell,layers", [("gru", 2), ("lstm", 2), ("tanh", 1)])
def test_saturated_gates_and_an_old_state(vs, cell, layers, monkeypatch):
    """The recurrent weights (weight_ih, weight_hh) times a gain, 64 steps without an episode end.  The gain is the smallest of
    GAINS at which the REFERENCE's gates, evaluated on the records of that gain's run, are saturated and unsaturated in the shares
    asserted below (nothing the kernel's error enters decides it)."""
    name, H, n, T = "qq-su", 24, 130, 64
    monkeypatch.setitem(rp.KW, name, dict(rp.KW[name], max_steps=10 * T))
    O, A = vs.env_dims(name)["O"], vs.env_dims(name)["A"]
    base = make_policy(vs, cell, H, layers, O, A, seed=7)
    for gain in GAINS:
        pol = copy.deepcopy(base)
        with torch.no_grad():
            for pname, p in pol.rnn_layers.named_parameters():
                if pname.startswith("weight_"):
                    p.mul_(gain)
        tr, hrec, hfin, e = run_kernel(vs, name, pol, n, (T,), False)
        _, _, _, _, pre, val = one_step(pol, tr["obs"].reshape(T * n, O), hrec.reshape(T * n, -1))
        shares, ok = saturation_shares(cell, pre, val)
        if ok or gain == GAINS[-1]:
            break
        e.close()
    print(f"\n{cell} x{layers}: gain {gain}, shares of the gate evaluations: " + ", ".join(f"{k} {v:.3f}" for k, v in shares.items()))
    assert shares["beyond 17"] >= 0.05 and shares["below 1"] >= 0.05
    if cell == "gru":
        assert shares["z > 0.999"] >= 0.01 and shares["z < 0.001"] >= 0.01
    assert not tr["done"].any() and e.error_count() == 0  # the state before the last step is 63 steps old on every lane
    pre, val, h0, nxt = check_records(pol, tr["obs"], tr["act"], hrec, hfin, f"{name} {cell} x{layers} gain {gain}")
    L = layers
    # the carry survives: a unit the reference holds keeps its state
    if cell == "gru":
        hold = (val["z"] > 1 - 2.0 ** -20).reshape(T * n, L * H)
        was, now = h0[:, :L * H][hold], nxt[:, :L * H][hold]
    elif cell == "lstm":
        hold = ((val["f"] > 1 - 2.0 ** -20) & (val["i"] < 2.0 ** -20)).reshape(T * n, L * H)
        was, now = h0[:, L * H:][hold], nxt[:, L * H:][hold]
    if cell != "tanh":
        assert hold.any()
        drift = np.abs(now.astype(np.float64) - was) / (np.abs(was) + 1.0)
        print(f"    {int(hold.sum())} held units, max |x' - x| / (|x| + 1) = {drift.max():.2e} (allowed {2.0 ** -19:.2e})")
        assert (drift <= 2.0 ** -19).all()
    # the same 64 steps as launches of 1 and 63: the same bits
    tr1, hrec1, hfin1, e1 = run_kernel(vs, name, pol, n, (1, T - 1), False)
    for key in tr:
        assert np.array_equal(tr[key], tr1[key]), key
    assert same_bits(hrec, hrec1) and same_bits(hfin, hfin1)
    e.close()
    e1.close()


# ------------------------------------------------------------------------------------------------ 3: the output nonlinearity's tails
@pytest.mark.parametrize("out_nonlin", ["sigmoid", "tanh", "relu"])
def test_output_nonlinearity_far_in_both_tails(vs, out_nonlin):
    """output biases of -100 and +100: exp2 overflows to +inf in the sigmoid's small tail, and 1 / inf has to come out as 0"""
    name, H, n, T = "qbb", 7, 130, 12
    O, A = vs.env_dims(name)["O"], vs.env_dims(name)["A"]
    assert A == 2
    for sign in (1.0, -1.0):
        pol = make_policy(vs, "gru", H, 1, O, A, out_nonlin, seed=41)
        with torch.no_grad():
            pol.output_layer.bias.copy_(torch.tensor([-100.0 * sign, 100.0 * sign]))
        tr, hrec, hfin, e = run_kernel(vs, name, pol, n, (T,), False)
        act = tr["act"]
        lo, hi = (0, 1) if sign > 0 else (1, 0)  # the action with the bias of -100, of +100
        nan = int(np.isnan(act).sum())
        print(f"\n{out_nonlin} bias {-100 * sign:+.0f} / {100 * sign:+.0f}: {nan} NaN of {act.size} recorded actions, "
              f"error_count {e.error_count()}, low tail in [{np.nanmin(act[..., lo]):.3e}, {np.nanmax(act[..., lo]):.3e}], "
              f"high tail in [{np.nanmin(act[..., hi]):.3e}, {np.nanmax(act[..., hi]):.3e}]")
        assert np.isfinite(act).all()
        assert e.error_count() == 0
        ref_a = one_step(pol, tr["obs"].reshape(T * n, O), hrec.reshape(T * n, -1))[0].reshape(T, n, A)
        if out_nonlin == "sigmoid":
            assert (np.abs(act[..., lo] - ref_a[..., lo]) <= FLUSH).all()  # ~ 4e-44: the sub-normal itself or 0
            assert (act[..., hi] == 1.0).all()
        elif out_nonlin == "tanh":
            assert (act[..., lo] == -1.0).all() and (act[..., hi] == 1.0).all()
        else:
            assert (act[..., lo] == 0.0).all()
        check_records(pol, tr["obs"], act, hrec, hfin, f"{name} gru H = {H} out {out_nonlin} bias {-100 * sign:+.0f} / {100 * sign:+.0f}",
                      done=tr["done"].astype(bool))
        e.close()


# ------------------------------------------------------------------------------------------------ 4: a population, hp != H
def test_population_path_at_a_padded_width(vs):
    """three parameter sets of a GRU with 5 units (hp = 8) in one launch: the workgroup's set moves the base of the kernel's
    scalar loads, and every set's lanes are held to that set's own reference"""
    from simurlacra_amd.policies import rnn_kernel_spec

    name, H, n, T, P = "qq-su", 5, 192, 10, 3
    O, A = vs.env_dims(name)["O"], vs.env_dims(name)["A"]
    pols = [make_policy(vs, "gru", H, 1, O, A, seed=60 + s) for s in range(P)]
    specs = [rnn_kernel_spec(p) for p in pols]
    lane_set = np.repeat(np.array([2, 0, 1]), 64).astype(np.int32)
    e = vs.VecSimEnv(name, n, **rp.KW[name])
    e.set_auto_reset(False, seed=31)
    e.reset(seed=5)
    e.set_policy_rnn(**specs[0])
    e.set_policy_population(torch.stack([sp["params"] for sp in specs]), lane_set)
    e.set_record_mode(2)
    e.set_traj_capacity(T)
    e.set_policy_hidden_record(pols[0].hidden_size)
    e.step_policy(T, record=True)
    tr = e.traj(T)
    hrec = e.hidden_record_tensor()[:T, :, :n].permute(0, 2, 1).cpu().numpy()
    hfin = e.policy_hidden()[:, :n].t().cpu().numpy()
    assert tuple(e.policy_hidden().shape) == (H, e.ld)
    assert not tr["done"].any() and e.error_count() == 0
    for s in range(P):
        lanes = np.flatnonzero(lane_set == s)
        assert len(lanes) == 64
        check_records(pols[s], tr["obs"][:, lanes], tr["act"][:, lanes], hrec[:, lanes], hfin[lanes], f"{name} gru H = {H} set {s}")
    # the sets differ: set 1's lanes are not what set 0's parameters give
    lanes = np.flatnonzero(lane_set == 1)
    other = one_step(pols[0], tr["obs"][:, lanes].reshape(T * 64, O), hrec[:, lanes].reshape(T * 64, -1))[0]
    assert np.abs(other - tr["act"][:, lanes].reshape(T * 64, A)).max() > 1e-3
    e.close()
