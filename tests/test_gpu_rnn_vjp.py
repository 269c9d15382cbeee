"""
vs_rollout_vjp_rnn / k_rollout_vjp_rnn: the reverse-mode sweep over CLOSED-LOOP recorded rollouts with a recurrent policy (Elman tanh /
relu, GRU, LSTM of one or two layers) in the loop, VecSimEnv.rollout_vjp_rnn and DifferentiableRecurrentRollout.

Shapes, scales and the tolerance rule are those of test_gpu_fnn_vjp.py / test_gpu_policy_vjp.py, all three from derivative_cases.py: 150 lanes
(64 + 64 + 22), T = 24, max_steps = 50, +-5 % per-lane parameters, lanes 0 .. 9 end early, random cotangents on all FIVE inputs (g_rew,
g_obs, g_act, g_state_last, g_hid_last); per lane 3e-3 |g| + 3e-4 max |g| against central differences of the fp64 closed loop at relative
steps 1e-6 and 1e-5 (closed_loop_cases.py: oracle.cpu_ref for the step, its NumPy cells for the policy).  The tolerance is taken
separately over the two blocks of a lane's entries: [every action offset n_t | every initial-state entry] and [every initial-hidden
entry (d_hid0) | additive offsets on p_{t+1} at a fixed random set of 40 (t, unit) pairs (d_hid), every layer's h and c block among
them; all T pairs of the one-unit cell] -- stricter than one maximum over both.  EVERY entry must be smooth, from the oracle alone, and
every entry is compared.

The weights (closed_loop_cases.make_rnn):
  * the policy's input rows are measured on a rollout under the bias action alone: mid and dev = half their range;
  * W_ih (x - mid) is bounded by amp = 1 (relu: 0.3) on that rollout, rows scaled by 1 / sqrt(fan-in) (relu: 1 / fan-in); layer 1 sees
    h' in [-1, 1] (relu: [0, 2]) with the same rule; the sum b_ih + b_hh is +-U(0, 0.7) (relu: +-U(0.5, 1.5), unit 0 of every layer
    positive so that the layer is alive), split evenly over the two biases;
  * W_hh = +-U(0.5, 1) whh / sqrt(H) (relu: whh / (2 H)): whh is the case's knob for the hidden adjoint;
  * the output layer adds at most +-gain x 0.12 ACT_IN to a bias of +-0.45 ACT_IN on the range of the top layer's h' measured on that
    rollout (rows scaled by 1 / fan-in, so the sum uses a fraction of the bound); under a tanh output the same in the pre-activation,
    +-0.24 around +-atanh(0.7).  Asserted on the closed loop: section 8e's box, |a| in [0.30, 0.60] ACT_IN (tanh output: [0.51, 0.83]).
  * gain, whh and the seed of a case are chosen on the CPU, from the oracle alone, until every entry is smooth, no relu pre-activation is
    within 1e-3 of 0, and d_init parts by more than 10 x the tolerance on at least half of the full-length lanes (a) from the open
    loop's (a kernel without gpol fails) and (b) from the closed loop's with the hidden adjoint cut -- the policy evaluated at the
    recorded p_t as constants, which is eta = 0 at every step -- (a kernel that drops eta fails).
"""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import closed_loop_cases as clc  # noqa: E402
from closed_loop_cases import (ELMAN_AS_FNN, ENVS, GAMMA, NT, RNN_AUTOGRAD as AUTOGRAD, RNN_ORACLE_CASES as ORACLE_CASES, TT, block_tolerance,  # noqa: E402
                               blocks_of, case, check_no_unit_near_a_kink, cotangents, flat_params, hidden_reference, oracle_reference,
                               recorded, reference, rnn_policy, rnn_step, shares, torch_policy, unpack_rnn, worst_in_blocks)
from derivative_cases import (ACT_IN, HIDDEN_FAMILIES, INIT_SCALE, KW, MAX_STEPS, N, N_EDGE, STARTS, STATE_BUFFERS, T,  # noqa: E402
                              check_hidden_block, check_hidden_start, check_net_keeps_the_box, dev, hidden_conditions, hidden_start,
                              scaled_hidden, smooth_per_lane, worst_of)


@pytest.fixture(scope="module")
def vs():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import simurlacra_amd

    return simurlacra_amd


def scaled(vs, c, d_act, d_init, d_hid, d_hid0):
    """the four outputs as one array [N, T A + S + Hs + pairs] in the units of reference().  The ENV's hidden rows of d_init are cut off:
    they are no further columns of a lane's row (derivative_cases.py says why) and go through scaled_hidden() and
    check_hidden_block() in test_env_hidden_adjoint_against_the_closed_loop_fp64_oracle."""
    ref, name = c["ref"], c["name"]
    d_act, d_init, d_hid, d_hid0 = (vs.lanes_first(x, N).cpu().numpy() for x in (d_act, d_init, d_hid, d_hid0))
    picked = np.stack([d_hid[:, t, u] for t, u in c["pairs"]], axis=1)
    got = np.concatenate([d_act.reshape(N, T * ref.A) * ACT_IN[name], d_init[:, :ref.S] * np.array(INIT_SCALE[name]), d_hid0, picked], axis=1)
    assert np.isfinite(got).all()
    return got.astype(np.float64)


def oracle_conditions(key):
    """everything the reference alone must meet (asserted before the GPU is asked) -> (c, f1, smooth, length, shares)"""
    c = case(key)
    r = oracle_reference(key)
    f1, length = r.f1, r.length
    smooth = smooth_per_lane(f1, r.f2)
    assert smooth.all(), (key, float((~smooth).mean()))  # every entry, none excluded
    check_net_keeps_the_box(c, r.acts, length)
    check_no_unit_near_a_kink(c, r.pres, length)
    assert (length[:N_EDGE] < T).any() and (length[N_EDGE:] == T).mean() > 0.9  # lanes that end early, lanes that run through
    seen = shares(c, f1, smooth, length, r.open_init, r.cut_init)
    assert seen[0] >= 0.5 and seen[1] >= 0.5, (key, seen)  # the test can see gpol, and it can see eta
    return c, f1, smooth, length, seen, r.open_init, r.cut_init


# --------------------------------------------------------------------------------------- 1. against the fp64 closed loop
@pytest.mark.parametrize("key", ORACLE_CASES)
def test_against_the_closed_loop_fp64_oracle(vs, key):
    """Worst error / tolerance over all entries as measured on the MI355X: see DESIGN.md section 8g (printed with -s)."""
    c, f1, smooth, length, seen, open_init, cut_init = oracle_conditions(key)
    ref = c["ref"]
    e = recorded(vs, key)
    assert np.array_equal(e.rollout_lengths(N, T)[0].cpu().numpy(), length)
    cot = cotangents(vs, key, e)
    got = scaled(vs, c, *e.rollout_vjp_rnn(T, **cot))
    # ---- the feedback and the hidden adjoint are there: along the same records the open-loop sweep's d_init is off where the oracle
    # says it must be, and the device's d_init is off from the oracle's with eta cut
    # (state columns only: gpol and eta enter through the observations, which no env hidden state reaches; the hidden rows of both
    # sweeps have their own tests, test_env_hidden_adjoint_against_the_closed_loop_fp64_oracle here and in test_gpu_rollout_vjp.py)
    _, oi = e.rollout_vjp(T, **{k: v for k, v in cot.items() if k not in ("g_act", "g_hid_last")})
    open_got = vs.lanes_first(oi, N).cpu().numpy()[:, :ref.S].astype(np.float64) * np.array(INIT_SCALE[c["name"]])
    cols = slice(T * ref.A, T * ref.A + ref.S)
    tol = block_tolerance(c, f1, smooth)[:, cols]
    full = length == T
    dev_open = float((np.abs(got[:, cols] - open_got) > 10.0 * tol).any(axis=1)[full].mean())
    dev_cut = float((np.abs(got[:, cols] - cut_init) > 10.0 * tol).any(axis=1)[full].mean())
    assert e.error_count() == 0
    e.close()
    worst = worst_in_blocks(c, got, f1, smooth)
    print(f"{key}: gpol seen on {seen[0]:.2f} (oracle) / {dev_open:.2f} (device), eta on {seen[1]:.2f} / {dev_cut:.2f} of the full lanes, "
          f"worst error / tolerance {worst:.4f}")
    assert dev_open >= 0.5 and dev_cut >= 0.5, (key, dev_open, dev_cut)
    assert worst <= 1.0, (key, worst)


HIDDEN_CASES = {"qcp-su": "qcp-su-lstm-33", "qbb": "qbb-lstm-2x64-tanh-out"}


@pytest.mark.parametrize("start", STARTS)
@pytest.mark.parametrize("name", HIDDEN_FAMILIES)
def test_env_hidden_adjoint_against_the_closed_loop_fp64_oracle(vs, name, start):
    """Rows S .. S + H - 1 of d_init -- the adjoint of the ENV's hidden state, which scaled() cuts off: it has another unit and another rule
    than a lane's state columns -- against central differences of the closed loop's Phi at HIDDEN_STEPS x HIDDEN_SCALE, per column and per
    HIDDEN_SCALE, from the hidden state that reset leaves and from hidden_start(); edge lanes like any other, lanes >= n exactly 0.  From
    hidden_start() the first block of test 1 (action offsets, initial state) goes through its check as well: every entry smooth, every
    entry held, the policy inside the box.  Worst error / tolerance per column as measured on the MI355X (printed with -s): DESIGN.md
    section 8d."""
    key = HIDDEN_CASES[name]
    c = case(key)
    g1, g2, length = hidden_reference(key, start)
    hidden_conditions(key, g1, g2)  # from the oracle alone, before the device is asked
    hidden = hidden_start(name, c) if start == "perturbed" else None
    e = recorded(vs, key, hidden=hidden)
    if hidden is None:
        assert np.array_equal(e.rollout_lengths(N, T)[0].cpu().numpy(), length)
    else:
        check_hidden_start(e, hidden, length)
    out = e.rollout_vjp_rnn(T, **cotangents(vs, key, e))
    assert e.error_count() == 0 and e.ld > N and not any(bool(x[..., N:].any()) for x in out)
    e.close()
    check_hidden_block(f"{key} vs_rollout_vjp_rnn from {start}", scaled_hidden(vs, c, out[1]), g1, g2)
    if start == "perturbed":
        r = oracle_reference(key, start)  # (from hidden_start() it is the first block alone)
        f1, smooth = r.f1, smooth_per_lane(r.f1, r.f2)
        assert np.array_equal(r.length, length) and smooth.all(), (key, float((~smooth).mean()))  # from the oracle alone
        check_net_keeps_the_box(c, r.acts, length)
        check_no_unit_near_a_kink(c, r.pres, length)
        worst = worst_of(scaled(vs, c, *out)[:, blocks_of(c)[0]], f1, smooth)
        print(f"{key} from {start}: action offsets and initial state: worst error / tolerance {worst:.4f}")
        assert worst <= 1.0, (key, worst)


def test_exploration_noise_is_an_additive_constant(vs):
    """The LSTM inside a NormalActNoiseExplStrat, handed over as rnn_kernel_spec describes it.  The recorded raw action contains the
    noise: n_t = a_recorded - F_a(obs_recorded, p_recorded), taken from the two record planes in fp64, is fed to the oracle as a
    constant offset; the comparison is test 1's."""
    key = "pend-lstm-8"
    c = case(key)
    ref, cn = c["ref"], c["net"]["cell"]
    env = vs.PendulumSim(max_steps=MAX_STEPS, **KW[c["name"]])
    policy = vs.NormalActNoiseExplStrat(vs.LSTMPolicy(env.spec, cn["hidden"], cn["n_layers"]), std_init=0.02 * ACT_IN[c["name"]])
    policy.policy.param_values = torch.as_tensor(flat_params(c["net"]))
    e = recorded(vs, key, spec=vs.rnn_kernel_spec(policy), noise_seed=77)
    tt = e.traj_tensors(T, N)
    obs, act = tt["obs"].cpu().numpy().astype(np.float64), tt["act"].cpu().numpy().astype(np.float64)  # [T, N, .]
    hid = e.hidden_record_tensor()[:T, :, :N].permute(0, 2, 1).cpu().numpy().astype(np.float64)        # [T, N, Hs]
    mean = rnn_step(cn, obs.reshape(T * N, ref.O), hid.reshape(T * N, c["Hs"]))[0].reshape(T, N, ref.A)
    offs = (act - mean).transpose(1, 0, 2)
    assert 0.5 < offs[N_EDGE:].std() / (0.02 * ACT_IN[c["name"]]) < 1.5  # the noise is there
    r = reference(c, np.ascontiguousarray(offs))
    f1, length, smooth = r.f1, r.length, smooth_per_lane(r.f1, r.f2)
    assert smooth.all()
    assert np.array_equal(e.rollout_lengths(N, T)[0].cpu().numpy(), length)
    got = scaled(vs, c, *e.rollout_vjp_rnn(T, **cotangents(vs, key, e)))
    assert e.error_count() == 0
    e.close()
    worst = worst_in_blocks(c, got, f1, smooth)
    print(f"{key} + noise: worst error / tolerance {worst:.4f}")
    assert worst <= 1.0, worst


# ------------------------------------------------------------------------------------------------- 2. degenerate policy
DEGENERATE = {"omo": "omo-relu-2x3", "bob": "bob-gru-64", "qq-su": "qq-su-gru-2x64", "qcp-su": "qcp-su-lstm-33", "pend": "pend-view-gru-5",
              "qbb": "qbb-lstm-2x64-tanh-out"}


@pytest.mark.parametrize("name", sorted(DEGENERATE))
def test_a_zero_output_layer_reduces_to_the_open_loop_sweep(vs, name):
    """W_out = 0: the action is a constant, gpol is 0 and d_act and d_init equal the open-loop sweep's by value; with g_hid_last = 0 the
    hidden adjoint stays 0"""
    key = DEGENERATE[name]
    net = dict(case(key)["net"])
    net["cell"] = dict(net["cell"], w_out=np.zeros_like(net["cell"]["w_out"]))
    e = recorded(vs, key, net=net)
    cot = cotangents(vs, key, e, with_act=False, with_hid=False)
    oa, oi = e.rollout_vjp(T, **cot)
    pa, pi, ph, ph0 = e.rollout_vjp_rnn(T, **cot)
    assert not torch.isnan(pa).any() and not torch.isnan(pi).any()
    assert bool((pa == oa).all()) and bool((pi == oi).all()) and bool(oa.any()) and bool(oi.any())
    assert not ph.any() and not ph0.any()
    assert e.error_count() == 0
    e.close()


U = 2.0 ** -24       # fp32 unit round-off
TANH_ABS = 2e-7      # tanh_fast's stated absolute error (vecsim_kernels.h; test_gpu_recurrent_policy_fp64.py uses the same figure)
RNN_XP, FNN_XS = 8, 12  # the padded input rows of the two kernels


@pytest.mark.parametrize("key", sorted(ELMAN_AS_FNN))
def test_an_elman_cell_without_recurrence_is_the_fnn_sweep(vs, key):
    """A one-layer Elman tanh cell with W_hh = 0 is the feed-forward network [H] tanh with bias b_ih + b_hh, so vs_rollout_vjp_rnn and
    vs_rollout_vjp_fnn -- two kernels with nothing in common but the env part -- must give the same d_act and d_init up to rounding.

    ONE set of records serves both sweeps: the closed loop is recorded once with the Elman cell and exploration noise (the first K = 12
    rows are swept, as in test_gpu_rollout_vjp.py), vs_rollout_vjp_rnn runs, then the network takes the cell's place on the same handle
    (the records stay) and vs_rollout_vjp_fnn runs.  The same initial states and the same noise, exactly: two recordings by the two
    forward kernels would part in the last bits of the first action and from there along the dynamics, which is no summation rounding
    of a sweep and which no bound of that form covers.

    Reference: the transposed chain in fp64 of vs_step_jac's fp32 Jacobians along the recorded actions (section 8d's; families without
    hidden env state), the policy's Jacobian in fp64 at the recorded observations, the Jacobian of the initial observation read off the
    device (vs_rollout_vjp over one row with unit g_obs[0]: vjp_observe's own entries).  Both sweeps are held to the reference, so their
    difference is at most twice the bound.

    Bound, first order, u = 2^-24; `abs` is the same recursion over magnitudes (section 8d: every product's absolute value, Sigma|terms|),
    e the error, both carried backwards together.  Per live step, with M = S + 1 + O:
      gob = g_obs[t + 1] + gpol          e(gob) = e(gpol) + u abs(gob)                                     (one addition)
      new = J^T (lam, g_rew, gob)        e(new) = |J_s|^T e(lam) + |J_o|^T e(gob) + M u abs(new)           (an fma chain of M terms: 8d)
      abar = new_a + g_act[t]            e(abar) = e(new_a) + u abs(abar)
      z = W_1 x + b, y = tanh z          B(z) = KZ u (sum |w x| + |b_ih| + |b_hh|), KZ = max(RNN_XP + 2, FNN_XS + 1) + 2: the longer of
                                         the two kernels' chains (8 fmas and two additions; the bias and 12 fmas) and 2 u |x| for
                                         E::observe evaluated in another kernel than the one that recorded x;  B(y) = B(z) + TANH_ABS
      g = 1 - y^2 (one fma)              B(g) = 2 |y| B(y) + u g
      d = W_out^T abar                   e(d) = |W_out|^T e(abar) + A u abs(d)                             (A fmas in both kernels)
      delta = d g                        e(delta) = e(d) g + abs(d) (B(g) + u g)
      gx = W_1^T delta                   e(gx) = |W_1|^T e(delta) + KG u abs(gx), KG = max(H, 8): H fmas in the recurrent kernel, a
                                         product and the 6 additions of a wave reduction in the network's, rounded up to 8
    and at the end d_init = lam + J_obs0^T gob (O fmas onto lam): e = e(lam) + |J_obs0|^T e(gob) + (O + 1) u abs(d_init).
    Unrolled, this recursion is section 8d's (L - t) terms u Sigma|terms| with `terms` the largest e / (u abs) of one step; the test
    asserts the recursion itself (never above that closed form) with 8d's factor 1.01 for the second order, and prints the worst ratio
    to it per kernel, the worst |rnn - fnn| / (2 bound) and e / ((L - t) u abs), the `terms` that the recursion amounts to.
    Measured on the MI355X: worst error / bound 0.877 (oscillator) and 0.289 (QQube) for either kernel against
    the reference, |rnn - fnn| / (2 bound) 0.155 and 0.016, terms <= 15.1 and <= 73.9."""
    K = 12
    c = case(key)
    ref, name = c["ref"], c["name"]
    S, A, O = ref.S, ref.A, ref.O
    cn = c["net"]["cell"]
    w, H = cn["layers"][0], cn["hidden"]
    assert ref.H == 0 and cn["cell"] == "tanh" and cn["n_layers"] == 1 and not w["w_hh"].any()
    W1, Wo, bo = w["w_ih"], cn["w_out"], cn["b_out"]  # float32 values in fp64
    b1 = w["b_ih"] + w["b_hh"]                        # (exact in fp64)
    std = [0.02 * ACT_IN[name]] * A
    e = recorded(vs, key, noise_seed=91, noise_std=std)
    tt = e.traj_tensors(K, N)
    obs, act = tt["obs"].cpu().numpy().astype(np.float64), tt["act"].cpu().numpy()  # [K, N, .]
    offs = act - (np.tanh(obs @ W1.T + b1) @ Wo.T + bo)
    assert 0.5 < offs[:, N_EDGE:].std() / (0.02 * ACT_IN[name]) < 1.5  # the noise is in the records
    length = e.rollout_lengths(N, K)[0].cpu().numpy()
    cot = {k: (v if k == "g_state_last" else v[:K + (k == "g_obs")].contiguous()) for k, v in cotangents(vs, key, e, with_hid=False).items()}
    host = lambda x: vs.lanes_first(x, N).cpu().numpy().astype(np.float64)  # noqa: E731
    ra, ri, rh, rh0 = e.rollout_vjp_rnn(K, **cot)
    assert not rh.any() and not rh0.any()  # W_hh = 0 and g_hid_last = 0: no hidden adjoint
    jobs0 = np.zeros((N, O, S))
    for q in range(O):
        g = torch.zeros(2, O, e.ld, device="cuda")
        g[0, q] = 1.0
        jobs0[:, q] = host(e.rollout_vjp(1, g_obs=g)[1])[:, :S]
    e.set_policy_fnn(np.concatenate([W1.reshape(-1), b1, Wo.reshape(-1), bo]).astype(np.float32), [H], hidden_nonlin="tanh", noise_std=std)
    fa, fi = e.rollout_vjp_fnn(K, **cot)
    assert e.error_count() == 0
    e.close()
    got = {"rnn": (host(ra), host(ri)[:, :S]), "fnn": (host(fa), host(fi)[:, :S])}
    # ---- the step Jacobians along the recorded actions
    j = vs.VecSimEnv(name, N, max_steps=MAX_STEPS, **KW[name])
    j.set_auto_reset(False)
    j.set_params(c["params"])
    j.reset(init_state=c["init"])
    jac = [j.step_jac(dev(act[t])) for t in range(K)]
    j.close()
    # ---- the reference, the magnitudes and the error bound, backwards
    g_rew, g_obs, g_act, g_last = (c[k].astype(np.float64) for k in ("g_rew", "g_obs", "g_act", "g_last"))
    M, KZ, KG = S + 1 + O, max(RNN_XP + 2, FNN_XS + 1) + 2, max(H, 8)
    aW1, aWo = np.abs(W1), np.abs(Wo)
    lam, a_lam, e_lam = g_last[:, :S].copy(), np.abs(g_last[:, :S]), np.zeros((N, S))
    gpol, a_gpol, e_gpol = np.zeros((N, O)), np.zeros((N, O)), np.zeros((N, O))
    want_act, a_act, e_act = np.zeros((N, K, A)), np.zeros((N, K, A)), np.zeros((N, K, A))
    for t in range(K - 1, -1, -1):
        js, jr, jo = (jac[t][k].astype(np.float64) for k in ("state", "rew", "obs"))
        gob, a_gob = g_obs[:, t + 1] + gpol, np.abs(g_obs[:, t + 1]) + a_gpol
        e_gob = e_gpol + U * a_gob
        new = np.einsum("nj,njk->nk", lam, js) + g_rew[:, t, None] * jr + np.einsum("nq,nqk->nk", gob, jo)
        a_new = np.einsum("nj,njk->nk", a_lam, np.abs(js)) + np.abs(g_rew[:, t, None] * jr) + np.einsum("nq,nqk->nk", a_gob, np.abs(jo))
        e_new = np.einsum("nj,njk->nk", e_lam, np.abs(js)) + np.einsum("nq,nqk->nk", e_gob, np.abs(jo)) + M * U * a_new
        abar, a_abar = new[:, S:] + g_act[:, t], a_new[:, S:] + np.abs(g_act[:, t])
        e_abar = e_new[:, S:] + U * a_abar
        x = obs[t]
        y = np.tanh(x @ W1.T + b1)
        gd = 1.0 - y * y
        b_z = KZ * U * (np.abs(x) @ aW1.T + np.abs(w["b_ih"]) + np.abs(w["b_hh"]))
        b_g = 2.0 * np.abs(y) * (b_z + TANH_ABS) + U * gd
        d, a_d = abar @ Wo, a_abar @ aWo
        e_d = e_abar @ aWo + A * U * a_d
        delta, a_delta = d * gd, a_d * gd
        e_delta = e_d * gd + a_d * (b_g + U * gd)
        gx, a_gx = delta @ W1, a_delta @ aW1
        e_gx = e_delta @ aW1 + KG * U * a_gx
        on = (t < length)[:, None]  # a lane that ended before step t keeps lambda = g_state_last and gpol = 0
        want_act[:, t], a_act[:, t], e_act[:, t] = np.where(on, abar, 0.0), np.where(on, a_abar, 0.0), np.where(on, e_abar, 0.0)
        lam, a_lam, e_lam = np.where(on, new[:, :S], lam), np.where(on, a_new[:, :S], a_lam), np.where(on, e_new[:, :S], e_lam)
        gpol, a_gpol, e_gpol = np.where(on, gx, gpol), np.where(on, a_gx, a_gpol), np.where(on, e_gx, e_gpol)
    gob, a_gob = g_obs[:, 0] + gpol, np.abs(g_obs[:, 0]) + a_gpol
    e_gob = e_gpol + U * a_gob
    want_init = lam + np.einsum("nq,nqk->nk", gob, jobs0)
    a_init = a_lam + np.einsum("nq,nqk->nk", a_gob, np.abs(jobs0))
    e_init = e_lam + np.einsum("nq,nqk->nk", e_gob, np.abs(jobs0)) + (O + 1) * U * a_init
    steps_left = np.maximum(length[:, None] - np.arange(K)[None, :], 0)
    inside = steps_left > 0
    assert (length[N_EDGE:] == K).mean() > 0.9 and (e_act[inside] > 0).all() and (e_init > 0).all()
    worst = {}
    for which, (d_act, d_init) in got.items():
        assert not d_act[~inside].any()
        worst[which] = max(float((np.abs(d_act - want_act)[inside] / (1.01 * e_act[inside])).max()),
                           float((np.abs(d_init - want_init) / (1.01 * e_init)).max()))
    both = max(float((np.abs(got["rnn"][0] - got["fnn"][0])[inside] / (2.02 * e_act[inside])).max()),
               float((np.abs(got["rnn"][1] - got["fnn"][1]) / (2.02 * e_init)).max()))
    terms = max(float((e_act[inside] / (steps_left[:, :, None] * U * a_act)[inside]).max()), float((e_init / (length[:, None] * U * a_init)).max()))
    feedback = float(np.abs(a_gpol).max())
    print(f"{key}: worst error / bound rnn {worst['rnn']:.3f}, fnn {worst['fnn']:.3f}, |rnn - fnn| / (2 bound) {both:.3f}; the bound is "
          f"(L - t) terms u abs with terms <= {terms:.1f}")
    assert feedback > 0.0  # the policy's pull-back is in the chain
    assert worst["rnn"] <= 1.0 and worst["fnn"] <= 1.0, (key, worst)


# ------------------------------------------------------------------------------------------------------------- 3. edges
@pytest.mark.parametrize("key", ["qq-su-gru-2x64", "qcp-su-lstm-33"])
def test_edges(vs, key):
    L = vs._lib
    c = case(key)
    e = recorded(vs, key)
    cot = cotangents(vs, key, e)
    before = [e.get(getattr(L, b)).copy() for b in STATE_BUFFERS]
    planes, words = e.traj_planes()
    rows = [p.clone() for p, _ in planes] + [words.clone(), e.hidden_record_tensor().clone(), e.policy_hidden().clone()]
    da, di, dh, dh0 = e.rollout_vjp_rnn(T, **cot)
    for b, x in zip(STATE_BUFFERS, before):  # the handle's state, step counter and flags are untouched
        assert np.array_equal(e.get(getattr(L, b)), x), b
    planes, words = e.traj_planes()
    now = [p for p, _ in planes] + [words, e.hidden_record_tensor(), e.policy_hidden()]
    assert all(torch.equal(a, b) for a, b in zip(now, rows)) and e.error_count() == 0  # both record planes and VS_POLICY_HIDDEN
    assert e.ld > N and not any(bool(x[..., N:].any()) for x in (da, di, dh, dh0))  # lanes >= n up to ld: exactly 0
    d_act, d_hid = vs.lanes_first(da, N).cpu().numpy(), vs.lanes_first(dh, N).cpu().numpy()
    length = e.rollout_lengths(N, T)[0].cpu().numpy()
    early = np.flatnonzero(length < T)
    assert early.size > 0 and (early < N_EDGE).all()
    g_hid = c["g_hid"]
    for n in early:
        assert not d_act[n, length[n]:].any() and d_act[n, :length[n]].all()
        assert not d_hid[n, length[n]:].any() and np.array_equal(d_hid[n, length[n] - 1], g_hid[n])  # eta starts as g_hid_last
    assert d_act[length == T].all() and bool(di[:, :N].any(dim=0).all()) and bool(dh0[:, :N].any(dim=0).all())
    assert np.array_equal(d_hid[length == T, T - 1], g_hid[length == T])
    for kw in ({k: torch.zeros_like(v) for k, v in cot.items()}, {}):  # zero cotangents, and none at all
        assert not any(bool(x.any()) for x in e.rollout_vjp_rnn(T, **kw))
    # ---- NULL d_hid / d_hid0: the other two outputs are the same bits
    lib = L.load()
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    order = ("g_rew", "g_obs", "g_act", "g_state_last", "g_hid_last")
    for with_hid, with_hid0 in ((False, False), (True, False), (False, True)):
        a2, i2, h2, h02 = torch.full_like(da, 7.0), torch.full_like(di, 7.0), torch.full_like(dh, 7.0), torch.full_like(dh0, 7.0)
        rc = lib.vs_rollout_vjp_rnn(e._h, T, *[ptr(cot[k]) for k in order], ptr(a2), ptr(i2), ptr(h2) if with_hid else None,
                                    ptr(h02) if with_hid0 else None)
        torch.cuda.synchronize()
        assert rc == L.VS_OK and torch.equal(a2, da) and torch.equal(i2, di)
        assert torch.equal(h2, dh) if with_hid else bool((h2 == 7.0).all())
        assert torch.equal(h02, dh0) if with_hid0 else bool((h02 == 7.0).all())
    # ---- t_steps below the capacity: the sweep over the first 17 rows is the sweep of a 17-step rollout
    short = {k: v[:17 + (k == "g_obs")].contiguous() if k not in ("g_state_last", "g_hid_last") else v for k, v in cot.items()}
    s = e.rollout_vjp_rnn(17, **short)
    assert tuple(s[0].shape) == (17, da.shape[1], e.ld) and tuple(s[2].shape) == (17, c["Hs"], e.ld)
    assert bool(s[0][..., :N].any()) and all(bool(torch.isfinite(x).all()) for x in s)
    f = recorded(vs, key, splits=(17,))
    assert all(torch.equal(a, b) for a, b in zip(f.rollout_vjp_rnn(17, **short), s))
    assert e.error_count() == 0 and f.error_count() == 0
    f.close()
    e.close()


# ---------------------------------------------------------------------------------------------------------- 4. refusals
def test_refusals_leave_the_outputs_untouched(vs):
    L = vs._lib
    lib = L.load()
    key = "pend-view-gru-5"
    c = case(key)
    d = vs.env_dims(c["name"])
    Hs = c["Hs"]
    e = recorded(vs, key)
    outs = [torch.full((T, d["A"], e.ld), 7.0, device="cuda"), torch.full((d["S"] + d["H"], e.ld), 7.0, device="cuda"),
            torch.full((T, Hs, e.ld), 7.0, device="cuda"), torch.full((Hs, e.ld), 7.0, device="cuda")]
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731

    def call(fn, handle, t_steps=T, out=outs):
        extra = (None,) if fn is lib.vs_rollout_vjp_rnn else ()
        tail = [ptr(x) for x in out] if fn is lib.vs_rollout_vjp_rnn else [ptr(out[0]), ptr(out[1])]
        head = (None, None, None) if fn is lib.vs_rollout_vjp else (None, None, None, None)
        rc = fn(handle._h if handle is not None else None, t_steps, *head, *extra, *tail)
        torch.cuda.synchronize()
        return rc

    def refused(code, *args, fn=lib.vs_rollout_vjp_rnn, **kw):
        assert call(fn, *args, **kw) == code
        assert all(bool((x == 7.0).all()) for x in outs)  # the sentinels

    def served():
        assert call(lib.vs_rollout_vjp_rnn, e) == L.VS_OK and not any(bool((x == 7.0).any()) for x in outs)
        for x in outs:
            x.fill_(7.0)

    refused(L.VS_ERR_ARG, None)
    refused(L.VS_ERR_ARG, e, out=[None] + outs[1:])
    refused(L.VS_ERR_ARG, e, out=[outs[0], None] + outs[2:])
    for t_steps in (0, -3, T + 1):
        refused(L.VS_ERR_ARG, e, t_steps)
    for fn in (lib.vs_rollout_vjp_policy, lib.vs_rollout_vjp_fnn):  # the other closed-loop sweeps keep refusing a recurrent policy
        refused(L.VS_ERR_STATE, e, fn=fn)
    e.set_traj_offset(3)
    refused(L.VS_ERR_STATE, e)
    with pytest.raises(RuntimeError):  # the Python face raises
        e.rollout_vjp_rnn(T)
    e.set_traj_offset(0)
    e.set_auto_reset(True)
    refused(L.VS_ERR_STATE, e)
    e.set_auto_reset(False)
    e.set_policy_population(np.tile(flat_params(c["net"])[None, :], (3, 1)), lane_set=np.arange(N) // 64)
    refused(L.VS_ERR_STATE, e)
    e.set_policy_population(None)
    served()                                                    # the same handle still serves
    e.set_policy_hidden_record(0)                               # no hidden-state record plane
    refused(L.VS_ERR_STATE, e)
    e.set_policy_hidden_record(Hs + 1)                          # ... or one of another width
    refused(L.VS_ERR_STATE, e)
    e.set_policy_hidden_record(Hs)
    e.set_policy_rnn(None)                                      # no policy
    refused(L.VS_ERR_STATE, e)
    e.set_policy_linear(np.zeros(d["A"], dtype=np.float32), ["const"])  # a linear policy
    refused(L.VS_ERR_STATE, e)
    e.set_policy_fnn(np.zeros((d["O"] + 1) * 8 + (8 + 1) * d["A"], dtype=np.float32), [8])  # a feed-forward network
    refused(L.VS_ERR_STATE, e)
    e.set_policy_playback(np.zeros((N, T, d["A"]), dtype=np.float32))  # a playback policy
    refused(L.VS_ERR_STATE, e)
    e.close()
    e = recorded(vs, key)                                       # (the plane was dropped and re-made above: fresh records)
    served()
    e.set_record_mode(1)
    e.set_traj_capacity(T)
    refused(L.VS_ERR_STATE, e)
    e.set_record_mode(2)
    e.set_traj_capacity(T)
    served()                                                    # after the refusals the same handle serves a good call
    assert e.error_count() == 0
    e.close()
    disc = vs.VecSimEnv("bob-d", 64, dt=0.01, max_steps=MAX_STEPS)
    disc.set_record_mode(2)
    disc.set_traj_capacity(T)
    o = [torch.full((T, 1, disc.ld), 7.0, device="cuda"), torch.full((4, disc.ld), 7.0, device="cuda")]
    assert lib.vs_rollout_vjp_rnn(disc._h, T, None, None, None, None, None, ptr(o[0]), ptr(o[1]), None, None) == L.VS_ERR_STATE
    torch.cuda.synchronize()
    assert bool((o[0] == 7.0).all()) and bool((o[1] == 7.0).all())
    disc.close()


# ----------------------------------------------------------------------------------------------------------- 5. autograd
def torch_case(name):
    return clc.torch_case("rnn", name)


def oracle_loss(name, flat, s0, length=None):
    """[NT] per-lane loss -discounted return + 1e-3 sum a^2 of the fp64 closed loop under the flat parameters, and the lane lengths"""
    tc = torch_case(name)
    cn = tc["net"]["cell"]
    net = dict(tc["net"], cell=unpack_rnn(flat, cn["cell"], cn["n_layers"], cn["hidden"], tc["ref"].O, tc["ref"].A))
    return clc.oracle_loss(tc, rnn_policy(net), s0, length)


def chosen_entries(name):
    """every parameter of the small policy; of the large one a fixed random 200, at least 20 in each of weight_ih, weight_hh, the two
    biases and the output layer"""
    tc = torch_case(name)
    cn = tc["net"]["cell"]
    n = flat_params(tc["net"]).size
    if name == "pend":
        return np.arange(n)
    rng = np.random.default_rng(41)
    w = cn["layers"][0]
    sizes = [w["w_ih"].size, w["w_hh"].size, w["b_ih"].size, w["b_hh"].size, cn["w_out"].size + cn["b_out"].size]
    assert sum(sizes) == n
    starts = np.concatenate([[0], np.cumsum(sizes)])
    picked = set()
    for s, k in zip(starts, sizes):
        picked |= set((s + rng.choice(k, 20, replace=False)).tolist())
    while len(picked) < 200:
        picked.add(int(rng.integers(n)))
    return np.array(sorted(picked))


@functools.lru_cache(maxsize=None)
def oracle_loss_gradients(name):
    tc = torch_case(name)
    th0, s0 = flat_params(tc["net"]).astype(np.float64), tc["init"].astype(np.float64)
    length = oracle_loss(name, th0, s0)[1]
    which = chosen_entries(name)
    gw, gs = [], []
    for h in (1e-6, 1e-5):
        g = np.zeros(which.size)
        for q, idx in enumerate(which):
            d = np.zeros_like(th0)
            d[idx] = h * abs(th0[idx])
            g[q] = (oracle_loss(name, th0 + d, s0, length)[0].sum() - oracle_loss(name, th0 - d, s0, length)[0].sum()) / (2.0 * h)
        gw.append(g.reshape(1, -1))
        g = np.zeros(s0.shape)
        for j in range(s0.shape[1]):
            d = np.zeros_like(s0)
            d[:, j] = h * INIT_SCALE[name][j]
            g[:, j] = (oracle_loss(name, th0, s0 + d, length)[0] - oracle_loss(name, th0, s0 - d, length)[0]) / (2.0 * h)
        gs.append(g)
    return gw, gs, length


@pytest.mark.parametrize("name", ["pend", "qcp-su"])
def test_autograd(vs, name):
    tc = torch_case(name)
    gw, gs, length = oracle_loss_gradients(name)
    for pair in (gw, gs):
        assert smooth_per_lane(*pair).all()
    cell, n_layers, H = AUTOGRAD[name][:3]
    env = getattr(vs, ENVS[name])(max_steps=MAX_STEPS, **KW[name])
    policy = torch_policy(env.spec, cell, n_layers, H)
    roll = vs.DifferentiableRecurrentRollout(env, policy)
    th0 = flat_params(tc["net"])
    which = chosen_entries(name)
    scale = np.abs(th0.astype(np.float64))

    def loss_of(init):
        obs, rew, act, lengths = roll(init, TT)
        assert tuple(obs.shape) == (NT, TT + 1, tc["ref"].O) and tuple(rew.shape) == (NT, TT) and tuple(act.shape) == (NT, TT, tc["ref"].A)
        assert not lengths.requires_grad and np.array_equal(lengths.cpu().numpy(), length)
        return -vs.discounted_return(rew, lengths, GAMMA).sum() + 1e-3 * act.pow(2).sum()

    def flat_grad(grads):
        return torch.cat([g.reshape(-1) for g in grads]).detach().cpu().numpy().astype(np.float64)

    policy.param_values = torch.as_tensor(th0)
    weights = list(policy.parameters())
    init = dev(tc["init"]).requires_grad_(True)
    loss = loss_of(init)
    g1 = torch.autograd.grad(loss, weights + [init], retain_graph=True)
    with torch.no_grad():
        roll(dev(tc["init"]) * 0.5, TT)  # another forward call overwrites the records
    g2 = torch.autograd.grad(loss, weights + [init])  # the re-record path
    assert all(torch.equal(a, b) for a, b in zip(g1, g2))
    got_w = (flat_grad(g1[:-1]) * scale)[which].reshape(1, -1)
    got_s = g1[-1].cpu().numpy().astype(np.float64) * np.array(INIT_SCALE[name])
    for what, got, (f1, f2) in (("parameters", got_w, gw), ("init_states", got_s, gs)):
        worst = worst_of(got, f1, smooth_per_lane(f1, f2))
        print(f"{name} {what}: worst error / tolerance {worst:.4f}")
        assert worst <= 1.0, (name, what, worst)
    # ---- two steps of plain gradient descent on the parameters (in units of |theta|) lower the oracle's loss; the step size moves no
    # parameter by more than 2 % of its magnitude in the first step
    s0 = tc["init"].astype(np.float64)
    eta = 0.02 / np.abs(flat_grad(g1[:-1]) * scale).max()
    losses = [oracle_loss(name, th0.astype(np.float64), s0, length)[0].sum()]
    for _ in range(2):
        for p in weights:
            p.grad = None
        loss_of(dev(tc["init"])).backward()
        with torch.no_grad():
            step = eta * flat_grad([p.grad for p in weights]) * scale ** 2
            policy.param_values = policy.param_values - torch.as_tensor(step, dtype=torch.float32)
        losses.append(oracle_loss(name, policy.param_values.detach().cpu().numpy().astype(np.float64), s0, length)[0].sum())
    print(f"{name}: oracle loss {losses[0]:.6f} -> {losses[1]:.6f} -> {losses[2]:.6f}")
    assert losses[2] < losses[1] < losses[0], losses
    roll.close()
