"""
What the GPU tests of the derivative kernels share (test_gpu_rollout_vjp*, test_gpu_trajectory_grad, test_gpu_policy_vjp, test_gpu_fnn_vjp,
test_gpu_rnn_vjp, test_gpu_param_derivatives_all, and through param_grad_cases.py the three parameter-gradient tests): the families' tables and shapes, the edge lanes, the fp64
open-loop rollout, the all-parameter oracle, the mode-2 recording launch loop, the playback cotangents and the project's tolerance.
Not a test module: import it by bare name.

The project's tolerance is 3e-3 |g| + 3e-4 max |g_smooth|, an entry smooth where the central differences of the fp64 oracle at
relative steps 1e-6 and 1e-5 agree to 1e-4 (it began in test_step_jacobians_against_finite_differences with one maximum over a whole
Jacobian; that test now applies it per Jacobian position: step_jacobian_cases.py).  `max |g_smooth|` needs entries of ONE unit, and
the derivative tests have three kinds of arrays, hence three rules -- all intended, none a special case of another:

  * per lane (smooth_per_lane, tolerance_per_lane, within_per_lane, worst_of): gradients with respect to action and state columns,
    [N, T A + S (+ hidden entries)], each column scaled by ACT_IN / INIT_SCALE.  The lanes differ by orders of magnitude (an edge lane
    against one at rest), so the maximum is taken over a lane's own row; a lane without a smooth entry gets the floor 1.0.  Users:
    test_gpu_rollout_vjp, test_gpu_policy_vjp, test_gpu_fnn_vjp, test_gpu_rnn_vjp (the last per block of columns).
  * global (smooth_global, within_global): derivatives per unit relative change of a domain parameter, d / d log theta, [N, G] and
    [N, G, G].  That unit is one per FAMILY -- the +-5 % lanes are of one size -- so there is one maximum over the whole array; without a
    mask every entry counts, and with nothing smooth the result is (0.0, 0.0).  Right for a handful of columns of similar size (the
    WRT sets).  Users: test_gpu_rollout_vjp_params, test_gpu_trajectory_grad.
  * per column (smooth_per_column, within_per_column): derivatives with respect to EVERY domain parameter of a family, [N, P], each
    column per PARAM_UNIT of its parameter (|theta|, or 0.1 where theta = 0: the angle offsets and volt thresholds that are 0 at
    nominal).  The columns of one family differ by three orders of magnitude (a damping against a length), so a floor of 3e-4 of the
    family's largest column lets a small column be wrong by tens of per cent; the maximum is taken over a column's own smooth entries
    instead, the lanes of a column being of one size.  The coefficients are the same.  Columns the oracle holds (almost) at zero have
    no unit of their own: null_columns() finds them, NULL_COLUMNS says why each is one, and their callers check them apart.  Right
    whenever the columns are not hand-picked.  Users: test_gpu_param_derivatives_all, test_param_derivative_columns_host.

The hidden env state (the cartpole's previous th_ddot, the ball balancer's two plate angles) is part of the differentiated input of
every reverse-mode sweep, rows S .. S + H - 1 of d_init, and of the carried tangents VS_ROLLOUT_SENS.  Both go by the PER-COLUMN rule
(check_hidden_block, check_tangents), each hidden column per HIDDEN_SCALE, and are NOT further columns of the per-lane rule: inside one
lane the hidden column is not of the size of that lane's state columns.  A cartpole lane's d Phi / d th_ddot_prev -- the Coulomb
friction's normal-force term, d f_normal / d th_ddot_prev = -m_p l_p / 2 sin th -- is between 2e-9 and 1.1e-4 of the lane's largest
state column (median 8e-7), all of it below the lane's floor 3e-4 max |g_smooth|: per lane a sweep that returned 0 or the wrong sign
there would pass (test_hidden_adjoint_host pins that).  Over the lanes the entries of one hidden column ARE of one size, which is
what the per-column floor needs.  The hidden columns also have central-difference steps of their own, HIDDEN_STEPS: see there.
"""
import functools
from typing import NamedTuple

import numpy as np

from oracle import cpu_ref

FAMILIES = ["omo", "bob", "qq-su", "qcp-su", "pend", "qbb"]
KW = {"omo": dict(dt=0.02), "bob": dict(dt=0.01), "qq-su": dict(dt=0.004), "qcp-su": dict(dt=0.002), "pend": dict(dt=0.01),
      "qbb": dict(dt=0.01)}
# action sizes strictly inside every lane's action box (and outside the dead zones): |a| in [0.3, 0.6] of these
ACT_IN = {"omo": 10.0, "bob": 10.0, "qq-su": 4.0, "qcp-su": 5.0, "pend": 3.0, "qbb": 2.5}
# the parameters differentiated (indices into vs_param_name): masses, lengths, motor constants, dampings -- none is 0 at nominal
WRT = {"omo": [0, 1, 2], "bob": [0, 1, 3, 6], "qq-su": [1, 2, 6, 8], "qcp-su": [1, 8, 12, 13], "pend": [0, 1, 2, 3],
       "qbb": [1, 4, 9, 10]}
# full initial states well inside the state space: uniform in +- these
INIT_SCALE = {"omo": [0.5, 1.0], "bob": [0.5, 0.1, 0.3, 0.1], "qq-su": [0.5, 1.0, 2.0, 3.0], "qcp-su": [0.1, 1.0, 0.3, 2.0],
              "pend": [2.0, 2.0], "qbb": [0.1, 0.1, 0.05, 0.05, 0.5, 0.5, 0.1, 0.1]}
# the unit of a hidden column (as INIT_SCALE is the unit of a state column) and the half-width of the non-trivial hidden start: 20 rad/s^2
# of th_ddot_prev keeps the cartpole's normal force positive (the smooth branch), 0.05 rad is the size of the plate angles themselves
HIDDEN_SCALE = {"qcp-su": [20.0], "qbb": [0.05, 0.05]}
# Relative central-difference steps for HIDDEN columns, in units of HIDDEN_SCALE.  NOT the (1e-6, 1e-5) of every other column, and not
# to be unified with them: |Phi| is about 10 and a cartpole entry about 2e-5, so at 1e-6 the difference of two Phi cancels to the last
# three digits of fp64 and half the cartpole entries come out "not smooth" by rounding alone.  Phi is smooth in h_0 on the scale of
# HIDDEN_SCALE (the normal force keeps its sign), so the larger steps cost no truncation error: at (1e-4, 1e-3) every entry is smooth.
HIDDEN_STEPS = (1e-4, 1e-3)
HIDDEN_FAMILIES = ("qcp-su", "qbb")
STARTS = ("reset", "perturbed")  # the hidden state that reset leaves, and hidden_start()
# 150 lanes (three waves, the last one partial), T = 24 steps in launches of 7 + 1 + 16 against one uncut launch, lanes 0 .. 9 at the edge
N, MAX_STEPS, T, SPLITS, N_EDGE = 150, 50, 24, (7, 1, 16), 10
# what a derivative call must leave untouched on the handle
STATE_BUFFERS = ("VS_STATE", "VS_HIDDEN", "VS_OBS", "VS_STEPCOUNT", "VS_DONE", "VS_REW", "VS_RETURNS", "VS_FAILED", "VS_ERRFLAG")
# a tanh output nonlinearity: the pre-activation is +-TANH_OUT_AMP around +-TANH_OUT_AT
TANH_OUT_AT, TANH_OUT_AMP = float(np.arctanh(0.7)), 0.24


# ------------------------------------------------------------------------------------------------------------ the inputs
def edge_states(name, init, n_edge=N_EDGE):
    """lanes 0 .. n_edge - 1 start at the edge of the state space, moving out: they end early"""
    init = init.copy()
    e = slice(0, n_edge)
    if name == "qbb":      # ball near the plate's edge, rolling outwards
        init[e, 2], init[e, 6] = 0.13, 0.45
    elif name == "qq-su":  # arm near its end stop, turning outwards
        init[e, 0], init[e, 2] = 2.0, 5.0
    elif name == "bob":    # ball near the beam's end
        init[e, 0], init[e, 2] = 0.98, 3.0
    elif name == "omo":
        init[e, 0], init[e, 1] = 0.98, 5.0
    elif name == "qcp-su":
        init[e, 0], init[e, 2] = 0.25, 0.6
    else:  # pend
        init[e, 0], init[e, 1] = 12.5, 5.0
    return init


def draw_params_and_init(ref, name, rng):
    """the first two draws of every case(): params [N, P] float32 (+-5 % per lane and parameter around nominal) and init [N, S] float32
    (uniform in +-INIT_SCALE, lanes 0 .. N_EDGE - 1 at the edge)"""
    nominal = ref.nominal_params(1).astype(np.float32)[0]
    params = (nominal[None, :] * (1.0 + 0.05 * rng.uniform(-1.0, 1.0, (N, nominal.size)))).astype(np.float32)
    init = edge_states(name, (rng.uniform(-1.0, 1.0, (N, ref.S)) * np.array(INIT_SCALE[name])).astype(np.float32))
    return params, init


def frozen(c, *more):
    """the case with every array in it (and in `more`) read-only: the tests leave their inputs unchanged"""
    for v in list(c.values()) + list(more):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def reset_hidden(c):
    """[N, H] float64: the hidden state the oracle's reset leaves under the case's parameters and initial states"""
    return c["ref"].reset(c["params"].astype(np.float64), c["init"].astype(np.float64), True)["hidden"]


def hidden_start(name, c):
    """[N, H] float32, read-only: a non-trivial initial hidden state for the case c (ref, params, init), the oracle's reset hidden state
    plus uniform +-HIDDEN_SCALE -- the same draws for every case of a family"""
    h0 = reset_hidden(c)
    out = (h0 + np.random.default_rng(29).uniform(-1.0, 1.0, h0.shape) * np.array(HIDDEN_SCALE[name])).astype(np.float32)
    out.setflags(write=False)
    return out


def start_hidden(name, c, start):
    """[N, H] float64: the oracle's initial hidden state of a start in STARTS"""
    return reset_hidden(c) if start == "reset" else hidden_start(name, c).astype(np.float64)


def playback_case(name):
    """the inputs of a family's playback rollouts, all float32: params [N, P], init [N, S], acts [N, T, A] strictly inside the box and
    outside the dead zones, and the cotangents g_rew [N, T], g_obs [N, T + 1, O], g_last [N, S + H] -> (the case, not yet frozen, and
    the generator it was drawn from, for a caller that draws more)"""
    ref = cpu_ref.make_ref(name, max_steps=MAX_STEPS, **KW[name])
    rng = np.random.default_rng(23)
    params, init = draw_params_and_init(ref, name, rng)
    acts = (ACT_IN[name] * rng.uniform(0.3, 0.6, (N, T, ref.A)) * rng.choice([-1.0, 1.0], (N, T, ref.A))).astype(np.float32)
    c = dict(name=name, ref=ref, params=params, init=init, acts=acts, g_rew=rng.normal(size=(N, T)).astype(np.float32),
             g_obs=rng.normal(size=(N, T + 1, ref.O)).astype(np.float32), g_last=rng.normal(size=(N, ref.S + ref.H)).astype(np.float32))
    return c, rng


@functools.lru_cache(maxsize=None)
def params_case(name):
    """the inputs of a family's domain-parameter derivative tests, all float32 and left unchanged by the tests: playback_case(name),
    and for the forward-mode comparison the residuals resid [N, T + 1, O] (target = recorded observation - resid) and the weights [O]"""
    c, rng = playback_case(name)
    O = c["ref"].O
    c["resid"] = (rng.uniform(0.05, 0.15, (N, T + 1, O)) * rng.choice([-1.0, 1.0], (N, T + 1, O))).astype(np.float32)
    c["weights"] = np.linspace(0.5, 2.0, O).astype(np.float32)
    return frozen(c)


def PARAM_UNIT(name, params):
    """[N, P] float64: the unit a family's domain-parameter derivatives are compared in and its finite differences step by, per lane
    and parameter: |theta|, or 0.1 where theta = 0 (0.1 rad for the angle offsets ang_offset, offset_th_x / _y, 0.1 V for the volt
    thresholds of qq / qcp; `name` is the family, for the caller's record: the rule is the same for all six)"""
    th = np.abs(np.asarray(params, dtype=np.float64))
    return np.where(th != 0.0, th, 0.1)


# ------------------------------------------------------------------------------------------------------- the fp64 oracle
class Rollout(NamedTuple):
    states: np.ndarray   # [T + 1, N, S]
    hiddens: np.ndarray  # [T + 1, N, H]
    obs: np.ndarray      # [T + 1, N, O]
    rew: np.ndarray      # [T, N]
    done: np.ndarray     # [T, N]


def oracle_rollout(ref, params, state0, hidden0, acts):
    """the fp64 oracle along acts [N, T, A] (it does not freeze at done: the caller sums a lane up to its own number of steps)"""
    st, hid = state0.copy(), hidden0.copy()
    states, hiddens, obs, rew, done = [st], [hid], [ref.observe(st)], [], []
    with np.errstate(all="ignore"):
        for t in range(acts.shape[1]):
            out = ref.step(st, hid, acts[:, t], params, np.full(st.shape[0], t))
            st, hid = out["state"], out["hidden"]
            states.append(st), hiddens.append(hid), obs.append(out["obs"]), rew.append(out["rew"]), done.append(out["done"])
    return Rollout(np.stack(states), np.stack(hiddens), np.stack(obs), np.stack(rew), np.stack(done))


def lengths_of(done):
    """[N]: 1 + the first step whose done flag is set, T if none is (done [T, N])"""
    return np.where(done.any(axis=0), done.argmax(axis=0) + 1, done.shape[0])


def phi_and_obs(c, params, params0, state0, hidden0, acts, length):
    """([n]: sum g_rew r + sum g_obs . obs + g_last . (s_L, h_L) of every lane over its first length[n] steps (fp64 oracle) along the
    rollout under `params`, and the observations [T + 1, n, O] of that rollout).  The reward function keeps the constants of params0
    (the project's convention, vecsim_envs.h: the reward FUNCTION, the bounds of the spaces, the initial state and the initial hidden
    state are constants with respect to the parameters; a final reward is a constant of the branch taken and drops out of the
    differences)"""
    ref, n, Tn = c["ref"], state0.shape[0], acts.shape[1]
    states, hiddens, obs, _, _ = oracle_rollout(ref, params, state0, hidden0, acts)
    with np.errstate(all="ignore"):
        rew = np.stack([ref.step_rew(states[t], acts[:, t], params0) for t in range(Tn)])
    k = np.arange(Tn + 1)[:, None]
    out = (np.where(k[:Tn] < length[None, :], c["g_rew"][:n, :Tn].T.astype(np.float64) * rew, 0.0)).sum(axis=0)
    out += np.where((k <= length[None, :])[:, :, None], c["g_obs"][:n, :Tn + 1].transpose(1, 0, 2).astype(np.float64) * obs, 0.0).sum(axis=(0, 2))
    last = np.concatenate([states[length, np.arange(n)], hiddens[length, np.arange(n)]], axis=1)
    return out + (c["g_last"][:n].astype(np.float64) * last).sum(axis=1), obs


def phi(c, params, params0, state0, hidden0, acts, length):
    return phi_and_obs(c, params, params0, state0, hidden0, acts, length)[0]


class ParamOracle(NamedTuple):
    f1: np.ndarray      # [N, P]: d Phi / d theta_j per PARAM_UNIT, central differences at h = 1e-6
    f2: np.ndarray      # [N, P]: the same at h = 1e-5
    gn1: np.ndarray     # [N, P]: sum over rows 1 .. length and q of w_q (d obs_q / d theta_j)^2 per PARAM_UNIT^2, at h = 1e-6
    gn2: np.ndarray     # [N, P]: the same at h = 1e-5
    disc1: np.ndarray   # [N, P]: sum over the same rows of 2 w_q resid_q d obs_q / d theta_j per PARAM_UNIT, at h = 1e-6: the gradient of
    disc2: np.ndarray   # the weighted squared discrepancy against target = obs - resid; [N, P]: the same at h = 1e-5
    length: np.ndarray  # [N]: the oracle's lane lengths
    unit: np.ndarray    # [N, P]: PARAM_UNIT of the case's parameters


@functools.lru_cache(maxsize=None)
def all_param_oracle(name, start="reset"):
    """Central differences of Phi (phi_and_obs, the cotangents of params_case(name)) with respect to EVERY domain parameter of every
    lane, the step h PARAM_UNIT ADDED to the parameter (a relative step cannot move a zero), h = 1e-6 and 1e-5, per PARAM_UNIT; and
    from the same perturbed rollouts the gradient and the diagonal of the Gauss-Newton matrix of the weighted squared discrepancy
    against the target obs - resid under the case's weights.  The initial
    hidden state comes from the oracle's reset under the unperturbed parameters (start = "perturbed": it is hidden_start()) and is
    held; a lane's length is held at its unperturbed value (the branch taken); the actions lie strictly inside every lane's box, so
    a moved bound changes nothing."""
    c = params_case(name)
    ref = c["ref"]
    P0 = c["params"].astype(np.float64)
    s0, a0 = c["init"].astype(np.float64), c["acts"].astype(np.float64)
    h0 = start_hidden(name, c, start)
    length = lengths_of(oracle_rollout(ref, P0, s0, h0, a0).done)
    unit = PARAM_UNIT(name, P0)
    summed = ((np.arange(T + 1)[:, None] >= 1) & (np.arange(T + 1)[:, None] <= length[None, :]))[:, :, None]  # [T + 1, N, 1]
    w = c["weights"].astype(np.float64)[None, None, :]
    resid = c["resid"].astype(np.float64).transpose(1, 0, 2)  # [T + 1, N, O]
    out = []
    for h in (1e-6, 1e-5):
        g, gn, disc = np.zeros(P0.shape), np.zeros(P0.shape), np.zeros(P0.shape)
        for pj in range(P0.shape[1]):
            lo, hi = P0.copy(), P0.copy()
            hi[:, pj] += h * unit[:, pj]
            lo[:, pj] -= h * unit[:, pj]
            (f_hi, o_hi), (f_lo, o_lo) = phi_and_obs(c, hi, P0, s0, h0, a0, length), phi_and_obs(c, lo, P0, s0, h0, a0, length)
            g[:, pj] = (f_hi - f_lo) / (2.0 * h)
            J = np.where(summed, (o_hi - o_lo) / (2.0 * h), 0.0)
            gn[:, pj] = (w * J * J).sum(axis=(0, 2))
            disc[:, pj] = (2.0 * w * resid * J).sum(axis=(0, 2))
        out.append((g, gn, disc))
    (g1, gn1, disc1), (g2, gn2, disc2) = out
    o = ParamOracle(g1, g2, gn1, gn2, disc1, disc2, length, unit)
    for a in o:
        a.setflags(write=False)
    return o


# ------------------------------------------------------------------------------------ the hidden block and the tangents
def hidden_differences(name, f, h0):
    """central differences of f(hidden0) -> [N] with respect to every entry of the initial hidden state h0 [N, H] at the steps
    HIDDEN_STEPS x HIDDEN_SCALE, per HIDDEN_SCALE: two arrays [N, H].  What f holds (lane lengths, a policy's own state, noise) is
    held."""
    out = []
    for h in HIDDEN_STEPS:
        g = np.zeros(h0.shape)
        for j in range(h0.shape[1]):
            d = np.zeros_like(h0)
            d[:, j] = h * HIDDEN_SCALE[name][j]
            g[:, j] = (f(h0 + d) - f(h0 - d)) / (2.0 * h)
        out.append(g)
    return out[0], out[1]


@functools.lru_cache(maxsize=None)
def open_loop_hidden_reference(name, start):
    """the hidden block of the open-loop sweeps (vs_rollout_vjp, vs_rollout_vjp_params) on params_case(name) -- playback_case's draws
    -- from a start in STARTS: hidden_differences of Phi [N, H] x 2, the oracle's lane lengths, and the initial hidden state"""
    c = params_case(name)
    P0, s0, a0 = (c[k].astype(np.float64) for k in ("params", "init", "acts"))
    h0 = start_hidden(name, c, start)
    length = lengths_of(oracle_rollout(c["ref"], P0, s0, h0, a0).done)
    g1, g2 = hidden_differences(name, lambda h: phi(c, P0, P0, s0, h, a0, length), h0)
    return g1, g2, length, h0


def hidden_conditions(tag, g1, g2):
    """what the oracle alone must meet before a device value is looked at -> the smooth mask [N, H]: at most 1 % of the hidden block
    not smooth, and no column without a smooth entry (tolerance_per_column raises on one)"""
    smooth = smooth_per_column(g1, g2)
    assert (~smooth).mean() <= 0.01, (tag, float((~smooth).mean()))
    tolerance_per_column(g1, smooth)
    return smooth


def check_hidden_block(tag, got, g1, g2):
    """got [N, H] (scaled_hidden) against the oracle's hidden block by the per-column rule; prints worst error / tolerance per column"""
    smooth = hidden_conditions(tag, g1, g2)
    assert np.isfinite(got).all(), tag
    bad, worst = within_per_column(got, g1, smooth)
    print(f"{tag}: hidden block: not smooth {(~smooth).mean():.4f}, bad share {bad:.2e}, worst error / tolerance per column "
          + ", ".join(f"{w:.4f}" for w in worst))
    assert bad <= 2e-3, (tag, bad, worst.round(4).tolist())
    return worst


class TangentOracle(NamedTuple):
    f1: np.ndarray      # [N, (S + H) G]: d (s_L, h_L)[j] / d log theta_k in column j G + k, central differences at h = 1e-6
    f2: np.ndarray      # the same at h = 1e-5
    length: np.ndarray  # [N]: the oracle's lane lengths
    theta: np.ndarray   # [N, G]: the WRT parameters of every lane


@functools.lru_cache(maxsize=None)
def tangent_oracle(name):
    """what VS_ROLLOUT_SENS holds after the playback rollout of params_case(name) under the WRT parameters: the state and hidden state
    at the lane's end L per unit relative change of a parameter.  Central differences at relative steps 1e-6 and 1e-5, the initial
    hidden state (the oracle's reset under the unperturbed parameters) and the lane's length held: the kernel's convention."""
    c = params_case(name)
    ref, wrt = c["ref"], WRT[name]
    P0, s0, a0 = (c[k].astype(np.float64) for k in ("params", "init", "acts"))
    h0 = reset_hidden(c)
    length = lengths_of(oracle_rollout(ref, P0, s0, h0, a0).done)
    lanes = np.arange(N)

    def end_of(P):
        r = oracle_rollout(ref, P, s0, h0, a0)
        return np.concatenate([r.states[length, lanes], r.hiddens[length, lanes]], axis=1)  # [N, S + H]

    out = []
    for h in (1e-6, 1e-5):
        g = np.zeros((N, ref.S + ref.H, len(wrt)))
        for k, pk in enumerate(wrt):
            lo, hi = P0.copy(), P0.copy()
            hi[:, pk] *= 1.0 + h
            lo[:, pk] *= 1.0 - h
            g[:, :, k] = (end_of(hi) - end_of(lo)) / (2.0 * h)
        out.append(g.reshape(N, -1))
    o = TangentOracle(out[0], out[1], length, P0[:, wrt])
    for a in o:
        a.setflags(write=False)
    return o


# The (row of (s, h), position in WRT) columns of VS_ROLLOUT_SENS that the oracle holds at zero, under the WRT sets.  Only the ball
# balancer has any, WRT = (ball_mass, arm_radius, motor_back_emf, motor_resistance): in this model the ball does not load the servos,
# th_ddot = (A_m V - B_eq_v th_dot) / J_eq holds neither ball_mass nor arm_radius, so the servo angles (rows 0, 1) and their rates
# (rows 4, 5) have no tangent along either; the plate angles of the hidden state (rows 8, 9) follow the servo angles through
# c_kin = 2 r_arm / l_plate, which leaves them without a tangent along ball_mass alone.  (ball_mass does reach the ball's own rows: it
# does not cancel against the ball's damping term.)
NULL_TANGENTS = {"omo": [], "bob": [], "qq-su": [], "qcp-su": [], "pend": [],
                 "qbb": [(0, 0), (0, 1), (1, 0), (1, 1), (4, 0), (4, 1), (5, 0), (5, 1), (8, 0), (9, 0)]}


def tangents_conditions(name):
    """from the oracle alone -> (the oracle, null [C] bool, smooth [N, live columns]): the null columns are NULL_TANGENTS, at most 1 %
    of the live entries not smooth, no live column without a smooth entry"""
    o = tangent_oracle(name)
    null = null_columns(o.f1, o.f2)
    assert [divmod(int(q), len(WRT[name])) for q in np.flatnonzero(null)] == NULL_TANGENTS[name], name
    live = ~null
    smooth = smooth_per_column(o.f1[:, live], o.f2[:, live])
    assert (~smooth).mean() <= 0.01, (name, float((~smooth).mean()))
    tolerance_per_column(o.f1[:, live], smooth)
    return o, null, smooth


def check_tangents(name, got):
    """got [N, (S + H) G] per unit relative change of the parameter (column j G + k: row j, parameter k) against tangent_oracle by the
    per-column rule, the null columns apart; prints worst error / tolerance per column"""
    o, null, smooth = tangents_conditions(name)
    live = ~null
    assert np.isfinite(got).all(), name
    bad, worst = within_per_column(got[:, live], o.f1[:, live], smooth)
    G = len(WRT[name])
    print(f"{name}: tangents: not smooth {(~smooth).mean():.4f}, bad share {bad:.2e}, worst error / tolerance {worst.max():.4f} at (row, "
          f"parameter) {divmod(int(np.flatnonzero(live)[worst.argmax()]), G)}; null columns {[divmod(int(q), G) for q in np.flatnonzero(null)]}")
    floor = CANCEL_FLOOR * np.abs(o.f1[:, live]).max(axis=0).min()
    if null.any():
        top = float(np.abs(got[:, null]).max())
        print(f"{name}: tangents: largest entry of a null column {top:.3e}, floor {floor:.3e}")
        assert top < floor, (name, top, floor)
    assert bad <= 2e-3, (name, bad, worst.round(3).tolist())
    return worst


def action_window(name, output_nonlin):
    """(lo, hi) of |a| under a network policy made as the FNN and RNN test modules make theirs: section 8e's box, or the tanh output's"""
    return (0.51, 0.83) if output_nonlin == "tanh" else (0.30 * ACT_IN[name], 0.60 * ACT_IN[name])


def check_net_keeps_the_box(c, acts, length):
    """the oracle's actions [T, N, A] inside the lanes' lengths lie in the window of the case's network c["net"]"""
    inside = (np.arange(T)[:, None] < length[None, :])[:, :, None]
    a = np.abs(acts)
    lo, hi = action_window(c["name"], c["net"]["output_nonlin"])
    assert (np.where(inside, a, lo) >= lo).all() and (np.where(inside, a, lo) <= hi).all(), c["name"]


# ------------------------------------------------------------------------------------------------------------ the device
def dev(x):
    import torch

    return torch.as_tensor(np.array(x)).cuda()  # (a copy: the case arrays are read-only)


def record_mode2(e, capacity, params, set_policy, init, splits, hidden=None, **step_kw):
    """rows 0 .. sum(splits) - 1 of the handle e hold the rollouts under the policy that set_policy(e) installs, from init under params,
    recorded in mode 2 by step_policy(k, record=True, **step_kw) in launches of `splits` steps -> e.  hidden [n, H] float32: the
    initial hidden state in place of the one reset leaves (the caller checks it with check_hidden_start)"""
    e.set_auto_reset(False)
    e.set_record_mode(2)
    e.set_traj_capacity(capacity)
    e.set_params(params)
    set_policy(e)
    e.reset(init_state=init)
    if hidden is not None:
        from simurlacra_amd import _lib as L

        e.put(L.VS_HIDDEN, hidden)
    t0 = 0
    for k in splits:
        e.set_traj_offset(t0)
        e.step_policy(k, record=True, **step_kw)
        t0 += k
    e.set_traj_offset(0)
    return e


def case_cotangents(vs, c, e, t_steps=T, last="g_state_last"):
    """g_rew, g_obs and g_last of the case on the device, lanes last, cut to the handle's lanes and to t_steps; `last`: the keyword
    the entry point has for g_last"""
    return {"g_rew": vs.lanes_last(dev(c["g_rew"][:e.n_envs, :t_steps]), e.ld),
            "g_obs": vs.lanes_last(dev(c["g_obs"][:e.n_envs, :t_steps + 1]), e.ld), last: vs.lanes_last(dev(c["g_last"][:e.n_envs]), e.ld)}


def scaled(vs, c, d_act, d_init, n=N):
    """d_act [T, A, ld] and d_init [S + H, ld] of the device -> [n, T A + S] float64 per unit of the inputs' scales (ACT_IN, INIT_SCALE).
    The hidden rows of d_init are cut off here on purpose: they are no further columns of a lane's row (the module docstring says why)
    and go through scaled_hidden() and check_hidden_block() in a test of their own next to every caller's oracle test."""
    ref, name = c["ref"], c["name"]
    d_act, d_init = vs.lanes_first(d_act, n).cpu().numpy(), vs.lanes_first(d_init, n).cpu().numpy()
    got = np.concatenate([d_act.reshape(n, T * ref.A) * ACT_IN[name], d_init[:, :ref.S] * np.array(INIT_SCALE[name])], axis=1)
    assert np.isfinite(got).all()
    return got.astype(np.float64)


def scaled_hidden(vs, c, d_init, n=N):
    """d_init [S + H, ld] of the device -> [n, H] float64: its hidden rows per HIDDEN_SCALE; lanes >= n of them must hold 0"""
    ref = c["ref"]
    assert not bool(d_init[ref.S:, n:].any())
    got = vs.lanes_first(d_init, n).cpu().numpy()[:, ref.S:].astype(np.float64) * np.array(HIDDEN_SCALE[c["name"]])
    assert got.shape == (n, ref.H) and np.isfinite(got).all()
    return got


def check_hidden_start(e, hidden, length, n=N, t_steps=T):
    """after record_mode2(..., hidden=hidden): row 0 of the mode-2 record holds exactly those bits, and the lanes' lengths are the
    oracle's from the same initial hidden state"""
    row0 = e.traj_tensors(1, n)["hidden"][0].cpu().numpy()
    assert np.array_equal(row0.view(np.uint32), np.asarray(hidden[:n]).view(np.uint32))
    assert np.array_equal(e.rollout_lengths(n, t_steps)[0].cpu().numpy(), length[:n])


# ---------------------------------------------------------------------------------------------- the tolerance, per lane
def smooth_per_lane(g1, g2):
    mag = np.maximum(np.abs(g1), np.abs(g2))
    return np.abs(g1 - g2) <= 1e-4 * mag + 1e-7 * (1 + mag.max(axis=1, keepdims=True))


def tolerance_per_lane(want, smooth):
    top = np.where(smooth, np.abs(want), 0.0).max(axis=1, keepdims=True)
    return 3e-3 * np.abs(want) + 3e-4 * np.where(smooth.any(axis=1, keepdims=True), top, 1.0)


def within_per_lane(got, want, smooth):
    """the project's tolerance per lane on the smooth entries -> (share of bad entries, worst error / tolerance); with no smooth entry
    at all the worst is the maximum of nothing: an error, not a pass"""
    tol = tolerance_per_lane(want, smooth)
    err = np.abs(got - want)
    bad = smooth & (err > tol)
    return float(bad.mean()), float((err[smooth] / tol[smooth]).max())


def worst_of(got, want, smooth):
    """worst error / tolerance over ALL entries, the tolerance per lane"""
    return float((np.abs(got - want) / tolerance_per_lane(want, smooth)).max())


# -------------------------------------------------------------------------------------- the tolerance, one unit per family
def smooth_global(g1, g2):
    mag = np.maximum(np.abs(g1), np.abs(g2))
    return np.abs(g1 - g2) <= 1e-4 * mag + 1e-7 * (1 + mag.max())


def within_global(got, want, smooth=None):
    """the project's tolerance on (smooth) entries -> (share of bad entries, worst error / tolerance)"""
    smooth = np.ones(want.shape, dtype=bool) if smooth is None else smooth
    tol = 3e-3 * np.abs(want) + 3e-4 * (np.abs(want[smooth]).max() if smooth.any() else 1.0)
    err = np.abs(got - want)
    bad = smooth & (err > tol)
    return float(bad.mean()), float((err[smooth] / tol[smooth]).max()) if smooth.any() else 0.0


# -------------------------------------------------------------------------------------- the tolerance, one unit per column
# The columns of an all-parameter array that the oracle holds at (almost) zero, and why.  "exact": the parameter reaches only code
# that runs on float values -- a dead-zone comparison, the bounds of the action or state box -- so no tangent ever leaves
# calc_consts<Dual>: the device column is 0.0 in every lane.  "cancels": the parameter drops out analytically and fp32 tangents
# leave rounding noise: the device column stays below CANCEL_FLOOR x the maximum of the family's smallest non-null column.
NULL_COLUMNS = {
    "omo": {},
    "bob": {2: ("cancels", "ball_radius: zeta_ball = m + J_ball / r^2 with J_ball = 2/5 m r^2, r^2 cancels (C_INV_ZETA_BALL is its only use)")},
    "qq-su": {9: ("exact", "voltage_thold_neg: C_TH_NEG is read by dead_zone's comparison alone"),
              10: ("exact", "voltage_thold_pos: C_TH_POS is read by dead_zone's comparison alone")},
    "qcp-su": {2: ("exact", "rail_length: C_XMAX and C_XDMAX, the state box, and nothing in f_dyn"),
               15: ("exact", "voltage_thold_neg: C_TH_NEG is read by f_dyn's dead-zone comparison alone"),
               16: ("exact", "voltage_thold_pos: C_TH_POS is read by f_dyn's dead-zone comparison alone")},
    "pend": {4: ("exact", "torque_thold: C_AMAX, the action box, and nothing in dynamics")},
    "qbb": {14: ("exact", "voltage_thold_x_pos: C_TXP is read by dead_zone's comparison alone"),
            15: ("exact", "voltage_thold_x_neg: C_TXN is read by dead_zone's comparison alone"),
            16: ("exact", "voltage_thold_y_pos: C_TYP is read by dead_zone's comparison alone"),
            17: ("exact", "voltage_thold_y_neg: C_TYN is read by dead_zone's comparison alone")},
}
NULL_BELOW, CANCEL_FLOOR = 1e-8, 3e-4


def null_columns(f1, f2):
    """[P] bool: the columns whose largest entry is below NULL_BELOW of the array's largest at both step sizes"""
    top1, top2 = np.abs(f1).max(axis=0), np.abs(f2).max(axis=0)
    return (top1 < NULL_BELOW * top1.max()) & (top2 < NULL_BELOW * top2.max())


def smooth_per_column(g1, g2):
    mag = np.maximum(np.abs(g1), np.abs(g2))
    return np.abs(g1 - g2) <= 1e-4 * mag + 1e-7 * (1 + mag.max(axis=0, keepdims=True))


def tolerance_per_column(want, smooth):
    """[N, P]: 3e-3 |g| + 3e-4 x the largest smooth entry of the column (a column without one: an error, not a floor)"""
    if not smooth.any(axis=0).all():
        raise ValueError(f"no smooth entry in columns {np.flatnonzero(~smooth.any(axis=0)).tolist()}")
    return 3e-3 * np.abs(want) + 3e-4 * np.where(smooth, np.abs(want), 0.0).max(axis=0, keepdims=True)


def within_per_column(got, want, smooth):
    """the project's tolerance per column on the smooth entries of [N, P] arrays -> (share of bad entries over the whole array, [P]:
    worst error / tolerance of every column)"""
    tol = tolerance_per_column(want, smooth)
    err = np.abs(got - want)
    bad = smooth & (err > tol)
    return float(bad.mean()), np.where(smooth, err / tol, 0.0).max(axis=0)
