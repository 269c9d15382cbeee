"""
closed_loop_cases.py, without a device: the ONE fp64 closed loop gives the three policy families the same rollout where their policies
coincide.  On the pendulum (150 lanes, the parameters, initial states and cotangents of the linear case "pend-const") the action is the
same constant b under a stack of `const` alone with the weight b, under a network whose output layer has zero weights and the bias b,
and under a recurrent policy with w_out = 0 and b_out = b: states, observations, rewards and actions must be equal bit for bit, and
Phi of the recurrent case with g_hid = 0 must equal Phi of the other two.
"""
import numpy as np

import closed_loop_cases as clc
from derivative_cases import N, T, lengths_of

SHARED = ("name", "ref", "params", "init", "h0", "g_rew", "g_obs", "g_act", "g_last")


def coinciding_cases():
    lin = clc.case("pend-const")
    ref = lin["ref"]
    b = lin["W"].astype(np.float64)[:, 0]  # [A]: the weight of the const feature
    rng = np.random.default_rng(5)
    shared = {k: lin[k] for k in SHARED}
    net = dict(W=[rng.normal(size=(8, ref.O)).astype(np.float32), np.zeros((ref.A, 8), dtype=np.float32)],
               b=[rng.normal(size=8).astype(np.float32), b.astype(np.float32)], hidden_nonlin=("tanh",), output_nonlin=None, feat=False,
               obs_idx=None, hidden=(8,))
    G, H = clc.GATES["gru"], 5
    cell = dict(cell="gru", n_layers=1, hidden=H, w_out=np.zeros((ref.A, H)), b_out=b,
                layers=[dict(w_ih=rng.normal(size=(G * H, ref.O)), w_hh=rng.normal(size=(G * H, H)), b_ih=rng.normal(size=G * H),
                             b_hh=rng.normal(size=G * H))])
    rnn = dict(shared, net=dict(cell=cell, output_nonlin=None, obs_idx=None), g_hid=np.zeros((N, H), dtype=np.float32))
    return lin, dict(shared, net=net), rnn


def test_the_three_families_share_one_rollout_where_their_policies_coincide():
    cases = coinciding_cases()
    lin = cases[0]
    s0, offs = lin["init"].astype(np.float64), np.zeros((N, T, lin["ref"].A))
    rolls = [clc.closed_loop(c["ref"], c["params"].astype(np.float64), s0, c["h0"], clc.policy_of(c), offs) for c in cases]
    assert [r.ps.shape for r in rolls] == [(T + 1, N, 0), (T + 1, N, 0), (T + 1, N, 5)]  # a stateless policy carries a state of width 0
    assert rolls[2].ps[1:].any()  # the recurrent policy does run: only its output layer is silent
    assert rolls[0].states.shape == (T + 1, N, lin["ref"].S) and np.isfinite(rolls[0].states).all()
    for other in rolls[1:]:
        for field in ("states", "hiddens", "obs", "rew", "done", "acts"):
            a, b = getattr(rolls[0], field), getattr(other, field)
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), field
    length = lengths_of(rolls[0].done)
    assert (length < T).any() and (length == T).any()  # lanes that end early, lanes that run through
    phis = [clc.phi(c, s0, offs, length) for c in cases]
    assert np.array_equal(phis[0], phis[1]) and np.array_equal(phis[0], phis[2]) and phis[0].any()
