"""
Closed-loop reverse-mode rollouts of recurrent policies, the parts that need no GPU: the C-ABI declaration, export and binding of
vs_rollout_vjp_rnn, its NULL refusals before any device call, DifferentiableRecurrentRollout's argument validation, the NumPy fp64
restatement of the three cells in tests/closed_loop_cases.py, the policy of the recurrent sweep's oracle (held to the torch modules here), and the
convention of the hidden-state adjoint: row t of d_hid is the cotangent of p_{t+1}, and one batched single-step pass over the recorded
(obs_t, p_t) with (abar_t, d_hid[t]) as grad_outputs is the parameter gradient of backpropagation through time.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import simurlacra_amd as vs
from simurlacra_amd import _lib as L

torch = pytest.importorskip("torch")

from closed_loop_cases import hidden_size, rnn_step, torch_policy, unpack_rnn  # noqa: E402  (the fp64 cells)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("cell,n_layers,hidden,out", [("tanh", 1, 1, None), ("relu", 2, 3, None), ("gru", 1, 5, None),
                                                      ("gru", 2, 64, "sigmoid"), ("lstm", 1, 33, None), ("lstm", 2, 64, "tanh")])
def test_numpy_cells_match_the_torch_modules(cell, n_layers, hidden, out):
    env = vs.QQubeSwingUpSim(dt=0.004, max_steps=30)
    O, A = env.obs_space.flat_dim, env.act_space.flat_dim
    torch.manual_seed(3)
    policy = torch_policy(env.spec, cell, n_layers, hidden, {None: None, "tanh": torch.tanh, "sigmoid": torch.sigmoid}[out]).double()
    net = unpack_rnn(policy.param_values.detach().numpy(), cell, n_layers, hidden, O, A)
    rng = np.random.default_rng(5)
    x, p = rng.normal(size=(7, O)), rng.normal(size=(7, policy.hidden_size))
    assert hidden_size(net) == policy.hidden_size
    for _ in range(3):  # the packed state of one step is the input of the next
        act, p_new, _ = rnn_step(net, x, p, out)
        with torch.no_grad():
            ta, tp = policy(torch.as_tensor(x), torch.as_tensor(p))
        assert np.abs(act - ta.numpy()).max() <= 1e-12 and np.abs(p_new - tp.numpy()).max() <= 1e-12
        p = p_new


# --------------------------------------------------------------------------------------------------------- the C-ABI
def test_header_declares_the_exact_signature():
    header = open(os.path.join(ROOT, "include", "vecsim.h")).read()
    sig = (r"int\s+vs_rollout_vjp_rnn\(vs_handle h, int t_steps, const float\* g_rew, const float\* g_obs, const float\* g_act,"
           r"\s*const float\* g_state_last, const float\* g_hid_last,\s*float\* d_act, float\* d_init, float\* d_hid, float\* d_hid0\);")
    assert re.search(sig, header)
    assert re.search(r"VS_BUFFER_COUNT\s*=\s*31\b", header)  # caller-owned outputs: no new vs_buffer entry
    assert "RNN policies have no closed-loop sweep" not in header


def test_symbol_is_exported_and_bound():
    lib = C.CDLL(L.LIB_PATH)
    assert hasattr(lib, "vs_rollout_vjp_rnn")
    assert "vs_rollout_vjp_rnn" in L.exported_symbols()
    fn = L.load().vs_rollout_vjp_rnn
    assert fn.restype is C.c_int and len(fn.argtypes) == 11 and fn.argtypes[1] is C.c_int
    assert L.load().vs_version() >= 314
    assert callable(vs.VecSimEnv.rollout_vjp_rnn)


def test_null_handle_and_null_outputs_are_refused_before_a_device_is_touched():
    out = (C.c_float * 4)()
    fn = L.load().vs_rollout_vjp_rnn
    assert fn(None, 1, None, None, None, None, None, out, out, out, out) == L.VS_ERR_ARG
    assert fn(None, 1, None, None, None, None, None, None, out, None, None) == L.VS_ERR_ARG
    assert fn(None, 1, None, None, None, None, None, out, None, None, None) == L.VS_ERR_ARG
    assert all(x == 0.0 for x in out)


def test_differentiable_recurrent_rollout_refusals():
    assert vs.DifferentiableRecurrentRollout is __import__("simurlacra_amd.diffsim", fromlist=["x"]).DifferentiableRecurrentRollout
    env = vs.QQubeSwingUpSim(dt=0.004, max_steps=30)
    good = vs.GRUPolicy(env.spec, hidden_size=8, num_recurrent_layers=2)
    # ---- the policy
    linear = vs.LinearPolicy(env.spec, vs.FeatureStack(vs.identity_feat, vs.const_feat))
    for other in (linear, vs.NormalActNoiseExplStrat(linear, std_init=0.1), vs.FNNPolicy(env.spec, [8], torch.tanh)):
        with pytest.raises(vs.TypeErr, match="GRUPolicy"):
            vs.DifferentiableRecurrentRollout(env, other)
    for bad in (vs.GRUPolicy(env.spec, hidden_size=8, num_recurrent_layers=2, dropout=0.1),   # dropout
                vs.LSTMPolicy(env.spec, hidden_size=8, num_recurrent_layers=3),               # three layers
                vs.RNNPolicy(env.spec, hidden_size=65, num_recurrent_layers=1),               # wider than the kernel's rows
                vs.GRUPolicy(env.spec, hidden_size=8, num_recurrent_layers=1, output_nonlin=torch.nn.functional.softplus)):
        with pytest.raises(vs.ValueErr):
            vs.DifferentiableRecurrentRollout(env, bad)
        with pytest.raises(vs.ValueErr):
            vs.DifferentiableRecurrentRollout(env, vs.NormalActNoiseExplStrat(bad, std_init=0.1))
    oscillator = vs.OneMassOscillatorSim(dt=0.02, max_steps=30)
    with pytest.raises(vs.ShapeErr, match="observation"):
        vs.DifferentiableRecurrentRollout(oscillator, good)
    # ---- the env: DifferentiableRollout's rules
    with pytest.raises(vs.ValueErr, match="discrete"):
        disc = vs.BallOnBeamDiscSim(dt=0.01, max_steps=30)
        vs.DifferentiableRecurrentRollout(disc, vs.GRUPolicy(disc.spec, hidden_size=8, num_recurrent_layers=1))
    with pytest.raises(vs.ValueErr, match="GaussianActNoiseWrapper"):
        vs.DifferentiableRecurrentRollout(vs.GaussianActNoiseWrapper(env, noise_std=np.array([0.1])), good)
    with pytest.raises(vs.ValueErr):
        vs.DifferentiableRecurrentRollout(env, good, batch_lanes=0)
    # ---- the call
    for policy in (good, vs.LSTMPolicy(env.spec, 64, 2, output_nonlin=torch.tanh), vs.RNNPolicy(env.spec, 3, 1, hidden_nonlin="relu"),
                   vs.NormalActNoiseExplStrat(good, std_init=0.1)):
        for wrapped in (env, vs.ActNormWrapper(env)):
            roll = vs.DifferentiableRecurrentRollout(wrapped, policy)
            with pytest.raises(vs.TypeErr, match="torch"):
                roll(np.zeros((3, 4), dtype=np.float32), 5)
            with pytest.raises(vs.ShapeErr, match="init_states"):
                roll(torch.zeros(3, 6), 5)                   # the full state has S = 4 rows
            with pytest.raises(vs.ValueErr):
                roll(torch.zeros(3, 4), 0)
            with pytest.raises(vs.ShapeErr, match="domain_params"):
                roll(torch.zeros(3, 4), 5, domain_params=[dict(), dict()])
            with pytest.raises(vs.TypeErr):
                roll(torch.zeros(3, 4), 5)                   # a host tensor
            assert not roll._vecs  # nothing touched a device


# ------------------------------------------------------------------------------- the convention of the hidden-state adjoint
@pytest.mark.parametrize("cell,n_layers", [("tanh", 2), ("gru", 1), ("lstm", 2)])
def test_single_step_parameter_pass_reproduces_bptt(cell, n_layers):
    """A closed loop with linear dynamics s' = A s + B a, obs = s, in torch fp64.  Full backpropagation through time gives the
    parameter gradients and, on the way, the total adjoints of every a_t and of every p_{t+1} (what the sweep returns as d_act[t]
    and d_hid[t]: everything downstream of step t, the cotangent of the final hidden state at the last step, step t's own output
    layer not included).  DifferentiableRecurrentRollout._param_grads -- one batched single-step pass over the recorded (obs_t, p_t),
    not sequential in time -- must give the same gradients from them; with the rows of d_hid shifted by one step it does not."""
    env = vs.QQubeSwingUpSim(dt=0.004, max_steps=30)
    S, A, n, T = env.obs_space.flat_dim, env.act_space.flat_dim, 5, 7
    torch.manual_seed(11)
    policy = torch_policy(env.spec, cell, n_layers, 4).double()
    params = list(policy.parameters())
    Am = torch.eye(S, dtype=torch.float64) + 0.1 * torch.randn(S, S, dtype=torch.float64)
    Bm = 0.5 * torch.randn(S, A, dtype=torch.float64)
    g_obs = torch.randn(T + 1, n, S, dtype=torch.float64)
    g_act = torch.randn(T, n, A, dtype=torch.float64)
    g_hid_last = torch.randn(n, policy.hidden_size, dtype=torch.float64)
    s, p = torch.randn(n, S, dtype=torch.float64), policy.init_hidden(n).double()
    obs, hid, acts, nexts = [], [], [], []
    loss = (g_obs[0] * s).sum()
    for t in range(T):
        obs.append(s), hid.append(p)
        a, p = policy(s, p)
        a.retain_grad(), p.retain_grad()
        acts.append(a), nexts.append(p)
        s = s @ Am.T + a @ Bm.T
        loss = loss + (g_obs[t + 1] * s).sum() + (g_act[t] * a).sum()
    loss = loss + (g_hid_last * p).sum()
    loss.backward()
    bptt = [q.grad.clone() for q in params]
    abar = torch.stack([a.grad for a in acts], dim=1)        # [n, T, A]
    d_hid = torch.stack([q.grad for q in nexts], dim=1)      # [n, T, Hs]: row t = the cotangent of p_{t+1}
    assert torch.equal(d_hid[:, T - 1], g_hid_last)          # nothing downstream of the last step but g_hid_last

    roll = vs.DifferentiableRecurrentRollout(env, policy)
    seen = torch.stack(obs, dim=1).detach()
    kept = [(d_hid[:3], torch.stack(hid, dim=1).detach()[:3]), (d_hid[3:], torch.stack(hid, dim=1).detach()[3:])]  # two batches
    got = roll._param_grads(seen, abar, kept)
    for g, want in zip(got, bptt):
        assert torch.allclose(g, want, rtol=1e-10, atol=1e-12)
    shifted = torch.cat([torch.zeros_like(d_hid[:, :1]), d_hid[:, :-1]], dim=1)  # "row t = the cotangent of p_t": the wrong convention
    off = roll._param_grads(seen, abar, [(shifted, torch.stack(hid, dim=1).detach())])
    assert not all(torch.allclose(g, want, rtol=1e-3, atol=1e-6) for g, want in zip(off, bptt))
