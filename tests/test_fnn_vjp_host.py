"""
Closed-loop reverse-mode rollouts of feed-forward network policies, the parts that need no GPU: the C-ABI declaration, export and
binding of vs_rollout_vjp_fnn, its NULL refusals before any device call, and DifferentiableNetRollout's argument validation.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import simurlacra_amd as vs
from simurlacra_amd import _lib as L

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_exact_signature():
    header = open(os.path.join(ROOT, "include", "vecsim.h")).read()
    sig = (r"int\s+vs_rollout_vjp_fnn\(vs_handle h, int t_steps, const float\* g_rew, const float\* g_obs, const float\* g_act,"
           r"\s*const float\* g_state_last, float\* d_act, float\* d_init\);")
    assert re.search(sig, header)
    assert re.search(r"VS_BUFFER_COUNT\s*=\s*31\b", header)  # caller-owned outputs: no new vs_buffer entry


def test_symbol_is_exported_and_bound():
    lib = C.CDLL(L.LIB_PATH)
    assert hasattr(lib, "vs_rollout_vjp_fnn")
    assert "vs_rollout_vjp_fnn" in L.exported_symbols()
    fn = L.load().vs_rollout_vjp_fnn
    assert fn.restype is C.c_int and len(fn.argtypes) == 8 and fn.argtypes[1] is C.c_int
    assert L.load().vs_version() >= 313
    assert callable(vs.VecSimEnv.rollout_vjp_fnn)


def test_null_handle_and_null_outputs_are_refused_before_a_device_is_touched():
    out = (C.c_float * 4)()
    fn = L.load().vs_rollout_vjp_fnn
    assert fn(None, 1, None, None, None, None, out, out) == L.VS_ERR_ARG
    assert fn(None, 1, None, None, None, None, None, out) == L.VS_ERR_ARG
    assert fn(None, 1, None, None, None, None, out, None) == L.VS_ERR_ARG
    assert all(x == 0.0 for x in out)


def test_differentiable_net_rollout_refusals():
    assert vs.DifferentiableNetRollout is __import__("simurlacra_amd.diffsim", fromlist=["x"]).DifferentiableNetRollout
    env = vs.QQubeSwingUpSim(dt=0.004, max_steps=30)
    O, A = env.obs_space.flat_dim, env.act_space.flat_dim

    def net(hidden, **kw):
        return vs.FNNPolicy(env.spec, hidden_sizes=hidden, hidden_nonlin=kw.pop("hidden_nonlin", torch.tanh), **kw)

    good = net([8, 5])
    # ---- the policy
    linear = vs.LinearPolicy(env.spec, vs.FeatureStack(vs.identity_feat, vs.const_feat))
    for other in (linear, vs.NormalActNoiseExplStrat(linear, std_init=0.1), vs.GRUPolicy(env.spec, hidden_size=8, num_recurrent_layers=1)):
        with pytest.raises(vs.TypeErr, match="FNN"):
            vs.DifferentiableNetRollout(env, other)
    for bad in (net([8, 8, 8]), net([8, 8, 8, 8]),                      # three and four hidden layers
                net([8], dropout=0.1),                                  # dropout
                net([8], hidden_nonlin=torch.nn.functional.elu),        # a nonlinearity the kernel lacks
                net([8], output_nonlin=torch.nn.functional.softplus),
                net([65])):                                             # wider than a wave
        with pytest.raises(vs.ValueErr):
            vs.DifferentiableNetRollout(env, bad)
    with pytest.raises(vs.ValueErr, match="hidden layers"):
        vs.DifferentiableNetRollout(env, vs.NormalActNoiseExplStrat(net([8, 8, 8]), std_init=0.1))
    oscillator = vs.OneMassOscillatorSim(dt=0.02, max_steps=30)
    with pytest.raises(vs.ShapeErr, match="observation"):
        vs.DifferentiableNetRollout(oscillator, good)
    with pytest.raises(vs.ShapeErr, match="observation"):               # a bare FNN is measured by its layers
        vs.DifferentiableNetRollout(env, vs.FNN(O + 2, A, [8], torch.tanh))
    with pytest.raises(vs.ShapeErr, match="observation"):
        vs.DifferentiableNetRollout(env, vs.FNN(O, A + 1, [8], torch.tanh))
    # ---- the env: DifferentiableRollout's rules
    with pytest.raises(vs.ValueErr, match="discrete"):
        disc = vs.BallOnBeamDiscSim(dt=0.01, max_steps=30)
        vs.DifferentiableNetRollout(disc, vs.FNN(disc.obs_space.flat_dim, disc.act_space.flat_dim, [8], torch.tanh))
    with pytest.raises(vs.ValueErr, match="GaussianActNoiseWrapper"):
        vs.DifferentiableNetRollout(vs.GaussianActNoiseWrapper(env, noise_std=np.array([0.1])), good)
    with pytest.raises(vs.ValueErr):
        vs.DifferentiableNetRollout(env, good, batch_lanes=0)
    # ---- the call
    for policy in (good, net([16], featurize=False), vs.FNN(O, A, [8, 8], torch.relu, output_nonlin=torch.tanh),
                   vs.NormalActNoiseExplStrat(good, std_init=0.1)):
        for wrapped in (env, vs.ActNormWrapper(env)):
            roll = vs.DifferentiableNetRollout(wrapped, policy)
            with pytest.raises(vs.TypeErr, match="torch"):
                roll(np.zeros((3, 4), dtype=np.float32), 5)
            with pytest.raises(vs.ShapeErr, match="init_states"):
                roll(torch.zeros(3, 6), 5)                   # the full state has S = 4 rows
            with pytest.raises(vs.ShapeErr, match="init_states"):
                roll(torch.zeros(3, 4, 1), 5)
            with pytest.raises(vs.ValueErr):
                roll(torch.zeros(3, 4), 0)
            with pytest.raises(vs.ShapeErr, match="domain_params"):
                roll(torch.zeros(3, 4), 5, domain_params=[dict(), dict()])
            with pytest.raises(vs.ValueErr, match="no_such"):
                roll(torch.zeros(3, 4), 5, domain_params=[dict(no_such=1.0)] * 3)
            with pytest.raises(vs.TypeErr):
                roll(torch.zeros(3, 4), 5)                   # a host tensor
            assert not roll._vecs  # nothing touched a device
