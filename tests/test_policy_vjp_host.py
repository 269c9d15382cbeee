"""
Closed-loop reverse-mode rollouts, the parts that need no GPU: the C-ABI declaration, export and binding of vs_rollout_vjp_policy, its
NULL refusals before any device call, and DifferentiablePolicyRollout's argument validation.
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
    sig = (r"int\s+vs_rollout_vjp_policy\(vs_handle h, int t_steps, const float\* g_rew, const float\* g_obs, const float\* g_act,"
           r"\s*const float\* g_state_last, float\* d_act, float\* d_init\);")
    assert re.search(sig, header)
    assert re.search(r"VS_BUFFER_COUNT\s*=\s*31\b", header)  # caller-owned outputs: no new vs_buffer entry


def test_symbol_is_exported_and_bound():
    lib = C.CDLL(L.LIB_PATH)
    assert hasattr(lib, "vs_rollout_vjp_policy")
    assert "vs_rollout_vjp_policy" in L.exported_symbols()
    fn = L.load().vs_rollout_vjp_policy
    assert fn.restype is C.c_int and len(fn.argtypes) == 8 and fn.argtypes[1] is C.c_int
    assert L.load().vs_version() >= 311
    assert callable(vs.VecSimEnv.rollout_vjp_policy)


def test_null_handle_and_null_outputs_are_refused_before_a_device_is_touched():
    out = (C.c_float * 4)()
    fn = L.load().vs_rollout_vjp_policy
    assert fn(None, 1, None, None, None, None, out, out) == L.VS_ERR_ARG
    assert fn(None, 1, None, None, None, None, None, out) == L.VS_ERR_ARG
    assert fn(None, 1, None, None, None, None, out, None) == L.VS_ERR_ARG
    assert all(x == 0.0 for x in out)


def test_differentiable_policy_rollout_refusals():
    assert vs.DifferentiablePolicyRollout is __import__("simurlacra_amd.diffsim", fromlist=["x"]).DifferentiablePolicyRollout
    env = vs.QQubeSwingUpSim(dt=0.004, max_steps=30)
    good = vs.LinearPolicy(env.spec, vs.FeatureStack(vs.identity_feat, vs.sin_feat, vs.const_feat, vs.MultFeat((0, 1))))
    # ---- the policy
    with pytest.raises(vs.TypeErr, match="LinearPolicy"):
        vs.DifferentiablePolicyRollout(env, vs.FNNPolicy(env.spec, hidden_sizes=[8], hidden_nonlin=torch.tanh))
    with pytest.raises(vs.TypeErr, match="LinearPolicy"):
        vs.DifferentiablePolicyRollout(env, vs.NormalActNoiseExplStrat(vs.FNNPolicy(env.spec, hidden_sizes=[8], hidden_nonlin=torch.tanh),
                                                                       std_init=0.1))
    for stack in (vs.FeatureStack(vs.identity_feat, vs.identity_feat),          # an elementwise kind twice
                  vs.FeatureStack(vs.MultFeat((0, 1, 2, 3, 4))),                # five rows
                  vs.FeatureStack(lambda x: x)):                                # not a feature function of the package
        with pytest.raises(vs.ValueErr, match="kernel"):
            vs.DifferentiablePolicyRollout(env, vs.LinearPolicy(env.spec, stack))
    other = vs.OneMassOscillatorSim(dt=0.02, max_steps=30)
    with pytest.raises(vs.ShapeErr, match="observation"):
        vs.DifferentiablePolicyRollout(other, good)
    # ---- the env: DifferentiableRollout's rules
    with pytest.raises(vs.ValueErr, match="discrete"):
        disc = vs.BallOnBeamDiscSim(dt=0.01, max_steps=30)
        vs.DifferentiablePolicyRollout(disc, vs.LinearPolicy(disc.spec, vs.FeatureStack(vs.const_feat)))
    with pytest.raises(vs.ValueErr, match="GaussianActNoiseWrapper"):
        vs.DifferentiablePolicyRollout(vs.GaussianActNoiseWrapper(env, noise_std=np.array([0.1])), good)
    with pytest.raises(vs.ValueErr):
        vs.DifferentiablePolicyRollout(env, good, batch_lanes=0)
    # ---- the call
    for policy in (good, vs.NormalActNoiseExplStrat(good, std_init=0.1)):
        for wrapped in (env, vs.ActNormWrapper(env)):
            roll = vs.DifferentiablePolicyRollout(wrapped, policy)
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
