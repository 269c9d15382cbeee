"""
Domain-parameter gradients in the reverse-mode playback sweep, the parts that need no GPU: the C-ABI declaration, export and binding
of vs_rollout_vjp_params, its NULL refusal before any device call, and DifferentiableRollout's checks of a parameter tensor.
"""
import ctypes as C
import os
import re

import pytest

import simurlacra_amd as vs
from simurlacra_amd import _lib as L

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_exact_signature():
    header = open(os.path.join(ROOT, "include", "vecsim.h")).read()
    sig = (r"int\s+vs_rollout_vjp_params\(vs_handle h, int t_steps, const float\* g_rew, const float\* g_obs,\s*"
           r"const float\* g_state_last,\s*const int32_t\* param_idx, int n_params,\s*float\* d_act, float\* d_init,\s*"
           r"float\* d_params\);")
    assert re.search(sig, header)
    assert re.search(r"VS_BUFFER_COUNT\s*=\s*31\b", header)  # caller-owned outputs: no new vs_buffer entry
    assert re.search(r"#define VS_SENS_MAX_PARAMS 4\b", header)


def test_symbol_is_exported_bound_and_versioned():
    lib = C.CDLL(L.LIB_PATH)
    assert hasattr(lib, "vs_rollout_vjp_params")
    assert "vs_rollout_vjp_params" in L.exported_symbols()
    assert L.load().vs_version() >= 316
    assert callable(vs.VecSimEnv.rollout_vjp_params)


def test_ctypes_signature_matches_the_prototype():
    res, args = L._SIGNATURES["vs_rollout_vjp_params"]
    p = C.c_void_p
    # handle, t_steps, g_rew, g_obs, g_state_last, param_idx, n_params, d_act, d_init, d_params
    assert res is C.c_int and args == [p, C.c_int, p, p, p, p, C.c_int, p, p, p]
    fn = L.load().vs_rollout_vjp_params
    assert fn.restype is C.c_int and list(fn.argtypes) == args


def test_null_handle_is_refused_before_a_device_is_touched():
    out = (C.c_float * 4)()
    idx = (C.c_int32 * 1)(0)
    assert L.load().vs_rollout_vjp_params(None, 1, None, None, None, idx, 1, out, out, out) == L.VS_ERR_ARG


def test_differentiable_rollout_checks_a_parameter_tensor():
    env = vs.QQubeSwingUpSim(dt=0.004, max_steps=30)
    names = ("motor_resistance", "mass_pend_pole")
    for wrapped in (env, vs.ActNormWrapper(env)):
        roll = vs.DifferentiableRollout(wrapped)
        act, init = torch.zeros(3, 5, 1), torch.zeros(3, 4)
        with pytest.raises(vs.ShapeErr, match="names"):
            roll(act, init, domain_params=torch.ones(3, 2, requires_grad=True))               # a tensor without names=
        with pytest.raises(vs.ShapeErr, match="domain_params"):
            roll(act, init, domain_params=torch.ones(3, 3, requires_grad=True), names=names)  # one column too many
        with pytest.raises(vs.ShapeErr, match="domain_params"):
            roll(act, init, domain_params=torch.ones(2, 2, requires_grad=True), names=names)  # one row per rollout
        with pytest.raises(vs.ShapeErr, match="domain_params"):
            roll(act, init, domain_params=torch.ones(3, requires_grad=True), names=names[:1])
        with pytest.raises(vs.TypeErr, match="float32"):
            roll(act, init, domain_params=torch.ones(3, 2, dtype=torch.float64, requires_grad=True), names=names)
        with pytest.raises(vs.ValueErr, match="repeated"):
            roll(act, init, domain_params=torch.ones(3, 2, requires_grad=True), names=(names[0], names[0]))
        with pytest.raises(vs.ValueErr, match="no_such"):
            roll(act, init, domain_params=torch.ones(3, 2, requires_grad=True), names=("motor_resistance", "no_such"))
        with pytest.raises(vs.TypeErr, match="GPU"):
            roll(act, init, domain_params=torch.ones(3, 2, requires_grad=True), names=names)  # the checks passed: host actions
        assert not roll._vecs  # nothing touched a device
