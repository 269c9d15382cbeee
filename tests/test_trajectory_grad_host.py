"""
Trajectory-match gradients, the parts that need no GPU: the C-ABI declaration and export of vs_set_rollout_sens, the ctypes
binding and buffer ids, the Python surface (VecSimEnv.set_rollout_sens, TrajectoryMatchSampler.evaluate_grad,
TrajectoryMatchGradResult), evaluate_grad's argument validation, lm_step against a NumPy solve and the upper-triangle expansion.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import simurlacra_amd as vs
from simurlacra_amd import _lib as L
from simurlacra_amd import sysid

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_library_and_binding():
    header = open(os.path.join(ROOT, "include", "vecsim.h")).read()
    assert re.search(r"int\s+vs_set_rollout_sens\(vs_handle h, const int32_t\* param_idx, int n_params\);", header)
    assert re.search(r"#define\s+VS_SENS_MAX_PARAMS\s+4\b", header)
    for name, val in (("VS_ROLLOUT_GRAD", 28), ("VS_ROLLOUT_GN", 29), ("VS_ROLLOUT_SENS", 30), ("VS_BUFFER_COUNT", 31)):
        assert re.search(rf"{name}\s*=\s*{val}\b", header), name
    lib = C.CDLL(L.LIB_PATH)
    assert hasattr(lib, "vs_set_rollout_sens")
    assert "vs_set_rollout_sens" in L.exported_symbols()
    assert (L.VS_ROLLOUT_GRAD, L.VS_ROLLOUT_GN, L.VS_ROLLOUT_SENS, L.VS_SENS_MAX_PARAMS) == (28, 29, 30, 4)
    assert L.load().vs_version() >= 309
    # every pointer is checked before a device is touched
    assert L.load().vs_set_rollout_sens(None, None, 1) == L.VS_ERR_ARG


def test_python_surface():
    assert vs.TrajectoryMatchGradResult is sysid.TrajectoryMatchGradResult
    assert issubclass(vs.TrajectoryMatchGradResult, vs.TrajectoryMatchResult)
    assert callable(vs.TrajectoryMatchSampler.evaluate_grad)
    for m in ("set_rollout_sens", "rollout_grad", "rollout_gn"):
        assert callable(getattr(vs.VecSimEnv, m)), m
    for m in ("grad_per_candidate", "gn_per_candidate", "lm_step"):
        assert callable(getattr(vs.TrajectoryMatchGradResult, m)), m


def sampler():
    env = vs.QQubeSwingUpSim(dt=0.004, max_steps=30)
    acts = [np.zeros((5, 1), dtype=np.float32), np.zeros((3, 1), dtype=np.float32)]
    obs = [np.zeros((6, 6), dtype=np.float32), np.zeros((4, 6), dtype=np.float32)]
    return vs.TrajectoryMatchSampler(env, acts, obs, np.zeros((2, 4), dtype=np.float32))


def test_evaluate_grad_validates_its_arguments_before_any_device_call():
    smp = sampler()
    with pytest.raises(vs.ValueErr, match="no_such_parameter"):
        smp.evaluate_grad([dict()], wrt=("motor_resistance", "no_such_parameter"))
    with pytest.raises(vs.ValueErr, match="repeated"):
        smp.evaluate_grad([dict()], wrt=("motor_resistance", "mass_pend_pole", "motor_resistance"))
    five = ("motor_resistance", "motor_back_emf", "mass_rot_pole", "mass_pend_pole", "length_pend_pole")
    with pytest.raises(vs.ValueErr, match="gauss_newton=False"):
        smp.evaluate_grad([dict()], wrt=five, gauss_newton=True)
    with pytest.raises(vs.ValueErr):
        smp.evaluate_grad([dict()], wrt=())
    assert smp._check_wrt(five, gauss_newton=False) == list(five)  # more than four names: passes of four, gradient only
    assert smp._vec is None  # nothing touched a device


def test_expand_upper_triangle():
    g = 4
    tri = torch.arange(2 * 3 * 10, dtype=torch.float32).reshape(2, 3, 10)
    full = vs.expand_upper_triangle(tri, g)
    assert tuple(full.shape) == (2, 3, g, g)
    assert torch.equal(full, full.transpose(-1, -2))
    q = 0
    for j in range(g):
        for l in range(j, g):  # row-major upper triangle: (0,0) (0,1) .. (0,3) (1,1) ..
            assert torch.equal(full[..., j, l], tri[..., q])
            q += 1
    assert torch.equal(vs.expand_upper_triangle(torch.tensor([[3.0]]), 1), torch.tensor([[[3.0]]]))
    with pytest.raises(vs.ShapeErr):
        vs.expand_upper_triangle(tri, 3)


def test_lm_step_against_numpy():
    rng = np.random.default_rng(0)
    P, R, G = 3, 4, 3
    J = rng.normal(size=(P, R, 7, G))
    gn = np.einsum("prkj,prkl->prjl", J, J)
    grad = rng.normal(size=(P, R, G))
    res = vs.TrajectoryMatchGradResult(torch.zeros(P, R, dtype=torch.float64), torch.ones(P, R, dtype=torch.int64),
                                       torch.as_tensor(grad), torch.as_tensor(gn), ("a", "b", "c"))
    assert np.allclose(res.grad_per_candidate().numpy(), grad.sum(1)) and np.allclose(res.gn_per_candidate().numpy(), gn.sum(1))
    for lam in (0.0, 1e-3, 10.0):
        step = res.lm_step(lam).numpy()
        assert step.shape == (P, G)
        for p in range(P):
            A = gn[p].sum(0)
            want = np.linalg.solve(A + lam * np.diag(np.diag(A)), -0.5 * grad[p].sum(0))
            np.testing.assert_allclose(step[p], want, rtol=1e-9, atol=1e-12)
    no_gn = vs.TrajectoryMatchGradResult(res.loss, res.steps, res.grad, None, res.wrt)
    with pytest.raises(vs.ValueErr):
        no_gn.lm_step(1e-3)
