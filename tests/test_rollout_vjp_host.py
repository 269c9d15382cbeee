"""
Differentiable playback rollouts, the parts that need no GPU: the C-ABI declaration, export and binding of vs_rollout_vjp, its NULL
refusal before any device call, the unchanged buffer count, the layout conversions between [N, T, ...] row-major and the kernels'
time-major struct-of-arrays layout, DifferentiableRollout's argument validation and discounted_return against an fp64 loop.
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
    sig = (r"int\s+vs_rollout_vjp\(vs_handle h, int t_steps, const float\* g_rew, const float\* g_obs, const float\* g_state_last,"
           r"\s*float\* d_act,\s*float\* d_init\);")
    assert re.search(sig, header)
    assert re.search(r"VS_BUFFER_COUNT\s*=\s*31\b", header)  # caller-owned outputs: no new vs_buffer entry


def test_symbol_is_exported_bound_and_versioned():
    lib = C.CDLL(L.LIB_PATH)
    assert hasattr(lib, "vs_rollout_vjp")
    assert "vs_rollout_vjp" in L.exported_symbols()
    assert L.load().vs_version() >= 310
    assert callable(vs.VecSimEnv.rollout_vjp)


def test_null_handle_is_refused_before_a_device_is_touched():
    out = (C.c_float * 4)()
    assert L.load().vs_rollout_vjp(None, 1, None, None, None, out, out) == L.VS_ERR_ARG


@pytest.mark.parametrize("n,ld", [(150, 192), (64, 64), (1, 64), (200, 256)])
def test_layout_conversions_round_trip(n, ld):
    g = torch.Generator().manual_seed(n)
    for shape in ((n, 5), (n, 5, 3), (n, 6, 1)):
        x = torch.randn(*shape, generator=g)
        y = vs.lanes_last(x, ld)
        assert tuple(y.shape) == shape[1:] + (ld,) and y.is_contiguous()
        assert not y[..., n:].any()                      # the padding lanes are 0
        assert torch.equal(y[..., 7 % n], x[7 % n])      # element (lane, t, d) sits at [t, d, lane]
        back = vs.lanes_first(y, n)
        assert torch.equal(back, x) and back.is_contiguous()
    with pytest.raises(vs.ShapeErr):
        vs.lanes_last(torch.zeros(ld + 1, 2), ld)
    with pytest.raises(vs.ShapeErr):
        vs.lanes_first(torch.zeros(2, ld), ld + 1)


def test_differentiable_rollout_refusals():
    assert vs.DifferentiableRollout is __import__("simurlacra_amd.diffsim", fromlist=["x"]).DifferentiableRollout
    with pytest.raises(vs.ValueErr, match="discrete"):
        vs.DifferentiableRollout(vs.BallOnBeamDiscSim(dt=0.01, max_steps=30))
    env = vs.QQubeSwingUpSim(dt=0.004, max_steps=30)
    with pytest.raises(vs.ValueErr, match="GaussianActNoiseWrapper"):
        vs.DifferentiableRollout(vs.GaussianActNoiseWrapper(env, noise_std=np.array([0.1])))
    with pytest.raises(vs.ValueErr):
        vs.DifferentiableRollout(env, batch_lanes=0)
    for wrapped in (env, vs.ActNormWrapper(env)):
        roll = vs.DifferentiableRollout(wrapped)
        with pytest.raises(vs.ShapeErr, match="actions"):
            roll(torch.zeros(3, 5, 2), torch.zeros(3, 4))    # A = 1
        with pytest.raises(vs.ShapeErr, match="actions"):
            roll(torch.zeros(3, 5), torch.zeros(3, 4))
        with pytest.raises(vs.ShapeErr, match="init_states"):
            roll(torch.zeros(3, 5, 1), torch.zeros(3, 6))    # the full state has S = 4 rows
        with pytest.raises(vs.ShapeErr, match="init_states"):
            roll(torch.zeros(3, 5, 1), torch.zeros(2, 4))
        with pytest.raises(vs.ShapeErr, match="domain_params"):
            roll(torch.zeros(3, 5, 1), torch.zeros(3, 4), domain_params=[dict(), dict()])
        with pytest.raises(vs.ValueErr, match="no_such"):
            roll(torch.zeros(3, 5, 1), torch.zeros(3, 4), domain_params=[dict(no_such=1.0)] * 3)
        with pytest.raises(vs.TypeErr):
            roll(torch.zeros(3, 5, 1), torch.zeros(3, 4))    # host tensors
        assert not roll._vecs  # nothing touched a device


def test_discounted_return_against_a_sequential_fp64_loop():
    rng = np.random.default_rng(0)
    n, T = 37, 29
    rew = rng.normal(size=(n, T)).astype(np.float32)
    lengths = rng.integers(0, T + 1, n)
    lengths[:3] = (0, 1, T)
    for gamma in (1.0, 0.99, 0.5, 0.0):
        want = np.zeros(n)
        absum = np.zeros(n)
        for j in range(n):
            y = 0.0
            for t in range(int(lengths[j]) - 1, -1, -1):
                y = float(rew[j, t]) + gamma * y
            want[j] = y
            absum[j] = sum(abs(float(rew[j, t])) * gamma ** t for t in range(int(lengths[j])))
        r = torch.tensor(rew, requires_grad=True)
        got = vs.discounted_return(r, torch.as_tensor(lengths), gamma)
        # fp32: gamma^t by pow (a few ulp), one product and a sum of at most T terms: (T + 8) 2^-24 of the absolute sum
        assert (np.abs(got.detach().numpy().astype(np.float64) - want) <= (T + 8) * 2.0 ** -24 * absum + 1e-30).all(), gamma
        got.sum().backward()
        disc = torch.pow(torch.tensor(gamma, dtype=torch.float32), torch.arange(T, dtype=torch.float32))
        inside = torch.arange(T)[None, :] < torch.as_tensor(lengths)[:, None]
        assert torch.equal(r.grad, torch.where(inside, disc[None, :].expand(n, T), torch.zeros(())))  # gamma^t inside, 0 behind the end
    with pytest.raises(vs.ShapeErr):
        vs.discounted_return(torch.zeros(3, 4), torch.zeros(2, dtype=torch.int64), 0.9)
    with pytest.raises(vs.ValueErr):
        vs.discounted_return(torch.zeros(3, 4), torch.zeros(3, dtype=torch.int64), 1.5)
