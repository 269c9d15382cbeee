"""
vs_noise_std_grad without a device: the convention of the sum it forms, pinned against torch autograd on a small closed loop, and the
C-ABI (header, exported symbol, binding, refusals that need no device).

The convention.  a_t = g(K x_t) + sigma (.) eps_t: the noise is added BEHIND the output nonlinearity, as k_rollout_fnn does, and the
sweeps' d_act is the TOTAL adjoint of the raw action a_t -- its direct cotangent plus everything downstream of it, the feedback through
the policy included.  Then d Phi / d sigma = sum over the live rows of abar eps exactly.  A wrong convention is told apart: the adjoint
of the pre-activation K x_t (delta_out = abar g'), which is what a parameter pass forms next and equals abar only for an identity
output; under a saturating tanh it misses by tens of per cent.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import noise_std_grad_cases as nsc
import param_grad_cases as pgc

torch = pytest.importorskip("torch")


def small_loop(out_tanh, seed=5, n=7, T=9, S=3, A=2):
    """a smooth closed loop in torch float64 -> (sigma.grad [A], abar [T, n, A], delta_out [T, n, A], eps [T, n, A], length [n])"""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64)  # noqa: E731
    F, B, K = 0.6 * rnd(S, S), 0.5 * rnd(S, A), 1.5 * rnd(A, S)
    eps, x = rnd(T, n, A), rnd(n, S).requires_grad_(True)  # (the initial state carries a gradient too, as in the sweeps)
    g_obs, g_act = rnd(T + 1, n, S), rnd(T, n, A)
    length = torch.tensor([T, T, 1, 4, T, 2, T - 1][:n])
    sigma = torch.tensor([0.3, 0.2][:A], dtype=torch.float64, requires_grad=True)
    acts, pres = [], []
    phi = (g_obs[0] * x).sum(dim=1)
    for t in range(T):
        pre = x @ K.T
        pre.retain_grad()
        a = (torch.tanh(pre) if out_tanh else pre) + sigma * eps[t]
        a.retain_grad()
        acts.append(a), pres.append(pre)
        x = torch.sin(x @ F.T) + a @ B.T
        live = (t < length).to(torch.float64)
        phi = phi + live * ((g_act[t] * a).sum(dim=1) + 0.1 * (a * a).sum(dim=1) + (g_obs[t + 1] * x).sum(dim=1))
    phi.sum().backward()
    num = lambda xs: torch.stack([v.grad for v in xs]).numpy()  # noqa: E731
    return sigma.grad.numpy(), num(acts), num(pres), eps.numpy(), length.numpy()


@pytest.mark.parametrize("out_tanh", [False, True])
def test_the_sum_is_the_total_adjoint_of_the_raw_action_times_the_noise(out_tanh):
    want, abar, delta, eps, length = small_loop(out_tanh)
    got, lane, mag, _ = nsc.noise_std_grad_np(abar, eps, length)
    assert np.abs(want).min() > 0.1 and (np.abs(got - want) <= 1e-12 * mag).all(), (got, want)
    assert np.allclose(lane.sum(axis=0), got, rtol=1e-13, atol=0.0)
    # the wrong convention: the adjoint of the pre-activation
    wrong = nsc.noise_std_grad_np(delta, eps, length)[0]
    if out_tanh:
        assert (np.abs(wrong - want) > 0.05 * np.abs(want)).all(), (wrong, want)
    else:
        assert np.allclose(wrong, want, rtol=1e-12)  # an identity output: the two are one


def test_rows_behind_a_lanes_end_are_not_read():
    want, abar, _, eps, length = small_loop(True)
    behind = (np.arange(abar.shape[0])[:, None] >= length[None, :])[:, :, None]
    assert behind.any()
    dirty_a, dirty_e = np.where(behind, np.nan, abar), np.where(behind, np.nan, eps)
    a, b = nsc.noise_std_grad_np(abar, eps, length), nsc.noise_std_grad_np(dirty_a, dirty_e, length)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and np.isfinite(b[0]).all()
    # a mask that is one step too long reads them
    assert np.isnan(nsc.noise_std_grad_np(dirty_a, dirty_e, np.minimum(length + 1, abar.shape[0]))[0]).any()


def test_grid_rule_and_chain():
    """a wave per tile up to 16 waves per compute unit, then runs; the chain grows with the run and with the workgroups"""
    assert nsc.noise_grid_of(256, 24, 256) == (24, 1)           # 96 tiles: 24 workgroups of 4 waves, a tile each
    assert nsc.noise_grid_of(256, 1, 256) == (1, 1)
    assert nsc.noise_grid_of(16384, 400, 256) == (1024, 25)     # 102 400 tiles on 4 096 waves
    assert nsc.noise_grid_of(64, 3, 256) == (1, 1)              # three tiles: one workgroup, its fourth wave idle
    assert nsc.chain_of(256, 24, 256) == 1 + 6 + 3 + pgc.reduce_chain(24)
    assert nsc.chain_of(256, 24, 256, 1) == nsc.chain_of(256, 24, 256) + 1
    source = open(os.path.join(pgc.ROOT, "simurlacra_amd", "csrc", "vecsim.hip")).read()
    assert re.search(r"noise_std_grad_wgs\(const vs_env\* h, int t_steps\) \{\s*const int64_t tiles = \(int64_t\)\(h->d\.ld / 64\) \* t_steps;\s*"
                     r"return \(int\)std::min<int64_t>\(\(tiles \+ NSG_WAVES - 1\) / NSG_WAVES, 4 \* \(int64_t\)h->n_cu\);", source)
    kernels = open(os.path.join(pgc.ROOT, "simurlacra_amd", "csrc", "vecsim_kernels.h")).read()
    assert re.search(r"constexpr int NSG_WAVES = 4;", kernels)


# ------------------------------------------------------------------------------------------------- the C-ABI, without a device
ENTRY = "vs_noise_std_grad"


def test_header_declares_the_signature():
    header = open(os.path.join(pgc.ROOT, "include", "vecsim.h")).read()
    assert re.search(rf"int\s+{ENTRY}\(vs_handle h, int t_steps, uint64_t noise_seed, const float\* abar, float\* d_std, int accumulate,\s*"
                     r"float\* d_std_lane, float\* eps\);", header)
    assert "stochastic_action.py:121-180" in header


def test_symbol_is_exported_and_bound():
    import simurlacra_amd as vs
    from simurlacra_amd import _lib as L

    assert hasattr(C.CDLL(L.LIB_PATH), ENTRY) and ENTRY in L.exported_symbols()
    fn = getattr(L.load(), ENTRY)
    assert fn.restype is C.c_int
    assert list(fn.argtypes) == [C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    assert L.load().vs_version() >= 320
    assert callable(vs.VecSimEnv.noise_std_grad) and callable(vs.VecSimEnv.policy_noise)


def test_null_handle_is_refused_whatever_the_pointers():
    from simurlacra_amd import _lib as L

    buf = (C.c_float * 8)()
    fn = getattr(L.load(), ENTRY)
    for ptrs in ((buf, buf, buf, buf), (None, None, None, buf), (buf, None, None, None), (None, None, None, None)):
        assert fn(None, 1, 7, ptrs[0], ptrs[1], 0, ptrs[2], ptrs[3]) == L.VS_ERR_ARG
    assert all(x == 0.0 for x in buf)


def test_the_rollout_classes_take_noise_std():
    import inspect

    import simurlacra_amd as vs
    from simurlacra_amd import diffsim

    for cls in (vs.DifferentiablePolicyRollout, vs.DifferentiableNetRollout, vs.DifferentiableRecurrentRollout):
        p = inspect.signature(cls.__call__).parameters
        assert "noise_std" in p and p["noise_std"].default is None
        assert cls.__call__ is diffsim._ClosedLoopRollout.__call__          # one call for the three
    assert "its std gets no gradient" not in (diffsim.DifferentiablePolicyRollout.__doc__ or "")
