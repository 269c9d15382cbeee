"""
What tests/test_gpu_noise_std_grad.py (on the device) and tests/test_noise_std_grad_host.py (without one) share: the NumPy restatement of
vs_noise_std_grad, the launch's grid rule and summation chain, and the cases.  Not a test module: import it by bare name.

The pass.  k_rollout_fnn / k_rollout_rnn / k_rollout_lin form the raw action as a_t = mean_t + sigma (.) eps_t and the closed-loop sweeps
return the TOTAL adjoint abar_t of the raw action, so d Phi / d sigma_j = sum over the live rows (t < L_i, i < n) of abar eps.

The chain.  Per action row the kernel adds `chunk` products into a lane's register (one fmaf, one rounding each), the 64 lanes of a
wave in 6 DPP additions (wave_sum_to_lane63), the four waves of a workgroup in 3, the workgroups' rows in k_fnn_param_reduce's chain, and
`accumulate` is one more.  Any order of fp32 additions in which no term passes through more than k of them is off by at most
gamma(k) sum |terms|, gamma(k) = k u / (1 - k u), u = 2^-24; the per-lane sum is a plain chain of t_steps.
"""
import numpy as np

import param_grad_cases as pgc
from derivative_cases import ACT_IN

U = 2.0 ** -24
NSG_WAVES = 4
# one case per policy kind, and the two-action network: z[0] and z[1] of a draw
CASES = ("qq-su", "pend-8", "qcp-su-lstm-33", "qbb-31x64-tanh-out")
SEEDS = (77, 2 ** 40 + 5)


def noise_grid_of(ld, t_steps, n_cu):
    """noise_std_grad_wgs of simurlacra_amd/csrc/vecsim.hip: a wave per tile while there are fewer tiles than wave slots, else four
    workgroups of four waves per compute unit, each wave a contiguous run of tiles -> (workgroups, products a lane accumulates at most)"""
    tiles = (ld // 64) * t_steps
    n_wg = min(-(-tiles // NSG_WAVES), 4 * n_cu)
    return n_wg, -(-tiles // (NSG_WAVES * n_wg))


def chain_of(ld, t_steps, n_cu, more_adds=0):
    """the additions a term of d_std passes through at most: the lane's run, the wave (6), the workgroup (3), the reduce chain"""
    n_wg, acc = noise_grid_of(ld, t_steps, n_cu)
    return acc + 6 + (NSG_WAVES - 1) + pgc.reduce_chain(n_wg, more_adds)


def gamma(k):
    return k * U / (1.0 - k * U)


def scale_of(c):
    """the unit of a case's actions: ACT_IN, or 1 under a tanh output"""
    net = c.get("net")
    return 1.0 if net is not None and net["output_nonlin"] == "tanh" else ACT_IN[c["name"]]


def sigma_of(c, rel):
    """[A] float32: rel x the case's action unit, the second action row at 3 / 4 of the first (so that the rows can be told apart)"""
    return (rel * scale_of(c) * np.array([1.0, 0.75][:c["ref"].A])).astype(np.float32)


def noise_std_grad_np(abar, eps, length):
    """(d_std [A], d_std_lane [n, A], sum |abar eps| [A], per lane [n, A]) in fp64 of abar, eps [T, n, A] and the lanes' lengths [n]:
    the sum of abar eps over the rows t < length[i]; what the arrays hold behind a lane's end is not read"""
    T = abar.shape[0]
    inside = (np.arange(T)[:, None] < np.asarray(length)[None, :])[:, :, None]
    prod = np.where(inside, np.where(inside, abar, 0.0).astype(np.float64) * np.where(inside, eps, 0.0).astype(np.float64), 0.0)
    return prod.sum(axis=(0, 1)), prod.sum(axis=0), np.abs(prod).sum(axis=(0, 1)), np.abs(prod).sum(axis=0)
