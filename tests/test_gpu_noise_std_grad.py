"""
vs_noise_std_grad / k_noise_std_grad (+ k_fnn_param_reduce): the gradient of the exploration noise's std over the recorded rows of a
handle, VecSimEnv.noise_std_grad / policy_noise and the noise_std= keyword of the three closed-loop rollout classes.

Shapes, policies and seeds are those of the closed-loop sweeps' tests (closed_loop_cases.py: 150 lanes = 64 + 64 + 22, T = 24, +-5 %
per-lane parameters, lanes 0 .. 9 end early), one case per policy kind and the two-action network (noise_std_grad_cases.CASES).

  1. The regenerated noise is the rollout's: mean + sigma eps, the mean in fp64 on the RECORDED observations (and hidden states),
     against the recorded raw actions.  The bound is the one the project's forward-policy fp64 tests hold the mean to -- the linear
     policy 1e-5 (1 + sum |w phi|) (test_gpu_linear_policy), the network twice policy_fp64.forward's first-order bound in the pinned
     '64' shape (test_gpu_policy_fp64), the recurrent policy 1e-5 (1 + |mean|) (test_gpu_recurrent_policy_fp64's flat figure) -- plus
     u |sigma eps| + u |a| for the one fmaf that adds the noise.
  2. The kernel against fp64 on the device's own abar and eps, within gamma(chain) sum |abar eps| (noise_std_grad_cases.chain_of).
  3. End to end: d_std_lane against central differences of the fp64 closed loop under the offsets sigma eps, sigma_j perturbed at
     relative steps 1e-6 and 1e-5 (closed_loop_cases.central), at the project's per-lane tolerance, every lane compared.
  4. The contract (param_grad_cases' shared bodies behind an adapter with their call shape), and the refusals.
  5. Autograd through noise_std= of the three rollout classes.
Worst ratios are printed (-s) and recorded in DESIGN.md 8s.
"""
import ctypes as C
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import closed_loop_cases as clc  # noqa: E402
import noise_std_grad_cases as nsc  # noqa: E402
import param_grad_cases as pgc  # noqa: E402
import policy_fp64  # noqa: E402
from derivative_cases import (KW, MAX_STEPS, N, N_EDGE, T, check_net_keeps_the_box, dev, record_mode2, smooth_per_lane,  # noqa: E402
                              tolerance_per_lane)
from param_grad_cases import n_cu, vs, worst_ratio  # noqa: E402,F401  (vs: the fixture)

U = nsc.U
SEED = nsc.SEEDS[0]
NOISE = types.SimpleNamespace(kind="noise", extra=(), version=320, entry="vs_noise_std_grad", method="std_grad", n_params="_std_n")


class Served:
    """a recorded handle behind the call shape of the parameter-gradient passes -- std_grad(t, abar, out=, accumulate=) and _std_n --
    so that the shared bodies of param_grad_cases take it; everything else is the handle's"""

    def __init__(self, e, seed=SEED):
        self._e, self._seed, self._std_n = e, seed, e.dims["A"]

    def std_grad(self, t, abar, out=None, accumulate=False):
        return self._e.noise_std_grad(t, self._seed, abar, out=out, accumulate=accumulate)

    def __getattr__(self, k):
        return getattr(self._e, k)


def recorded(vs, key, sigma=None, seed=SEED, splits=(T,), n=N, idx0=0, cap=None, shape=None):
    """closed_loop_cases.recorded with an index offset: rows 0 .. sum(splits) - 1 hold the case's rollouts under noise_std = sigma"""
    c = clc.case(key)
    policy = clc.policy_of(c)
    e = vs.VecSimEnv(c["name"], n, max_steps=MAX_STEPS, **KW[c["name"]])

    def install(e):
        policy.install(e, noise_std=sigma)
        e.set_index_offset(idx0)
        if shape is not None:
            e.set_policy_shape(shape)

    rs = lambda x: np.resize(x, (n,) + x.shape[1:])  # noqa: E731
    return record_mode2(e, sum(splits) if cap is None else cap, rs(c["params"]), install, rs(c["init"]), splits, noise_seed=seed)


def lanes_first64(vs, x, n):
    """a device array [t, W, ld] -> [t, n, W] float64"""
    return vs.lanes_first(x, n).cpu().numpy().transpose(1, 0, 2).astype(np.float64)


def lengths(e, n=N, t=T):
    return e.rollout_lengths(n, t)[0].cpu().numpy()


def dense_abar(e, t, seed=11):
    """abar [t, A, ld] on the device: dense, not zero-mean"""
    g = torch.Generator("cuda").manual_seed(seed)
    return 0.3 + torch.randn(t, e.dims["A"], e.ld, device="cuda", generator=g)


def sweep(vs, key, e):
    """the case's closed-loop sweep on the handle -> its returns, d_act first"""
    c = clc.case(key)
    cot = clc.cotangents(vs, key, e)
    if "terms" in c:
        return e.rollout_vjp_policy(T, **cot)
    return e.rollout_vjp_rnn(T, **cot) if "cell" in c["net"] else e.rollout_vjp_fnn(T, **cot)


# ------------------------------------------------------------------------------------------------- 1. the noise is the rollout's
def mean_and_bound(vs, key, e, n, t):
    """(fp64 mean [t n, A] of the case's policy on the recorded rows, the forward-policy bound of the kernel's fp32 mean)"""
    c = clc.case(key)
    obs, _, _ = pgc.rows_of(e, n, t)
    obs64 = obs.astype(np.float64)
    policy = clc.policy_of(c)
    if "terms" in c:
        x = obs64 if c["obs_idx"] is None else obs64[:, list(c["obs_idx"])]
        W = c["W"].astype(np.float64)
        return policy.step(obs64, None)[0], 1e-5 * (1.0 + np.abs(clc.features(c["terms"], x)) @ np.abs(W).T)
    if "cell" in c["net"]:
        mean = policy.step(obs64, pgc.hidden_rows(vs, e, n, t).astype(np.float64))[0]
        return mean, 1e-5 * (1.0 + np.abs(mean))
    net = c["net"]
    spec = policy_fp64.Spec(tuple(net["hidden"]), tuple(net["hidden_nonlin"]), net["output_nonlin"], net["feat"], net["obs_idx"])
    x, bx = policy_fp64.input_rows(obs, spec)
    fw = policy_fp64.forward([W.astype(np.float64) for W in net["W"]], [b.astype(np.float64) for b in net["b"]], spec, x, bx, "64")
    mean = policy.step(obs64, None)[0]
    policy_fp64.assert_restates(fw.act, mean)
    return mean, 2.0 * fw.bound


def check_noise_is_the_rollouts(vs, key, seed, what, **kw):
    c = clc.case(key)
    sigma = nsc.sigma_of(c, 0.05)
    fnn = "terms" not in c and "cell" not in c["net"]
    e = recorded(vs, key, sigma, seed, shape="64" if fnn else None, **kw)
    n, t, A = e.n_envs, T, c["ref"].A
    eps_dev = e.policy_noise(t, seed)
    assert eps_dev.dtype == torch.float32 and tuple(eps_dev.shape) == (t, A, e.ld)
    L = lengths(e, n, t)
    inside = (np.arange(t)[:, None] < L[None, :])
    assert (L[:N_EDGE] < t).any() and e.ld > n
    # ---- exact zeros behind a lane's end and at lanes >= n; inside, draws of a standard normal, the two action rows apart
    assert not bool(eps_dev[:, :, n:].any())
    eps = lanes_first64(vs, eps_dev, n)
    assert not eps[~inside].any() and np.isfinite(eps).all()
    z = eps[inside]
    assert (z != 0.0).all() and abs(z.mean()) < 0.1 and abs(z.std() - 1.0) < 0.1
    assert A == 1 or abs(np.corrcoef(z[:, 0], z[:, 1])[0, 1]) < 0.1
    # ---- mean + sigma eps against the recorded raw actions
    act = e.traj_tensors(t, n)["act"].cpu().numpy().astype(np.float64).reshape(t * n, A)
    mean, bound = mean_and_bound(vs, key, e, n, t)
    noise = sigma.astype(np.float64) * eps.reshape(t * n, A)
    want = mean + noise
    bound = bound + U * np.abs(noise) + U * np.abs(want)
    live = inside.reshape(-1)
    r = worst_ratio(np.abs(act - want)[live], bound[live])
    told = float((np.abs(noise[live]) / bound[live]).min(axis=0).max()), float(np.median(np.abs(noise[live]) / bound[live]))
    print(f"{what}: worst |act - (mean + sigma eps)| / bound {r:.3f}; |sigma eps| / bound: median {told[1]:.0f}")
    assert r <= 1.0 and told[1] > 100.0, (what, r, told)  # (the noise is far above the bound: another draw would not pass)
    return e, eps_dev


@pytest.mark.parametrize("key", nsc.CASES)
def test_regenerated_noise_is_the_rollouts_noise(vs, key):
    e, eps = check_noise_is_the_rollouts(vs, key, nsc.SEEDS[0], key)
    other = e.policy_noise(T, nsc.SEEDS[1])
    assert not torch.equal(other, eps) and torch.equal(e.policy_noise(T, nsc.SEEDS[0]), eps)  # keyed by the seed; the same bits twice
    e.close()


def test_second_seed_index_offset_and_two_launches(vs):
    key = "qbb-31x64-tanh-out"
    e, eps = check_noise_is_the_rollouts(vs, key, nsc.SEEDS[1], key + " seed 2, index offset 1000, launches of 10 + 14", idx0=1000,
                                         splits=(10, 14))
    # ---- the index offset keys the draw: lane i at offset 1000 draws what lane i + 64 draws at offset 936 (wherever both are live)
    f = recorded(vs, key, nsc.sigma_of(clc.case(key), 0.05), nsc.SEEDS[1], idx0=936)
    other = f.policy_noise(T, nsc.SEEDS[1])
    both = (eps[:, :, :N - 64] != 0) & (other[:, :, 64:N] != 0)
    assert bool(both.float().mean() > 0.8) and torch.equal(eps[:, :, :N - 64][both], other[:, :, 64:N][both])
    assert not torch.equal(eps[:, :, :N - 64][both], other[:, :, :N - 64][both])
    f.close()
    e.close()


def test_zero_std_is_served_with_the_keys_noise(vs):
    """a policy set without noise: eps is the noise a launch with this seed WOULD add -- the bits a noisy handle regenerates"""
    key = "pend-8"
    quiet, noisy = recorded(vs, key, None), recorded(vs, key, nsc.sigma_of(clc.case(key), 0.005))
    a, b = quiet.policy_noise(T, SEED), noisy.policy_noise(T, SEED)
    both = (a != 0) & (b != 0)
    assert bool(both[:, :, :N].float().mean() > 0.8) and torch.equal(a[both], b[both])
    g = quiet.noise_std_grad(T, SEED, dense_abar(quiet, T))
    assert bool(torch.isfinite(g).all()) and bool(g.all())
    quiet.close()
    noisy.close()


# ------------------------------------------------------------------------------------------------- 2. the kernel against fp64
def held(vs, e, n, t, abar, seed, what, more_adds=0):
    eps = lanes_first64(vs, e.policy_noise(t, seed), n)
    L = lengths(e, n, t)
    want, want_lane, mag, mag_lane = nsc.noise_std_grad_np(lanes_first64(vs, abar, n), eps, L)
    got, lane = e.noise_std_grad(t, seed, abar, per_lane=True)
    A = e.dims["A"]
    assert got.dtype == torch.float32 and tuple(got.shape) == (A,) and tuple(lane.shape) == (A, e.ld) and got.is_cuda
    assert not bool(lane[:, n:].any()) and e.error_count() == 0
    got, lane = got.cpu().numpy().astype(np.float64), lane[:, :n].t().cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all() and np.isfinite(lane).all()
    chain = nsc.chain_of(e.ld, t, n_cu(), more_adds)
    r = worst_ratio(np.abs(got - want), nsc.gamma(chain) * mag)
    rl = worst_ratio(np.abs(lane - want_lane), nsc.gamma(t) * mag_lane)
    print(f"{what}: worst |kernel - fp64| / bound: d_std {r:.3f} (chain {chain}), d_std_lane {rl:.3f} (chain {t})")
    assert np.abs(want).min() > 0.0 and r <= 1.0 and rl <= 1.0, (what, r, rl)
    assert (lane[L == 0] == 0).all()
    return got


@pytest.mark.parametrize("key", nsc.CASES)
def test_against_fp64_on_the_same_inputs(vs, key):
    """Worst |kernel - fp64| / bound measured on the MI355X (printed with -s): DESIGN.md section 8s."""
    e = recorded(vs, key, nsc.sigma_of(clc.case(key), 0.005))
    held(vs, e, N, T, dense_abar(e, T), SEED, key)
    e.close()


@pytest.mark.parametrize("n,t", [(1, T), (65, T), (N, 1), (1537, 41)])
def test_small_batches_and_runs_of_tiles(vs, n, t):
    """one lane, a second lane group of one lane, one step; 1537 lanes x 41 steps: 28 lane groups are 1148 tiles, and once the grid is
    at its cap a wave's run crosses lane-group boundaries (the lengths and the episode are taken again in mid-run)"""
    key = "qbb-31x64-tanh-out"
    e = recorded(vs, key, nsc.sigma_of(clc.case(key), 0.005), splits=(t,), n=n)
    held(vs, e, n, t, dense_abar(e, t), SEED, f"{key} n={n} T={t}")
    e.close()


def test_a_grid_at_its_cap(vs):
    """9 000 lanes x 130 steps: 18 720 tiles on 4 096 waves (256 compute units), runs of 5 tiles"""
    key, n, t = "pend-8", 9000, 130
    e = recorded(vs, key, nsc.sigma_of(clc.case(key), 0.005), splits=(t,), n=n)
    n_wg, acc = nsc.noise_grid_of(e.ld, t, n_cu())
    if n_cu() == 256:
        assert n_wg == 1024 and acc == 5
    held(vs, e, n, t, dense_abar(e, t), SEED, f"{key} n={n} T={t}")
    e.close()


# ------------------------------------------------------------------------------------------------- 3. against the oracle
@pytest.mark.parametrize("key", nsc.CASES)
def test_per_lane_gradient_against_the_oracle(vs, key):
    """d Phi / d log sigma_j per lane: sigma_j d_std_lane[j] against central differences of the fp64 closed loop's Phi along
    d offs = sigma_j eps[:, :, j].  From the oracle alone: the lanes keep the action box (and no relu unit is near its kink), so every
    lane is smooth and every lane is compared; the gradient is not negligible on at least half the full-length lanes."""
    c = clc.case(key)
    ref, A = c["ref"], c["ref"].A
    sigma = nsc.sigma_of(c, 0.005)
    e = recorded(vs, key, sigma)
    eps = lanes_first64(vs, e.policy_noise(T, SEED), N).transpose(1, 0, 2)  # [N, T, A]
    offs0 = sigma.astype(np.float64) * eps
    s0 = c["init"].astype(np.float64)
    roll = clc.closed_loop(ref, c["params"].astype(np.float64), s0, c["h0"], clc.policy_of(c), offs0)
    length = clc.lengths_of(roll.done)
    assert np.array_equal(lengths(e), length)
    # ---- what the oracle alone must meet
    if "terms" in c:
        clc.check_policy_keeps_the_box(c, roll.acts, length)
    else:
        check_net_keeps_the_box(c, roll.acts, length)
        clc.check_no_unit_near_a_kink(c, roll.pres, length)
    f1, f2 = np.zeros((N, A)), np.zeros((N, A))
    for j in range(A):
        d = np.zeros_like(offs0)
        d[:, :, j] = offs0[:, :, j]                                         # a relative step of sigma_j
        f1[:, j], f2[:, j] = clc.central(c, length, s0, offs0, d_offs=d)
    smooth = smooth_per_lane(f1, f2)
    tol = tolerance_per_lane(f1, smooth)
    assert smooth.all(), (key, float((~smooth).mean()))
    full = length == T
    seen = float((np.abs(f1) > 10.0 * tol).any(axis=1)[full].mean())
    assert seen >= 0.5, (key, seen)                                         # a kernel that returned zeros would not pass
    # ---- the device
    d_act = sweep(vs, key, e)[0]
    g, lane = e.noise_std_grad(T, SEED, d_act, per_lane=True)
    got = lane[:, :N].t().cpu().numpy().astype(np.float64) * sigma.astype(np.float64)
    worst = float((np.abs(got - f1) / tol).max())
    total = float((np.abs(g.cpu().numpy() * sigma - f1.sum(axis=0)) / (3e-3 * np.abs(f1.sum(axis=0)) + 3e-4 * np.abs(f1).sum(axis=0).max())).max())
    print(f"{key}: worst |sigma d_std_lane - oracle| / tolerance {worst:.3f} over {N} lanes ({int(full.sum())} full), d_std {total:.3f}; "
          f"not negligible on {seen:.2f} of the full-length lanes")
    assert np.isfinite(got).all() and worst <= 1.0 and total <= 1.0, (key, worst, total)
    e.close()


# ------------------------------------------------------------------------------------------------- 4. the contract
def test_zero_adjoints_give_zeros(vs):
    key = "qbb-31x64-tanh-out"
    e = recorded(vs, key, nsc.sigma_of(clc.case(key), 0.005))
    pgc.check_zero_adjoints_give_zeros(Served(e), NOISE, T, [e.dims["A"]])
    g, lane = e.noise_std_grad(T, SEED, torch.zeros(T, e.dims["A"], e.ld, device="cuda"), per_lane=True)
    assert not bool(g.any()) and not bool(lane.any())
    e.close()


@pytest.mark.parametrize("key", ["qq-su", "qbb-31x64-tanh-out"])
def test_nan_behind_the_rows_changes_no_bit(vs, key):
    """NaN in abar at every row t >= L, at lanes n .. ld - 1 and in rows t_steps .. of a larger buffer: the same bits as with zeros there"""
    e = recorded(vs, key, nsc.sigma_of(clc.case(key), 0.005))
    ab = dense_abar(e, T)
    pgc.check_nan_behind_the_rows(Served(e), NOISE, N, T, [ab])
    dirty = ab.clone()
    L = e.rollout_lengths(N, T)[0]
    dirty[:, :, :N] = torch.where((torch.arange(T, device="cuda")[:, None] >= L[None, :])[:, None, :], torch.full((), float("nan"), device="cuda"),
                                  dirty[:, :, :N])
    dirty[:, :, N:] = float("nan")
    a, b = e.noise_std_grad(T, SEED, ab, per_lane=True), e.noise_std_grad(T, SEED, dirty, per_lane=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and bool(torch.isfinite(b[1]).all())
    e.close()


def test_two_calls_and_accumulate_are_exact(vs):
    key = "qbb-31x64-tanh-out"
    e = recorded(vs, key, nsc.sigma_of(clc.case(key), 0.005))
    ab = dense_abar(e, T)
    pgc.check_two_calls_and_accumulate(vs, Served(e), NOISE, T, [ab], [ab[:, :, :64].contiguous()], dense=True)
    a, b = e.noise_std_grad(T, SEED, ab, per_lane=True), e.noise_std_grad(T, SEED, ab, per_lane=True)
    assert torch.equal(a[1], b[1]) and torch.equal(a[0], e.noise_std_grad(T, SEED, ab))  # with and without the per-lane sums
    e.close()


@pytest.mark.parametrize("key", ["qq-su", "qcp-su-lstm-33"])
def test_the_handle_is_untouched_and_goes_on_serving(vs, key):
    e = recorded(vs, key, nsc.sigma_of(clc.case(key), 0.005))
    more = (lambda: [e.hidden_record_tensor()]) if "net" in clc.case(key) else (lambda: [])
    steps = e.get(vs._lib.VS_STEPCOUNT).copy()
    pgc.check_the_handle_is_untouched(vs, Served(e), NOISE, T, lambda: sweep(vs, key, e), more)  # straight on the sweep's d_act
    before = [e.get(getattr(vs._lib, b)).copy() for b in pgc.STATE_BUFFERS]
    e.policy_noise(T, SEED)
    torch.cuda.synchronize()
    assert all(np.array_equal(e.get(getattr(vs._lib, b)), x) for b, x in zip(pgc.STATE_BUFFERS, before))
    assert np.array_equal(e.get(vs._lib.VS_STEPCOUNT), steps)
    e.close()


def test_t_steps_below_the_capacity(vs):
    key = "qbb-31x64-tanh-out"
    sigma = nsc.sigma_of(clc.case(key), 0.005)
    e = recorded(vs, key, sigma)
    ab = dense_abar(e, 17)
    short = held(vs, e, N, 17, ab, SEED, key + " 17 of 24 rows")
    f = recorded(vs, key, sigma, splits=(17,))
    assert np.array_equal(f.noise_std_grad(17, SEED, ab).cpu().numpy().astype(np.float64), short)
    assert torch.equal(f.policy_noise(17, SEED), e.policy_noise(17, SEED))
    f.close()
    e.close()


class Raw:
    """the entry point called raw with sentinel-filled outputs: refused(code, ...) leaves every sentinel and names the entry point"""

    def __init__(self, vs, e, t):
        self.vs, self.e, self.t, self.lib = vs, e, t, vs._lib.load()
        A = e.dims["A"]
        self.abar = dense_abar(e, t)
        self.outs = dict(d_std=torch.full((A + 1,), 7.0, device="cuda"), lane=torch.full((A, e.ld), 7.0, device="cuda"),
                         eps=torch.full((t, A, e.ld), 7.0, device="cuda"))

    def call(self, handle, t_steps=None, abar=True, d_std=True, lane=True, eps=True, bufs=None):
        o = bufs or self.outs
        p = lambda on, x: C.c_void_p(x.data_ptr()) if on else None  # noqa: E731
        rc = self.lib.vs_noise_std_grad(handle._h if handle is not None else None, self.t if t_steps is None else t_steps, SEED,
                                        p(abar, o.get("abar", self.abar)), p(d_std, o["d_std"]), 0, p(lane, o["lane"]), p(eps, o["eps"]))
        torch.cuda.synchronize()
        return rc

    def refused(self, code, handle, **kw):
        assert self.call(handle, **kw) == code
        assert all(bool((x == 7.0).all()) for k, x in (kw.get("bufs") or self.outs).items() if k != "abar")  # the sentinels
        if handle is not None:
            assert "vs_noise_std_grad" in self.lib.vs_last_error(handle._h).decode()

    def served(self, **kw):
        A = self.e.dims["A"]
        assert self.call(self.e, **kw) == self.vs._lib.VS_OK
        o = self.outs
        if kw.get("d_std", True):
            assert not bool((o["d_std"][:A] == 7.0).any()) and float(o["d_std"][A]) == 7.0
        for k in ("lane", "eps"):
            assert bool((o[k] != 7.0).all()) == kw.get(k, True)
        for x in o.values():
            x.fill_(7.0)


def test_refusals_leave_the_outputs_untouched(vs):
    key = "qq-su"
    c = clc.case(key)
    e = recorded(vs, key, nsc.sigma_of(c, 0.005))
    L, r = vs._lib, Raw(vs, e, T)
    own = lambda: clc.policy_of(c).install(e, noise_std=nsc.sigma_of(c, 0.005))  # noqa: E731
    r.served()
    r.served(lane=False, eps=False)
    r.served(abar=False, d_std=False, lane=False)                                # the eps-only call
    # ---- arguments
    r.refused(L.VS_ERR_ARG, None)
    r.refused(L.VS_ERR_ARG, e, d_std=False)                                      # NULL d_std next to abar
    r.refused(L.VS_ERR_ARG, e, d_std=False, eps=False)
    r.refused(L.VS_ERR_ARG, e, abar=False)                                       # NULL abar next to d_std
    r.refused(L.VS_ERR_ARG, e, abar=False, d_std=False)                          # ... or next to d_std_lane
    r.refused(L.VS_ERR_ARG, e, abar=False, d_std=False, lane=False, eps=False)   # nothing asked for
    for t_steps in (0, -3, T + 1):
        r.refused(L.VS_ERR_ARG, e, t_steps=t_steps)
    # ---- what vs_rollout_vjp refuses
    e.set_traj_offset(3)
    r.refused(L.VS_ERR_STATE, e)
    e.set_traj_offset(0)
    e.set_auto_reset(True)
    r.refused(L.VS_ERR_STATE, e)
    e.set_auto_reset(False)
    r.served()
    # ---- the policy slot: a population, no policy, a playback policy; every other kind is served
    e.set_policy_population(np.tile(c["W"].reshape(1, -1), ((e.n_envs - 1) // 64 + 1, 1)), lane_set=np.arange(e.n_envs) // 64)
    r.refused(L.VS_ERR_STATE, e)
    e.set_policy_population(None)
    r.served()
    e.set_policy_linear(None, None)
    r.refused(L.VS_ERR_STATE, e)
    d = vs.env_dims(c["name"])
    kinds = pgc.other_kinds(e, d, T)
    kinds["playback"]()
    r.refused(L.VS_ERR_STATE, e)
    for kind in ("fnn", "fnn3", "gru", "linear"):                                # (three hidden layers: no sweep, but the noise is the same)
        kinds[kind]()
        r.served()
    own()
    e.set_record_mode(1)
    e.set_traj_capacity(T)
    r.refused(L.VS_ERR_STATE, e)
    e.set_record_mode(2)
    e.set_traj_capacity(T)
    r.served()                                                                   # after the refusals the same handle serves a good call
    assert e.error_count() == 0
    # ---- the Python face
    ab = r.abar
    with pytest.raises(vs.ShapeErr):
        e.noise_std_grad(T, SEED, ab[:, :, :64].contiguous())
    with pytest.raises(vs.ValueErr):
        e.noise_std_grad(T, SEED, ab, accumulate=True)
    with pytest.raises(vs.ValueErr):
        e.policy_noise(0, SEED)
    e.close()
    # ---- the discrete-action family has no action gradient
    disc = vs.VecSimEnv("bob-d", 64, dt=0.01, max_steps=MAX_STEPS)
    disc.set_record_mode(2)
    disc.set_traj_capacity(T)
    A = disc.dims["A"]
    bufs = dict(abar=torch.zeros(T, A, disc.ld, device="cuda"), d_std=torch.full((A + 1,), 7.0, device="cuda"),
                lane=torch.full((A, disc.ld), 7.0, device="cuda"), eps=torch.full((T, A, disc.ld), 7.0, device="cuda"))
    r.refused(L.VS_ERR_STATE, disc, bufs=bufs)
    disc.close()


# ------------------------------------------------------------------------------------------------- 5. autograd
NT, TT = clc.NT, clc.TT


def autograd_setup(vs, kind):
    """(torch_case, env, torch policy, rollout class) of a kind: the policies of the three parameter-gradient tests' autograd cases"""
    name = {"linear": "qq-su", "fnn": "qq-su", "rnn": "pend"}[kind]
    tc = clc.torch_case(kind, name)
    env = getattr(vs, clc.ENVS[name])(max_steps=MAX_STEPS, **KW[name])
    if kind == "linear":
        policy = vs.LinearPolicy(env.spec, vs.FeatureStack(vs.identity_feat, vs.sin_feat, vs.const_feat, vs.MultFeat((0, 1))))
        with torch.no_grad():
            policy.net.weight.copy_(torch.as_tensor(tc["W"]))
        return name, tc, env, policy, vs.DifferentiablePolicyRollout, clc.linear_policy(clc.SMALL, None, tc["W"])
    if kind == "fnn":
        policy = vs.FNNPolicy(env.spec, hidden_sizes=list(clc.FNN_AUTOGRAD[name]), hidden_nonlin=torch.tanh, featurize=False)
        policy.param_values = torch.as_tensor(clc.flat_params(tc["net"]))
        return name, tc, env, policy, vs.DifferentiableNetRollout, clc.fnn_policy(tc["net"])
    cell, n_layers, H = clc.RNN_AUTOGRAD[name][:3]
    policy = clc.torch_policy(env.spec, cell, n_layers, H)
    policy.param_values = torch.as_tensor(clc.flat_params(tc["net"]))
    return name, tc, env, policy, vs.DifferentiableRecurrentRollout, clc.rnn_policy(tc["net"])


def oracle_loss(tc, policy, s0, offs, length=None):
    """closed_loop_cases.oracle_loss under the action offsets offs [NT, TT, A]"""
    roll = clc.closed_loop(tc["ref"], tc["params"], s0, tc["h0"], policy, offs)
    length = clc.lengths_of(roll.done) if length is None else length
    inside = np.arange(TT)[:, None] < length[None, :]
    disc = clc.GAMMA ** np.arange(TT)[:, None]
    return -np.where(inside, disc * roll.rew, 0.0).sum(axis=0) + 1e-3 * np.where(inside[:, :, None], roll.acts ** 2, 0.0).sum(axis=(0, 2)), length


def loss_of(vs, roll, init, **kw):
    obs, rew, act, lengths = roll(init, TT, **kw)
    return -vs.discounted_return(rew, lengths, clc.GAMMA).sum() + 1e-3 * act.pow(2).sum(), (obs, rew, act, lengths)


@pytest.mark.parametrize("kind", ["linear", "fnn", "rnn"])
@pytest.mark.parametrize("param_pass", ["kernel", "torch"])
def test_autograd_noise_std(vs, kind, param_pass, monkeypatch):
    name, tc, env, policy, cls, policy64 = autograd_setup(vs, kind)
    weights = list(policy.parameters())
    A = tc["ref"].A
    sigma_np = (0.005 * clc.ACT_IN[name] * np.array([1.0, 0.75][:A])).astype(np.float32)
    roll = cls(env, policy, param_pass=param_pass)
    init = dev(tc["init"])
    # ---- before any noise_std= call: the outputs and the weight gradients of a plain call
    loss0, out0 = loss_of(vs, roll, init)
    g0 = torch.autograd.grad(loss0, weights)
    # ---- noise_std=
    sigma = dev(sigma_np).requires_grad_(True)
    loss, out = loss_of(vs, roll, init, noise_std=sigma, noise_seed=SEED)
    assert not torch.equal(out[2], out0[2])                                             # the noise is there
    seen = []
    plain = vs.VecSimEnv.noise_std_grad

    def spy(self, t_steps, noise_seed, abar, out=None, accumulate=False, per_lane=False):
        seen.append((self.n_envs, bool(accumulate), lanes_first64(vs, abar, self.n_envs), lanes_first64(vs, self.policy_noise(t_steps, noise_seed), self.n_envs),
                     lengths(self, self.n_envs, t_steps), self.ld))
        return plain(self, t_steps, noise_seed, abar, out=out, accumulate=accumulate, per_lane=per_lane)

    monkeypatch.setattr(vs.VecSimEnv, "noise_std_grad", spy)
    g = torch.autograd.grad(loss, [sigma] + weights, retain_graph=True)
    again = torch.autograd.grad(loss, [sigma] + weights, retain_graph=True)
    assert all(torch.equal(a, b) for a, b in zip(g, again))                             # backward() twice: the same bits
    assert g[0].shape == sigma.shape and g[0].dtype == torch.float32 and bool(torch.isfinite(g[0]).all())
    assert [s[:2] for s in seen] == [(NT, False)] * 2
    # ---- against central differences of the fp64 closed loop under the offsets sigma eps
    eps = seen[0][3].transpose(1, 0, 2)                                                 # [NT, TT, A]
    s0 = tc["init"].astype(np.float64)
    offs0 = sigma_np.astype(np.float64) * eps
    base, length = oracle_loss(tc, policy64, s0, offs0)
    assert np.array_equal(out[3].cpu().numpy(), length)
    f = np.zeros((2, A))
    for j in range(A):
        d = np.zeros_like(offs0)
        d[:, :, j] = offs0[:, :, j]
        for k, h in enumerate((clc.H1, clc.H2)):
            f[k, j] = (oracle_loss(tc, policy64, s0, offs0 + h * d, length)[0].sum() - oracle_loss(tc, policy64, s0, offs0 - h * d, length)[0].sum()) / (2.0 * h)
    smooth = smooth_per_lane(f[:1], f[1:])
    tol = tolerance_per_lane(f[:1], smooth)
    got = g[0].cpu().numpy().astype(np.float64) * sigma_np
    worst = float((np.abs(got - f[0]) / tol).max())
    print(f"{kind} {param_pass}: sigma d loss / d sigma {got}, oracle {f[0]}, worst error / tolerance {worst:.3f}")
    assert smooth.all() and (np.abs(f[0]) > 10.0 * tol).all() and worst <= 1.0, (kind, worst)
    # ---- three batches accumulate to the one-batch result within the chain bound (rollout n draws env index n's noise in either)
    small = cls(env, policy, batch_lanes=32, param_pass=param_pass)
    seen.clear()
    sigma3 = dev(sigma_np).requires_grad_(True)
    loss3, out3 = loss_of(vs, small, init, noise_std=sigma3, noise_seed=SEED)
    assert all(torch.equal(a, b) for a, b in zip(out3, out))
    g3 = torch.autograd.grad(loss3, [sigma3] + weights)
    assert [s[:2] for s in seen] == [(32, False), (32, True), (6, True)]
    assert np.array_equal(np.concatenate([s[3] for s in seen], axis=1), eps.transpose(1, 0, 2))
    mag = sum(nsc.noise_std_grad_np(s[2], s[3], s[4])[2] for s in seen)
    bound = (nsc.gamma(nsc.chain_of(256, TT, n_cu())) + nsc.gamma(nsc.chain_of(seen[0][5], TT, n_cu()) + 2)) * mag
    r = worst_ratio(np.abs(g3[0].cpu().numpy().astype(np.float64) - g[0].cpu().numpy().astype(np.float64)), bound)
    print(f"{kind} {param_pass}: three batches against one, worst difference / chain bound {r:.3f}")
    assert r <= 1.0, (kind, r)
    small.close()
    monkeypatch.setattr(vs.VecSimEnv, "noise_std_grad", plain)
    # ---- noise_std=None afterwards: the bits of the call made before
    loss1, out1 = loss_of(vs, roll, init)
    g1 = torch.autograd.grad(loss1, weights)
    assert all(torch.equal(a, b) for a, b in zip(out1, out0)) and all(torch.equal(a, b) for a, b in zip(g1, g0))
    roll.close()


def test_noise_std_argument_checks_and_a_scalar(vs):
    name, tc, env, policy, cls, _ = autograd_setup(vs, "fnn")
    roll = cls(env, policy)
    init = dev(tc["init"])
    with pytest.raises(vs.ValueErr):
        roll(init, TT, noise_std=torch.tensor([-0.1]))
    with pytest.raises(vs.ShapeErr):
        roll(init, TT, noise_std=torch.tensor([0.1, 0.1]))
    with pytest.raises(vs.ShapeErr):
        roll(init, TT, noise_std=torch.tensor([[0.1]]))
    with pytest.raises(vs.TypeErr):
        roll(init, TT, noise_std=torch.tensor([0.1], dtype=torch.float64))
    with pytest.raises(vs.TypeErr):
        roll(init, TT, noise_std=0.1)
    # ---- a scalar on the host: broadcast, its gradient comes back on the host; a vector gives the same bits
    s = torch.tensor(0.02, requires_grad=True)
    v = torch.tensor([0.02], device="cuda", requires_grad=True)
    ls, _ = loss_of(vs, roll, init, noise_std=s, noise_seed=SEED)
    lv, _ = loss_of(vs, roll, init, noise_std=v, noise_seed=SEED)
    gs, gv = torch.autograd.grad(ls, s)[0], torch.autograd.grad(lv, v)[0]
    assert gs.shape == s.shape and not gs.is_cuda and gv.is_cuda and float(gs) == float(gv[0]) and float(gs) != 0.0
    # ---- a std that does not require grad is a constant: no pass runs
    const, _ = loss_of(vs, roll, init, noise_std=torch.tensor([0.02]), noise_seed=SEED)
    assert torch.equal(const, lv) and not any(p.grad is not None for p in policy.parameters())
    roll.close()
