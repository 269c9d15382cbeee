"""
What the tests of the three parameter-gradient passes share (test_gpu_fnn_param_grad, test_gpu_lin_param_grad, test_gpu_rnn_param_grad
and their *_host files): the launches' grid rules, the reduce chain, the recorded rows of a handle, the recurrent cases, and the bodies of
the checks that are one per family in name only.  Not a test module: import it by bare name, like closed_loop_cases.py; it imports
without a device (torch is imported where a device is used).  The fp64 references stay per family: fnn_param_grad_fp64.py,
lin_param_grad_fp64.py, rnn_param_grad_fp64.py.

A family is a Family(kind, extra, version): the entry point vs_<kind>_param_grad, the handle method <kind>_param_grad, the attribute
_<kind>_n_params, the names of the input pointers after abar, and the library version that brought the entry point.  A check takes the
handle, the family and the input buffers `bufs` in the entry point's order -- (abar,) or (abar, d_hid), lanes last [t, W, ld].
"""
import ctypes as C
import functools
import os
import re
from typing import NamedTuple

import numpy as np
import pytest

import closed_loop_cases as clc
from derivative_cases import KW, MAX_STEPS, N, STATE_BUFFERS, T, dev, draw_params_and_init, frozen, record_mode2
from oracle import cpu_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Family(NamedTuple):
    kind: str
    extra: tuple
    version: int
    entry = property(lambda self: f"vs_{self.kind}_param_grad")
    method = property(lambda self: f"{self.kind}_param_grad")
    n_params = property(lambda self: f"_{self.kind}_n_params")


FNN, LIN, RNN = Family("fnn", (), 315), Family("lin", (), 318), Family("rnn", ("d_hid",), 317)


@pytest.fixture(scope="module")
def vs():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import simurlacra_amd

    return simurlacra_amd


# ------------------------------------------------------------------------------------------------- the launches' grid rules
# (workgroups, rows a wave or workgroup accumulates at most) as functions of (ld, t_steps, compute units); a tile is 64 lanes x one
# step.  Each mirrors one function of simurlacra_amd/csrc/vecsim.hip.
def fnn_grid_of(ld, t_steps, n_cu):
    """fnn_param_grad_wgs: a wave per tile while there are fewer tiles than wave slots, else two workgroups of four waves per compute
    unit, each wave a contiguous run of tiles"""
    tiles = (ld // 64) * t_steps
    n_wg = min(-(-tiles // 4), 2 * n_cu)
    return n_wg, 64 * -(-tiles // (4 * n_wg))


def rnn_grid_of(ld, t_steps, n_cu):
    """rnn_param_grad_wgs: a workgroup per tile while there are fewer tiles than compute units, else one per compute unit, each a
    contiguous run of tiles"""
    tiles = (ld // 64) * t_steps
    n_wg = min(tiles, n_cu)
    return n_wg, 64 * -(-tiles // n_wg)


def lin_grid_of(ld, t_steps, n_cu):
    """lin_param_grad_wgs: workgroups of ONE wave; a wave per tile while there are fewer tiles than wave slots, else four waves per
    compute unit, each a contiguous run of tiles"""
    tiles = (ld // 64) * t_steps
    n_wg = min(tiles, 4 * n_cu)
    return n_wg, 64 * -(-tiles // n_wg)


def reduce_chain(n_wg, more_adds=0):
    """the adds of k_fnn_param_reduce across the workgroups' rows: n_wg / 4 per partial sum, 2 to join the four"""
    return -(-n_wg // 4) + 2 + more_adds


def chains_of(grid, more_adds=0):
    """the chains argument of the FNN and recurrent references from a grid rule's result"""
    n_wg, acc = grid
    return dict(acc=acc, wg=reduce_chain(n_wg, more_adds))


def chain_of(ld, t_steps, n_cu=256, more_adds=0):
    """length of the accumulation chain of one parameter of the linear pass: the FMAs of a wave's run, the reduce chain, 1 for
    accumulate"""
    n_wg, acc = lin_grid_of(ld, t_steps, n_cu)
    return acc + reduce_chain(n_wg, more_adds) + 1


def n_cu():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


def worst_ratio(err, bound):
    """max err / bound; an entry whose bound is 0 (every term of it is 0: a dead relu unit) must be met exactly"""
    return float(np.where(bound > 0.0, err / np.where(bound > 0.0, bound, 1.0), np.where(err == 0.0, 0.0, np.inf)).max())


# ------------------------------------------------------------------------------------------------- the recurrent cases
RNN_N, RNN_T = 70, 12
# case -> (family, cell, layers, units, output nonlinearity, obs_idx, seed, gain of the output layer, whh, inside a noise strategy)
CASES = {
    "omo-tanh-3": ("omo", "tanh", 1, 3, None, None, 71, 1.0, 1.5, False),          # padded to 4 units
    "pend-view-relu-8": ("pend", "relu", 1, 8, None, (2, 0), 72, 2.0, 4.0, False),  # the policy sees (th_dot, sin th)
    "pend-gru-8": ("pend", "gru", 1, 8, None, None, 73, 2.5, 1.0, False),
    "qq-su-gru-2x64": ("qq-su", "gru", 2, 64, None, None, 74, 3.0, 1.0, False),
    "qcp-su-lstm-64": ("qcp-su", "lstm", 1, 64, None, None, 75, 3.0, 1.0, False),
    "qbb-lstm-2x33-tanh-out": ("qbb", "lstm", 2, 33, "tanh", None, 76, 1.0, 1.0, False),
    "bob-gru-63-noise": ("bob", "gru", 1, 63, None, None, 77, 3.0, 1.0, True),
}
# Elman tanh cells WITHOUT recurrence: the feed-forward network [H] tanh with bias b_ih + b_hh
ELMAN_AS_FNN = {"omo-elman-3": ("omo", "tanh", 1, 3, None, None, 81, 1.0, 0.0, False),
                "qq-su-elman-64": ("qq-su", "tanh", 1, 64, None, None, 82, 3.0, 0.0, False)}


@functools.lru_cache(maxsize=None)
def case(key):
    name, cell, n_layers, H, out, obs_idx, seed, gain, whh, noisy = {**CASES, **ELMAN_AS_FNN}[key]
    ref = cpu_ref.make_ref(name, max_steps=MAX_STEPS, **KW[name])
    rng = np.random.default_rng(500 + seed)
    params, init = draw_params_and_init(ref, name, rng)          # 150 lanes, lanes 0 .. 9 at the edge
    lanes = np.concatenate([np.arange(64), np.arange(6)])        # the second lane group: six edge lanes
    params, init = params[lanes].copy(), init[lanes].copy()
    h0 = ref.reset(params.astype(np.float64), init.astype(np.float64), True)["hidden"]
    net = clc.make_rnn(ref, name, cell, n_layers, H, out, obs_idx, params.astype(np.float64), init.astype(np.float64), h0, rng, RNN_T, gain, whh)
    Hs = clc.hidden_size(net["cell"])
    cot = lambda *shape: (rng.normal(size=shape) / (RNN_N * RNN_T)).astype(np.float32)  # noqa: E731  (test_gpu_rnn_param_grad's docstring)
    return frozen(dict(name=name, ref=ref, params=params, init=init, net=net, Hs=Hs, noisy=noisy, g_rew=cot(RNN_N, RNN_T),
                       g_obs=cot(RNN_N, RNN_T + 1, ref.O), g_act=cot(RNN_N, RNN_T, ref.A), g_last=cot(RNN_N, ref.S + ref.H), g_hid=cot(RNN_N, Hs)))


# ------------------------------------------------------------------------------------------------- the records of a handle
def recorded(vs, c, install, n=N, t=T, lanes=None, cap=None, noise_seed=0):
    """a handle whose rows 0 .. t - 1 hold the closed-loop rollouts of the case c under the policy that install(e) sets (lane k repeats
    lane k % N, or the case's lanes `lanes`); cap: the capacity in rows where it is not t"""
    name = c["name"]
    pick = (lambda x: np.resize(x, (n,) + x.shape[1:])) if lanes is None else (lambda x: np.resize(x[lanes], (n,) + x.shape[1:]))
    e = vs.VecSimEnv(name, n, max_steps=MAX_STEPS, **KW[name])
    return record_mode2(e, t if cap is None else cap, pick(c["params"]), install, pick(c["init"]), (t,), noise_seed=noise_seed)


def rows_of(e, n, t, obs_idx=None):
    """(obs [t n, O], inside [t n], lengths [n]) of the handle's records, step-major; obs_idx: the view of a recurrent policy"""
    obs = e.traj_tensors(t, n)["obs"].cpu().numpy()  # [t, n, O]
    if obs_idx is not None:
        obs = obs[:, :, list(obs_idx)]
    length = e.rollout_lengths(n, t)[0].cpu().numpy()
    inside = np.arange(t)[:, None] < length[None, :]
    return obs.reshape(t * n, -1), inside.reshape(-1), length


def device_rows(vs, x, n):
    """a device array [t, W, ld], lanes last, as step-major rows [t n, W]"""
    return vs.lanes_first(x, n).cpu().numpy().transpose(1, 0, 2).reshape(x.shape[0] * n, -1)


def hidden_rows(vs, e, n, t):
    """the policy's hidden states before every step, [t n, Hs]"""
    return device_rows(vs, e.hidden_record_tensor()[:t], n)


# ------------------------------------------------------------------------------------------------- checks on a recorded handle
def check_zero_adjoints_give_zeros(e, fam, t, widths):
    import torch

    out = torch.full((getattr(e, fam.n_params),), 7.0, device="cuda")
    assert getattr(e, fam.method)(t, *[torch.zeros(t, w, e.ld, device="cuda") for w in widths], out=out) is out
    assert not out.any()


def check_nan_behind_the_rows(e, fam, n, t, bufs, records=()):
    """NaN in every input buffer at every row t >= L, at lanes n .. ld - 1 and in rows t_steps .. of a larger buffer, and (in place) in
    the record planes `records` behind L and n: the same bits as with zeros there, and finite"""
    import torch

    length = e.rollout_lengths(n, t)[0]
    assert e.ld > n and bool((length < t).any())
    behind = (torch.arange(t, device="cuda")[:, None] >= length[None, :])[:, None, :]  # [t, 1, n]
    nan = torch.full((), float("nan"), device="cuda")
    clean_in, dirty_in = [], []
    for x in bufs:
        big = torch.zeros(t + 5, x.shape[1], e.ld, device="cuda")
        big[:t, :, :n] = torch.where(behind, torch.zeros((), device="cuda"), x[:t, :, :n])
        dirty = big.clone()
        dirty[:t, :, :n] = torch.where(behind, nan, dirty[:t, :, :n])
        dirty[:, :, n:] = float("nan")
        dirty[t:] = float("nan")
        clean_in.append(big[:t])
        dirty_in.append(dirty[:t])
    clean = getattr(e, fam.method)(t, *clean_in)
    for x in records:
        x[:t, :, :n] = torch.where(behind, nan, x[:t, :, :n])
        x[:t, :, n:] = float("nan")
    assert all(bool(torch.isnan(x[:t, :, :n]).any()) for x in dirty_in + list(records))
    got = getattr(e, fam.method)(t, *dirty_in)
    assert bool(clean.any()) and bool(torch.isfinite(got).all()) and torch.equal(got, clean)


def check_two_calls_and_accumulate(vs, e, fam, t, bufs, bad, dense):
    """the same bits from call to call, with another grid in between, into out= and on top of out= under accumulate; `bad`: buffers of
    a wrong shape; dense: every entry of the gradient is non-zero (a linear stack has structurally zero slots)"""
    import torch

    grad = getattr(e, fam.method)
    g = grad(t, *bufs)
    assert torch.equal(grad(t, *bufs), g) and bool(g.all() if dense else g.any())
    grad(t - 5, *[x[:t - 5].contiguous() for x in bufs])  # another grid in between
    twice = grad(t, *bufs)
    assert torch.equal(twice, g)
    assert grad(t, *bufs, out=twice, accumulate=True) is twice and torch.equal(twice, 2.0 * g)
    r = torch.randn(g.shape, device="cuda", generator=torch.Generator("cuda").manual_seed(3))
    out = r.clone()
    assert grad(t, *bufs, out=out, accumulate=True) is out
    assert torch.equal(out, r + g)
    out.fill_(7.0)
    assert grad(t, *bufs, out=out) is out and torch.equal(out, g)
    with pytest.raises(vs.ValueErr):
        grad(t, *bufs, accumulate=True)
    with pytest.raises(vs.ShapeErr):
        grad(t, *bad)


def check_the_handle_is_untouched(vs, e, fam, t, sweep, more=lambda: []):
    """the pass run straight on the sweep's outputs (sweep() -> the input buffers first) changes no state buffer, no record plane and
    nothing of more(), and the sweep gives the same bits afterwards -> the gradient"""
    import torch

    L = vs._lib
    first = sweep()

    def records():
        planes, words = e.traj_planes()
        return [p for p, _ in planes] + [words] + more()

    before = [e.get(getattr(L, b)).copy() for b in STATE_BUFFERS]
    rows = [x.clone() for x in records()]
    g = getattr(e, fam.method)(t, *first[:1 + len(fam.extra)])
    torch.cuda.synchronize()
    assert bool(torch.isfinite(g).all()) and bool(g.any())
    for b, x in zip(STATE_BUFFERS, before):
        assert np.array_equal(e.get(getattr(L, b)), x), b
    assert all(torch.equal(a, b) for a, b in zip(records(), rows)) and e.error_count() == 0
    assert all(torch.equal(a, b) for a, b in zip(sweep(), first))
    return g


class Refusals:
    """The entry point called raw on a recorded handle e, its output one element longer than the gradient and full of sentinels:
    refused(code, handle, ...) leaves every sentinel and names the entry point in the handle's error; served() fills the gradient."""

    def __init__(self, vs, e, fam, t, bufs):
        import torch

        self.vs, self.e, self.fam, self.t, self.bufs = vs, e, fam, t, tuple(bufs)
        self.lib = vs._lib.load()
        self.n_params = getattr(e, fam.n_params)
        self.out = torch.full((self.n_params + 1,), 7.0, device="cuda")

    def call(self, handle, t_steps=None, null=None, n=None, bufs=None):
        """null: the index of a pointer to pass as NULL (the inputs in order, then d_params)"""
        import torch

        ptrs = [None if k == null else C.c_void_p(x.data_ptr()) for k, x in enumerate(tuple(bufs or self.bufs) + (self.out,))]
        rc = getattr(self.lib, self.fam.entry)(handle._h if handle is not None else None, self.t if t_steps is None else t_steps, *ptrs,
                                               self.n_params if n is None else n, 0)
        torch.cuda.synchronize()
        return rc

    def refused(self, code, handle, **kw):
        assert self.call(handle, **kw) == code
        assert bool((self.out == 7.0).all())  # the sentinels
        if handle is not None:
            assert self.fam.entry in self.lib.vs_last_error(handle._h).decode()

    def served(self):
        n = self.n_params
        assert self.call(self.e) == self.vs._lib.VS_OK and not bool((self.out[:n] == 7.0).any()) and float(self.out[n]) == 7.0
        self.out.fill_(7.0)

    def arguments(self):
        """NULL handle and pointers, t_steps 0 / -3 / T + 1, n_params +- 1, a trajectory offset, auto-reset"""
        L, e = self.vs._lib, self.e
        self.refused(L.VS_ERR_ARG, None)
        for null in range(len(self.bufs) + 1):
            self.refused(L.VS_ERR_ARG, e, null=null)
        for t_steps in (0, -3, self.t + 1):
            self.refused(L.VS_ERR_ARG, e, t_steps=t_steps)
        for n in (self.n_params - 1, self.n_params + 1):
            self.refused(L.VS_ERR_ARG, e, n=n)
        e.set_traj_offset(3)
        self.refused(L.VS_ERR_STATE, e)
        e.set_traj_offset(0)
        e.set_auto_reset(True)
        self.refused(L.VS_ERR_STATE, e)
        e.set_auto_reset(False)
        self.served()

    def policies(self, d, theta, clear, own, others):
        """a population of the flat parameters theta on the handle, no policy (clear()), each policy of another kind (others: a name of
        other_kinds -> extra arguments of refused), record mode 1; in between the family's own policy (own()) is served, and at the end
        the policy installed BEFORE the record mode changed is served again, not set anew: it, its workspace and a recurrent policy's
        hidden record survive the change of mode and capacity.  d: the family's env_dims"""
        L, e = self.vs._lib, self.e
        e.set_policy_population(np.tile(theta.reshape(1, -1), ((e.n_envs - 1) // 64 + 1, 1)), lane_set=np.arange(e.n_envs) // 64)
        self.refused(L.VS_ERR_STATE, e)
        e.set_policy_population(None)
        self.served()
        clear()
        self.refused(L.VS_ERR_STATE, e)
        for kind, kw in others.items():
            other_kinds(e, d, self.t)[kind]()
            self.refused(L.VS_ERR_STATE, e, **kw)
        own()
        self.served()
        e.set_record_mode(1)
        e.set_traj_capacity(self.t)
        self.refused(L.VS_ERR_STATE, e)
        e.set_record_mode(2)
        e.set_traj_capacity(self.t)
        self.served()                                             # after the refusals the same handle serves a good call
        assert e.error_count() == 0

    def discrete_family(self):
        """the discrete-action family has no action gradient"""
        import torch

        vs, t = self.vs, self.t
        disc = vs.VecSimEnv("bob-d", 64, dt=0.01, max_steps=MAX_STEPS)
        disc.set_record_mode(2)
        disc.set_traj_capacity(t)
        self.refused(vs._lib.VS_ERR_STATE, disc, bufs=[torch.zeros(t, x.shape[1], disc.ld, device="cuda") for x in self.bufs])
        disc.close()


def other_kinds(e, d, t):
    """name -> a call that puts a small policy of that kind on the handle e (d: its env_dims)"""
    zeros = lambda n: np.zeros(n, dtype=np.float32)  # noqa: E731
    return dict(linear=lambda: e.set_policy_linear(zeros(d["A"]), ["const"]),
                fnn=lambda: e.set_policy_fnn(zeros((d["O"] + 1) * 8 + (8 + 1) * d["A"]), [8]),
                fnn3=lambda: e.set_policy_fnn(zeros((d["O"] + 1) * 8 + 2 * (8 + 1) * 8 + (8 + 1) * d["A"]), [8, 8, 8]),  # three hidden layers
                gru=lambda: e.set_policy_rnn(zeros(3 * 8 * (d["O"] + 8 + 2) + (8 + 1) * d["A"]), cell="gru", n_layers=1, hidden_size=8),
                playback=lambda: e.set_policy_playback(np.zeros((e.n_envs, t, d["A"]), dtype=np.float32)))


# ------------------------------------------------------------------------------------------------- autograd
def autograd_loss(vs, roll, init):
    """(-discounted return + 1e-3 sum a^2 of the rollout class from init, (obs, rew, act))"""
    obs, rew, act, lengths = roll(init, clc.TT)
    return -vs.discounted_return(rew, lengths, clc.GAMMA).sum() + 1e-3 * act.pow(2).sum(), (obs, rew, act)


def autograd_grads(vs, roll, tc, weights):
    """(gradients of the loss by weights + [init], the loss, (obs, rew, act)); the graph is kept"""
    import torch

    init = dev(tc["init"]).requires_grad_(True)
    loss, outs = autograd_loss(vs, roll, init)
    return torch.autograd.grad(loss, weights + [init], retain_graph=True), loss, outs


def flat_grads(gs):
    import torch

    return torch.cat([x.reshape(-1) for x in gs]).detach().cpu().numpy().astype(np.float64)


class Seen(NamedTuple):
    """what one call of the handle method saw: step-major rows, the handle's ld, lanes and the accumulate flag"""
    obs: np.ndarray
    hid: object
    bufs: list
    inside: np.ndarray
    ld: int
    accumulate: bool
    n: int


def spy_on(vs, monkeypatch, fam, seen):
    """VecSimEnv's method of the family behind a recorder: every call appends a Seen to `seen`, then runs"""
    plain = getattr(vs.VecSimEnv, fam.method)

    def spy(self, t_steps, *bufs, out=None, accumulate=False):
        n = self.n_envs
        obs, inside, _ = rows_of(self, n, t_steps)
        seen.append(Seen(obs, hidden_rows(vs, self, n, t_steps) if fam.extra else None, [device_rows(vs, x, n) for x in bufs], inside,
                         self.ld, bool(accumulate), n))
        return plain(self, t_steps, *bufs, out=out, accumulate=accumulate)

    monkeypatch.setattr(vs.VecSimEnv, fam.method, spy)


def check_three_batches_accumulate(seen):
    assert [s.accumulate for s in seen] == [False, True, True] and [s.n for s in seen] == [32, 32, 6]


def check_backward_twice_and_the_sweep(loss, weights, g_kernel, g_torch):
    """g_kernel, g_torch: the gradients by weights + [init] through the two passes"""
    import torch

    again = torch.autograd.grad(loss, weights, retain_graph=True)
    assert all(torch.equal(a, b) for a, b in zip(again, g_kernel[:-1]))                # backward() twice: the same bits
    assert torch.equal(g_kernel[-1], g_torch[-1]) and bool(g_kernel[-1].any())         # d init_states: the same sweep
    assert all(a.shape == w.shape for a, w in zip(g_kernel, weights))


def check_kernel_against_torch_pass(name, seen, bound_of, g_kernel, g_torch, factor, label):
    """the two passes' flat gradients differ by at most factor x the bounds of the three batches' calls, summed (bound_of(Seen))"""
    bound = sum(np.reshape(bound_of(s), -1) for s in seen[:3])
    worst = worst_ratio(np.abs(g_kernel - g_torch), factor * bound)
    print(f"{name}: kernel against torch parameter pass, worst difference / ({label}) {worst:.3f}")
    assert np.abs(g_torch).max() > 0.0 and worst <= 1.0, (name, worst)


def check_fp64_takes_the_torch_pass(vs, roll, tc, weights):
    """a rollout class built on a .double() policy: the torch pass, whatever was asked for, and float64 gradients"""
    import torch

    assert roll.param_pass == "torch"
    g = torch.autograd.grad(autograd_loss(vs, roll, dev(tc["init"]))[0], weights)
    assert all(x.dtype == torch.float64 and bool(torch.isfinite(x).all()) for x in g) and any(bool(x.any()) for x in g)


# ------------------------------------------------------------------------------------------------- the C-ABI, without a device
def check_header_declares_the_signature(fam):
    """-> the header's text"""
    header = open(os.path.join(ROOT, "include", "vecsim.h")).read()
    more = "".join(rf"const float\* {x},\s*" for x in fam.extra)
    assert re.search(rf"int\s+{fam.entry}\(vs_handle h, int t_steps, const float\* abar, {more}float\* d_params, int64_t n_params, "
                     r"int accumulate\);", header)
    return header


def check_symbol_is_exported_and_bound(fam):
    import simurlacra_amd as vs
    from simurlacra_amd import _lib as L

    lib = C.CDLL(L.LIB_PATH)
    assert hasattr(lib, fam.entry)
    assert fam.entry in L.exported_symbols()
    fn = getattr(L.load(), fam.entry)
    assert fn.restype is C.c_int
    assert list(fn.argtypes) == [C.c_void_p, C.c_int] + [C.c_void_p] * (2 + len(fam.extra)) + [C.c_int64, C.c_int]
    assert L.load().vs_version() >= fam.version
    assert callable(getattr(vs.VecSimEnv, fam.method))


def check_null_handle_and_null_pointers_are_refused(fam):
    from simurlacra_amd import _lib as L

    buf = (C.c_float * 4)()
    fn = getattr(L.load(), fam.entry)
    k = 2 + len(fam.extra)  # pointers: abar, the extra inputs, d_params
    assert fn(None, 1, *[buf] * k, 4, 0) == L.VS_ERR_ARG
    for null in range(k):
        assert fn(None, 1, *[None if j == null else buf for j in range(k)], 4, int(null == k - 1)) == L.VS_ERR_ARG
    assert all(x == 0.0 for x in buf)
