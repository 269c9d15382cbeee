"""
ParameterExploringSampler (P/sampling/parameter_exploration_sampler.py): the sampler of the episodic algorithms (HC, PEPG, NES,
PoWER, CEM, REPS).  It evaluates a population of policy parameter vectors, every vector on the same rollouts: the same
`num_domains` domain parameter sets and the same `num_init_states_per_domain` initial states per domain (common random
numbers).

The reference hands every (parameter set, domain, init state) triple to a worker process.  Here the whole population is ONE
batch of lanes of a libvecsim handle when the fused kernel evaluates the policy (FNN / FNNPolicy, RNN / GRU / LSTM policies,
LinearPolicy on a feature stack; see fnn_kernel_spec / rnn_kernel_spec / linear_kernel_spec): vs_set_policy_population gives every aligned group of 64 lanes its own parameter
vector, and one vs_step_policy launch chain runs all sets at once.

Lane layout (population_lane_layout): set s owns lanes s * stride .. (s + 1) * stride - 1, stride = R (rollouts per set)
rounded up to a multiple of 64, and its rollouts are the first R of them.  The library takes one set per aligned group of 64
lanes, so the padding lanes behind a set's R run that set too (a plain rollout from the init space, in SIMD lanes the group
occupies anyway) and are dropped before any StepSequence is built.  A stride that is a multiple of 256 keeps the 256-env
shapes of the network kernel available.  A call of more than `batch_lanes` lanes is cut
into batches of whole sets.  Any other policy, or fuse_policy=False, loops over the sets on the host (policy.param_values =
the set's vector, then the ParallelRolloutSampler path): slow, but exact, and the reference path of the tests.
"""
from typing import List, NamedTuple, Optional, Sequence

import numpy as np
import torch

from .exceptions import TypeErr, ValueErr
from .policies import NormalActNoiseExplStrat
from .sampling import ParallelRolloutSampler, StepSequence, fused_policy_specs
from .wrappers import (DomainRandWrapper, DomainRandWrapperBuffer, DomainRandWrapperLive, fuse_wrappers, inner_env,
                       remove_all_dr_wrappers, typed_env)

_PAD = (None, None)  # the work entry of a padding lane


class ParameterSample(NamedTuple):
    """One parameter vector and the rollouts it produced"""

    params: torch.Tensor
    rollouts: List[StepSequence]

    @property
    def mean_undiscounted_return(self) -> float:
        return float(np.mean([ro.undiscounted_return() for ro in self.rollouts]))

    @property
    def num_rollouts(self) -> int:
        return len(self.rollouts)


class ParameterSamplingResult(Sequence[ParameterSample]):
    """The ParameterSamples of one sample() call, in the order of the parameter sets"""

    def __init__(self, samples: Sequence[ParameterSample]):
        self._samples = list(samples)

    def __getitem__(self, idx):
        if isinstance(idx, slice):
            return ParameterSamplingResult(self._samples[idx])
        return self._samples[idx]

    def __len__(self) -> int:
        return len(self._samples)

    @property
    def parameters(self) -> torch.Tensor:
        return torch.stack([s.params for s in self._samples])

    @property
    def mean_returns(self) -> np.ndarray:
        return np.array([s.mean_undiscounted_return for s in self._samples])

    @property
    def rollouts(self) -> list:
        return [s.rollouts for s in self._samples]

    @property
    def num_rollouts(self) -> int:
        return sum(s.num_rollouts for s in self._samples)


class PopulationReturns:
    """What sample_returns() hands the episodic algorithms, all on the device: `parameters` [P, n_params], `returns` [P, R]
    (float32: the discounted return of rollout r of set s), `lengths` [P, R] (int64), `mean_returns` [P] and `packed`, the
    PackedRollouts of every batch (padding lanes included, see population_lane_layout)"""

    def __init__(self, parameters, returns, lengths, packed):
        self.parameters, self.returns, self.lengths, self.packed = parameters, returns, lengths, packed

    @property
    def mean_returns(self) -> torch.Tensor:
        return self.returns.mean(dim=1)

    def __len__(self) -> int:
        return int(self.returns.shape[0])


# ------------------------------------------------------------------------------------------------ pure functions
def draw_domain_params(dr_wrapper, num_domains: int) -> list:
    """`num_domains` domain parameter sets for one sample() call: a live randomizer's draws, random entries of a buffer
    (np.random.randint), or -- without a DR wrapper -- None each (the env's nominal parameters)"""
    if isinstance(dr_wrapper, DomainRandWrapperLive):
        dr_wrapper.randomizer.randomize(num_domains)
        return list(dr_wrapper.randomizer.get_params(fmt="list", dtype="numpy"))
    if isinstance(dr_wrapper, DomainRandWrapperBuffer) and dr_wrapper.buffer:
        buf = dr_wrapper.buffer
        if isinstance(buf, dict):
            return [buf] * num_domains
        return [buf[int(i)] for i in np.random.randint(0, len(buf), num_domains)]
    return [None] * num_domains


def draw_init_states(init_space, num_init_states: int, init_states=None) -> list:
    """`num_init_states` initial states: the caller's (exactly that many) or init_space.sample_uniform() draws (global NumPy RNG)"""
    if init_states is not None:
        init_states = list(init_states)
        if len(init_states) != num_init_states:
            raise ValueErr(msg=f"expected {num_init_states} init states (num_init_states_per_domain), got {len(init_states)}")
        return init_states
    return [init_space.sample_uniform() for _ in range(num_init_states)]


def param_work_list(domain_params: list, init_states: list) -> list:
    """[(init_state, domain_param)] of ONE parameter set: domain outer, init state inner (every set runs this list)"""
    return [(s, d) for d in domain_params for s in init_states]


def population_lane_layout(num_sets: int, rollouts_per_set: int, batch_lanes: int):
    """(stride, batches): set s of a batch owns lanes k * stride .. k * stride + rollouts_per_set - 1 of it (k = s - first set
    of the batch), stride = rollouts_per_set rounded up to a multiple of 64; batches = [(first set, number of sets)], whole
    sets of at most batch_lanes lanes each (at least one set)"""
    stride = -(-rollouts_per_set // 64) * 64
    per = max(1, batch_lanes // stride)
    return stride, [(s0, min(per, num_sets - s0)) for s0 in range(0, num_sets, per)]


def population_lane_set(n_sets: int, stride: int) -> np.ndarray:
    """the lane table of one batch (vs_set_policy_population): set k in all stride lanes of its block, padding included"""
    return np.repeat(np.arange(n_sets, dtype=np.int32), stride)


def population_real_lanes(n_sets: int, rollouts_per_set: int, stride: int) -> np.ndarray:
    """the lanes of one batch that are rollouts, in rollout order (set, then rollout)"""
    return (np.arange(n_sets)[:, None] * stride + np.arange(rollouts_per_set)[None, :]).reshape(-1)


def lane_of(set_idx: int, rollout: int, stride: int) -> int:
    return set_idx * stride + rollout


def rollout_of_lane(lane: int, stride: int, rollouts_per_set: int):
    """(set, rollout) of a lane, or None for a padding lane"""
    s, r = divmod(int(lane), stride)
    return (s, r) if r < rollouts_per_set else None


def _check_count(name, value):
    if not isinstance(value, int) or isinstance(value, bool):
        raise TypeErr(given=value, expected_type=int)
    if value < 1:
        raise ValueErr(given_name=name, given=value, ge_constraint="1")


class ParameterExploringSampler:
    """Drop-in for P/sampling/parameter_exploration_sampler.py.  `num_workers` is accepted and ignored (lanes replace worker
    processes); batch_lanes, chunk, full_records, fuse_policy and owned_arrays are ParallelRolloutSampler's."""

    def __init__(self, env, policy, num_init_states_per_domain: int, num_domains: int, num_workers: int = 1, seed=None, *,
                 batch_lanes: int = 65536, chunk: int = 128, full_records: bool = True, fuse_policy: bool = True,
                 owned_arrays: bool = False):
        _check_count("num_init_states_per_domain", num_init_states_per_domain)
        _check_count("num_domains", num_domains)
        self.num_init_states_per_domain = num_init_states_per_domain
        self.num_domains = num_domains
        self.num_workers = num_workers  # ignored
        self.policy = policy
        # the domain parameters are drawn here, per sample() call, and handed to the lanes: the outermost DR wrapper is
        # remembered and every DR wrapper leaves the chain
        self._dr_wrapper = typed_env(env, DomainRandWrapper)
        self.env = remove_all_dr_wrappers(env)
        self._batch_lanes = int(batch_lanes)
        self._fuse_policy = bool(fuse_policy)
        self._sampler = ParallelRolloutSampler(self.env, policy, min_rollouts=self.num_rollouts_per_param, seed=seed,
                                               batch_lanes=batch_lanes, chunk=chunk, full_records=full_records,
                                               fuse_policy=fuse_policy, owned_arrays=owned_arrays)

    @property
    def num_rollouts_per_param(self) -> int:
        return self.num_init_states_per_domain * self.num_domains

    def close(self):
        self._sampler.close()

    def reinit(self, env=None, policy=None):
        if env is not None:
            self._dr_wrapper = typed_env(env, DomainRandWrapper)
            self.env = remove_all_dr_wrappers(env)
        if policy is not None:
            self.policy = policy
        self._sampler.reinit(self.env if env is not None else None, policy)

    def _fused(self) -> bool:
        """the condition of ParallelRolloutSampler's fused policy path"""
        if not self._fuse_policy:
            return False
        return any(spec is not None for spec in fused_policy_specs(self.policy, fuse_wrappers(self.env), inner_env(self.env).name))

    def _begin_call(self, param_sets, init_states):
        """what sample() and sample_returns() share: (params [P, n_params] float32, the work list of ONE set, stride, batches --
        population_lane_layout's) after the call's draws of domain parameters and init states; counts the call (one Philox key
        per call, as ParallelRolloutSampler.sample)"""
        params = torch.as_tensor(param_sets).detach()
        if params.dim() == 1:
            params = params.unsqueeze(0)
        if params.dim() != 2 or params.shape[0] < 1:
            raise ValueErr(msg=f"param_sets must be [num_sets, num_params], got shape {tuple(params.shape)}")
        params = params.to(torch.float32)
        dps = draw_domain_params(self._dr_wrapper, self.num_domains)
        inits = draw_init_states(inner_env(self.env).init_space, self.num_init_states_per_domain, init_states)
        work = param_work_list(dps, inits)
        self._sampler._sample_count += 1
        return (params, work) + population_lane_layout(params.shape[0], len(work), self._batch_lanes)

    def _population_batches(self, params, work, stride, batches, packed_out):
        """one population batch per group of whole sets; rollout r of set s is lane lane_of(s, r, stride) of the call.  Yields
        (number of sets, real lanes, what _run_batch returned) of every batch"""
        R = len(work)
        for s0, nb in batches:
            work_b = [_PAD] * (nb * stride)
            for k in range(nb):
                work_b[k * stride:k * stride + R] = work
            real = population_real_lanes(nb, R, stride)
            yield nb, real, self._sampler._run_batch(work_b, lane_of(s0, 0, stride), True, packed_out=packed_out,
                                                     population=dict(params=params[s0:s0 + nb],
                                                                     lane_set=population_lane_set(nb, stride), real=real))

    def sample(self, param_sets, init_states: Optional[List[np.ndarray]] = None) -> ParameterSamplingResult:
        """Every parameter vector (rows of param_sets, [P, n_params]) on the same num_rollouts_per_param rollouts (eval=True)"""
        params, work, stride, batches = self._begin_call(param_sets, init_states)
        if self._fused():
            R = len(work)
            rollouts = [ros[k * R:(k + 1) * R] for nb, _, ros in self._population_batches(params, work, stride, batches, False)
                        for k in range(nb)]
        else:
            rollouts = self._sample_loop(params, work, stride)
        return ParameterSamplingResult([ParameterSample(params=params[s].clone(), rollouts=rollouts[s])
                                        for s in range(params.shape[0])])

    def sample_returns(self, param_sets, init_states: Optional[List[np.ndarray]] = None, gamma: float = 1.0) -> PopulationReturns:
        """sample() for the algorithms that consume the returns per parameter set only (HC, PEPG, NES, CEM, REPS): the same draws,
        work list, lanes, batches and Philox keys, but every batch stays on the device as a PackedRollouts and its discounted
        returns come from vs_returns_scan -- no StepSequence is built and nothing is copied to the host.  Needs a policy the fused
        kernel evaluates (ValueErr otherwise)."""
        params, work, stride, batches = self._begin_call(param_sets, init_states)
        R = len(work)
        rets, lens, packed = [], [], []
        for nb, real, p in self._population_batches(params, work, stride, batches, True):
            real_t = torch.as_tensor(real, dtype=torch.int64, device=p.lengths.device)  # the padding lanes drop out by index
            rets.append(p.discounted_returns(gamma).index_select(0, real_t).view(nb, R))
            lens.append(p.lengths.index_select(0, real_t).view(nb, R))
            packed.append(p)
        return PopulationReturns(params.to(rets[0].device), torch.cat(rets), torch.cat(lens), packed)

    def _sample_loop(self, params, work, stride):
        """the sets one after the other through ParallelRolloutSampler's path: policy.param_values = the set's vector (the
        policy's own values are restored afterwards)"""
        target = self.policy.policy if isinstance(self.policy, NormalActNoiseExplStrat) else self.policy
        if not hasattr(target, "param_values"):
            raise TypeErr(msg="the policy has no param_values to explore")
        keep = target.param_values.detach().clone()
        bl = self._sampler._batch_lanes
        out = []
        try:
            for s in range(params.shape[0]):
                target.param_values = params[s].to(keep.device, keep.dtype)
                ros = []
                for a in range(0, len(work), bl):
                    ros += self._sampler._run_batch(work[a:a + bl], lane_of(s, a, stride), True)
                out.append(ros)
        finally:
            target.param_values = keep
        return out
