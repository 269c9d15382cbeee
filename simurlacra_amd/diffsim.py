"""
Differentiable playback rollouts: a batch of open-loop rollouts whose observations and rewards are attached to torch autograd.

The forward pass is the recording playback launch the library already has (vs_set_policy_playback, record mode 2, one launch of T
steps); the backward pass is ONE reverse-mode sweep over those records (vs_rollout_vjp, k_rollout_vjp) that turns the incoming
gradients of the observations and rewards into gradients of the actions and of the initial states.  What it serves: shooting
trajectory optimisation on the return, initial-state estimation next to the parameter identification of sysid.py, and any loss
written in torch over the observations and rewards of a rollout.

Conventions are those of the kernel: the raw action is the variable (ActNormWrapper's map, the clip and the dead zone are inside
the step, kinks follow the branch taken), domain parameters and the initial hidden state are constants.  DifferentiableRollout
also takes the domain parameters as a torch tensor: the backward pass is then the sweep that carries their gradient next to the
others (vs_rollout_vjp_params, k_rollout_vjp_dp) -- system identification with any loss written in torch over the observations.
The reward, the bounds of the spaces and the initial state are constants with respect to the parameters.

DifferentiablePolicyRollout is the closed-loop form: a LinearPolicy on a feature stack runs inside the recording launch
(vs_set_policy_linear), and the backward pass is one closed-loop sweep (vs_rollout_vjp_policy, k_rollout_vjp_lin) -- the action's
dependence on the observation is part of the adjoint -- followed by one batched torch pass over the recorded observations for the
gradient of the policy's parameters.  DifferentiableNetRollout is the same for a feed-forward network of one or two hidden layers
(vs_set_policy_fnn, vs_rollout_vjp_fnn, k_rollout_vjp_fnn): backpropagation through time with the network inside the sweep.
DifferentiableRecurrentRollout is the form for RNNPolicy / GRUPolicy / LSTMPolicy (vs_set_policy_rnn, vs_rollout_vjp_rnn,
k_rollout_vjp_rnn): the sweep carries a second adjoint for the policy's hidden state, and the parameter pass is one batched
single-step pass over the recorded observations and hidden states.
DifferentiablePopulationRollout runs a POPULATION of linear policies or networks on handles with a policy population
(vs_set_policy_population): one gradient row per member from one sweep (vs_rollout_vjp_pop) and one device parameter pass
(vs_pop_param_grad) per batch.
"""
from typing import Optional, Sequence

import torch

from . import _lib as L
from .exceptions import ShapeErr, TypeErr, ValueErr
from .sysid import check_playback_env, domain_param_matrix, vec_env_like
from .vec_env import lanes_first, lanes_last


def discounted_return(rew, lengths, gamma: float):
    """[N]: sum over t < lengths[n] of gamma^t rew[n, t]; rew [N, T], lengths [N] (torch tensors on one device).  The gradient of
    its sum with respect to rew[n, t] is the float32 value gamma^t inside a rollout and 0 behind its end."""
    if rew.dim() != 2 or tuple(lengths.shape) != (rew.shape[0],):
        raise ShapeErr(msg=f"rew [N, T] and lengths [N], got {tuple(rew.shape)} and {tuple(lengths.shape)}")
    if not 0.0 <= float(gamma) <= 1.0:
        raise ValueErr(given=gamma, ge_constraint="0", le_constraint="1")
    steps = torch.arange(rew.shape[1], device=rew.device)
    disc = torch.pow(torch.tensor(float(gamma), dtype=rew.dtype, device=rew.device), steps.to(rew.dtype))
    inside = (steps[None, :] < lengths[:, None]).to(rew.dtype)
    return (rew * (disc[None, :] * inside)).sum(dim=1)


class _RecordedBatches:
    """What the two rollout classes share: the env checks, one handle per batch of at most batch_lanes lanes, and a token per handle
    that says which rollouts its records hold, so that a backward pass re-records only after another forward call overwrote them."""

    def __init__(self, env, who: str, batch_lanes: int):
        self._base, self._act_norm = check_playback_env(env, who)
        if batch_lanes < 1:
            raise ValueErr(given=batch_lanes, ge_constraint="1")
        self.env = env
        self._batch_lanes = int(batch_lanes)
        self._vecs = {}  # batch index -> [handle, token of the rollouts its records hold]
        self._calls = 0

    def close(self):
        for v, _ in self._vecs.values():
            v.close()
        self._vecs = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _dims(self):
        b = self._base
        return b.act_space.flat_dim, b.state_space.flat_dim, b.obs_space.flat_dim

    def _batches(self, N):
        return [(n0, min(n0 + self._batch_lanes, N)) for n0 in range(0, N, self._batch_lanes)]

    def _recorded(self, b, token, n, launch):
        """the handle of batch b with the records `token` names: launch(handle) records them (on the caller's stream) unless the
        handle still holds them"""
        slot = self._vecs.get(b)
        if slot is not None and slot[0].n_envs != n:
            slot[0].close()
            slot = None
        if slot is None:
            v = vec_env_like(self._base, n, self._act_norm)
            v.set_record_mode(2)
            slot = self._vecs[b] = [v, None]
        v = slot[0]
        if slot[1] == token:
            return v
        with v.on_current_stream():
            launch(v)
        slot[1] = token
        return v


class DifferentiableRollout(_RecordedBatches):
    """rollout = DifferentiableRollout(env);  obs, rew, lengths = rollout(actions, init_states, domain_params=None)

    env: one of the pysim envs, optionally inside an ActNormWrapper (the actions are then in [-1, 1] units); any other wrapper and
    the discrete-action family raise ValueErr.  actions [N, T, A] and init_states [N, S] (the FULL state every rollout starts
    from) are float32 tensors on the env's device.  Returns obs [N, T + 1, O] (row k: the observation after k steps), rew [N, T]
    and lengths [N] (int64: the steps a rollout took before its episode ended); rows behind a rollout's end are 0.  obs and rew
    carry gradients to actions and init_states; domain_params -- a list of N dicts or an [N, n_names] array with names=, as for
    TrajectoryMatchSampler.param_matrix; None: the env's own -- gets none.  domain_params may also be a float32 torch tensor
    [N, len(names)] with names= (distinct names): when it requires grad, obs and rew carry gradients to it as well -- through
    _calc_constants and the dynamics; the reward's own dependence on a parameter, the bounds of the spaces and the initial state are
    constants, as for TrajectoryMatchSampler.evaluate_grad.  Up to VS_SENS_MAX_PARAMS names are one backward sweep
    (rollout_vjp_params), more run as further sweeps of that many over the same records.  A tensor that does not require grad
    takes the plain sweep.  More than batch_lanes rollouts run in batches."""

    def __init__(self, env, batch_lanes: int = 65536):
        super().__init__(env, "DifferentiableRollout", batch_lanes)

    def _record(self, b, token, actions, init_states, params):
        """the recording playback launch of one batch on its handle; a handle that still holds these records is left alone"""
        T = actions.shape[1]

        def launch(v):
            v.set_params(params)
            v.set_policy_playback(actions)                          # one recording per lane: lane i replays recording i
            v.reset(init_state=init_states.detach().cpu().numpy())
            v.set_traj_offset(0)
            v.step_policy(T, record=True)

        return self._recorded(b, token, actions.shape[0], launch)

    def __call__(self, actions, init_states, domain_params=None, names: Optional[Sequence[str]] = None):
        A, S, _ = self._dims()
        if not hasattr(actions, "dim") or not hasattr(init_states, "dim"):
            raise TypeErr(msg="actions and init_states must be torch tensors")
        if actions.dim() != 3 or actions.shape[2] != A or actions.shape[0] < 1 or actions.shape[1] < 1:
            raise ShapeErr(msg=f"actions must be [N, T, {A}], got shape {tuple(actions.shape)}")
        if tuple(init_states.shape) != (actions.shape[0], S):
            raise ShapeErr(msg=f"init_states must be [{actions.shape[0]}, {S}], got shape {tuple(init_states.shape)}")
        N = actions.shape[0]
        ptensor = domain_params if isinstance(domain_params, torch.Tensor) else None
        if ptensor is not None:
            if names is None:
                raise ShapeErr(msg="domain_params as a tensor needs names=, one per column")
            if ptensor.dim() != 2 or tuple(ptensor.shape) != (N, len(names)):
                raise ShapeErr(msg=f"domain_params must be [{N}, {len(names)}] (one column per name), got shape {tuple(ptensor.shape)}")
            if ptensor.dtype != torch.float32:
                raise TypeErr(msg=f"domain_params must be a float32 tensor, got {ptensor.dtype}")
            if len(set(names)) != len(names):
                raise ValueErr(msg=f"domain_params: a name is repeated in {list(names)}")
        params = domain_param_matrix(self._base, [dict()] * N if domain_params is None else domain_params, names)
        if params.shape[0] != N:
            raise ShapeErr(msg=f"domain_params needs one row per rollout ({N}), got {params.shape[0]}")
        for name, x in (("actions", actions), ("init_states", init_states)):
            if not x.is_cuda or x.dtype != torch.float32:
                raise TypeErr(msg=f"{name} must be a float32 tensor on the GPU")
        self._calls += 1
        wrt = tuple(names) if ptensor is not None else None
        obs, rew, lengths = _RolloutFn.apply(self, self._calls, params, wrt, ptensor, actions, init_states)
        return obs, rew, lengths

    def _forward(self, call, params, actions, init_states):
        A, S, O = self._dims()
        N, T = actions.shape[0], actions.shape[1]
        obs = torch.empty(N, T + 1, O, dtype=torch.float32, device=actions.device)
        rew = torch.empty(N, T, dtype=torch.float32, device=actions.device)
        lengths = torch.empty(N, dtype=torch.int64, device=actions.device)
        for b, (n0, n1) in enumerate(self._batches(N)):
            n = n1 - n0
            v = self._record(b, (call, b), actions[n0:n1].contiguous(), init_states[n0:n1], params[n0:n1])
            with v.on_current_stream():
                tt = v.traj_tensors(T, n)
                lengths[n0:n1] = v.rollout_lengths(n, T)[0]
                obs[n0:n1, :T] = tt["obs"].transpose(0, 1)
                obs[n0:n1, T] = v.tensor(L.VS_OBS)[:, :n].t()       # (a lane that ended early is frozen at its last state)
                rew[n0:n1] = tt["rew"].t()
        steps = torch.arange(T + 1, device=actions.device)
        obs = obs * (steps[None, :] <= lengths[:, None]).to(obs.dtype)[:, :, None]
        rew = rew * (steps[None, :T] < lengths[:, None]).to(rew.dtype)
        return obs, rew, lengths

    def _backward(self, call, params, actions, init_states, grad_obs, grad_rew, wrt=None):
        """(d actions, d init_states, d domain parameters [N, len(wrt)] or None); wrt: the names whose gradient is asked for"""
        A, S, O = self._dims()
        N, T = actions.shape[0], actions.shape[1]
        d_act = torch.empty(N, T, A, dtype=torch.float32, device=actions.device)
        d_init = torch.empty(N, S, dtype=torch.float32, device=actions.device)
        d_par = torch.empty(N, len(wrt), dtype=torch.float32, device=actions.device) if wrt else None
        P = L.VS_SENS_MAX_PARAMS
        for b, (n0, n1) in enumerate(self._batches(N)):
            n = n1 - n0
            v = self._record(b, (call, b), actions[n0:n1].contiguous(), init_states[n0:n1], params[n0:n1])
            with v.on_current_stream():
                g_rew = None if grad_rew is None else lanes_last(grad_rew[n0:n1].to(torch.float32), v.ld)
                g_obs = None if grad_obs is None else lanes_last(grad_obs[n0:n1].to(torch.float32), v.ld)
                if wrt:  # passes of P names over the same records; d_act and d_init are the same in each: the first one's are taken
                    da, di, dp = v.rollout_vjp_params(T, wrt[:P], g_rew=g_rew, g_obs=g_obs)
                    d_par[n0:n1, :P] = lanes_first(dp, n)
                    for j0 in range(P, len(wrt), P):
                        d_par[n0:n1, j0:j0 + P] = lanes_first(v.rollout_vjp_params(T, wrt[j0:j0 + P], g_rew=g_rew, g_obs=g_obs)[2], n)
                else:
                    da, di = v.rollout_vjp(T, g_rew=g_rew, g_obs=g_obs)
                d_act[n0:n1] = lanes_first(da, n)
                d_init[n0:n1] = lanes_first(di[:S], n)             # (the initial hidden state is a constant)
        return d_act, d_init, d_par


class _RolloutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, roll, call, params, wrt, ptensor, actions, init_states):
        # params [N, P] is the matrix the handles get (ptensor's values are in it already); ptensor only ties the graph to wrt
        obs, rew, lengths = roll._forward(call, params, actions.detach(), init_states.detach())
        ctx.roll, ctx.call, ctx.params, ctx.wrt = roll, call, params, wrt
        ctx.pdev = None if ptensor is None else ptensor.device
        ctx.save_for_backward(actions, init_states)
        ctx.mark_non_differentiable(lengths)
        return obs, rew, lengths

    @staticmethod
    def backward(ctx, grad_obs, grad_rew, _grad_lengths):
        actions, init_states = ctx.saved_tensors
        wrt = ctx.wrt if ctx.needs_input_grad[4] else None
        d_act, d_init, d_par = ctx.roll._backward(ctx.call, ctx.params, actions.detach(), init_states.detach(), grad_obs, grad_rew, wrt)
        return None, None, None, None, None if d_par is None else d_par.to(ctx.pdev), d_act, d_init


class _ClosedLoopRollout(_RecordedBatches):
    """What the closed-loop classes share: the call, the recording launch, the outputs and the backward pass.  A subclass sets
    self.policy (what the caller gave), self._mean (the module whose parameters get gradients: the policy without its exploration
    noise) and says how the policy reaches a handle (_set_policy), which sweep runs (_sweep) and what the noise's std is now.
    A policy with more than the action adjoint to pull back (a hidden state) also says what it keeps of a batch's sweep (_keep)
    and how the parameter gradients come from it (_param_grads): that is the torch pass.  Every subclass takes param_pass
    ("kernel" or "torch") through _check_param_pass and _set_param_pass and says which handle method the device pass is
    (_device_pass).  Under "kernel" it runs per batch on a running flat gradient -- the first batch writes it,
    later batches add to it -- and _needs_rows is False: the [N, T, .] copies of abar and of the observations are not made."""

    _needs_rows = True  # _param_grads reads abar [N, T, A] and the recorded observations [N, T, O]

    @staticmethod
    def _check_param_pass(param_pass):
        if param_pass not in ("kernel", "torch"):
            raise ValueErr(msg=f"param_pass is 'kernel' or 'torch', got {param_pass!r}")

    def _set_param_pass(self, param_pass):
        """self.param_pass: what was asked, or "torch" when a parameter of self._mean is not float32"""
        fp32 = all(p.dtype == torch.float32 for p in self._mean.parameters())
        self.param_pass = param_pass if fp32 else "torch"
        self._needs_rows = self.param_pass == "torch"

    def _check_dims(self, obs_dim, act_dim):
        A, _, O = self._dims()
        if obs_dim != O or act_dim != A:
            raise ShapeErr(msg=f"the policy maps {obs_dim} observation rows to {act_dim} actions, the env has {O} and {A}")

    def _noise_std(self):
        raise NotImplementedError

    def _set_policy(self, v, params, noise_std):
        raise NotImplementedError

    def _sweep(self, v, T, g_rew, g_obs, g_act):
        """(d_act, d_init, anything else the sweep returns) of one batch"""
        raise NotImplementedError

    def _keep(self, v, T, n, more):
        """what _param_grads needs of a batch beyond abar and the observations; `more`: the sweep's further returns"""
        return None

    def _device_pass(self, v, T, da, more, out, accumulate):
        """the handle's parameter-gradient pass of one batch; da: the sweep's action adjoints [T, A, ld] as returned (lanes last),
        `more`: its further returns; returns the flat gradient (`out`, or a new tensor when out is None)"""
        raise NotImplementedError

    def _param_grads(self, seen, abar, kept):
        """gradients of self._mean's parameters: one batched pass over the [N T] recorded observations"""
        N, T, O = seen.shape
        with torch.enable_grad():
            mean = self._mean(seen.detach().reshape(N * T, O))
            return torch.autograd.grad(mean, list(self._mean.parameters()),
                                       grad_outputs=abar.reshape(N * T, -1).to(device=mean.device, dtype=mean.dtype))

    def _check_noise_std(self, noise_std):
        """noise_std= of a call as a float32 tensor [A] (a scalar is broadcast: its gradient is the sum over the entries)"""
        A = self._dims()[0]
        if not hasattr(noise_std, "dim"):
            raise TypeErr(msg="noise_std must be a torch tensor (or None: the exploration strategy's own std, a constant)")
        if noise_std.dtype != torch.float32:
            raise TypeErr(msg=f"noise_std must be a float32 tensor, got {noise_std.dtype}")
        if noise_std.dim() > 1 or (noise_std.dim() == 1 and noise_std.shape[0] != A):
            raise ShapeErr(msg=f"noise_std must be [{A}] or a scalar, got shape {tuple(noise_std.shape)}")
        std = noise_std.expand(A)
        if not bool((std.detach() >= 0).all()):
            raise ValueErr(msg=f"noise_std must be >= 0, got {std.detach().cpu().tolist()}")
        return std

    def __call__(self, init_states, T, domain_params=None, names: Optional[Sequence[str]] = None, noise_seed: int = 0,
                 noise_std=None):
        """noise_std: None -- the std of the NormalActNoiseExplStrat around the policy (none: no noise), a constant of the graph;
        or a float32 tensor [A] (a scalar is broadcast): the recording launch adds noise_std * eps_t with these values, eps_t keyed
        by noise_seed, and obs, rew and act carry gradients to it -- a_t = mean_t + noise_std * eps_t, reparameterised: one
        noise_std_grad per batch straight on the sweep's action adjoints (vs_noise_std_grad), under either param_pass; rollout n
        then draws the noise of env index n whatever batch_lanes is.  Entries below 0 raise ValueErr, another shape ShapeErr."""
        _, S, _ = self._dims()
        if not hasattr(init_states, "dim"):
            raise TypeErr(msg="init_states must be a torch tensor")
        if init_states.dim() != 2 or init_states.shape[1] != S or init_states.shape[0] < 1:
            raise ShapeErr(msg=f"init_states must be [N, {S}], got shape {tuple(init_states.shape)}")
        if int(T) < 1:
            raise ValueErr(given=T, ge_constraint="1")
        N = init_states.shape[0]
        params = domain_param_matrix(self._base, [dict()] * N if domain_params is None else domain_params, names)
        if params.shape[0] != N:
            raise ShapeErr(msg=f"domain_params needs one row per rollout ({N}), got {params.shape[0]}")
        if not init_states.is_cuda or init_states.dtype != torch.float32:
            raise TypeErr(msg="init_states must be a float32 tensor on the GPU")
        std = None if noise_std is None else self._check_noise_std(noise_std)
        if std is None:
            noise_std = self._noise_std()                            # (the std may have been updated since the constructor)
        else:
            noise_std = std.detach().cpu().numpy()                   # (the values the recording launch adds the noise with)
        self._calls += 1
        # with noise_std= the noise of rollout n is keyed by n itself, whatever the batches are (the index offset of a batch's handle)
        setup = (self, self._calls, params, int(T), noise_std, int(noise_seed), std is not None)
        obs, rew, act, lengths = _PolicyRolloutFn.apply(setup, std, init_states, *self._mean.parameters())
        return obs, rew, act, lengths

    def _record(self, b, setup, n0, n1, init_states, weights):
        """the recording closed-loop launch of one batch (rollouts n0 .. n1 - 1) on its handle; a handle that still holds these
        records is left alone"""
        _, call, params, T, noise_std, noise_seed, by_index = setup

        def launch(v):
            v.set_index_offset(n0 if by_index else 0)
            v.set_params(params[n0:n1])
            self._set_policy(v, weights, noise_std)
            v.reset(init_state=init_states[n0:n1].detach().cpu().numpy())
            v.set_traj_offset(0)
            v.step_policy(T, record=True, noise_seed=noise_seed)

        return self._recorded(b, (call, b), n1 - n0, launch)

    def _forward(self, setup, init_states, weights):
        A, S, O = self._dims()
        N, T, dev = init_states.shape[0], setup[3], init_states.device
        obs = torch.empty(N, T + 1, O, dtype=torch.float32, device=dev)
        rew = torch.empty(N, T, dtype=torch.float32, device=dev)
        act = torch.empty(N, T, A, dtype=torch.float32, device=dev)
        lengths = torch.empty(N, dtype=torch.int64, device=dev)
        for b, (n0, n1) in enumerate(self._batches(N)):
            n = n1 - n0
            v = self._record(b, setup, n0, n1, init_states, weights)
            with v.on_current_stream():
                tt = v.traj_tensors(T, n)
                lengths[n0:n1] = v.rollout_lengths(n, T)[0]
                obs[n0:n1, :T] = tt["obs"].transpose(0, 1)
                obs[n0:n1, T] = v.tensor(L.VS_OBS)[:, :n].t()       # (a lane that ended early is frozen at its last state)
                rew[n0:n1] = tt["rew"].t()
                act[n0:n1] = tt["act"].transpose(0, 1)
        steps = torch.arange(T + 1, device=dev)
        inside = (steps[None, :T] < lengths[:, None]).to(torch.float32)
        obs = obs * (steps[None, :] <= lengths[:, None]).to(obs.dtype)[:, :, None]
        return obs, rew * inside, act * inside[:, :, None], lengths

    def _backward(self, setup, init_states, weights, grad_obs, grad_rew, grad_act, want_std=False):
        """(gradients of the policy's parameters, d init_states, d noise_std [A] or None); want_std: the call's noise_std= asks for
        its gradient -- one noise_std_grad per batch on the sweep's action adjoints, the first batch writes, later batches add"""
        A, S, O = self._dims()
        N, T, dev = init_states.shape[0], setup[3], init_states.device
        kernel = self.param_pass == "kernel"
        rows = self._needs_rows
        abar = torch.empty(N, T, A, dtype=torch.float32, device=dev) if rows else None
        seen = torch.empty(N, T, O, dtype=torch.float32, device=dev) if rows else None
        d_init = torch.empty(N, S, dtype=torch.float32, device=dev)
        flat, kept, d_std = None, [], None
        for b, (n0, n1) in enumerate(self._batches(N)):
            n = n1 - n0
            v = self._record(b, setup, n0, n1, init_states, weights)
            with v.on_current_stream():
                g = [None if x is None else lanes_last(x[n0:n1].to(torch.float32), v.ld) for x in (grad_rew, grad_obs, grad_act)]
                da, di, *more = self._sweep(v, T, g[0], g[1], g[2])
                d_init[n0:n1] = lanes_first(di[:S], n)             # (the initial hidden state is a constant)
                if rows:
                    abar[n0:n1] = lanes_first(da, n)               # (0 behind a rollout's end: the kernel writes it so)
                    seen[n0:n1] = v.traj_tensors(T, n)["obs"].transpose(0, 1)
                if kernel:
                    flat = self._device_pass(v, T, da, more, out=flat, accumulate=flat is not None)
                else:
                    kept.append(self._keep(v, T, n, more))
                if want_std:
                    d_std = v.noise_std_grad(T, setup[5], da, out=d_std, accumulate=d_std is not None)
        if not kernel:
            return self._param_grads(seen, abar, kept), d_init, d_std
        grads, at = [], 0
        for p in self._mean.parameters():  # parameters_to_vector's order
            grads.append(flat[at:at + p.numel()].view_as(p).to(p.device))  # (as the torch pass: on the parameter's device)
            at += p.numel()
        return tuple(grads), d_init, d_std


class DifferentiablePolicyRollout(_ClosedLoopRollout):
    """roll = DifferentiablePolicyRollout(env, policy);  obs, rew, act, lengths = roll(init_states, T, domain_params=None)

    Closed-loop rollouts of a LinearPolicy on a FeatureStack that linear_kernel_spec accepts (optionally inside a
    NormalActNoiseExplStrat; any other policy raises TypeErr, a stack the kernel cannot take ValueErr), attached to torch autograd.
    env: as for DifferentiableRollout.  init_states [N, S] is a float32 tensor on the env's device, T the number of steps.  Returns
    obs [N, T + 1, O], rew [N, T], act [N, T, A] (the raw policy actions, exploration noise included) and lengths [N] (int64);
    rows behind a rollout's end are 0.  obs, rew and act carry gradients to init_states and to policy.parameters() -- through the
    dynamics AND through the policy's dependence on the observations.  The exploration noise (keyed by noise_seed) is a constant
    of the graph, and so is the strategy's std -- unless the call hands the std over as a tensor (noise_std=, see __call__ of
    _ClosedLoopRollout): then it gets its gradient from vs_noise_std_grad; domain_params get none.
    Forward: set_policy_linear from the module's current weights, reset(init_state), one recording step_policy(T).  Backward: one
    rollout_vjp_policy per batch for the action adjoints and d init_states, and the weight gradient by param_pass:
      "torch"   (the default) ONE batched pass of the policy over the recorded [N T] observations;
      "kernel"  one lin_param_grad per batch (vs_lin_param_grad), straight on the sweep's action adjoints and the handle's records:
                the first batch writes the flat gradient, later batches add to it; no [N, T, .] copy of the adjoints or of the
                observations and no [N T, num_feat] feature matrix is made.  Deterministic: backward() twice returns the same bits.
    A policy whose weight is not float32 takes the torch pass whatever is asked (self.param_pass says which one runs); any other
    value raises ValueErr."""

    def __init__(self, env, policy, batch_lanes: int = 65536, param_pass: str = "torch"):
        from .policies import LinearPolicy, NormalActNoiseExplStrat, linear_kernel_spec

        self._check_param_pass(param_pass)
        inner = policy.policy if isinstance(policy, NormalActNoiseExplStrat) else policy
        if not isinstance(inner, LinearPolicy):
            raise TypeErr(msg="DifferentiablePolicyRollout takes a LinearPolicy, optionally inside a NormalActNoiseExplStrat, got "
                              f"{type(inner).__name__}")
        spec = linear_kernel_spec(policy)
        if spec is None:
            raise ValueErr(msg=f"the rollout kernel cannot evaluate {inner.features}: every elementwise feature and const_feat at "
                               "most once, MultFeat of 2 .. 4 rows, ATan2Feat, at most 39 of those two and 128 features in all")
        super().__init__(env, "DifferentiablePolicyRollout", batch_lanes)
        self._check_dims(inner.env_spec.obs_space.flat_dim, inner.env_spec.act_space.flat_dim)
        self.policy, self._mean, self._terms = policy, inner, spec["terms"]
        self._set_param_pass(param_pass)

    def _device_pass(self, v, T, da, more, out, accumulate):
        return v.lin_param_grad(T, da, out=out, accumulate=accumulate)

    def _param_grads(self, seen, abar, kept):  # (the rows in the weight's dtype: a no-op for a float32 policy)
        return super()._param_grads(seen.to(next(self._mean.parameters()).dtype), abar, kept)

    def _noise_std(self):
        from .policies import linear_kernel_spec

        return linear_kernel_spec(self.policy)["noise_std"]

    def _set_policy(self, v, weights, noise_std):
        v.set_policy_linear(weights[0].detach().to(torch.float32).reshape(-1), self._terms, noise_std=noise_std)

    def _sweep(self, v, T, g_rew, g_obs, g_act):
        return v.rollout_vjp_policy(T, g_rew=g_rew, g_obs=g_obs, g_act=g_act)


class DifferentiableNetRollout(_ClosedLoopRollout):
    """roll = DifferentiableNetRollout(env, policy);  obs, rew, act, lengths = roll(init_states, T, domain_params=None)

    DifferentiablePolicyRollout for a feed-forward network: an FNN or FNNPolicy (its featurisation included) that fnn_kernel_spec
    accepts, with one or two hidden layers, optionally inside a NormalActNoiseExplStrat.  Another policy raises TypeErr; three or
    four hidden layers, dropout or a nonlinearity the kernel lacks ValueErr; a network that does not map the env's observation to
    its action ShapeErr.  Call, return values and what carries gradients are DifferentiablePolicyRollout's: obs, rew and act reach
    init_states and every parameter of the network -- backpropagation through time over the closed loop.
    Forward: set_policy_fnn from the module's current weights, reset(init_state), one recording step_policy(T).  Backward: one
    rollout_vjp_fnn per batch for the action adjoints and d init_states, and the parameter gradients by param_pass:
      "kernel"  one fnn_param_grad per batch (vs_fnn_param_grad), straight on the sweep's action adjoints and the handle's records:
                the first batch writes the flat gradient, later batches add to it; no [N, T, .] copy of the adjoints or of the
                observations is made.  Deterministic: backward() twice returns the same bits;
      "torch"   ONE batched torch pass of the network over the recorded [N T] observations.
    A network with a parameter that is not float32 takes the torch pass whatever is asked (self.param_pass says which one runs);
    any other value raises ValueErr.  The torch pass hands the network the recorded observations in its parameters' dtype: nothing
    changes for a float32 network, and a float64 FNN or FNNPolicy, whose backward pass used to fail on the float32 rows
    (a dtype mismatch in the first Linear), now gets float64 gradients."""

    def __init__(self, env, policy, batch_lanes: int = 65536, param_pass: str = "kernel"):
        from .policies import FNN, FNNPolicy, NormalActNoiseExplStrat, fnn_kernel_spec

        self._check_param_pass(param_pass)
        inner = policy.policy if isinstance(policy, NormalActNoiseExplStrat) else policy
        if not isinstance(inner, (FNN, FNNPolicy)):
            raise TypeErr(msg="DifferentiableNetRollout takes an FNN or FNNPolicy, optionally inside a NormalActNoiseExplStrat, got "
                              f"{type(inner).__name__}")
        spec = fnn_kernel_spec(policy)
        if spec is None:
            raise ValueErr(msg="the rollout kernel cannot evaluate this network: hidden layers of at most 64 units, tanh / relu / "
                               "sigmoid / no nonlinearities, no dropout")
        if len(spec["hidden_sizes"]) > 2:
            raise ValueErr(msg=f"the closed-loop sweep takes one or two hidden layers, got {len(spec['hidden_sizes'])}")
        super().__init__(env, "DifferentiableNetRollout", batch_lanes)
        net = inner.net if isinstance(inner, FNNPolicy) else inner
        self._check_dims(net.hidden_layers[0].in_features - (1 if spec["feat"] else 0), net.output_layer.out_features)
        self.policy, self._mean = policy, inner
        self._arch = {k: spec[k] for k in ("hidden_sizes", "hidden_nonlin", "output_nonlin", "feat")}
        self._set_param_pass(param_pass)

    def _device_pass(self, v, T, da, more, out, accumulate):
        return v.fnn_param_grad(T, da, out=out, accumulate=accumulate)

    def _param_grads(self, seen, abar, kept):  # (the rows in the parameters' dtype: a no-op for a float32 network)
        return super()._param_grads(seen.to(next(self._mean.parameters()).dtype), abar, kept)

    def _noise_std(self):
        from .policies import fnn_kernel_spec

        return fnn_kernel_spec(self.policy)["noise_std"]

    def _set_policy(self, v, weights, noise_std):
        flat = torch.cat([w.detach().to(torch.float32).reshape(-1) for w in weights])   # parameters_to_vector's order
        v.set_policy_fnn(flat, noise_std=noise_std, **self._arch)

    def _sweep(self, v, T, g_rew, g_obs, g_act):
        return v.rollout_vjp_fnn(T, g_rew=g_rew, g_obs=g_obs, g_act=g_act)


class DifferentiableRecurrentRollout(_ClosedLoopRollout):
    """roll = DifferentiableRecurrentRollout(env, policy);  obs, rew, act, lengths = roll(init_states, T, domain_params=None)

    DifferentiableNetRollout for a recurrent policy: an RNNPolicy (tanh / relu), GRUPolicy or LSTMPolicy that rnn_kernel_spec accepts
    (one or two layers of at most 64 units), optionally inside a NormalActNoiseExplStrat.  Another policy raises TypeErr; dropout or
    a shape the kernel lacks ValueErr; a policy that does not map the env's observation to its action ShapeErr.  Call, return
    values and what carries gradients are DifferentiableNetRollout's: backpropagation through time over the closed loop, the
    policy's hidden state included.  Every rollout starts from init_hidden(), a constant.
    Forward: set_policy_rnn from the module's current weights (that zeroes the hidden state), set_policy_hidden_record(Hs),
    reset(init_state), one recording step_policy(T).  Backward: one rollout_vjp_rnn per batch for the adjoints of the actions and of
    the hidden states and d init_states, and the parameter gradients by param_pass:
      "torch"   (the default) ONE batched single-step pass of the policy over the recorded [N T] observations and hidden states --
                not sequential in time, 2^20 rows at a time;
      "kernel"  one rnn_param_grad per batch (vs_rnn_param_grad), straight on the sweep's d_act and d_hid and the handle's records:
                the first batch writes the flat gradient, later batches add to it; no [N, T, .] copy of d_hid, of the hidden-state
                record or of the observations is made.  Deterministic: backward() twice returns the same bits.
    A policy with a parameter that is not float32 takes the torch pass whatever is asked (self.param_pass says which one runs); any
    other value raises ValueErr."""

    _PASS_ROWS = 1 << 20  # rows of the batched parameter pass at a time (the device RNN library's tensors are indexed with 32 bits)

    def __init__(self, env, policy, batch_lanes: int = 65536, param_pass: str = "torch"):
        from .policies import NormalActNoiseExplStrat, _RNNPolicyBase, rnn_kernel_spec

        self._check_param_pass(param_pass)
        inner = policy.policy if isinstance(policy, NormalActNoiseExplStrat) else policy
        if not isinstance(inner, _RNNPolicyBase):
            raise TypeErr(msg="DifferentiableRecurrentRollout takes an RNNPolicy, GRUPolicy or LSTMPolicy, optionally inside a "
                              f"NormalActNoiseExplStrat, got {type(inner).__name__}")
        spec = rnn_kernel_spec(policy)
        if spec is None:
            raise ValueErr(msg="the rollout kernel cannot evaluate this recurrent policy: one or two layers of at most 64 units, "
                               "tanh / relu / sigmoid / no output nonlinearity, no dropout")
        super().__init__(env, "DifferentiableRecurrentRollout", batch_lanes)
        self._check_dims(inner.rnn_layers.input_size, inner.output_layer.out_features)
        self.policy, self._mean = policy, inner
        self._arch = {k: spec[k] for k in ("cell", "n_layers", "hidden_size", "output_nonlin")}
        self._hs = inner.hidden_size
        self._set_param_pass(param_pass)

    def _device_pass(self, v, T, da, more, out, accumulate):
        return v.rnn_param_grad(T, da, more[0], out=out, accumulate=accumulate)

    def _noise_std(self):
        from .policies import rnn_kernel_spec

        return rnn_kernel_spec(self.policy)["noise_std"]

    def _set_policy(self, v, weights, noise_std):
        flat = torch.cat([w.detach().to(torch.float32).reshape(-1) for w in weights])   # parameters_to_vector's order
        v.set_policy_rnn(flat, noise_std=noise_std, **self._arch)                       # (hidden state: zeros = init_hidden())
        v.set_policy_hidden_record(self._hs)

    def _sweep(self, v, T, g_rew, g_obs, g_act):
        return v.rollout_vjp_rnn(T, g_rew=g_rew, g_obs=g_obs, g_act=g_act)

    def _keep(self, v, T, n, more):
        """(cotangents of p_{t+1} [n, T, Hs], recorded p_t [n, T, Hs])"""
        return lanes_first(more[0], n), lanes_first(v.hidden_record_tensor()[:T], n)

    def _param_grads(self, seen, abar, kept):
        N, T, O = seen.shape
        seen = seen.detach()
        params, total = list(self._mean.parameters()), None
        lanes = max(1, self._PASS_ROWS // T)  # whole rollouts per pass (the rows are independent: any split gives the same sum)
        n0 = 0
        for d_hid, hid in kept:  # batch by batch, sliced from what the batch kept: no second copy of all [N T] rows
            for l0 in range(0, d_hid.shape[0], lanes):
                at, rows = slice(l0, min(l0 + lanes, d_hid.shape[0])), slice(n0 + l0, n0 + min(l0 + lanes, d_hid.shape[0]))
                with torch.enable_grad():
                    act, p_new = self._mean(seen[rows].reshape(-1, O), hid[at].detach().reshape(-1, self._hs))
                    g = torch.autograd.grad((act, p_new), params, grad_outputs=(
                        abar[rows].reshape(-1, abar.shape[2]).to(device=act.device, dtype=act.dtype),
                        d_hid[at].reshape(-1, self._hs).to(device=p_new.device, dtype=p_new.dtype)))
                total = g if total is None else tuple(a + b for a, b in zip(total, g))
            n0 += d_hid.shape[0]
        return total


def population_lanes(n_members: int, n_rollouts: int):
    """The lanes of a population of n_members members with n_rollouts rollouts each: every member takes whole groups of 64 lanes.
    Returns (src, real, lane_set) as int64 / bool / int32 numpy arrays over the n_members * 64 * ceil(n_rollouts / 64) lanes:
    src[l] the flat rollout index (member * n_rollouts + rollout) lane l runs -- the padding lanes of a member's last group repeat
    its last rollout --, real[l] whether the lane IS that rollout (padding lanes get zero cotangents), lane_set[l] its member."""
    import numpy as np

    per = -(-int(n_rollouts) // 64) * 64
    j = np.tile(np.arange(per, dtype=np.int64), int(n_members))
    member = np.repeat(np.arange(int(n_members), dtype=np.int64), per)
    return member * int(n_rollouts) + np.minimum(j, int(n_rollouts) - 1), j < int(n_rollouts), member.astype(np.int32)


class DifferentiablePopulationRollout(_RecordedBatches):
    """roll = DifferentiablePopulationRollout(env, policy);  obs, rew, act, lengths = roll.roll(params, init_states, T)

    The closed-loop rollouts of a POPULATION of policies of one architecture, attached to torch autograd: one gradient per member
    from the same launches (SVPG-style particles, ensembles, multi-start backpropagation through time).  policy gives the
    architecture only -- a LinearPolicy on a stack that linear_kernel_spec accepts, or an FNN / FNNPolicy of one or two hidden layers
    that fnn_kernel_spec accepts, optionally inside a NormalActNoiseExplStrat whose noise is a constant of the sweep; another policy
    raises TypeErr, one the kernel cannot take ValueErr.  The weights come with the call: params [P, n_params] float32, row s in the
    order of the policy's setter (net.weight flattened, or parameters_to_vector), and init_states [P, M, S].  Returns obs
    [P, M, T + 1, O], rew [P, M, T], act [P, M, T, A] and lengths [P, M]; obs, rew and act carry gradients to params and init_states.
    Every member takes whole groups of 64 lanes of a handle with a policy population (set_policy_population); the padding lanes of
    its last group repeat its last initial state and get zero cotangents, so they add exact zeros.  More than batch_lanes lanes run
    in batches that split on group boundaries; a member may span batches.  Backward: per batch one rollout_vjp_population and one
    population_param_grad straight on its action adjoints -- the first batch writes the [P, n_params] gradient (zeros for members it
    does not hold), later batches add to it; no [N, T, .] copy of observations or adjoints is made.  Deterministic: backward() twice
    returns the same bits.  Recurrent policies are not taken (vs_rollout_vjp_pop refuses them), and the std of the noise gets no
    gradient here."""

    def __init__(self, env, policy, batch_lanes: int = 65536):
        from .policies import FNN, FNNPolicy, LinearPolicy, NormalActNoiseExplStrat, fnn_kernel_spec, linear_kernel_spec

        inner = policy.policy if isinstance(policy, NormalActNoiseExplStrat) else policy
        if isinstance(inner, LinearPolicy):
            spec = linear_kernel_spec(policy)
            if spec is None:
                raise ValueErr(msg=f"the rollout kernel cannot evaluate {inner.features}")
            terms = spec["terms"]
            self._install = lambda v, flat, std: v.set_policy_linear(flat, terms, noise_std=std)
            self._spec_of = linear_kernel_spec
            dims = inner.env_spec.obs_space.flat_dim, inner.env_spec.act_space.flat_dim
        elif isinstance(inner, (FNN, FNNPolicy)):
            spec = fnn_kernel_spec(policy)
            if spec is None:
                raise ValueErr(msg="the rollout kernel cannot evaluate this network: hidden layers of at most 64 units, tanh / relu / "
                                   "sigmoid / no nonlinearities, no dropout")
            if len(spec["hidden_sizes"]) > 2:
                raise ValueErr(msg=f"the closed-loop sweep takes one or two hidden layers, got {len(spec['hidden_sizes'])}")
            arch = {k: spec[k] for k in ("hidden_sizes", "hidden_nonlin", "output_nonlin", "feat")}
            self._install = lambda v, flat, std: v.set_policy_fnn(flat, noise_std=std, **arch)
            self._spec_of = fnn_kernel_spec
            net = inner.net if isinstance(inner, FNNPolicy) else inner
            dims = net.hidden_layers[0].in_features - (1 if spec["feat"] else 0), net.output_layer.out_features
        else:
            raise TypeErr(msg="DifferentiablePopulationRollout takes a LinearPolicy, an FNN or an FNNPolicy, optionally inside a "
                              f"NormalActNoiseExplStrat, got {type(inner).__name__}")
        if batch_lanes < 64:
            raise ValueErr(given=batch_lanes, ge_constraint="64")
        super().__init__(env, "DifferentiablePopulationRollout", batch_lanes // 64 * 64)  # (batches split on group boundaries)
        A, _, O = self._dims()
        if dims != (O, A):
            raise ShapeErr(msg=f"the policy maps {dims[0]} observation rows to {dims[1]} actions, the env has {O} and {A}")
        self.policy = policy
        self.n_params = sum(p.numel() for p in inner.parameters())

    def roll(self, params, init_states, T, noise_seed: int = 0):
        _, S, _ = self._dims()
        if not hasattr(params, "dim") or not hasattr(init_states, "dim"):
            raise TypeErr(msg="params and init_states must be torch tensors")
        if params.dim() != 2 or params.shape[0] < 1 or params.shape[1] != self.n_params:
            raise ShapeErr(msg=f"params must be [P, {self.n_params}], got shape {tuple(params.shape)}")
        if init_states.dim() != 3 or init_states.shape[0] != params.shape[0] or init_states.shape[1] < 1 or init_states.shape[2] != S:
            raise ShapeErr(msg=f"init_states must be [{params.shape[0]}, M, {S}], got shape {tuple(init_states.shape)}")
        if int(T) < 1:
            raise ValueErr(given=T, ge_constraint="1")
        for name, x in (("params", params), ("init_states", init_states)):
            if not x.is_cuda or x.dtype != torch.float32:
                raise TypeErr(msg=f"{name} must be a float32 tensor on the GPU")
        self._calls += 1
        setup = (self, self._calls, int(T), self._spec_of(self.policy)["noise_std"], int(noise_seed))
        return tuple(_PopulationRolloutFn.apply(setup, params, init_states))

    __call__ = roll

    def _record(self, b, setup, l0, l1, lanes, params, init_flat):
        _, call, T, noise_std, noise_seed = setup
        src, _, lane_set = lanes

        def launch(v):
            v.set_index_offset(0)
            v.set_params(domain_param_matrix(self._base, [dict()] * (l1 - l0)))
            flat = params.detach().contiguous()
            self._install(v, flat[0], noise_std)
            v.set_policy_population(flat, lane_set=lane_set[l0:l1])
            v.reset(init_state=init_flat[torch.as_tensor(src[l0:l1], device=init_flat.device)].cpu().numpy())
            v.set_traj_offset(0)
            v.step_policy(T, record=True, noise_seed=noise_seed)

        return self._recorded(b, (call, b), l1 - l0, launch)

    def _forward(self, setup, params, init_states):
        A, S, O = self._dims()
        (P, M), T, dev = init_states.shape[:2], setup[2], init_states.device
        lanes = population_lanes(P, M)
        init_flat = init_states.reshape(P * M, S)
        obs = torch.empty(P * M, T + 1, O, dtype=torch.float32, device=dev)
        rew = torch.empty(P * M, T, dtype=torch.float32, device=dev)
        act = torch.empty(P * M, T, A, dtype=torch.float32, device=dev)
        lengths = torch.empty(P * M, dtype=torch.int64, device=dev)
        for b, (l0, l1) in enumerate(self._batches(len(lanes[0]))):
            n = l1 - l0
            v = self._record(b, setup, l0, l1, lanes, params, init_flat)
            at = torch.as_tensor(lanes[1][l0:l1].nonzero()[0], device=dev)   # the batch's lanes that are rollouts ...
            to = torch.as_tensor(lanes[0][l0:l1][lanes[1][l0:l1]], device=dev)  # ... and which ones
            with v.on_current_stream():
                tt = v.traj_tensors(T, n)
                lengths[to] = v.rollout_lengths(n, T)[0][at]
                obs[to, :T] = tt["obs"].transpose(0, 1)[at]
                obs[to, T] = v.tensor(L.VS_OBS)[:, :n].t()[at]
                rew[to] = tt["rew"].t()[at]
                act[to] = tt["act"].transpose(0, 1)[at]
        steps = torch.arange(T + 1, device=dev)
        inside = (steps[None, :T] < lengths[:, None]).to(torch.float32)
        obs = obs * (steps[None, :] <= lengths[:, None]).to(obs.dtype)[:, :, None]
        return (obs.view(P, M, T + 1, O), (rew * inside).view(P, M, T), (act * inside[:, :, None]).view(P, M, T, A), lengths.view(P, M))

    def _backward(self, setup, params, init_states, grad_obs, grad_rew, grad_act):
        """(d params [P, n_params], d init_states [P, M, S])"""
        A, S, O = self._dims()
        (P, M), T, dev = init_states.shape[:2], setup[2], init_states.device
        lanes = population_lanes(P, M)
        init_flat = init_states.reshape(P * M, S)
        d_init = torch.empty(P * M, S, dtype=torch.float32, device=dev)
        grads = [None if g is None else g.reshape((P * M,) + tuple(g.shape[2:])).to(torch.float32) for g in (grad_rew, grad_obs, grad_act)]
        d_params = None
        for b, (l0, l1) in enumerate(self._batches(len(lanes[0]))):
            n = l1 - l0
            v = self._record(b, setup, l0, l1, lanes, params, init_flat)
            src = torch.as_tensor(lanes[0][l0:l1], device=dev)
            real = torch.as_tensor(lanes[1][l0:l1], device=dev)
            with v.on_current_stream():
                # the batch's cotangents, lanes last; a padding lane gets zeros: its sweep and its rows of the parameter pass are 0
                g = [None if x is None else lanes_last(x[src] * real.view((n,) + (1,) * (x.dim() - 1)).to(x.dtype), v.ld) for x in grads]
                da, di = v.rollout_vjp_population(T, g_rew=g[0], g_obs=g[1], g_act=g[2])
                d_init[src[real]] = lanes_first(di[:S], n)[real]
                d_params = v.population_param_grad(T, da, out=d_params, accumulate=d_params is not None)
        return d_params, d_init.view(P, M, S)


class _PopulationRolloutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, setup, params, init_states):
        obs, rew, act, lengths = setup[0]._forward(setup, params.detach(), init_states.detach())
        ctx.setup = setup
        ctx.save_for_backward(params, init_states)
        ctx.mark_non_differentiable(lengths)
        return obs, rew, act, lengths

    @staticmethod
    def backward(ctx, grad_obs, grad_rew, grad_act, _grad_lengths):
        params, init_states = ctx.saved_tensors
        d_params, d_init = ctx.setup[0]._backward(ctx.setup, params.detach(), init_states.detach(), grad_obs, grad_rew, grad_act)
        return None, d_params.clone(), d_init


class _PolicyRolloutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, setup, noise_std, init_states, *params):
        # noise_std [A] or None: its values are in setup already (the recording launch's); the tensor only ties the graph to it
        roll = setup[0]
        obs, rew, act, lengths = roll._forward(setup, init_states.detach(), [p.detach() for p in params])
        ctx.setup = setup
        ctx.std_device = None if noise_std is None else noise_std.device
        ctx.save_for_backward(init_states, *params)
        ctx.mark_non_differentiable(lengths)
        return obs, rew, act, lengths

    @staticmethod
    def backward(ctx, grad_obs, grad_rew, grad_act, _grad_lengths):
        init_states, *params = ctx.saved_tensors
        want_std = ctx.std_device is not None and ctx.needs_input_grad[1]
        d_params, d_init, d_std = ctx.setup[0]._backward(ctx.setup, init_states.detach(), [p.detach() for p in params], grad_obs,
                                                         grad_rew, grad_act, want_std)
        return (None, d_std.to(ctx.std_device) if want_std else None, d_init) + tuple(d_params)
