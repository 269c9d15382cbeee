"""
Trajectory matching for system identification and simulation-based inference (the inner loop of SysIdViaEpisodicRL, SimOpt,
BayesSim, NPDR on these simulators): P domain-parameter candidates x R recorded real-robot segments.  For every pair the
candidate's parameters are set, the env is reset to the segment's recorded state, the segment's recorded actions are replayed
(vs_set_policy_playback) and the simulated observations are compared with the recorded ones INSIDE the rollout kernel
(vs_set_rollout_target): one float per pair comes back, nothing per step leaves the device.

Lane layout: the pair (candidate p, segment r) is lane p * R + r of a batch, its recording is r.  Candidates beyond
batch_lanes // R go into further batches; a candidate is never split.
"""
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib as L
from .exceptions import ShapeErr, ValueErr
from .vec_env import expand_upper_triangle  # noqa: F401  (re-exported)
from .wrappers import ActNormWrapper, EnvWrapper, all_envs, inner_env


# ------------------------------------------------------------------------------------------------------ lane arithmetic
def lane_of(p: int, r: int, num_segments: int) -> int:
    """lane of (candidate p of the batch, segment r)"""
    return p * num_segments + r


def pair_of(lane: int, num_segments: int) -> Tuple[int, int]:
    """(candidate of the batch, segment) of a lane"""
    return divmod(lane, num_segments)


def candidate_batches(num_candidates: int, num_segments: int, batch_lanes: int) -> List[Tuple[int, int]]:
    """[(first candidate, one past the last)] of every batch: batch_lanes // R whole candidates each (at least one)"""
    if num_candidates < 0 or num_segments < 1 or batch_lanes < 1:
        raise ValueErr(msg="candidate_batches: num_candidates >= 0, num_segments >= 1, batch_lanes >= 1")
    per = max(1, batch_lanes // num_segments)
    return [(p0, min(p0 + per, num_candidates)) for p0 in range(0, num_candidates, per)]


def batch_lane_rec(num_candidates: int, num_segments: int) -> np.ndarray:
    """lane_rec of a batch of num_candidates candidates: lane p * R + r replays segment r"""
    return np.tile(np.arange(num_segments, dtype=np.int32), num_candidates)


def pad_recordings(recs: Sequence, width: int, extra_rows: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """(table [R, max T_r + extra_rows, width] float32, zero behind a recording's end; lengths [R] int32 = rows - extra_rows)"""
    arrs = []
    for r in recs:
        a = np.asarray(r.detach().cpu().numpy() if hasattr(r, "detach") else r, dtype=np.float32)
        if a.ndim != 2 or a.shape[1] != width or a.shape[0] < extra_rows:
            raise ShapeErr(msg=f"a recording must be [T + {extra_rows}, {width}], got shape {a.shape}")
        arrs.append(a)
    lens = np.array([a.shape[0] - extra_rows for a in arrs], dtype=np.int32)
    tab = np.zeros((len(arrs), max(1, int(lens.max())) + extra_rows, width), dtype=np.float32)
    for k, a in enumerate(arrs):
        tab[k, : a.shape[0]] = a
    return tab, lens


def check_playback_env(env, who: str):
    """(innermost env, whether an ActNormWrapper is around it) of a plain env or one inside an ActNormWrapper; anything else raises"""
    for w in all_envs(env):
        if isinstance(w, EnvWrapper) and not isinstance(w, ActNormWrapper):
            raise ValueErr(msg=f"{who} takes a plain env or one inside an ActNormWrapper, not {type(w).__name__}")
    base = inner_env(env)
    if base.name == "bob-d":
        raise ValueErr(msg="the discrete-action family takes no playback policy")
    return base, any(isinstance(w, ActNormWrapper) for w in all_envs(env))


def vec_env_like(base, n: int, act_norm: bool):
    """a handle of n lanes built with the constructor arguments of the env `base`, auto-reset off"""
    from .vec_env import vec_env_of

    v = vec_env_of(base, n)
    v.set_act_norm(act_norm)
    v.set_auto_reset(False)
    return v


def domain_param_matrix(base, domain_params, names: Optional[Sequence[str]] = None) -> np.ndarray:
    """[P, all parameters of the family] float32: the domain parameters of the env `base` with every row's entries on top.
    domain_params: a list of P dicts (names missing from a dict keep the env's value), or a [P, n_names] array with names="""
    from .vec_env import param_names

    all_names = param_names(base.name)
    nominal = np.array([base.domain_param[k] for k in all_names], dtype=np.float32)
    if isinstance(domain_params, (list, tuple)) and (len(domain_params) == 0 or isinstance(domain_params[0], dict)):
        mat = np.tile(nominal, (len(domain_params), 1))
        for p, d in enumerate(domain_params):
            for k, val in d.items():
                if k not in all_names:
                    raise ValueErr(msg=f"unsupported domain parameter {k!r} for env {base.name}")
                mat[p, all_names.index(k)] = float(np.asarray(val).reshape(-1)[0])
        return mat
    arr = np.asarray(domain_params.detach().cpu().numpy() if hasattr(domain_params, "detach") else domain_params, dtype=np.float32)
    if names is None or arr.ndim != 2 or arr.shape[1] != len(names):
        raise ShapeErr(msg="domain_params: a list of dicts, or a [P, n_names] array together with names=")
    mat = np.tile(nominal, (arr.shape[0], 1))
    for c, k in enumerate(names):
        if k not in all_names:
            raise ValueErr(msg=f"unsupported domain parameter {k!r} for env {base.name}")
        mat[:, all_names.index(k)] = arr[:, c]
    return mat


class TrajectoryMatchResult:
    """loss [P, R]: sum over the compared steps k and observation rows d of w_d (obs_sim - obs_rec)^2 (fp32, device);
    steps [P, R]: how many steps went into each sum (int64, device): the segment's length, or fewer when the simulated episode
    ended early under the candidate's parameters."""

    def __init__(self, loss, steps):
        self.loss, self.steps = loss, steps

    def mean_loss(self):
        """[P]: a candidate's summed loss over its segments divided by the steps it took"""
        return self.loss.sum(dim=1) / self.steps.sum(dim=1).clamp(min=1).to(self.loss.dtype)


class TrajectoryMatchGradResult(TrajectoryMatchResult):
    """loss [P, R] and steps [P, R] as TrajectoryMatchResult (the same bits as evaluate()); grad [P, R, G]: d loss / d wrt[j];
    gn [P, R, G, G] or None: the Gauss-Newton matrix sum_k sum_d w_d J^T J, J = d obs_sim / d wrt (fp32, device); wrt: the names."""

    def __init__(self, loss, steps, grad, gn, wrt):
        super().__init__(loss, steps)
        self.grad, self.gn, self.wrt = grad, gn, tuple(wrt)

    def grad_per_candidate(self):
        """[P, G]: summed over the segments"""
        return self.grad.sum(dim=1)

    def gn_per_candidate(self):
        """[P, G, G]: summed over the segments"""
        if self.gn is None:
            raise ValueErr(msg="no Gauss-Newton matrix: evaluate_grad(..., gauss_newton=True)")
        return self.gn.sum(dim=1)

    def lm_step(self, damping: float = 1e-3):
        """[P, G]: the Levenberg-Marquardt step delta of every candidate, (GN + damping diag GN) delta = -grad / 2"""
        import torch

        gn = self.gn_per_candidate()
        lhs = gn + float(damping) * torch.diag_embed(torch.diagonal(gn, dim1=-2, dim2=-1))
        return torch.linalg.solve(lhs, -0.5 * self.grad_per_candidate().unsqueeze(-1)).squeeze(-1)


class TrajectoryMatchSampler:
    """Evaluate domain-parameter candidates against recorded segments.

    env: one of the pysim envs, optionally inside an ActNormWrapper (the recorded actions are then in [-1, 1] units); any other
    wrapper raises ValueErr.  act_recordings: R arrays [T_r, A]; obs_recordings: R arrays [T_r + 1, O], row k the observation
    after k steps; init_states: [R, S], the FULL state each segment starts from; obs_weights: [O] >= 0 or None (all 1)."""

    def __init__(self, env, act_recordings, obs_recordings, init_states, obs_weights=None, batch_lanes: int = 65536,
                 chunk: int = 128):
        self._base, self._act_norm = check_playback_env(env, "TrajectoryMatchSampler")
        self.env = env
        A, O, S = self._base.act_space.flat_dim, self._base.obs_space.flat_dim, self._base.state_space.flat_dim
        if len(act_recordings) < 1 or len(act_recordings) != len(obs_recordings):
            raise ShapeErr(msg="one observation recording per action recording, at least one")
        self._act, self._len = pad_recordings(act_recordings, A)
        self._obs, obs_len = pad_recordings(obs_recordings, O, extra_rows=1)
        if not np.array_equal(self._len, obs_len):
            raise ShapeErr(msg="an observation recording has one row more than its action recording")
        self._init = np.asarray(init_states, dtype=np.float32)
        if self._init.shape != (len(act_recordings), S):
            raise ShapeErr(given=self._init, expected_match=(len(act_recordings), S))
        self._weights = None if obs_weights is None else np.asarray(obs_weights, dtype=np.float32).reshape(-1)
        if batch_lanes < 1 or chunk < 1:
            raise ValueErr(msg="batch_lanes >= 1 and chunk >= 1")
        self._batch_lanes, self._chunk = int(batch_lanes), int(chunk)
        self._vec = None

    @property
    def num_segments(self) -> int:
        return int(self._act.shape[0])

    def close(self):
        if self._vec is not None:
            self._vec.close()
            self._vec = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _vec_for(self, n):
        """a handle of n lanes configured like the env, with the recordings and the target on it"""
        if self._vec is not None and self._vec.n_envs != n:
            self.close()
        if self._vec is None:
            v = vec_env_like(self._base, n, self._act_norm)
            v.set_policy_playback(self._act, self._len, batch_lane_rec(n // self.num_segments, self.num_segments))
            v.set_rollout_target(self._obs, self._weights)
            self._vec = v
        return self._vec

    def param_matrix(self, domain_params, names: Optional[Sequence[str]] = None) -> np.ndarray:
        """[P, all parameters of the family] float32: the env's current domain parameters with every candidate's entries on top"""
        return domain_param_matrix(self._base, domain_params, names)

    def _check_wrt(self, wrt, gauss_newton: bool) -> List[str]:
        """the validated list of parameter names to differentiate with respect to (needs no device)"""
        from .vec_env import param_names

        all_names = param_names(self._base.name)
        wrt = [wrt] if isinstance(wrt, str) else list(wrt)
        if len(wrt) < 1:
            raise ValueErr(msg="evaluate_grad: wrt names at least one domain parameter")
        for k in wrt:
            if k not in all_names:
                raise ValueErr(msg=f"unsupported domain parameter {k!r} for env {self._base.name}")
        if len(set(wrt)) != len(wrt):
            raise ValueErr(msg=f"evaluate_grad: a name is repeated in wrt={tuple(wrt)}")
        if gauss_newton and len(wrt) > L.VS_SENS_MAX_PARAMS:
            raise ValueErr(msg=f"evaluate_grad: more than {L.VS_SENS_MAX_PARAMS} parameters run in several passes, which leaves the "
                               "cross blocks of the Gauss-Newton matrix out: pass gauss_newton=False")
        return wrt

    def _run(self, mat, sens=None, gauss_newton=False):
        """The launch loop of evaluate() and evaluate_grad(): per batch of whole candidates set the parameters, reset to the
        segments' states, replay.  sens: the names of one pass of sensitivities, or None for the plain kernel.
        Returns (losses, steps, grads, gns): lists with one entry per batch (grads / gns empty without sens / gauss_newton)."""
        import torch

        P, R = mat.shape[0], self.num_segments
        t_max = int(self._len.max())
        losses, steps, grads, gns = [], [], [], []
        for p0, p1 in candidate_batches(P, R, self._batch_lanes):
            nc = p1 - p0
            n = nc * R
            v = self._vec_for(n)
            with v.on_current_stream():
                try:
                    if sens or getattr(v, "_sens_n", 0):
                        v.set_rollout_sens(sens)                         # (evaluate(): the plain kernel, no extra call)
                    v.set_params(np.repeat(mat[p0:p1], R, axis=0))      # lane p * R + r: candidate p
                    v.reset(init_state=np.tile(self._init, (nc, 1)))     # ... from segment r's recorded state (zeroes the sums)
                    done_t = v.tensor(L.VS_DONE)[0, :n]
                    t = 0
                    while t < t_max:
                        k = min(self._chunk, t_max - t)
                        v.step_policy(k, record=False)
                        t += k
                        if t < t_max and bool(done_t.bool().all()):  # one scalar sync per launch
                            break
                    lens = torch.as_tensor(np.tile(self._len, nc).astype(np.int64), device=done_t.device)
                    losses.append(v.rollout_loss().clone().reshape(nc, R))
                    steps.append(torch.minimum(v.tensor(L.VS_STEPCOUNT)[0, :n].to(torch.int64), lens).reshape(nc, R))
                    if sens:
                        grads.append(v.rollout_grad().clone().reshape(nc, R, len(sens)))
                        if gauss_newton:
                            gns.append(v.rollout_gn().reshape(nc, R, len(sens), len(sens)))
                finally:
                    if sens:
                        v.set_rollout_sens(None)
        return losses, steps, grads, gns

    def evaluate(self, domain_params, names: Optional[Sequence[str]] = None) -> TrajectoryMatchResult:
        """The discrepancy of every (candidate, segment) pair.  domain_params: a list of P dicts (names missing from a dict
        keep the env's value), or a [P, n_names] array with names=."""
        import torch

        mat = self.param_matrix(domain_params, names)
        R = self.num_segments
        losses, steps, _, _ = self._run(mat)
        if not losses:
            dev = f"cuda:{self._base._ctor.get('device', 0)}"
            return TrajectoryMatchResult(torch.zeros(0, R, device=dev), torch.zeros(0, R, dtype=torch.int64, device=dev))
        return TrajectoryMatchResult(torch.cat(losses), torch.cat(steps))

    def evaluate_grad(self, domain_params, names: Optional[Sequence[str]] = None, wrt: Sequence[str] = (),
                      gauss_newton: bool = True) -> TrajectoryMatchGradResult:
        """evaluate() together with the gradient of every pair's discrepancy with respect to the domain parameters named in wrt
        and, with gauss_newton, its Gauss-Newton matrix -- computed inside the rollout kernel by forward-mode sensitivities
        (vs_set_rollout_sens).  Up to VS_SENS_MAX_PARAMS names run in one pass; more run in passes of that many, with
        gauss_newton=False only."""
        import torch

        wrt = self._check_wrt(wrt, gauss_newton)
        mat = self.param_matrix(domain_params, names)
        R, G = self.num_segments, len(wrt)
        loss = step = None
        grad_cols, gn = [], None
        for g0 in range(0, G, L.VS_SENS_MAX_PARAMS):
            part = wrt[g0: g0 + L.VS_SENS_MAX_PARAMS]
            losses, steps, grads, gns = self._run(mat, sens=part, gauss_newton=gauss_newton)
            if not losses:
                dev = f"cuda:{self._base._ctor.get('device', 0)}"
                return TrajectoryMatchGradResult(torch.zeros(0, R, device=dev), torch.zeros(0, R, dtype=torch.int64, device=dev),
                                                 torch.zeros(0, R, G, device=dev),
                                                 torch.zeros(0, R, G, G, device=dev) if gauss_newton else None, wrt)
            if loss is None:
                loss, step = torch.cat(losses), torch.cat(steps)
            grad_cols.append(torch.cat(grads))
            if gauss_newton:
                gn = torch.cat(gns)
        return TrajectoryMatchGradResult(loss, step, torch.cat(grad_cols, dim=2), gn, wrt)
