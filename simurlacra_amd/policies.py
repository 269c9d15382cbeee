"""The two trivial policies the reference's tests drive the envs with (P/policies/feed_forward/dummy.py:40-84)."""
import torch

from .features import (ATan2Feat, FeatureStack, MultFeat, abs_feat, bell_feat, const_feat, cos_feat, cubic_feat,  # noqa: F401
                       identity_feat, sig_feat, sign_feat, sin_feat, sincos_feat, sinsin_feat, squared_feat)


class Policy(torch.nn.Module):
    is_recurrent = False

    def __init__(self, spec):
        super().__init__()
        self.env_spec = spec

    def reset(self, **kwargs):
        pass


class IdlePolicy(Policy):
    """always zero (dummy.py:40-57)"""

    def forward(self, obs: torch.Tensor = None) -> torch.Tensor:
        shape = tuple(self.env_spec.act_space.shape)
        if obs is not None and obs.dim() == 2:
            shape = (obs.shape[0],) + shape
        return torch.zeros(shape, device=obs.device if obs is not None else None)


class DummyPolicy(Policy):
    """uniform random action in the action space, cast to fp32 (dummy.py:60-84); batched when obs is [N, O]"""

    def forward(self, obs: torch.Tensor = None) -> torch.Tensor:
        lo = torch.as_tensor(self.env_spec.act_space.bound_lo, dtype=torch.float32)
        hi = torch.as_tensor(self.env_spec.act_space.bound_up, dtype=torch.float32)
        if obs is not None and obs.dim() == 2:
            lo, hi = lo.to(obs.device), hi.to(obs.device)
            return lo + (hi - lo) * torch.rand(obs.shape[0], lo.numel(), device=obs.device)
        return torch.from_numpy(self.env_spec.act_space.sample_uniform()).to(torch.float32)


# ------------------------------------------------------------------------------------------------- feed-forward network
def _init_linear(m):
    """init_param for nn.Linear (P/policies/initialization.py:64-70): PyTorch's default initialisation"""
    from math import sqrt

    torch.nn.init.kaiming_uniform_(m.weight, a=sqrt(5))
    if m.bias is not None:
        fan_in = m.weight.shape[1]
        bound = 1 / sqrt(fan_in) if fan_in > 0 else 0
        torch.nn.init.uniform_(m.bias, -bound, bound)


class FNN(torch.nn.Module):
    """Feed-forward neural network (P/policies/feed_back/fnn.py:43-160): hidden Linear layers with a nonlinearity each, a
    Linear output layer with an optional one.  Parameters in the reference's order: hidden_layers.i.weight / .bias ...,
    output_layer.weight / .bias."""

    def __init__(self, input_size, output_size, hidden_sizes, hidden_nonlin, dropout=0.0, output_nonlin=None,
                 init_param_kwargs=None, use_cuda=False):
        super().__init__()
        self._device = "cuda" if use_cuda and torch.cuda.is_available() else "cpu"
        hidden_sizes = list(hidden_sizes)
        self.hidden_nonlin = list(hidden_nonlin) if isinstance(hidden_nonlin, (list, tuple)) else len(hidden_sizes) * [hidden_nonlin]
        self.dropout = dropout
        self.output_nonlin = output_nonlin
        self.hidden_layers = torch.nn.ModuleList()
        last = input_size
        for hs in hidden_sizes:
            self.hidden_layers.append(torch.nn.Linear(last, hs))
            last = hs
            if self.dropout > 0:
                self.hidden_layers.append(torch.nn.Dropout(p=self.dropout))
        self.output_layer = torch.nn.Linear(last, output_size)
        self.init_param(None, **(init_param_kwargs or {}))
        self.to(self._device)

    @property
    def device(self):
        return self._device

    @property
    def param_values(self):
        return torch.nn.utils.parameters_to_vector(self.parameters())

    @param_values.setter
    def param_values(self, param):
        torch.nn.utils.vector_to_parameters(param, self.parameters())

    def init_param(self, init_values=None, **kwargs):
        if init_values is None:
            for layer in list(self.hidden_layers) + [self.output_layer]:
                if isinstance(layer, torch.nn.Linear):
                    _init_linear(layer)
        else:
            self.param_values = init_values

    def forward(self, obs):
        p0 = next(self.parameters(), None)
        x = obs if p0 is None else obs.to(p0.device)  # (fnn.py: obs.to(self.device); a no-op on the same device, also under graph capture)
        for i, layer in enumerate(self.hidden_layers):
            x = layer(x)
            if self.dropout == 0:
                if self.hidden_nonlin[i] is not None:
                    x = self.hidden_nonlin[i](x)
            elif i % 2 == 0 and self.hidden_nonlin[i // 2] is not None:
                x = self.hidden_nonlin[i // 2](x)
        out = self.output_layer(x)
        return self.output_nonlin(out) if self.output_nonlin is not None else out


class FNNPolicy(Policy):
    """Feed-forward neural network policy (P/policies/feed_back/fnn.py:163-222).  The fork's forward() feeds the network
    [o_0, sin o_1, cos o_1, o_2 ..] -- its cartpole observes the state (quanser_cartpole.py:107-109 in the fork returns it
    unchanged), so row 1 is the pole angle -- and sizes the input layer obs_dim + 1 accordingly: `featurize=True` (default) is
    that behaviour, `featurize=False` the plain net(obs) of upstream Pyrado."""

    name = "fnn"

    def __init__(self, spec, hidden_sizes, hidden_nonlin, dropout=0.0, output_nonlin=None, init_param_kwargs=None,
                 use_cuda=False, featurize=True):
        super().__init__(spec)
        self.featurize = bool(featurize)
        # the reference's order (fnn.py:187-201): the net initialises once WITHOUT the kwargs, then the policy calls
        # init_param(None, **init_param_kwargs) -- the same draws from torch's RNG as the reference under the same seed
        self.net = FNN(spec.obs_space.flat_dim + (1 if self.featurize else 0), spec.act_space.flat_dim, hidden_sizes,
                       hidden_nonlin, dropout, output_nonlin, None, use_cuda)
        self.init_param(None, **(init_param_kwargs or {}))

    @property
    def param_values(self):
        return torch.nn.utils.parameters_to_vector(self.parameters())

    @param_values.setter
    def param_values(self, param):
        torch.nn.utils.vector_to_parameters(param, self.parameters())

    def init_param(self, init_values=None, **kwargs):
        if init_values is None:
            self.net.init_param(None, **kwargs)
        else:
            self.param_values = init_values

    def forward(self, obs):
        if self.featurize:
            obs = torch.cat([obs[..., 0:1], torch.sin(obs[..., 1:2]), torch.cos(obs[..., 1:2]), obs[..., 2:]], dim=-1)
        return self.net(obs)


# ------------------------------------------------------------------------------------------- linear policy on features
class LinearPolicy(Policy):
    """Linear policy on a stack of feature functions (upstream Pyrado policies/feed_forward/linear.py): act = net(feats(obs))
    with net = nn.Linear(num_feat, act_dim, bias=False), so param_values is net.weight flattened as [act_dim][num_feat], the
    features in stack order.  The parameters keep torch's default initialisation (init_param(None)); Pyrado's init_param draws
    are not reproduced."""

    name = "lin"

    def __init__(self, spec, feats: FeatureStack, init_param_kwargs=None, use_cuda=False):
        if not isinstance(feats, FeatureStack):
            from .exceptions import TypeErr

            raise TypeErr(given=feats, expected_type=FeatureStack)
        super().__init__(spec)
        self._feats = feats
        self.num_active_feat = feats.get_num_feat(spec.obs_space.flat_dim)
        self.net = torch.nn.Linear(self.num_active_feat, spec.act_space.flat_dim, bias=False)
        self.init_param(None, **(init_param_kwargs or {}))
        self.to("cuda" if use_cuda and torch.cuda.is_available() else "cpu")

    @property
    def features(self) -> FeatureStack:
        return self._feats

    @property
    def param_values(self):
        return torch.nn.utils.parameters_to_vector(self.parameters())

    @param_values.setter
    def param_values(self, param):
        torch.nn.utils.vector_to_parameters(param, self.parameters())

    def init_param(self, init_values=None, **kwargs):
        if init_values is None:
            _init_linear(self.net)
        else:
            self.param_values = init_values

    def eval_feats(self, obs: torch.Tensor) -> torch.Tensor:
        return self._feats(obs)

    def forward(self, obs: torch.Tensor) -> torch.Tensor:
        w = self.net.weight
        return self.net(self.eval_feats(obs.to(device=w.device, dtype=w.dtype)))


# ----------------------------------------------------------------------------------------------------- recurrent policies
class RecurrentPolicy(Policy):
    """A policy with a hidden state: forward(obs, hidden=None) -> (act, new_hidden) (P/policies/base.py RecurrentPolicy).
    The hidden state is one flat vector per env -- [H] unbatched, [N, H] batched -- and a rollout starts from init_hidden()."""

    is_recurrent = True

    @property
    def hidden_size(self) -> int:
        raise NotImplementedError

    def init_hidden(self, batch_size: int = None) -> torch.Tensor:
        p0 = next(self.parameters(), None)
        shape = (self.hidden_size,) if batch_size is None else (int(batch_size), self.hidden_size)
        return torch.zeros(shape, device=p0.device if p0 is not None else None)


class _RNNPolicyBase(RecurrentPolicy):
    """torch.nn.RNN / GRU / LSTM layers (bias, batch_first=False) and a Linear output layer (P/policies/recurrent/rnn.py).

    Packed hidden layout, Pyrado's: the h of layer 0, 1, .. concatenated, and for the LSTM the c of every layer behind them in
    the same order -- hidden_size = layers x units (x 2 for the LSTM).  Parameters in torch's order (param_values):
    rnn_layers.weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0, [.. _l1], output_layer.weight, output_layer.bias.
    The parameters keep torch's default initialisation (init_param(None)); Pyrado's init_param draws are not reproduced."""

    _rnn_cls = None

    def __init__(self, spec, hidden_size, num_recurrent_layers, output_nonlin=None, dropout=0.0, init_param_kwargs=None,
                 use_cuda=False, **rnn_kwargs):
        super().__init__(spec)
        self._hidden = int(hidden_size)
        self.num_recurrent_layers = int(num_recurrent_layers)
        self.dropout = float(dropout)
        self.output_nonlin = output_nonlin
        self.rnn_layers = self._rnn_cls(input_size=spec.obs_space.flat_dim, hidden_size=self._hidden,
                                        num_layers=self.num_recurrent_layers, bias=True, batch_first=False,
                                        dropout=self.dropout, **rnn_kwargs)
        self.output_layer = torch.nn.Linear(self._hidden, spec.act_space.flat_dim)
        self.init_param(None, **(init_param_kwargs or {}))
        self.to("cuda" if use_cuda and torch.cuda.is_available() else "cpu")

    @property
    def hidden_size(self) -> int:
        return self.num_recurrent_layers * self._hidden * (2 if self._rnn_cls is torch.nn.LSTM else 1)

    @property
    def param_values(self):
        return torch.nn.utils.parameters_to_vector(self.parameters())

    @param_values.setter
    def param_values(self, param):
        torch.nn.utils.vector_to_parameters(param, self.parameters())

    def init_param(self, init_values=None, **kwargs):
        if init_values is not None:
            self.param_values = init_values

    def _unpack(self, hidden):  # [N, hidden_size] -> the module's [layers, N, units] (LSTM: a pair)
        n, L, u = hidden.shape[0], self.num_recurrent_layers, self._hidden
        if self._rnn_cls is torch.nn.LSTM:
            h = hidden[:, :L * u].reshape(n, L, u).transpose(0, 1).contiguous()
            c = hidden[:, L * u:].reshape(n, L, u).transpose(0, 1).contiguous()
            return h, c
        return hidden.reshape(n, L, u).transpose(0, 1).contiguous()

    def _pack(self, hidden):
        if self._rnn_cls is torch.nn.LSTM:
            h, c = hidden
            return torch.cat([h.transpose(0, 1).reshape(h.shape[1], -1), c.transpose(0, 1).reshape(c.shape[1], -1)], dim=1)
        return hidden.transpose(0, 1).reshape(hidden.shape[1], -1)

    def forward(self, obs, hidden=None):
        p0 = next(self.parameters())
        obs = obs.to(device=p0.device, dtype=p0.dtype)
        batched = obs.dim() == 2
        x = obs if batched else obs.unsqueeze(0)
        if hidden is None:
            hidden = self.init_hidden(x.shape[0])
        hd = hidden.to(device=p0.device, dtype=p0.dtype)
        hd = hd if hd.dim() == 2 else hd.unsqueeze(0)
        out, new = self.rnn_layers(x.unsqueeze(0), self._unpack(hd))  # one time step of a batch
        act = self.output_layer(out.squeeze(0))
        if self.output_nonlin is not None:
            act = self.output_nonlin(act)
        new = self._pack(new)
        return (act, new) if batched else (act.squeeze(0), new.squeeze(0))


class RNNPolicy(_RNNPolicyBase):
    """Elman RNN policy (P/policies/recurrent/rnn.py RNNPolicy): hidden_nonlin 'tanh' | 'relu'"""

    name = "rnn"
    _rnn_cls = torch.nn.RNN

    def __init__(self, spec, hidden_size, num_recurrent_layers, hidden_nonlin="tanh", output_nonlin=None, dropout=0.0,
                 init_param_kwargs=None, use_cuda=False):
        if hidden_nonlin not in ("tanh", "relu"):
            raise ValueError(f"hidden_nonlin must be 'tanh' or 'relu', got {hidden_nonlin!r}")
        self.hidden_nonlin = hidden_nonlin
        super().__init__(spec, hidden_size, num_recurrent_layers, output_nonlin, dropout, init_param_kwargs, use_cuda,
                         nonlinearity=hidden_nonlin)


class GRUPolicy(_RNNPolicyBase):
    """GRU policy (P/policies/recurrent/rnn.py GRUPolicy)"""

    name = "gru"
    _rnn_cls = torch.nn.GRU


class LSTMPolicy(_RNNPolicyBase):
    """LSTM policy (P/policies/recurrent/rnn.py LSTMPolicy); the packed hidden state is [h of every layer | c of every layer]"""

    name = "lstm"
    _rnn_cls = torch.nn.LSTM


class NormalActNoiseExplStrat(Policy):
    """Gaussian noise on the actions of a wrapped policy (P/exploration/stochastic_action.py:121-180, shallow form: a fixed
    or externally updated diagonal std)"""

    def __init__(self, policy, std_init, std_min=1e-3):
        super().__init__(policy.env_spec)
        self.policy = policy
        n = policy.env_spec.act_space.flat_dim
        std = torch.as_tensor(std_init, dtype=torch.float32).reshape(-1)
        # a buffer: policy.to(device) moves it (a pageable CPU tensor copied inside forward() is a synchronous host-to-device
        # copy, illegal during the stream capture of ParallelRolloutSampler(graph_policy=True))
        self.register_buffer("std", torch.clamp(std.expand(n).clone(), min=float(std_min)))

    def reset(self, **kwargs):
        self.policy.reset(**kwargs)

    @property
    def is_recurrent(self):
        return bool(getattr(self.policy, "is_recurrent", False))

    @property
    def hidden_size(self):
        return self.policy.hidden_size

    def init_hidden(self, batch_size=None):
        return self.policy.init_hidden(batch_size)

    def forward(self, obs, hidden=None):
        if self.is_recurrent:  # the noise goes on the action only, never into the hidden state
            act, hidden = self.policy(obs, hidden)
        else:
            act = self.policy(obs)
        std = self.std if self.std.device == act.device else self.std.to(act.device)
        act = act + std.to(act.dtype) * torch.randn_like(act)
        return (act, hidden) if self.is_recurrent else act


_NONLIN_NAMES = {torch.tanh: "tanh", torch.nn.functional.tanh: "tanh", torch.relu: "relu", torch.nn.functional.relu: "relu",
                 torch.sigmoid: "sigmoid", torch.nn.functional.sigmoid: "sigmoid", None: None}


def _nonlin_name(f):
    if isinstance(f, torch.nn.Tanh):
        return "tanh"
    if isinstance(f, torch.nn.ReLU):
        return "relu"
    if isinstance(f, torch.nn.Sigmoid):
        return "sigmoid"
    if isinstance(f, torch.nn.Identity):
        return None
    return _NONLIN_NAMES[f]  # KeyError: not a nonlinearity the kernel has


def fnn_kernel_spec(policy):
    """The arguments of VecSimEnv.set_policy_fnn for a policy the fused kernel can evaluate itself -- an FNN / FNNPolicy of at
    most 4 hidden layers of at most 64 units, tanh / relu / sigmoid / no nonlinearities, no dropout, optionally inside a
    NormalActNoiseExplStrat -- or None (the sampler then keeps the policy in torch, one vs_step_record per step)."""
    noise_std = None
    if isinstance(policy, NormalActNoiseExplStrat):
        noise_std = policy.std.detach().cpu().numpy()
        policy = policy.policy
    feat = False
    if isinstance(policy, FNNPolicy):
        feat, net = policy.featurize, policy.net
    elif isinstance(policy, FNN):
        net = policy
    else:
        return None
    if net.dropout > 0:
        return None
    sizes = [layer.out_features for layer in net.hidden_layers]
    if not 1 <= len(sizes) <= 4 or max(sizes) > 64:
        return None
    try:
        hidden_nonlin = [_nonlin_name(f) for f in net.hidden_nonlin[:len(sizes)]]
        output_nonlin = _nonlin_name(net.output_nonlin)
    except (KeyError, TypeError):
        return None
    return dict(params=torch.nn.utils.parameters_to_vector(net.parameters()).detach().to(torch.float32),
                hidden_sizes=sizes, hidden_nonlin=hidden_nonlin, output_nonlin=output_nonlin, feat=feat, noise_std=noise_std)


_RNN_CELL_NAMES = {torch.nn.GRU: "gru", torch.nn.LSTM: "lstm"}


def rnn_kernel_spec(policy):
    """The arguments of VecSimEnv.set_policy_rnn for a recurrent policy the fused kernel can evaluate itself -- RNNPolicy
    (tanh / relu), GRUPolicy or LSTMPolicy of 1 or 2 layers of at most 64 units, no dropout, no projection, one direction, an
    output nonlinearity None / tanh / relu / sigmoid, optionally inside a NormalActNoiseExplStrat -- or None (the sampler then
    keeps the policy in torch)."""
    noise_std = None
    if isinstance(policy, NormalActNoiseExplStrat):
        noise_std = policy.std.detach().cpu().numpy()
        policy = policy.policy
    if not isinstance(policy, _RNNPolicyBase):
        return None
    m = policy.rnn_layers
    if not 1 <= m.num_layers <= 2 or not 1 <= m.hidden_size <= 64 or m.dropout > 0 or m.bidirectional:
        return None
    if getattr(m, "proj_size", 0) or not m.bias or m.batch_first:
        return None
    if isinstance(m, torch.nn.RNN):
        cell = m.nonlinearity
    else:
        cell = _RNN_CELL_NAMES.get(type(m))
    if cell not in ("tanh", "relu", "gru", "lstm") or m.input_size > 8:
        return None
    try:
        output_nonlin = _nonlin_name(policy.output_nonlin)
    except (KeyError, TypeError):
        return None
    return dict(params=torch.nn.utils.parameters_to_vector(policy.parameters()).detach().to(torch.float32), cell=cell,
                n_layers=m.num_layers, hidden_size=m.hidden_size, output_nonlin=output_nonlin, noise_std=noise_std)


# feature function -> the kind name VecSimEnv.set_policy_linear takes (every elementwise function and the constant)
_FEAT_NAMES = {identity_feat: "identity", sign_feat: "sign", abs_feat: "abs", squared_feat: "squared", cubic_feat: "cubic",
               sig_feat: "sig", bell_feat: "bell", sin_feat: "sin", cos_feat: "cos", sinsin_feat: "sinsin",
               sincos_feat: "sincos", const_feat: "const"}
LIN_MAX_FEAT, LIN_MAX_XTERMS = 128, 39  # the fused kernel's caps: features in all, MultFeat / ATan2Feat terms


def linear_kernel_spec(policy):
    """The arguments of VecSimEnv.set_policy_linear for a LinearPolicy whose FeatureStack the fused kernel can take -- every
    elementwise function and const_feat at most once, MultFeat of 2 .. 4 rows, ATan2Feat, at most 39 of the latter two and 128
    features in all -- optionally inside a NormalActNoiseExplStrat, or None (the sampler then keeps the policy in torch).
    terms: [(kind name, indices)] in stack order; the indices count the rows the policy sees."""
    noise_std = None
    if isinstance(policy, NormalActNoiseExplStrat):
        noise_std = policy.std.detach().cpu().numpy()
        policy = policy.policy
    if not isinstance(policy, LinearPolicy):
        return None
    n_vis = policy.env_spec.obs_space.flat_dim
    terms, seen, n_x = [], set(), 0
    for f in policy.features.feat_fcns:
        if isinstance(f, (MultFeat, ATan2Feat)):
            idcs = tuple(f.idcs)
            if len(idcs) > 4 or any(not 0 <= i < n_vis for i in idcs):
                return None
            n_x += 1
            terms.append(("mult" if isinstance(f, MultFeat) else "atan2", idcs))
            continue
        try:
            name = _FEAT_NAMES.get(f)
        except TypeError:  # (an unhashable callable)
            name = None
        if name is None or name in seen:
            return None
        seen.add(name)
        terms.append((name, ()))
    if n_vis > 8 or n_x > LIN_MAX_XTERMS or not terms or policy.num_active_feat > LIN_MAX_FEAT:
        return None
    return dict(params=policy.net.weight.detach().to(torch.float32).reshape(-1), terms=terms, noise_std=noise_std)


_LIN_KINDS = ("identity", "sign", "abs", "squared", "cubic", "sig", "bell", "sin", "cos", "sinsin", "sincos", "const", "mult",
              "atan2")  # the library's kind codes (VS_FEAT_*), in order


def linear_slot_map(terms, n_vis, act_dim):
    """The index map of the library's packer for a linear policy, restated: entry [j * 128 + slot] = the index into the flat
    torch parameter vector ([act_dim][num_feat]) of the weight the fused kernel reads in that slot of action row j, -1 where
    the stack has no feature.  Slot order of a row, whatever the stack's order: elementwise kind q (the order of the
    VS_FEAT_* codes) of visible row k at 8 q + k, the constant at 88, the i-th MultFeat / ATan2Feat term at 89 + i."""
    slots, n_x = [], 0
    for name, _ in terms:
        q = _LIN_KINDS.index(name)
        if q < 11:
            slots += [8 * q + k for k in range(n_vis)]
        elif q == 11:
            slots.append(88)
        else:
            slots.append(89 + n_x)
            n_x += 1
    num_feat = len(slots)
    out = [-1] * (act_dim * 128)
    for j in range(act_dim):
        for f, sl in enumerate(slots):
            out[j * 128 + sl] = j * num_feat + f
    return out


# ------------------------------------------------------------------------------------------------- open-loop policies
class PlaybackPolicy(Policy):
    """Replays recorded actions, whatever the observation (upstream Pyrado policies/feed_forward/playback.py).
    act_recordings: a list of [T_r, A] arrays.  reset() moves to the next recording, cyclically, and rewinds it -- the first
    reset() selects recording 0 -- unless no_reset is set; forward() returns the current row and advances, zeros once the
    recording has ended."""

    name = "pb"

    def __init__(self, spec, act_recordings, no_reset: bool = False, use_cuda=False):
        import numpy as np

        super().__init__(spec)
        if not isinstance(act_recordings, (list, tuple)) or len(act_recordings) == 0:
            from .exceptions import TypeErr

            raise TypeErr(given=act_recordings, expected_type=list)
        A = spec.act_space.flat_dim
        self._recs = []
        for r in act_recordings:
            arr = np.asarray(r.detach().cpu().numpy() if hasattr(r, "detach") else r, dtype=np.float32)
            arr = arr.reshape(-1, A) if arr.ndim <= 1 else arr
            if arr.ndim != 2 or arr.shape[1] != A:
                from .exceptions import ShapeErr

                raise ShapeErr(given=arr, expected_match=(arr.shape[0], A))
            self._recs.append(torch.from_numpy(np.ascontiguousarray(arr)))
        self._no_reset = bool(no_reset)
        self._curr_rec = -1
        self._curr_step = 0
        self._tables = {}

    @property
    def num_rec(self) -> int:
        return len(self._recs)

    @property
    def curr_rec(self) -> int:
        return self._curr_rec

    @property
    def curr_step(self) -> int:
        return self._curr_step

    @property
    def no_reset(self) -> bool:
        return self._no_reset

    @no_reset.setter
    def no_reset(self, value: bool):
        self._no_reset = bool(value)

    def init_param(self, init_values=None, **kwargs):
        pass

    def reset(self, **kwargs):
        if not self._no_reset:
            self._curr_rec = (self._curr_rec + 1) % len(self._recs)
            self._curr_step = 0

    def forward(self, obs: torch.Tensor = None) -> torch.Tensor:
        rec = self._recs[max(self._curr_rec, 0)]  # (before the first reset: recording 0)
        act = rec[self._curr_step].clone() if self._curr_step < rec.shape[0] else torch.zeros(rec.shape[1])
        self._curr_step += 1
        return act

    def table(self):
        """(actions [n_rec, t_len, A] float32, zero beyond a recording's end, lengths [n_rec] int64), t_len >= 1"""
        t_len = max(1, max(r.shape[0] for r in self._recs))
        tab = torch.zeros(len(self._recs), t_len, self._recs[0].shape[1])
        for k, r in enumerate(self._recs):
            tab[k, : r.shape[0]] = r
        return tab, torch.tensor([r.shape[0] for r in self._recs], dtype=torch.int64)

    def actions_at(self, steps, recs) -> torch.Tensor:
        """The actions [n, A] of n independent replays: entry i is row steps[i] of recording recs[i], zeros from that
        recording's end on (what forward() returns at that step after the reset that selected that recording).  steps / recs:
        integer tensors or arrays [n]; the result lives on the device of `steps`."""
        steps = torch.as_tensor(steps).to(torch.int64).reshape(-1)
        dev = steps.device
        recs = torch.as_tensor(recs).to(device=dev, dtype=torch.int64).reshape(-1)
        if dev not in self._tables:
            tab, lens = self.table()
            self._tables[dev] = (tab.to(dev), lens.to(dev))
        tab, lens = self._tables[dev]
        inside = (steps >= 0) & (steps < lens[recs])
        rows = tab[recs, steps.clamp(0, tab.shape[1] - 1)]
        return torch.where(inside[:, None], rows, torch.zeros_like(rows))


class TimePolicy(Policy):
    """An action that is a function of the time since the last reset (upstream Pyrado policies/feed_forward/time.py):
    forward() returns fcn_of_time(t) and then advances t by dt; reset() sets t = 0.  t is a Python float, accumulated by
    repeated addition -- tabulate() accumulates it the same way, so a table holds the floats forward() returns."""

    name = "time"

    def __init__(self, spec, fcn_of_time, dt: float, use_cuda=False):
        if not callable(fcn_of_time):
            from .exceptions import TypeErr

            raise TypeErr(given=fcn_of_time, expected_type="callable")
        super().__init__(spec)
        self._fcn_of_time = fcn_of_time
        self._dt = float(dt)
        self._curr_time = 0.0

    def init_param(self, init_values=None, **kwargs):
        pass

    def reset(self, **kwargs):
        self._curr_time = 0.0

    def _eval(self, t: float) -> torch.Tensor:
        return torch.as_tensor(self._fcn_of_time(t), dtype=torch.float32).reshape(-1)

    def forward(self, obs: torch.Tensor = None) -> torch.Tensor:
        act = self._eval(self._curr_time)
        self._curr_time += self._dt
        return act

    def tabulate(self, num_steps: int) -> torch.Tensor:
        """[num_steps, A]: what num_steps forward() calls after a reset() return (the policy's own clock is left alone)"""
        t, rows = 0.0, []
        for _ in range(int(num_steps)):
            rows.append(self._eval(t))
            t += self._dt
        return torch.stack(rows) if rows else torch.zeros(0, self.env_spec.act_space.flat_dim)


def playback_kernel_spec(policy, max_steps=None):
    """The arguments of VecSimEnv.set_policy_playback for an open-loop policy -- dict(actions=[n_rec, t_len, A] float32 array,
    zero beyond each recording's end, rec_len=[n_rec] int32) -- or None for every other policy.  A PlaybackPolicy gives one
    table row per recording; a TimePolicy one recording of max_steps rows (None without max_steps: an unbounded table)."""
    import numpy as np

    if isinstance(policy, PlaybackPolicy):
        tab, lens = policy.table()
        return dict(actions=tab.numpy(), rec_len=lens.numpy().astype(np.int32))
    if isinstance(policy, TimePolicy):
        if max_steps is None or not np.isfinite(max_steps) or int(max_steps) < 1:
            return None
        tab = policy.tabulate(int(max_steps))
        return dict(actions=tab.numpy()[None].copy(), rec_len=np.array([int(max_steps)], dtype=np.int32))
    return None
