"""Feature functions and the feature stack of Pyrado's linear policies (upstream Pyrado policies/features.py).

The elementwise functions map a tensor [..., O] to [..., O]; const_feat, MultFeat and ATan2Feat yield one feature each.
FeatureStack concatenates the values of its functions, in stack order, along the last dimension.  RBFFeat is not part of
this package."""
from typing import Callable, Sequence

import torch

from .exceptions import TypeErr, ValueErr


def const_feat(inp: torch.Tensor) -> torch.Tensor:
    """the constant 1: one feature, [..., O] -> [..., 1]"""
    return torch.ones(tuple(inp.shape[:-1]) + (1,), dtype=inp.dtype, device=inp.device)


def identity_feat(inp: torch.Tensor) -> torch.Tensor:
    return inp.clone()


def sign_feat(inp: torch.Tensor) -> torch.Tensor:
    return torch.sign(inp)


def abs_feat(inp: torch.Tensor) -> torch.Tensor:
    return torch.abs(inp)


def squared_feat(inp: torch.Tensor) -> torch.Tensor:
    return torch.pow(inp, 2)


def cubic_feat(inp: torch.Tensor) -> torch.Tensor:
    return torch.pow(inp, 3)


def sig_feat(inp: torch.Tensor) -> torch.Tensor:
    return torch.sigmoid(inp)


def bell_feat(inp: torch.Tensor) -> torch.Tensor:
    return torch.exp(-torch.pow(inp, 2) / 2)


def sin_feat(inp: torch.Tensor) -> torch.Tensor:
    return torch.sin(inp)


def cos_feat(inp: torch.Tensor) -> torch.Tensor:
    return torch.cos(inp)


def sinsin_feat(inp: torch.Tensor) -> torch.Tensor:
    return torch.sin(inp) * torch.sin(inp)


def sincos_feat(inp: torch.Tensor) -> torch.Tensor:
    return torch.sin(inp) * torch.cos(inp)


class MultFeat:
    """The product of at least two entries of the input: one feature, the last dimension kept"""

    def __init__(self, idcs: Sequence[int]):
        if not isinstance(idcs, (tuple, list)):
            raise TypeErr(given=idcs, expected_type=[tuple, list])
        if len(idcs) < 2:
            raise ValueErr(msg="Provide at least two indices.")
        self._idcs = [int(i) for i in idcs]

    @property
    def idcs(self) -> list:
        return list(self._idcs)

    def __call__(self, inp: torch.Tensor) -> torch.Tensor:
        return torch.prod(inp[..., self._idcs], dim=-1, keepdim=True)


class ATan2Feat:
    """atan2(inp[idx_sin], inp[idx_cos]): the angle of a (sin, cos) pair of the observation, one feature"""

    def __init__(self, idx_sin: int, idx_cos: int):
        self._idx_sin, self._idx_cos = int(idx_sin), int(idx_cos)

    @property
    def idcs(self) -> list:
        return [self._idx_sin, self._idx_cos]

    def __call__(self, inp: torch.Tensor) -> torch.Tensor:
        return torch.atan2(inp[..., self._idx_sin], inp[..., self._idx_cos]).unsqueeze(-1)


class FeatureStack:
    """Feature functions evaluated on the same input and concatenated, in order, along the last dimension"""

    def __init__(self, *feat_fcns: Callable):
        if len(feat_fcns) == 1 and isinstance(feat_fcns[0], (list, tuple)):  # (upstream also takes one sequence)
            feat_fcns = tuple(feat_fcns[0])
        self.feat_fcns = list(feat_fcns)

    def __str__(self):
        return "FeatureStack(" + ", ".join(getattr(f, "__name__", type(f).__name__) for f in self.feat_fcns) + ")"

    def __call__(self, inp: torch.Tensor) -> torch.Tensor:
        return torch.cat([f(inp) for f in self.feat_fcns], dim=-1)

    def get_num_feat(self, inp_flat_dim: int) -> int:
        """const_feat, MultFeat and ATan2Feat count one feature each, every other function inp_flat_dim"""
        num = 0
        for f in self.feat_fcns:
            if f is const_feat or isinstance(f, (MultFeat, ATan2Feat)):
                num += 1
            else:
                num += int(inp_flat_dim)
        return num
