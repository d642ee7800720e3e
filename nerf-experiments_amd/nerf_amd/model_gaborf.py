"""GaborF field MLPs (Gabor-activation radiance / proposal networks) on gfx950 kernels.

Mirrors, with the same class names, constructor arguments, submodule names and construction
order (so ``th.manual_seed`` gives the reference's initial parameters and state_dicts
interchange):
  * ``GaborAct``          gaborf/gabor.py:32-64 (GaborActivation autograd :8-29)
  * ``RadianceNetwork``   gaborf/model_radiance.py:9-91
  * ``ProposalNetwork``   gaborf/model_proposal.py:9-56
The learning-rate arguments are optional, as in model_garf.py; ``param_groups`` exist when they
are given.  Networks, lowering and forward are the GARF ones (field_family.py) with
y = exp(-z^2 (s^2 + 1e-6)) cos(spread z) per channel (nerf_param_act_fwd / _bwd, or the GEMM
epilogues of nerf_linear_act_x3).
"""
from __future__ import annotations

import math
from typing import Iterator

import torch as th
import torch.nn as nn

from . import _lib
from .field_family import FieldBase, ParamActFn, ProposalField, RadianceField, strip_compile_prefix


class GaborAct(nn.Module):
    def __init__(self, features_in: int, inv_standard_deviation_init_min: float = 0.,
                 inv_standard_deviation_init_max: float = 1.):
        super().__init__()
        # negative values allowed: only inv_std ** 2 is used (gabor.py:54-57)
        self.inv_standard_deviation = nn.Parameter(
            th.rand(features_in) * (inv_standard_deviation_init_max - inv_standard_deviation_init_min)
            + inv_standard_deviation_init_min)
        self.spread = nn.Parameter(th.rand(features_in) * 2 * math.pi)

    def forward(self, x: th.Tensor) -> th.Tensor:
        return ParamActFn.apply(_lib.NERF_ACT_GABOR, x, self.inv_standard_deviation, self.spread)


class _GaborfBase(FieldBase):
    _act_type = GaborAct

    def __init__(self, gaussian_init_min: float, gaussian_init_max: float):
        super().__init__()
        self.gaussian_init_min = gaussian_init_min
        self.gaussian_init_max = gaussian_init_max
        self._parameters_gabor = self._parameters_act

    def _make_act(self, features_in) -> GaborAct:
        return GaborAct(features_in, self.gaussian_init_min, self.gaussian_init_max)

    @staticmethod
    def _act_params(act):
        return (act.inv_standard_deviation, act.spread)

    @classmethod
    def _lower(cls, act):
        return {"act": (_lib.NERF_ACT_GABOR, cls._act_params(act))}

    def parameters_gabor(self) -> Iterator[nn.Parameter]:
        return iter(self._parameters_gabor)


class RadianceNetwork(_GaborfBase, RadianceField):
    def __init__(self, gaussian_init_min: float, gaussian_init_max: float, learning_rate_start: float | None = None,
                 learning_rate_stop: float | None = None, learning_rate_decay_end: float = 0,
                 gabor_learning_rate_factor: float = 1.0, weight_decay: float = 0.0):
        super().__init__(gaussian_init_min, gaussian_init_max)
        self._build()
        self._maybe_param_groups(learning_rate_start, learning_rate_stop, learning_rate_decay_end,
                                 gabor_learning_rate_factor, weight_decay)


class ProposalNetwork(_GaborfBase, ProposalField):
    def __init__(self, gaussian_init_min: float, gaussian_init_max: float, learning_rate_start: float | None = None,
                 learning_rate_stop: float | None = None, learning_rate_decay_end: float = 0,
                 gabor_learning_rate_factor: float = 1.0, weight_decay: float = 0.0):
        super().__init__(gaussian_init_min, gaussian_init_max)
        self._build()
        self._maybe_param_groups(learning_rate_start, learning_rate_stop, learning_rate_decay_end,
                                 gabor_learning_rate_factor, weight_decay)


__all__ = ["GaborAct", "RadianceNetwork", "ProposalNetwork", "strip_compile_prefix"]
