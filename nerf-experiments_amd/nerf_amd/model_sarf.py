"""SARF field MLPs (Sarf-activation radiance / proposal networks) on gfx950 kernels.

Mirrors, with the same class names, constructor arguments, submodule names and construction
order (so ``th.manual_seed`` gives the reference's initial parameters):
  * ``SarfAct``           sarf/activation.py:40-65 — the ``cos(f / (x^2 + 1/f^2)) * exp(-x^2)`` form
                          its forward returns, x = |z| + 1e-4 (not the commented-out SarfActivation)
  * ``RadianceNetwork``   sarf/model_radiance.py:9-96 (its Sequentials are built under ``th.compile``,
                          whose state_dict keys carry an extra ``_orig_mod.`` — see
                          ``strip_compile_prefix``)
  * ``ProposalNetwork``   sarf/model_proposal.py:9-56
The learning-rate arguments are optional, as in model_garf.py; ``param_groups`` exist when they
are given.  Networks, lowering and forward are the GARF ones (field_family.py).

``frequency == 0`` is outside the contract: 1 / f^2 is infinite and the reference's own gradient
is not finite there.  (The reference initialises f in [0.5, 2].)
"""
from __future__ import annotations

from typing import Iterator

import torch as th
import torch.nn as nn

from . import _lib
from .field_family import FieldBase, ParamActFn, ProposalField, RadianceField, strip_compile_prefix


class SarfAct(nn.Module):
    def __init__(self, features_in: int, frequency_init_min: float, frequency_init_max: float):
        super().__init__()
        self.frequency = nn.Parameter(
            th.rand(features_in) * (frequency_init_max - frequency_init_min) + frequency_init_min)

    def forward(self, x: th.Tensor) -> th.Tensor:
        return ParamActFn.apply(_lib.NERF_ACT_SARF, x, self.frequency)


class _SarfBase(FieldBase):
    _act_type = SarfAct

    def __init__(self, frequency_init_min: float, frequency_init_max: float):
        super().__init__()
        self.frequency_init_min = frequency_init_min
        self.frequency_init_max = frequency_init_max
        self._parameters_activation = self._parameters_act

    def _make_act(self, features_in) -> SarfAct:
        return SarfAct(features_in, self.frequency_init_min, self.frequency_init_max)

    @staticmethod
    def _act_params(act):
        return (act.frequency,)

    @classmethod
    def _lower(cls, act):
        return {"act": (_lib.NERF_ACT_SARF, cls._act_params(act))}

    def parameters_activation(self) -> Iterator[nn.Parameter]:
        return iter(self._parameters_activation)


class RadianceNetwork(_SarfBase, RadianceField):
    def __init__(self, frequency_init_min: float, frequency_init_max: float, learning_rate_start: float | None = None,
                 learning_rate_stop: float | None = None, learning_rate_decay_end: float = 0,
                 activation_learning_rate_factor: float = 1.0, weight_decay: float = 0.0):
        super().__init__(frequency_init_min, frequency_init_max)
        self._build()
        self._maybe_param_groups(learning_rate_start, learning_rate_stop, learning_rate_decay_end,
                                 activation_learning_rate_factor, weight_decay)


class ProposalNetwork(_SarfBase, ProposalField):
    def __init__(self, frequency_init_min: float, frequency_init_max: float, learning_rate_start: float | None = None,
                 learning_rate_stop: float | None = None, learning_rate_decay_end: float = 0,
                 activation_learning_rate_factor: float = 1.0, weight_decay: float = 0.0):
        super().__init__(frequency_init_min, frequency_init_max)
        self._build()
        self._maybe_param_groups(learning_rate_start, learning_rate_stop, learning_rate_decay_end,
                                 activation_learning_rate_factor, weight_decay)


__all__ = ["SarfAct", "RadianceNetwork", "ProposalNetwork", "strip_compile_prefix"]
