"""GARF field MLPs (Gaussian-activation radiance / proposal networks) on gfx950 kernels.

Mirrors, with the same class names, constructor arguments, submodule names and construction
order (so ``th.manual_seed`` gives the reference's initial parameters and state_dicts
interchange):
  * ``GaussAct``          garf/gaussian.py:34-63 (GaussActivation autograd :8-31); copy barf/gaussian.py
  * ``RadianceNetwork``   barf/model_garf_radiance.py:10-113 (garf/model_radiance.py:9-96 is the
                          same network built under ``th.compile``, whose state_dict keys carry an
                          extra ``_orig_mod.`` — see ``strip_compile_prefix``)
  * ``ProposalNetwork``   barf/model_garf_proposal.py:10-77 (garf/model_proposal.py:9-56)
The learning-rate arguments of the barf copies are optional, so the garf two-argument
constructor works too; ``param_groups`` exist when they are given.

Each network runs as ONE ``MLPFunction`` autograd node: every Linear on the MFMA linear
kernels (fp32 or 3 x bf16 split, per ``torch.get_float32_matmul_precision``), each Gaussian
activation in ``nerf_gauss_act_fwd/bwd`` (per-channel inverse-std gradient reduced in a fixed
order), RadianceNetwork's ``z1[:, :128] + z2[:, :128]`` folded into the accumulate epilogue of
the last density layer, and the concatenations ``[z1 | pos]`` / ``[z1 + z2 | dir]`` read as
multi-segment GEMM operands (never materialised).  Only the final softplus / sigmoid heads are
applied with torch ops, as in NerfModel.forward.  The topology, its lowering and the forward are
shared with the GaborF / SARF networks (field_family.py).
"""
from __future__ import annotations

from typing import Iterator

import torch as th
import torch.nn as nn

from . import kernels as K
from .field_family import FieldBase, ProposalField, RadianceField, strip_compile_prefix


class _GaussActFn(th.autograd.Function):
    @staticmethod
    def forward(ctx, x, inv_std):
        K._require_cuda_f32("x", x)
        if x.dim() != 2 or x.shape[1] != inv_std.shape[0]:
            raise ValueError(f"GaussAct expects [batch, {inv_std.shape[0]}] input, got {tuple(x.shape)}")
        if x.stride(1) != 1:
            x = x.contiguous()
        y = th.empty(x.shape, device=x.device, dtype=th.float32)
        K.gauss_act_fwd(x, x.shape[1], inv_std, y)
        ctx.save_for_backward(x, inv_std)
        return y

    @staticmethod
    def backward(ctx, g):
        x, inv_std = ctx.saved_tensors
        g = g.contiguous()
        dx = th.empty_like(x)
        ds = th.empty_like(inv_std)
        K.gauss_act_bwd(g, x, x.shape[1], inv_std, dx, ds)
        return dx, ds


class GaussAct(nn.Module):
    def __init__(self, features_in: int, inv_standard_deviation_init_min: float = 0.,
                 inv_standard_deviation_init_max: float = 1.):
        super().__init__()
        # negative values allowed: only inv_std ** 2 is used (gaussian.py:56-59)
        self.inv_standard_deviation = nn.Parameter(
            th.rand(features_in) * (inv_standard_deviation_init_max - inv_standard_deviation_init_min)
            + inv_standard_deviation_init_min)

    def forward(self, x: th.Tensor) -> th.Tensor:
        return _GaussActFn.apply(x, self.inv_standard_deviation)


class _GarfBase(FieldBase):
    _act_type = GaussAct

    def __init__(self, gaussian_init_min: float, gaussian_init_max: float):
        super().__init__()
        self.gaussian_init_min = gaussian_init_min
        self.gaussian_init_max = gaussian_init_max
        self._parameters_gaussian = self._parameters_act

    def _make_act(self, features_in) -> GaussAct:
        return GaussAct(features_in, self.gaussian_init_min, self.gaussian_init_max)

    @staticmethod
    def _act_params(act):
        return (act.inv_standard_deviation,)

    @classmethod
    def _lower(cls, act):
        return {"gauss": act.inv_standard_deviation}

    def parameters_gaussian(self) -> Iterator[nn.Parameter]:
        return iter(self._parameters_gaussian)


class RadianceNetwork(_GarfBase, RadianceField):
    def __init__(self, gaussian_init_min: float, gaussian_init_max: float, learning_rate_start: float | None = None,
                 learning_rate_stop: float | None = None, learning_rate_decay_end: float = 0,
                 gaussian_learning_rate_factor: float = 1.0, weight_decay: float = 0.0):
        super().__init__(gaussian_init_min, gaussian_init_max)
        self._build()
        self._maybe_param_groups(learning_rate_start, learning_rate_stop, learning_rate_decay_end,
                                 gaussian_learning_rate_factor, weight_decay)


class ProposalNetwork(_GarfBase, ProposalField):
    def __init__(self, gaussian_init_min: float, gaussian_init_max: float, learning_rate_start: float | None = None,
                 learning_rate_stop: float | None = None, learning_rate_decay_end: float = 0,
                 gaussian_learning_rate_factor: float = 1.0, weight_decay: float = 0.0):
        super().__init__(gaussian_init_min, gaussian_init_max)
        self._build()
        self._maybe_param_groups(learning_rate_start, learning_rate_stop, learning_rate_decay_end,
                                 gaussian_learning_rate_factor, weight_decay)


__all__ = ["GaussAct", "RadianceNetwork", "ProposalNetwork", "strip_compile_prefix"]
