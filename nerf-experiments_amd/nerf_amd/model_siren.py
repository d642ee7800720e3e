"""SIREN field networks on gfx950 kernels, with the reference's nerf-siren module API.

* ``LinearSine(in_features, out_features, scale=1.0, first_layer=False)`` (nerf-siren/
  linear_sine.py:8-45): ``sin(Linear(scale * x))`` with the ``scale`` buffer (omega_0 per input
  column), the constructor's checks and the SIREN initialisation in the reference's order, so
  ``th.manual_seed`` gives its parameters.  On its own it is one autograd node: the split-precision
  GEMM with the sine in its epilogue (nerf_linear_sine_x3), or at "highest" matmul precision the fp32
  GEMM followed by nerf_sine_act_fwd / _bwd; gradients for ``x``, ``weight`` and ``bias``.
* ``NerfModel(input_scale)`` (nerf-siren/nerf_model.py:7-74): ``model_density_1`` (4 LinearSine),
  ``model_density_2`` (3 LinearSine on ``[z | pos]`` and a Linear to 256 + 3 + 1 columns) and
  ``model_color`` (LinearSine on ``[rgb_latent | dir]`` and a Linear to 3), lowered to ONE ``MLPPlan``
  / ``MLPFunction`` node of 10 layers as the GARF family's RadianceField is: the two concatenations
  are multi-segment GEMM operands, the base colour columns 256..258 and the density column 259 of the
  260-wide layer leave as ``[M]`` column outputs, and only ``softplus(. - 1, threshold=8)`` and
  ``sigmoid`` are torch ops.  ``forward(pos, dir) -> (density, rgb)``, the reference's order (GARF's
  RadianceNetwork returns them the other way round).
  ``scale`` is 1 on every hidden column and ``input_scale`` on the ``pos`` / ``dir`` columns, so the
  hidden activations are never scaled: the two ``[M, 3]`` inputs are multiplied once per forward
  where they are padded to 4 columns, which is the reference's own ``scale * x`` on those columns
  (``weight.grad`` therefore is the reference's), and the gradient hands the factor back.
* ``NerfSiren(near_sphere_normalized, far_sphere_normalized, samples_per_ray_fine,
  samples_per_ray_coarse, learning_rate=1e-4, learning_rate_decay=0.5, weight_decay=0.0)``
  (nerf-siren/model.py:9-325): ``model_coarse`` and ``model_fine = NerfModel(32)`` under the renderer
  it shares with NaiveINGP (model_ingp.CoarseFineRenderer); ``forward -> (rgb_fine, rgb_coarse)``,
  ``training_loss`` (the step helper without logging) and ``configure_optimizers`` (Adam +
  ExponentialLR, model.py:311-325).  An ``nn.Module``; INTEGRATION.md gives the Lightning mix-in.
"""
from __future__ import annotations

from math import sqrt

import torch as th
import torch.nn as nn
import torch.nn.functional as F

from . import kernels as K
from .mlp import LayerPlan, MLPFunction, MLPPlan, Source
from .model_ingp import CoarseFineRenderer


class _ScalePad4Fn(th.autograd.Function):
    """[M, 3] -> [M, 4] = [scale * x | 0]: the input scale of the SIREN first / skip / colour layers
    applied where the MFMA kernels' 16-byte operand rows are formed; backward scale * g[:, :3]."""

    @staticmethod
    def forward(ctx, x, scale: float):
        ctx.scale = scale
        x = (x if scale == 1.0 else x * scale).contiguous()
        params = K.make_pe_params(0, 0, True, 1.0)
        return K.encode_fwd(params, 3, x=x, n_samples=x.shape[0], n_rays=x.shape[0], out_ld=4, device=x.device)

    @staticmethod
    def backward(ctx, g):
        g = g[:, :3]
        return (g if ctx.scale == 1.0 else g * ctx.scale), None


def _scale_pad4(x: th.Tensor, scale: float) -> th.Tensor:
    if x.dim() != 2 or x.shape[1] != 3:
        raise ValueError(f"expected [batch, 3] input, got {tuple(x.shape)}")
    K._require_cuda_f32("input", x)
    return _ScalePad4Fn.apply(x, float(scale))


class LinearSine(nn.Module):
    def __init__(self, in_features: int, out_features: int, scale: float | th.Tensor = 1.0,
                 first_layer: bool = False):
        if isinstance(scale, int):
            scale = float(scale)
        if isinstance(scale, float):
            assert scale > 0, "Scale must be positive."
        elif isinstance(scale, th.Tensor):
            assert scale.shape[0] == in_features, "Scale must have the same dimensionality as input features."
            assert all(scale > 0), "Scale must be positive."
        else:
            raise TypeError("Scale must be either a float or a tensor.")
        super().__init__()
        # omega_0 of the SIREN paper, per input column
        self.register_buffer("scale", th.ones(in_features) * scale)
        self.first_layer = first_layer
        self.linear = nn.Linear(in_features, out_features)
        self.reset_parameters()
        self._plan: MLPPlan | None = None

    @th.no_grad()
    def _init_weights(self, weight_width) -> None:
        self.linear.weight.uniform_(-1, 1)
        self.linear.weight *= weight_width

    def reset_parameters(self) -> None:
        if self.first_layer:
            self._init_weights(1 / self.linear.in_features)
        else:
            self._init_weights(sqrt(6 / self.linear.in_features) / self.scale)

    def _get_plan(self) -> MLPPlan:
        if self._plan is None:
            k = self.linear.in_features
            self._plan = MLPPlan([LayerPlan(self.linear, [Source("pos", k, K.pad32(k))], False, sine=True)], [0])
        return self._plan

    def forward(self, x: th.Tensor) -> th.Tensor:
        k, n = self.linear.in_features, self.linear.out_features
        if x.dim() != 2 or x.shape[1] != k:
            raise ValueError(f"expected [batch, {k}] input, got {tuple(x.shape)}")
        K._require_cuda_f32("x", x)
        # the kernels read operand rows in 16-byte quads: [scale * x | 0 ...] of 4-column multiples
        xs = F.pad(self.scale * x, (0, -k % 4))
        plan = self._get_plan()
        (y,) = MLPFunction.apply(plan, x.shape[0], xs, None, 1, *plan.params())
        return y if y.shape[1] == n else y[:, :n]


class NerfModel(nn.Module):
    def __init__(self, input_scale: float):
        super().__init__()
        self.input_scale = input_scale
        self.hidden_dim = h = 256
        self.model_density_1 = nn.Sequential(
            LinearSine(3, h, scale=input_scale, first_layer=True),
            LinearSine(h, h),
            LinearSine(h, h),
            LinearSine(h, h),
        )
        self.model_density_2 = nn.Sequential(
            LinearSine(h + 3, h, scale=th.cat((th.ones(h), th.ones(3) * input_scale))),
            LinearSine(h, h),
            LinearSine(h, h),
            nn.Linear(h, h + 3 + 1),           # latent | base colour | density
        )
        self.softplus = nn.Softplus(threshold=8)
        self.model_color = nn.Sequential(
            LinearSine(h + 3, h, scale=th.cat((th.ones(h), th.ones(3) * input_scale))),
            nn.Linear(h, 3),
        )
        self.sigmoid = nn.Sigmoid()
        self._plan: MLPPlan | None = None

    def _check_scales(self) -> None:
        """The lowering scales pos / dir by input_scale and nothing else: the buffers must say so
        (they do unless a state dict of another input scale was loaded)."""
        h, s = self.hidden_dim, float(self.input_scale)
        for seq in (self.model_density_1, self.model_density_2, self.model_color):
            for m in seq:
                if not isinstance(m, LinearSine):
                    continue
                want = th.ones(m.linear.in_features)
                if m.linear.in_features != h:
                    want[-3:] = s
                if not th.equal(m.scale.detach().cpu(), want):
                    raise ValueError("NerfModel: LinearSine.scale buffers differ from (1 on hidden columns, "
                                     f"input_scale = {s} on pos / dir columns)")

    def _get_plan(self) -> MLPPlan:
        if self._plan is None:
            self._check_scales()
            h = self.hidden_dim
            layers: list[LayerPlan] = []
            pos = Source("pos", 3, K.pad32(3))

            def chain(seq, first_sources):
                srcs = first_sources
                for m in seq:
                    lin = m.linear if isinstance(m, LinearSine) else m
                    if srcs is None:
                        srcs = [Source("act", h, K.pad32(h), len(layers) - 1)]
                    layers.append(LayerPlan(lin, srcs, False, sine=isinstance(m, LinearSine)))
                    srcs = None
                return len(layers) - 1

            z1 = chain(self.model_density_1, [pos])
            z2 = chain(self.model_density_2, [Source("act", h, h, z1), pos])
            head = chain(self.model_color, [Source("act", h, h, z2), Source("dir", 3, K.pad32(3))])
            # base colour z2[:, 256:259] and density z2[:, 259] are read one column at a time: [M]
            # outputs, so nothing touches (or differentiates) the 260-wide buffer again
            self._plan = MLPPlan(layers, [head], [(z2, h), (z2, h + 1), (z2, h + 2), (z2, h + 3)])
        return self._plan

    def forward(self, pos: th.Tensor, dir: th.Tensor) -> tuple[th.Tensor, th.Tensor]:
        plan = self._get_plan()
        s = float(self.input_scale)
        head, r, g, b, sigma_raw = MLPFunction.apply(plan, pos.shape[0], _scale_pad4(pos, s), _scale_pad4(dir, s), 1,
                                                     *plan.params())
        density = F.softplus(sigma_raw - 1, beta=1, threshold=8)
        rgb = th.sigmoid(th.stack((r, g, b), dim=1) + head[:, :3])
        return density, rgb


class NerfSiren(CoarseFineRenderer):
    def __init__(self, near_sphere_normalized: float, far_sphere_normalized: float, samples_per_ray_fine: int,
                 samples_per_ray_coarse: int, learning_rate: float = 1e-4, learning_rate_decay: float = 0.5,
                 weight_decay: float = 0.0):
        super().__init__(near_sphere_normalized, far_sphere_normalized, samples_per_ray_fine,
                         samples_per_ray_coarse, learning_rate, learning_rate_decay, weight_decay)
        self.model_coarse = NerfModel(input_scale=32)
        self.model_fine = NerfModel(input_scale=32)

    def configure_optimizers(self):
        optimizer = self._adam()
        scheduler = th.optim.lr_scheduler.ExponentialLR(optimizer, gamma=self.learning_rate_decay)
        return {"optimizer": optimizer, "lr_scheduler": scheduler}
