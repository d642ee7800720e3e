"""What the GARF, GaborF and SARF field MLPs share (garf/, gaborf/, sarf/ of the reference: one
RadianceNetwork / ProposalNetwork topology, three learnable per-channel activations).

``RadianceField`` / ``ProposalField`` build the reference's submodules in its construction order
(so ``th.manual_seed`` gives its initial parameters and state_dicts interchange), lower them to one
``MLPPlan`` and run them as ONE ``MLPFunction`` autograd node: every Linear on the MFMA linear
kernels, each activation in the GEMM epilogue or its own pass, RadianceNetwork's
``z1[:, :128] + z2[:, :128]`` folded into the accumulate epilogue of the last density layer, the
concatenations ``[z1 | pos]`` / ``[z1 + z2 | dir]`` read as multi-segment GEMM operands.  Only the
final softplus / sigmoid heads are torch ops.  A family (model_garf.py, model_gaborf.py,
model_sarf.py) supplies ``_make_act`` / ``_act_params`` / ``_lower``.
"""
from __future__ import annotations

from typing import Iterator

import torch as th
import torch.nn as nn
import torch.nn.functional as F

from . import kernels as K
from .mlp import LayerPlan, MLPFunction, MLPPlan, Source
from .model_interpolation_architecture import NerfBaseModel


class _Pad4Fn(th.autograd.Function):
    """[M,3] -> [M,4] (zero 4th column) with nerf_encode_fwd's identity encoding: the
    MFMA linear kernels read operand rows in 16-byte quads."""

    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        params = K.make_pe_params(0, 0, True, 1.0)
        return K.encode_fwd(params, 3, x=x, n_samples=x.shape[0], n_rays=x.shape[0], out_ld=4, device=x.device)

    @staticmethod
    def backward(ctx, g):
        return g[:, :3]


def _pad4(x: th.Tensor) -> th.Tensor:
    if x.dim() != 2 or x.shape[1] != 3:
        raise ValueError(f"expected [batch, 3] input, got {tuple(x.shape)}")
    K._require_cuda_f32("input", x)
    return _Pad4Fn.apply(x)


def strip_compile_prefix(state_dict: dict) -> dict:
    """State dict of the reference's ``th.compile``-wrapped networks -> this package's key names."""
    return {k.replace("._orig_mod", ""): v for k, v in state_dict.items()}


class ParamActFn(th.autograd.Function):
    """A Gabor / Sarf activation module used on its own (nerf_param_act_fwd / _bwd)."""

    @staticmethod
    def forward(ctx, kind, x, *params):
        K._require_cuda_f32("x", x)
        if x.dim() != 2 or x.shape[1] != params[0].shape[0]:
            raise ValueError(f"expected [batch, {params[0].shape[0]}] input, got {tuple(x.shape)}")
        if x.stride(1) != 1:
            x = x.contiguous()
        y = th.empty(x.shape, device=x.device, dtype=th.float32)
        K.param_act_fwd(kind, x, x.shape[1], params, y)
        ctx.kind = kind
        ctx.save_for_backward(x, *params)
        return y

    @staticmethod
    def backward(ctx, g):
        x, *params = ctx.saved_tensors
        g = g.contiguous()
        dx = th.empty_like(x)
        grads = [th.empty_like(p) for p in params]
        K.param_act_bwd(ctx.kind, g, x, x.shape[1], params, dx, grads)
        return (None, dx, *grads)


class FieldBase(NerfBaseModel):
    def __init__(self):
        super().__init__()
        self._parameters_linear: list[nn.Parameter] = []
        self._parameters_act: list[nn.Parameter] = []
        self._plan: MLPPlan | None = None

    # ---- supplied by the family
    def _make_act(self, features_in: int) -> nn.Module:
        raise NotImplementedError

    @staticmethod
    def _act_params(act: nn.Module) -> tuple[nn.Parameter, ...]:
        """The activation's parameters in state-dict order."""
        raise NotImplementedError

    @classmethod
    def _lower(cls, act: nn.Module) -> dict:
        """LayerPlan keyword arguments of a layer followed by ``act``."""
        raise NotImplementedError

    # ---- construction
    def _create_linear(self, features_in: int, features_out: int) -> nn.Linear:
        linear = nn.Linear(features_in, features_out)
        self._parameters_linear.append(linear.weight)
        self._parameters_linear.append(linear.bias)
        return linear

    def _create_act(self, features_in: int) -> nn.Module:
        act = self._make_act(features_in)
        self._parameters_act.extend(self._act_params(act))
        return act

    def parameters_linear(self) -> Iterator[nn.Parameter]:
        return iter(self._parameters_linear)

    def _maybe_param_groups(self, learning_rate_start, learning_rate_stop, learning_rate_decay_end,
                            act_learning_rate_factor, weight_decay):
        if learning_rate_start is None:
            return
        self._add_param_group(self.parameters_linear(), learning_rate_start, learning_rate_stop,
                              learning_rate_decay_end, weight_decay)
        self._add_param_group(iter(self._parameters_act), learning_rate_start * act_learning_rate_factor,
                              learning_rate_stop * act_learning_rate_factor, learning_rate_decay_end,
                              weight_decay)

    # ---- lowering
    def _chain(self, seq: nn.Sequential, first_sources: list[Source], layers: list[LayerPlan]) -> int:
        """Lower Linear/activation pairs of ``seq`` (a trailing Linear without activation allowed);
        returns the index of the last layer."""
        mods = list(seq)
        i = 0
        srcs = first_sources
        while i < len(mods):
            lin = mods[i]
            if not isinstance(lin, nn.Linear):
                break
            act = mods[i + 1] if i + 1 < len(mods) and isinstance(mods[i + 1], self._act_type) else None
            if srcs is None:
                prev = layers[-1].module.out_features
                srcs = [Source("act", prev, K.pad32(prev), len(layers) - 1)]
            layers.append(LayerPlan(lin, srcs, False, **(self._lower(act) if act is not None else {})))
            srcs = None
            i += 2 if act is not None else 1
        return len(layers) - 1


class RadianceField(FieldBase):
    """garf/model_radiance.py:9-96 = gaborf/model_radiance.py:9-91 = sarf/model_radiance.py:9-96."""

    def _build(self):
        self.model_density_1 = nn.Sequential(
            self._create_linear(3, 1024), self._create_act(1024),
            self._create_linear(1024, 256), self._create_act(256),
            self._create_linear(256, 128), self._create_act(128),
            self._create_linear(128, 128), self._create_act(128),
        )
        self.model_density_2 = nn.Sequential(
            self._create_linear(128 + 3, 512), self._create_act(512),
            self._create_linear(512, 256), self._create_act(256),
            self._create_linear(256, 128), self._create_act(128),
            self._create_linear(128, 128 + 1),
        )
        self.softplus = nn.Softplus(threshold=8)
        self.model_color = nn.Sequential(
            self._create_linear(128 + 3, 256), self._create_act(256),
            self._create_linear(256, 3), nn.Sigmoid(),
        )

    def _get_plan(self) -> MLPPlan:
        if self._plan is None:
            layers: list[LayerPlan] = []
            pos = Source("pos", 3, K.pad32(3))
            z1 = self._chain(self.model_density_1, [pos], layers)
            z2 = self._chain(self.model_density_2, [Source("act", 128, 128, z1), pos], layers)
            # z2 output holds [z1[:, :128] + z2[:, :128] | z2[:, 128]] (model_radiance.py:89,92)
            layers[z2].residual, layers[z2].residual_cols = z1, 128
            head = self._chain(self.model_color, [Source("act", 128, 128, z2), Source("dir", 3, K.pad32(3))],
                               layers)
            # sigma = softplus(z2[:, 128] - 1) reads one column: exposed as its own [M] output
            self._plan = MLPPlan(layers, [z2, head], [(z2, 128)])
        return self._plan

    def forward(self, pos: th.Tensor, dir: th.Tensor) -> tuple[th.Tensor, th.Tensor]:
        plan = self._get_plan()
        _, head, sigma_raw = MLPFunction.apply(plan, pos.shape[0], _pad4(pos), _pad4(dir), 1, *plan.params())
        density = F.softplus(sigma_raw - 1, beta=1, threshold=8)
        rgb = th.sigmoid(head[:, :3])
        return rgb, density


class ProposalField(FieldBase):
    """garf/model_proposal.py:9-56 = gaborf/model_proposal.py:9-56 = sarf/model_proposal.py:9-56."""

    def _build(self):
        self.model = nn.Sequential(
            self._create_linear(3, 512), self._create_act(512),
            self._create_linear(512, 256), self._create_act(256),
            self._create_linear(256, 128), self._create_act(128),
            self._create_linear(128, 1), nn.Softplus(threshold=8),
        )

    def _get_plan(self) -> MLPPlan:
        if self._plan is None:
            layers: list[LayerPlan] = []
            out = self._chain(self.model, [Source("pos", 3, K.pad32(3))], layers)
            self._plan = MLPPlan(layers, [out])
        return self._plan

    def forward(self, pos: th.Tensor) -> th.Tensor:
        plan = self._get_plan()
        (y,) = MLPFunction.apply(plan, pos.shape[0], _pad4(pos), None, 1, *plan.params())
        return F.softplus(y[:, :1], beta=1, threshold=8)
