"""The Instant-NGP radiance field for the occupancy-grid path, on gfx950 kernels.

nerfacc's examples train ``NGPRadianceField`` through ``OccGridEstimator``; this module restates that
field with nerfacc's constructor names and defaults.  Neither nerfacc nor tiny-cuda-nn is vendored or
installed, so everything here follows their published behaviour and is **parity unpinned**, like the
estimators.  Differences that are deliberate:

* the hash grid is the project's own (``model_ingp.INGPEncoding``: its corner order, hash, bijective
  coarse levels and resolutions ``floor(base * b^l)``), not tiny-cuda-nn's indexing and offsets;
* the layers are ``nn.Linear`` **with bias** (tiny-cuda-nn's fully fused MLP has none);
* directions are used as given, the caller normalises: tiny-cuda-nn's ``(d + 1) / 2`` and ``2u - 1``
  round trip is not made.

Parts:

* ``SHEncoding(degree=4)`` — the real spherical harmonics of degree <= 4 in tiny-cuda-nn's order and
  sign, ``output_dim = degree^2``; one autograd node over nerf_sh_encode_fwd / _bwd.  ``forward`` and
  ``encode_padded`` return rows of ``pad32(output_dim)`` columns, the pad columns zero: the buffer
  the colour head's first layer reads.
* ``contract_to_unisphere(x, aabb)`` / ``normalize_to_aabb(x, aabb)`` -> ``(u, inside)``: scene
  coordinates to the hash grid's unit cube (nerfacc's inf-norm contraction, or the plain box map) and
  the fp32 0 / 1 selector of points strictly inside it; one autograd node over nerf_unit_cube_fwd /
  _bwd.  ``inside`` carries no gradient.
* ``UnitCubeHashEncoding`` — ``model_ingp.INGPEncoding`` on points already in the unit cube (that
  class hard-codes its scene's ``x / 8 + 0.5``); resolutions, packed table, deterministic table
  gradient and position gradient are inherited.
* ``trunc_exp`` — ``exp(x)`` whose backward is ``g * exp(clamp(x, max=15))``.
* ``NGPRadianceField`` — position map -> hash grid (F = 2) -> Linear(32 -> 64), ReLU,
  Linear(64 -> 1 + geo_feat_dim); ``density = trunc_exp(z[:, 0] - 1) * inside``; colour:
  ``[SH(dir) | z[:, 1:]]`` -> Linear -> 64, ReLU, Linear -> 64, ReLU, Linear -> 3, sigmoid.  The
  layers run as one ``MLPFunction`` node on the fp32 / split-precision GEMM kernels; ``z[:, 1:]``
  feeds the head through a column map, so nothing is sliced into a new buffer.  ``query_density``
  runs a plan of the two density layers alone.  ``forward(positions, directions) -> (rgb [N, 3],
  density [N, 1])`` is the convention ``OccGridRenderer`` takes.
"""
from __future__ import annotations

import torch as th
import torch.nn as nn

from . import kernels as K
from .mlp import LayerPlan, MLPFunction, MLPPlan, Source
from .model_ingp import INGPEncoding


def _points(name: str, x: th.Tensor) -> th.Tensor:
    if not isinstance(x, th.Tensor) or x.dim() != 2 or x.shape[1] != 3:
        raise ValueError(f"{name} must be [N, 3] (got {tuple(getattr(x, 'shape', ()))})")
    K._require_cuda_f32(name, x)
    return x.contiguous()


def _box(aabb) -> tuple[float, ...]:
    """The six floats of a box on the host (a device tensor is read back: a synchronisation; modules
    convert theirs once at construction)."""
    vals = [float(v) for v in (aabb.detach().reshape(-1).tolist() if isinstance(aabb, th.Tensor) else aabb)]
    if len(vals) != 6:
        raise ValueError("aabb must hold six values (lo_0, lo_1, lo_2, hi_0, hi_1, hi_2)")
    if any(not hi > lo for lo, hi in zip(vals[:3], vals[3:])):
        raise ValueError(f"aabb must have hi > lo on every axis (got {vals})")
    return tuple(vals)


# ----------------------------------------------------------------------------- SH direction encoding
class _SHFn(th.autograd.Function):
    @staticmethod
    def forward(ctx, dirs, degree, cols):
        used = degree * degree
        out = th.empty(dirs.shape[0], cols, device=dirs.device, dtype=th.float32)
        if cols > used:
            out[:, used:].zero_()
        if dirs.shape[0]:
            K.sh_encode_fwd(dirs, degree, out)
        ctx.degree = degree
        ctx.save_for_backward(dirs)
        return out

    @staticmethod
    def backward(ctx, g):
        (dirs,) = ctx.saved_tensors
        if g is None or not ctx.needs_input_grad[0]:
            return None, None, None
        if dirs.shape[0] == 0:
            return th.zeros_like(dirs), None, None
        return K.sh_encode_bwd(dirs, ctx.degree, g.contiguous()), None, None


class SHEncoding(nn.Module):
    def __init__(self, degree: int = 4):
        super().__init__()
        if not 1 <= int(degree) <= 4:
            raise ValueError(f"degree must be in 1..4 (got {degree})")
        self.degree = int(degree)
        self.output_dim = self.degree ** 2

    @property
    def padded_dim(self) -> int:
        return K.pad32(self.output_dim)

    def encode_padded(self, dir: th.Tensor) -> th.Tensor:
        """[N, pad32(output_dim)] basis values of dir [N, 3] (used as given), pad columns zero."""
        return _SHFn.apply(_points("dir", dir), self.degree, self.padded_dim)

    def forward(self, dir: th.Tensor) -> th.Tensor:
        return self.encode_padded(dir)


# ----------------------------------------------------------------------------- position map
class _UnitCubeFn(th.autograd.Function):
    @staticmethod
    def forward(ctx, x, box, mode):
        u, inside = K.unit_cube_fwd(x, box, mode)
        ctx.box, ctx.mode = box, mode
        ctx.save_for_backward(x)
        ctx.mark_non_differentiable(inside)
        return u, inside

    @staticmethod
    def backward(ctx, g_u, _g_inside):
        (x,) = ctx.saved_tensors
        if g_u is None or not ctx.needs_input_grad[0]:
            return None, None, None
        return K.unit_cube_bwd(x, ctx.box, ctx.mode, g_u.contiguous()), None, None


def normalize_to_aabb(x: th.Tensor, aabb):
    """(u [N, 3], inside [N]): ``u = (x - lo) / (hi - lo)``; inside = 1.0 where 0 < u < 1 on every axis."""
    return _UnitCubeFn.apply(_points("x", x), _box(aabb), 0)


def contract_to_unisphere(x: th.Tensor, aabb):
    """(u [N, 3], inside [N]): nerfacc's ``contract_to_unisphere`` with the inf-norm.  The box maps to
    [0.25, 0.75]^3 and everything outside it into the rest of the unit cube (``c = 2 v - 1``;
    ``c (2 - 1/m) / m`` where ``m = max |c| > 1``; ``u = c / 4 + 0.5``)."""
    return _UnitCubeFn.apply(_points("x", x), _box(aabb), 1)


# ----------------------------------------------------------------------------- hash grid on the unit cube
class UnitCubeHashEncoding(INGPEncoding):
    """``INGPEncoding`` whose input already lies in the unit cube: no ``x / 8 + 0.5``."""

    def _params(self, query: int = 1):
        return K.make_hashgrid_params(self.n_levels, self.table_size, self.n_features, self.resolutions, query,
                                      primes=(self.pi1, self.pi2, self.pi3), normalize=False)


# ----------------------------------------------------------------------------- density activation
class _TruncExp(th.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return th.exp(x)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return g * th.exp(x.clamp(max=15))


def trunc_exp(x: th.Tensor) -> th.Tensor:
    """``exp(x)`` with the backward ``g * exp(clamp(x, max=15))`` (instant-ngp's density activation)."""
    return _TruncExp.apply(x)


# ----------------------------------------------------------------------------- the field
class NGPRadianceField(nn.Module):
    HIDDEN = 64

    def __init__(self, aabb, num_dim: int = 3, use_viewdirs: bool = True, unbounded: bool = False,
                 base_resolution: int = 16, max_resolution: int = 4096, geo_feat_dim: int = 15, n_levels: int = 16,
                 log2_hashmap_size: int = 19):
        super().__init__()
        if num_dim != 3:
            raise ValueError("NGPRadianceField: the hash grid and the position map are 3-D (num_dim must be 3)")
        if geo_feat_dim < 1 or (1 + geo_feat_dim) % 4:
            raise ValueError("NGPRadianceField: 1 + geo_feat_dim must be a positive multiple of 4 (the GEMM kernels' "
                             f"row width; got geo_feat_dim = {geo_feat_dim})")
        box = _box(aabb)
        self.register_buffer("aabb", th.tensor(box, dtype=th.float32))
        self._box = box
        self.num_dim = num_dim
        self.use_viewdirs = bool(use_viewdirs)
        self.unbounded = bool(unbounded)
        self.base_resolution = base_resolution
        self.max_resolution = max_resolution
        self.geo_feat_dim = geo_feat_dim
        self.n_levels = n_levels
        self.log2_hashmap_size = log2_hashmap_size
        self.position_encoding = UnitCubeHashEncoding(max_resolution, base_resolution, 2 ** log2_hashmap_size, 2, n_levels)
        self.direction_encoding = SHEncoding(4) if self.use_viewdirs else None
        h = self.HIDDEN
        self.mlp_base = nn.Sequential(nn.Linear(self.position_encoding.output_dim, h), nn.ReLU(inplace=True),
                                      nn.Linear(h, 1 + geo_feat_dim))
        head_in = (self.direction_encoding.output_dim if self.use_viewdirs else 0) + geo_feat_dim
        self.mlp_head = nn.Sequential(nn.Linear(head_in, h), nn.ReLU(inplace=True), nn.Linear(h, h),
                                      nn.ReLU(inplace=True), nn.Linear(h, 3))
        self._density_plan: MLPPlan | None = None
        self._plan: MLPPlan | None = None

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)
        self._box = _box(self.aabb)          # the kernels take the box from the host: follow a loaded one

    # -- plans ----------------------------------------------------------------------------------
    def _base_layers(self) -> list[LayerPlan]:
        d, h = self.position_encoding.output_dim, self.HIDDEN
        return [LayerPlan(self.mlp_base[0], [Source("pos", d, K.pad32(d))], True),
                LayerPlan(self.mlp_base[2], [Source("act", h, K.pad32(h), 0)], False)]

    def density_plan(self) -> MLPPlan:
        """The two density layers alone; its one output is the raw density column z[:, 0]."""
        if self._density_plan is None:
            self._density_plan = MLPPlan(self._base_layers(), [], [(1, 0)])
        return self._density_plan

    def plan(self) -> MLPPlan:
        """Density layers and colour head; outputs: the head [N, 4] and the raw density column."""
        if self._plan is None:
            h, w = self.HIDDEN, 1 + self.geo_feat_dim
            # z[:, 1:] of the density layers' output feeds the head's inputs after the direction's;
            # z[:, 0], the raw density, has no weight there
            geo = Source("act", w, K.pad32(w), 1, cols=[-1] + list(range(self.geo_feat_dim)))
            srcs = [geo]
            if self.use_viewdirs:
                sh = self.direction_encoding.output_dim
                srcs = [Source("dir", sh, K.pad32(sh)), geo]
            layers = self._base_layers() + [
                LayerPlan(self.mlp_head[0], srcs, True),
                LayerPlan(self.mlp_head[2], [Source("act", h, K.pad32(h), 2)], True),
                LayerPlan(self.mlp_head[4], [Source("act", h, K.pad32(h), 3)], False)]
            self._plan = MLPPlan(layers, [4], [(1, 0)])
        return self._plan

    # -- evaluation -----------------------------------------------------------------------------
    def _features(self, positions: th.Tensor):
        x = _points("positions", positions)
        u, inside = _UnitCubeFn.apply(x, self._box, 1 if self.unbounded else 0)
        return self.position_encoding.encode_padded(u), inside

    def _density(self, raw: th.Tensor, inside: th.Tensor) -> th.Tensor:
        return (trunc_exp(raw - 1.0) * inside).view(-1, 1)

    def query_density(self, x: th.Tensor) -> th.Tensor:
        """Density [N, 1] at x [N, 3]; the colour layers are not run."""
        if x.shape[0] == 0:
            return _points("positions", x).new_zeros(0, 1)
        feat, inside = self._features(x)
        plan = self.density_plan()
        (raw,) = MLPFunction.apply(plan, x.shape[0], feat, None, 1, *plan.params())
        return self._density(raw, inside)

    def forward(self, positions: th.Tensor, directions: th.Tensor | None = None):
        """(rgb [N, 3], density [N, 1]) at positions [N, 3] seen along unit directions [N, 3]."""
        if self.use_viewdirs:
            if directions is None:
                raise ValueError("NGPRadianceField(use_viewdirs=True) needs directions")
            directions = _points("directions", directions)
            if directions.shape[0] != positions.shape[0]:
                raise ValueError("positions and directions must share their row count")
        n = positions.shape[0]
        if n == 0:
            e = _points("positions", positions)
            return e.new_zeros(0, 3), e.new_zeros(0, 1)
        feat, inside = self._features(positions)
        sh = self.direction_encoding.encode_padded(directions) if self.use_viewdirs else None
        plan = self.plan()
        head, raw = MLPFunction.apply(plan, n, feat, sh, 1, *plan.params())
        return th.sigmoid(head[:, :3]), self._density(raw, inside)


__all__ = ["NGPRadianceField", "SHEncoding", "UnitCubeHashEncoding", "contract_to_unisphere", "normalize_to_aabb",
           "trunc_exp"]
