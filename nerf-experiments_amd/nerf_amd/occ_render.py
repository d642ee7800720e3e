"""Training a field through the occupancy grid: the sample points of packed samples, the distortion
loss, and the renderer module that joins estimator, field, packed compositing and grid update.

nerfacc is not vendored and not installed; ``distortion`` restates its published behaviour with its
call signature (**parity unpinned**, like ``OccGridEstimator``), ``packed_points`` is the closure every
nerfacc example writes by hand (``rays_o[ray_indices] + rays_d[ray_indices] * t_mid[:, None]``) as one
autograd node, and ``OccGridRenderer`` is that example's render function as an ``nn.Module``.

  * ``packed_points``: nerf_packed_points_fwd / _bwd (csrc/packed_points.hip).  The points are bitwise
    the midpoints whose cells the marching tested (the points contract of include/nerf_amd.h), and
    the gradient to ``rays_o`` / ``rays_d`` (the pose gradient of BARF / GARF) is a fixed-order fp64
    segment sum, bitwise reproducible, where torch's ``index_add`` backward uses fp32 atomics.
  * ``distortion``: nerf_distortion_fwd / _bwd (csrc/distortion.hip), fp64 segmented prefix sums.
  * ``OccGridRenderer``: sampling -> points -> field -> ``rendering(..., ray_indices=...)``.
"""
from __future__ import annotations

from typing import Callable, Optional

import torch as th
from torch import nn

from . import kernels as K
from .prop_sampler import _segments, rendering


def _check_flat(pairs, n=None) -> int:
    """Shape / dtype checks that need no device: float32 flat tensors of one length."""
    for name, t in pairs:
        if not isinstance(t, th.Tensor) or t.dtype != th.float32:
            raise ValueError(f"{name} must be a float32 tensor")
        if t.dim() != 1:
            raise ValueError(f"{name} must be a flat [n_samples] tensor")
        n = t.shape[0] if n is None else n
        if t.shape[0] != n:
            raise ValueError(f"{name} must have one entry per sample ({n})")
    return n


def _check_ray_indices(ray_indices, n: int) -> None:
    if not isinstance(ray_indices, th.Tensor) or ray_indices.dtype != th.int64 or tuple(ray_indices.shape) != (n,):
        raise ValueError("ray_indices must be an int64 [n_samples] tensor")
    # Sorted ascending is the contract (nerfacc's too).  On the device it is not checked, that would
    # take a synchronisation; a host tensor is checked because there the check is free.
    if ray_indices.device.type == "cpu" and n > 1 and bool((ray_indices[1:] < ray_indices[:-1]).any()):
        raise ValueError("ray_indices must be sorted ascending (samples ray-major)")


class _PackedPointsFn(th.autograd.Function):
    """nerf_packed_points_fwd / _bwd: (positions, dirs or an empty tensor); one node carries the
    gradients of both to rays_o and rays_d.  Nothing flows to t_starts / t_ends."""

    @staticmethod
    def forward(ctx, rays_o, rays_d, ray_indices, t_starts, t_ends, want_dirs):
        rays_o, rays_d = rays_o.contiguous(), rays_d.contiguous()
        ray_indices, t_starts, t_ends = ray_indices.contiguous(), t_starts.contiguous(), t_ends.contiguous()
        pos, dirs = K.packed_points_fwd(rays_o, rays_d, ray_indices, t_starts, t_ends, want_dirs)
        ctx.n_rays = rays_o.shape[0]
        ctx.save_for_backward(ray_indices, t_starts, t_ends)
        if dirs is None:
            dirs = pos.new_zeros(0)
            ctx.mark_non_differentiable(dirs)
        return pos, dirs

    @staticmethod
    def backward(ctx, g_pos, g_dirs):
        ray_indices, t_starts, t_ends = ctx.saved_tensors
        n = t_starts.shape[0]
        g_pos = g_pos.contiguous() if g_pos is not None else t_starts.new_zeros(n, 3)
        if g_dirs is not None:
            g_dirs = g_dirs.contiguous() if g_dirs.numel() == 3 * n and n else None
        g_o, g_d = K.packed_points_bwd(_segments(ray_indices, ctx.n_rays), t_starts, t_ends, g_pos, g_dirs)
        return (g_o if ctx.needs_input_grad[0] else None, g_d if ctx.needs_input_grad[1] else None,
                None, None, None, None)


def packed_points(rays_o: th.Tensor, rays_d: th.Tensor, ray_indices: th.Tensor, t_starts: th.Tensor,
                  t_ends: th.Tensor, n_rays: Optional[int] = None, want_dirs: bool = True):
    """(positions [N, 3], dirs [N, 3] or None with ``want_dirs=False``) of packed samples:
    ``positions_i = rays_o[r] + ((t_starts_i + t_ends_i) * 0.5) * rays_d[r]``, ``dirs_i = rays_d[r]``,
    r = ray_indices[i], every operation rounded to fp32 on its own: bitwise the points whose cells
    ``OccGridEstimator.sampling`` tested.  ray_indices: int64, sorted ascending (needed by the
    backward only).  Differentiable in rays_o and rays_d, deterministically; not in t."""
    for name, t in (("rays_o", rays_o), ("rays_d", rays_d)):
        if not isinstance(t, th.Tensor) or t.dtype != th.float32 or t.dim() != 2 or t.shape[1] != 3:
            raise ValueError(f"{name} must be a float32 [n_rays, 3] tensor")
    if rays_o.shape != rays_d.shape:
        raise ValueError("rays_o and rays_d must share their shape")
    if n_rays is not None and int(n_rays) != rays_o.shape[0]:
        raise ValueError(f"n_rays = {n_rays} but rays_o holds {rays_o.shape[0]} rays")
    n = _check_flat((("t_starts", t_starts), ("t_ends", t_ends)))
    _check_ray_indices(ray_indices, n)
    pos, dirs = _PackedPointsFn.apply(rays_o, rays_d, ray_indices, t_starts, t_ends, bool(want_dirs))
    return pos, (dirs if want_dirs else None)


class _DistortionFn(th.autograd.Function):
    """nerf_distortion_fwd / _bwd on flat samples: loss [n_rays], differentiable in the weights."""

    @staticmethod
    def forward(ctx, weights, t_starts, t_ends, seg):
        weights, t_starts, t_ends = weights.contiguous(), t_starts.contiguous(), t_ends.contiguous()
        ctx.save_for_backward(weights, t_starts, t_ends, seg)
        return K.distortion_fwd(weights, t_starts, t_ends, seg)

    @staticmethod
    def backward(ctx, g_loss):
        weights, t_starts, t_ends, seg = ctx.saved_tensors
        return K.distortion_bwd(weights, t_starts, t_ends, seg, g_loss.contiguous()), None, None, None


def distortion(weights: th.Tensor, t_starts: th.Tensor, t_ends: th.Tensor, ray_indices: Optional[th.Tensor] = None,
               n_rays: Optional[int] = None) -> th.Tensor:
    """nerfacc.distortion: the distortion loss of mip-NeRF 360 per ray, [n_rays],
    ``sum_ij w_i w_j |m_i - m_j| + 1/3 sum_i w_i^2 (t_ends_i - t_starts_i)`` with the midpoints m
    ascending along each ray (the contract, not checked).  Packed samples: flat [N] tensors with
    ray_indices (int64, sorted ascending) and n_rays; batched [R, S] tensors with ray_indices=None run
    the same kernel on equal segments.  Differentiable in weights only."""
    if ray_indices is None:
        if not isinstance(weights, th.Tensor) or weights.dim() != 2:
            raise ValueError("without ray_indices, weights / t_starts / t_ends must be [n_rays, n_samples]")
        if t_starts.shape != weights.shape or t_ends.shape != weights.shape:
            raise ValueError("weights, t_starts and t_ends must share their shape")
        R, S = weights.shape
        if n_rays is not None and int(n_rays) != R:
            raise ValueError(f"n_rays = {n_rays} but weights holds {R} rays")
        flat = [x.reshape(-1) for x in (weights, t_starts, t_ends)]
        _check_flat(zip(("weights", "t_starts", "t_ends"), flat))
        seg = th.arange(R + 1, device=weights.device) * S
    else:
        n = _check_flat((("weights", weights), ("t_starts", t_starts), ("t_ends", t_ends)))
        _check_ray_indices(ray_indices, n)
        if n_rays is None:
            raise ValueError("n_rays is required with ray_indices (reading it off the device would synchronise)")
        flat = [weights, t_starts, t_ends]
        for name, t in zip(("weights", "t_starts", "t_ends"), flat):
            K._require_cuda_f32(name, t)
        seg = _segments(ray_indices, int(n_rays))
    return _DistortionFn.apply(*flat, seg)


class OccGridRenderer(nn.Module):
    """Renders and trains any ``radiance(pos [N, 3], dir [N, 3]) -> (rgb [N, 3], density [N] or [N, 1])``
    (the convention of the GARF / GaborF / SARF ``RadianceNetwork``) through an ``OccGridEstimator``, or,
    for unbounded scenes, a ``CascadedOccGridEstimator`` with ``cone_angle > 0`` (nerfacc's examples use
    0.004 with four levels).

    ``forward(rays_o, rays_d, stratified=None)`` -> (rgb [R, 3], opacity [R, 1], depth [R, 1], extras):
    ``estimator.sampling`` (with the visibility filter, a no_grad density pass at the packed points,
    only when ``alpha_thre > 0`` or ``early_stop_eps > 0``), then ``packed_points``, the field, and
    ``rendering(..., ray_indices=..., n_rays=R)``.  ``stratified`` defaults to ``self.training``.
    ``extras`` is ``rendering``'s plus ``ray_indices``, ``t_starts``, ``t_ends``.  Host synchronisations:
    those of ``sampling`` (one for the sample total, one more with the visibility filter), no others.
    A batch in which no sample is kept does not call the field: it returns zeros (plus the background)
    that carry **no graph**, so a training loop must not call ``backward`` on such a batch alone
    (``rgb.requires_grad`` tells).  Gradients reach the field's parameters and, where they require
    grad, ``rays_o`` / ``rays_d``; none reaches the sample positions along the ray."""

    def __init__(self, radiance: Callable, estimator: nn.Module, near_plane: float, far_plane: float,
                 render_step_size: float, alpha_thre: float = 0.0, early_stop_eps: float = 1e-4,
                 render_bkgd: Optional[th.Tensor] = None, density_fn: Optional[Callable] = None,
                 cone_angle: float = 0.0):
        super().__init__()
        self.radiance = radiance
        self.estimator = estimator
        self.near_plane, self.far_plane = float(near_plane), float(far_plane)
        self.render_step_size = float(render_step_size)
        self.alpha_thre, self.early_stop_eps = float(alpha_thre), float(early_stop_eps)
        self.register_buffer("render_bkgd", None if render_bkgd is None
                             else th.as_tensor(render_bkgd, dtype=th.float32).clone())
        self.density_fn = density_fn
        self.cone_angle = float(cone_angle)
        self._n_rays = None

    def _density(self, pos: th.Tensor, dirs: Optional[th.Tensor] = None) -> th.Tensor:
        """Density at points: density_fn if given, else the field's at the given directions (one fixed
        unit direction without them)."""
        if self.density_fn is not None:
            return self.density_fn(pos).reshape(-1)
        if dirs is None:
            dirs = pos.new_tensor([0.0, 0.0, 1.0]).expand(pos.shape[0], 3).contiguous()
        return self.radiance(pos, dirs)[1].reshape(-1)

    def forward(self, rays_o: th.Tensor, rays_d: th.Tensor, stratified: Optional[bool] = None):
        if stratified is None:
            stratified = self.training
        R = rays_o.shape[0]
        self._n_rays = R
        o_s, d_s = rays_o.detach().contiguous(), rays_d.detach().contiguous()
        sigma_fn = None
        if self.alpha_thre > 0 or self.early_stop_eps > 0:
            def sigma_fn(ts, te, idx):                   # called under sampling's no_grad
                pos, dirs = packed_points(o_s, d_s, idx, ts, te, R, want_dirs=self.density_fn is None)
                return self._density(pos, dirs)
        # cone_angle is passed only when set: a one-level estimator is called exactly as before
        cone = {"cone_angle": self.cone_angle} if self.cone_angle != 0.0 else {}
        ray_indices, t_starts, t_ends = self.estimator.sampling(
            o_s, d_s, sigma_fn=sigma_fn, near_plane=self.near_plane, far_plane=self.far_plane,
            render_step_size=self.render_step_size, early_stop_eps=self.early_stop_eps, alpha_thre=self.alpha_thre,
            stratified=bool(stratified), **cone)
        where = {"ray_indices": ray_indices, "t_starts": t_starts, "t_ends": t_ends}
        if ray_indices.numel() == 0:                    # a shape: known on the host since sampling
            f = dict(device=rays_o.device, dtype=th.float32)
            rgb = th.zeros(R, 3, **f)
            if self.render_bkgd is not None:
                rgb = rgb + self.render_bkgd
            e = th.zeros(0, **f)
            return rgb, th.zeros(R, 1, **f), th.zeros(R, 1, **f), {
                "weights": e, "trans": e, "sigmas": e, "rgbs": th.zeros(0, 3, **f), "alphas": e, **where}

        def rgb_sigma_fn(ts, te, idx):
            pos, dirs = packed_points(rays_o, rays_d, idx, ts, te, R)
            rgb, sigma = self.radiance(pos, dirs)
            return rgb, sigma.reshape(-1)
        rgb, opacity, depth, extras = rendering(t_starts, t_ends, ray_indices, R, rgb_sigma_fn, self.render_bkgd)
        extras.update(where)
        return rgb, opacity, depth, extras

    def distortion_loss(self, extras: dict, n_rays: Optional[int] = None) -> th.Tensor:
        """Mean over the rays of ``distortion(weights, t_starts, t_ends, ray_indices)`` of a forward's
        extras; n_rays defaults to the ray count of the last ``forward``."""
        n_rays = self._n_rays if n_rays is None else int(n_rays)
        if n_rays is None:
            raise ValueError("distortion_loss needs n_rays before the first forward")
        if n_rays == 0:
            return extras["weights"].new_zeros(())
        return distortion(extras["weights"], extras["t_starts"], extras["t_ends"], extras["ray_indices"],
                          n_rays).mean()

    def update_grid(self, step: int, **kw) -> None:
        """``estimator.update_every_n_steps(step, occ_eval_fn, **kw)`` with
        ``occ_eval_fn(x) = density(x) * render_step_size``: density_fn if given, else the field's density
        at the fixed unit direction (0, 0, 1)."""
        self.estimator.update_every_n_steps(step, lambda x: self._density(x) * self.render_step_size, **kw)


__all__ = ["OccGridRenderer", "distortion", "packed_points"]
