"""nerfacc's occupancy-grid estimator (one level) on the device: empty-space skipping in front of
the packed renderer (``nerf_amd.prop_sampler.rendering(..., ray_indices=...)``).

nerfacc is an external CUDA package, not vendored in the reference and not installed here; this
module restates its published behaviour (``OccGridEstimator.sampling`` / ``update_every_n_steps``)
with the same call signatures and a marching contract of our own (include/nerf_amd.h), and its
numerics are **parity unpinned**, like ``PropNetEstimator``'s.

  * ``sampling`` marches every ray through the grid's box on a fixed-step lattice and keeps the
    steps whose midpoint lies in an occupied cell: nerf_occ_march_count / nerf_occ_march_write
    (csrc/occgrid.hip), two passes around one ``torch.cumsum``.  The sample total is read back once
    to allocate the outputs: **one host synchronisation per call**.  With ``sigma_fn`` / ``alpha_fn``
    the marched samples are then filtered by opacity and transmittance
    (nerf_composite_packed_fwd); that compaction is a boolean index, a second synchronisation.
  * ``update_every_n_steps`` is nerfacc's schedule in plain torch ops (not a hot path).
  * ``CascadedOccGridEstimator`` is nerfacc's ``OccGridEstimator(levels=L)`` for unbounded scenes:
    several levels, ``cone_angle`` and per-ray ``t_min`` / ``t_max`` through the cascaded marching
    contract (nerf_occ_cascade_count / nerf_occ_cascade_write, csrc/occgrid_cascade.hip).  A class of
    its own: ``OccGridEstimator`` keeps its one level, its kernels and its refusals.
Out of scope: ``mark_invisible_cells``.
"""
from __future__ import annotations

from typing import Callable, Optional, Sequence, Union

import torch as th
from torch import nn

from . import kernels as K
from .model_interpolation import _rng_seed


def pack_grid_bits(binaries: th.Tensor) -> th.Tensor:
    """Bool cells (any shape, flattened x-major) -> int32 words, bit (i & 31) of word i >> 5 = cell i."""
    flat = binaries.reshape(-1)
    pad = (-flat.numel()) % 32
    if pad:
        flat = th.cat([flat, flat.new_zeros(pad)])
    v = (flat.view(-1, 32).to(th.int64) << th.arange(32, device=flat.device)).sum(dim=1)
    return th.where(v >= 2 ** 31, v - 2 ** 32, v).to(th.int32)


class OccGridEstimator(nn.Module):
    """nerfacc.OccGridEstimator(roi_aabb, resolution=128, levels=1) restated.  Buffers (in
    ``state_dict``): ``occs`` fp32 [cells], ``binaries`` bool [1, rx, ry, rz] (x-major).  The kernel
    reads a bit-packed copy of ``binaries`` that is rebuilt whenever the buffer was written or
    replaced (an update, ``load_state_dict``, ``.to()``)."""

    def __init__(self, roi_aabb: Sequence[float], resolution: Union[int, Sequence[int]] = 128, levels: int = 1):
        super().__init__()
        if levels != 1:
            raise NotImplementedError("nerf_amd.occ_grid.OccGridEstimator supports levels=1")
        aabb = [float(v) for v in (roi_aabb.tolist() if isinstance(roi_aabb, th.Tensor) else roi_aabb)]
        if len(aabb) != 6 or not all(lo < hi for lo, hi in zip(aabb[:3], aabb[3:])):
            raise ValueError("roi_aabb must be [xmin, ymin, zmin, xmax, ymax, zmax] with min < max")
        res = [int(resolution)] * 3 if isinstance(resolution, int) else [int(r) for r in resolution]
        if len(res) != 3 or min(res) < 1:
            raise ValueError("resolution must be a positive int or three of them")
        self.aabb = tuple(aabb)
        self.resolution = tuple(res)
        self.cells = res[0] * res[1] * res[2]
        self.register_buffer("occs", th.zeros(self.cells))
        self.register_buffer("binaries", th.zeros([1] + res, dtype=th.bool))
        self._bits = None
        self._bits_src = None       # (the binaries tensor the bits were packed from, its version)
        self._status = None

    # -- the kernel's view of the grid ----------------------------------------------------------
    def grid_bits(self) -> th.Tensor:
        """The bit-packed ``binaries`` (int32 words); rebuilt when the buffer is another tensor than
        the one packed last (``.to()``, an assignment) or was written since (its version counter:
        ``load_state_dict``, an update).  No synchronisation."""
        b = self.binaries
        src = self._bits_src
        if src is None or src[0] is not b or src[1] != b._version:
            self._bits = pack_grid_bits(b)
            self._bits_src = (b, b._version)
        return self._bits

    def status(self) -> th.Tensor:
        """Device int32 word the marching ORs into: bit 0 a ray was cut at NERF_OCC_MAX_STEPS, bit 1
        at the mask capacity (never, by construction of the capacity).  Cleared by the caller."""
        dev = self.binaries.device
        if self._status is None or self._status.device != dev:
            self._status = th.zeros(1, device=dev, dtype=th.int32)
        return self._status

    # -- sampling -------------------------------------------------------------------------------
    @th.no_grad()
    def _march(self, rays_o: th.Tensor, rays_d: th.Tensor, near_plane: float, far_plane: float,
               render_step_size: float, stratified: bool):
        """The marching alone: (ray_indices, t_starts, t_ends) of every lattice step in an occupied cell."""
        if self.binaries.device.type != "cuda":
            raise RuntimeError("OccGridEstimator.sampling needs the estimator on a ROCm device; there is no CPU path")
        rays_o, rays_d = rays_o.contiguous(), rays_d.contiguous()
        n_rays = rays_o.shape[0]
        dev = rays_o.device
        seed = _rng_seed() if stratified else 0
        words = K.occ_mask_words(near_plane, far_plane, render_step_size)
        ws = th.empty(K.occ_march_workspace_bytes(n_rays, words), device=dev, dtype=th.uint8)
        counts = K.occ_march_count(rays_o, rays_d, self.aabb, self.resolution, self.grid_bits(), near_plane,
                                   far_plane, render_step_size, stratified, seed, words, ws, self.status())
        offsets = th.cumsum(counts, dim=0)
        total = int(offsets[-1].item()) if n_rays else 0      # the one host synchronisation
        return K.occ_march_write(n_rays, render_step_size, words, ws, offsets, total)

    @th.no_grad()
    def sampling(self, rays_o: th.Tensor, rays_d: th.Tensor, sigma_fn: Optional[Callable] = None,
                 alpha_fn: Optional[Callable] = None, near_plane: float = 0.0, far_plane: float = 1e10,
                 render_step_size: float = 1e-3, early_stop_eps: float = 1e-4, alpha_thre: float = 0.0,
                 stratified: bool = False, cone_angle: float = 0.0):
        """(ray_indices int64 [N], t_starts fp32 [N], t_ends fp32 [N]), ray-major and ascending along
        each ray.  ``sigma_fn(t_starts, t_ends, ray_indices)`` -> densities [N] (or ``alpha_fn`` ->
        opacities [N]) drops the samples with alpha < alpha_thre or transmittance < early_stop_eps."""
        if cone_angle != 0.0:
            raise NotImplementedError("nerf_amd.occ_grid.OccGridEstimator.sampling supports cone_angle=0")
        if sigma_fn is not None and alpha_fn is not None:
            raise ValueError("give sigma_fn or alpha_fn, not both")
        marched = self._march(rays_o, rays_d, near_plane, far_plane, render_step_size, stratified)
        return self._visible(*marched, rays_o.shape[0], sigma_fn, alpha_fn, early_stop_eps, alpha_thre)

    @staticmethod
    def _visible(ray_indices: th.Tensor, t_starts: th.Tensor, t_ends: th.Tensor, n_rays: int,
                 sigma_fn: Optional[Callable], alpha_fn: Optional[Callable], early_stop_eps: float,
                 alpha_thre: float):
        """The visibility filter of ``sampling`` on marched samples."""
        if (sigma_fn is None and alpha_fn is None) or ray_indices.numel() == 0:
            return ray_indices, t_starts, t_ends
        from .prop_sampler import render_weight_from_density
        if sigma_fn is not None:
            sigmas = sigma_fn(t_starts, t_ends, ray_indices).reshape(-1).float()
            _, trans, alphas = render_weight_from_density(t_starts, t_ends, sigmas, ray_indices, n_rays)
        else:
            # transmittance of given opacities through the same kernel: b = log(1 - alpha) over a unit
            # interval (alpha capped below 1, where b would be -inf)
            alphas = alpha_fn(t_starts, t_ends, ray_indices).reshape(-1).float()
            b = th.log1p(-alphas.clamp(max=1.0 - 2.0 ** -24))
            _, trans, _ = render_weight_from_density(th.zeros_like(b), th.ones_like(b), -b, ray_indices, n_rays)
        keep = (alphas >= alpha_thre) & (trans >= early_stop_eps)
        return ray_indices[keep], t_starts[keep], t_ends[keep]

    # -- grid update ----------------------------------------------------------------------------
    @th.no_grad()
    def update_every_n_steps(self, step: int, occ_eval_fn: Callable, occ_thre: float = 1e-2, ema_decay: float = 0.95,
                             warmup_steps: int = 256, n: int = 16) -> None:
        """nerfacc's schedule: every n steps, evaluate ``occ_eval_fn`` ([M, 3] points -> [M] or [M, 1]
        occupancy) at one jittered point of each chosen cell (all cells during warm-up, afterwards a
        quarter drawn uniformly plus up to a quarter drawn from the occupied ones);
        occs = max(occs * ema_decay, occ); binaries = occs > min(occ_thre, mean(occs))."""
        if step % n != 0:
            return
        dev = self.occs.device
        rx, ry, rz = self.resolution
        if step < warmup_steps:
            idx = th.arange(self.cells, device=dev)
        else:
            quarter = self.cells // 4
            uniform = th.randint(self.cells, (quarter,), device=dev)
            occupied = th.nonzero(self.binaries.reshape(-1))[:, 0]
            if quarter < occupied.numel():
                occupied = occupied[th.randint(occupied.numel(), (quarter,), device=dev)]
            idx = th.cat([uniform, occupied])
        coords = th.stack([idx // (ry * rz), (idx // rz) % ry, idx % rz], dim=-1).float()
        x = (coords + th.rand_like(coords)) / th.tensor([rx, ry, rz], device=dev, dtype=th.float32)
        lo = th.tensor(self.aabb[:3], device=dev)
        hi = th.tensor(self.aabb[3:], device=dev)
        occ = occ_eval_fn(lo + x * (hi - lo)).reshape(-1).float()
        self.occs[idx] = th.maximum(self.occs[idx] * ema_decay, occ)
        thre = th.clamp(self.occs.mean(), max=occ_thre)
        self.binaries.copy_((self.occs > thre).view_as(self.binaries))


class CascadedOccGridEstimator(OccGridEstimator):
    """nerfacc.OccGridEstimator(roi_aabb, resolution=128, levels=L) restated, for unbounded scenes:
    Instant-NGP's cascaded grids.  Level l covers the region of interest enlarged 2^l times about its
    centre, every level at the same resolution, so cells double in size away from it.  Buffers (in
    ``state_dict``, nerfacc's layout): ``occs`` fp32 [levels * cells], ``binaries`` bool [levels, rx,
    ry, rz]; ``aabbs`` fp32 [levels, 6] are the boxes the kernel is given.  ``sampling`` also takes
    ``cone_angle >= 0`` (the step grows as t * cone_angle once that exceeds render_step_size) and per-ray
    ``t_min`` / ``t_max``: nerf_occ_cascade_count / nerf_occ_cascade_write (csrc/occgrid_cascade.hip),
    the cascaded marching contract of include/nerf_amd.h.  With levels=1, cone_angle=0 and no ray bounds
    the samples are ``OccGridEstimator``'s bit for bit."""

    def __init__(self, roi_aabb: Sequence[float], resolution: Union[int, Sequence[int]] = 128, levels: int = 1):
        nn.Module.__init__(self)        # not the base's: it refuses levels != 1
        levels = int(levels)
        if not 1 <= levels <= K._lib.NERF_OCC_MAX_LEVELS:
            raise ValueError(f"levels must lie in [1, {K._lib.NERF_OCC_MAX_LEVELS}]")
        aabb = [float(v) for v in (roi_aabb.tolist() if isinstance(roi_aabb, th.Tensor) else roi_aabb)]
        if len(aabb) != 6 or not all(lo < hi for lo, hi in zip(aabb[:3], aabb[3:])):
            raise ValueError("roi_aabb must be [xmin, ymin, zmin, xmax, ymax, zmax] with min < max")
        res = [int(resolution)] * 3 if isinstance(resolution, int) else [int(r) for r in resolution]
        if len(res) != 3 or min(res) < 1:
            raise ValueError("resolution must be a positive int or three of them")
        self.aabb = tuple(aabb)
        self.resolution = tuple(res)
        self.levels = levels
        self.cells = res[0] * res[1] * res[2]
        # nerfacc's enlargement, every operation in fp32 (the contract: the kernel derives nothing)
        lo, hi = th.tensor(aabb[:3], dtype=th.float32), th.tensor(aabb[3:], dtype=th.float32)
        c, h = (lo + hi) * 0.5, (hi - lo) * 0.5
        aabbs = th.stack([th.cat([c - h * 2.0 ** l, c + h * 2.0 ** l]) for l in range(levels)])
        self._boxes = aabbs.tolist()    # the host copy the kernel call takes
        self.register_buffer("aabbs", aabbs, persistent=False)
        self.register_buffer("occs", th.zeros(levels * self.cells))
        self.register_buffer("binaries", th.zeros([levels] + res, dtype=th.bool))
        self._bits = None
        self._bits_src = None
        self._status = None

    @th.no_grad()
    def _march(self, rays_o: th.Tensor, rays_d: th.Tensor, near_plane: float, far_plane: float,
               render_step_size: float, stratified: bool, cone_angle: float = 0.0,
               t_min: Optional[th.Tensor] = None, t_max: Optional[th.Tensor] = None):
        if self.binaries.device.type != "cuda":
            raise RuntimeError("CascadedOccGridEstimator.sampling needs the estimator on a ROCm device; "
                               "there is no CPU path")
        rays_o, rays_d = rays_o.contiguous(), rays_d.contiguous()
        n_rays = rays_o.shape[0]
        seed = _rng_seed() if stratified else 0
        # a step is never shorter than render_step_size, so the lattice's capacity bounds every ray
        words = K.occ_mask_words(near_plane, far_plane, render_step_size)
        ws = th.empty(K.occ_march_workspace_bytes(n_rays, words), device=rays_o.device, dtype=th.uint8)
        bound = lambda t: None if t is None else t.to(th.float32).contiguous()
        counts = K.occ_cascade_count(rays_o, rays_d, self._boxes, self.resolution, self.grid_bits(), near_plane,
                                     far_plane, render_step_size, cone_angle, stratified, seed, words, ws,
                                     self.status(), bound(t_min), bound(t_max))
        offsets = th.cumsum(counts, dim=0)
        total = int(offsets[-1].item()) if n_rays else 0      # the one host synchronisation
        return K.occ_cascade_write(n_rays, render_step_size, cone_angle, words, ws, offsets, total)

    @th.no_grad()
    def sampling(self, rays_o: th.Tensor, rays_d: th.Tensor, sigma_fn: Optional[Callable] = None,
                 alpha_fn: Optional[Callable] = None, near_plane: float = 0.0, far_plane: float = 1e10,
                 render_step_size: float = 1e-3, early_stop_eps: float = 1e-4, alpha_thre: float = 0.0,
                 stratified: bool = False, cone_angle: float = 0.0, t_min: Optional[th.Tensor] = None,
                 t_max: Optional[th.Tensor] = None):
        """``OccGridEstimator.sampling`` through the cascade, plus ``cone_angle >= 0`` and per-ray
        ``t_min`` / ``t_max`` (fp32 [n_rays], each optional; they narrow [near_plane, far_plane]).  The
        same outputs, the same one host synchronisation, the same visibility filter."""
        if not float(cone_angle) >= 0.0:
            raise ValueError("cone_angle must be >= 0")
        if sigma_fn is not None and alpha_fn is not None:
            raise ValueError("give sigma_fn or alpha_fn, not both")
        marched = self._march(rays_o, rays_d, near_plane, far_plane, render_step_size, stratified,
                              float(cone_angle), t_min, t_max)
        return self._visible(*marched, rays_o.shape[0], sigma_fn, alpha_fn, early_stop_eps, alpha_thre)

    @th.no_grad()
    def update_every_n_steps(self, step: int, occ_eval_fn: Callable, occ_thre: float = 1e-2, ema_decay: float = 0.95,
                             warmup_steps: int = 256, n: int = 16) -> None:
        """nerfacc's schedule per level: every n steps, ``occ_eval_fn`` at one jittered point of each
        chosen cell, mapped into the cell's own level's box (all cells of all levels during warm-up,
        afterwards per level a quarter drawn uniformly plus up to a quarter drawn from the level's
        occupied cells); then one EMA and one threshold over all levels:
        occs = max(occs * ema_decay, occ); binaries = occs > min(occ_thre, mean(occs))."""
        if step % n != 0:
            return
        dev = self.occs.device
        rx, ry, rz = self.resolution
        res = th.tensor([rx, ry, rz], device=dev, dtype=th.float32)
        boxes = self.aabbs
        for l in range(self.levels):
            if step < warmup_steps:
                idx = th.arange(self.cells, device=dev)
            else:
                quarter = self.cells // 4
                uniform = th.randint(self.cells, (quarter,), device=dev)
                occupied = th.nonzero(self.binaries[l].reshape(-1))[:, 0]
                if quarter < occupied.numel():
                    occupied = occupied[th.randint(occupied.numel(), (quarter,), device=dev)]
                idx = th.cat([uniform, occupied])
            coords = th.stack([idx // (ry * rz), (idx // rz) % ry, idx % rz], dim=-1).float()
            x = (coords + th.rand_like(coords)) / res
            lo, hi = boxes[l, :3], boxes[l, 3:]
            occ = occ_eval_fn(lo + x * (hi - lo)).reshape(-1).float()
            idx = idx + l * self.cells
            self.occs[idx] = th.maximum(self.occs[idx] * ema_decay, occ)
        thre = th.clamp(self.occs.mean(), max=occ_thre)
        self.binaries.copy_((self.occs > thre).view_as(self.binaries))


__all__ = ["CascadedOccGridEstimator", "OccGridEstimator", "pack_grid_bits"]
