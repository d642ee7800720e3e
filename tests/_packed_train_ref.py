"""CPU restatements for training through the occupancy grid, shared by tests/test_packed_train_logic.py
(CPU), test_gpu_packed_points.py, test_gpu_distortion.py and test_gpu_occ_render.py.  No GPU, no HIP
library.

points_ref32        the points contract of include/nerf_amd.h in numpy fp32: every operation rounded to
                    fp32 on its own, nothing contracted; NaN rows for ray indices out of range;
points_bwd_ref64    its gradient to the rays: fp64 segment sums with the forward's fp32 midpoint;
distortion_direct64 the distortion loss as the direct O(S^2) double sum in fp64, gradient by autograd;
distortion_prefix   the prefix form the kernels evaluate (exclusive cumsums of w and w m), in a given
                    dtype, loss and the closed-form gradient of the contract;
distortion_case     the inputs of the distortion tests;
render_ref64        the packed renderer in fp64 torch (plain indexing for the points, the compositing
                    contract per segment) with the graph kept from the rays and the field's parameters.
"""
import numpy as np
import torch

import _occgrid_ref as R

F32 = np.float32
LENGTHS = [0, 1, 63, 64, 65, 0, 0, 128, 129, 1500, 2, 0]


def points_ref32(rays_o, rays_d, ray_indices, t_starts, t_ends):
    """(positions fp32 [N, 3], dirs fp32 [N, 3])."""
    o = np.asarray(rays_o, dtype=F32).reshape(-1, 3)
    d = np.asarray(rays_d, dtype=F32).reshape(-1, 3)
    ri = np.asarray(ray_indices, dtype=np.int64)
    t0, t1 = np.asarray(t_starts, dtype=F32), np.asarray(t_ends, dtype=F32)
    ok = (ri >= 0) & (ri < o.shape[0])
    safe = np.where(ok, ri, 0)
    pos = np.full((ri.size, 3), np.nan, dtype=F32)
    dirs = np.full((ri.size, 3), np.nan, dtype=F32)
    if o.shape[0] == 0:
        return pos, dirs
    tm = ((t0 + t1).astype(F32) * F32(0.5)).astype(F32)
    p = (o[safe] + (tm[:, None] * d[safe]).astype(F32)).astype(F32)
    pos[ok], dirs[ok] = p[ok], d[safe][ok]
    return pos, dirs


def points_bwd_ref64(seg, t_starts, t_ends, g_positions, g_dirs=None):
    """(g_o fp64 [R, 3], g_d fp64 [R, 3]); tm is the forward's fp32 midpoint."""
    seg = np.asarray(seg, dtype=np.int64)
    t0, t1 = np.asarray(t_starts, dtype=F32), np.asarray(t_ends, dtype=F32)
    tm = ((t0 + t1).astype(F32) * F32(0.5)).astype(np.float64)
    gp = np.asarray(g_positions, dtype=np.float64)
    n_rays = seg.size - 1
    g_o, g_d = np.zeros((n_rays, 3)), np.zeros((n_rays, 3))
    for r in range(n_rays):
        a, b = int(seg[r]), int(seg[r + 1])
        g_o[r] = gp[a:b].sum(0)
        g_d[r] = (tm[a:b, None] * gp[a:b]).sum(0)
        if g_dirs is not None:
            g_d[r] += np.asarray(g_dirs, dtype=np.float64)[a:b].sum(0)
    return g_o, g_d


def _ray_terms(w, t0, t1):
    return w, (t0 + t1) / 2, t1 - t0


def distortion_direct64(weights, t_starts, t_ends, seg, g_loss=None):
    """(loss fp64 [R], d weights fp64 [N] of <g_loss, loss> by autograd, None without g_loss):
    sum_ij w_i w_j |m_i - m_j| + 1/3 sum_i w_i^2 delta_i per segment, nothing assumed of the order."""
    w_all = weights.detach().double().clone().requires_grad_(True)
    t0, t1 = t_starts.double(), t_ends.double()
    losses = []
    for r in range(seg.numel() - 1):
        a, b = int(seg[r]), int(seg[r + 1])
        w, m, delta = _ray_terms(w_all[a:b], t0[a:b], t1[a:b])
        pair = (w[:, None] * w[None, :] * (m[:, None] - m[None, :]).abs()).sum()
        losses.append(pair + (w * w * delta).sum() / 3)
    loss = torch.stack(losses) if losses else torch.zeros(0, dtype=torch.float64)
    grad = None
    if g_loss is not None:
        (loss * g_loss.double()).sum().backward()
        grad = w_all.grad if w_all.grad is not None else torch.zeros_like(w_all)
    return loss.detach(), grad


def distortion_prefix(weights, t_starts, t_ends, seg, dtype, g_loss=None):
    """The contract's prefix form evaluated with torch ops of `dtype` (fp64: what the kernels
    accumulate; fp32: what an eager implementation gives): (loss [R], d weights [N] by the closed
    form of the contract, None without g_loss)."""
    w_all, t0, t1 = weights.to(dtype), t_starts.to(dtype), t_ends.to(dtype)
    n_rays = seg.numel() - 1
    loss = torch.zeros(n_rays, dtype=dtype)
    grad = torch.zeros_like(w_all) if g_loss is not None else None
    for r in range(n_rays):
        a, b = int(seg[r]), int(seg[r + 1])
        if a == b:
            continue
        w, m, delta = _ray_terms(w_all[a:b], t0[a:b], t1[a:b])
        wm = w * m
        W_in, WM_in = torch.cumsum(w, 0), torch.cumsum(wm, 0)
        W_ex, WM_ex = W_in - w, WM_in - wm
        loss[r] = (w * w * delta / 3 + 2 * w * (m * W_ex - WM_ex)).sum()
        if grad is not None:
            W_af, WM_af = W_in[-1] - W_in, WM_in[-1] - WM_in
            grad[a:b] = g_loss[r].to(dtype) * (2.0 / 3.0 * w * delta + 2 * (m * W_ex - WM_ex + WM_af - m * W_af))
    return loss, grad


def distortion_case():
    """(weights fp32 [N], t_starts [N], t_ends [N], seg [R + 1], g_loss fp32 [R]): the fp32-rounded
    weights of the packed compositing restatement on packed_inputs(LENGTHS, 7), with its intervals
    (abutting, so the midpoints ascend; every t below far = 6)."""
    args = R.packed_inputs(LENGTHS, 7)
    sigma, rgb, t0, t1, seg = args[:5]
    w = R.packed_composite_ref64(sigma, rgb, t0, t1, seg)[3].float()
    g = torch.Generator().manual_seed(77)
    g_loss = torch.randn(len(LENGTHS), generator=g)
    return w, t0, t1, seg, g_loss


def render_ref64(field64, rays_o, rays_d, ray_indices, t_starts, t_ends, bkgd=None):
    """The packed renderer in fp64 torch with the graph kept from the rays (leaf fp64 tensors) and the
    field's parameters to the outputs: points by plain indexing at the forward's fp32 midpoint, the
    compositing contract per segment.  (colors [R, 3], opacity [R, 1], depth [R, 1], weights [N])."""
    n_rays = rays_o.shape[0]
    tm = ((t_starts + t_ends) * 0.5).double()                       # fp32 operations, then widened
    dirs = rays_d[ray_indices]
    pos = rays_o[ray_indices] + tm[:, None] * dirs
    rgb, sigma = field64(pos, dirs)
    sigma = sigma.reshape(-1)
    t0, t1 = t_starts.double(), t_ends.double()
    seg = torch.searchsorted(ray_indices, torch.arange(n_rays + 1))
    colors, opacity, depth, ws = [], [], [], []
    for r in range(n_rays):
        a, b_ = int(seg[r]), int(seg[r + 1])
        b = -sigma[a:b_] * (t1[a:b_] - t0[a:b_])
        w = torch.exp(torch.cumsum(b, 0) - b) * (1 - torch.exp(b))
        ws.append(w)
        colors.append((w[:, None] * rgb[a:b_]).sum(0))
        opacity.append(w.sum())
        depth.append((w * tm[a:b_]).sum())
    colors, opacity = torch.stack(colors), torch.stack(opacity)[:, None]
    if bkgd is not None:
        colors = colors + bkgd.double() * (1 - opacity)
    return colors, opacity, torch.stack(depth)[:, None], torch.cat(ws)


def ray_indices_of(lengths):
    return torch.repeat_interleave(torch.arange(len(lengths)), torch.tensor(lengths))
