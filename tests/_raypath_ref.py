"""CPU restatements of the stand-alone ray-path kernels (csrc/composite.hip, csrc/sampling.hip),
shared by tests/test_raypath_ref.py (CPU), test_gpu_composite_edges.py and
test_gpu_sampling_edges.py.  No GPU, no HIP library.

composite_ref64        the compositing contract of include/nerf_amd.h in fp64 torch, gradients
                       through autograd;
sample_uniform_ref     sample_uniform_kernel in numpy fp32: every operation rounded to fp32 in the
                       kernel's order and nothing contracted (the kernel is built with fp contract
                       off), except what the kernel spells out: far - D in double, rounded once, and
                       one fused multiply-add per linspace element;
resample_fallback_ref  the `status & 1` branch of resample_finish_kernel, the same way.
"""
import numpy as np
import torch

from oracle import nerf_oracle as O

F32 = np.float32


def _split(head_or_pair):
    """[..., 4] rows of [rgb | sigma], or a (sigma, color) pair -> (sigma [B, S], color [B, S, 3])."""
    if isinstance(head_or_pair, (tuple, list)):
        sigma, color = head_or_pair
        return sigma, color
    return head_or_pair[..., 3], head_or_pair[..., :3]


def composite_ref64(head_or_pair, dist, sa, sb, act, shift=0.0, g_rgb=None, g_w=None):
    """fp64 compositing of raw inputs: with act, sigma = softplus(raw - shift) (threshold 8: the
    identity above it) and c = sigmoid(raw colour); b = ((-sigma delta) sa) sb, T = exp of the
    exclusive prefix sum of b, w = T (1 - e^b), rgb = sum_s w c.

    Returns (rgb [B, 3], w [B, S], d_sigma [B, S], d_color [B, S, 3]) as fp64 tensors; the two
    gradients are those of <g_rgb, rgb> + <g_w, w> with respect to the raw inputs (None when
    g_rgb is None; g_w = None is a zero weight gradient)."""
    sigma, color = _split(head_or_pair)
    B, S = dist.shape
    raw_s = sigma.detach().double().reshape(B, S).clone().requires_grad_(True)
    raw_c = color.detach().double().reshape(B, S, 3).clone().requires_grad_(True)
    if act:
        x = raw_s - float(shift)
        # the clamp keeps exp finite on the branch that `where` discards (its gradient is 0 * inf)
        sig = torch.where(x > 8, x, torch.log1p(torch.exp(torch.clamp(x, max=8.0))))
        c = torch.sigmoid(raw_c)
    else:
        sig, c = raw_s, raw_c
    b = ((-sig * dist.double()) * float(np.float32(sa))) * float(np.float32(sb))
    T = torch.exp(torch.cumsum(b, dim=1) - b)
    w = T * (1 - torch.exp(b))
    rgb = torch.sum(w.unsqueeze(-1) * c, dim=1)
    if g_rgb is None:
        return rgb.detach(), w.detach(), None, None
    loss = (rgb * g_rgb.double()).sum()
    if g_w is not None:
        loss = loss + (w * g_w.double()).sum()
    loss.backward()
    return rgb.detach(), w.detach(), raw_s.grad, raw_c.grad


def _fma32(a, b, c):
    """fp32 fused multiply-add a * b + c on arrays (b integer-valued below 2^24): the product of two
    24-bit significands is exact in double, and the sum is checked to be exact in double as well
    (TwoSum), so the single rounding to fp32 is the fused operation's."""
    a, b, c = (np.asarray(x, dtype=np.float64) for x in (a, b, c))
    p = a * b
    s = c + p
    bb = s - c
    assert np.all((c - (s - bb)) + (p - bb) == 0), "fma emulation: the double sum is not exact"
    return s.astype(F32)


def linspace_at(start, end, steps, idx):
    """csrc/common.h linspace_at (torch.linspace's formula) on fp32 scalars and an integer index
    array: step = (end - start) / (steps - 1) in fp32; the first half is fma(step, idx, start), the
    second half fma(-step, steps - idx - 1, end); one step gives start."""
    start, end = F32(start), F32(end)
    idx = np.asarray(idx, dtype=np.int64)
    if steps == 1:
        return np.full(idx.shape, start, F32)
    step = F32(F32(end - start) / F32(steps - 1))
    up = _fma32(step, idx, start)
    down = _fma32(-step, steps - idx - 1, end)
    return np.where(idx < steps // 2, up, down).astype(F32)


def last_sample_start(near, far, steps):
    """csrc/common.h last_sample_start: far - (far - near) / steps in double on the fp32 near and
    far, rounded to fp32 once."""
    near, far = float(F32(near)), float(F32(far))
    return F32(far - (far - near) / steps)


def _t_end(t_start, far):
    t_end = np.empty_like(t_start)
    t_end[:, :-1] = t_start[:, 1:]
    t_end[:, -1] = F32(far)
    return t_end


def sample_uniform_ref(B, S, near, far, stratified, offset_size, seed, counter):
    """sample_uniform_kernel: t[ray, s] = linspace_at(near, last_sample_start(near, far, S), S, s),
    + U[ray S + s] D when stratified, with D = (far - near) / S formed in fp32, + (U'[ray] D)
    offset_size when the offset is not zero; U = Philox(seed, counter), U' = Philox(seed, counter ^
    2^63).  t_end is the next
    t_start (recomputed by the kernel with the same operations, so the same bits), far at the end.
    Returns (t_start, t_end) as fp32 arrays [B, S]."""
    near, far, offset_size = F32(near), F32(far), F32(offset_size)
    interval = F32(F32(far - near) / F32(S))
    s = np.arange(S, dtype=np.int64)
    t = np.broadcast_to(linspace_at(near, last_sample_start(near, far, S), S, s), (B, S)).astype(F32)
    if stratified:
        idx = np.arange(B, dtype=np.uint64)[:, None] * np.uint64(S) + np.arange(S, dtype=np.uint64)[None, :]
        u = O.philox_uniform(seed, counter, idx)
        t = (t + (u * interval).astype(F32)).astype(F32)
    if offset_size != 0:
        u = O.philox_uniform(seed, counter ^ (1 << 63), np.arange(B, dtype=np.uint64))[:, None]
        t = (t + ((u * interval).astype(F32) * offset_size).astype(F32)).astype(F32)
    return t, _t_end(t, far)


def resample_fallback_ref(B, N, near, far, seed, counter):
    """The batch-wide fallback of nerf_resample_pdf (resample_finish_kernel, status bit 0 set):
    equidistant samples shifted per ray by -(U'[ray] D), D = (far - near) / N in fp32,
    U' = Philox(seed, counter ^ 2^63).  Returns (t_start, t_end) as fp32 arrays [B, N]."""
    near, far = F32(near), F32(far)
    interval = F32(F32(far - near) / F32(N))
    u = O.philox_uniform(seed, counter ^ (1 << 63), np.arange(B, dtype=np.uint64))[:, None]
    base = linspace_at(near, last_sample_start(near, far, N), N, np.arange(N, dtype=np.int64))[None, :]
    t = (base + ((u * interval).astype(F32) * F32(-1.0)).astype(F32)).astype(F32)
    return t, _t_end(t, far)


def composite_inputs(B, S, seed):
    """The edge tests' inputs: raw [rgb | sigma] head rows with every 7th sample's density pushed
    past the softplus threshold, interval lengths that let transmittance decay over the whole ray at
    any S, and per-ray output gradients."""
    g = torch.Generator().manual_seed(seed)
    head = torch.randn(B, S, 4, generator=g) * 3
    head[:, ::7, 3] += 9
    dist = torch.rand(B, S, generator=g) * 3.2 / max(S, 16)
    g_rgb = torch.randn(B, 3, generator=g)
    g_w = torch.randn(B, S, generator=g)
    return head, dist, g_rgb, g_w


def activate32(head, shift):
    """fp32 softplus(thr 8)(raw - shift) and sigmoid of head rows: the act = 0 kernels' inputs."""
    return O.softplus8(head[..., 3] - shift).contiguous(), torch.sigmoid(head[..., :3]).contiguous()
