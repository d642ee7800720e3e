"""CPU restatements for the occupancy-grid sampler and the packed compositing, shared by
tests/test_occgrid_logic.py (CPU), test_gpu_occgrid.py and test_gpu_composite_packed.py.  No GPU, no
HIP library.

march_ref              the marching contract of include/nerf_amd.h (csrc/occgrid.hip) in numpy fp32:
                       every operation rounded to fp32 on its own, in the kernel's order, nothing
                       contracted; min / max as the comparisons the contract spells out;
packed_composite_ref64 the packed compositing contract in fp64: tests/_raypath_ref.py's composite_ref64
                       per segment, plus opacity, depth, trans and alphas;
packed_composite_fp32  the same contract evaluated with fp32 torch ops (what an eager fp32
                       implementation gives), for the distance that sets the bars' margin.
"""
import numpy as np
import torch

from _raypath_ref import activate32, composite_inputs, composite_ref64
from oracle import nerf_oracle as O

F32 = np.float32
MAX_STEPS = 8192


def march_ref(rays_o, rays_d, aabb, res, binaries, near, far, dt, stratified=False, seed=0, counter=0,
              mask_words=MAX_STEPS // 64):
    """(ray_indices int64 [N], t_starts fp32 [N], t_ends fp32 [N], status int, steps considered per
    ray int [R]).  binaries: bool array [rx, ry, rz] (or flat, x-major)."""
    rays_o = np.asarray(rays_o, dtype=F32).reshape(-1, 3)
    rays_d = np.asarray(rays_d, dtype=F32).reshape(-1, 3)
    lo = np.asarray(aabb[:3], dtype=F32)
    hi = np.asarray(aabb[3:], dtype=F32)
    res = [int(r) for r in res]
    flat = np.asarray(binaries, dtype=bool).reshape(-1)
    assert flat.size == res[0] * res[1] * res[2]
    near, far, dt = F32(near), F32(far), F32(dt)
    ext = (hi - lo).astype(F32)
    out_r, out_0, out_1, considered = [], [], [], []
    status = 0
    with np.errstate(all="ignore"):
        for r in range(rays_o.shape[0]):
            o, d = rays_o[r], rays_d[r]
            tn, tf = F32(-np.inf), F32(np.inf)
            hit = True
            for a in range(3):
                if d[a] == 0:
                    if not (lo[a] <= o[a] < hi[a]):
                        hit = False
                else:
                    inv = F32(F32(1.0) / d[a])
                    ta = F32(F32(lo[a] - o[a]) * inv)
                    tb = F32(F32(hi[a] - o[a]) * inv)
                    mn = ta if ta < tb else tb
                    mx = tb if ta < tb else ta
                    tn = mn if mn > tn else tn
                    tf = mx if mx < tf else tf
            t_min = near if near > tn else tn
            t_max = far if far < tf else tf
            hit = hit and bool(t_min < t_max)
            n = 0
            if hit:
                if stratified:
                    u = O.philox_uniform(seed, counter, np.array([r], dtype=np.uint64))[0]
                    t_min = F32(t_min + F32(u * dt))
                x = np.ceil(F32(F32(t_max - t_min) / dt))
                if x > MAX_STEPS:
                    status |= 1
                n = (int(x) if x < MAX_STEPS else MAX_STEPS) if x >= 1 else 0
                if n > 64 * mask_words:
                    status |= 2
                    n = 64 * mask_words
            considered.append(n)
            if n == 0:
                continue
            k = np.arange(n)
            t0 = (t_min + (k.astype(F32) * dt).astype(F32)).astype(F32)
            e1 = (t_min + ((k + 1).astype(F32) * dt).astype(F32)).astype(F32)
            t1 = np.where(e1 < t_max, e1, t_max).astype(F32)
            keep = t0 < t1
            tm = ((t0 + t1).astype(F32) * F32(0.5)).astype(F32)
            cell = np.zeros(n, dtype=np.int64)
            for a in range(3):
                p = (o[a] + (tm * d[a]).astype(F32)).astype(F32)
                c = np.floor((((p - lo[a]).astype(F32) / ext[a]).astype(F32) * F32(res[a])).astype(F32))
                keep &= (c >= 0) & (c < res[a])
                cell = cell * res[a] + np.where(keep, c, 0).astype(np.int64)
            keep &= flat[np.where(keep, cell, 0)]
            out_r.append(np.full(int(keep.sum()), r, dtype=np.int64))
            out_0.append(t0[keep])
            out_1.append(t1[keep])
    cat = lambda xs, dt_: np.concatenate(xs).astype(dt_) if xs else np.zeros(0, dtype=dt_)
    return cat(out_r, np.int64), cat(out_0, F32), cat(out_1, F32), status, np.asarray(considered, dtype=np.int64)


def count_construction(m):
    """The count construction: grid [0, 1]^3 at 8^3, all occupied, near 0, far 1e9, dt 1, the ray
    o = (-1, 0.3, 0.6), d = (1/m, 0, 0): exactly m samples, all abutting bitwise."""
    aabb = [0.0, 0.0, 0.0, 1.0, 1.0, 1.0]
    o = np.array([[-1.0, 0.3, 0.6]], dtype=F32)
    d = np.array([[F32(1.0) / F32(m), 0.0, 0.0]], dtype=F32)
    return o, d, aabb, (8, 8, 8), np.ones((8, 8, 8), dtype=bool), 0.0, 1e9, 1.0


COUNT_M = (1, 2, 63, 64, 65, 128, 129, 200)


def checkerboard_case():
    """64 seeded rays aimed at a checkerboard 8^3 grid over [-1, 1]^3, dt 1/64, near/far 0.05/6; every
    eighth ray un-normalised."""
    rng = np.random.default_rng(20240607)
    o = rng.normal(size=(64, 3))
    o = (o / np.linalg.norm(o, axis=1, keepdims=True) * 2.5).astype(F32)
    target = rng.uniform(-0.8, 0.8, size=(64, 3))
    d = target - o
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    d[::8] *= rng.uniform(0.3, 2.5, size=(8, 1))
    i, j, k = np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij")
    binaries = ((i + j + k) % 2).astype(bool)
    return o, d.astype(F32), [-1.0, -1.0, -1.0, 1.0, 1.0, 1.0], (8, 8, 8), binaries, 0.05, 6.0, 1.0 / 64


def segments_of(lengths):
    seg = np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))])
    return torch.from_numpy(seg)


def packed_inputs(lengths, seed, far=6.0):
    """Packed inputs: every non-empty segment r is one ray of composite_inputs(1, L, seed + r),
    activated as the act = 0 layout of the edge tests activates it (activate32, shift 0: softplus
    densities, some past the threshold, and sigmoid colours), its intervals abutting from t = 1 with
    composite_inputs' lengths (so every t stays below 4.2 < far).  Returns (sigma [N], rgb [N, 3],
    t_starts [N], t_ends [N], seg, g_colors [R, 3], g_opacity [R], g_depth [R], g_weights [N])."""
    R = len(lengths)
    sig, col, t0, t1, g_w = [], [], [], [], []
    g_rgb = torch.zeros(R, 3)
    for r, L in enumerate(lengths):
        if L == 0:
            continue
        head, dist, gr, gw = composite_inputs(1, L, seed + r)
        s_, c_ = activate32(head, 0.0)
        start = 1.0 + torch.cumsum(dist[0], 0) - dist[0]
        sig.append(s_[0]); col.append(c_[0]); t0.append(start); t1.append(start + dist[0]); g_w.append(gw[0])
        g_rgb[r] = gr[0]
    cat = lambda xs, shape: torch.cat(xs).contiguous() if xs else torch.zeros(shape)
    g = torch.Generator().manual_seed(seed + 1000)
    g_op, g_dep = torch.randn(R, generator=g), torch.randn(R, generator=g)
    t1 = cat(t1, 0)
    assert t1.numel() == 0 or float(t1.max()) < far
    return (cat(sig, 0), cat(col, (0, 3)), cat(t0, 0), t1, segments_of(lengths), g_rgb, g_op, g_dep, cat(g_w, 0))


def _packed(sigma, rgb, t0, t1, seg, dtype, g_colors=None, g_opacity=None, g_depth=None, g_weights=None):
    R = seg.numel() - 1
    s = sigma.detach().to(dtype).clone().requires_grad_(True)
    c = rgb.detach().to(dtype).clone().requires_grad_(True) if rgb is not None else None
    t0, t1 = t0.to(dtype), t1.to(dtype)
    colors, opacity, depth, ws, Ts, als = [], [], [], [], [], []
    for r in range(R):
        a, b_ = int(seg[r]), int(seg[r + 1])
        b = -s[a:b_] * (t1[a:b_] - t0[a:b_])
        T = torch.exp(torch.cumsum(b, 0) - b)
        al = 1 - torch.exp(b)
        w = T * al
        ws.append(w); Ts.append(T); als.append(al)
        colors.append((w[:, None] * c[a:b_]).sum(0) if c is not None else torch.zeros(3, dtype=dtype))
        opacity.append(w.sum())
        depth.append((w * ((t0[a:b_] + t1[a:b_]) / 2)).sum())
    colors, opacity, depth = torch.stack(colors), torch.stack(opacity), torch.stack(depth)
    w, T, al = torch.cat(ws), torch.cat(Ts), torch.cat(als)
    d_sigma = d_rgb = None
    if g_colors is not None:
        loss = (opacity * g_opacity.to(dtype)).sum() + (depth * g_depth.to(dtype)).sum() + (w * g_weights.to(dtype)).sum()
        if c is not None:
            loss = loss + (colors * g_colors.to(dtype)).sum()
        loss.backward()
        d_sigma, d_rgb = s.grad, (c.grad if c is not None else None)
    return tuple(x.detach() if x is not None else None for x in (colors, opacity, depth, w, T, al, d_sigma, d_rgb))


def packed_composite_ref64(sigma, rgb, t0, t1, seg, g_colors=None, g_opacity=None, g_depth=None, g_weights=None):
    """fp64, tests/_raypath_ref.py::composite_ref64 (act 0, scales 1) on each segment as a one-ray
    batch: (colors [R, 3], opacity [R], depth [R], weights [N], trans [N], alphas [N], d sigma [N],
    d rgb [N, 3]).  opacity = sum w and depth = sum w tm are linear in the weights, so the gradients of
    <g_colors, colors> + <g_opacity, opacity> + <g_depth, depth> + <g_weights, weights> are
    composite_ref64's with the weight gradient g_weights + g_opacity + g_depth tm (None without
    g_colors; d rgb None without rgb).  An empty ray gives zeros."""
    R, N = seg.numel() - 1, sigma.numel()
    f = dict(dtype=torch.float64)
    colors, opacity, depth = torch.zeros(R, 3, **f), torch.zeros(R, **f), torch.zeros(R, **f)
    w, T, al = torch.zeros(N, **f), torch.zeros(N, **f), torch.zeros(N, **f)
    grads = g_colors is not None
    d_sigma = torch.zeros(N, **f) if grads else None
    d_rgb = torch.zeros(N, 3, **f) if grads and rgb is not None else None
    for r in range(R):
        a, b_ = int(seg[r]), int(seg[r + 1])
        if a == b_:
            continue
        dist = (t1[a:b_].double() - t0[a:b_].double())[None]
        tm = (t0[a:b_].double() + t1[a:b_].double()) / 2
        col = rgb[a:b_][None] if rgb is not None else torch.zeros(1, b_ - a, 3)
        g_rgb = g_w = None
        if grads:
            g_rgb = g_colors[r][None] if rgb is not None else torch.zeros(1, 3)
            g_w = (g_weights[a:b_].double() + g_opacity[r].double() + g_depth[r].double() * tm)[None]
        c_r, w_r, ds, dc = composite_ref64((sigma[a:b_][None], col), dist, 1.0, 1.0, 0, 0.0, g_rgb, g_w)
        colors[r], w[a:b_] = c_r[0], w_r[0]
        opacity[r], depth[r] = w_r[0].sum(), (w_r[0] * tm).sum()
        b = -sigma[a:b_].double() * dist[0]
        T[a:b_], al[a:b_] = torch.exp(torch.cumsum(b, 0) - b), 1 - torch.exp(b)
        if grads:
            d_sigma[a:b_] = ds[0]
            if d_rgb is not None:
                d_rgb[a:b_] = dc[0]
    return colors, opacity, depth, w, T, al, d_sigma, d_rgb


def packed_composite_direct64(*args):
    """The packed contract written out in fp64 torch with autograd through every output: an independent
    derivation that packed_composite_ref64's chain rule is checked against."""
    return _packed(*args[:5], torch.float64, *args[5:])


def packed_composite_fp32(sigma, rgb, t0, t1, seg, g_colors=None, g_opacity=None, g_depth=None, g_weights=None):
    return _packed(sigma, rgb, t0, t1, seg, torch.float32, g_colors, g_opacity, g_depth, g_weights)
