"""One training step (forward + backward) of a GARF RadianceNetwork on 4096 rays through the occupancy
grid, on tools/occgrid_bench.py's scene: a pinhole camera at (0, 0, 4) (focal 1111 at 800 x 800), near /
far 2 / 6, a 128^3 grid over [-1.5, 1.5]^3 with a centred ball set so that 100 %, 25 % and 5 % of the
cells are occupied, render_step_size = (far - near) / 256.  The rays are a seeded draw of the frame.

Loss: mean squared colour against a fixed random target + 0.01 * mean distortion loss.  Three routes:
  batched       rendering() on the [4096, 256] lattice, distortion() on the [R, S] weights;
  packed-eager  sampling + rendering(ray_indices=...) with the sample points as eager torch indexing
                and the distortion loss as eager fp32 torch ops (global cumsums minus the value at each
                ray's start, index_add per ray);
  packed-hip    OccGridRenderer + distortion_loss (nerf_packed_points_*, nerf_distortion_*).
No visibility filter (early_stop_eps = alpha_thre = 0), so both packed routes see the same samples.

Then the two kernel pairs alone against their eager forms at that grid's N (forward + backward,
random output gradients), with the algorithmic bytes nerf_amd.kernels counts for them over the time,
as a fraction of the 8 TB/s HBM peak, and last the four kernels by themselves (events around each launch).

HIP events around each step after a warm-up of every route and shape; --rounds rounds visit the
routes in turn, so the spread across rounds is visible next to the differences.  Medians are printed.
Usage: python tools/occtrain_bench.py [--rounds R] [--rays 4096] [--out FILE]"""
import argparse
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "nerf-experiments_amd")]

import torch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--rays", type=int, default=4096)
ap.add_argument("--samples", type=int, default=256)
ap.add_argument("--out", default=None)
args = ap.parse_args()

import nerf_amd  # noqa: E402,F401
from nerf_amd import OccGridEstimator, OccGridRenderer, RadianceNetwork, distortion, packed_points  # noqa: E402
from nerf_amd.prop_sampler import _segments, rendering  # noqa: E402

if not torch.cuda.is_available():
    raise SystemExit("occtrain_bench: needs a GPU (there is no CPU path to time)")
dev = torch.device("cuda", 0)
torch.manual_seed(0)
model = RadianceNetwork(0.5, 2.0).to(dev)
NEAR, FAR, S = 2.0, 6.0, args.samples
DT = (FAR - NEAR) / S
LAMBDA = 0.01
HBM_PEAK = 8.0e12
lines = []


def emit(s):
    print(s, flush=True)
    lines.append(s)


def batch_rays(n):
    H = W = 800
    g = torch.Generator().manual_seed(1)
    pix = torch.randint(H * W, (n,), generator=g)
    j, i = (pix // W).float(), (pix % W).float()
    d = torch.stack([(i - W / 2 + 0.5) / 1111.0, -(j - H / 2 + 0.5) / 1111.0, -torch.ones_like(i)], -1)
    d = torch.nn.functional.normalize(d, dim=-1)
    o = torch.tensor([0.0, 0.0, 4.0]).expand_as(d).contiguous()
    return o.to(dev), d.to(dev), torch.rand(n, 3, generator=g).to(dev)


def ball_grid(fraction):
    est = OccGridEstimator([-1.5] * 3 + [1.5] * 3, resolution=128).to(dev)
    c = (torch.arange(128, device=dev, dtype=torch.float32) + 0.5) / 128 * 3.0 - 1.5
    r2 = c[:, None, None] ** 2 + c[None, :, None] ** 2 + c[None, None, :] ** 2
    if fraction >= 1.0:
        est.binaries.fill_(True)
    else:
        radius = (fraction * 27.0 * 3 / (4 * math.pi)) ** (1 / 3)
        est.binaries.copy_((r2 < radius * radius)[None])
    return est, float(est.binaries.float().mean())


rays_o, rays_d, target = batch_rays(args.rays)
R = args.rays
t_edges = NEAR + DT * torch.arange(S + 1, device=dev, dtype=torch.float32)


def eager_points(o, d, ri, t0, t1):
    dirs = d[ri]
    return o[ri] + dirs * ((t0 + t1) * 0.5)[:, None], dirs


def eager_distortion(w, t0, t1, ri, n_rays):
    m, delta = (t0 + t1) * 0.5, t1 - t0
    wm = w * m
    cw, cwm = torch.cumsum(w, 0), torch.cumsum(wm, 0)
    start = _segments(ri, n_rays)[:-1][ri]
    prev = (start - 1).clamp(min=0)
    first = start == 0
    w_ex = cw - w - torch.where(first, torch.zeros_like(w), cw[prev])
    wm_ex = cwm - wm - torch.where(first, torch.zeros_like(w), cwm[prev])
    per = w * w * delta / 3 + 2 * w * (m * w_ex - wm_ex)
    return torch.zeros(n_rays, device=w.device).index_add_(0, ri, per)


def finish(rgb, dist):
    model.zero_grad(set_to_none=True)
    loss = ((rgb - target) ** 2).mean() + LAMBDA * dist
    loss.backward()


def step_batched(_est, _ren):
    t0, t1 = t_edges[:-1].expand(R, S).contiguous(), t_edges[1:].expand(R, S).contiguous()

    def field(ts, te, _):
        pos = rays_o[:, None, :] + rays_d[:, None, :] * ((ts + te) * 0.5)[..., None]
        rgb, sigma = model(pos.reshape(-1, 3), rays_d[:, None, :].expand(R, S, 3).reshape(-1, 3))
        return rgb.reshape(R, S, 3), sigma.reshape(R, S)
    rgb, _, _, ex = rendering(t0, t1, rgb_sigma_fn=field)
    finish(rgb, distortion(ex["weights"], t0, t1).mean())
    return R * S


def step_packed_eager(est, _ren):
    ri, t0, t1 = est.sampling(rays_o, rays_d, near_plane=NEAR, far_plane=FAR, render_step_size=DT)

    def field(ts, te, idx):
        rgb, sigma = model(*eager_points(rays_o, rays_d, idx, ts, te))
        return rgb, sigma.reshape(-1)
    rgb, _, _, ex = rendering(t0, t1, ri, R, field)
    finish(rgb, eager_distortion(ex["weights"], t0, t1, ri, R).mean())
    return ri.numel()


def step_packed_hip(_est, ren):
    rgb, _, _, ex = ren(rays_o, rays_d, stratified=False)
    finish(rgb, ren.distortion_loss(ex))
    return ex["ray_indices"].numel()


def timed(fn, *a):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    n = fn(*a)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e), n


def kernel_pairs(est):
    """(name, bytes, fn) of the two pairs, hip and eager, on this grid's samples."""
    ri, t0, t1 = est.sampling(rays_o, rays_d, near_plane=NEAR, far_plane=FAR, render_step_size=DT)
    N = ri.numel()
    g = torch.Generator(device=dev).manual_seed(2)
    g_pos, g_dirs = torch.randn(N, 3, device=dev, generator=g), torch.randn(N, 3, device=dev, generator=g)
    w = torch.rand(N, device=dev, generator=g) * (2.0 / S)
    g_loss = torch.randn(R, device=dev, generator=g)
    o, d = rays_o.clone().requires_grad_(True), rays_d.clone().requires_grad_(True)
    wr = w.clone().requires_grad_(True)

    def points(fn):
        def run():
            o.grad = d.grad = None
            pos, dirs = fn(o, d, ri, t0, t1)
            torch.autograd.backward([pos, dirs], [g_pos, g_dirs])
            return N
        return run

    def dist(fn):
        def run():
            wr.grad = None
            fn(wr, t0, t1, ri, R).backward(g_loss)
            return N
        return run
    # forward 28 + 12 bytes per sample, backward 20 + 12 (nerf_amd/kernels.py packed_points_fwd / _bwd);
    # distortion 12 forward, 28 backward (two walks)
    return N, [("points hip", 72 * N + 56 * R, points(packed_points)), ("points eager", 72 * N + 56 * R, points(eager_points)),
               ("distortion hip", 40 * N + 24 * R, dist(distortion)), ("distortion eager", 40 * N + 24 * R, dist(eager_distortion))]


emit(f"occtrain_bench: {R} rays, near/far {NEAR}/{FAR}, step {DT:.6f} ({S} per full chord), {args.rounds} rounds, "
     f"forward + backward, loss = mse + {LAMBDA} * distortion")
routes = {"batched": step_batched, "packed-eager": step_packed_eager, "packed-hip": step_packed_hip}
grids = []
for f in (1.0, 0.25, 0.05):
    est, frac = ball_grid(f)
    ren = OccGridRenderer(model, est, NEAR, FAR, DT, early_stop_eps=0.0).to(dev)
    grids.append((est, ren, frac, *kernel_pairs(est)))
for est, ren, frac, N, pairs in grids:
    for fn in routes.values():
        fn(est, ren)                            # warm-up of every route and shape
    for _, _, fn in pairs:
        fn()
torch.cuda.synchronize()
ms = {}
kept = {}
for _ in range(args.rounds):
    for gi, (est, ren, frac, N, pairs) in enumerate(grids):
        for r, fn in routes.items():
            t, n = timed(fn, est, ren)
            ms.setdefault((gi, r), []).append(t)
            kept[(gi, r)] = n
        for name, nbytes, fn in pairs:
            t, _ = timed(fn)
            ms.setdefault((gi, name), []).append(t)
for gi, (est, ren, frac, N, pairs) in enumerate(grids):
    for r in routes:
        v = ms[(gi, r)]
        emit(f"cells set {100 * frac:5.1f} %  step {r:14s} median {statistics.median(v):9.3f} ms  (min {min(v):.3f}, max "
             f"{max(v):.3f})  samples {kept[(gi, r)]:>9d}")
    for name, nbytes, _ in pairs:
        v = ms[(gi, name)]
        med = statistics.median(v)
        emit(f"cells set {100 * frac:5.1f} %  pair {name:16s} median {med * 1e3:9.1f} us  (min {min(v) * 1e3:.1f}, max "
             f"{max(v) * 1e3:.1f})  N {N:>9d}  {nbytes / 1e6:8.2f} MB  {nbytes / (med * 1e-3) / HBM_PEAK * 100:5.1f} % of HBM peak")
# the four kernels by themselves: HIP events around each launch (nerf_amd.kernels.KernelTimer), so the
# autograd and searchsorted work of the pairs above is outside; mean of 5 launches
from nerf_amd import kernels as K  # noqa: E402
for est, ren, frac, N, pairs in grids:
    K.TIMER = K.KernelTimer()
    for _ in range(5):
        for name, _, fn in pairs:
            if name.endswith("hip"):
                fn()
    for fn_name, d in K.TIMER.summary(by="fn").items():
        us, nbytes = d["ms"] * 1e3 / d["launches"], d["bytes"] / d["launches"]
        emit(f"cells set {100 * frac:5.1f} %  kernel {fn_name:26s} mean {us:8.1f} us  N {N:>9d}  {nbytes / 1e6:8.2f} MB  "
             f"{nbytes / (us * 1e-6) / HBM_PEAK * 100:5.1f} % of HBM peak")
    K.TIMER = None
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
