"""Empty-space skipping on one 800 x 800 frame: the occupancy-grid marching alone, the packed path
end to end (OccGridEstimator.sampling + rendering(ray_indices=...)) and the batched rendering of the
same rays at 256 samples per ray, alternating on one card.

Workload: a pinhole camera at (0, 0, 4) looking at the origin (focal 1111, the Blender scenes'), a
randomly initialised GARF RadianceNetwork, near / far 2 / 6, a 128^3 grid over [-1.5, 1.5]^3 with a
centred ball marked occupied so that 100 %, 25 % and 5 % of the cells are set (100 %: every cell).
render_step_size = (far - near) / 256, the batched lattice's spacing, so a ray that is inside the
box from near to far has 256 steps.  The field runs under no_grad in chunks of --chunk rays, in
both paths; the packed path marches each chunk (one host synchronisation per chunk) and renders it.
Also timed: one nerf_composite_fwd launch on the whole batched lattice (random inputs), the cost the
marching has to stay below to be worth a launch of its own.

HIP events around each whole frame after a warm-up frame of every route; --rounds rounds visit the
routes in turn, so the spread across rounds is visible next to the difference between routes.
Usage: python tools/occgrid_bench.py [--rounds R] [--chunk RAYS] [--size 800] [--routes march,packed,...] [--out FILE]
(--routes march under `rocprofv3 --kernel-trace --stats` splits the marching into its two kernels.)
Prints one line per (occupancy, route): median, minimum and maximum ms per frame, and the samples kept."""
import argparse
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "nerf-experiments_amd")]

import torch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--chunk", type=int, default=4096)
ap.add_argument("--size", type=int, default=800)
ap.add_argument("--samples", type=int, default=256)
ap.add_argument("--routes", default="march,packed,batched,composite", help="comma-separated subset of the routes")
ap.add_argument("--out", default=None)
args = ap.parse_args()

import nerf_amd  # noqa: E402,F401
from nerf_amd import OccGridEstimator, RadianceNetwork  # noqa: E402
from nerf_amd import kernels as K  # noqa: E402
from nerf_amd.prop_sampler import rendering  # noqa: E402

if not torch.cuda.is_available():
    raise SystemExit("occgrid_bench: needs a GPU (there is no CPU path to time)")
dev = torch.device("cuda", 0)
torch.manual_seed(0)
model = RadianceNetwork(0.5, 2.0).to(dev)
NEAR, FAR, S = 2.0, 6.0, args.samples
DT = (FAR - NEAR) / S
H = W = args.size
lines = []


def emit(s):
    print(s, flush=True)
    lines.append(s)


def frame_rays():
    j, i = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    focal = 1111.0 * W / 800
    d = torch.stack([(i - W / 2 + 0.5) / focal, -(j - H / 2 + 0.5) / focal, -torch.ones_like(i)], -1).reshape(-1, 3)
    d = torch.nn.functional.normalize(d, dim=-1)
    o = torch.tensor([0.0, 0.0, 4.0]).expand_as(d).contiguous()
    return o.to(dev), d.to(dev)


def ball_grid(fraction):
    """Estimator whose occupied cells are those with their centre in a centred ball holding `fraction`
    of the cells (1.0: all of them)."""
    est = OccGridEstimator([-1.5] * 3 + [1.5] * 3, resolution=128).to(dev)
    c = (torch.arange(128, device=dev, dtype=torch.float32) + 0.5) / 128 * 3.0 - 1.5
    r2 = c[:, None, None] ** 2 + c[None, :, None] ** 2 + c[None, None, :] ** 2
    if fraction >= 1.0:
        est.binaries.fill_(True)
    else:
        radius = (fraction * 27.0 * 3 / (4 * math.pi)) ** (1 / 3)
        est.binaries.copy_((r2 < radius * radius)[None])
    return est, float(est.binaries.float().mean())


rays_o, rays_d = frame_rays()
n_rays = rays_o.shape[0]


def march_only(est):
    return est.sampling(rays_o, rays_d, near_plane=NEAR, far_plane=FAR, render_step_size=DT)[0].numel()


@torch.no_grad()
def packed_frame(est):
    out = torch.empty(n_rays, 3, device=dev)
    kept = 0
    for a in range(0, n_rays, args.chunk):
        o, d = rays_o[a:a + args.chunk], rays_d[a:a + args.chunk]
        ri, t0, t1 = est.sampling(o, d, near_plane=NEAR, far_plane=FAR, render_step_size=DT)
        kept += ri.numel()

        def field(ts, te, idx):
            if ts.numel() == 0:
                return ts.new_zeros(0, 3), ts.new_zeros(0)
            dirs = d[idx]
            rgb, sigma = model(o[idx] + dirs * ((ts + te) * 0.5)[:, None], dirs)
            return rgb, sigma.reshape(-1)
        out[a:a + args.chunk] = rendering(t0, t1, ri, o.shape[0], field)[0]
    return kept


t_edges = NEAR + DT * torch.arange(S + 1, device=dev, dtype=torch.float32)


@torch.no_grad()
def batched_frame(_est=None):
    out = torch.empty(n_rays, 3, device=dev)
    for a in range(0, n_rays, args.chunk):
        o, d = rays_o[a:a + args.chunk], rays_d[a:a + args.chunk]
        B = o.shape[0]
        t0, t1 = t_edges[:-1].expand(B, S).contiguous(), t_edges[1:].expand(B, S).contiguous()

        def field(ts, te, _):
            pos = o[:, None, :] + d[:, None, :] * ((ts + te) * 0.5)[..., None]
            rgb, sigma = model(pos.reshape(-1, 3), d[:, None, :].expand(B, S, 3).reshape(-1, 3))
            return rgb.reshape(B, S, 3), sigma.reshape(B, S)
        out[a:a + args.chunk] = rendering(t0, t1, rgb_sigma_fn=field)[0]
    return n_rays * S


def composite_launch():
    """One nerf_composite_fwd launch over the whole batched lattice."""
    g = torch.Generator(device=dev).manual_seed(1)
    sigma = torch.rand(n_rays, S, device=dev, generator=g)
    rgb = torch.rand(n_rays, S, 3, device=dev, generator=g)
    dist = torch.full((n_rays, S), DT, device=dev)

    def launch(_est=None):
        K.composite_fwd(sigma, 1, rgb, 3, dist, n_rays, S, 1.0, 1.0, False)
        return n_rays * S
    return launch


def timed(fn, est):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    n = fn(est)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e), n


emit(f"occgrid_bench: {H} x {W} rays, near/far {NEAR}/{FAR}, step {DT:.6f} ({S} per full chord), chunk {args.chunk} rays, "
     f"{args.rounds} rounds")
routes = {"march": march_only, "packed": packed_frame, "batched": batched_frame}
if "composite" in args.routes.split(","):
    routes["composite_fwd launch"] = composite_launch()
routes = {r: fn for r, fn in routes.items() if r.split("_")[0] in args.routes.split(",")}
grids = [ball_grid(f) for f in (1.0, 0.25, 0.05)]
for est, frac in grids:
    for fn in routes.values():
        fn(est)                                 # warm-up of every route and shape
torch.cuda.synchronize()
ms = {(gi, r): [] for gi in range(len(grids)) for r in routes}
kept = {}
for _ in range(args.rounds):
    for gi, (est, frac) in enumerate(grids):
        for r, fn in routes.items():
            t, n = timed(fn, est)
            ms[(gi, r)].append(t)
            kept[(gi, r)] = n
for gi, (est, frac) in enumerate(grids):
    for r in routes:
        v = ms[(gi, r)]
        emit(f"cells set {100 * frac:5.1f} %  {r:22s} median {statistics.median(v):10.3f} ms  (min {min(v):.3f}, max "
             f"{max(v):.3f})  samples {kept[(gi, r)]:>11d}")
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
