"""The cascaded occupancy-grid marching on one 800 x 800 frame, the marching alone (sampling without a
field), alternating on one card:

  one-level      OccGridEstimator.sampling (nerf_occ_march_count / _write), tools/occgrid_bench.py's frame:
                 camera at (0, 0, 4), near / far 2 / 6, a 128^3 grid over [-1.5, 1.5]^3 with a centred
                 ball holding 25 % of the cells, render_step_size (6 - 2) / 256;
  cascade L1     CascadedOccGridEstimator(levels=1).sampling on the same grid, cone_angle 0: the same
                 samples bit for bit (checked), so the difference is the price of the general kernel;
  cascade L4 ... levels=4 (boxes up to [-12, 12]^3), the ball on level 0 and, as a stand-in for the
                 ground of an unbounded scene, every cell with its centre below y = 0 on levels 1-3,
                 far 16, at cone_angle 0 and 0.004 (nerfacc's setting for mip-NeRF 360 scenes).

HIP events around each whole call (count kernel, cumsum, the one host synchronisation, write kernel)
after a warm-up of every route; --rounds rounds visit the routes in turn.
Usage: python tools/occgrid_cascade_bench.py [--rounds R] [--size 800] [--out FILE]
Prints one line per route: median, minimum and maximum ms per frame, and the samples kept."""
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
ap.add_argument("--size", type=int, default=800)
ap.add_argument("--out", default=None)
args = ap.parse_args()

import nerf_amd  # noqa: E402,F401
from nerf_amd import CascadedOccGridEstimator, OccGridEstimator  # noqa: E402

if not torch.cuda.is_available():
    raise SystemExit("occgrid_cascade_bench: needs a GPU (there is no CPU path to time)")
dev = torch.device("cuda", 0)
NEAR, FAR, FAR_OUT = 2.0, 6.0, 16.0
DT = (FAR - NEAR) / 256
ROI = [-1.5] * 3 + [1.5] * 3
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


def centres(level):
    return ((torch.arange(128, device=dev, dtype=torch.float32) + 0.5) / 128 * 3.0 - 1.5) * 2.0 ** level


def ball():
    c = centres(0)
    radius = (0.25 * 27.0 * 3 / (4 * math.pi)) ** (1 / 3)
    return c[:, None, None] ** 2 + c[None, :, None] ** 2 + c[None, None, :] ** 2 < radius * radius


rays_o, rays_d = frame_rays()
one = OccGridEstimator(ROI, resolution=128).to(dev)
one.binaries.copy_(ball()[None])
l1 = CascadedOccGridEstimator(ROI, resolution=128, levels=1).to(dev)
l1.binaries.copy_(ball()[None])
l4 = CascadedOccGridEstimator(ROI, resolution=128, levels=4).to(dev)
l4.binaries[0] = ball()
for level in (1, 2, 3):
    l4.binaries[level] = (centres(level) < 0)[None, :, None].expand(128, 128, 128)


def route(est, far, **kw):
    return lambda: est.sampling(rays_o, rays_d, near_plane=NEAR, far_plane=far, render_step_size=DT, **kw)


routes = {
    "one-level (far 6)": route(one, FAR),
    "cascade L1 cone 0 (far 6)": route(l1, FAR),
    "cascade L4 cone 0 (far 6)": route(l4, FAR),
    "cascade L4 cone 0 (far 16)": route(l4, FAR_OUT),
    "cascade L4 cone 0.004 (far 16)": route(l4, FAR_OUT, cone_angle=0.004),
}


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    n = fn()[0].numel()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e), n


emit(f"occgrid_cascade_bench: {H} x {W} rays, near {NEAR}, step {DT:.6f}, 128^3 cells per level, {args.rounds} rounds")
a, b = routes["one-level (far 6)"](), routes["cascade L1 cone 0 (far 6)"]()
identical = all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                            y.view(torch.int32) if y.dtype == torch.float32 else y) for x, y in zip(a, b))
emit(f"cascade L1 cone 0 against the one-level kernels: {'identical' if identical else 'DIFFERENT'} samples")
del a, b
for fn in routes.values():
    fn()                                        # warm-up of every route and shape
torch.cuda.synchronize()
ms = {r: [] for r in routes}
kept = {}
for _ in range(args.rounds):
    for r, fn in routes.items():
        t, kept[r] = timed(fn)
        ms[r].append(t)
for r, v in ms.items():
    emit(f"{r:32s} median {statistics.median(v):9.3f} ms  (min {min(v):.3f}, max {max(v):.3f})  samples {kept[r]:>11d}")
status = int(l4.status().item()) | int(l1.status().item())
emit(f"status words: {status}")
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
if not identical:
    raise SystemExit("occgrid_cascade_bench: the general kernel's one-level samples differ")
