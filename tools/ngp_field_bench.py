"""The NGP radiance field behind the occupancy grid, timed.

(a) The two kernel pairs of csrc/ngp_field.hip against their eager torch forms (tests/_ngp_field_ref.py:
    the same formulas as tensor ops) at n = 2^20, forward + backward with random output gradients: SH
    degree 4 on unit directions, and the position map in both modes on points a third inside the box, a
    third with 1 < m < 4, the rest with m up to 1e6.  Also the four kernels by themselves (HIP events
    around each launch) with the algorithmic bytes nerf_amd.kernels counts, as a fraction of the 8 TB/s
    HBM peak.
(b) One training step (forward + backward, mean squared colour against a fixed random target) of
    OccGridRenderer on 4096 rays of tools/occtrain_bench.py's scene (camera at (0, 0, 4), near / far
    2 / 6, a 128^3 grid over [-1.5, 1.5]^3 with 100 %, 25 % and 5 % of the cells set, no visibility
    filter): NGPRadianceField with a 2^16 and with a 2^19 table, and the GARF RadianceNetwork that
    tools/occtrain_bench.py times, in the same run.

HIP events around each step after a warm-up of every route and shape; --rounds rounds visit the routes in
turn, so the spread across rounds is visible next to the differences.  Medians are printed.
Usage: python tools/ngp_field_bench.py [--rounds R] [--rays 4096] [--out FILE]"""
import argparse
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "nerf-experiments_amd"), os.path.join(ROOT, "tests")]

import torch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--rays", type=int, default=4096)
ap.add_argument("--samples", type=int, default=256)
ap.add_argument("--n", type=int, default=2 ** 20)
ap.add_argument("--out", default=None)
args = ap.parse_args()

import nerf_amd  # noqa: E402,F401
import _ngp_field_ref as REF  # noqa: E402
from nerf_amd import (NGPRadianceField, OccGridEstimator, OccGridRenderer, RadianceNetwork, SHEncoding,  # noqa: E402
                      contract_to_unisphere, normalize_to_aabb)
from nerf_amd import kernels as K  # noqa: E402

if not torch.cuda.is_available():
    raise SystemExit("ngp_field_bench: needs a GPU (there is no CPU path to time)")
dev = torch.device("cuda", 0)
torch.manual_seed(0)
NEAR, FAR, S = 2.0, 6.0, args.samples
DT = (FAR - NEAR) / S
HBM_PEAK = 8.0e12
lines = []


def emit(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn, *a):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    n = fn(*a)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e), n


# ----------------------------------------------------------------------------- (a) the kernel pairs
n = args.n
dirs = torch.from_numpy(REF.unit_dirs(n)).to(dev).requires_grad_(True)
pts_np, box_np = REF.field_points(n)
pts = torch.from_numpy(pts_np).to(dev).requires_grad_(True)
box_t = torch.from_numpy(box_np).to(dev)
box_l = [float(v) for v in box_np]
gen = torch.Generator(device=dev).manual_seed(2)
g_sh = torch.randn(n, 32, device=dev, generator=gen)
g_sh16 = g_sh[:, :16].contiguous()               # the eager form's own [n, 16] gradient: no copy inside its figure
g_u = torch.randn(n, 3, device=dev, generator=gen)
sh = SHEncoding(4)


def pair(x, fn, g):
    def run():
        x.grad = None
        fn(x).backward(g)
        return n
    return run


# bytes: nerf_amd.kernels' counts (SH 12 + 64 forward, 24 + 64 backward; position map 28 forward, 36 backward)
pairs = [
    ("SH hip", 164 * n, pair(dirs, sh.encode_padded, g_sh)),
    ("SH eager", 164 * n, pair(dirs, lambda d: REF.sh_torch(d, 4), g_sh16)),
    ("box map hip", 64 * n, pair(pts, lambda x: normalize_to_aabb(x, box_l)[0], g_u)),
    ("box map eager", 64 * n, pair(pts, lambda x: REF.unit_cube_torch(x, box_t, 0)[0], g_u)),
    ("contraction hip", 64 * n, pair(pts, lambda x: contract_to_unisphere(x, box_l)[0], g_u)),
    ("contraction eager", 64 * n, pair(pts, lambda x: REF.unit_cube_torch(x, box_t, 1)[0], g_u)),
]


# ----------------------------------------------------------------------------- (b) the training step
def batch_rays(m):
    H = W = 800
    g = torch.Generator().manual_seed(1)
    pix = torch.randint(H * W, (m,), generator=g)
    j, i = (pix // W).float(), (pix % W).float()
    d = torch.stack([(i - W / 2 + 0.5) / 1111.0, -(j - H / 2 + 0.5) / 1111.0, -torch.ones_like(i)], -1)
    d = torch.nn.functional.normalize(d, dim=-1)
    o = torch.tensor([0.0, 0.0, 4.0]).expand_as(d).contiguous()
    return o.to(dev), d.to(dev), torch.rand(m, 3, generator=g).to(dev)


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


R = args.rays
rays_o, rays_d, target = batch_rays(R)
fields = {
    "NGP T=2^16": NGPRadianceField([-1.5] * 3 + [1.5] * 3, log2_hashmap_size=16).to(dev),
    "NGP T=2^19": NGPRadianceField([-1.5] * 3 + [1.5] * 3, log2_hashmap_size=19).to(dev),
    "GARF": RadianceNetwork(0.5, 2.0).to(dev),
}


def step(field, ren):
    field.zero_grad(set_to_none=True)
    rgb, _, _, ex = ren(rays_o, rays_d, stratified=False)
    ((rgb - target) ** 2).mean().backward()
    return ex["ray_indices"].numel()


emit(f"ngp_field_bench: matmul precision {torch.get_float32_matmul_precision()!r}, {args.rounds} rounds")
grids = []
for f in (1.0, 0.25, 0.05):
    est, frac = ball_grid(f)
    rens = {name: OccGridRenderer(fld, est, NEAR, FAR, DT, early_stop_eps=0.0).to(dev) for name, fld in fields.items()}
    grids.append((frac, rens))
for _, _, fn in pairs:
    fn()
for frac, rens in grids:
    for name, ren in rens.items():
        step(fields[name], ren)
torch.cuda.synchronize()
ms, kept = {}, {}
for _ in range(args.rounds):
    for name, _, fn in pairs:
        ms.setdefault(name, []).append(timed(fn)[0])
    for gi, (frac, rens) in enumerate(grids):
        for name, ren in rens.items():
            t, m = timed(step, fields[name], ren)
            ms.setdefault((gi, name), []).append(t)
            kept[(gi, name)] = m
for name, nbytes, _ in pairs:
    v = ms[name]
    med = statistics.median(v)
    emit(f"pair {name:18s} fwd + bwd  median {med * 1e3:9.1f} us  (min {min(v) * 1e3:.1f}, max {max(v) * 1e3:.1f})  "
         f"n {n}  {nbytes / 1e6:8.2f} MB  {nbytes / (med * 1e-3) / HBM_PEAK * 100:5.1f} % of HBM peak")
K.TIMER = K.KernelTimer()
for _ in range(5):
    for name, _, fn in pairs:
        if name.endswith("hip"):
            fn()
for fn_name, d in K.TIMER.summary(by="fn").items():
    us, nbytes = d["ms"] * 1e3 / d["launches"], d["bytes"] / d["launches"]
    emit(f"kernel {fn_name:24s} mean {us:8.1f} us over {d['launches']} launches  n {n}  {nbytes / 1e6:8.2f} MB  "
         f"{nbytes / (us * 1e-6) / HBM_PEAK * 100:5.1f} % of HBM peak")
K.TIMER = None
emit(f"training step: {R} rays, near/far {NEAR}/{FAR}, step {DT:.6f}, 128^3 grid, forward + backward")
for gi, (frac, rens) in enumerate(grids):
    for name in rens:
        v = ms[(gi, name)]
        emit(f"cells set {100 * frac:5.1f} %  field {name:11s} median {statistics.median(v):9.3f} ms  (min {min(v):.3f}, "
             f"max {max(v):.3f})  samples {kept[(gi, name)]:>9d}")
# where the NGP step's time goes at the full grid: the launches nerf_amd.kernels brackets
for name in ("NGP T=2^16", "NGP T=2^19"):
    K.TIMER = K.KernelTimer()
    step(fields[name], grids[0][1][name])
    rows = sorted(K.TIMER.summary(by="fn").items(), key=lambda kv: -kv[1]["ms"])
    K.TIMER = None
    total = sum(d["ms"] for _, d in rows)
    emit(f"{name}, 100 % grid: {total:.3f} ms inside bracketed launches; the largest:")
    for fn_name, d in rows[:8]:
        emit(f"    {fn_name:32s} {d['ms']:8.3f} ms  {d['launches']:3d} launches")
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
