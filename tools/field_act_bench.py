"""Forward + backward time of the radiance network of the three field families (GARF, GaborF,
SARF) at the GARF benchmark's radiance batch (4096 rays x 192 samples), with the activation in
the GEMM epilogues and as separate passes: HIP events, warm-up, >= 20 repetitions.
Usage: python tools/field_act_bench.py [--iters N] [--M rows] [--precision high|highest]
Prints one line per (family, route): ms per forward + backward, and the ratio to GARF's fused route."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "nerf-experiments_amd")]

import torch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--M", type=int, default=4096 * 192)
ap.add_argument("--precision", default="high", choices=("highest", "high"))
args = ap.parse_args()

import nerf_amd  # noqa: E402,F401
from nerf_amd import mlp as mlp_mod  # noqa: E402
from nerf_amd import model_gaborf, model_garf, model_sarf  # noqa: E402

torch.set_float32_matmul_precision(args.precision)
dev = torch.device("cuda", 0)
g = torch.Generator().manual_seed(0)
M = args.M
pos = (torch.rand(M, 3, generator=g) * 4 - 2).to(dev)
dirs = torch.nn.functional.normalize(torch.randn(M, 3, generator=g), dim=1).to(dev)
gc = torch.randn(M, 3, generator=g).to(dev)
gd = torch.randn(M, generator=g).to(dev)

# the families' main.py init ranges
FAMILIES = (("garf", model_garf, (0.5, 2.0)), ("gaborf", model_gaborf, (0.0, 2.0)), ("sarf", model_sarf, (0.5, 2.0)))


def step(m):
    for p in m.parameters():
        p.grad = None
    rgb, dens = m(pos, dirs)
    ((rgb * gc).sum() + (dens * gd).sum()).backward()


base = None
for name, mod, init in FAMILIES:
    for fused in (True, False):
        mlp_mod.GAUSS_EPILOGUE = fused
        torch.manual_seed(0)
        m = mod.RadianceNetwork(*init).to(dev)
        for _ in range(args.warmup):
            step(m)
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(args.iters):
            step(m)
        e.record()
        torch.cuda.synchronize()
        ms = s.elapsed_time(e) / args.iters
        base = ms if base is None else base
        print(f"{name:7s} {'epilogue' if fused else 'separate'}  M={M}  {args.precision}: {ms:8.3f} ms fwd+bwd  "
              f"({ms / base:.3f} x GARF epilogue)", flush=True)
        del m
mlp_mod.GAUSS_EPILOGUE = True
