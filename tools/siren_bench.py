"""Forward + backward time of the SIREN field network NerfModel(32) (nerf_amd/model_siren.py) at the
reference's training load (nerf-siren/main.py:26,71-72: 2048 rays x 64 coarse samples and x 256 =
64 + 192 fine samples) on three routes, alternating on one card:
  epilogue   the sine in the split-precision GEMM epilogues (nerf_linear_sine_x3), forward and backward
  separate   the same GEMMs with nerf_sine_act_fwd / _bwd as separate passes
  eager      a torch restatement of the reference's modules (F.linear + th.sin, th.cat) on the same weights
HIP events around `--iters` steps, after warm-up of every route and shape; `--rounds` rounds that visit
the routes in turn, so the spread across rounds is visible next to the difference between routes.
Usage: python tools/siren_bench.py [--iters N] [--rounds R] [--rays B] [--precision high|highest]
Prints one line per (samples per ray, route): median, minimum and maximum ms per forward + backward."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "nerf-experiments_amd")]

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--rays", type=int, default=2048)
ap.add_argument("--precision", default="high", choices=("highest", "high"))
args = ap.parse_args()

import nerf_amd  # noqa: E402,F401
from nerf_amd import mlp as mlp_mod  # noqa: E402
from nerf_amd import model_siren  # noqa: E402

if not torch.cuda.is_available():
    raise SystemExit("siren_bench: needs a GPU (there is no CPU path to time)")
torch.set_float32_matmul_precision(args.precision)
dev = torch.device("cuda", 0)
torch.manual_seed(0)
model = model_siren.NerfModel(32).to(dev)


def eager(pos, d):
    """The reference's forward (nerf-siren/nerf_model.py:58-74) on this model's parameters."""
    def seq(mods, x):
        for m in mods:
            x = torch.sin(F.linear(m.scale * x, m.linear.weight, m.linear.bias)) \
                if isinstance(m, model_siren.LinearSine) else F.linear(x, m.weight, m.bias)
        return x
    z = seq(model.model_density_1, pos)
    z = seq(model.model_density_2, torch.cat((z, pos), dim=1))
    density = F.softplus(z[:, 259] - 1, threshold=8)
    rgb = torch.sigmoid(z[:, 256:259] + seq(model.model_color, torch.cat((z[:, :256], d), dim=1)))
    return density, rgb


def make_step(route, M):
    g = torch.Generator().manual_seed(1)
    pos = (torch.rand(M, 3, generator=g) * 2 - 1).to(dev)
    d = F.normalize(torch.randn(M, 3, generator=g), dim=1).to(dev)
    w = torch.linspace(0.5, 1.5, M).to(dev)

    def step():
        for p in model.parameters():
            p.grad = None
        mlp_mod.GAUSS_EPILOGUE = route == "epilogue"
        density, rgb = eager(pos, d) if route == "eager" else model(pos, d)
        (w * (density + rgb.sum(dim=1))).sum().backward()
    return step


def timed(step):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(args.iters):
        step()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / args.iters


ROUTES = ("epilogue", "separate", "eager")
try:
    for S in (64, 256):
        M = args.rays * S
        steps = {r: make_step(r, M) for r in ROUTES}
        for r in ROUTES:
            for _ in range(args.warmup):
                steps[r]()
        torch.cuda.synchronize()
        ms = {r: [] for r in ROUTES}
        for _ in range(args.rounds):
            for r in ROUTES:
                ms[r].append(timed(steps[r]))
        for r in ROUTES:
            print(f"NerfModel(32) {r:9s} M = {args.rays} x {S:3d} = {M:7d}  {args.precision}: "
                  f"median {statistics.median(ms[r]):8.3f} ms fwd+bwd  (min {min(ms[r]):.3f}, max {max(ms[r]):.3f}, "
                  f"{args.rounds} rounds x {args.iters} steps)", flush=True)
finally:
    mlp_mod.GAUSS_EPILOGUE = True
