"""Times the register-staged weight-gradient kernel (linear_wgrad_x3_tr_kernel) alone at the mip
bench's merged row count (M = 786432: coarse + fine rows of 4096 rays) for the trunk's shapes, with
HIP events on the stream the kernel runs on.  Pick the library with NERF_AMD_LIB (diagnostic
NERF_WT_DIAG_* builds need NERF_ALLOW_DIAG_BUILD=1).  Prints one JSON line.
With --quad every shape is also timed on the quad-split image of the same X (x_split_mask = 1),
fp32 and quad-split alternating twice (K<k>_f32_us, K<k>_quad_us, then the *b repeats): the
256-column figures drift within a process, so only figures in the same position compare.
Usage: python tools/wgrad_tr_diag.py [M] [--quad]"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "nerf-experiments_amd"))
from nerf_amd import kernels as K  # noqa: E402

QUAD = "--quad" in sys.argv
_args = [a for a in sys.argv[1:] if a != "--quad"]
M = int(_args[0]) if _args else 786432
dev = torch.device("cuda:0")
out = {"lib": os.path.basename(os.environ.get("NERF_AMD_LIB", "libnerf_amd.so")), "M": M}
dY = torch.randn(M, 256, device=dev)
for kd in (() if QUAD else (256, 96, 32)):
    X = torch.randn(M, kd, device=dev)
    ws = torch.empty((K.linear_wgrad_workspace_bytes(M, 256, kd) + 3) // 4, device=dev)
    for _ in range(3):
        K.linear_wgrad_x3(dY, 256, [(X, kd, 1)], M, ws)
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = 20
    s.record()
    for _ in range(n):
        K.linear_wgrad_x3(dY, 256, [(X, kd, 1)], M, ws)
    e.record()
    torch.cuda.synchronize()
    us = s.elapsed_time(e) * 1e3 / n
    out[f"K{kd}_us"] = round(us, 1)
    out[f"K{kd}_TBps"] = round(M * 4 * (256 + kd) / us / 1e6, 3)
    del X, ws
if QUAD:
    for kd in (256, 96):
        X = torch.randn(M, kd, device=dev).relu()
        Xq = K.quad_split_pack(X)
        ws = torch.empty((K.linear_wgrad_workspace_bytes(M, 256, kd) + 3) // 4, device=dev)
        for tag, x, mask in (("f32", X, 0), ("quad", Xq, 1), ("f32b", X, 0), ("quadb", Xq, 1)):
            for _ in range(3):
                K.linear_wgrad_x3(dY, 256, [(x, kd, 1)], M, ws, x_split_mask=mask)
            torch.cuda.synchronize()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(20):
                K.linear_wgrad_x3(dY, 256, [(x, kd, 1)], M, ws, x_split_mask=mask)
            e.record()
            torch.cuda.synchronize()
            out[f"K{kd}_{tag}_us"] = round(s.elapsed_time(e) * 1e3 / 20, 1)
        del X, Xq, ws
print(json.dumps(out))
