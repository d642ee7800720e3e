"""Child process of tests/test_gpu_hashgrid_edges.py::test_non_default_switches: the library reads its
NERF_HG_* switches once per process, so each setting gets a fresh interpreter.  Runs the forward and
the table gradient (minimal and full workspace) of configs A, B, C and G at n = 65, 257 and 4097 on
the inputs of tests/_hashgrid3d_ref.py and saves the results to the .npz file named by argv[1]; the
parent compares them with the CPU restatement."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "nerf-experiments_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _hashgrid3d_ref as R  # noqa: E402
from nerf_amd import kernels as K  # noqa: E402
from oracle import hashgrid_oracle as O  # noqa: E402

TAGS = ("A", "B", "C", "G")
NS = (65, 257, 4097)


def main(path: str) -> None:
    dev = torch.device("cuda", 0)
    out = {}
    for tag in TAGS:
        res, T, F, primes, normalize = R.cfg_args(tag)
        L = len(res)
        p = K.make_hashgrid_params(L, T, F, res, primes=primes, normalize=normalize)
        table = torch.from_numpy(O.pack(R.tables(tag))).to(dev)
        rows = K.hashgrid_table_rows(p)
        for n in NS:
            x = torch.from_numpy(R.points(tag, n)).to(dev)
            g = torch.from_numpy(R.grads(tag, n, wide=True)).to(dev)
            feat = torch.full((n, L * F), float("nan"), device=dev)
            K.hashgrid_fwd(p, table, feat, x=x, n_samples=n)
            out[f"{tag}.{n}.fwd"] = feat.cpu().numpy()
            for name, nbytes in (("min", K.hashgrid_workspace_bytes(p)), ("full", K.hashgrid_workspace_bytes(p, n))):
                ws = torch.full(((nbytes + 7) // 8,), -3, dtype=torch.int64, device=dev)
                gt = torch.full((rows, F), float("nan"), device=dev)
                K.hashgrid_bwd(p, g, gt, ws, x=x, n_samples=n)
                out[f"{tag}.{n}.bwd_{name}"] = gt.cpu().numpy()
    torch.cuda.synchronize()
    np.savez(path, **out)


if __name__ == "__main__":
    main(sys.argv[1])
