"""Restatements of the 2-D hash-grid image fit that the tests and tools/ingp2d_bench.py run against
(test infrastructure only; no kernels):

* ``encode`` — numpy: oracle/hashgrid_oracle.py::encode_2d with selectable primes and the domain
  rule of nerf_hashgrid2d_fwd (a bijective-level corner outside [0, r]^2 is dropped and flagged);
  on points of [0, 1)^2 with the default primes it is encode_2d (tests/test_ingp2d_logic.py).
* ``table_grad_fixed`` — numpy int64: the fixed-point table gradient of nerf_hashgrid2d_bwd, rule by
  rule as include/nerf_amd.h states it, bit for bit.  ``table_grad_f64``: the same gradient as a
  plain fp64 scatter.
* ``RefGigapixel`` — torch: the module's forward in eager tensor ops (per level: scale, floor, the
  four corners stacked, int64 rows, gather, weights, sum over the stacked corners), with the state_dict
  layout of nerf_amd.model_ingp2d.Gigapixel; bitwise the fixture's features on the CPU.
"""
from __future__ import annotations

import math

import numpy as np
import torch as th
import torch.nn as nn

PRIMES = (1, 2654435761)
CORNERS = ((0, 0), (0, 1), (1, 0), (1, 1))


def schedule(resolution_max: int, resolution_min: int, n_levels: int) -> list[int]:
    """The levels' resolutions in the reference's fp32 tensor arithmetic (main.py's (2048, 16, 16)
    ends at 2047)."""
    b = 1 if n_levels == 1 else math.exp((math.log(resolution_max) - math.log(resolution_min)) / (n_levels - 1))
    return [int(r) for r in th.floor(resolution_min * b ** th.arange(n_levels))]


def level_rows(r: int, table_size: int) -> int:
    return (r + 1) ** 2 if (r + 1) ** 2 <= table_size else table_size


def level_corners(x: np.ndarray, r: int, table_size: int, primes=PRIMES):
    """(rows [N, 4] int64, weights [N, 4] fp32, in-domain mask [N, 4]) of one level."""
    xh = x.astype(np.float32) * np.float32(r)
    with np.errstate(invalid="ignore"):
        base = np.floor(xh).astype(np.int64)
    idx = np.zeros((x.shape[0], 4), dtype=np.int64)
    w = np.empty((x.shape[0], 4), dtype=np.float32)
    ok = np.ones((x.shape[0], 4), dtype=bool)
    bij = (r + 1) ** 2 <= table_size
    for k, (i, j) in enumerate(CORNERS):
        c = base + np.array([i, j], dtype=np.int64)
        d = np.float32(1.0) - np.abs(xh - c.astype(np.float32))
        w[:, k] = d[:, 0] * d[:, 1]
        if bij:
            ok[:, k] = (c[:, 0] >= 0) & (c[:, 0] <= r) & (c[:, 1] >= 0) & (c[:, 1] <= r) & np.isfinite(xh).all(axis=1)
            idx[:, k] = np.where(ok[:, k], c[:, 0] + (r + 1) * c[:, 1], 0)
        else:
            with np.errstate(over="ignore"):
                h = (c[:, 0] * np.array(primes[0]).astype(np.int64)) ^ (c[:, 1] * np.array(primes[1]).astype(np.int64))
            idx[:, k] = np.mod(h, np.int64(table_size))
    return idx, w, ok


def encode(x: np.ndarray, tables, res, table_size: int, primes=PRIMES):
    """(features [N, L * F] fp32, status): per level the in-domain corners' w * row, products rounded,
    added in corner order from 0; status bit 0 = some corner was dropped."""
    outs, status = [], 0
    for t, r in zip(tables, res):
        idx, w, ok = level_corners(x, int(r), table_size, primes)
        acc = np.zeros((x.shape[0], t.shape[1]), dtype=np.float32)
        for k in range(4):
            term = acc + t[idx[:, k]] * w[:, k:k + 1]
            acc = np.where(ok[:, k:k + 1], term, acc)
        status |= int(not ok.all())
        outs.append(acc)
    return np.concatenate(outs, axis=1), status


def fixed_shift(gmax: float, n: int):
    """The exponent s of the fixed-point grid (None: non-finite gradient)."""
    if not np.isfinite(gmax):
        return None
    if gmax == 0:
        return 60
    _, e = math.frexp(4.0 * float(n) * float(gmax))
    return min(62 - e, 120)


def table_grad_fixed(x: np.ndarray, g: np.ndarray, res, table_size: int, n_features: int, primes=PRIMES) -> np.ndarray:
    """Packed [sum rows, F] fp32 table gradient of sum(encode(x) * g), g [N, >= L * F]."""
    F, n = n_features, x.shape[0]
    rows = [level_rows(int(r), table_size) for r in res]
    g = g[:, :len(res) * F].astype(np.float32)
    s = fixed_shift(float(np.abs(g).max()) if g.size else 0.0, n)
    if s is None:
        return np.full((sum(rows), F), np.nan, dtype=np.float32)
    scale = math.ldexp(1.0, s)
    out = []
    for l, r in enumerate(res):
        idx, w, ok = level_corners(x, int(r), table_size, primes)
        gs = g[:, l * F:(l + 1) * F].astype(np.float64) * scale
        acc = np.zeros((rows[l], F), dtype=np.int64)
        for k in range(4):
            q = np.rint(w[:, k:k + 1].astype(np.float64) * gs).astype(np.int64)
            m = ok[:, k]
            np.add.at(acc, idx[m, k], q[m])
        out.append((acc.astype(np.float64) * math.ldexp(1.0, -s)).astype(np.float32))
    return np.concatenate(out, axis=0)


def table_grad_f64(x: np.ndarray, g: np.ndarray, res, table_size: int, n_features: int, primes=PRIMES) -> np.ndarray:
    F = n_features
    out = []
    for l, r in enumerate(res):
        idx, w, ok = level_corners(x, int(r), table_size, primes)
        acc = np.zeros((level_rows(int(r), table_size), F), dtype=np.float64)
        for k in range(4):
            m = ok[:, k]
            np.add.at(acc, idx[m, k], (w[:, k:k + 1].astype(np.float64) * g[:, l * F:(l + 1) * F].astype(np.float64))[m])
        out.append(acc)
    return np.concatenate(out, axis=0)


# ----------------------------------------------------------------------------- torch restatement
class RefTable(nn.Module):
    def __init__(self, resolution: int, table_size: int, n_features: int, pi1: int, pi2: int):
        super().__init__()
        self.resolution, self.table_size, self.pi1, self.pi2 = int(resolution), table_size, pi1, pi2
        self.bijective = (self.resolution + 1) ** 2 <= table_size
        self.table = nn.Parameter(th.zeros(level_rows(self.resolution, table_size), n_features))

    def forward(self, x: th.Tensor) -> th.Tensor:
        scaled = x * self.resolution
        lo = th.floor(scaled)
        ends = th.stack((lo, lo + 1), dim=1)                                          # [N, 2 (lo / hi), 2 (dim)]
        dims = th.arange(2, device=x.device)
        corners = th.stack([ends[:, [i, j], dims] for i, j in CORNERS], dim=1).to(th.int64)   # [N, 4, 2]
        if self.bijective:
            rows = corners[..., 0] + (self.resolution + 1) * corners[..., 1]
        else:
            rows = th.remainder(th.bitwise_xor(self.pi1 * corners[..., 0], self.pi2 * corners[..., 1]), self.table_size)
        weights = th.prod(1 - th.abs(scaled.unsqueeze(1) - corners), dim=-1)
        return th.sum(self.table[rows] * weights.unsqueeze(-1), dim=1)


class RefEncoding(nn.Module):
    def __init__(self, resolutions, table_size: int, n_features: int, pi1: int = PRIMES[0], pi2: int = PRIMES[1]):
        super().__init__()
        self.output_dim = n_features * len(resolutions)
        self.encodings = nn.ModuleList([RefTable(int(r), table_size, n_features, pi1, pi2) for r in resolutions])

    def forward(self, x: th.Tensor) -> th.Tensor:
        return th.cat([e(x) for e in self.encodings], dim=1)


class RefGigapixel(nn.Module):
    """state_dict-compatible with nerf_amd.model_ingp2d.Gigapixel (load_state_dict to fill it)."""

    def __init__(self, n_hidden: int, hidden_dim: int, position_encoder: RefEncoding):
        super().__init__()
        self.position_encoder = position_encoder
        d = position_encoder.output_dim
        if n_hidden == 0:
            self.net = nn.Linear(d, 3)
        else:
            mods = [nn.Linear(d, hidden_dim)]
            for _ in range(n_hidden - 1):
                mods += [nn.ReLU(), nn.Linear(hidden_dim, hidden_dim)]
            self.net = nn.Sequential(*mods, nn.ReLU(), nn.Linear(hidden_dim, 3))

    def forward(self, pos: th.Tensor) -> th.Tensor:
        return th.sigmoid(self.net(self.position_encoder(pos)))


def fixture_model(golden: dict, tag: str, table_size: int, n_features: int, n_hidden: int, hidden_dim: int = 64):
    """RefGigapixel holding configuration ``tag``'s state of tests/golden/ingp2d.npz."""
    enc = RefEncoding([int(r) for r in golden[f"{tag}.res"]], table_size, n_features)
    model = RefGigapixel(n_hidden, hidden_dim, enc)
    model.load_state_dict({str(k): th.from_numpy(golden[f"{tag}.sd.{k}"]) for k in golden[f"{tag}.keys"]})
    return model
