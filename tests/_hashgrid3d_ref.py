"""CPU restatements for the 3-D hash-grid kernels (csrc/hashgrid.hip), built on
oracle/hashgrid_oracle.py: the fixed-point rule of nerf_hashgrid_bwd reproduced bit for bit
(include/nerf_amd.h states it), the ray form's fp32 positions, the position gradient in fp64 with an
elementwise error bound, and the case table shared by tests/test_hashgrid3d_logic.py (CPU) and
tests/test_gpu_hashgrid_edges.py (GPU).  Tables of at most 4 096 rows a level: every reference runs
in milliseconds."""
from __future__ import annotations

import math

import numpy as np

from oracle import hashgrid_oracle as O

U = 2.0 ** -24                      # fp32 unit roundoff

# tag: resolutions, table size, features, primes, normalize — and the path each one reaches
CONFIGS = {
    # one bijective level walked, three hashed ones bucketed (the SMALL field of the NGP tests)
    "A": dict(res=[4, 10, 25, 64], T=2 ** 10, F=2, primes=O.PRIMES, normalize=True),
    # a table size that is no power of two (64-bit remainder), F = 4 buckets, unnormalised points
    "B": dict(res=[7, 13, 40], T=1000, F=4, primes=(73856093, 19349663, 83492791), normalize=False),
    # non-monotone: hashed levels 0 and 2 stay with the walk, only the last is bucketed; F = 1
    "C": dict(res=[40, 3, 50, 5, 64], T=2 ** 9, F=1, primes=O.PRIMES, normalize=True),
    # F = 3: no restage, no buckets; 15 columns, so the scalar max kernel
    "D": dict(res=[5, 9, 17, 33, 65], T=2 ** 11, F=3, primes=O.PRIMES, normalize=True),
    # every level bijective: no bucket region
    "E": dict(res=[3, 5], T=2 ** 12, F=2, primes=O.PRIMES, normalize=True),
    # every level hashed: no walk launch, everything bucketed
    "G": dict(res=[32, 64, 128], T=2 ** 8, F=2, primes=O.PRIMES, normalize=True),
    # the most levels and features: 256 columns
    "H": dict(res=[2 + 3 * i for i in range(32)], T=2 ** 8, F=8, primes=O.PRIMES, normalize=True),
}
# 64: the restage tile; 256: the workgroup and the llrint -> rint_fixed switch; 4096: one slab -> two
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 4097]

EDGE_NORMALISED = np.array([[0, 0, 0], [4, 4, 4], [-4, -4, -4], [3.999999, -4, 0], [1e6, -1e6, 2], [-4.5, 0.25, 4.5]],
                           dtype=np.float32)
EDGE_UNIT = np.array([[0, 0, 0], [1 - 2.0 ** -24] * 3, [0.5, 0.5, 0.5]], dtype=np.float32)


def cfg_args(tag: str) -> tuple:
    """(res, T, F, primes, normalize) of a config, in the order the functions below take them."""
    c = CONFIGS[tag]
    return c["res"], c["T"], c["F"], c["primes"], c["normalize"]


def edge_rows(tag: str) -> np.ndarray:
    return EDGE_NORMALISED if CONFIGS[tag]["normalize"] else EDGE_UNIT


def points(tag: str, n: int, seed: int = 0) -> np.ndarray:
    """n seeded points: uniform in [-4.5, 4.5]^3 (clipped corners of bijective levels occur), or in
    [0, 1)^3 for the unnormalised config; the first rows are the edge rows, as far as n allows."""
    rng = np.random.default_rng([seed, n, ord(tag)])
    if CONFIGS[tag]["normalize"]:
        x = rng.uniform(-4.5, 4.5, size=(n, 3)).astype(np.float32)
    else:
        x = rng.random((n, 3), dtype=np.float32)
    e = edge_rows(tag)[:n]
    x[:e.shape[0]] = e
    return x


def tables(tag: str, seed: int = 0, scale: float = 0.5) -> list[np.ndarray]:
    res, T, F, _, _ = cfg_args(tag)
    rng = np.random.default_rng([seed, ord(tag), 1])
    return [(rng.standard_normal((O.level_rows(r, T), F)) * scale).astype(np.float32) for r in res]


def grads(tag: str, n: int, seed: int = 0, wide: bool = False) -> np.ndarray:
    """grad_out [n, L F] ~ N(0, 1).  wide: every element scaled by its own 2^-k, k uniform in 0 .. 35.
    The fixed-point grid 2^-s follows the batch's largest |g|; a contribution is rounded visibly (in
    the fp32 result) only where it is some 2^25 times smaller than that, so a gradient of one
    magnitude would hide how the kernel rounds — with the wide one the table gradient's bits depend on
    it (tests/test_hashgrid3d_logic.py)."""
    res, _, F, _, _ = cfg_args(tag)
    rng = np.random.default_rng([seed, n, ord(tag), 2])
    g = rng.standard_normal((n, len(res) * F))
    if wide:
        g = np.ldexp(g, -rng.integers(0, 36, size=g.shape))
    return g.astype(np.float32)


def rays(tag: str, B: int, S: int, n: int | None = None, seed: int = 0):
    """(o [B, 3], d [B, 3], t0 [n], t1 [n]) fp32: B rays of S sorted samples whose points cover the
    config's domain and leave it; n < B * S cuts the last ray short."""
    n = B * S if n is None else n
    rng = np.random.default_rng([seed, B, S, ord(tag), 3])
    d = rng.standard_normal((B, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    if CONFIGS[tag]["normalize"]:
        o = (rng.standard_normal((B, 3)) * 1.5).astype(np.float32)
        t = np.sort(rng.uniform(0.0, 5.0, size=(B, S + 1)), axis=1).astype(np.float32)
    else:
        o = rng.uniform(0.2, 0.8, size=(B, 3)).astype(np.float32)
        t = np.sort(rng.uniform(0.0, 0.4, size=(B, S + 1)), axis=1).astype(np.float32)
    return o, d, np.ascontiguousarray(t[:, :-1]).reshape(-1)[:n], np.ascontiguousarray(t[:, 1:]).reshape(-1)[:n]


def ray_query(t0: np.ndarray, t1: np.ndarray, query: int) -> np.ndarray:
    """t_q in fp32: the sample point (query 0) or the interval's midpoint (t0 + t1) / 2 (query 1)."""
    t0 = t0.astype(np.float32)
    return t0 if query == 0 else (t0 + t1.astype(np.float32)) / np.float32(2.0)


def ray_positions(o: np.ndarray, d: np.ndarray, t0: np.ndarray, t1: np.ndarray, S: int, query: int) -> np.ndarray:
    """Positions [n, 3] of the ray form in fp32, o[ray] + t_q * d[ray] with ray = sample // S: the
    product rounded, then added."""
    ray = np.arange(t0.shape[0]) // S
    tq = ray_query(t0, t1, query)
    return o.astype(np.float32)[ray] + tq[:, None] * d.astype(np.float32)[ray]


# ----------------------------------------------------------------------------- table gradient
def fixed_shift(n: int, gmax: float):
    """The exponent s of nerf_hashgrid_bwd's fixed-point grid: 8 n gmax < 2^e, s = min(62 - e, 120);
    60 for an all-zero gradient; None for a non-finite one."""
    if not np.isfinite(gmax):
        return None
    if gmax == 0:
        return 60
    _, e = math.frexp(8.0 * n * float(gmax))
    return min(62 - e, 120)


def table_grad_fixed(x: np.ndarray, g: np.ndarray, res, T: int, F: int, primes=O.PRIMES, normalize: bool = True,
                     accumulate: np.ndarray | None = None, *, corners=O.level_corners, rnd=np.rint, shift: int = 0,
                     n_corners: int = 8) -> np.ndarray:
    """Packed [rows, F] fp32 table gradient of sum(encode(x) * g), g [n, >= L * F], by the kernel's
    rule: per corner and feature one rounding of w * (g * 2^s) to an int64, integer sums, one rounding
    back, added in fp32 onto `accumulate` when given.  The keyword-only arguments exist for
    tests/test_hashgrid3d_logic.py's mutations of the rule and keep their defaults everywhere else."""
    n, L = x.shape[0], len(res)
    rows = [O.level_rows(int(r), T) for r in res]
    g = np.asarray(g)[:, :L * F].astype(np.float32)
    s = fixed_shift(max(n, 1), float(np.abs(g).max()) if g.size else 0.0)
    if s is None:
        return np.full((sum(rows), F), np.nan, dtype=np.float32)
    s += shift
    out = []
    for l, r in enumerate(res):
        acc = np.zeros((rows[l], F), dtype=np.int64)
        if n:
            idx, w = corners(x, int(r), T, primes, normalize)
            gs = np.ldexp(g[:, l * F:(l + 1) * F].astype(np.float64), s)
            for k in range(n_corners):
                np.add.at(acc, idx[:, k], rnd(w[:, k:k + 1].astype(np.float64) * gs).astype(np.int64))
        out.append((acc * math.ldexp(1.0, -s)).astype(np.float32))
    grad = np.concatenate(out, axis=0)
    return grad if accumulate is None else accumulate.astype(np.float32) + grad


def table_grad64(x: np.ndarray, g: np.ndarray, res, T: int, F: int, primes=O.PRIMES, normalize: bool = True):
    """(fp64 oracle gradient [rows, F], contributions per row [rows])."""
    ref = O.pack(O.encode_backward(x, g.astype(np.float64), res, T, F, primes, normalize))
    hits = []
    for r in res:
        idx, _ = O.level_corners(x, int(r), T, primes, normalize)
        hits.append(np.bincount(idx.reshape(-1), minlength=O.level_rows(int(r), T)))
    return ref, np.concatenate(hits)


# ----------------------------------------------------------------------------- position gradient
def pos_bound_constant(L: int, F: int) -> int:
    """Roundings on the longest path of hashgrid_bwd_pos_kernel: F products and adds for G, two weight
    products, the product with G, 8 corner adds, * r, / 8, L level adds — F + L + 13 — with a slack
    of 3."""
    return F + L + 16


def pos_grad64_with_bound(x: np.ndarray, tabs, res, T: int, g: np.ndarray, primes=O.PRIMES, normalize: bool = True):
    """(reference [n, 3], bound [n, 3]) in fp64: oracle.encode_position_grad, and per element
    (F + L + 16) 2^-24 A with A the same sum over levels, corners and features with every term replaced
    by its absolute value."""
    L, F = len(res), tabs[0].shape[1]
    ref = O.encode_position_grad(x, tabs, res, T, g, primes, normalize)
    A = np.zeros((x.shape[0], 3), dtype=np.float64)
    for l, (t, r) in enumerate(zip(tabs, res)):
        idx, _ = O.level_corners(x, int(r), T, primes, normalize)
        u32 = O.normalised(x) if normalize else x.astype(np.float32)
        xh = (u32 * np.float32(r)).astype(np.float64)
        base = np.floor(xh)
        gl = np.abs(g[:, l * F:(l + 1) * F].astype(np.float64))
        lvl = np.zeros_like(A)
        for k, off in enumerate(O.CORNERS_3D):
            u = xh - (base + np.array(off, dtype=np.float64))
            fac, dfac = np.abs(1.0 - np.abs(u)), np.abs(np.sign(u))
            G = (gl * np.abs(t[idx[:, k]].astype(np.float64))).sum(axis=1)
            for dim in range(3):
                e0, e1 = [e for e in range(3) if e != dim]
                lvl[:, dim] += G * dfac[:, dim] * fac[:, e0] * fac[:, e1]
        A += lvl * (r / 8.0 if normalize else float(r))
    return ref, pos_bound_constant(L, F) * U * A


def ray_grad64_with_bound(ref: np.ndarray, bound: np.ndarray, tq: np.ndarray, B: int, S: int):
    """The ray form's (grad_o, bound_o, grad_d, bound_d) [B, 3] from the per-sample reference and
    bound [B * S, 3] and t_q [B * S] (fp32 values): sums over each ray's samples in fp64; the fp32 sums
    of hashgrid_pos_rays_kernel (ceil(S / 64) strided adds, the product with t_q, six wave-sum adds,
    one of slack) add (ceil(S / 64) + 8) 2^-24 sum_s |dpos_s| (|t_q| |dpos_s| for grad_d)."""
    r3, b3 = ref.reshape(B, S, 3), bound.reshape(B, S, 3)
    t = np.abs(tq.astype(np.float64)).reshape(B, S, 1)
    ts = tq.astype(np.float64).reshape(B, S, 1)
    c = (-(-S // 64) + 8) * U
    mag = np.abs(r3) + b3
    return (r3.sum(1), b3.sum(1) + c * mag.sum(1), (ts * r3).sum(1), (t * b3).sum(1) + c * (t * mag).sum(1))
