"""fp64 restatement of the encoding forward kernels (csrc/encode.hip: nerf_encode_fwd's
encode_fwd_lds_kernel and encode_fwd_kernel, nerf_encode_rays) with a derived per-column error
bound, and the cases the CPU self-check (test_encode_fwd_ref.py) and the GPU tests
(test_gpu_encode_fwd_edges.py) share.  CPU, torch, vectorised; nothing here touches a device.  The
case type, the inputs and the per-sample mirror are _encode_bwd_ref.py's.

One row (include/nerf_amd.h; csrc/encode_common.h enc_column), per sample, coordinate d and level k,
a = pm_d s_k, s_k = fp32(scale) 2^k, m_k the mask (1 without one):

    identity (when asked for)  pm_0 pm_1 pm_2
    cos block, column d L + k  m_k w cos a
    sin block, column d L + k  m_k w sin a        w = exp(-(vb_d 4^k) / 2) for kind 1, 1 for kind 0
    columns out_dim .. ld - 1  0

pm is the position (x, or o + tq d in ray mode), for kind 1 shifted along the ray by mu_diff d.

Per-sample quantities (tq, pos, mu_diff, pm, st, sr, vb, and the argument a) are formed in fp32, one
rounding per operation, in the order of load_pos_dir / ipe_sample, and promoted to fp64, for
_encode_bwd_ref.py's reason: one ulp of a 1e6 argument is 0.06 rad, and the kernel, not the rounding
of its inputs, is what is measured.  exact=True forms all of them in fp64, for the comparison with
the oracle's encodings evaluated in fp64.

Identity columns.  An explicit x of kind 0 is copied.  o + tq d and pos + mu_diff d are the same
correctly rounded IEEE operations on the device and here (contraction is off in the kernels, and
td^4, the one operation that cannot be mirrored, is not on pm's path): the fp32-formed value
(FwdRef.ident) is held bit for bit, bound 0.

Bound of a cos / sin column:

    m_k w (SINCOS + n_ops 2^-24 + [kind 1] (2 + N_VB x) 2^-23) + 2^-125 m_k,     x = vb_d 4^k / 2

SINCOS = 2e-7: the shared sin / cos against fp64 sin / cos of the fp32 argument, its result's own
  rounding included (test_gpu_sincos_range.py's figure; both of sincos_enc's branches).
n_ops, in units of 2^-24 (one fp32 rounding, relative to the product, itself at most m_k w), counts
  the operations after the sin / cos, from csrc/encode.hip (phase 1 of encode_fwd_lds_kernel) and
  enc_column: cs * w (kind 1 only) and m * cs (only when a mask is passed): n_ops = [kind 1] +
  [mask].  Without either the column is the sin / cos itself and the bound is SINCOS.
w: vb_d * 4^k and the division by 2 are exact (powers of two), so w is expf of the exact -x of the
  kernel's own vb: 2 ulps of expf, and N_VB ulps of vb (the two td^4; _encode_bwd_ref.py derives the 9)
  carried through the exponential, d w / w = x d vb / vb.
floor: a product below 2^-126 (w underflows from x = 87 on) may be flushed to zero; with |sin|,
  |cos| <= 1 what is lost is below 2^-126 m_k.
A column whose mask is 0 has bound 0: m * cs is then +-0 for every finite cs.

A ratio err / bound above 1 on the device is a finding: a bug, or a rounding this count missed."""
import math
from dataclasses import dataclass

import torch

from _encode_bwd_ref import (FLOOR, N_VB, RAY_CASES, SINCOS, U, Case, _ipe, _levels_identity, _scales, _VAR, by_name,
                             expand_pw, ray_inputs, sample_inputs)

__all__ = ["RAY_CASES", "SAMPLE_CASES", "Case", "by_name", "ray_inputs", "sample_inputs", "expand_pw"]

# nerf_encode_fwd on explicit positions (x, and xdir / t / pixel widths for kind 1, pw_mode 2): the
# level / identity set for each kind, the four variance forms in turn, row counts around the 64-row
# tile of the LDS kernel (1, 63, 64, 65, and 129 = two tiles and one row), the two scales in turn
# (at 2 pi and 16 levels the arguments of positions in [-6, 6] pass 2^19), one mask per kind.
_ROWS = [1, 63, 64, 65, 129]
SAMPLE_CASES = [
    Case(f"k{kind}_L{L}_{'id' if ident else 'noid'}"
         + (f"_{'dist' if _VAR[i % 4][0] else 'diag'}_s{_VAR[i % 4][1]:g}" if kind else "")
         + f"_n{_ROWS[(i + kind) % 5]}" + ("_mask" if i == masked else ""),
         kind, L, ident, _ROWS[(i + kind) % 5], 1, scale=(1.0, 2 * math.pi)[(i + kind) % 2],
         distribute=bool(kind) and _VAR[i % 4][0], sigma=_VAR[i % 4][1] if kind else 0.0, pw_mode=2,
         alpha=alpha if i == masked else None, seed=80 + 20 * kind + i)
    for kind, masked, alpha in ((0, 4, 7.3), (1, 7, 9.6))
    for i, (L, ident) in enumerate(_levels_identity())
]


@dataclass
class Quantities:
    pm: torch.Tensor                 # [N, 3], the dtype they were formed in
    vb: torch.Tensor | None          # [N, 3], kind 1
    copied: bool = False             # pm is the caller's x itself


def ray_quantities(c: Case, inp, exact=False) -> Quantities:
    """Ray mode (x == NULL): load_pos_dir, then ipe_sample for kind 1."""
    dt = torch.float64 if exact else torch.float32
    B, S = c.n_rays, c.samples
    o, d = inp["o"].to(dt), inp["d"].to(dt)
    t0, t1 = inp["t0"].to(dt).reshape(-1), inp["t1"].to(dt).reshape(-1)
    tq = t0 if c.query == 0 else (t0 + t1) / torch.tensor(2.0, dtype=dt)
    dv = d.repeat_interleave(S, dim=0)
    pos = o.repeat_interleave(S, dim=0) + tq.unsqueeze(1) * dv
    if c.kind == 0:
        return Quantities(pos, None)
    q = _ipe(c, pos, dv, t0, t1, expand_pw(inp["pw"], c.pw_mode, B, S).to(dt), dt)
    return Quantities(q["pm"], q["vb"])


def sample_quantities(c: Case, inp, exact=False) -> Quantities:
    """Explicit positions x (kind 1: with xdir, t_start, t_end and one pixel width per sample)."""
    dt = torch.float64 if exact else torch.float32
    x = inp["x"].to(dt)
    if c.kind == 0:
        return Quantities(x, None, copied=True)
    q = _ipe(c, x, inp["d"].to(dt), inp["t0"].to(dt).reshape(-1), inp["t1"].to(dt).reshape(-1),
             inp["pw"].to(dt).reshape(-1), dt)
    return Quantities(q["pm"], q["vb"])


def _mask(c: Case, dt):
    if c.alpha is None:
        return torch.ones(c.levels, dtype=dt)
    return torch.tensor(c.mask(), dtype=torch.float32).to(dt)


def n_ops(c: Case):
    return int(c.kind == 1) + int(c.alpha is not None)


@dataclass
class FwdRef:
    ref: torch.Tensor                # [N, out_dim] fp64
    bound: torch.Tensor              # [N, out_dim] fp64; 0: the column is held bit for bit
    ident: torch.Tensor | None       # [N, 3] the identity columns as formed (fp32 unless exact)
    w: torch.Tensor                  # [N, 3, L] fp64
    x: torch.Tensor                  # [N, 3, L] vb 4^k / 2
    mw: torch.Tensor                 # [N, 3, L] m_k w
    unmasked: torch.Tensor           # [N, 3, L]


def fwd_ref(c: Case, q: Quantities) -> FwdRef:
    """Reference row and per-column bound from the per-sample quantities."""
    N, L = q.pm.shape[0], c.levels
    dt = q.pm.dtype
    s = _scales(c, dt).view(1, 1, L)
    a = (q.pm.unsqueeze(2) * s).double()
    m = _mask(c, torch.float64).view(1, 1, L)
    if c.kind == 1:
        x = q.vb.double().unsqueeze(2) * (4.0 ** torch.arange(L, dtype=torch.float64)).view(1, 1, L) / 2
        w = torch.exp(-x)
    else:
        x = torch.zeros(N, 3, L, dtype=torch.float64)
        w = torch.ones(N, 3, L, dtype=torch.float64)
    mw = m * w
    eps = SINCOS + n_ops(c) * U + ((2 + N_VB * x) * 2 * U if c.kind == 1 else 0.0)
    b = (mw * eps + FLOOR * m).reshape(N, 3 * L)
    parts = [(mw * torch.cos(a)).reshape(N, 3 * L), (mw * torch.sin(a)).reshape(N, 3 * L)]
    bounds = [b, b]
    if c.identity:
        parts.insert(0, q.pm.double())
        bounds.insert(0, torch.zeros(N, 3, dtype=torch.float64))
    return FwdRef(torch.cat(parts, dim=1), torch.cat(bounds, dim=1), q.pm if c.identity else None, w, x, mw,
                  (m != 0).expand(N, 3, L))


def fwd_fp32(c: Case, q: Quantities) -> torch.Tensor:
    """The same row by torch in fp32, operation by operation in enc_column's order: what the kernel
    computes with torch's sin / cos / exp in place of its own."""
    assert q.pm.dtype == torch.float32
    N, L = q.pm.shape[0], c.levels
    a = q.pm.unsqueeze(2) * _scales(c, torch.float32).view(1, 1, L)
    cs, sn = torch.cos(a), torch.sin(a)
    if c.kind == 1:
        w = torch.exp((-(q.vb.unsqueeze(2) * (4.0 ** torch.arange(L, dtype=torch.float32)).view(1, 1, L))) / 2.0)
        cs, sn = cs * w, sn * w
    if c.alpha is not None:
        m = _mask(c, torch.float32).view(1, 1, L)
        cs, sn = m * cs, m * sn
    parts = [cs.reshape(N, 3 * L), sn.reshape(N, 3 * L)]
    if c.identity:
        parts.insert(0, q.pm)
    return torch.cat(parts, dim=1)


def ray_case(c: Case, exact=False):
    inp = ray_inputs(c)
    return inp, fwd_ref(c, ray_quantities(c, inp, exact))


def sample_case(c: Case, exact=False):
    inp = sample_inputs(c)
    return inp, fwd_ref(c, sample_quantities(c, inp, exact))
