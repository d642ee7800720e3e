"""Quad-split X segments of the single-tile weight gradient (linear_wgrad_x3_tr_kernel,
nerf_linear_wgrad_x3_rows_q / _rays_q): the 16 bytes of 4 columns hold their bf16 hi halves, then
their lo halves (kernels.quad_split_pack), and the kernel copies them to its operand image instead
of splitting fp32 values.  Every slab-reduced dW, db and per-ray sum must be BIT-IDENTICAL between
the fp32 call and the call on the packed image of the same values.

The same shapes also run on fp32 X against a float64 product, which covers the kernel's scalar row
addressing and its role-specialised loops on their own.  Bound: 1e-6 of the reference's scale, the
bound tests/test_gpu_wgrad_tr.py uses.  That bound is the one of fp32 summation order, so the
float64 reference forms the products the kernel is specified to form (linear_x3.hip's header:
lo*hi + hi*lo + hi*hi of the bf16 halves, each exact in float64) and differs from the kernel in
the accumulation alone; db and the per-ray sums are fp32 sums of dY against float64 sums.  The
distance to the float64 product of the UNSPLIT values is the format's, not the kernel's: with
u = 2^-8 (bf16, round to nearest even) hi + lo carries an operand to u^2, so a product misses by at
most (2 u^2 + u^2 for the dropped lo*lo) |dY X| < 2^-14 |dY X|.  It is printed and bounded by
(2^-14 + M 2^-24) sum_m |dY X|, element by element (measured: 4e-6 to 8.4e-6 of the scale, the
largest for case (a), where a few large products carry the sum).

X holds exact zeros (a ReLU's share, about half), both signs and magnitudes from 2^-20 to 2^8; no
nonzero |x| < 2^-120, so the host packing does not depend on the denormal mode.

Case (d), N = 64 and K = 128, is not a shape of the tile kernel (it needs N or K above 128): its
fp32 run is checked against float64 like the others, and its quad-split call must be refused, as
every route other than the tile kernel is."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "nerf-experiments_amd")

# name -> (M0, M1, N, segments [(k, width of the tensor it is a view of, column offset, per-ray?)],
#          rays (S0, S1) or None, quad masks to run)
CASES = {
    "a_one_split_partial": (16 * 3 + 5, 0, 256, [(256, 256, 0, False)], None, [1]),
    "b_splits_partial": (2 * 3072 + 37, 0, 256, [(256, 256, 0, False)], None, [1]),
    "c_narrow_k_padded": (16 * 5 + 3, 0, 256, [(96, 96, 0, False)], None, [1]),
    "d_n64_k128": (16 * 5 + 3, 0, 64, [(128, 128, 0, False)], None, []),
    "e_two_blocks": (128 * 2, 128 * 3 + 16, 256, [(256, 256, 0, False)], None, [1]),
    "f_rays_mixed": (128 * 2, 128 * 3 + 32, 256, [(192, 192, 0, False), (32, 32, 0, True)], (16, 32), [1]),
    "g_column_view": (16 * 7 + 9, 0, 256, [(256, 512, 256, False)], None, [1]),
    "h_two_segments": (16 * 6 + 11, 0, 256, [(128, 128, 0, False), (96, 96, 0, False)], None, [1, 2, 3]),
}


def _x_values(rows, cols, g, dev):
    u = torch.rand(rows, cols, device=dev, generator=g) * 28.0 - 20.0           # exponents in [-20, 8)
    sign = torch.where(torch.rand(rows, cols, device=dev, generator=g) < 0.5, -1.0, 1.0)
    zero = torch.rand(rows, cols, device=dev, generator=g) < 0.5
    x = torch.where(zero, torch.zeros((), device=dev), sign * torch.exp2(u))
    nz = x[x != 0].abs()
    assert torch.isfinite(x).all() and (nz.numel() == 0 or nz.min() >= 2.0 ** -120)
    assert nz.min() < 2.0 ** -12 and nz.max() > 2.0 ** 4 and (x < 0).any() and (x > 0).any() and (x == 0).any()
    return x


@pytest.fixture(scope="module")
def K():
    from nerf_amd import kernels
    return kernels


def _build(name, K, dev):
    M0, M1, N, segdefs, rays, masks = CASES[name]
    g = torch.Generator(device=dev).manual_seed(1234 + M0 + 7 * M1 + N)
    N4 = (N + 3) // 4 * 4
    blocks = []
    for bi, M in enumerate((M0, M1)):
        M_alloc = max(M, 1)
        dY = torch.randn(M_alloc, N4, device=dev, generator=g)
        S = rays[bi] if rays else 1
        full = []
        for k, width, off, per_ray in segdefs:
            rd = S if per_ray else 1
            full.append((_x_values((M_alloc + rd - 1) // rd, width, g, dev), k, off, rd))
        blocks.append((dY, full, M))
    return blocks, N, N4, rays, masks


def _run(K, blocks, N, N4, rays, mask, dev):
    """dW [N, Kp], db [N], raysum or None for the blocks with the segments of `mask` quad-split."""
    def segs_of(full):
        out = []
        for j, (x, k, off, rd) in enumerate(full):
            t = K.quad_split_pack(x) if (mask >> j) & 1 else x
            out.append((t[:, off:off + k], k, rd))
        return out
    (dY0, f0, M0), (dY1, f1, M1) = blocks
    b0, b1 = (dY0, segs_of(f0), M0), (dY1, segs_of(f1), M1)
    Kp = sum(K.pad32(k) for _, k, _, _ in f0)
    ws = torch.empty((K.linear_wgrad_workspace_bytes(M0 + M1, N4, Kp) + 3) // 4, device=dev)
    col_map = torch.arange(Kp, dtype=torch.int32, device=dev)
    dW = torch.empty(N, Kp, device=dev)
    db = torch.empty(N, device=dev)
    rs = None
    if rays is not None:
        rs = torch.zeros(M0 // rays[0] + M1 // rays[1], N4, device=dev)
        K.linear_wgrad_x3_rays([b0, b1], N4, ws, rs, rays[0], rays[1], x_split_mask=mask)
    elif M1 > 0:
        K.linear_wgrad_x3_rows([b0, b1], N4, ws, x_split_mask=mask)
    else:
        K.linear_wgrad_x3(dY0, N4, b0[1], M0, ws, x_split_mask=mask)
    K.linear_wgrad_reduce(M0 + M1, N4, Kp, N, ws, col_map, dW, db)
    torch.cuda.synchronize()
    return dW, db, rs


def _halves(x):
    hi = x.bfloat16().float()
    return hi.double(), (x - hi).bfloat16().double()


def _reference(K, blocks, N, rays, dev):
    """float64: dW of the split products, dW of the unsplit values, sum_m |dY X|, db, raysum."""
    (dY0, f0, M0), (dY1, f1, M1) = blocks
    Kp = sum(K.pad32(k) for _, k, _, _ in f0)
    dW = torch.zeros(N, Kp, device=dev, dtype=torch.float64)
    dWu, dWa = torch.zeros_like(dW), torch.zeros_like(dW)
    db = torch.zeros(N, device=dev, dtype=torch.float64)
    rs = []
    for dY, full, M in ((dY0, f0, M0), (dY1, f1, M1)):
        if M == 0:
            continue
        d = dY[:M, :N].double()
        db += d.sum(0)
        koff = 0
        for x, k, off, rd in full:
            xf = x[:, off:off + k].repeat_interleave(rd, dim=0)[:M]
            (yh, yl), (xh, xl) = _halves(dY[:M, :N]), _halves(xf)
            dW[:, koff:koff + k] += yl.t() @ xh + yh.t() @ xl + yh.t() @ xh
            dWu[:, koff:koff + k] += d.t() @ xf.double()
            dWa[:, koff:koff + k] += d.abs().t() @ xf.double().abs()
            koff += K.pad32(k)
    if rays is not None:
        for (dY, _, M), S in zip((blocks[0], blocks[1]), rays):
            if M:
                rs.append(dY[:M, :N].double().view(M // S, S, N).sum(1))
    return dW, dWu, dWa, db, torch.cat(rs) if rs else None


@pytest.fixture(scope="module")
def fp32_runs(K):
    """The fp32 call of every case, computed once: (blocks, N, N4, rays, masks, (dW, db, rs))."""
    dev = torch.device("cuda", 0)
    out = {}
    for name in CASES:
        blocks, N, N4, rays, masks = _build(name, K, dev)
        out[name] = (blocks, N, N4, rays, masks, _run(K, blocks, N, N4, rays, 0, dev))
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_fp32_x_against_float64(K, fp32_runs, name):
    dev = torch.device("cuda", 0)
    blocks, N, N4, rays, _, (dW, db, rs) = fp32_runs[name]
    rW, rWu, rWa, rb, rr = _reference(K, blocks, N, rays, dev)
    M = blocks[0][2] + blocks[1][2]
    eW = ((dW.double() - rW).abs().max() / rW.abs().max()).item()
    eWu = ((dW.double() - rWu).abs().max() / rWu.abs().max()).item()
    eb = ((db.double() - rb).abs().max() / rb.abs().max()).item()
    print(f"{name}: dW err/scale {eW:.3e} (unsplit values: {eWu:.3e})  db err/scale {eb:.3e}")
    assert eW <= 1e-6, (name, eW)
    assert eb <= 1e-6, (name, eb)
    assert ((dW.double() - rWu).abs() <= (2.0 ** -14 + M * 2.0 ** -24) * rWa).all(), name
    if rr is not None:
        er = ((rs[:, :N].double() - rr).abs().max() / rr.abs().max()).item()
        print(f"{name}: raysum err/scale {er:.3e}")
        assert er <= 1e-6, (name, er)


@pytest.mark.parametrize("name,mask", [(n, m) for n in CASES for m in CASES[n][5]])
def test_quad_split_x_is_bit_identical(K, fp32_runs, name, mask):
    dev = torch.device("cuda", 0)
    blocks, N, N4, rays, _, (dW, db, rs) = fp32_runs[name]
    qW, qb, qr = _run(K, blocks, N, N4, rays, mask, dev)
    assert torch.equal(qW, dW), (name, mask, (qW - dW).abs().max().item())
    assert torch.equal(qb, db), (name, mask)
    if rs is not None:
        assert torch.equal(qr, rs), (name, mask)


def test_pack_is_the_kernels_split(K):
    """The host packing against the halves' definition, element by element."""
    dev = torch.device("cuda", 0)
    x = _x_values(37, 64, torch.Generator(device=dev).manual_seed(5), dev)
    hi, lo = K.quad_split_unpack(K.quad_split_pack(x))
    assert torch.equal(hi, x.bfloat16().float())
    assert torch.equal(lo, (x - x.bfloat16().float()).bfloat16().float())
    raw = K.quad_split_pack(x).view(torch.int16).view(37, 16, 8)
    assert torch.equal(raw[:, :, :4].reshape(37, 64), x.bfloat16().view(torch.int16))


def test_quad_split_argument_errors(K, fp32_runs):
    dev = torch.device("cuda", 0)
    # a quad-split segment read one row per ray
    blocks, N, N4, rays, _, _ = fp32_runs["f_rays_mixed"]
    with pytest.raises(RuntimeError, match="status -1"):
        _run(K, blocks, N, N4, rays, 2, dev)
    # a quad-split X beside the 257th row
    g = torch.Generator(device=dev).manual_seed(3)
    M = 64
    dY = torch.randn(M, 260, device=dev, generator=g)
    x = _x_values(M, 256, g, dev)
    ws = torch.empty((K.linear_wgrad_workspace_bytes(M, 260, 256) + 3) // 4, device=dev)
    K.linear_wgrad_x3(dY, 257, [(x, 256, 1)], M, ws)                      # (the fp32 call is fine)
    with pytest.raises(RuntimeError, match="status -1"):
        K.linear_wgrad_x3(dY, 257, [(K.quad_split_pack(x), 256, 1)], M, ws, x_split_mask=1)
    # a shape of another kernel: the 128-tile kernel (case d), the small-N kernel
    blocks, N, N4, rays, _, _ = fp32_runs["d_n64_k128"]
    with pytest.raises(RuntimeError, match="status -1"):
        _run(K, blocks, N, N4, rays, 1, dev)
    with pytest.raises(RuntimeError, match="status -1"):
        K.linear_wgrad_x3(dY[:, :4].contiguous(), 4, [(K.quad_split_pack(x), 256, 1)], M, ws, x_split_mask=1)
    # a bit past the segments
    with pytest.raises(RuntimeError, match="status -1"):
        K.linear_wgrad_x3(dY[:, :256].contiguous(), 256, [(x, 256, 1)], M, ws, x_split_mask=2)
    torch.cuda.synchronize()


CHILD = r"""
import sys, torch
sys.path.insert(0, {pkg!r})
from nerf_amd import kernels as K
dev = torch.device("cuda", 0)
M = 64
dY = torch.randn(M, 256, device=dev)
x = torch.randn(M, 256, device=dev)
ws = torch.empty((K.linear_wgrad_workspace_bytes(M, 256, 256) + 3) // 4, device=dev)
K.linear_wgrad_x3(dY, 256, [(x, 256, 1)], M, ws)
try:
    K.linear_wgrad_x3(dY, 256, [(K.quad_split_pack(x), 256, 1)], M, ws, x_split_mask=1)
except RuntimeError as e:
    assert "status -1" in str(e), e
    torch.cuda.synchronize()
    print("refused")
"""


def test_quad_split_refused_with_the_tile_kernel_routed_off():
    """NERF_WGRAD_TR=0 is read once per process: a child."""
    env = dict(os.environ, NERF_WGRAD_TR="0")
    r = subprocess.run([sys.executable, "-c", CHILD.format(pkg=PKG)], env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "refused", (r.stdout, r.stderr[-2000:])
