"""The shared sine / cosine (csrc/common.h sincos_enc, csrc/param_act.h sincos_arg) over its whole
argument range, through every kernel family that calls it: SIREN's sine (nerf_sine_act_*), the
Fourier / BARF / integrated encodings at 16 levels (nerf_encode_fwd in both layouts, nerf_encode_bwd)
and the Gabor / Sarf activations with a grown spread / frequency (nerf_param_act_*).  Every reference
is fp64 math on the CPU of the same fp32 inputs.

sincos_enc has two paths: the fp32 Cody-Waite fast path for |x| < T = kSincosFastMax (read from
common.h below; swept exhaustively on the host by test_sincos_host.py) and sincosf from T on.  The
inputs here cross T, 2^24 (where the fast path would leave [-1, 1]) and 2^30 (the former limit).

Bounds.  The sine: 2e-7 absolute on y, 2e-7 plus one fp32 ulp of |cos| on dz at grad_y = 1
(test_gpu_siren.py's bounds), |y|, |dz| <= 1.  Encodings: 2e-7 absolute per column against fp64 cos /
sin of the argument formed in fp32 as the kernel and the reference model form it (one ulp of a 1e6
argument is 0.06: an fp64 product would measure the input's rounding, not the kernel); the backward
(2e-7 + (L + 4) 2^-23) A, A = |g_id| + sum_k m_k s_k (|g_cos| + |g_sin|): the sin / cos error plus the
fp32 product and accumulation rounding of L terms.  Gabor / Sarf: test_ragged_multi_slab's bounds,
unchanged."""
import math
import os
import re

import numpy as np
import pytest
import torch

from _gabor_sarf_ref import KINDS, PARAMS, act_bwd, act_fwd
from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = 0xA5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "nerf-experiments_amd", "csrc", "common.h")) as _f:
    T = float(re.search(r"kSincosFastMax\s*=\s*([0-9.]+)f", _f.read()).group(1))
FLT_MAX = float(np.finfo(np.float32).max)


@pytest.fixture(scope="module", autouse=True)
def _lib():
    import nerf_amd
    nerf_amd._lib.load()
    yield


def _guarded(rows, ld, guard_rows=3):
    """A [rows + guard_rows, ld] fp32 buffer whose every byte holds the sentinel."""
    return torch.full(((rows + guard_rows) * ld * 4,), SENT, dtype=torch.uint8, device=DEV).view(torch.float32) \
        .view(rows + guard_rows, ld)


def _guards_untouched(buf, M, N):
    b = buf.view(torch.uint8).view(buf.shape[0], buf.shape[1], 4)
    return bool((b[M:] == SENT).all()) and bool((b[:, N:] == SENT).all())


def _ulp32(a):
    """One fp32 ulp at |a| (fp64 tensor in, fp64 out)."""
    a32 = a.float().abs()
    return (torch.nextafter(a32, torch.full_like(a32, float("inf"))) - a32).double()


def _bits(i):
    return torch.from_numpy(np.asarray(i, dtype=np.uint32).view(np.float32).copy())


def _around(x, ulps):
    """The fp32 values from `ulps` below to `ulps` above float32(x), x > 0."""
    b = int(np.float32(x).view(np.uint32))
    return _bits(np.arange(b - ulps, b + ulps + 1, dtype=np.int64).astype(np.uint32))


# ------------------------------------------------------------------------------------ the sine
def _sine_inputs():
    """[2048 * 260] fp32, deterministic: 1024 mantissas (1000 seeded; 0, all-ones and eleven neighbours
    of each) in every binade 2^-126 .. 2^127 and among the subnormals, both signs (+-0 included); the
    fp32 values nearest k pi/2 and (k + 1/2) pi/2 and two ulps either side, k = 2^j, 2^j +- 1, j = 0 .. 29;
    eight ulps either side of T and of 2^30; +-FLT_MAX; the rest seeded uniform in [-2 T, 2 T]."""
    rng = np.random.RandomState(41)
    mant = np.concatenate((rng.randint(0, 1 << 23, 1000), np.arange(12), (1 << 23) - 1 - np.arange(12)))
    mant = mant.astype(np.uint32)
    assert mant.size == 1024
    expo = np.arange(0, 255, dtype=np.uint32)                           # 0: subnormals and zero
    pos = _bits(((expo[:, None] << 23) | mant[None, :]).reshape(-1))
    parts = [pos]
    ks = sorted({k for j in range(30) for k in (2 ** j - 1, 2 ** j, 2 ** j + 1) if k > 0})
    for k in ks:
        for m in (k, k + 0.5):
            parts.append(_around(m * math.pi / 2, 2))
    parts += [_around(T, 8), _around(2.0 ** 30, 8), torch.tensor([FLT_MAX])]
    z = torch.cat(parts)
    z = torch.cat((z, -z))
    n = 2048 * 260
    assert z.numel() <= n
    fill = torch.from_numpy(rng.uniform(-2 * T, 2 * T, n - z.numel()).astype(np.float32))
    return torch.cat((z, fill)).view(2048, 260)


def test_sine_act_whole_range():
    """nerf_sine_act_fwd / _bwd, one [2048, 260] launch with ragged row strides, grad_y = 1 so that
    dz is the cosine.  Every finite element is held to the bounds; none is left out."""
    from nerf_amd import kernels as K
    M, N = 2048, 260
    z = _sine_inputs()
    assert torch.isfinite(z).all()
    zb, yb, gb, dzb = _guarded(M, 263), _guarded(M, 261), _guarded(M, 267), _guarded(M, 262)
    zb[:M, :N] = z.to(DEV)
    gb[:M, :N] = 1.0
    K.sine_act_fwd(zb[:M], N, yb[:M])
    K.sine_act_bwd(gb[:M], zb[:M], N, dzb[:M])
    torch.cuda.synchronize()
    for buf in (yb, dzb, zb, gb):
        assert _guards_untouched(buf, M, N)
    assert torch.equal(zb[:M, :N].cpu().view(torch.int32), z.view(torch.int32))        # inputs unchanged
    y, dz = yb[:M, :N].cpu().double(), dzb[:M, :N].cpu().double()
    z64 = z.double()
    rs, rc = torch.sin(z64), torch.cos(z64)
    err_y = (y - rs).abs()
    over_dz = (dz - rc).abs() - (2e-7 + _ulp32(rc))
    fast = z.abs() < T
    for name, sel in (("fast path |z| < T", fast), ("sincosf path |z| >= T", ~fast)):
        i = err_y[sel].argmax()
        j = (dz - rc).abs()[sel].argmax()
        print(f"sine, {name} ({int(sel.sum())} values): max|y - sin| = {err_y[sel].max().item():.3e} at z = "
              f"{z[sel][i].item()!r}, max|dz - cos| = {(dz - rc).abs()[sel].max().item():.3e} at z = "
              f"{z[sel][j].item()!r}, dz over its bound by {over_dz[sel].max().item():.3e}")
    assert torch.isfinite(y).all() and torch.isfinite(dz).all()
    assert y.abs().max().item() <= 1.0 and dz.abs().max().item() <= 1.0
    assert err_y.max().item() <= 2e-7
    assert over_dz.max().item() <= 0


def test_sine_act_nonfinite():
    """+-inf and NaN give NaN, forward and backward."""
    from nerf_amd import kernels as K
    z = torch.tensor([[float("inf"), float("-inf"), float("nan"), 1.0]] * 3, device=DEV)
    y, dz = torch.zeros_like(z), torch.zeros_like(z)
    K.sine_act_fwd(z, 4, y)
    K.sine_act_bwd(torch.ones_like(z), z, 4, dz)
    assert torch.isnan(y[:, :3]).all() and torch.isnan(dz[:, :3]).all()
    assert torch.isfinite(y[:, 3]).all() and torch.isfinite(dz[:, 3]).all()


# ------------------------------------------------------------------------------- the encodings
L16 = 16
BARF_MASK = [1.0] * 12 + [0.3, 0.0, 0.0, 0.0]
MAGS = [1e-3, 0.4, 2.5, 2.6, 6.0, 80.0, 3000.0]


def _positions():
    """[197, 3] (three 64-row tiles and a ragged tail): +-{1e-3, 0.4, 2.5, 2.6, 6, 80, 3000}, exactly in
    the first rows, then with a seeded factor in [0.5, 1]: arguments scale * 2^k * |x| from 3e-3 to 6e8."""
    rng = np.random.RandomState(42)
    n = 197
    mag = np.asarray(MAGS)[(np.arange(n)[:, None] + 3 * np.arange(3)[None, :]) % 7]
    fac = np.where(np.arange(n)[:, None] < 14, 1.0, rng.uniform(0.5, 1.0, (n, 3)))
    sign = np.where((np.arange(n)[:, None] // 7 + np.arange(3)[None, :]) % 2 == 0, 1.0, -1.0)
    return torch.from_numpy((mag * fac * sign).astype(np.float32))


def _args32(x, levels, scale):
    """The kernels' fp32 arguments x_d * (float32(scale) * 2^k), [N, 3 * levels] d-major, and the
    per-column fp32 scales."""
    s = (torch.tensor(scale, dtype=torch.float32) * (2.0 ** torch.arange(levels, dtype=torch.float32))).repeat(3)
    return x.repeat_interleave(levels, dim=1) * s, s


def _fourier_ref(x, mask):
    a, _ = _args32(x, L16, 2 * math.pi)
    m = torch.tensor(mask if mask is not None else [1.0] * L16, dtype=torch.float32).double().repeat(3)
    return torch.cat((x.double(), m * torch.cos(a.double()), m * torch.sin(a.double())), dim=1), a


@pytest.mark.parametrize("mask", [None, BARF_MASK], ids=["fourier", "barf_mask"])
def test_encode_fwd_16_levels(mask):
    """nerf_encode_fwd on explicit positions, 16 levels at scale 2 pi, identity columns: the LDS kernel
    (out_ld = 100) and the per-quad kernel (out_ld = 163) agree bitwise, pad columns are zero, every
    column within 2e-7 of fp64 cos / sin of the fp32-formed argument; masked levels exactly 0."""
    from nerf_amd import kernels as K
    x = _positions()
    p = K.make_pe_params(0, L16, True, 2 * math.pi, mask=mask)
    xd = x.to(DEV)
    outs = [K.encode_fwd(p, 99, x=xd, n_samples=x.shape[0], out_ld=ld, device=DEV).cpu() for ld in (100, 163)]
    assert torch.equal(outs[0][:, :99].view(torch.int32), outs[1][:, :99].view(torch.int32))
    for out in outs:
        assert torch.all(out[:, 99:] == 0)
    ref, a = _fourier_ref(x, mask)
    assert a.abs().min().item() < 1e-2 and a.abs().max().item() > 5e8
    assert ((a.abs() >= T).sum().item() > 100) and ((a.abs() < T).sum().item() > 100)
    got = outs[0][:, :99].double()
    assert torch.equal(got[:, :3], x.double())
    err = (got - ref).abs()[:, 3:]
    a2 = torch.cat((a, a), dim=1).abs()
    for name, sel in (("fast path", a2 < T), ("sincosf path", a2 >= T)):
        print(f"encode_fwd L=16 {'masked' if mask else 'plain'}, {name}: max|err| = {err[sel].max().item():.3e}")
    assert torch.isfinite(got).all() and got[:, 3:].abs().max().item() <= 1.0
    assert err.max().item() <= 2e-7
    if mask is not None:
        off = torch.tensor([m == 0.0 for m in mask]).repeat(6)
        assert torch.all(outs[0][:, 3:99][:, off] == 0) and torch.all(outs[1][:, 3:99][:, off] == 0)


@pytest.mark.parametrize("mask", [None, BARF_MASK], ids=["fourier", "barf_mask"])
def test_encode_bwd_16_levels(mask):
    """nerf_encode_bwd on the same positions with a seeded grad_out (row stride 104) against the fp64
    sum over the fp32-formed arguments: dx_d = g_id + sum_k m_k s_k (-g_cos sin a + g_sin cos a), per
    output within (2e-7 + (L + 4) 2^-23) A, A = |g_id| + sum_k m_k s_k (|g_cos| + |g_sin|)."""
    from nerf_amd import kernels as K
    x = _positions()
    n = x.shape[0]
    g = torch.randn(n, 104, generator=torch.Generator().manual_seed(43))[:, :99]
    p = K.make_pe_params(0, L16, True, 2 * math.pi, mask=mask)
    gd = torch.zeros(n, 104, device=DEV)
    gd[:, :99] = g.to(DEV)
    dx = K.encode_bwd(p, x.to(DEV), gd[:, :99]).cpu().double()
    a, s = _args32(x, L16, 2 * math.pi)
    a, s, g64 = a.double(), s.double(), g.double()
    m = torch.tensor(mask if mask is not None else [1.0] * L16, dtype=torch.float32).double().repeat(3)
    gc, gs = g64[:, 3:51], g64[:, 51:99]
    terms = m * s * (-gc * torch.sin(a) + gs * torch.cos(a))
    ref = g64[:, :3] + terms.view(n, 3, L16).sum(dim=2)
    A = g64[:, :3].abs() + (m * s * (gc.abs() + gs.abs())).view(n, 3, L16).sum(dim=2)
    ratio = (dx - ref).abs() / A
    print(f"encode_bwd L=16 {'masked' if mask else 'plain'}: max|dx - ref| / A = {ratio.max().item():.3e} "
          f"(bound {2e-7 + (L16 + 4) * 2.0 ** -23:.3e}), max|dx| = {dx.abs().max().item():.3e}")
    assert torch.isfinite(dx).all()
    assert ratio.max().item() <= 2e-7 + (L16 + 4) * 2.0 ** -23


def test_integrated_encoding_16_levels():
    """The integrated (mip-NeRF) encoding, 16 levels at scale 1 (so that the fp32 argument pm * 2^k is
    exact), ray mode, 41 rays x 5 samples with |o| up to 40: arguments up to 1.3e6, both sides of T.
    Reference: oracle.nerf_oracle.integrated_pe in fp64, given the mean-shifted position as the kernel
    forms it in fp32 (o + tq d, + mu_diff d, each operation rounded).  Bound per column: 2e-7 times the
    column's weight w = exp(-vb 4^k / 2) plus two fp32 ulps of w for the expf; identity columns exact.

    The intervals are 8e-6 long and the pixels 1e-6 wide, so vb 4^15 / 2 stays below 0.01: the bound
    has no term for the fp32 rounding of vb (a few ulps, 1e-6 relative), which enters a column as
    w (vb 4^k / 2) 1e-6; kept below 1e-8 here it leaves the sin / cos as what is measured."""
    from nerf_amd import kernels as K
    B, S = 41, 5
    rng = np.random.RandomState(44)
    o = torch.from_numpy(rng.uniform(-40, 40, (B, 3)).astype(np.float32))
    o[0] = torch.tensor([40.0, -40.0, 1e-3])
    d = torch.nn.functional.normalize(torch.from_numpy(rng.normal(size=(B, 3)).astype(np.float32)), dim=1)
    t0 = torch.from_numpy(rng.uniform(2, 6, (B, 1)).astype(np.float32)) + torch.arange(S, dtype=torch.float32) * 8e-6
    t1 = t0 + 8e-6
    pw = torch.full((B,), 1e-6)
    p = K.make_pe_params(1, L16, True, 1.0, query=1, pixel_width_sigma=0.0, distribute_variance=False, pw_mode=0)
    outs = [K.encode_fwd(p, 99, ray_o=o.to(DEV), ray_d=d.to(DEV), t_start=t0.to(DEV).contiguous(),
                         t_end=t1.to(DEV).contiguous(), pixel_width=pw.to(DEV), n_samples=B * S, samples_per_ray=S,
                         n_rays=B, out_ld=ld, device=DEV).cpu() for ld in (100, 163)]
    assert torch.equal(outs[0][:, :99].view(torch.int32), outs[1][:, :99].view(torch.int32))
    for out in outs:
        assert torch.all(out[:, 99:] == 0)
    # the mean-shifted position in the kernel's fp32 operation order (encode_common.h)
    dv = d.repeat_interleave(S, dim=0)
    t0f, t1f = t0.reshape(-1, 1), t1.reshape(-1, 1)
    tq = (t0f + t1f) / 2.0
    pos = o.repeat_interleave(S, dim=0) + tq * dv
    td = (t1f - t0f) / 2.0
    tm2, td2 = tq * tq, td * td
    mu = ((2.0 * tq) * td2) / ((3.0 * tm2) + td2)
    pm = pos + mu * dv
    # fp64: the oracle shifts by its own mu_diff, so hand it pm - mu_diff d (to 1 fp64 ulp of pm)
    t064, t164, d64 = t0f.double(), t1f.double(), dv.double()
    tm64, td64 = (t064 + t164) / 2, (t164 - t064) / 2
    mu64 = 2 * tm64 * td64 ** 2 / (3 * tm64 ** 2 + td64 ** 2)
    pw64 = pw.double().repeat_interleave(S).view(-1, 1)
    ref = O.integrated_pe(pm.double() - mu64 * d64, d64, pw64, t064, t164, L16, 1.0, True, False, 0.0)
    w = O.integrated_pe(-mu64 * d64, d64, pw64, t064, t164, L16, 1.0, False, False, 0.0)[:, :48]       # cos(0) w
    assert ref.dtype == torch.float64 and w.min().item() > 0.98
    got = outs[0][:, :99].double()
    assert torch.equal(got[:, :3], pm.double())
    a = (pm.repeat_interleave(L16, dim=1) * (2.0 ** torch.arange(L16, dtype=torch.float32)).repeat(3)).abs()
    assert (a >= T).sum().item() > 100 and (a < T).sum().item() > 100 and a.max().item() > 1e6
    w2, a2 = torch.cat((w, w), dim=1), torch.cat((a, a), dim=1)
    err = (got[:, 3:] - ref[:, 3:]).abs()
    over = err - (2e-7 * w2 + 2 * _ulp32(w2))
    for name, sel in (("fast path", a2 < T), ("sincosf path", a2 >= T)):
        print(f"integrated L=16, {name}: max|err| = {err[sel].max().item():.3e}, over the bound by "
              f"{over[sel].max().item():.3e}")
    assert torch.isfinite(got).all()
    assert over.max().item() <= 0


# --------------------------------------------------------------------------- Gabor and Sarf
SPREADS = [25.0, 1e3, 1e5, 4e5, 6e5, 2e7, 2e9]                # p z up to 3e9; T / 1.5 = 3.5e5
FREQS = [2.0, 20.0, 64.0, 81.0, 100.0, 300.0]                  # f / q up to f^3 = 2.7e7; 81^3 > T > 80^3
ZS = [0.0, 1e-4, 1e-3, 1e-2, 0.1, 1.0]


def _large_case(family):
    M, N = 257, 37
    gen = torch.Generator().manual_seed(45)
    gy = torch.randn(M, N, generator=gen)
    if family == "gaborf":
        z = torch.rand(M, N, generator=gen) * 3 - 1.5
        ps = [torch.full((N,), 0.5), torch.tensor(SPREADS).repeat(6)[:N].clone()]
    else:
        zi = torch.randint(0, len(ZS), (M, N), generator=gen)
        z = torch.tensor(ZS)[zi] * (torch.randint(0, 2, (M, N), generator=gen) * 2 - 1).float()
        ps = [torch.tensor(FREQS).repeat(7)[:N].clone()]
    return M, N, z, gy, ps


@pytest.mark.parametrize("family", ["gaborf", "sarf"])
def test_gabor_sarf_large_arguments(family):
    """nerf_param_act_fwd / _bwd at [257, 37] (ragged in columns, no multiple of 4) with a grown spread
    (Gabor: p in {25 .. 2e9}, inv_standard_deviation 0.5, z uniform in [-1.5, 1.5], so the envelope stays
    above 0.57) or frequency (Sarf: f in {2 .. 300}, |z| in {0 .. 1}, so f / q runs up to f^3), against
    the fp64 restatement (_gabor_sarf_ref.py).  |y| <= 1; two backward runs bit-identical.

    Bounds: test_ragged_multi_slab's, unchanged (y: 1e-7 + 1e-6 |ref|, dz: 1e-6 + 1e-5 |ref|, parameter
    gradients: 1e-3 + 1e-4 |ref|).  dz carries sin(a) times a factor that grows with the parameter (p
    for Gabor, (f / q^2) 2 t for Sarf, up to 1e10 here), so an absolute sine error of 1e-7 would be far
    outside its bound wherever sin(a) is near 0.  It holds because the sine is accurate relative to
    itself there: the reduced argument is small and carries no absolute error of its own (the
    Cody-Waite remainder and the fp64-wrapped hi + lo are exact to their own ulp, sincosf likewise).
    Sarf's arguments reach f^3 = 2.7e7, Gabor's 3e9: the first-order path, the fp64 wrap on both sides
    of T, and sincosf."""
    from nerf_amd import kernels as K
    M, N, z, gy, ps = _large_case(family)
    psd = [p.to(DEV) for p in ps]
    zb, yb = _guarded(M, 40), _guarded(M, 41)
    zb[:M, :N] = z.to(DEV)
    K.param_act_fwd(KINDS[family], zb[:M], N, psd, yb[:M])
    runs = []
    for _ in range(2):
        gb, dzb = _guarded(M, 43), _guarded(M, 39)
        gb[:M, :N] = gy.to(DEV)
        grads = [torch.full((N,), float("nan"), device=DEV) for _ in ps]
        K.param_act_bwd(KINDS[family], gb[:M], zb[:M], N, psd, dzb[:M], grads)
        runs.append((dzb, grads))
    torch.cuda.synchronize()
    for buf in (zb, yb, runs[0][0], runs[1][0]):
        assert _guards_untouched(buf, M, N)
    assert torch.equal(runs[0][0][:M, :N].view(torch.int32), runs[1][0][:M, :N].view(torch.int32))
    for a, b in zip(runs[0][1], runs[1][1]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    z64, g64, p64 = z.double(), gy.double(), [p.double() for p in ps]
    ref = (act_fwd(family, z64, *p64),) + tuple(act_bwd(family, g64, z64, *p64))
    got = (yb[:M, :N].cpu(), runs[0][0][:M, :N].cpu()) + tuple(t.cpu() for t in runs[0][1])
    for t in got:
        assert torch.isfinite(t).all()
    assert got[0].abs().max().item() <= 1.0
    if family == "gaborf":
        env = torch.exp(-(z64 * z64) * (p64[0] * p64[0] + 1e-6))
        assert env.min().item() > 0.56 and (p64[1] * z64).abs().max().item() > 2.0 ** 31
    else:
        t = z64.abs() + 1e-4
        assert (p64[0] / (t * t + 1 / (p64[0] * p64[0]))).max().item() > 2.6e7
    names = ["y", "dz"] + [f"d_{p}" for p in PARAMS[family]]
    tols = [(1e-7, 1e-6), (1e-6, 1e-5)] + [(1e-3, 1e-4)] * (len(names) - 2)
    worst = []
    for n, a, b, (atol, rtol) in zip(names, got, ref, tols):
        err = (a.double() - b).abs()
        over = (err - (atol + rtol * b.abs())).max().item()
        print(f"{family} {n}: max|HIP - f64| = {err.max().item():.3e}, max|ref| = {b.abs().max().item():.3e}, "
              f"over {atol:g} + {rtol:g} |ref| by {over:.3e}")
        worst.append((n, over))
    for n, over in worst:
        assert over <= 0, (n, over)
