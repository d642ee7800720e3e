"""GPU tests of the 3-D hash-grid kernels (csrc/hashgrid.hip: nerf_hashgrid_fwd / _bwd / _bwd_pos) at
their edge shapes, against the CPU restatements of tests/_hashgrid3d_ref.py.

Cases: the seven level layouts of ``R.CONFIGS`` (tables of at most 4 096 rows a level) at the batch
sizes ``R.SIZES`` — around the restage tile (64), the workgroup and the llrint -> rint_fixed switch
(256) and the second slab (4096).  Every output lies in a guarded buffer (tests/_guarded.py), tables
between NaN canary rows, gradient rows carry 1e30 in their pad columns, workspaces start as garbage.

Forward and table gradient: BITWISE oracle.encode and R.table_grad_fixed (the rule include/nerf_amd.h
states), for explicit points and for the ray form, with the minimal and the full workspace, under
every non-default NERF_HG_* switch (one child process each).  The table gradient's grad_out spans 35
binades, so that the way the kernel rounds shows in the result's bits (tests/test_hashgrid3d_logic.py).

Position gradient: every element within R.pos_grad64_with_bound's derived bound,
(F + L + 16) 2^-24 A (A: the same sum with every term's absolute value), of the fp64 oracle; the ray
form adds (ceil(S / 64) + 8) 2^-24 sum |dpos| for the per-ray fp32 sums.  Every measured error is
printed next to its bound.  Measured on an MI355X, as fractions of each tensor's largest reference entry
(the worst case over the batch sizes, or over S and the query mode): largest error | largest bound
            grad_x               grad_o               grad_d
    A   2.0e-07 | 2.6e-06    1.6e-07 | 1.7e-05    1.2e-07 | 2.3e-05
    B   1.3e-07 | 3.4e-06    1.8e-07 | 2.6e-05    2.0e-07 | 3.1e-05
    C   1.7e-07 | 3.8e-06    1.3e-07 | 1.8e-05    1.9e-07 | 1.9e-05
    D   1.4e-07 | 9.4e-06    1.3e-07 | 2.9e-05    1.2e-07 | 2.8e-05
    E   2.1e-07 | 7.6e-06    1.0e-07 | 1.3e-05    1.9e-07 | 1.1e-05
    G   1.4e-07 | 2.8e-06    1.8e-07 | 2.5e-05    1.8e-07 | 2.1e-05
    H   1.7e-07 | 4.5e-05    2.0e-07 | 2.7e-04    2.9e-07 | 2.5e-04
In absolute terms: grad_x errors of 4.4e-08 (E, n = 1, values to 0.21) to 3.7e-05 (H, n = 4097, values
to 220); no element of any case used more than 0.145 of its bound.  The bound is a worst case over signs
(every term's absolute value), so it is loose where many terms cancel: 256 columns (H), and a ray's
bound, the sum of its samples' bounds, grows like S where the summed gradient grows like sqrt(S) —
per sample it stays below 1e-4 of the largest entry in every case (asserted), per ray of 65 samples
it reaches 2.7e-4 at H.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _hashgrid3d_ref as R
from _guarded import Guarded
from oracle import hashgrid_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"
TAGS = list(R.CONFIGS)
OK, INVALID, WORKSPACE = 0, -1, -4


@pytest.fixture(scope="module", autouse=True)
def _lib():
    import nerf_amd
    nerf_amd._lib.load()  # fail loudly if the HIP library is missing
    yield


def lib():
    import nerf_amd
    return nerf_amd._lib.load()


def stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def params(tag, query=1):
    from nerf_amd import kernels as K
    res, T, F, primes, normalize = R.cfg_args(tag)
    return K.make_hashgrid_params(len(res), T, F, res, query, primes=primes, normalize=normalize)


def dims(tag):
    res, _, F, _, _ = R.cfg_args(tag)
    return len(res), F, len(res) * F


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


class Points:
    """The position arguments of the three entry points: explicit x [n, 3], or rays (o, d [B, 3],
    t0, t1 [n], S samples a ray)."""

    def __init__(self, x=None, rays=None, S=1):
        self.keep = [dev(a) for a in ((x,) if rays is None else rays)]
        self.S = S
        self.rays = rays is not None

    def args(self, n):
        """(x, ray_o, ray_d, t_start, t_end, n, samples_per_ray); an empty tensor's pointer is null."""
        p = [t.data_ptr() or None for t in self.keep]
        return ((None, *p) if self.rays else (p[0], None, None, None, None)) + (n, self.S)


class Table:
    """The packed table between NaN canary rows (a stray read poisons the result), optionally `shift`
    floats off its 8-byte alignment."""

    def __init__(self, tabs, shift=0, guard=64):
        packed = O.pack(tabs)
        F = packed.shape[1]
        self.buf = torch.full(((packed.shape[0] + 2 * guard) * F + 2,), float("nan"), device=DEV)
        self.lo, self.size = guard * F + shift, packed.size
        self.buf[self.lo:self.lo + self.size] = dev(packed).view(-1)

    def ptr(self):
        return self.buf.data_ptr() + 4 * self.lo

    def check(self):
        assert torch.isnan(self.buf[:self.lo]).all() and torch.isnan(self.buf[self.lo + self.size:]).all()


def fwd(tag, tabs, n, pts, query=1, ld=None, out_shift=0, table_shift=0):
    """Features [n, L F] from nerf_hashgrid_fwd into a guarded [n + 3, ld] buffer: only the L F columns
    of the n rows may change, and all of them must."""
    L, F, cols = dims(tag)
    ld = cols + 5 if ld is None else ld
    rows = n + 3
    e = torch.arange(rows * ld)
    named = torch.zeros(rows * ld + out_shift, dtype=torch.bool)
    named[out_shift:] = (e // ld < n) & (e % ld < cols)
    out, tb, p = Guarded(rows * ld + out_shift, named=named), Table(tabs, table_shift), params(tag, query)
    st = lib().nerf_hashgrid_fwd(ctypes.byref(p), *pts.args(n), tb.ptr(), out.ptr() + 4 * out_shift, ld, stream())
    assert st == OK, st
    out.check(f"features {tag} n={n} ld={ld}")
    tb.check()
    return out.body[out_shift:].view(rows, ld)[:n, :cols].cpu().numpy()


def garbage(nbytes, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randint(-2 ** 62, 2 ** 62, ((nbytes + 7) // 8,), dtype=torch.int64, device=DEV, generator=gen)


def bwd(tag, n, g, pts, query=1, full=False, accumulate=None, pad=3, seed=1):
    """Packed table gradient [rows, F] from nerf_hashgrid_bwd: grad_out rows of stride L F + pad whose
    pad columns hold 1e30 (they must not enter the max), a garbage workspace of the minimal or the
    full (nerf_hashgrid_workspace_n) size, the gradient in a guarded buffer."""
    from nerf_amd import kernels as K
    L, F, cols = dims(tag)
    p = params(tag, query)
    rows = K.hashgrid_table_rows(p)
    gp = np.full((n, cols + pad), 1e30, dtype=np.float32)
    gp[:, :cols] = g
    gd = dev(gp)
    ws = garbage(K.hashgrid_workspace_bytes(p, n) if full else K.hashgrid_workspace_bytes(p), seed)
    gt = Guarded(rows * F)
    if accumulate is not None:
        gt.body.copy_(dev(accumulate).view(-1))
    st = lib().nerf_hashgrid_bwd(ctypes.byref(p), *pts.args(n), gd.data_ptr() or None, cols + pad, gt.ptr(),
                                 int(accumulate is not None), ws.data_ptr(), ws.numel() * 8, stream())
    assert st == OK, st
    gt.check(f"table gradient {tag} n={n}")
    return gt.body.view(rows, F).cpu().numpy()


# ----------------------------------------------------------------------------- forward
@pytest.mark.parametrize("n", R.SIZES)
@pytest.mark.parametrize("tag", TAGS)
def test_forward_bitwise(tag, n):
    res, T, _, primes, normalize = R.cfg_args(tag)
    tabs, x = R.tables(tag), R.points(tag, n)
    got = fwd(tag, tabs, n, Points(x))
    assert same_bits(got, O.encode(x, tabs, res, T, primes, normalize))


@pytest.mark.parametrize("n", [65, 257])
def test_forward_fallback_kernel(n):
    """F = 2 with an odd row stride, an output or a table 4 bytes off the 8-byte alignment takes the
    per-(sample, level) kernel: bitwise the aligned call."""
    res, T, _, primes, normalize = R.cfg_args("A")
    tabs, x = R.tables("A"), R.points("A", n)
    want = fwd("A", tabs, n, Points(x), ld=10)
    assert same_bits(want, O.encode(x, tabs, res, T, primes, normalize))
    assert same_bits(fwd("A", tabs, n, Points(x), ld=9), want)
    assert same_bits(fwd("A", tabs, n, Points(x), ld=10, out_shift=1), want)
    assert same_bits(fwd("A", tabs, n, Points(x), ld=10, table_shift=1), want)


RAY_B = 5


def ray_cases(sizes):
    for S in sizes:
        for n in ((RAY_B * S, RAY_B * S - 1) if S > 1 else (RAY_B * S,)):
            for query in (0, 1):
                yield S, n, query


@pytest.mark.parametrize("tag", TAGS)
def test_forward_ray_form_bitwise(tag):
    res, T, _, primes, normalize = R.cfg_args(tag)
    tabs = R.tables(tag)
    for S, n, query in ray_cases((1, 3, 64, 65)):
        o, d, t0, t1 = R.rays(tag, RAY_B, S, n)
        pos = R.ray_positions(o, d, t0, t1, S, query)
        got = fwd(tag, tabs, n, Points(rays=(o, d, t0, t1), S=S), query=query)
        assert same_bits(got, O.encode(pos, tabs, res, T, primes, normalize)), (S, n, query)


# ----------------------------------------------------------------------------- table gradient
@pytest.mark.parametrize("n", R.SIZES)
@pytest.mark.parametrize("tag", TAGS)
def test_table_gradient_bitwise(tag, n):
    res, T, F, primes, normalize = R.cfg_args(tag)
    cols = len(res) * F
    x, g = R.points(tag, n), R.grads(tag, n, wide=True)
    want = R.table_grad_fixed(x, g, res, T, F, primes, normalize)
    if n == 0:
        assert not want.any()
    pts = Points(x)
    for full in (False, True):
        assert same_bits(bwd(tag, n, g, pts, full=full, seed=1), want), full
        # again from other garbage; where the columns allow it with a vector row stride (the float4 max)
        assert same_bits(bwd(tag, n, g, pts, full=full, seed=2, pad=4 if cols % 4 == 0 else 3), want), full
    base = np.random.default_rng(n).standard_normal(want.shape).astype(np.float32)
    assert same_bits(bwd(tag, n, g, pts, full=True, accumulate=base), base + want)
    assert same_bits(R.table_grad_fixed(x, g, res, T, F, primes, normalize, accumulate=base), base + want)
    if n == 0:
        assert same_bits(bwd(tag, n, g, pts, accumulate=base), base)


def test_table_gradient_scales():
    res, T, F, primes, normalize = R.cfg_args("A")
    n = 257
    x, g = R.points("A", n), R.grads("A", n)
    pts = Points(x)

    def both(gg):
        got = bwd("A", n, gg, pts)
        assert same_bits(bwd("A", n, gg, pts, full=True), got)
        return got

    tiny = (g * np.float32(1e-30)).astype(np.float32)             # the shift capped at 120
    assert R.fixed_shift(n, float(np.abs(tiny).max())) == 120
    assert same_bits(both(tiny), R.table_grad_fixed(x, tiny, res, T, F, primes, normalize))
    huge = (g * np.float32(1e30)).astype(np.float32)              # a negative shift
    assert R.fixed_shift(n, float(np.abs(huge).max())) < 0
    assert same_bits(both(huge), R.table_grad_fixed(x, huge, res, T, F, primes, normalize))
    assert not both(np.zeros_like(g)).any()
    for bad in (np.nan, np.inf):
        gb = g.copy()
        gb[100, 5] = bad
        assert np.isnan(both(gb)).all()
        clean = both(g)                                          # nothing carried over
        assert np.isfinite(clean).all() and same_bits(clean, R.table_grad_fixed(x, g, res, T, F, primes, normalize))


def test_table_gradient_at_the_rint_fixed_limit():
    """n = 256 is the first batch whose contributions are rounded by rint_fixed, which needs |x| < 2^51:
    the shift rule gives gmax 2^s < 2^51 with nothing to spare.  Row 0 is (0, 0, 0), a grid corner of
    levels 0, 1 and 3 of config A (weight 1), and carries the batch's largest |g| = 1 - 2^-24."""
    res, T, F, primes, normalize = R.cfg_args("A")
    n = 256
    x = R.points("A", n)
    g = np.clip(R.grads("A", n) * np.float32(0.3), -0.99, 0.99).astype(np.float32)
    top = np.float32(1.0) - np.float32(2.0 ** -24)
    g[0] = top * np.where(np.arange(g.shape[1]) % 2 == 0, 1, -1).astype(np.float32)
    assert R.fixed_shift(n, float(np.abs(g).max())) == 51
    _, w = O.level_corners(x[:1], res[0], T, primes, normalize)
    assert w.max() == 1.0
    want = R.table_grad_fixed(x, g, res, T, F, primes, normalize)
    for full in (False, True):
        assert same_bits(bwd("A", n, g, Points(x), full=full), want)


@pytest.mark.parametrize("tag", ["A", "B", "D"])
def test_table_gradient_ray_form_bitwise(tag):
    res, T, F, primes, normalize = R.cfg_args(tag)
    for S, n, query in ray_cases((1, 64, 65)):
        o, d, t0, t1 = R.rays(tag, RAY_B, S, n)
        pos = R.ray_positions(o, d, t0, t1, S, query)
        g = R.grads(tag, n, wide=True)
        want = R.table_grad_fixed(pos, g, res, T, F, primes, normalize)
        pts = Points(rays=(o, d, t0, t1), S=S)
        for full in (False, True):
            assert same_bits(bwd(tag, n, g, pts, query=query, full=full), want), (S, n, query, full)


SWITCHES = [("NERF_HG_FWD", "0"), ("NERF_HG_FWD", "2"), ("NERF_HG_BWD", "1"), ("NERF_HG_BWD", "2"),
            ("NERF_HG_MERGE", "1"), ("NERF_HG_BUCKET", "0"), ("NERF_HG_PACK", "0")]


def test_non_default_switches(tmp_path):
    """The library reads its switches once per process: a fresh child per setting, one after the other;
    a child that fails ends the test before the next one starts."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_hashgrid3d_child.py")
    want = {}
    for tag in ("A", "B", "C", "G"):
        res, T, F, primes, normalize = R.cfg_args(tag)
        tabs = R.tables(tag)
        for n in (65, 257, 4097):
            x, g = R.points(tag, n), R.grads(tag, n, wide=True)
            want[f"{tag}.{n}.fwd"] = O.encode(x, tabs, res, T, primes, normalize)
            want[f"{tag}.{n}.bwd_min"] = want[f"{tag}.{n}.bwd_full"] = R.table_grad_fixed(x, g, res, T, F, primes, normalize)
    clean = {k: v for k, v in os.environ.items() if not k.startswith("NERF_HG_")}
    for name, value in SWITCHES:
        f = str(tmp_path / f"{name}_{value}.npz")
        r = subprocess.run([sys.executable, child, f], env=dict(clean, **{name: value}), capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0, (name, value, r.stderr[-3000:])
        got = dict(np.load(f, allow_pickle=False))
        assert got.keys() == want.keys()
        for k in want:
            assert same_bits(got[k], want[k]), (name, value, k)


# ----------------------------------------------------------------------------- position gradient
def report(what, got, ref, bound):
    err = np.abs(got.astype(np.float64) - ref)
    used = np.divide(err, bound, out=np.zeros_like(err), where=bound > 0)
    print(f"{what}: largest error {err.max():.3e}, largest bound {bound.max():.3e} "
          f"({bound.max() / np.abs(ref).max():.1e} of the largest value {np.abs(ref).max():.3e}); "
          f"largest error / bound of one element {used.max():.3f}")
    assert (err <= bound).all(), what


def padded(g, pad=3):
    gp = np.full((g.shape[0], g.shape[1] + pad), np.nan, dtype=np.float32)
    gp[:, :g.shape[1]] = g
    return dev(gp)


def bwd_pos_x(tag, tb, n, x, gd, g_ld, accumulate=None):
    gx, p = Guarded(n * 3), params(tag)
    if accumulate is not None:
        gx.body.copy_(dev(accumulate).view(-1))
    st = lib().nerf_hashgrid_bwd_pos(ctypes.byref(p), x.data_ptr(), None, None, None, None, n, 1, tb.ptr(), gd.data_ptr(),
                                     g_ld, gx.ptr(), None, None, int(accumulate is not None), None, 0, stream())
    assert st == OK, st
    gx.check(f"grad_x {tag} n={n}")
    tb.check()
    return gx.body.view(n, 3).cpu().numpy()


@pytest.mark.parametrize("n", R.SIZES[1:])
@pytest.mark.parametrize("tag", TAGS)
def test_position_gradient_within_the_derived_bound(tag, n):
    res, T, F, primes, normalize = R.cfg_args(tag)
    tabs, x, g = R.tables(tag), R.points(tag, n), R.grads(tag, n)
    ref, bound = R.pos_grad64_with_bound(x, tabs, res, T, g, primes, normalize)
    assert bound.max() <= 1e-4 * np.abs(ref).max()
    tb, xd, gd = Table(tabs), dev(x), padded(g)
    got = bwd_pos_x(tag, tb, n, xd, gd, g.shape[1] + 3)
    report(f"grad_x {tag} n={n}", got, ref, bound)
    assert same_bits(bwd_pos_x(tag, tb, n, xd, gd, g.shape[1] + 3), got)
    base = np.random.default_rng(n).standard_normal(got.shape).astype(np.float32)
    assert same_bits(bwd_pos_x(tag, tb, n, xd, gd, g.shape[1] + 3, accumulate=base), base + got)
    if normalize:       # the (0, 0, 0) row lies on a cell face of every even level: sign(0) = 0 there
        assert np.isfinite(got[0]).all() and (np.abs(got[0].astype(np.float64) - ref[0]) <= bound[0]).all()


def bwd_pos_rays(tag, tb, n, B, pts, query, gd, g_ld, which, accumulate=None):
    """(grad_o, grad_d) [B, 3] (None when not asked for: its guarded buffer must stay untouched); the
    workspace is guarded beyond its 12 n bytes."""
    p = params(tag, query)
    bufs = {k: Guarded(B * 3) for k in "od"}
    if accumulate is not None:
        for k in which:
            bufs[k].body.copy_(dev(accumulate[k]).view(-1))
    ws = Guarded(3 * n)
    st = lib().nerf_hashgrid_bwd_pos(ctypes.byref(p), *pts.args(n), tb.ptr(), gd.data_ptr(), g_ld, None,
                                     bufs["o"].ptr() if "o" in which else None, bufs["d"].ptr() if "d" in which else None,
                                     int(accumulate is not None), ws.ptr(), 12 * n, stream())
    assert st == OK, st
    for k in "od":
        bufs[k].check(f"grad_{k} {tag} n={n} which={which}", written=k in which)
    ws.check(f"workspace {tag} n={n}")
    tb.check()
    return tuple(bufs[k].body.view(B, 3).cpu().numpy() if k in which else None for k in "od")


@pytest.mark.parametrize("tag", TAGS)
def test_position_gradient_ray_form_within_the_derived_bound(tag):
    res, T, F, primes, normalize = R.cfg_args(tag)
    tabs = R.tables(tag)
    tb, B = Table(tabs), RAY_B
    for S in (1, 3, 64, 65):
        n = B * S
        o, d, t0, t1 = R.rays(tag, B, S)
        g = R.grads(tag, n)
        gd = padded(g)
        pts = Points(rays=(o, d, t0, t1), S=S)
        for query in (0, 1):
            pos = R.ray_positions(o, d, t0, t1, S, query)
            ref, bound = R.pos_grad64_with_bound(pos, tabs, res, T, g, primes, normalize)
            assert bound.max() <= 1e-4 * np.abs(ref).max()          # per sample; a ray's bound is their sum
            ref_o, bound_o, ref_d, bound_d = R.ray_grad64_with_bound(ref, bound, R.ray_query(t0, t1, query), B, S)
            go, gdd = bwd_pos_rays(tag, tb, n, B, pts, query, gd, g.shape[1] + 3, "od")
            report(f"grad_o {tag} S={S} query={query}", go, ref_o, bound_o)
            report(f"grad_d {tag} S={S} query={query}", gdd, ref_d, bound_d)
            only_o = bwd_pos_rays(tag, tb, n, B, pts, query, gd, g.shape[1] + 3, "o")
            only_d = bwd_pos_rays(tag, tb, n, B, pts, query, gd, g.shape[1] + 3, "d")
            assert only_o[1] is None and only_d[0] is None
            assert same_bits(only_o[0], go) and same_bits(only_d[1], gdd)
            rng = np.random.default_rng(S)
            base = {k: rng.standard_normal((B, 3)).astype(np.float32) for k in "od"}
            ao, ad = bwd_pos_rays(tag, tb, n, B, pts, query, gd, g.shape[1] + 3, "od", accumulate=base)
            assert same_bits(ao, base["o"] + go) and same_bits(ad, base["d"] + gdd)


# ----------------------------------------------------------------------------- arguments
def test_bad_arguments_return_before_any_launch_and_leave_the_guards():
    from nerf_amd import kernels as K
    tag, n, S = "A", 8, 4
    L, F, cols = dims(tag)
    tb = Table(R.tables(tag))
    x, g = dev(R.points(tag, n)), dev(R.grads(tag, n))
    o, d, t0, t1 = (dev(a) for a in R.rays(tag, n // S, S))
    good = params(tag)
    rows = K.hashgrid_table_rows(good)
    need = K.hashgrid_workspace_bytes(good)
    ws = garbage(need + 512, 3)
    before = ws.clone()
    out, gt, gx, go, gd, pw = Guarded(n * cols), Guarded(rows * F), Guarded(n * 3), Guarded(6), Guarded(6), Guarded(3 * n)
    Lb, s = lib(), stream()
    X = (x.data_ptr(), None, None, None, None)
    RAYS = (None, o.data_ptr(), d.data_ptr(), t0.data_ptr(), t1.data_ptr())

    def bad(**kw):
        p = params(tag)
        for k, v in kw.items():
            setattr(p, k, v)
        return ctypes.byref(p)

    def f(p=None, pos=X, n_=n, spr=1, ld=cols):
        return Lb.nerf_hashgrid_fwd(p or ctypes.byref(good), *pos, n_, spr, tb.ptr(), out.ptr(), ld, s)

    def b(p=None, pos=X, n_=n, spr=1, ld=cols, w=ws.data_ptr(), wb=need):
        return Lb.nerf_hashgrid_bwd(p or ctypes.byref(good), *pos, n_, spr, g.data_ptr(), ld, gt.ptr(), 0, w, wb, s)

    def q(p=None, pos=X, n_=n, spr=1, ld=cols, outs=None, w=None, wb=0):
        outs = (gx.ptr(), None, None) if outs is None else outs
        return Lb.nerf_hashgrid_bwd_pos(p or ctypes.byref(good), *pos, n_, spr, tb.ptr(), g.data_ptr(), ld, *outs, 0, w, wb, s)

    RO = (None, go.ptr(), gd.ptr())
    calls = []
    for kw in (dict(levels=0), dict(levels=33), dict(features=0), dict(features=9), dict(normalize=2), dict(query=2)):
        pb = bad(**kw)
        calls += [(INVALID, f(pb)), (INVALID, b(pb)), (INVALID, q(pb))]
    no_end = RAYS[:4] + (None,)
    calls += [
        (INVALID, f(ld=cols - 1)), (INVALID, b(ld=cols - 1)), (INVALID, q(ld=cols - 1)),
        # ray form, midpoint query, no t_end
        (INVALID, f(pos=no_end, spr=S)), (INVALID, b(pos=no_end, spr=S)),
        (INVALID, q(pos=no_end, spr=S, outs=RO, w=pw.ptr(), wb=12 * n)),
        (INVALID, f(pos=RAYS, spr=0)), (INVALID, b(pos=RAYS, spr=0)),
        # grad_x together with grad_o; ray outputs for explicit points; no output at all
        (INVALID, q(outs=(gx.ptr(), go.ptr(), None))),
        (INVALID, q(pos=RAYS, spr=S, outs=(gx.ptr(), go.ptr(), None), w=pw.ptr(), wb=12 * n)),
        (INVALID, q(pos=RAYS, spr=S, outs=(None, None, None), w=pw.ptr(), wb=12 * n)),
        # a last ray cut short
        (INVALID, q(pos=RAYS, n_=n - 1, spr=S, outs=RO, w=pw.ptr(), wb=12 * n)),
        # workspaces: short, missing, misaligned
        (WORKSPACE, b(wb=need - 1)), (WORKSPACE, q(pos=RAYS, spr=S, outs=RO, w=pw.ptr(), wb=12 * n - 1)),
        (WORKSPACE, q(pos=RAYS, spr=S, outs=RO, w=None, wb=12 * n)),
        (INVALID, b(w=None)), (INVALID, b(w=ws.data_ptr() + 16, wb=need + 256)),
        (INVALID, q(pos=RAYS, spr=S, outs=RO, w=pw.ptr() + 4, wb=12 * n)),
        # null data pointers with n > 0
        (INVALID, f(pos=(None,) * 5)), (INVALID, b(pos=(None,) * 5)), (INVALID, q(pos=(None,) * 5, outs=RO, w=pw.ptr(), wb=12 * n)),
        (INVALID, f(n_=-1)), (INVALID, b(n_=-1)), (INVALID, q(n_=-1)),
        # n == 0 succeeds whatever the data pointers are, and stores nothing here (accumulate = 0 only
        # clears grad_table: checked in test_empty_batch_through_the_c_abi)
        (OK, f(n_=0)), (OK, q(n_=0)), (OK, q(pos=RAYS, n_=0, spr=S, outs=RO, w=pw.ptr(), wb=0)),
    ]
    torch.cuda.synchronize()
    for i, (want, got) in enumerate(calls):
        assert got == want, (i, want, got)
    for name, buf in (("out", out), ("grad_table", gt), ("grad_x", gx), ("grad_o", go), ("grad_d", gd), ("workspace", pw)):
        buf.check(name, written=False)
    assert torch.equal(ws, before)
    tb.check()


def test_empty_batch_through_the_c_abi():
    """n_samples == 0 with every data pointer NULL: NERF_OK from all three entry points.  Nothing is
    stored, except that a non-accumulating nerf_hashgrid_bwd clears grad_table."""
    from nerf_amd import kernels as K
    Lb, s = lib(), stream()
    for tag in ("A", "B", "H"):
        L, F, cols = dims(tag)
        p = params(tag)
        nul = (None,) * 5
        assert Lb.nerf_hashgrid_fwd(ctypes.byref(p), *nul, 0, 1, None, None, cols, s) == OK
        assert Lb.nerf_hashgrid_bwd(ctypes.byref(p), *nul, 0, 1, None, cols, None, 0, None, 0, s) == OK
        assert Lb.nerf_hashgrid_bwd_pos(ctypes.byref(p), *nul, 0, 1, None, None, cols, None, None, None, 0, None, 0, s) == OK
        rows = K.hashgrid_table_rows(p)
        base = np.random.default_rng(0).standard_normal((rows, F)).astype(np.float32)
        for accumulate in (0, 1):
            for w in (None, garbage(K.hashgrid_workspace_bytes(p), 4)):
                gt = Guarded(rows * F)
                gt.body.copy_(dev(base).view(-1))
                st = Lb.nerf_hashgrid_bwd(ctypes.byref(p), *nul, 0, 1, None, cols, gt.ptr(), accumulate,
                                          None if w is None else w.data_ptr(), 0 if w is None else w.numel() * 8, s)
                assert st == OK
                gt.check(f"empty {tag}")
                assert same_bits(gt.body.view(rows, F).cpu().numpy(), base if accumulate else np.zeros_like(base))
        # a workspace that is given is still checked
        w = garbage(K.hashgrid_workspace_bytes(p), 5)
        assert Lb.nerf_hashgrid_bwd(ctypes.byref(p), *nul, 0, 1, None, cols, None, 0, w.data_ptr(), 8, s) == WORKSPACE
        assert Lb.nerf_hashgrid_bwd(ctypes.byref(p), *nul, 0, 1, None, cols - 1, None, 0, None, 0, s) == INVALID


def test_empty_batch_through_the_modules():
    from nerf_amd.model_ingp import INGPEncoding, INGPTable
    torch.manual_seed(0)
    table = INGPTable(25, 2 ** 10, 2, 1, 2654435761, 805459861).to(DEV)
    enc = INGPEncoding(64, 4, 2 ** 10, 2, 4).to(DEV)
    for module, width in ((table, 2), (enc, 8)):
        out = module(torch.zeros(0, 3, device=DEV))
        assert out.shape == (0, width) and out.device.type == "cuda"
        out.sum().backward()
        tables = [table.table] if module is table else [e.table for e in enc.encodings]
        for t in tables:
            assert t.grad is not None and t.grad.shape == t.shape and not t.grad.any()
            t.grad = None
    xg = torch.zeros(0, 3, device=DEV, requires_grad=True)
    (enc(xg) * 2).sum().backward()
    assert xg.grad is None or (xg.grad.shape == (0, 3))
    S = 4
    og, dg = (torch.zeros(0, 3, device=DEV, requires_grad=True) for _ in range(2))
    t = torch.zeros(0, S, device=DEV)
    feat = enc.encode_rays(og, dg, t, t, None, S, 1)
    assert feat.shape == (0, enc.padded_dim)
    feat.sum().backward()
    for e in enc.encodings:
        assert e.table.grad is not None and e.table.grad.shape == e.table.shape and not e.table.grad.any()
    # and a batch after the empty one is served as before
    x = R.points("A", 65)
    tabs = [e.table.detach().cpu().numpy() for e in enc.encodings]
    got = enc(dev(x)).detach().cpu().numpy()
    assert same_bits(got, O.encode(x, tabs, enc.resolutions, 2 ** 10))
