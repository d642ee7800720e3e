"""The encoding forward kernels (csrc/encode.hip: nerf_encode_fwd's encode_fwd_lds_kernel and
encode_fwd_kernel, nerf_encode_rays) at their edge shapes, against the fp64 restatement and its
derived per-column bound (_encode_fwd_ref.py; the cases and inputs are defined there and checked on
the CPU by test_encode_fwd_ref.py).  Every case is a few hundred rows at the most.

Each case runs through every layout that reaches another code path:

    lds       ld = out_dim rounded up to 4          encode_fwd_lds_kernel, Q = ld / 4 (1 at 0 levels)
    lds128    ld = 128                              encode_fwd_lds_kernel, Q = 32
    quad132   ld = 132                              encode_fwd_kernel, 16-byte stores, Q = 33, RB = 7
    scalar    ld = out_dim + 1 or + 2, ld % 4 != 0  encode_fwd_kernel, scalar stores
    quad516   ld = 516                              encode_fwd_kernel, Q = 129, RB = 1: 127 idle threads
    offset    ld as lds, out 4 bytes past a 16-byte boundary: encode_fwd_kernel, scalar stores

and holds every cos / sin column to its bound (identity columns and masked columns bit for bit),
the pad columns to zero, the guards of the output buffer (_guarded.py) to their bytes, and all
layouts to the bits of the first.  The largest err / bound is printed per case and layout.

Measured on an MI355X, the largest err / bound over all cases (the two kernels store the same bits
in every case, so one figure serves both encode_fwd_lds_kernel and encode_fwd_kernel):

    nerf_encode_fwd, ray mode        kind 0: 0.42 (k0_L11_id_q0)       kind 1: 0.22 (k1_diag_s0_L10_id_narrow)
    nerf_encode_fwd, explicit x      kind 0: 0.45 (k0_L16_noid_n64)    kind 1: 0.19 (k1_L16_id_dist_s0_n64)
    nerf_encode_rays                 0.35 (the directions of k0_L16)
    0 levels (identity columns only, bound 0): bit-equal

Kind 0's 0.45 of 2e-7 is the shared sin / cos's own 9.5e-8 (test_sincos_host.py); kind 1's bound is
led by the N_VB x term, which only the two td^4 would use up.  Identity columns and masked columns
are bit-equal to the restatement in every case and layout.

What this file sees and the earlier encoding tests do not, tried on a scratch build: with the
thread mapping's threshold off by one (TPR = tl <= 33 ? 32 : 64, so that at 11 levels column 32 of
the cos and of the sin block is never written) twelve tests here fail, every case of 11 levels, and
the 213 tests of test_gpu_parity, test_gpu_mip_pose_feed, test_gpu_sincos_range,
test_gpu_fused_encoding, test_gpu_encode_bwd_edges and test_gpu_garf_ipe pass.  (The weight formed
with 2^k for 4^k at every level count fails seventeen tests here, and the golden vectors at 10
levels as well.)
"""
import ctypes
import dataclasses
import functools

import pytest
import torch

import _encode_fwd_ref as F
from _guarded import GUARD, SENTINEL, Guarded

pytestmark = pytest.mark.gpu

DEV = "cuda"
RAYS = F.by_name(F.RAY_CASES)
SAMPLES = F.by_name(F.SAMPLE_CASES)
OK, INVALID = 0, -1


@pytest.fixture(scope="module", autouse=True)
def _lib():
    import nerf_amd
    nerf_amd._lib.load()
    yield


@functools.lru_cache(maxsize=None)
def _case(name):
    if name in RAYS:
        c = RAYS[name]
        inp, ref = F.ray_case(c)
    else:
        c = SAMPLES[name]
        inp, ref = F.sample_case(c)
    return c, inp, ref


def _params(c):
    from nerf_amd import kernels as K
    return K.make_pe_params(c.kind, c.levels, c.identity, c.scale, query=c.query, pixel_width_sigma=c.sigma,
                            distribute_variance=c.distribute, pw_mode=c.pw_mode, mask=c.mask())


def _stream():
    from nerf_amd import kernels as K
    return K._stream(torch.device(DEV))


def _dev(t):
    return t.to(DEV).contiguous()


def layouts(out_dim):
    """(name, ld, byte offset of out from a 16-byte boundary)."""
    ld4 = (out_dim + 3) // 4 * 4
    odd = out_dim + 1 if (out_dim + 1) % 4 else out_dim + 2
    return [("lds", ld4, 0), ("lds128", 128, 0), ("quad132", 132, 0), ("scalar", odd, 0), ("quad516", 516, 0),
            ("offset", ld4, 4)]


def run_fwd(c, inp, ld, offset=0, x=None):
    """nerf_encode_fwd through the C entry point into a guarded buffer: the [N, ld] rows on the CPU.
    Ray mode for a case of RAY_CASES, explicit positions (x overrides the case's) otherwise."""
    import nerf_amd
    lib = nerf_amd._lib.load()
    p = _params(c)
    n = c.n_rays * c.samples
    shift = offset // 4
    named = torch.ones(n * ld + shift, dtype=torch.bool)
    named[:shift] = False
    out = Guarded(n * ld + shift, named=named)
    assert out.ptr() % 16 == 0
    ptr = lambda t: None if t is None else t.data_ptr()
    t0 = t1 = pw = xs = xd = o = d = None
    if c.name in RAYS:
        o, d, t0 = _dev(inp["o"]), _dev(inp["d"]), _dev(inp["t0"])
        t1 = None if c.t_end_null else _dev(inp["t1"])
    else:
        xs = _dev(inp["x"] if x is None else x)
        if c.kind == 1:
            xd, t0, t1 = _dev(inp["d"]), _dev(inp["t0"]), _dev(inp["t1"])
    if c.kind == 1:
        pw = _dev(inp["pw"])
    st = lib.nerf_encode_fwd(ctypes.byref(p), ptr(xs), ptr(xd), ptr(o), ptr(d), ptr(t0), ptr(t1), ptr(pw), n,
                             c.samples, c.n_rays, out.ptr() + offset, ld, _stream())
    assert st == OK, st
    torch.cuda.synchronize()
    out.check(f"nerf_encode_fwd {c.name} ld {ld} offset {offset}")
    return out.body[shift:].cpu().view(n, ld).clone()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def check_rows(c, ref, rows, what):
    """Columns against the bound (bound 0: exact, the identity columns bit for bit), pads zero; the
    largest err / bound."""
    od = c.out_dim
    got = rows[:, :od]
    assert torch.isfinite(got).all(), what
    assert (_bits(rows[:, od:]) == 0).all(), f"{what}: pad columns"
    err = (got.double() - ref.ref).abs()
    zero = ref.bound == 0
    assert (err[zero] == 0).all(), f"{what}: a masked or identity column is off"
    if c.identity:
        assert ref.ident.dtype == torch.float32
        assert _same(got[:, :3], ref.ident), f"{what}: identity columns"
    return torch.where(zero, torch.zeros_like(err), err / ref.bound).max().item()


@pytest.mark.parametrize("name", list(RAYS) + list(SAMPLES))
def test_forward_against_reference(name):
    """Ray mode: every ray case (levels {0, 1, 10, 11, 16} with and without identity; tiles of 1, 2, 5,
    6, 10 and 18 rows and 195, 260 and 585 rows over several tiles; query 0 / 1, t_end NULL; masks;
    both variance forms, sigma 0 / 0.7; pw_mode 0 / 1 / 2; an empty interval).  Explicit positions: the
    same level / identity set for each kind at 1, 63, 64, 65 and 129 rows.  Every layout within the
    bound, pads zero, guards intact, all layouts bitwise the first, a second launch bitwise the first."""
    c, inp, ref = _case(name)
    first = None
    worst = {}
    for lname, ld, offset in layouts(c.out_dim):
        rows = run_fwd(c, inp, ld, offset)
        worst[lname] = check_rows(c, ref, rows, f"{name} {lname}")
        if first is None:
            first = rows[:, :c.out_dim]
            assert _same(run_fwd(c, inp, ld, offset)[:, :c.out_dim], first), f"{name}: not repeatable"
        else:
            assert _same(rows[:, :c.out_dim], first), f"{name}: {lname} differs from the first layout"
    print(f"encode_fwd {name} (kind {c.kind}): max err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0


@pytest.mark.parametrize("name", ["k0_L16", "k0_L11_id_q0", "k1_diag_s0_L10_id_pw0", "k0_L1_q0"])
def test_encode_rays_against_reference(name):
    """nerf_encode_rays (plain Fourier features of explicit rows) on a case's directions, its levels,
    scale and identity, in an LDS and a per-quad layout: the kind-0 restatement's bound."""
    import nerf_amd
    lib = nerf_amd._lib.load()
    src, inp, _ = _case(name)
    c = dataclasses.replace(src, kind=0, samples=1, alpha=None, name=name + "_dirs")
    ref = F.fwd_ref(c, F.sample_quantities(c, {"x": inp["d"]}))
    p = _params(c)
    d = _dev(inp["d"])
    first = None
    for ld in ((c.out_dim + 3) // 4 * 4, 132):
        out = Guarded(c.n_rays * ld)
        assert lib.nerf_encode_rays(ctypes.byref(p), d.data_ptr(), c.n_rays, out.ptr(), ld, _stream()) == OK
        torch.cuda.synchronize()
        out.check(f"nerf_encode_rays {name} ld {ld}")
        rows = out.body.cpu().view(c.n_rays, ld).clone()
        r = check_rows(c, ref, rows, f"encode_rays {name} ld {ld}")
        print(f"encode_rays {name} ld {ld}: max err / bound {r:.3f}")
        assert r <= 1.0
        first = rows[:, :c.out_dim] if first is None else first
        assert _same(rows[:, :c.out_dim], first)
    # kind 1 is not this entry point's
    p.kind = 1
    out = Guarded(c.n_rays * 132)
    assert lib.nerf_encode_rays(ctypes.byref(p), d.data_ptr(), c.n_rays, out.ptr(), 132, _stream()) == INVALID
    torch.cuda.synchronize()
    out.check("refused nerf_encode_rays", written=False)


@pytest.mark.parametrize("name", ["k0_L11_noid_n1", "k0_L16_id_n63", "k1_L11_noid_diag_s0.7_n63",
                                  "k1_L10_noid_dist_s0.7_n129", "k1_L16_noid_dist_s0.7_n65_mask"])
def test_nan_position_stays_in_its_row(name):
    """A NaN position makes every encoded column of its row NaN (a masked column too: 0 * NaN) and
    leaves every other row bitwise unchanged, in the LDS and in the per-quad kernel."""
    c, inp, _ = _case(name)
    bad = c.n_rays // 3
    x = inp["x"].clone()
    x[bad] = float("nan")
    keep = torch.arange(c.n_rays) != bad
    for lname, ld, offset in layouts(c.out_dim)[:3]:
        clean = run_fwd(c, inp, ld, offset)
        rows = run_fwd(c, inp, ld, offset, x=x)
        assert torch.isnan(rows[bad, :c.out_dim]).all(), lname
        assert (_bits(rows[bad, c.out_dim:]) == 0).all(), lname
        assert _same(rows[keep], clean[keep]), lname


def test_argument_contract():
    """What nerf_encode_fwd refuses it refuses before any launch (the output keeps its bytes), and 0
    samples are OK and touch nothing."""
    import nerf_amd
    lib = nerf_amd._lib.load()
    c, inp, _ = _case("k1_diag_s0_L10_id_pw0")
    n = c.n_rays * c.samples
    o, d, t0, t1, pw = (_dev(inp[k]) for k in ("o", "d", "t0", "t1", "pw"))
    x = _dev(torch.zeros(n, 3))
    out = Guarded(n * 1028)

    def call(p, *, x=None, xdir=None, o=o.data_ptr(), d=d.data_ptr(), t0=t0.data_ptr(), t1=t1.data_ptr(),
             pw=pw.data_ptr(), n=n, ld=64, dst=out.ptr()):
        return lib.nerf_encode_fwd(ctypes.byref(p), x, xdir, o, d, t0, t1, pw, n, c.samples, c.n_rays, dst, ld,
                                   _stream())

    def params(**kw):
        p = _params(c)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    assert c.out_dim == 63
    assert call(params(levels=17), ld=128) == INVALID
    assert call(params(levels=-1)) == INVALID
    assert call(params(), ld=62) == INVALID                      # out_ld < out_dim
    assert call(params(), ld=1028) == INVALID
    assert call(params(), pw=None) == INVALID                    # kind 1 without pixel widths
    assert call(params(), t1=None) == INVALID                    # kind 1 without t_end
    assert call(params(pw_mode=3)) == INVALID
    assert call(params(kind=2)) == INVALID
    assert call(params(), d=None) == INVALID                     # ray mode without directions
    assert call(params(kind=0), d=None) == INVALID
    assert call(params(kind=0), t1=None) == INVALID              # query 1 without t_end
    assert call(params(), x=x.data_ptr()) == INVALID             # kind 1 on explicit positions without xdir
    assert call(params(levels=0, include_identity=0)) == INVALID
    assert call(params(), dst=None) == INVALID
    assert call(params(), n=-1) == INVALID
    assert call(params(), n=0) == OK
    torch.cuda.synchronize()
    out.check("refused nerf_encode_fwd", written=False)
    # the accepted edges next to the refused ones
    assert call(params(), ld=63) == OK
    assert call(params(), ld=1024) == OK
    torch.cuda.synchronize()
    bits = out.flat.cpu()
    assert (bits[:GUARD] == SENTINEL).all() and (bits[GUARD + n * 1024:] == SENTINEL).all()
    assert (bits[GUARD:GUARD + n * 1024] != SENTINEL).all()
