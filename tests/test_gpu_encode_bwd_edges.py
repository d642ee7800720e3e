"""The encoding backward kernels (csrc/encode.hip: nerf_encode_bwd_rays, nerf_encode_bwd_integrated,
nerf_encode_bwd) at their edge shapes, against the fp64 restatement and its derived bound
(_encode_bwd_ref.py; the cases and inputs are defined there and checked on the CPU by
test_encode_bwd_ref.py).  Every case is a few hundred samples at the most.

The comparisons hold each output to its own bound = sum_i eps_i |T_i| (about 1e-6 of the sum of the
absolute terms) and print the largest err / bound.  Measured on an MI355X:

    nerf_encode_bwd_rays        kind 0: d_origs 0.23, d_dirs 0.29    kind 1: d_origs 0.14, d_dirs 0.08
                                (0 levels, where the bound is the one final fp32 rounding: 0.98 and 0.52)
    nerf_encode_bwd_integrated  dx 0.33, ddir 0.13
    nerf_encode_bwd             dx 0.19
    ray kernel against the per-sample kernels: 0.02 of the two bounds' sum

The bitwise properties (one output against both, accumulate, NaN pads in a wider row stride,
repeatability, NaN isolation) compare the kernel with itself; outputs lie in guarded buffers
(_guarded.py)."""
import ctypes
import functools

import pytest
import torch

import _encode_bwd_ref as R
from _guarded import Guarded

pytestmark = pytest.mark.gpu

DEV = "cuda"
RAYS = R.by_name(R.RAY_CASES)
INTEGRATED = R.by_name(R.INTEGRATED_CASES)
FOURIER = R.by_name(R.FOURIER_CASES)
INVALID, UNSUPPORTED = -1, -2

# the cases the bitwise properties run on: both kinds, one and two column slots, a ragged last block
SOME_RAYS = ["k0_L10_q0_null", "k0_L16_id_mask", "k1_diag_s07_L16_pw1", "k1_dist_s0_L11_id_pw2",
             "k1_diag_s0_L10_id_pw0"]
SOME_INTEGRATED = [c.name for c in R.INTEGRATED_CASES if c.levels in (11, 16)]       # diagonal and distributed


@pytest.fixture(scope="module", autouse=True)
def _lib():
    import nerf_amd
    nerf_amd._lib.load()
    yield


@functools.lru_cache(maxsize=None)
def _ray_case(name):
    c = RAYS[name]
    inp = R.ray_inputs(c)
    return c, inp, R.rays_ref(c, inp)


@functools.lru_cache(maxsize=None)
def _sample_case(name):
    c = INTEGRATED[name] if name in INTEGRATED else FOURIER[name]
    inp = R.sample_inputs(c)
    if c.kind == 1:
        return c, inp, R.integrated_ref(c, inp["x"], inp["d"], inp["t0"], inp["t1"], inp["pw"], inp["g"])
    return c, inp, R.fourier_ref(c, inp["x"], inp["g"])


def _params(c):
    from nerf_amd import kernels as K
    return K.make_pe_params(c.kind, c.levels, c.identity, c.scale, query=c.query, pixel_width_sigma=c.sigma,
                            distribute_variance=c.distribute, pw_mode=c.pw_mode, mask=c.mask())


def _stream():
    from nerf_amd import kernels as K
    return K._stream(torch.device(DEV))


def _dev(t):
    return t.to(DEV).contiguous()


def _grad_rows(g, ld, pad):
    """g [N, out_dim] in rows of stride ld, the pad columns holding `pad`."""
    buf = torch.full((g.shape[0], ld), pad, dtype=torch.float32, device=DEV)
    buf[:, :g.shape[1]] = g.to(DEV)
    return buf


def strided_ld(out_dim):
    return (out_dim + 31) // 32 * 32 + 8


def _outputs(n, want, preset):
    outs = []
    for i, w in enumerate(want):
        b = Guarded(3 * n) if w else None
        if b is not None and preset is not None:
            b.body.copy_(preset[i].reshape(-1).to(DEV))
        outs.append(b)
    return outs


def _collect(outs, n, what):
    torch.cuda.synchronize()
    res = []
    for b in outs:
        if b is not None:
            b.check(what)
        res.append(None if b is None else b.body.cpu().view(n, 3).clone())
    return res


def _ptr(b):
    return None if b is None else b.ptr()


def run_rays(c, inp, *, g=None, g_ld=None, pad=0.0, want=(True, True), accumulate=0, preset=None):
    """nerf_encode_bwd_rays through the C entry point, outputs in guarded buffers: (d_origs, d_dirs)
    as CPU [n_rays, 3], None for an output not asked for."""
    import nerf_amd
    lib = nerf_amd._lib.load()
    p = _params(c)
    B, S = c.n_rays, c.samples
    ld = c.out_dim if g_ld is None else g_ld
    gbuf = _grad_rows(inp["g"] if g is None else g, ld, pad)
    o, d, t0 = _dev(inp["o"]), _dev(inp["d"]), _dev(inp["t0"])
    t1 = None if c.t_end_null else _dev(inp["t1"])
    pw = _dev(inp["pw"]) if c.kind == 1 else None
    outs = _outputs(B, want, preset)
    st = lib.nerf_encode_bwd_rays(ctypes.byref(p), o.data_ptr(), d.data_ptr(), t0.data_ptr(),
                                  None if t1 is None else t1.data_ptr(), None if pw is None else pw.data_ptr(),
                                  gbuf.data_ptr(), ld, B, S, _ptr(outs[0]), _ptr(outs[1]), accumulate, _stream())
    assert st == 0, st
    return _collect(outs, B, f"nerf_encode_bwd_rays {c.name}")


def run_integrated(c, inp, *, g_ld=None, pad=0.0, want=(True, True), accumulate=0, preset=None):
    import nerf_amd
    lib = nerf_amd._lib.load()
    p = _params(c)
    n = c.n_rays
    ld = c.out_dim if g_ld is None else g_ld
    gbuf = _grad_rows(inp["g"], ld, pad)
    x, d, t0, t1, pw = (_dev(inp[k]) for k in ("x", "d", "t0", "t1", "pw"))
    outs = _outputs(n, want, preset)
    st = lib.nerf_encode_bwd_integrated(ctypes.byref(p), x.data_ptr(), d.data_ptr(), t0.data_ptr(), t1.data_ptr(),
                                        pw.data_ptr(), gbuf.data_ptr(), ld, n, _ptr(outs[0]), _ptr(outs[1]),
                                        accumulate, _stream())
    assert st == 0, st
    return _collect(outs, n, f"nerf_encode_bwd_integrated {c.name}")


def run_fourier(c, inp, *, g_ld=None, pad=0.0, accumulate=0, preset=None):
    import nerf_amd
    lib = nerf_amd._lib.load()
    p = _params(c)
    n = c.n_rays
    ld = c.out_dim if g_ld is None else g_ld
    gbuf = _grad_rows(inp["g"], ld, pad)
    x = _dev(inp["x"])
    outs = _outputs(n, (True,), None if preset is None else (preset,))
    st = lib.nerf_encode_bwd(ctypes.byref(p), x.data_ptr(), gbuf.data_ptr(), ld, n, _ptr(outs[0]), accumulate,
                             _stream())
    assert st == 0, st
    return _collect(outs, n, f"nerf_encode_bwd {c.name}")[0]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _ratio(got, ref, bound):
    """max err / bound; where the bound is 0 (every term of the output is 0: a zero direction
    component, an empty interval's mu_diff) the output must be exact."""
    assert torch.isfinite(got).all()
    err = (got.double() - ref).abs()
    assert (err[bound == 0] == 0).all()
    return torch.where(bound > 0, err / bound, torch.zeros_like(err)).max().item()


def _preset(n, seed):
    return torch.randn(n, 3, generator=torch.Generator().manual_seed(seed)) * 3.0


# ------------------------------------------------------------------------ nerf_encode_bwd_rays
@pytest.mark.parametrize("name", list(RAYS))
def test_rays_against_reference(name):
    """Every ray case (levels {0, 1, 10, 11, 16} with and without identity: one and two column slots;
    rays {1, 3, 4, 5, 9}; samples {1, 2, 65}; query 0 / 1, t_end NULL; masks; both variance forms,
    sigma 0 / 0.7; pw_mode 0 / 1 / 2; wide and 1 / 555 pixels; non-unit directions; an empty
    interval): each output within its bound, and a second call bitwise the same."""
    c, inp, ref = _ray_case(name)
    d_o, d_d = run_rays(c, inp)
    r_o, r_d = _ratio(d_o, ref.d_o, ref.d_o_bound), _ratio(d_d, ref.d_d, ref.d_d_bound)
    print(f"encode_bwd_rays {name} (kind {c.kind}): max err / bound d_origs {r_o:.3f}, d_dirs {r_d:.3f}; "
          f"max bound / sum|T| {(ref.d_d_bound / ref.d_d_sum).max().item():.2e}")
    assert r_o <= 1.0 and r_d <= 1.0
    again = run_rays(c, inp)
    assert _same(again[0], d_o) and _same(again[1], d_d)


@pytest.mark.parametrize("name", SOME_RAYS)
def test_rays_row_stride_with_nan_pads(name):
    """g_ld = the column count rounded up to 32, plus 8, the pad columns NaN: bitwise the result of
    zero pads and of the dense rows."""
    c, inp, _ = _ray_case(name)
    ld = strided_ld(c.out_dim)
    dense = run_rays(c, inp)
    zero = run_rays(c, inp, g_ld=ld, pad=0.0)
    nan = run_rays(c, inp, g_ld=ld, pad=float("nan"))
    for a, b, d in zip(nan, zero, dense):
        assert torch.isfinite(a).all()
        assert _same(a, b) and _same(a, d)


@pytest.mark.parametrize("name", SOME_RAYS)
def test_rays_one_output(name):
    """d_origs alone and d_dirs alone each equal the joint call bitwise."""
    c, inp, _ = _ray_case(name)
    d_o, d_d = run_rays(c, inp)
    only_o = run_rays(c, inp, want=(True, False))
    only_d = run_rays(c, inp, want=(False, True))
    assert only_o[1] is None and only_d[0] is None
    assert _same(only_o[0], d_o) and _same(only_d[1], d_d)


@pytest.mark.parametrize("name", SOME_RAYS)
def test_rays_accumulate(name):
    """accumulate = 1 on seeded values: bitwise fp32(preset + result at accumulate 0); guards intact."""
    c, inp, _ = _ray_case(name)
    d_o, d_d = run_rays(c, inp)
    pre = (_preset(c.n_rays, 70), _preset(c.n_rays, 71))
    a_o, a_d = run_rays(c, inp, accumulate=1, preset=pre)
    assert _same(a_o, pre[0] + d_o) and _same(a_d, pre[1] + d_d)
    assert not _same(a_o, d_o)
    # accumulate = 0 overwrites whatever was there
    w_o, w_d = run_rays(c, inp, accumulate=0, preset=pre)
    assert _same(w_o, d_o) and _same(w_d, d_d)


@pytest.mark.parametrize("name", ["k0_L11_id_q0", "k1_diag_s07_L16_pw1"])
def test_rays_nan_isolation(name):
    """A NaN in one ray's gradient rows makes that ray's outputs NaN and leaves every other ray
    bitwise unchanged."""
    c, inp, _ = _ray_case(name)
    d_o, d_d = run_rays(c, inp)
    bad = 4
    g = inp["g"].clone()
    g[bad * c.samples:(bad + 1) * c.samples] = float("nan")
    n_o, n_d = run_rays(c, inp, g=g)
    keep = torch.arange(c.n_rays) != bad
    assert _same(n_o[keep], d_o[keep]) and _same(n_d[keep], d_d[keep])
    assert torch.isnan(n_o[bad]).all() and torch.isnan(n_d[bad]).all()


def test_rays_refusals():
    """Both outputs NULL, a 0-level encoding without identity columns, and query 1 / kind 1 without
    t_end are refused before any launch; the outputs keep their bytes."""
    import nerf_amd
    lib = nerf_amd._lib.load()
    c, inp, _ = _ray_case("k0_L10_q0_null")
    o, d, t0, t1, g = (_dev(inp[k]) for k in ("o", "d", "t0", "t1", "g"))
    outs = _outputs(c.n_rays, (True, True), None)

    def call(p, t_end, d_o, d_d, ld):
        return lib.nerf_encode_bwd_rays(ctypes.byref(p), o.data_ptr(), d.data_ptr(), t0.data_ptr(), t_end, None,
                                        g.data_ptr(), ld, c.n_rays, c.samples, d_o, d_d, 0, _stream())

    p = _params(c)
    assert call(p, None, None, None, c.out_dim) == INVALID
    p.query = 1
    assert call(p, None, outs[0].ptr(), outs[1].ptr(), c.out_dim) == INVALID
    p.query = 0
    p.levels = 0
    assert call(p, None, outs[0].ptr(), outs[1].ptr(), c.out_dim) == INVALID
    p.levels = 10
    assert call(p, None, outs[0].ptr(), outs[1].ptr(), c.out_dim - 1) == INVALID
    p.kind = 1
    assert call(p, t1.data_ptr(), outs[0].ptr(), outs[1].ptr(), c.out_dim) == INVALID       # no pixel widths
    torch.cuda.synchronize()
    for b in outs:
        b.check("refused nerf_encode_bwd_rays", written=False)


@pytest.mark.parametrize("name", ["k0_L10_id_mask", "k0_L11_id_q0", "k1_diag_s0_L10_id_pw0", "k1_diag_s0_L16_id_pw1",
                                  "k1_dist_s0_L11_id_pw2", "k1_diag_s07_L11_id_S65_pw2"])
def test_restated_position_is_the_device_position(name):
    """The anchor: the restated pm (fp32-formed, kind 1 mean-shifted) equals bitwise the identity
    columns of nerf_encode_fwd on the same rays."""
    from nerf_amd import kernels as K
    c, inp, ref = _ray_case(name)
    out = K.encode_fwd(_params(c), c.out_dim, ray_o=_dev(inp["o"]), ray_d=_dev(inp["d"]), t_start=_dev(inp["t0"]),
                       t_end=_dev(inp["t1"]), pixel_width=_dev(inp["pw"]) if c.kind == 1 else None,
                       n_samples=c.n_rays * c.samples, samples_per_ray=c.samples, n_rays=c.n_rays, device=DEV)
    assert ref.pm.dtype == torch.float32
    assert _same(out[:, :3].cpu(), ref.pm)


@pytest.mark.parametrize("name", ["k0_L10_id_mask", "k0_L11_id_q0", "k0_L16", "k1_diag_s0_L10_id_pw0",
                                  "k1_diag_s07_L16_pw1", "k1_dist_s0_L11_id_pw2", "k1_diag_s07_L11_mask_pw2"])
def test_rays_against_the_per_sample_kernels(name):
    """nerf_encode_bwd / nerf_encode_bwd_integrated on the same (fp32-formed) positions: the fp64
    segment sums sum_s dx and sum_s (tq dx + ddir) agree with the ray kernel within the sum of the
    two bounds."""
    import dataclasses
    c, inp, ref = _ray_case(name)
    B, S = c.n_rays, c.samples
    d_o, d_d = run_rays(c, inp)
    cs = dataclasses.replace(c, n_rays=B * S, samples=1, pw_mode=2)
    dv = inp["d"].repeat_interleave(S, dim=0)
    per = {"x": ref.pos, "d": dv, "t0": inp["t0"].reshape(-1), "t1": inp["t1"].reshape(-1),
           "pw": R.expand_pw(inp["pw"], c.pw_mode, B, S), "g": inp["g"]}
    tq = ref.tq.double().unsqueeze(1)
    if c.kind == 1:
        dx, ddir = run_integrated(cs, per)
        sref = R.integrated_ref(cs, per["x"], per["d"], per["t0"], per["t1"], per["pw"], per["g"])
        per_d = tq * dx.double() + ddir.double()
        per_d_bound = tq.abs() * sref.dx_bound + sref.ddir_bound
    else:
        dx = run_fourier(cs, per)
        sref = R.fourier_ref(cs, per["x"], per["g"])
        per_d = tq * dx.double()
        per_d_bound = tq.abs() * sref.dx_bound
    seg = lambda v: v.reshape(B, S, 3).sum(1)
    r_o = ((d_o.double() - seg(dx.double())).abs() / (ref.d_o_bound + seg(sref.dx_bound))).max().item()
    r_d = ((d_d.double() - seg(per_d)).abs() / (ref.d_d_bound + seg(per_d_bound))).max().item()
    print(f"{name}: ray kernel against per-sample kernel, max diff / (bound + bound): d_origs {r_o:.3f}, "
          f"d_dirs {r_d:.3f}")
    assert r_o <= 1.0 and r_d <= 1.0


@pytest.mark.parametrize("kind", [0, 1])
def test_rays_autograd_one_input(kind):
    """encode_rays with requires_grad on the origins only, then on the directions only, gives the
    values of the kernel call with both outputs."""
    from nerf_amd import BarfPositionalEncoding, IntegratedFourierFeatures
    name = "k0_L10_id_mask" if kind == 0 else "k1_diag_s0_L10_id_pw0"
    c, inp, _ = _ray_case(name)
    if kind == 0:
        enc = BarfPositionalEncoding(c.levels, c.alpha, 0, 1, c.identity, c.scale)
    else:
        enc = IntegratedFourierFeatures(c.levels, c.scale, c.identity, c.distribute)
        enc.pixel_width_sigma = c.sigma
    enc = enc.to(DEV)
    ld = enc.padded_dim
    d_o, d_d = run_rays(c, inp, g_ld=ld)
    gpad = _grad_rows(inp["g"], ld, 0.0)
    for which, want in (("o", d_o), ("d", d_d)):
        o, d = _dev(inp["o"]), _dev(inp["d"])
        leaf = (o if which == "o" else d).requires_grad_(True)
        out = enc.encode_rays(o, d, _dev(inp["t0"]), _dev(inp["t1"]), _dev(inp["pw"]), c.samples, c.query, c.pw_mode)
        assert out.shape == (c.n_rays * c.samples, ld)
        out.backward(gpad)
        other = d if which == "o" else o
        assert other.grad is None
        assert _same(leaf.grad.cpu(), want)


# ------------------------------------------------------------------ nerf_encode_bwd_integrated
@pytest.mark.parametrize("name", list(INTEGRATED))
def test_integrated_against_reference(name):
    """Levels {0, 1, 10, 11, 16} with and without identity, both variance forms, sigma 0 / 0.7, wide
    pixels, non-unit directions, 1 / 255 / 256 / 257 samples: dx and ddir within their bounds."""
    c, inp, ref = _sample_case(name)
    dx, ddir = run_integrated(c, inp)
    r_x, r_d = _ratio(dx, ref.dx, ref.dx_bound), _ratio(ddir, ref.ddir, ref.ddir_bound)
    print(f"encode_bwd_integrated {name}: max err / bound dx {r_x:.3f}, ddir {r_d:.3f}; max bound / sum|T| "
          f"{(ref.ddir_bound / ref.ddir_sum.clamp_min(1e-300)).max().item():.2e}")
    assert r_x <= 1.0 and r_d <= 1.0


@pytest.mark.parametrize("name", SOME_INTEGRATED)
def test_integrated_bitwise_properties(name):
    """dx alone and ddir alone each equal the joint call bitwise; so do NaN pads in a wider row stride;
    accumulate = 1 gives fp32(preset + result)."""
    c, inp, _ = _sample_case(name)
    dx, ddir = run_integrated(c, inp)
    only_x = run_integrated(c, inp, want=(True, False))
    only_d = run_integrated(c, inp, want=(False, True))
    assert only_x[1] is None and only_d[0] is None
    assert _same(only_x[0], dx) and _same(only_d[1], ddir)
    nan = run_integrated(c, inp, g_ld=strided_ld(c.out_dim), pad=float("nan"))
    assert _same(nan[0], dx) and _same(nan[1], ddir)
    pre = (_preset(c.n_rays, 72), _preset(c.n_rays, 73))
    a_x, a_d = run_integrated(c, inp, accumulate=1, preset=pre)
    assert _same(a_x, pre[0] + dx) and _same(a_d, pre[1] + ddir)
    a_d_only = run_integrated(c, inp, want=(False, True), accumulate=1, preset=pre)
    assert _same(a_d_only[1], pre[1] + ddir)


def test_integrated_refusals():
    import nerf_amd
    lib = nerf_amd._lib.load()
    c, inp, _ = _sample_case(SOME_INTEGRATED[0])
    x, d, t0, t1, pw, g = (_dev(inp[k]) for k in ("x", "d", "t0", "t1", "pw", "g"))
    out = Guarded(3 * c.n_rays)

    def call(p, dx, ddir):
        return lib.nerf_encode_bwd_integrated(ctypes.byref(p), x.data_ptr(), d.data_ptr(), t0.data_ptr(),
                                              t1.data_ptr(), pw.data_ptr(), g.data_ptr(), c.out_dim, c.n_rays, dx,
                                              ddir, 0, _stream())

    p = _params(c)
    assert call(p, None, None) == INVALID
    p.levels, p.include_identity = 0, 0
    assert call(p, out.ptr(), None) == INVALID
    torch.cuda.synchronize()
    out.check("refused nerf_encode_bwd_integrated", written=False)


# ----------------------------------------------------------------------------- nerf_encode_bwd
@pytest.mark.parametrize("name", list(FOURIER))
def test_fourier_against_reference(name):
    """0 (identity only), 1 and 11 levels with and without identity, masks, 1 / 85 / 86 samples (3 n
    either side of a block): dx within its bound; the strided rows with NaN pads and accumulate = 1
    bitwise."""
    c, inp, ref = _sample_case(name)
    dx = run_fourier(c, inp)
    r = _ratio(dx, ref.dx, ref.dx_bound)
    print(f"encode_bwd {name}: max err / bound dx {r:.3f}; max bound / sum|T| "
          f"{(ref.dx_bound / ref.dx_sum).max().item():.2e}")
    assert r <= 1.0
    assert _same(run_fourier(c, inp, g_ld=strided_ld(c.out_dim), pad=float("nan")), dx)
    pre = _preset(c.n_rays, 74)
    assert _same(run_fourier(c, inp, accumulate=1, preset=pre), pre + dx)
    assert _same(run_fourier(c, inp, accumulate=0, preset=pre), dx)


def test_fourier_refusals():
    """Kind 1 is NERF_ERR_UNSUPPORTED; a 0-level encoding without identity is refused; dx untouched."""
    import nerf_amd
    lib = nerf_amd._lib.load()
    c, inp, _ = _sample_case("L11_id_mask_n86")
    x, g = _dev(inp["x"]), _dev(inp["g"])
    out = Guarded(3 * c.n_rays)
    p = _params(c)
    call = lambda: lib.nerf_encode_bwd(ctypes.byref(p), x.data_ptr(), g.data_ptr(), c.out_dim, c.n_rays, out.ptr(),
                                       0, _stream())
    p.kind = 1
    assert call() == UNSUPPORTED
    p.kind = 0
    p.levels, p.include_identity = 0, 0
    assert call() == INVALID
    torch.cuda.synchronize()
    out.check("refused nerf_encode_bwd", written=False)
