"""The stand-alone compositing kernels (csrc/composite.hip: nerf_composite_fwd / _bwd) at their edge
shapes, called with every pointer layout chosen on purpose and compared with the fp64 restatement
tests/_raypath_ref.py::composite_ref64.

Bars (the project's compositing tolerances, tests/test_gpu_parity.py): rgb and weights 2e-6 abs,
raw-input gradients 2e-5 abs + 1e-5 rel.  On these inputs (B = 9, every S from 1 to 129 and the
larger S of the sweep, both scale sets) the fp32 oracle (O.render_rays on fp32 activations, on the
CPU) lies within 5.2e-7 (rgb), 8.5e-8 (weights) and 0.7 % of the gradient bar of composite_ref64
(tests/test_raypath_ref.py), so the reference's own rounding leaves a margin of more than three.

Every output of the shape and layout sweeps is a view into a buffer filled with a NaN bit pattern,
with 1024 floats of guard on either side; after the call every guard element and every column the
contract does not name still holds that pattern, and every element it names does not.
"""
import numpy as np
import pytest
import torch

from _raypath_ref import activate32, composite_inputs, composite_ref64

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = 0x7FC0BEEF          # a quiet NaN no kernel produces
GUARD = 1024
SCALES = [(3.0, 7.0, 0.0), (1.0, 1.0, 1.5)]   # (scale_a, scale_b, density_shift)
S_SWEEP = [1, 2, 63, 64, 65, 200, 256, 321, 384, 385, 449, 512, 513, 1000, 1024]
ACT1_LAYOUTS = ["packed", "packed_split", "c4", "c4_off1", "wide32"]
WALK = 8192                     # rays in flight of the capped grid (kMaxBlocks * 4)


@pytest.fixture(scope="module", autouse=True)
def _lib():
    import nerf_amd
    nerf_amd._lib.load()  # fail loudly if the HIP library is missing
    yield


class Guarded:
    """n floats between two guards, all preset to SENTINEL.  `named` (bool [n], default all) marks the
    elements the kernel's contract writes; `shift` moves the body off 16-byte alignment."""

    def __init__(self, n, named=None, shift=0):
        self.lo, self.n = GUARD + shift, n
        self.flat = torch.full((self.lo + n + GUARD,), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
        self.body = self.flat[self.lo:self.lo + n]
        self.named = torch.ones(n, dtype=torch.bool) if named is None else named

    def check(self, what, written=True):
        bits = self.flat.view(torch.int32).cpu()
        keep = torch.ones(bits.numel(), dtype=torch.bool)
        if written:
            keep[self.lo:self.lo + self.n] = ~self.named
        stray = int((bits[keep] != SENTINEL).sum())
        assert stray == 0, f"{what}: {stray} stores outside the elements the contract names"
        if written:
            missing = int((bits[~keep] == SENTINEL).sum())
            assert missing == 0, f"{what}: {missing} named elements never stored"


def columns(n, width, ncols):
    m = torch.zeros(n, width, dtype=torch.bool)
    m[:, :ncols] = True
    return m.reshape(-1)


class Layout:
    """Device inputs of one pointer layout for head rows [B, S, 4] = [rgb | sigma] (raw values), and
    guarded gradient buffers for it.
      packed        [rgb | sigma] rows of width 4 in, packed gradient rows out
      packed_split  packed in; grad_density stride 1 and grad_color stride 3 out
      c4            density stride 1; colour stride 4, 16-byte aligned (one 16-byte load per sample)
      c4_off1       the same on a base shifted by one float: the generic colour path
      wide32        width-32 head rows in and out
      act0_s3       act = 0: activated density stride 1 and colour stride 3"""

    def __init__(self, name, head, shift):
        self.name, self.act = name, int(name != "act0_s3")
        B, S, _ = head.shape
        n = self.n = B * S
        rows = head.reshape(n, 4)
        self.ref_in = head
        if name in ("packed", "packed_split"):
            flat = rows.to(DEV).contiguous().view(-1)
            self.density, self.ds, self.color, self.cs = flat[3:], 4, flat, 4
        elif name in ("c4", "c4_off1"):
            off = int(name == "c4_off1")
            buf = torch.full((4 * n + 4,), 777.0, device=DEV)
            self.color, self.cs = buf[off:off + 4 * n], 4
            self.color.view(n, 4)[:, :3] = rows[:, :3].to(DEV)
            self.density, self.ds = rows[:, 3].contiguous().to(DEV), 1
            assert self.color.data_ptr() % 16 == 4 * off
        elif name == "wide32":
            wide = torch.full((n, 32), 777.0)
            wide[:, :4] = rows
            flat = wide.to(DEV).view(-1)
            self.density, self.ds, self.color, self.cs = flat[3:], 32, flat, 32
        else:
            sig, col = activate32(head, shift)
            self.ref_in = (sig, col)
            self.density, self.ds = sig.reshape(n).to(DEV), 1
            self.color, self.cs = col.reshape(3 * n).to(DEV), 3

    def grads(self):
        """(grad_density, gd_stride, grad_color, gc_stride, guarded buffers, extract)."""
        n, name = self.n, self.name
        if name == "packed":
            g = Guarded(4 * n)
            rows = g.body.view(n, 4)
            return g.body[3:], 4, g.body, 4, [g], lambda: (rows[:, 3], rows[:, :3])
        if name == "wide32":
            g = Guarded(32 * n, columns(n, 32, 4))
            rows = g.body.view(n, 32)
            return g.body[3:], 32, g.body, 32, [g], lambda: (rows[:, 3], rows[:, :3])
        gd = Guarded(n)
        if name in ("c4", "c4_off1"):
            gc = Guarded(4 * n, columns(n, 4, 3), shift=int(name == "c4_off1"))
            rows = gc.body.view(n, 4)
            return gd.body, 1, gc.body, 4, [gd, gc], lambda: (gd.body, rows[:, :3])
        gc = Guarded(3 * n)
        return gd.body, 1, gc.body, 3, [gd, gc], lambda: (gd.body, gc.body.view(n, 3))


def stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def fwd_guarded(lay, dist, B, S, sa, sb, shift):
    """nerf_composite_fwd through the C ABI into guarded outputs (kernels.composite_fwd allocates its
    own): (status, rgb buffer, weights buffer)."""
    import nerf_amd
    rgb, w = Guarded(3 * B), Guarded(B * S)
    st = nerf_amd._lib.load().nerf_composite_fwd(lay.density.data_ptr(), lay.ds, lay.color.data_ptr(), lay.cs,
                                                 dist.data_ptr(), B, S, sa, sb, lay.act, shift,
                                                 rgb.body.data_ptr(), w.body.data_ptr(), stream())
    return st, rgb, w


def bwd(lay, dist, B, S, sa, sb, shift, g_rgb, g_w, gd, gds, gc, gcs):
    from nerf_amd import kernels as K
    K.composite_bwd(lay.density, lay.ds, lay.color, lay.cs, dist, B, S, sa, sb, lay.act, shift, g_rgb, g_w,
                    gd, gds, gc, gcs)


def close(got, ref, grad, what):
    atol, rtol = (2e-5, 1e-5) if grad else (2e-6, 0.0)
    got, ref = got.detach().cpu().double().numpy(), ref.numpy()
    err = np.abs(got - ref.reshape(got.shape))
    print(f"{what}: max |err| = {err.max():.3e}")
    np.testing.assert_allclose(got, ref.reshape(got.shape), atol=atol, rtol=rtol, err_msg=what)


def run_case(name, B, S, sa, sb, shift):
    """Forward then backward (with a weight gradient) of one layout against composite_ref64, every
    output guarded; the binding's own forward returns the same bits."""
    from nerf_amd import kernels as K
    head, dist, g_rgb, g_w = composite_inputs(B, S, 1000 * B + S)
    lay = Layout(name, head, shift)
    ref_rgb, ref_w, ref_ds, ref_dc = composite_ref64(lay.ref_in, dist, sa, sb, lay.act, shift, g_rgb, g_w)
    dd = dist.to(DEV)
    st, rgb, w = fwd_guarded(lay, dd, B, S, sa, sb, shift)
    assert st == 0
    rgb.check(f"{name} rgb")
    w.check(f"{name} weights")
    close(rgb.body.view(B, 3), ref_rgb, False, f"{name} S={S} rgb")
    close(w.body.view(B, S), ref_w, False, f"{name} S={S} weights")
    rgb2, w2 = K.composite_fwd(lay.density, lay.ds, lay.color, lay.cs, dd, B, S, sa, sb, bool(lay.act), shift)
    assert torch.equal(rgb2.view(-1), rgb.body) and torch.equal(w2.view(-1), w.body)
    gd, gds, gc, gcs, bufs, extract = lay.grads()
    bwd(lay, dd, B, S, sa, sb, shift, g_rgb.to(DEV), g_w.to(DEV), gd, gds, gc, gcs)
    for b in bufs:
        b.check(f"{name} gradients")
    d_sigma, d_color = extract()
    close(d_sigma, ref_ds, True, f"{name} S={S} d sigma")
    close(d_color, ref_dc, True, f"{name} S={S} d colour")


@pytest.mark.parametrize("name", ["packed", "act0_s3"])
@pytest.mark.parametrize("sa,sb,shift", SCALES)
@pytest.mark.parametrize("B,S", [(9, S) for S in S_SWEEP] + [(1, 1), (1, 1024)])
def test_shapes(B, S, sa, sb, shift, name):
    """Every instantiation R = ceil(S / 64) in {1, 2, 3, 4, 5, 6, 8, 16} (7 runs as 8) on both sides
    of each boundary, a ragged last block of rays, a single ray."""
    run_case(name, B, S, sa, sb, shift)


@pytest.mark.parametrize("name", ACT1_LAYOUTS + ["act0_s3"])
@pytest.mark.parametrize("sa,sb,shift", SCALES)
@pytest.mark.parametrize("S", [65, 385])
def test_layouts(S, sa, sb, shift, name):
    run_case(name, 9, S, sa, sb, shift)


@pytest.mark.parametrize("S", [65, 385])
def test_optional_pointers(S):
    """weights_out = NULL leaves rgb bitwise; a NULL grad_density or grad_color leaves the other
    gradient bitwise; grad_weights = NULL is a zero weight gradient, bitwise."""
    from nerf_amd import kernels as K
    B, (sa, sb, shift) = 9, SCALES[1]
    head, dist, g_rgb, g_w = composite_inputs(B, S, 7 + S)
    lay = Layout("packed_split", head, shift)
    dd, gr, gw = dist.to(DEV), g_rgb.to(DEV), g_w.to(DEV)
    args = (lay.density, lay.ds, lay.color, lay.cs, dd, B, S, sa, sb, True, shift)
    rgb, w = K.composite_fwd(*args)
    rgb_only, none = K.composite_fwd(*args, want_weights=False)
    assert none is None and torch.equal(rgb, rgb_only)

    def grads(g_w, want_d=True, want_c=True):
        gd, gds, gc, gcs, (bd, bc), extract = lay.grads()
        bwd(lay, dd, B, S, sa, sb, shift, gr, g_w, gd if want_d else None, gds, gc if want_c else None, gcs)
        bd.check("grad_density", written=want_d)
        bc.check("grad_color", written=want_c)
        return tuple(x.clone() for x in extract())

    d_sigma, d_color = grads(gw)
    assert torch.equal(grads(gw, want_d=False)[1], d_color)
    assert torch.equal(grads(gw, want_c=False)[0], d_sigma)
    z_sigma, z_color = grads(torch.zeros_like(gw))
    n_sigma, n_color = grads(None)
    assert torch.equal(n_sigma, z_sigma) and torch.equal(n_color, z_color)
    assert not torch.equal(z_sigma, d_sigma)
    # packed [d rgb | d sigma] rows hold the same bits as the separate buffers
    gd, gds, gc, gcs, _, extract = Layout("packed", head, shift).grads()
    bwd(lay, dd, B, S, sa, sb, shift, gr, gw, gd, gds, gc, gcs)
    p_sigma, p_color = extract()
    assert torch.equal(p_sigma, d_sigma) and torch.equal(p_color, d_color)


@pytest.mark.parametrize("name", ["packed", "act0_s3"])
@pytest.mark.parametrize("S", [5, 70])
@pytest.mark.parametrize("n_rays", [WALK + 3, 2 * WALK + 7])
def test_ray_walk(n_rays, S, name):
    """More rays than the capped grid holds in flight (S <= 128): each wave walks to ray + 8192 with
    the next ray's samples, and in the backward its g_rgb, handed over in registers.  Every ray
    against composite_ref64 (each ray has its own g_rgb and g_w); the first 8192 rays are bitwise
    those of a call on just them, which never takes the walk."""
    from nerf_amd import kernels as K
    sa, sb, shift = SCALES[0]
    head, dist, g_rgb, g_w = composite_inputs(n_rays, S, n_rays + S)
    ref_rgb, ref_w, ref_ds, ref_dc = None, None, None, None
    outs = []
    for B in (n_rays, WALK):
        lay = Layout(name, head[:B], shift)
        dd, gr, gw = dist[:B].contiguous().to(DEV), g_rgb[:B].to(DEV), g_w[:B].contiguous().to(DEV)
        rgb, w = K.composite_fwd(lay.density, lay.ds, lay.color, lay.cs, dd, B, S, sa, sb, bool(lay.act), shift)
        gd, gds, gc, gcs, bufs, extract = lay.grads()
        bwd(lay, dd, B, S, sa, sb, shift, gr, gw, gd, gds, gc, gcs)
        for b in bufs:
            b.check(f"{name} gradients, {B} rays")
        d_sigma, d_color = extract()
        outs.append((rgb, w, d_sigma.reshape(B, S), d_color.reshape(B, S, 3)))
        if B == n_rays:
            ref_rgb, ref_w, ref_ds, ref_dc = composite_ref64(lay.ref_in, dist, sa, sb, lay.act, shift, g_rgb, g_w)
    full, head_only = outs
    close(full[0], ref_rgb, False, "rgb")
    close(full[1], ref_w, False, "weights")
    close(full[2], ref_ds, True, "d sigma")
    close(full[3], ref_dc, True, "d colour")
    for a, b, what in zip(full, head_only, ("rgb", "weights", "d sigma", "d colour")):
        assert torch.equal(a[:WALK], b), f"{what}: the first {WALK} rays differ from a call on them alone"


@pytest.mark.parametrize("act", [1, 0])
def test_extremes(act):
    """Rows of one batch at S = 130: an opaque wall (raw density 1e4 from mid-ray on), all dist = 0,
    raw density -100, raw colours of +-40.  Everything finite and inside the bars; nothing behind the
    wall receives a gradient (T = 0 there and the fp64 suffix sums cancel exactly)."""
    from nerf_amd import kernels as K
    B, S, (sa, sb, shift) = 6, 130, SCALES[0]
    head, dist, g_rgb, g_w = composite_inputs(B, S, 99)
    head[0, S // 2:, 3] = 1e4
    dist[0] = dist[0].clamp(min=0.01)          # b <= -1e4 * 0.01 * 21: e^b = 0 in fp32 and fp64
    dist[1] = 0
    head[2, :, 3] = -100.0
    head[3, :, :3] = 40.0
    head[4, :, :3] = -40.0
    head[4, 1::2, :3] = 40.0
    lay = Layout("packed" if act else "act0_s3", head, shift)
    ref_rgb, ref_w, ref_ds, ref_dc = composite_ref64(lay.ref_in, dist, sa, sb, act, shift, g_rgb, g_w)
    dd = dist.to(DEV)
    rgb, w = K.composite_fwd(lay.density, lay.ds, lay.color, lay.cs, dd, B, S, sa, sb, bool(act), shift)
    gd, gds, gc, gcs, bufs, extract = lay.grads()
    bwd(lay, dd, B, S, sa, sb, shift, g_rgb.to(DEV), g_w.to(DEV), gd, gds, gc, gcs)
    for b in bufs:
        b.check("gradients")
    d_sigma, d_color = (x.reshape(B, S, -1) for x in extract())
    for x in (rgb, w, d_sigma, d_color):
        assert torch.isfinite(x).all()
    close(rgb, ref_rgb, False, "rgb")
    close(w, ref_w, False, "weights")
    close(d_sigma, ref_ds, True, "d sigma")
    close(d_color, ref_dc, True, "d colour")
    behind = slice(S // 2 + 1, None)
    assert torch.all(w[0, behind] == 0)
    assert torch.all(d_sigma[0, behind] == 0) and torch.all(d_color[0, behind] == 0)
    assert torch.all(ref_ds[0, behind] == 0) and torch.all(ref_dc[0, behind] == 0)
    assert torch.all(w[1] == 0) and torch.all(rgb[1] == 0) and torch.all(d_sigma[1] == 0)


def test_refuses_more_than_1024_samples():
    """S = 1025 with valid pointers: NERF_ERR_UNSUPPORTED, nothing launched, outputs untouched."""
    from nerf_amd import kernels as K
    from nerf_amd._lib import NERF_ERR_UNSUPPORTED
    B, S, (sa, sb, shift) = 3, 1025, SCALES[0]
    head, dist, g_rgb, g_w = composite_inputs(B, S, 5)
    lay = Layout("packed", head, shift)
    dd = dist.to(DEV)
    st, rgb, w = fwd_guarded(lay, dd, B, S, sa, sb, shift)
    torch.cuda.synchronize()
    assert st == NERF_ERR_UNSUPPORTED
    rgb.check("rgb", written=False)
    w.check("weights", written=False)
    with pytest.raises(RuntimeError, match=f"status {NERF_ERR_UNSUPPORTED}"):
        K.composite_fwd(lay.density, lay.ds, lay.color, lay.cs, dd, B, S, sa, sb, True, shift)
    gd, gds, gc, gcs, bufs, _ = lay.grads()
    with pytest.raises(RuntimeError, match=f"status {NERF_ERR_UNSUPPORTED}"):
        bwd(lay, dd, B, S, sa, sb, shift, g_rgb.to(DEV), g_w.to(DEV), gd, gds, gc, gcs)
    torch.cuda.synchronize()
    bufs[0].check("gradients", written=False)
