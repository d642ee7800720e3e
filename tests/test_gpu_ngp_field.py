"""GPU tests of the NGP radiance field: the SH-encoding and unit-cube kernel pairs
(csrc/ngp_field.hip) and nerf_amd.model_ngp, against tests/_ngp_field_ref.py.

Forward kernels: bitwise against the numpy fp32 restatements of the two contracts of
include/nerf_amd.h.  Backward kernels: against the hand-derived fp64 Jacobians at the project's
gradient bar (2e-5 + 1e-5 rel), g ~ N(0, 1), inputs without an argmax tie; two runs give the same
bits.  Every output is written into a buffer guarded by a NaN pattern (tests/_guarded.py); with a row
stride above the row width the pad columns must keep the pattern.

Field: NGPRadianceField with n_levels = 4, log2_hashmap_size = 10, max_resolution = 64 and
base_resolution = 4 (resolutions 4, 10, 25, 64: the coarsest level bijective, the others hashed; with
the default base of 16 every level of a 2^10 table is hashed) against the eager torch restatement
``ref_field`` on the CPU in fp32 from the same state.  Unit-cube coordinates, hash features and SH
values are asserted to be the same bits in both; everything behind a GEMM is held to bounds derived
by the forward-error method of tests/test_gpu_ingp2d.py carried element by element (``field_bounds``:
ours at the matmul precision's per-product error, 2^-24 for "highest" and 2^-17 for "high", plus theirs
at 2^-24), and every gradient tensor's largest bound must stay below half of its largest reference entry
(``BOUND_TO_VALUE``), so that a missing, sign-flipped or rescaled gradient path fails.  Every measured
distance is printed next to its bound.  Measured on an MI355X at n = 1000 ("highest" / "high", bounded;
the contracted field within a digit of these):
    rgb        bound 3.5e-05 / 1.1e-04   measured 6.0e-08 / 1.8e-07
    density    bound 1.4e-06 / 4.8e-06   measured 3.0e-08 / 3.0e-08
    loss       bound 7.8e-05 / 2.4e-04   measured 3.7e-09 / 1.9e-09
    gradients  positions bound 2.9e-07 / 8.8e-07, measured 5.8e-11 / 2.0e-09 (values to 3.0e-04);
               directions bound 4.6e-08 / 1.4e-07, measured 2.5e-11 / 8.2e-10 (values to 1.3e-04);
               the loosest tensor, mlp_base.2.bias, bound 2.1e-05 / 2.4e-05 on values to 1.5e-03
    one sample: position gradient bound 4.4e-04 ("high") on a value of 5.6e-03, the loosest case
Backward kernels at n = 4099: SH degree 4 1.4e-06 on values to 13, box map 7.1e-08 on values to 1.3,
contraction 3.5e-08 on values to 0.64.

Fit: a coloured density ball rendered through the same renderer is the target of 256 rays;
``FIT_STEPS`` FusedAdam steps at lr 1e-2.  See test_fit_analytic_ball for the recorded losses.
"""
import numpy as np
import pytest
import torch

import _ngp_field_ref as R
from _guarded import Guarded
from oracle import hashgrid_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"
SIZES = [1, 63, 64, 65, 257, 4099]
AABB = np.array([-1.0, -2.0, 0.0, 1.0, 2.0, 4.0], dtype=np.float32)
SMALL = dict(n_levels=4, log2_hashmap_size=10, max_resolution=64, base_resolution=4)
FIT_STEPS = 100


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


def box(aabb=AABB):
    import ctypes
    return (ctypes.c_float * 6)(*[float(v) for v in aabb])


def bits(x):
    return torch.as_tensor(np.ascontiguousarray(x)).view(torch.int32)


def strided(a: np.ndarray, stride: int) -> torch.Tensor:
    """a [n, w] as the first w columns of a device [n, stride] tensor (the rest NaN: never read)."""
    t = torch.full((a.shape[0], stride), float("nan"))
    t[:, :a.shape[1]] = torch.from_numpy(a)
    return t.to(DEV)


def cols(n: int, ld: int, w: int) -> torch.Tensor:
    return (torch.arange(n * ld) % ld) < w


def cube_points(n: int) -> np.ndarray:
    """The edge rows (centre, both faces of an axis, m = 1 exactly, 1e6 away, a NaN row), then seeded
    points inside, near and far outside AABB; the first n of them."""
    edge = np.array([[0, 0, 2], [1, 0, 2], [-1, 0, 2], [0.25, 2, 1], [1e6, 0, 2], [0, -1e6, 3], [np.nan, 0, 2],
                     [0.5, np.nan, np.nan]], dtype=np.float32)
    x, _ = R.field_points(max(n, 16), seed=7)
    rng = np.random.default_rng(8)
    lo, hi = AABB[:3].astype(np.float64), AABB[3:].astype(np.float64)
    x = (rng.uniform(-1, 2, x.shape) * (hi - lo) + lo).astype(np.float32)
    x[::5] = ((10 ** rng.uniform(0, 5, (len(x[::5]), 1))) * rng.standard_normal((len(x[::5]), 3))).astype(np.float32)
    return np.concatenate([edge, x])[:n]


# ----------------------------------------------------------------------------- forward kernels
@pytest.mark.parametrize("n", SIZES)
def test_sh_forward_bitwise(n):
    d = R.unit_dirs(n, seed=n)
    for degree in (1, 2, 3, 4):
        ref = R.sh32(d, degree)
        w = degree * degree
        for ds in (3, 4):
            dd = strided(d, ds)
            for ld in (16, 32):
                out = Guarded(n * ld, named=cols(n, ld, w))
                st = lib().nerf_sh_encode_fwd(dd.data_ptr(), ds, n, degree, out.ptr(), ld, stream())
                assert st == 0
                out.check(f"sh n={n} degree={degree} ld={ld}")
                got = out.body.view(n, ld)[:, :w].cpu().contiguous().view(torch.int32)
                assert torch.equal(got, bits(ref)), (n, degree, ds, ld)


@pytest.mark.parametrize("n", SIZES)
def test_unit_cube_forward_bitwise(n):
    x = cube_points(n)
    for mode in (0, 1):
        ref_u, ref_in = R.unit_cube32(x, AABB, mode)
        for xs in (3, 4):
            xd = strided(x, xs)
            for us in (3, 4):
                u, inside = Guarded(n * us, named=cols(n, us, 3)), Guarded(n)
                st = lib().nerf_unit_cube_fwd(xd.data_ptr(), xs, n, box(), mode, u.ptr(), us, inside.ptr(), stream())
                assert st == 0
                u.check(f"u n={n} mode={mode}")
                inside.check(f"inside n={n} mode={mode}")
                got = u.body.view(n, us)[:, :3].cpu()
                nan = np.isnan(ref_u)
                assert np.array_equal(torch.isnan(got).numpy(), nan), (n, mode)
                assert torch.equal(got.contiguous().view(torch.int32)[torch.from_numpy(~nan)], bits(ref_u)[torch.from_numpy(~nan)])
                assert torch.equal(inside.body.cpu().view(torch.int32), bits(ref_in)), (n, mode, xs, us)


def test_unit_cube_edge_rows_on_the_device():
    x = cube_points(8)
    for mode in (0, 1):
        u, inside = Guarded(8 * 3), Guarded(8)
        assert lib().nerf_unit_cube_fwd(strided(x, 3).data_ptr(), 3, 8, box(), mode, u.ptr(), 3, inside.ptr(), stream()) == 0
        uu, ins = u.body.view(8, 3).cpu().numpy(), inside.body.cpu().numpy()
        assert np.array_equal(uu[0], [0.5, 0.5, 0.5]) and ins[0] == 1                     # the centre
        if mode == 0:
            assert uu[1, 0] == 1 and uu[2, 0] == 0 and uu[3, 1] == 1                      # on a face
            assert not ins[1:6].any()
        else:
            assert uu[1, 0] == 0.75 and uu[2, 0] == 0.25 and uu[3, 1] == 0.75             # m = 1: not contracted
            assert ins[:6].all() and 0.99 < uu[4, 0] < 1 and 0 < uu[5, 1] < 0.01          # 1e6 away
        assert np.isnan(uu[6, 0]) and ins[6] == 0 and np.isnan(uu[7, 1:]).all() and ins[7] == 0
        inside_skipped = Guarded(8)
        u2 = Guarded(8 * 3)
        assert lib().nerf_unit_cube_fwd(strided(x, 3).data_ptr(), 3, 8, box(), mode, u2.ptr(), 3, None, stream()) == 0
        inside_skipped.check("inside skipped", written=False)
        assert torch.equal(u2.body.view(torch.int32), u.body.view(torch.int32))


# ----------------------------------------------------------------------------- backward kernels
def close_grad(got, ref, what):
    got = got.detach().cpu().double().numpy()
    err = np.abs(got - ref)
    print(f"{what}: max |err| = {err.max():.3e} (largest value {np.abs(ref).max():.3e})")
    np.testing.assert_allclose(got, ref, atol=2e-5, rtol=1e-5, err_msg=what)


@pytest.mark.parametrize("n", SIZES)
def test_sh_backward_against_fp64(n):
    d = R.unit_dirs(n, seed=100 + n)
    g = np.random.default_rng(n).standard_normal((n, 16)).astype(np.float32)
    for degree in (1, 2, 3, 4):
        ref = R.sh_bwd64(d, g, degree)
        runs = []
        for ds, gld, gds in ((3, 16, 3), (4, 32, 4)):
            dd, gg = strided(d, ds), strided(g, gld)
            for _ in range(2):
                gd = Guarded(n * gds, named=cols(n, gds, 3))
                st = lib().nerf_sh_encode_bwd(dd.data_ptr(), ds, n, degree, gg.data_ptr(), gld, gd.ptr(), gds, stream())
                assert st == 0
                gd.check(f"grad_dirs n={n} degree={degree}")
                runs.append(gd.body.view(n, gds)[:, :3].clone())
        close_grad(runs[0], ref, f"SH backward n={n} degree={degree}")
        for r in runs[1:]:
            assert torch.equal(r.contiguous().view(torch.int32), runs[0].contiguous().view(torch.int32))


def no_tie_points(n, seed):
    x, aabb = R.field_points(4 * n + 64, seed)
    a = aabb.astype(np.float64)
    c = np.sort(np.abs((x - a[:3]) / (a[3:] - a[:3]) * 2 - 1), axis=1)
    keep = (c[:, 2] - c[:, 1] > 1e-3 * c[:, 2]) & (np.abs(c[:, 2] - 1) > 1e-3)
    x = x[keep][:n]
    assert x.shape[0] == n
    return x, aabb


@pytest.mark.parametrize("n", SIZES)
def test_unit_cube_backward_against_fp64(n):
    x, aabb = no_tie_points(n, seed=200 + n)
    g = np.random.default_rng(n).standard_normal((n, 3)).astype(np.float32)
    for mode in (0, 1):
        ref = R.unit_cube_bwd64(x, aabb, mode, g)
        runs = []
        for xs, gus, gxs in ((3, 3, 3), (4, 4, 4)):
            xd, gg = strided(x, xs), strided(g, gus)
            for _ in range(2):
                gx = Guarded(n * gxs, named=cols(n, gxs, 3))
                st = lib().nerf_unit_cube_bwd(xd.data_ptr(), xs, n, box(aabb), mode, gg.data_ptr(), gus, gx.ptr(), gxs,
                                              stream())
                assert st == 0
                gx.check(f"grad_x n={n} mode={mode}")
                runs.append(gx.body.view(n, gxs)[:, :3].clone())
        close_grad(runs[0], ref, f"unit-cube backward n={n} mode={mode}")
        for r in runs[1:]:
            assert torch.equal(r.contiguous().view(torch.int32), runs[0].contiguous().view(torch.int32))


def test_zero_rows_and_bad_arguments_leave_the_guards():
    d = strided(R.unit_dirs(4), 3)
    out, gd, u, ins = Guarded(4 * 16), Guarded(4 * 3), Guarded(4 * 3), Guarded(4)
    L, s = lib(), stream()
    calls = [
        (0, L.nerf_sh_encode_fwd(d.data_ptr(), 3, 0, 4, out.ptr(), 16, s)),
        (0, L.nerf_sh_encode_bwd(d.data_ptr(), 3, 0, 4, d.data_ptr(), 16, gd.ptr(), 3, s)),
        (0, L.nerf_unit_cube_fwd(d.data_ptr(), 3, 0, box(), 1, u.ptr(), 3, ins.ptr(), s)),
        (0, L.nerf_unit_cube_bwd(d.data_ptr(), 3, 0, box(), 1, d.data_ptr(), 3, gd.ptr(), 3, s)),
        (-1, L.nerf_sh_encode_fwd(d.data_ptr(), 3, 4, 5, out.ptr(), 16, s)),
        (-1, L.nerf_sh_encode_fwd(d.data_ptr(), 3, 4, 0, out.ptr(), 16, s)),
        (-1, L.nerf_sh_encode_fwd(d.data_ptr(), 3, 4, 4, out.ptr(), 15, s)),
        (-1, L.nerf_sh_encode_fwd(d.data_ptr(), 2, 4, 4, out.ptr(), 16, s)),
        (-1, L.nerf_sh_encode_fwd(d.data_ptr(), 3, 4, 4, out.ptr() + 2, 16, s)),
        (-1, L.nerf_sh_encode_fwd(None, 3, 4, 4, out.ptr(), 16, s)),
        (-1, L.nerf_sh_encode_bwd(d.data_ptr(), 3, 4, 4, d.data_ptr(), 15, gd.ptr(), 3, s)),
        (-1, L.nerf_sh_encode_bwd(d.data_ptr(), 3, 4, 4, d.data_ptr(), 16, gd.ptr(), 2, s)),
        (-1, L.nerf_sh_encode_bwd(d.data_ptr(), 3, 4, 4, d.data_ptr(), 16, gd.ptr() + 1, 3, s)),
        (-1, L.nerf_sh_encode_bwd(d.data_ptr(), 3, 4, 7, d.data_ptr(), 64, gd.ptr(), 3, s)),
        (-1, L.nerf_unit_cube_fwd(d.data_ptr(), 3, 4, box(), 2, u.ptr(), 3, ins.ptr(), s)),
        (-1, L.nerf_unit_cube_fwd(d.data_ptr(), 3, 4, box(), 0, u.ptr(), 2, ins.ptr(), s)),
        (-1, L.nerf_unit_cube_fwd(d.data_ptr(), 3, 4, box(), 0, u.ptr(), 3, ins.ptr() + 2, s)),
        (-1, L.nerf_unit_cube_fwd(d.data_ptr(), 3, 4, None, 0, u.ptr(), 3, ins.ptr(), s)),
        (-1, L.nerf_unit_cube_fwd(d.data_ptr(), 3, 4, box(), 0, None, 3, ins.ptr(), s)),
        (-1, L.nerf_unit_cube_bwd(d.data_ptr(), 3, 4, box(), -1, d.data_ptr(), 3, gd.ptr(), 3, s)),
        (-1, L.nerf_unit_cube_bwd(d.data_ptr(), 3, 4, box(), 1, d.data_ptr(), 3, gd.ptr(), 2, s)),
        (-1, L.nerf_unit_cube_bwd(d.data_ptr(), 3, 4, box(), 1, None, 3, gd.ptr(), 3, s)),
    ]
    torch.cuda.synchronize()
    for i, (want, got) in enumerate(calls):
        assert got == want, (i, want, got)
    for name, buf in (("out", out), ("grad", gd), ("u", u), ("inside", ins)):
        buf.check(name, written=False)


# ----------------------------------------------------------------------------- public pieces
def test_public_encodings_and_maps():
    from nerf_amd import SHEncoding, contract_to_unisphere, normalize_to_aabb
    d = R.unit_dirs(130, seed=4)
    g = np.random.default_rng(4).standard_normal((130, 32)).astype(np.float32)
    for degree in (2, 4):
        dd = torch.from_numpy(d).to(DEV).requires_grad_(True)
        enc = SHEncoding(degree)
        y = enc(dd)
        w = degree * degree
        assert y.shape == (130, 32) and torch.all(y[:, w:] == 0)
        assert torch.equal(y[:, :w].detach().cpu().contiguous().view(torch.int32), bits(R.sh32(d, degree)))
        assert torch.equal(enc.encode_padded(dd).detach(), y.detach())
        (y * torch.from_numpy(g).to(DEV)).sum().backward()
        close_grad(dd.grad, R.sh_bwd64(d, g, degree), f"SHEncoding({degree}) gradient")
    x, aabb = no_tie_points(130, seed=11)
    gu = np.random.default_rng(5).standard_normal((130, 3)).astype(np.float32)
    for fn, mode in ((normalize_to_aabb, 0), (contract_to_unisphere, 1)):
        xx = torch.from_numpy(x).to(DEV).requires_grad_(True)
        u, inside = fn(xx, torch.from_numpy(aabb))
        ref_u, ref_in = R.unit_cube32(x, aabb, mode)
        assert torch.equal(u.detach().cpu().view(torch.int32), bits(ref_u))
        assert torch.equal(inside.cpu().view(torch.int32), bits(ref_in)) and not inside.requires_grad
        (u * torch.from_numpy(gu).to(DEV)).sum().backward()
        close_grad(xx.grad, R.unit_cube_bwd64(x, aabb, mode, gu), f"{fn.__name__} gradient")
        assert fn(torch.zeros(0, 3, device=DEV), list(aabb))[0].shape == (0, 3)
    # one row may carry any row stride: a transposed [3, 1] is a contiguous [1, 3] with stride(0) = 1
    one = torch.tensor([[0.3], [-0.5], [0.8]], device=DEV).t()
    assert one.shape == (1, 3) and one.is_contiguous() and one.stride(0) == 1
    ref1 = one.cpu().numpy().copy()
    assert torch.equal(SHEncoding(4)(one)[:, :16].cpu().contiguous().view(torch.int32), bits(R.sh32(ref1, 4)))
    assert torch.equal(contract_to_unisphere(one, list(aabb))[0].cpu().view(torch.int32),
                       bits(R.unit_cube32(ref1, aabb, 1)[0]))


def test_hash_encoding_subclass_against_the_oracle():
    from nerf_amd.model_ngp import UnitCubeHashEncoding
    torch.manual_seed(3)
    enc = UnitCubeHashEncoding(64, 4, 2 ** 10, 2, 4)
    tables = [e.table.detach().numpy().copy() * 1e4 for e in enc.encodings]
    with torch.no_grad():
        for e, t in zip(enc.encodings, tables):
            e.table.copy_(torch.from_numpy(t))
    enc = enc.to(DEV)
    u = np.random.default_rng(0).uniform(0, 1, (1000, 3)).astype(np.float32)
    u[:4] = [[0, 0, 0], [1, 1, 1], [0.5, 0.5, 0.5], [0.25, 1.0, 0.0]]
    got = enc(torch.from_numpy(u).to(DEV))
    ref = O.encode(u, tables, enc.resolutions, 2 ** 10, normalize=False)
    assert torch.equal(got.detach().cpu().contiguous().view(torch.int32), bits(ref))


# ----------------------------------------------------------------------------- the field against eager torch
@pytest.fixture(params=["highest", "high"])
def matmul_precision(request):
    old = torch.get_float32_matmul_precision()
    torch.set_float32_matmul_precision(request.param)
    yield request.param
    torch.set_float32_matmul_precision(old)


def make_field(unbounded: bool, seed: int = 0, table_scale: float = 1e3, use_viewdirs: bool = True):
    """The small field with tables scaled up from the 1e-4 initialisation, so that the hash features,
    and with them every gradient path through the grid, carry weight in the comparison."""
    from nerf_amd import NGPRadianceField
    torch.manual_seed(seed)
    f = NGPRadianceField(AABB, unbounded=unbounded, use_viewdirs=use_viewdirs, **SMALL)
    with torch.no_grad():
        for e in f.position_encoding.encodings:
            e.table.mul_(table_scale)
    return f


def field_inputs(n: int, unbounded: bool, seed: int):
    rng = np.random.default_rng(seed)
    lo, hi = AABB[:3].astype(np.float64), AABB[3:].astype(np.float64)
    v = rng.uniform(-1.5, 2.5, (n, 3)) if unbounded else rng.uniform(-0.1, 1.1, (n, 3))
    if n > 1:
        v[0] = 0.5                                                          # the centre
    x = (v * (hi - lo) + lo).astype(np.float32)
    d = R.unit_dirs(n, seed=seed + 1)
    g_rgb = rng.standard_normal((n, 3)).astype(np.float32)
    g_dens = rng.standard_normal(n).astype(np.float32)
    return x, d, g_rgb, g_dens


# a gradient's bound has to stay under the gradient: a missing path is off by the value itself, a flipped
# sign by twice it, a factor of 2 or 1/2 by half of it or more, so a tolerance below half of the tensor's
# largest reference entry notices each of them there; one at or above it would be no check
BOUND_TO_VALUE = 0.5


def compare_with_restatement(field, n: int, precision: str):
    """Outputs, loss and every gradient of `field` (on the CPU, moved here) on n samples against
    ref_field in fp32 on the CPU from the same state, element by element within field_bounds."""
    unbounded, views = field.unbounded, field.use_viewdirs
    cfg = R.field_cfg(field)
    sd = {k: v.detach().clone() for k, v in field.state_dict().items()}
    field = field.to(DEV)
    x, d, g_rgb, g_dens = field_inputs(n, unbounded, seed=40 + n)
    eps = 2.0 ** -24 if precision == "highest" else 2.0 ** -17
    sd64 = {k: v.double() for k, v in sd.items()}
    ours = R.field_bounds(sd64, cfg, x, d, g_rgb, g_dens, eps)
    theirs = R.field_bounds(sd64, cfg, x, d, g_rgb, g_dens, 2.0 ** -24)

    # the restatement: fp32 on the CPU
    leaves = {k: v.clone().requires_grad_(k != "aabb") for k, v in sd.items()}
    xr, dr = torch.from_numpy(x).requires_grad_(True), torch.from_numpy(d).requires_grad_(True)
    keep = {}
    rgb_r, dens_r = R.ref_field(leaves, cfg, xr, dr, keep=keep)
    loss_r = R.field_loss(rgb_r, dens_r, torch.from_numpy(g_rgb), torch.from_numpy(g_dens))
    loss_r.backward()

    # the kernels
    from nerf_amd.model_ngp import _UnitCubeFn
    xg, dg = torch.from_numpy(x).to(DEV).requires_grad_(True), torch.from_numpy(d).to(DEV).requires_grad_(True)
    u, inside = _UnitCubeFn.apply(xg.detach(), field._box, 1 if unbounded else 0)
    assert torch.equal(u.cpu().view(torch.int32), keep["u"].detach().view(torch.int32))
    assert torch.equal(inside.cpu(), keep["inside"])
    feat = field.position_encoding(u)
    assert torch.equal(feat.detach().cpu().contiguous().view(torch.int32), keep["feat"].detach().view(torch.int32))
    if views:
        sh = field.direction_encoding(dg.detach())[:, :16]
        assert torch.equal(sh.cpu().contiguous().view(torch.int32), keep["sh"].detach().view(torch.int32))
    rgb, dens = field(xg, dg) if views else field(xg)
    assert rgb.shape == (n, 3) and dens.shape == (n, 1)
    loss = R.field_loss(rgb, dens, torch.from_numpy(g_rgb).to(DEV), torch.from_numpy(g_dens).to(DEV))
    loss.backward()

    tag = f"n={n} {'unbounded' if unbounded else 'bounded'}{'' if views else ' no viewdirs'} {precision}"

    def check(what, got, ref, tol, grad=False):
        err = (got.detach().cpu().double() - ref.detach().double()).abs().numpy()
        tol = np.broadcast_to(np.asarray(tol, dtype=np.float64), err.shape)
        scale = float(ref.detach().abs().max())
        print(f"{tag}: {what} err {err.max():.3e} largest bound {tol.max():.3e} (largest value {scale:.3e})")
        worst = int(np.argmax(err - tol))
        assert (err <= tol).all(), (what, float(err.reshape(-1)[worst]), float(tol.reshape(-1)[worst]))
        if grad:
            assert scale > 0 and tol.max() <= BOUND_TO_VALUE * scale, (what, float(tol.max()), scale)

    check("rgb", rgb, rgb_r, ours["rgb"] + theirs["rgb"])
    check("density", dens, dens_r, ours["density"] + theirs["density"])
    check("loss", loss, loss_r, ours["loss"] + theirs["loss"])
    if not unbounded:
        out = keep["inside"] == 0
        assert out.any() or n == 1
        assert torch.all(dens.detach().cpu().reshape(-1)[out] == 0)         # exactly 0 outside the box
    for k, p in field.named_parameters():
        assert p.grad is not None, k
        check(f"grad {k}", p.grad, leaves[k].grad, ours["grad"][k] + theirs["grad"][k], grad=True)
    check("grad positions", xg.grad, xr.grad, ours["grad"]["positions"] + theirs["grad"]["positions"], grad=True)
    if views:
        check("grad directions", dg.grad, dr.grad, ours["grad"]["directions"] + theirs["grad"]["directions"], grad=True)
    else:
        assert dg.grad is None


@pytest.mark.parametrize("unbounded", [False, True])
@pytest.mark.parametrize("n", [1, 130, 1000])
def test_field_against_the_eager_restatement(matmul_precision, n, unbounded):
    compare_with_restatement(make_field(unbounded), n, matmul_precision)


def test_field_without_viewdirs_against_the_eager_restatement(matmul_precision):
    """use_viewdirs=False: the head reads the geometry features alone (15 inputs), no direction buffer."""
    field = make_field(False, use_viewdirs=False)
    assert field.direction_encoding is None and field.mlp_head[0].in_features == 15
    assert [s.kind for s in field.plan().layers[2].sources] == ["act"]
    compare_with_restatement(field, 130, matmul_precision)


def test_query_density_is_forwards_density_and_runs_no_colour_layer():
    from nerf_amd import mlp
    field = make_field(False).to(DEV)
    x, d, _, _ = field_inputs(1000, False, seed=9)
    xg, dg = torch.from_numpy(x).to(DEV), torch.from_numpy(d).to(DEV)
    mlp.CAPTURE = []
    try:
        with torch.no_grad():
            _, dens = field(xg, dg)
            q = field.query_density(xg)
        runs = mlp.CAPTURE
    finally:
        mlp.CAPTURE = None
    assert q.shape == (1000, 1) and torch.equal(q.view(torch.int32), dens.view(torch.int32))
    assert float(q.max()) > 0
    # the plans the two calls ran, by the layer outputs they produced: five layers, then the two density layers
    assert [len(acts) for acts, _ in runs] == [5, 2]
    assert [a.shape[1] for a in runs[1][0]] == [64, 16]
    assert len(field.density_plan().layers) == 2 and field.density_plan() is not field.plan()
    # with gradients: the density path alone reaches the base layers and the table, not the head
    field.zero_grad()
    field.query_density(xg).sum().backward()
    assert field.mlp_base[0].weight.grad is not None and field.position_encoding.encodings[0].table.grad is not None
    assert all(p.grad is None for p in field.mlp_head.parameters())


# ----------------------------------------------------------------------------- through the renderer
def camera_rays(n: int, seed: int, centre, radius: float):
    g = torch.Generator().manual_seed(seed)
    c = torch.tensor(centre, dtype=torch.float32)
    o = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=1) * radius + c
    target = c + 0.3 * (torch.rand(n, 3, generator=g) - 0.5)
    return o.contiguous(), torch.nn.functional.normalize(target - o, dim=1).contiguous()


def test_renderer_bounded_and_grid_update():
    from nerf_amd import OccGridEstimator, OccGridRenderer
    field = make_field(False).to(DEV)
    est = OccGridEstimator(list(AABB), 16).to(DEV)
    est.binaries.fill_(True)
    ren = OccGridRenderer(field, est, 0.05, 12.0, 0.05, density_fn=field.query_density)
    o, d = camera_rays(64, 1, [0.0, 0.0, 2.0], 4.0)
    o, d = o.to(DEV).requires_grad_(True), d.to(DEV).requires_grad_(True)
    rgb, opacity, depth, ex = ren(o, d, stratified=False)
    assert rgb.shape == (64, 3) and ex["ray_indices"].numel() > 64
    rgb.sum().backward()
    for name, t in (("rgb", rgb), ("rays_o.grad", o.grad), ("rays_d.grad", d.grad)):
        assert torch.isfinite(t).all() and float(t.detach().abs().max()) > 0, name
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in field.parameters())
    # a point outside the box has density exactly 0
    outside = torch.tensor([[1.5, 0.0, 2.0], [0.0, 0.0, -0.5], [1.0, 0.0, 2.0]], device=DEV)
    assert torch.all(field.query_density(outside) == 0) and torch.all(field(outside, outside)[1] == 0)
    # the grid update through density_fn, and the next forward on the new grid
    before = ex["ray_indices"].numel()
    torch.manual_seed(5)
    with torch.no_grad():
        dens = field.query_density(torch.from_numpy(field_inputs(1000, False, 3)[0]).to(DEV))
        thre = float(dens[dens > 0].median()) * 0.05
        ren.update_grid(0, occ_thre=thre, n=16)
    kept = int(est.binaries.sum())
    assert 0 < kept < est.cells
    _, _, _, ex2 = ren(o.detach(), d.detach(), stratified=False)
    assert 0 < ex2["ray_indices"].numel() < before


def test_renderer_unbounded_cascade_with_cone_angle():
    from nerf_amd import CascadedOccGridEstimator, OccGridRenderer
    field = make_field(True).to(DEV)
    est = CascadedOccGridEstimator(list(AABB), 16, levels=2).to(DEV)
    est.binaries.fill_(True)
    ren = OccGridRenderer(field, est, 0.05, 12.0, 0.05, density_fn=field.query_density, cone_angle=0.004)
    o, d = camera_rays(64, 2, [0.0, 0.0, 2.0], 4.0)
    o, d = o.to(DEV).requires_grad_(True), d.to(DEV).requires_grad_(True)
    rgb, _, _, ex = ren(o, d, stratified=False)
    assert ex["ray_indices"].numel() > 64
    rgb.sum().backward()
    for name, t in (("rgb", rgb), ("rays_o.grad", o.grad), ("rays_d.grad", d.grad)):
        assert torch.isfinite(t).all() and float(t.detach().abs().max()) > 0, name
    # samples beyond the inner box exist, and the contracted field gives them density
    from nerf_amd import packed_points
    pos, _ = packed_points(o.detach(), d.detach(), ex["ray_indices"], ex["t_starts"], ex["t_ends"])
    m = R.contraction_m(pos.cpu().numpy(), AABB)
    assert (m > 1).any()
    with torch.no_grad():
        far = field.query_density(pos[torch.from_numpy(m > 1).to(DEV)])
    assert torch.all(far > 0)
    with torch.no_grad():
        ren.update_grid(0, n=16)
    rgb2, _, _, _ = ren(o.detach(), d.detach(), stratified=False)
    assert torch.isfinite(rgb2).all()


# ----------------------------------------------------------------------------- fit
class Ball(torch.nn.Module):
    """A coloured density ball at the box's centre: density 30 inside radius 0.6, colour from the position."""

    def forward(self, pos, dirs):
        c = pos.new_tensor([0.0, 0.0, 2.0])
        r = (pos - c).norm(dim=1)
        sigma = 30.0 * torch.sigmoid((0.6 - r) * 20.0)
        rgb = torch.sigmoid(2.0 * (pos - c))
        return rgb, sigma


def fit(make, steps: int):
    """(initial loss, final loss) of `steps` FusedAdam steps of make() (a field on the device) on 256 rays
    of the ball, lr 1e-2, stratified=False, all cells set."""
    from nerf_amd import FusedAdam, OccGridEstimator, OccGridRenderer
    est = OccGridEstimator(list(AABB), 16).to(DEV)
    est.binaries.fill_(True)
    o, d = camera_rays(256, 3, [0.0, 0.0, 2.0], 4.0)
    o, d = o.to(DEV), d.to(DEV)
    with torch.no_grad():
        target = OccGridRenderer(Ball(), est, 0.05, 12.0, 0.05, early_stop_eps=0.0)(o, d, stratified=False)[0]
    field = make()
    ren = OccGridRenderer(field, est, 0.05, 12.0, 0.05, early_stop_eps=0.0)
    opt = FusedAdam(list(field.parameters()), lr=1e-2)
    losses = []
    for _ in range(steps + 1):
        opt.zero_grad()
        loss = torch.nn.functional.mse_loss(ren(o, d, stratified=False)[0], target)
        losses.append(loss.detach())
        if len(losses) <= steps:
            loss.backward()
            opt.step()
    return float(losses[0]), float(losses[-1])


def test_fit_analytic_ball():
    """FIT_STEPS = 100 steps in "highest".  The eager restatement (R.RefNGPField on the device, trained by
    fit() from the same state) is what the step count was chosen on; recorded on an MI355X, from an
    initial loss of 0.044894 in both:
        eager restatement   20 steps: 0.058 x    60 steps: 0.0100 x    100 steps: 0.000065 (0.0015 x)
        kernel path         20 steps: 0.058 x    60 steps: 0.0100 x    100 steps: 0.000065 (0.0015 x)
    The issue's bar for the kernel path is 0.25 x its initial loss, to be tightened if both land close:
    they land on the same figure, seven times under 0.01 x, so the kernel path is held to 0.01 x, where a
    degraded gradient path (the 60-step figure) already fails."""
    old = torch.get_float32_matmul_precision()
    torch.set_float32_matmul_precision("highest")
    try:
        first, last = fit(lambda: make_field(False, seed=1, table_scale=1.0).to(DEV), FIT_STEPS)
    finally:
        torch.set_float32_matmul_precision(old)
    print(f"fit: loss {first:.5f} -> {last:.6f} ({last / first:.3f} x)")
    assert np.isfinite(last) and last <= 0.01 * first
