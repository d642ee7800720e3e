"""CPU checks of the NGP field's restatements (tests/_ngp_field_ref.py) and of the module's pieces
that need no device.

The fp32 restatements of the two forward contracts against their fp64 forms on 10^5 seeded unit
directions / points (extents in [1, 4]; a third of the points inside the box, a third with
1 < m < 4, the rest with m up to 1e6), measured here:
    SH degree 4        max |fp32 - fp64| = 1.9e-07    (values up to 0.75)
    unit cube, mode 0  max relative       = 1.7e-07   (|u| up to 5e5: one subtraction, one division)
    unit cube, mode 1  max |fp32 - fp64|  = 1.6e-07   (u in [0, 1])
asserted at four times the measured maxima as the regression bar.
"""
import numpy as np
import pytest
import torch

import _ngp_field_ref as R
from oracle import hashgrid_oracle as O

N = 100_000
SH_BAR = 4 * 1.9e-7
CUBE0_BAR = 4 * 1.7e-7
CUBE1_BAR = 4 * 1.6e-7


def test_sh_is_orthonormal_by_quadrature():
    d, w = R.sphere_quadrature()
    assert abs(w.sum() - 4 * np.pi) < 1e-12
    Y = R.sh64(d, 4)
    gram = (Y * w[:, None]).T @ Y
    err = np.abs(gram - np.eye(16)).max()
    print(f"SH gram matrix: max |G - I| = {err:.2e}")
    assert err < 1e-12
    for degree in (1, 2, 3):
        assert np.array_equal(R.sh64(d, degree), Y[:, :degree * degree])


def test_sh_fp32_restatement_distance():
    d = R.unit_dirs(N)
    for degree in (1, 2, 3, 4):
        y32, y64 = R.sh32(d, degree), R.sh64(d, degree)
        assert y32.dtype == np.float32 and y32.shape == (N, degree * degree)
        err = np.abs(y32.astype(np.float64) - y64).max()
        print(f"SH degree {degree}: max |fp32 - fp64| = {err:.2e} (largest value {np.abs(y64).max():.3f})")
        assert err <= SH_BAR
    # the torch form in fp32 is the numpy form's bits
    assert np.array_equal(R.sh_torch(torch.from_numpy(d), 4).numpy(), R.sh32(d, 4))


def test_unit_cube_fp32_restatement_distance():
    x, aabb = R.field_points(N)
    m = R.contraction_m(x, aabb)
    third = N // 3
    print(f"points: {np.mean(m < 1):.3f} inside, {np.mean((m > 1) & (m < 4)):.3f} with 1 < m < 4, "
          f"largest m = {m.max():.3e}")
    assert abs(np.sum(m < 1) - third) < 50 and abs(np.sum((m > 1) & (m < 4)) - third) < 50 and m.max() > 1e5
    u32, in32 = R.unit_cube32(x, aabb, 0)
    u64, in64 = R.unit_cube64(x, aabb, 0)
    rel = (np.abs(u32.astype(np.float64) - u64) / np.maximum(np.abs(u64), 1.0)).max()
    print(f"unit cube mode 0: max relative |fp32 - fp64| = {rel:.2e} (|u| up to {np.abs(u64).max():.3e})")
    assert rel <= CUBE0_BAR
    u32, in32 = R.unit_cube32(x, aabb, 1)
    u64, in64 = R.unit_cube64(x, aabb, 1)
    err = np.abs(u32.astype(np.float64) - u64).max()
    print(f"unit cube mode 1: max |fp32 - fp64| = {err:.2e}")
    assert err <= CUBE1_BAR
    assert u64.min() > 0 and u64.max() < 1 and in64.all()
    # the box itself maps to [0.25, 0.75]^3, uncontracted
    box = m < 1
    assert (np.abs(u64[box] - 0.5) < 0.25).all()
    # the torch form in fp32 is the numpy form's bits, in both modes
    for mode in (0, 1):
        ut, it = R.unit_cube_torch(torch.from_numpy(x), torch.from_numpy(aabb), mode)
        un, inn = R.unit_cube32(x, aabb, mode)
        assert np.array_equal(ut.numpy(), un) and np.array_equal(it.numpy(), inn)


def test_unit_cube_edge_rows():
    aabb = np.array([-1, -2, 0, 1, 2, 4], dtype=np.float32)
    x = np.array([[0, 0, 2],             # the centre
                  [1, 0, 2],             # on a face: u = 1 (mode 0), m = 1 exactly (mode 1: not contracted)
                  [-1, 0, 2],            # on the opposite face: u = 0
                  [1e6, 0, 2],           # far away
                  [np.nan, 0, 2]], dtype=np.float32)
    u, ins = R.unit_cube32(x, aabb, 0)
    assert np.array_equal(u[0], [0.5, 0.5, 0.5]) and ins[0] == 1
    assert u[1, 0] == 1 and ins[1] == 0 and u[2, 0] == 0 and ins[2] == 0 and ins[3] == 0
    assert np.isnan(u[4, 0]) and ins[4] == 0
    u, ins = R.unit_cube32(x, aabb, 1)
    assert np.array_equal(u[0], [0.5, 0.5, 0.5]) and u[1, 0] == 0.75 and u[2, 0] == 0.25 and ins[:3].all()
    assert 0.99 < u[3, 0] < 1 and ins[3] == 1
    assert np.isnan(u[4, 0]) and ins[4] == 0 and np.array_equal(u[4, 1:], [0.5, 0.5])


def _no_tie_points(n, seed):
    x, aabb = R.field_points(n, seed)
    a = aabb.astype(np.float64)
    c = np.sort(np.abs((x - a[:3]) / (a[3:] - a[:3]) * 2 - 1), axis=1)
    keep = (c[:, 2] - c[:, 1] > 1e-3 * c[:, 2]) & (np.abs(c[:, 2] - 1) > 1e-3)
    return x[keep], aabb


def test_sh_jacobian_against_differences_and_autograd():
    d = R.unit_dirs(500, seed=3).astype(np.float64)
    J = R.sh_jac64(d, 4)
    h = 1e-6
    for a in range(3):
        e = np.zeros(3)
        e[a] = h
        fd = (R.sh64(d + e, 4) - R.sh64(d - e, 4)) / (2 * h)
        assert np.abs(fd - J[:, :, a]).max() < 1e-8
    g = np.random.default_rng(0).standard_normal((500, 16))
    dt = torch.tensor(d, requires_grad=True)
    (R.sh_torch(dt, 4) * torch.tensor(g)).sum().backward()
    assert np.abs(dt.grad.numpy() - R.sh_bwd64(d, g, 4)).max() < 1e-12
    for degree in (1, 2, 3):
        assert np.array_equal(R.sh_jac64(d, degree), J[:, :degree * degree])


@pytest.mark.parametrize("mode", [0, 1])
def test_unit_cube_jacobian_against_differences_and_autograd(mode):
    x, aabb = _no_tie_points(3000, seed=5)
    x = x[R.contraction_m(x, aabb) < 1e3].astype(np.float64)                # differences need |x| h-resolvable
    assert x.shape[0] > 1000
    J = R.unit_cube_jac64(x, aabb, mode)
    h = 1e-6
    for i in range(3):
        e = np.zeros(3)
        e[i] = h
        fd = (R.unit_cube64(x + e, aabb, mode)[0] - R.unit_cube64(x - e, aabb, mode)[0]) / (2 * h)
        err = np.abs(fd - J[:, :, i]).max()
        assert err < 1e-7, (mode, i, err)
    g = np.random.default_rng(1).standard_normal(x.shape)
    xt = torch.tensor(x, requires_grad=True)
    u, inside = R.unit_cube_torch(xt, torch.tensor(aabb.astype(np.float64)), mode)
    assert not inside.requires_grad
    (u * torch.tensor(g)).sum().backward()
    ref = R.unit_cube_bwd64(x, aabb, mode, g)
    assert np.abs(xt.grad.numpy() - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())
    if mode == 1:
        # dy_k / dc_k = 1 / m^2 on the axis that attains m
        far = R.contraction_m(x, aabb) > 1
        a = aabb.astype(np.float64)
        c = (x - a[:3]) / (a[3:] - a[:3]) * 2 - 1
        k = np.abs(c).argmax(axis=1)
        m = np.abs(c).max(axis=1)
        rows = np.arange(x.shape[0])
        diag = J[rows, k, k] * 2 * (a[3:] - a[:3])[k]
        assert np.allclose(diag[far], 1 / m[far] ** 2, rtol=1e-12)


def test_trunc_exp_matches_its_definition():
    from nerf_amd.model_ngp import trunc_exp
    x = torch.tensor([-30.0, -1.0, 0.0, 3.5, 14.999, 15.0, 15.001, 20.0], dtype=torch.float64, requires_grad=True)
    g = torch.tensor([1.0, -2.0, 0.5, 3.0, 1.0, 1.0, -1.0, 2.0], dtype=torch.float64)
    y = trunc_exp(x)
    assert torch.equal(y, torch.exp(x.detach()))
    y.backward(g)
    assert torch.equal(x.grad, g * torch.exp(x.detach().clamp(max=15)))
    assert x.grad[-1] == 2.0 * np.exp(15.0) and y[-1] == np.exp(20.0)
    x32 = torch.tensor([20.0, 1.0], requires_grad=True)
    trunc_exp(x32).sum().backward()
    assert torch.equal(x32.grad, torch.exp(torch.tensor([15.0, 1.0])))


def test_hash_encoding_subclass_takes_unit_cube_points():
    """The struct field the kernels read: no x / 8 + 0.5.  The oracle's encode(normalize=False) is the
    statement the GPU test holds the subclass to."""
    from nerf_amd.model_ingp import INGPEncoding
    from nerf_amd.model_ngp import UnitCubeHashEncoding
    enc = UnitCubeHashEncoding(64, 4, 2 ** 10, 2, 4)
    assert isinstance(enc, INGPEncoding)
    p = enc._params()
    assert p.normalize == 0 and p.levels == 4 and p.features == 2 and p.table_size == 2 ** 10
    assert INGPEncoding(64, 4, 2 ** 10, 2, 4)._params().normalize == 1
    assert [p.res[l] for l in range(4)] == enc.resolutions == [4, 10, 25, 64]     # floor in fp32 tensor arithmetic
    kinds = [(r + 1) ** 3 <= 2 ** 10 for r in enc.resolutions]
    assert any(kinds) and not all(kinds)                                    # bijective and hashed levels
    assert [e.table.shape[0] for e in enc.encodings] == [O.level_rows(r, 2 ** 10) for r in enc.resolutions]
    assert enc.padded_dim == 32 and enc.output_dim == 8


def test_field_layout_and_cpu_tensors_raise():
    import nerf_amd
    from nerf_amd import NGPRadianceField, SHEncoding, contract_to_unisphere
    f = NGPRadianceField([-1, -1, -1, 1, 1, 1], n_levels=4, log2_hashmap_size=10, max_resolution=64,
                         base_resolution=4)
    assert f.mlp_base[0].in_features == 8 and f.mlp_base[2].out_features == 16
    assert f.mlp_head[0].in_features == 16 + 15 and f.mlp_head[4].out_features == 3
    assert all(m.bias is not None for m in list(f.mlp_base) + list(f.mlp_head) if isinstance(m, torch.nn.Linear))
    d = NGPRadianceField([-1, -1, -1, 1, 1, 1])
    assert (d.n_levels, d.log2_hashmap_size, d.base_resolution, d.max_resolution, d.geo_feat_dim) == (16, 19, 16, 4096, 15)
    assert d.position_encoding.output_dim == 32 and not d.unbounded and d.use_viewdirs
    # the density plan holds the two density layers and nothing of the head
    dp, fp = f.density_plan(), f.plan()
    assert [lp.module for lp in dp.layers] == [f.mlp_base[0], f.mlp_base[2]]
    assert [lp.module for lp in fp.layers] == [f.mlp_base[0], f.mlp_base[2], f.mlp_head[0], f.mlp_head[2], f.mlp_head[4]]
    geo = fp.layers[2].sources[1]
    assert geo.kind == "act" and geo.layer == 1 and geo.cols == [-1] + list(range(15))
    assert SHEncoding(4).output_dim == 16 and SHEncoding(3).output_dim == 9 and SHEncoding(3).padded_dim == 32
    x = torch.zeros(4, 3)
    with pytest.raises(ValueError):
        f(x, x)
    with pytest.raises(ValueError):
        f.query_density(x)
    with pytest.raises(ValueError):
        SHEncoding()(x)
    with pytest.raises(ValueError):
        contract_to_unisphere(x, [-1, -1, -1, 1, 1, 1])
    with pytest.raises(ValueError):
        nerf_amd.normalize_to_aabb(x, [-1, -1, -1, 1, 1])
    with pytest.raises(ValueError):
        SHEncoding(5)
    with pytest.raises(ValueError):
        NGPRadianceField([-1, -1, -1, 1, 1, 1], num_dim=2)
    for name in ("NGPRadianceField", "SHEncoding", "contract_to_unisphere", "trunc_exp"):
        assert hasattr(nerf_amd, name)
    for name in ("nerf_sh_encode_fwd", "nerf_sh_encode_bwd", "nerf_unit_cube_fwd", "nerf_unit_cube_bwd"):
        assert name in nerf_amd._lib.EXPORTED_SYMBOLS


def test_entry_points_reject_bad_arguments_without_a_device():
    """Status codes that need no launch: bad degree / mode, n == 0, null or misaligned pointers, narrow rows."""
    import ctypes
    from nerf_amd import _lib
    lib = _lib.load()
    box = (ctypes.c_float * 6)(-1, -1, -1, 1, 1, 1)
    for degree in (0, 5, -1):
        assert lib.nerf_sh_encode_fwd(16, 3, 4, degree, 16, 16, None) == -1
        assert lib.nerf_sh_encode_bwd(16, 3, 4, degree, 16, 16, 16, 3, None) == -1
    for mode in (-1, 2):
        assert lib.nerf_unit_cube_fwd(16, 3, 4, box, mode, 16, 3, 16, None) == -1
        assert lib.nerf_unit_cube_bwd(16, 3, 4, box, mode, 16, 3, 16, 3, None) == -1
    assert lib.nerf_sh_encode_fwd(None, 3, 0, 4, None, 16, None) == 0
    assert lib.nerf_sh_encode_bwd(None, 3, 0, 4, None, 16, None, 3, None) == 0
    assert lib.nerf_unit_cube_fwd(None, 3, 0, box, 1, None, 3, None, None) == 0
    assert lib.nerf_unit_cube_bwd(None, 3, 0, box, 1, None, 3, None, 3, None) == 0
    assert lib.nerf_sh_encode_fwd(16, 3, -1, 4, 16, 16, None) == -1
    # null, misaligned, narrow
    assert lib.nerf_sh_encode_fwd(None, 3, 4, 4, 16, 16, None) == -1
    assert lib.nerf_sh_encode_fwd(16, 3, 4, 4, None, 16, None) == -1
    assert lib.nerf_sh_encode_fwd(18, 3, 4, 4, 16, 16, None) == -1
    assert lib.nerf_sh_encode_fwd(16, 2, 4, 4, 16, 16, None) == -1
    assert lib.nerf_sh_encode_fwd(16, 3, 4, 4, 16, 15, None) == -1
    assert lib.nerf_sh_encode_fwd(16, 3, 4, 3, 16, 8, None) == -1
    assert lib.nerf_sh_encode_bwd(16, 3, 4, 4, None, 16, 16, 3, None) == -1
    assert lib.nerf_sh_encode_bwd(16, 3, 4, 4, 16, 15, 16, 3, None) == -1
    assert lib.nerf_sh_encode_bwd(16, 3, 4, 4, 16, 16, 17, 3, None) == -1
    assert lib.nerf_sh_encode_bwd(16, 3, 4, 4, 16, 16, 16, 2, None) == -1
    assert lib.nerf_unit_cube_fwd(None, 3, 4, box, 0, 16, 3, 16, None) == -1
    assert lib.nerf_unit_cube_fwd(16, 3, 4, None, 0, 16, 3, 16, None) == -1
    assert lib.nerf_unit_cube_fwd(16, 3, 4, box, 0, 16, 2, 16, None) == -1
    assert lib.nerf_unit_cube_fwd(16, 2, 4, box, 0, 16, 3, 16, None) == -1
    assert lib.nerf_unit_cube_fwd(16, 3, 4, box, 0, 16, 3, 18, None) == -1
    assert lib.nerf_unit_cube_bwd(16, 3, 4, box, 1, None, 3, 16, 3, None) == -1
    assert lib.nerf_unit_cube_bwd(16, 3, 4, box, 1, 16, 3, None, 3, None) == -1
    assert lib.nerf_unit_cube_bwd(16, 3, 4, box, 1, 16, 3, 16, 2, None) == -1
    assert lib.nerf_unit_cube_bwd(16, 3, 4, box, 1, 17, 3, 16, 3, None) == -1
