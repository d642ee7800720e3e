"""2-D hash-grid image fit (nerf_amd.model_ingp2d, nerf_hashgrid2d_*): what holds without a GPU.

The fixture tests/golden/ingp2d.npz comes from the reference's own 2d-ingp/model.py
(tests/golden/make_golden_ingp2d.py); tests/_ingp2d_ref.py holds the restatements the GPU tests
compare against, pinned here to that fixture and to oracle/hashgrid_oracle.py.
"""
import copy
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import torch as th

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ingp2d_ref as R  # noqa: E402

CONFIGS = {"A": dict(enc=(64, 4, 2 ** 8, 2, 5), n_hidden=2), "B": dict(enc=(100, 3, 1000, 4, 4), n_hidden=0)}
# the three gradient shapes of the GPU tests: (resolutions, T, F, points)
MAIN = dict(res=R.schedule(2048, 16, 16), T=2 ** 16, F=2)


def _build(tag):
    from nerf_amd import model_ingp2d as M
    th.manual_seed(0)
    enc = M.INGPEncoding(*CONFIGS[tag]["enc"])
    return M.Gigapixel(CONFIGS[tag]["n_hidden"], 64, enc)


def test_class_signatures_mirror_the_reference():
    from nerf_amd import model_ingp2d as M
    import nerf_amd
    sig = lambda c: list(inspect.signature(c.__init__).parameters)[1:]
    assert sig(M.INGPTable) == ["resolution", "table_size", "n_features", "pi1", "pi2"]
    assert sig(M.INGPEncoding) == ["resolution_max", "resolution_min", "table_size", "n_features", "n_levels", "pi1",
                                   "pi2"]
    d = inspect.signature(M.INGPEncoding.__init__).parameters
    assert d["pi1"].default == 1 and d["pi2"].default == 2654435761
    assert sig(M.Gigapixel) == ["n_hidden", "hidden_dim", "position_encoder"]
    assert nerf_amd.Gigapixel is M.Gigapixel
    # the package's INGPTable / INGPEncoding stay the 3-D ones
    assert nerf_amd.INGPEncoding is not M.INGPEncoding and nerf_amd.INGPTable is not M.INGPTable


@pytest.mark.parametrize("tag", ["A", "B"])
def test_state_dict_keys_and_init_checksums(golden, tag):
    g = golden("ingp2d")
    model = _build(tag)
    sd = model.state_dict()
    assert list(sd.keys()) == [str(k) for k in g[f"{tag}.keys"]]
    for k, v in sd.items():
        want = g[f"{tag}.sdsum.{k}"]
        got = np.array([v.double().sum().item(), v.double().abs().sum().item()])
        assert np.array_equal(got, want), k
        assert tuple(v.shape) == g[f"{tag}.sd.{k}"].shape, k
    enc = model.position_encoder
    assert enc.resolutions == [int(r) for r in g[f"{tag}.res"]]
    assert [bool(e.bijective) for e in enc.encodings] == [bool(b) for b in g[f"{tag}.bijective"]]
    assert enc.output_dim == CONFIGS[tag]["enc"][3] * CONFIGS[tag]["enc"][4]


def test_main_schedule_ends_at_2047():
    from nerf_amd import model_ingp2d as M
    enc = M.INGPEncoding(2048, 16, 2 ** 4, 1, 16)
    assert enc.resolutions == MAIN["res"] and enc.resolutions[0] == 16 and enc.resolutions[-1] == 2047
    assert sum(R.level_rows(r, MAIN["T"]) for r in MAIN["res"]) == 554051


def _views_ok(enc):
    buf = enc.packed_table()
    off = 0
    for e in enc.encodings:
        assert e.table.data_ptr() == buf.data_ptr() + off * enc.n_features * 4
        off += e.table.shape[0]
    assert off == buf.shape[0]


def test_packed_views_survive_load_and_copy(golden):
    g = golden("ingp2d")
    model = _build("A")
    enc = model.position_encoder
    _views_ok(enc)
    model.load_state_dict({str(k): th.from_numpy(g[f"A.sd.{k}"]) for k in g["A.keys"]})
    _views_ok(enc)
    want = np.concatenate([g[f"A.sd.position_encoder.encodings.{l}.table"] for l in range(5)])
    assert np.array_equal(enc.packed_table().numpy(), want)
    twin = copy.deepcopy(model)
    _views_ok(twin.position_encoder)
    assert np.array_equal(twin.position_encoder.packed_table().numpy(), want)
    assert twin.position_encoder.packed_table().data_ptr() != enc.packed_table().data_ptr()
    # a reassigned level is packed again on the next use
    enc.encodings[1].table = th.nn.Parameter(th.ones_like(enc.encodings[1].table))
    _views_ok(enc)
    assert float(enc.packed_table()[25:106].min()) == 1.0


def test_pixel_centres_bitwise():
    from nerf_amd.model_ingp2d import pixel_centres
    for res in (1, 16, 61, 2048):
        x, y = th.meshgrid(th.arange(res), th.arange(res), indexing="ij")
        x, y = x.flatten(), y.flatten()
        want = th.hstack((x.float().unsqueeze(1) / res, y.float().unsqueeze(1) / res))
        want += 1 / 2 / res
        got = pixel_centres(res)
        assert got.shape == (res * res, 2) and th.equal(got, want)


@pytest.mark.parametrize("tag", ["A", "B"])
def test_restatements_bitwise_the_fixture(golden, tag):
    from oracle import hashgrid_oracle as O
    g = golden("ingp2d")
    T, F = CONFIGS[tag]["enc"][2], CONFIGS[tag]["enc"][3]
    x = g["x"]
    model = R.fixture_model(g, tag, T, F, CONFIGS[tag]["n_hidden"])
    with th.no_grad():
        feat = model.position_encoder(th.from_numpy(x)).numpy()
        rgb = model(th.from_numpy(x)).numpy()
    assert np.array_equal(feat, g[f"{tag}.features"])
    assert np.array_equal(rgb, g[f"{tag}.rgb"])
    res = [int(r) for r in g[f"{tag}.res"]]
    tables = [g[f"{tag}.sd.position_encoder.encodings.{l}.table"] for l in range(len(res))]
    got, status = R.encode(x, tables, res, T)
    assert status == 0
    assert np.array_equal(got, g[f"{tag}.features"])
    assert np.array_equal(got, O.encode_2d(x, tables, res, T))
    # autograd's table gradient of the restatement against the fixture's
    model.zero_grad()
    loss = th.nn.functional.mse_loss(model(th.from_numpy(x)), th.from_numpy(g["y"]))
    loss.backward()
    assert np.array_equal(loss.detach().numpy(), g[f"{tag}.loss"])
    for k, p in model.named_parameters():
        ref = g[f"{tag}.grad.{k}"]
        assert np.abs(p.grad.numpy() - ref).max() <= 1e-6 * max(np.abs(ref).max(), 1e-30), k


def _grad_case(name):
    rng = np.random.default_rng(5)
    if name == "main":
        res, T, F, n = MAIN["res"], MAIN["T"], MAIN["F"], 20000
        x = rng.random((n, 2), dtype=np.float32)
    elif name == "B":
        res, T, F, n = R.schedule(100, 3, 4), 1000, 4, 257
        x = rng.random((n, 2), dtype=np.float32)
    else:
        res, T, F, n = R.schedule(64, 4, 5), 256, 8, 4096
        x = np.tile(np.array([[0.3183, 0.7071]], dtype=np.float32), (n, 1))
    g = rng.standard_normal((n, len(res) * F)).astype(np.float32)
    return x, g, res, T, F


@pytest.mark.parametrize("name", ["main", "B", "contended"])
def test_fixed_point_gradient_against_fp64_scatter(name):
    x, g, res, T, F = _grad_case(name)
    fixed = R.table_grad_fixed(x, g, res, T, F)
    ref = R.table_grad_f64(x, g, res, T, F)
    assert fixed.dtype == np.float32 and fixed.shape == ref.shape
    err = np.abs(fixed.astype(np.float64) - ref).max() / np.abs(ref).max()
    print(f"{name}: max |fixed - fp64| / max |ref| = {err:.3e}")
    assert err <= 1e-6


def test_fixed_point_rule_edges():
    res, T, F = [3, 9], 1000, 1
    x = np.array([[0.25, 0.5], [1.5, 0.5]], dtype=np.float32)
    g = np.ones((2, 2), dtype=np.float32)
    assert R.fixed_shift(0.0, 5) == 60 and R.fixed_shift(float("inf"), 5) is None
    assert R.fixed_shift(1.0, 1) == 62 - 3          # 4 < 2^3
    assert R.fixed_shift(1e-38, 1) == 120
    full = R.table_grad_fixed(x, g, res, T, F)
    only = R.table_grad_fixed(x[:1], g[:1], res, T, F)
    assert np.array_equal(full, only)               # the out-of-domain point adds nothing
    assert np.isnan(R.table_grad_fixed(x, g * np.float32("nan"), res, T, F)).all()
    _, status = R.encode(x, [np.ones((16, 1), np.float32), np.ones((100, 1), np.float32)], res, T)
    assert status == 1


def test_cpu_tensors_raise_value_error():
    from nerf_amd import kernels as K
    from nerf_amd import model_ingp2d as M
    p = K.make_hashgrid_params(2, 1000, 1, [3, 9], 0, primes=(1, 2654435761, 0), normalize=False)
    assert K.hashgrid2d_level_rows(3, 1000) == 16 and K.hashgrid2d_level_rows(31, 1000) == 1000
    assert K.hashgrid2d_table_rows(p) == 116
    x, table, out = th.zeros(4, 2), th.zeros(116, 1), th.zeros(4, 2)
    with pytest.raises(ValueError):
        K.hashgrid2d_fwd(p, table, out, x)
    with pytest.raises(ValueError):
        K.hashgrid2d_bwd(p, out, table, th.zeros(4096, dtype=th.int64), x)
    enc = M.INGPEncoding(9, 3, 1000, 1, 2)
    with pytest.raises(ValueError):
        enc(x)
    with pytest.raises(ValueError):
        enc.encodings[0](x)
    with pytest.raises(ValueError):
        M.Gigapixel(0, 64, enc)(x)
    with pytest.raises(ValueError, match="gradient"):
        enc(x.clone().requires_grad_(True))
    with pytest.raises(ValueError):
        enc(th.zeros(4, 3))


def _params(levels=2, T=1000, F=2, normalize=0, res=(3, 9)):
    from nerf_amd import _lib
    p = _lib.NerfHashgridParams()
    p.levels, p.table_size, p.features, p.query, p.normalize = levels, T, F, 0, normalize
    p.primes[0], p.primes[1], p.primes[2] = 1, 2654435761, 0
    for i, r in enumerate(res):
        p.res[i] = r
    return p


def test_entry_points_reject_bad_arguments_without_a_launch():
    """Every call below returns before any HIP call: this machine has no device to launch on, and the
    pointers are made-up addresses that a launch would fault on."""
    from nerf_amd import _lib
    lib = _lib.load()
    A = 1 << 20                                     # a 256-byte aligned made-up address
    ok = _params()
    need = lib.nerf_hashgrid2d_workspace(ctypes.byref(ok))
    assert lib.nerf_hashgrid2d_table_rows(ctypes.byref(ok), 0) == 16
    assert lib.nerf_hashgrid2d_table_rows(ctypes.byref(ok), 1) == 100
    assert lib.nerf_hashgrid2d_table_rows(ctypes.byref(ok), -1) == 116
    assert lib.nerf_hashgrid2d_table_rows(ctypes.byref(ok), 2) == -1
    assert need == 256 + 116 * 2 * 8

    def fwd(p, n=4, x=A, table=A, out=A, ld=4):
        return lib.nerf_hashgrid2d_fwd(ctypes.byref(p), x, n, table, out, ld, None, None)

    def bwd(p, n=4, x=A, g=A, ld=4, gt=A, ws=A, nbytes=need):
        return lib.nerf_hashgrid2d_bwd(ctypes.byref(p), x, n, g, ld, gt, 0, ws, nbytes, None)

    bad = [_params(levels=0), _params(levels=33), _params(F=0), _params(F=9), _params(normalize=1),
           _params(res=(3, 0)), _params(T=0)]
    for p in bad:
        assert fwd(p) == -1 and bwd(p) == -1
        assert lib.nerf_hashgrid2d_table_rows(ctypes.byref(p), -1) == -1
        assert lib.nerf_hashgrid2d_workspace(ctypes.byref(p)) == 0
    assert lib.nerf_hashgrid2d_fwd(None, A, 4, A, A, 4, None, None) == -1
    assert fwd(ok, ld=3) == -1 and bwd(ok, ld=3) == -1
    assert fwd(ok, n=-1) == -1 and bwd(ok, n=-1) == -1
    assert bwd(ok, nbytes=need - 1) == -4
    assert bwd(ok, ws=A + 8, nbytes=need + 8) == -1
    assert bwd(ok, ws=None) == -1
    for name in ("x", "table", "out"):
        assert fwd(ok, **{name: None}) == -1
    for name in ("x", "g", "gt"):
        assert bwd(ok, **{name: None}) == -1
    # n == 0 succeeds and launches nothing (null pointers are then fine)
    assert fwd(ok, n=0, x=None, table=None, out=None) == 0
    assert lib.nerf_hashgrid2d_bwd(ctypes.byref(ok), None, 0, None, 4, None, 1, None, 0, None) == 0
    assert lib.nerf_hashgrid2d_bwd(ctypes.byref(ok), None, 0, None, 4, None, 0, None, 0, None) == 0
    assert bwd(ok, n=0, nbytes=need - 1) == -4
