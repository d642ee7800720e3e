"""Host-side checks of the packed training path (nerf_amd.occ_render): the restatements the GPU tests
compare against, the Python argument errors, the four new C-ABI symbols, and the renderer on a CPU
estimator.  No GPU.
"""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import _packed_train_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("nerf_packed_points_fwd", "nerf_packed_points_bwd", "nerf_distortion_fwd", "nerf_distortion_bwd")


@pytest.fixture(scope="module")
def case():
    return P.distortion_case()


def test_prefix_form_equals_the_direct_double_sum(case):
    """The contract's prefix form (loss and closed-form gradient) is the O(S^2) double sum with its
    autograd gradient, both in fp64: they differ by rounding only (values up to 0.40 and 2.7)."""
    w, t0, t1, seg, g_loss = case
    for g in (torch.ones_like(g_loss), g_loss):
        direct, d_grad = P.distortion_direct64(w, t0, t1, seg, g)
        prefix, p_grad = P.distortion_prefix(w, t0, t1, seg, torch.float64, g)
        print(f"loss {float((prefix - direct).abs().max()):.3e}  gradient {float((p_grad - d_grad).abs().max()):.3e}")
        assert float((prefix - direct).abs().max()) < 1e-14
        assert float((p_grad - d_grad).abs().max()) < 1e-13
    empty = [i for i, L in enumerate(P.LENGTHS) if L == 0]
    assert torch.all(direct[empty] == 0) and torch.all(prefix[empty] == 0)


def test_margin_of_the_distortion_bars(case):
    """The distances that set the GPU test's margin, for exactly its inputs (unit g_loss): the fp64
    accumulation rounded to fp32, which is the kernels' contract, lies within 1.4e-8 (loss) and 1.2e-7
    (gradient) of the direct sum, more than an order of magnitude inside the bars 2e-6 and 2e-5 + 1e-5
    rel; the eager fp32 prefix form is several times further out and still inside."""
    w, t0, t1, seg, g_loss = case
    one = torch.ones_like(g_loss)
    direct, d_grad = P.distortion_direct64(w, t0, t1, seg, one)
    assert 0.39 < float(direct.max()) < 0.41 and 2.6 < float(d_grad.abs().max()) < 2.8
    l64, g64 = P.distortion_prefix(w, t0, t1, seg, torch.float64, one)
    l32, g32 = P.distortion_prefix(w, t0, t1, seg, torch.float32, one)
    e = [float((l64.float().double() - direct).abs().max()), float((g64.float().double() - d_grad).abs().max()),
         float((l32.double() - direct).abs().max()), float((g32.double() - d_grad).abs().max())]
    print("fp64 rounded: loss %.3e gradient %.3e; eager fp32: loss %.3e gradient %.3e" % tuple(e))
    assert e[0] <= 1.4e-8 and e[1] <= 1.2e-7
    assert e[2] <= 2e-6 and torch.all((g32.double() - d_grad).abs() <= 2e-5 + 1e-5 * d_grad.abs())


def test_points_restatement_rounds_each_operation():
    """points_ref32 differs from the fused (fp64, rounded once) evaluation somewhere, and never by more
    than an ulp of the result's terms: it is the separately rounded form, not a contracted one."""
    rng = np.random.default_rng(3)
    o, d = rng.normal(size=(5, 3)).astype(np.float32), rng.normal(size=(5, 3)).astype(np.float32)
    ri = np.sort(rng.integers(0, 5, size=400))
    t0 = rng.uniform(0, 5, size=400).astype(np.float32)
    t1 = (t0 + rng.uniform(0.001, 0.1, size=400)).astype(np.float32)
    pos, dirs = P.points_ref32(o, d, ri, t0, t1)
    tm = ((t0 + t1) * np.float32(0.5)).astype(np.float64)
    fused = (o[ri].astype(np.float64) + tm[:, None] * d[ri].astype(np.float64)).astype(np.float32)
    assert np.array_equal(dirs, d[ri]) and not np.array_equal(pos, fused)
    np.testing.assert_allclose(pos, fused, rtol=0, atol=2e-6)
    bad, _ = P.points_ref32(o, d, np.array([0, 5, -1]), t0[:3], t1[:3])
    assert np.isfinite(bad[0]).all() and np.isnan(bad[1:]).all()
    g_o, g_d = P.points_bwd_ref64(np.array([0, 2, 2, 3]), t0[:3], t1[:3], np.ones((3, 3)), np.ones((3, 3)))
    assert np.array_equal(g_o, [[2] * 3, [0] * 3, [1] * 3]) and np.all(g_d[1] == 0)
    assert np.allclose(g_d[2], tm[2] + 1)


def test_distortion_argument_errors():
    from nerf_amd import distortion
    w = torch.rand(6)
    t0, t1 = torch.arange(6.0), torch.arange(6.0) + 1
    ri = torch.tensor([0, 0, 1, 1, 2, 2])
    with pytest.raises(ValueError, match="n_rays is required"):
        distortion(w, t0, t1, ri)
    with pytest.raises(ValueError, match="sorted ascending"):
        distortion(w, t0, t1, torch.tensor([0, 1, 0, 1, 2, 2]), 3)
    with pytest.raises(ValueError, match="int64"):
        distortion(w, t0, t1, ri.int(), 3)
    with pytest.raises(ValueError, match="int64"):
        distortion(w, t0, t1, ri[:5], 3)
    with pytest.raises(ValueError, match="float32"):
        distortion(w.double(), t0, t1, ri, 3)
    with pytest.raises(ValueError, match="one entry per sample"):
        distortion(w, t0[:5], t1, ri, 3)
    with pytest.raises(ValueError, match=r"\[n_rays, n_samples\]"):
        distortion(w, t0, t1)
    with pytest.raises(ValueError, match="share their shape"):
        distortion(w.view(2, 3), t0.view(3, 2), t1.view(2, 3))
    with pytest.raises(ValueError, match="n_rays = 5"):
        distortion(w.view(2, 3), t0.view(2, 3), t1.view(2, 3), None, 5)
    with pytest.raises(ValueError, match="ROCm device"):       # well-formed, but there is no CPU path
        distortion(w, t0, t1, ri, 3)
    with pytest.raises(ValueError, match="ROCm device"):
        distortion(w.view(2, 3), t0.view(2, 3), t1.view(2, 3))


def test_packed_points_argument_errors():
    from nerf_amd import packed_points
    o, d = torch.zeros(3, 3), torch.ones(3, 3)
    t0, t1 = torch.arange(6.0), torch.arange(6.0) + 1
    ri = torch.tensor([0, 0, 1, 1, 2, 2])
    with pytest.raises(ValueError, match=r"rays_o must be a float32 \[n_rays, 3\]"):
        packed_points(o.double(), d, ri, t0, t1)
    with pytest.raises(ValueError, match=r"rays_d must be a float32 \[n_rays, 3\]"):
        packed_points(o, torch.ones(3, 4), ri, t0, t1)
    with pytest.raises(ValueError, match="share their shape"):
        packed_points(o, torch.ones(4, 3), ri, t0, t1)
    with pytest.raises(ValueError, match="n_rays = 4"):
        packed_points(o, d, ri, t0, t1, n_rays=4)
    with pytest.raises(ValueError, match="one entry per sample"):
        packed_points(o, d, ri, t0, t1[:4])
    with pytest.raises(ValueError, match="flat"):
        packed_points(o, d, ri, t0.view(2, 3), t1.view(2, 3))
    with pytest.raises(ValueError, match="int64"):
        packed_points(o, d, ri.float(), t0, t1)
    with pytest.raises(ValueError, match="sorted ascending"):
        packed_points(o, d, ri.flip(0), t0, t1)
    for want_dirs in (True, False):                             # both reach the device check alike
        with pytest.raises(ValueError, match="ROCm device"):
            packed_points(o, d, ri, t0, t1, want_dirs=want_dirs)


def test_new_symbols_in_header_binding_and_library():
    from nerf_amd import _lib
    with open(os.path.join(ROOT, "include", "nerf_amd.h")) as f:
        header = f.read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.EXPORTED_SYMBOLS and name in exported, name
        assert getattr(lib, name).restype is _lib.c_i32
    assert lib.nerf_abi_version() == 10
    # the argument counts of the binding are the header's
    for name in NEW_SYMBOLS:
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % name, header).group(1)
        assert len(decl.split(",")) == len(_lib._SIGNATURES[name][1]), name


def test_entry_points_reject_bad_arguments_without_a_device():
    """Zero sizes succeed without a launch; null, misaligned and short-stride arguments are refused
    before any launch (no GPU is needed to see either)."""
    import ctypes
    from nerf_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(256)
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    ok, bad = 0, -1                                             # NERF_OK, NERF_ERR_INVALID_ARG
    assert lib.nerf_packed_points_fwd(None, None, 0, None, None, None, 5, None, 3, None, 3, None) == ok
    assert lib.nerf_packed_points_fwd(None, None, 5, None, None, None, 0, None, 3, None, 3, None) == ok
    assert lib.nerf_packed_points_bwd(None, 0, None, None, 5, None, 3, None, 3, None, None, None) == ok
    assert lib.nerf_distortion_fwd(None, None, None, None, 4, 0, None, None) == ok
    assert lib.nerf_distortion_bwd(None, None, None, None, 0, 4, None, None, None) == ok
    assert lib.nerf_packed_points_fwd(p, p, 1, p, p, p, 1, None, 3, None, 3, None) == bad        # null positions
    assert lib.nerf_packed_points_fwd(p, p, 1, p, p, p, 1, p, 2, None, 3, None) == bad           # stride < 3
    assert lib.nerf_packed_points_fwd(p, p, 1, p + 4, p, p, 1, p, 3, None, 3, None) == bad       # int64 at 4 mod 8
    assert lib.nerf_packed_points_fwd(p, p + 2, 1, p, p, p, 1, p, 3, None, 3, None) == bad       # float at 2 mod 4
    assert lib.nerf_packed_points_fwd(p, p, -1, p, p, p, 1, p, 3, None, 3, None) == bad
    assert lib.nerf_packed_points_bwd(p, 1, p, p, 1, None, 3, None, 3, p, p, None) == bad        # null g_positions
    assert lib.nerf_packed_points_bwd(p + 4, 1, p, p, 1, p, 3, None, 3, p, p, None) == bad
    assert lib.nerf_packed_points_bwd(p, 1, p, p, 1, p, 3, p, 2, p, p, None) == bad
    assert lib.nerf_distortion_fwd(p, p, p, p, 1, 1, None, None) == bad
    assert lib.nerf_distortion_fwd(p, p, p, p + 4, 1, 1, p, None) == bad
    assert lib.nerf_distortion_fwd(p, p + 1, p, p, 1, 1, p, None) == bad
    assert lib.nerf_distortion_bwd(p, p, p, p, 1, 1, None, p, None) == bad
    assert lib.nerf_distortion_bwd(p, p, p, p, 1, 1, p, p + 2, None) == bad


def test_renderer_on_a_cpu_estimator_raises_the_estimators_error():
    import nerf_amd
    from nerf_amd.occ_render import OccGridRenderer
    assert nerf_amd.OccGridRenderer is OccGridRenderer
    est = nerf_amd.OccGridEstimator([-1.0] * 3 + [1.0] * 3, resolution=8)
    calls = []

    def field(pos, dirs):
        calls.append(pos.shape)
        return pos, pos[:, 0]
    ren = OccGridRenderer(field, est, 0.05, 6.0, 1 / 64, render_bkgd=torch.ones(3))
    assert isinstance(ren, torch.nn.Module) and ren.estimator is est and "estimator.occs" in ren.state_dict()
    assert ren.training and ren.alpha_thre == 0.0 and ren.early_stop_eps == 1e-4
    with pytest.raises(RuntimeError, match="needs the estimator on a ROCm device"):
        ren(torch.zeros(4, 3), torch.ones(4, 3))
    assert not calls
    with pytest.raises(ValueError, match="before the first forward"):
        OccGridRenderer(field, est, 0.05, 6.0, 1 / 64).distortion_loss({})
    # update_grid is plain torch: it runs on the CPU estimator, with density_fn and without
    ball = lambda x: 20.0 * (x.norm(dim=-1) < 0.5).float()
    OccGridRenderer(field, est, 0.05, 6.0, 1 / 64, density_fn=ball).update_grid(0, n=16)
    assert 0 < int(est.binaries.sum()) < est.cells
    before = est.binaries.clone()
    ren.update_grid(5, n=16)                                    # not a multiple of n: nothing happens
    assert torch.equal(est.binaries, before) and not calls
    ren.update_grid(16, n=16)                                   # the field's density at a fixed direction
    assert calls == [torch.Size([est.cells, 3])]
