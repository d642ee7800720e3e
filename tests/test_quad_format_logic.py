"""The quad-split activation format on the host (kernels.quad_split_pack / quad_split_unpack,
include/nerf_amd.h) and the register budget of the kernels around it, checked on the compiled
gfx950 ISA (CPU: hipcc cross-compiles, nothing runs): no scratch and at least 2 waves per SIMD
for the fused field-MLP kernels and every linear_wgrad_x3_tr_kernel instantiation."""
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "nerf-experiments_amd")
HIPCC = "/opt/rocm/bin/hipcc"


def _values(rows, cols, seed):
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(rows, cols, generator=g) * 28.0 - 20.0
    sign = torch.where(torch.rand(rows, cols, generator=g) < 0.5, -1.0, 1.0)
    return torch.where(torch.rand(rows, cols, generator=g) < 0.5, torch.zeros(()), sign * torch.exp2(u))


def test_pack_layout_and_round_trip():
    from nerf_amd import kernels as K
    x = _values(19, 72, 1)
    q = K.quad_split_pack(x)
    assert q.shape == x.shape and q.dtype == torch.float32 and q.stride() == x.stride()
    hi = x.bfloat16()
    lo = (x - hi.float()).bfloat16()
    raw = q.view(torch.int16).view(19, 18, 8)                # per 4 columns: 16 bytes = 8 bf16
    assert torch.equal(raw[:, :, :4].reshape(19, 72), hi.view(torch.int16))
    assert torch.equal(raw[:, :, 4:].reshape(19, 72), lo.view(torch.int16))
    h, l = K.quad_split_unpack(q)
    assert torch.equal(h, hi.float()) and torch.equal(l, lo.float())
    # hi + lo carries x to 2^-16 (two 8-bit significands, round to nearest even: |x - hi| <= 2^-8 |x|,
    # |x - hi - lo| <= 2^-8 |x - hi|)
    nz = x != 0
    assert ((h.double() + l.double() - x.double()).abs()[nz] <= 2.0 ** -16 * x.double().abs()[nz]).all()
    # zeros (a ReLU's output, pad columns) stay zero in both halves
    assert (h[~nz] == 0).all() and (l[~nz] == 0).all()


def test_a_view_at_a_multiple_of_32_columns_is_format_local():
    from nerf_amd import kernels as K
    x = _values(7, 512, 2)
    q = K.quad_split_pack(x)
    assert torch.equal(q[:, 256:512], K.quad_split_pack(x[:, 256:512].contiguous()))
    assert torch.equal(q[:, 32:96], K.quad_split_pack(x[:, 32:96].contiguous()))


def test_pack_refuses_other_shapes():
    from nerf_amd import kernels as K
    with pytest.raises(ValueError):
        K.quad_split_pack(torch.zeros(3, 6))
    with pytest.raises(ValueError):
        K.quad_split_pack(torch.zeros(3, 8, dtype=torch.float64))
    with pytest.raises(ValueError):
        K.quad_split_unpack(torch.zeros(3, 6))


def _compile(tu, out_dir):
    out = os.path.join(out_dir, f"{tu}.s")
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "include"), "-I",
           os.path.join(PKG, "csrc"), "--cuda-device-only", "-S", os.path.join(PKG, "csrc", f"{tu}.hip"), "-o", out]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    return out


def _resources(path):
    """{mangled kernel name: {"ScratchSize": n, "Occupancy": n, "NumVgprs": n}} of a listing."""
    out, name = {}, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name = m.group(1)
            continue
        m = re.match(r"^; (ScratchSize|Occupancy|NumVgprs): (\d+)", line)
        if m and name:
            out.setdefault(name, {})[m.group(1)] = int(m.group(2))
    return {k: v for k, v in out.items() if "Occupancy" in v}


@pytest.fixture(scope="module")
def listings(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    d = str(tmp_path_factory.mktemp("quad_isa"))
    with ThreadPoolExecutor(max_workers=2) as ex:
        paths = list(ex.map(lambda tu: _compile(tu, d), ["linear_x3", "mlp_fused"]))
    return dict(zip(["linear_x3", "mlp_fused"], paths))


def test_tile_kernel_instantiations_keep_their_registers(listings):
    res = {k: v for k, v in _resources(listings["linear_x3"]).items() if "linear_wgrad_x3_tr_kernel" in k}
    assert len(res) == 10, sorted(res)                       # {ROW257, RAYS, plain} x JN x passes, as launched
    for k, v in res.items():
        assert v["ScratchSize"] == 0 and v["Occupancy"] >= 2 and v["NumVgprs"] <= 256, (k, v)


def test_fused_kernels_keep_their_registers(listings):
    res = {k: v for k, v in _resources(listings["mlp_fused"]).items() if "mlp_fused_kernel" in k}
    assert res
    for k, v in res.items():
        assert v["ScratchSize"] == 0 and v["Occupancy"] >= 2, (k, v)


# ------------------------------------------------------------------ which layers are stored quad-split
def _plans():
    import math
    from nerf_amd import BarfPositionalEncoding, FourierFeatures, NerfModel
    from nerf_amd.model_garf import ProposalNetwork, RadianceNetwork
    from nerf_amd.model_ingp import FourierFeatures as IngpFourier, INGPEncoding, NerfModelINGP
    from nerf_amd.positional_encodings import IntegratedBarfFourierFeatures
    torch.manual_seed(0)
    ipe = IntegratedBarfFourierFeatures(10, 10, 1.28, 6.4, True, 1.0, True)
    ipe.pixel_width_sigma = 0.0
    models = {
        "n2v": NerfModel(4, 256, True, True, 2, FourierFeatures(10, 2 * math.pi), FourierFeatures(4, 1.0)),
        "barf": NerfModel(4, 256, True, False, 2, BarfPositionalEncoding(10, 10.0, 0, 1, True, 1.0),
                          BarfPositionalEncoding(4, 4.0, 0, 1, True, 1.0)),
        "mip": NerfModel(4, 256, True, False, 2, ipe, BarfPositionalEncoding(4, 4, 1.28, 6.4, True, 1.0)),
        "garf_radiance": RadianceNetwork(0.5, 1.5),
        "garf_proposal": ProposalNetwork(0.5, 1.5),
        "ingp": NerfModelINGP(8, 256, INGPEncoding(1600, 16, 2 ** 16, 2, 16), IngpFourier(4)),
    }
    plans = {}
    for name, m in models.items():
        plan = m._get_plan()
        plan.to_device(torch.device("cpu"))
        plans[name] = plan
    return plans


@pytest.fixture(scope="module")
def plans():
    return _plans()


def _servable(plan, l, M, dir_rd):
    """Independent of mlp.split_layers: layer l's stored output has one reader, the next layer's
    first segment; it is no exposed or column output; and every weight-gradient launch that reads
    it — with and without the per-ray route — is a single 256 x 256 tile of at most 256 rows."""
    from nerf_amd import kernels as K, mlp
    lp = plan.layers[l]
    if l in plan.outputs or l in dict(plan.column_outputs) or lp.N > 256 or l == len(plan.layers) - 1:
        return False
    readers = [(c, si) for c, cl in enumerate(plan.layers) for si, s in enumerate(cl.sources)
               if s.kind == "act" and s.layer == l]
    if readers != [(l + 1, 0)] or any(cl.residual == l for cl in plan.layers):
        return False
    cl = plan.layers[l + 1]
    if cl.N == 257 or cl.gauss is not None:
        return False
    N4 = (cl.N + 3) // 4 * 4
    segs = [(None, s.k_seg, dir_rd if s.kind == "dir" else 1) for s in cl.sources]
    for rays in (True, False):
        for nr, piece in mlp.wgrad_launches(segs, N4, N4, M, rays):
            kp = sum(k for _, k in piece)
            if any(j == 0 for j, _ in piece) and not (K.WGRAD_TR and nr <= 256 and kp <= 256 and (nr > 128 or kp > 128)
                                                      and not (nr <= 16 and K.WGRAD_SMALLN)):
                return False
    return True


@pytest.mark.parametrize("M,rd", [(3 * 64 + 5, 1), (1000, 1), (128 * 3, 64), (4096 * 64, 64)])
def test_selection_on_the_model_plans(plans, M, rd, monkeypatch):
    from nerf_amd import mlp, mlp_fused
    assert mlp.CAPTURE is None
    assert mlp.split_layers(plans["mip"], M, rd) == frozenset() or mlp.SAVE_SPLIT     # the module switch
    monkeypatch.setattr(mlp, "SAVE_SPLIT", True)
    # NerfModel trunks: every hidden layer but the one feeding the 257-row layer (barf, mip), the
    # exposed feature layer and the 128-wide colour layer (its reader is the small-N kernel)
    assert mlp.split_layers(plans["n2v"], M, rd) == frozenset(range(9))
    assert mlp.split_layers(plans["barf"], M, rd) == frozenset(range(8))
    assert mlp.split_layers(plans["mip"], M, rd) == frozenset(range(8))
    # GARF's Gaussian layers never run the fused forward: nothing is selected
    assert mlp.split_layers(plans["garf_radiance"], M, rd) == frozenset()
    assert mlp.split_layers(plans["garf_proposal"], M, rd) == frozenset()
    for name, plan in plans.items():
        sel = mlp.split_layers(plan, M, rd)
        if sel:
            assert mlp_fused.dgrad_eligible(plan, M), name
        for l in range(len(plan.layers)):
            assert (l in sel) <= _servable(plan, l, M, rd), (name, l)
    assert mlp.split_layers(plans["ingp"], M, rd) == frozenset(
        l for l in range(len(plans["ingp"].layers)) if _servable(plans["ingp"], l, M, rd)
    ) or not mlp_fused.dgrad_eligible(plans["ingp"], M)


def test_selection_gates(plans, monkeypatch):
    from nerf_amd import mlp, mlp_fused
    plan = plans["mip"]
    monkeypatch.setattr(mlp, "SAVE_SPLIT", True)
    assert mlp.split_layers(plan, 1000, 1)
    monkeypatch.setattr(mlp, "CAPTURE", [])
    assert mlp.split_layers(plan, 1000, 1) == frozenset()
    monkeypatch.setattr(mlp, "CAPTURE", None)
    monkeypatch.setattr(mlp, "SAVE_SPLIT", False)
    assert mlp.split_layers(plan, 1000, 1) == frozenset()
    monkeypatch.setattr(mlp, "SAVE_SPLIT", True)
    monkeypatch.setattr(mlp_fused, "dgrad_eligible", lambda plan, M: False)
    assert mlp.split_layers(plan, 1000, 1) == frozenset()


def test_route_predicate_matches_the_launch_shapes():
    from nerf_amd import kernels as K, mlp
    assert K.wgrad_single_tile(256, 256) and K.wgrad_single_tile(257, 256) and K.wgrad_single_tile(256, 96)
    assert not K.wgrad_single_tile(64, 128) and not K.wgrad_single_tile(256, 288) and not K.wgrad_single_tile(260, 256)
    assert K.wgrad_single_tile(4, 256) != K.WGRAD_SMALLN
    assert K.wgrad_reads_quad_split(256, 256) == K.WGRAD_TR and not K.wgrad_reads_quad_split(257, 256)
    # the skip layer [trunk 256 | encoding 64]: two single-tile launches; the colour layer
    # [features 256 | per-ray directions 32]: the per-ray route, or one launch without it
    assert mlp.wgrad_launches([(None, 256, 1), (None, 64, 1)], 256, 256, 1024) == [(256, [(0, 256)]), (256, [(1, 64)])]
    assert mlp.wgrad_launches([(None, 256, 1), (None, 28, 64)], 128, 128, 1024) == [(128, [(0, 256)]), (128, [(1, 32)])]
    assert mlp.wgrad_launches([(None, 256, 1), (None, 28, 64)], 128, 128, 1024, rays=False) == [(128, [(0, 256), (1, 32)])]


def test_fused_mask_bits_to_maskout_layout():
    import numpy as np
    from nerf_amd import mlp
    rng = np.random.default_rng(3)
    alive = rng.random((9, 256)) < 0.5
    fused = np.zeros((9, 8), dtype=np.uint32)        # NERF_FUSED_MASK: set = dead
    want = np.zeros((9, 8), dtype=np.uint32)         # NERF_EPI_MASKOUT: set = alive
    for n in range(256):
        c, g, r = n // 16, (n // 4) % 4, n % 4
        fused[:, 2 * g + (c >> 3)] |= (~alive[:, n]).astype(np.uint32) << np.uint32(4 * (7 - (c & 7)) + r)
        e, h, b = n % 4, (n // 4) // 32, (n // 4) % 32
        want[:, 2 * e + h] |= alive[:, n].astype(np.uint32) << np.uint32(b)
    got = mlp.fused_mask_to_maskout(torch.from_numpy(fused.view(np.uint8).reshape(9, 32).copy()))
    assert got.dtype == torch.uint8 and got.shape == (9, 32)
    assert np.array_equal(got.numpy().view(np.uint32).reshape(9, 8), want)
