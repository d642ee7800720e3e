"""Occupancy-grid marching (csrc/occgrid.hip: nerf_occ_march_count / nerf_occ_march_write) and
nerf_amd.occ_grid.OccGridEstimator.sampling against the numpy fp32 restatement of the marching
contract, tests/_occgrid_ref.py::march_ref: ray_indices, t_starts and t_ends bit for bit, no case
left out.  The C-ABI calls write into buffers guarded by a NaN pattern (tests/_guarded.py): no store
may land outside the N samples the counts name.
"""
import numpy as np
import pytest
import torch

import _occgrid_ref as R
from _guarded import GUARD, SENTINEL, Guarded

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _lib():
    import nerf_amd
    nerf_amd._lib.load()  # fail loudly if the HIP library is missing
    yield


def estimator(aabb, res, binaries):
    from nerf_amd import OccGridEstimator
    est = OccGridEstimator(aabb, resolution=list(res)).to(DEV)
    est.binaries.copy_(torch.from_numpy(np.asarray(binaries)).reshape(est.binaries.shape))
    return est


def march_guarded(est, o, d, near, far, dt, stratified=False, seed=0, mask_words=None):
    """Both passes through the kernel wrappers' C calls with guarded outputs: (ray_indices, t_starts,
    t_ends, status, counts) on the host."""
    import nerf_amd
    from nerf_amd import kernels as K
    lib = nerf_amd._lib.load()
    o, d = torch.from_numpy(o).to(DEV).contiguous(), torch.from_numpy(d).to(DEV).contiguous()
    n = o.shape[0]
    words = mask_words or K.occ_mask_words(near, far, dt)
    nbytes = K.occ_march_workspace_bytes(n, words)
    ws = Guarded((nbytes + 3) // 4, dtype=torch.int32)
    # the guard sits 4096 bytes into a torch allocation: the body is 256-byte aligned
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    counts = K.occ_march_count(o, d, est.aabb, est.resolution, est.grid_bits(), near, far, dt, stratified, seed, words,
                               ws.body, status)
    offsets = torch.cumsum(counts, 0)
    total = int(offsets[-1]) if n else 0
    ri, t0, t1 = Guarded(total, dtype=torch.int64), Guarded(total), Guarded(total)
    st = lib.nerf_occ_march_write(n, dt, words, ws.ptr(), nbytes, offsets.data_ptr() if n else None, total, ri.ptr(),
                                  t0.ptr(), t1.ptr(), torch.cuda.current_stream().cuda_stream)
    assert st == 0
    torch.cuda.synchronize()
    for buf, what in ((ri, "ray_indices"), (t0, "t_starts"), (t1, "t_ends")):
        buf.check(what)
    guards = torch.cat([ws.flat[:GUARD], ws.flat[-GUARD:]]).cpu()     # the body is scratch; its guards are not
    assert int((guards != SENTINEL).sum()) == 0, "workspace: stores outside its bytes"
    return ri.body.cpu().numpy(), t0.body.cpu().numpy(), t1.body.cpu().numpy(), int(status.item()), counts.cpu().numpy()


def same(got, ref, what):
    ri, t0, t1 = got[:3]
    assert ri.shape == ref[0].shape, f"{what}: {ri.size} samples, the restatement has {ref[0].size}"
    assert np.array_equal(ri, ref[0]), f"{what}: ray_indices differ"
    assert np.array_equal(t0.view(np.uint32), ref[1].view(np.uint32)), f"{what}: t_starts differ in their bits"
    assert np.array_equal(t1.view(np.uint32), ref[2].view(np.uint32)), f"{what}: t_ends differ in their bits"
    assert got[3] == ref[3], f"{what}: status {got[3]}, the restatement has {ref[3]}"


def test_count_construction():
    """All eight rays d = (1/m, 0, 0) in one call: exactly m samples each, abutting bitwise."""
    cases = [R.count_construction(m) for m in R.COUNT_M]
    o = np.concatenate([c[0] for c in cases])
    d = np.concatenate([c[1] for c in cases])
    _, _, aabb, res, binaries, near, far, dt = cases[0]
    est = estimator(aabb, res, binaries)
    ref = R.march_ref(o, d, aabb, res, binaries, near, far, dt)
    got = march_guarded(est, o, d, near, far, dt)
    same(got, ref, "count construction")
    assert list(got[4]) == list(R.COUNT_M)
    ri, t0, t1 = got[:3]
    inner = ri[:-1] == ri[1:]
    assert np.array_equal(t1[:-1][inner].view(np.uint32), t0[1:][inner].view(np.uint32))
    # the estimator's own call returns the same bits
    ri2, t02, t12 = est.sampling(torch.from_numpy(o).to(DEV), torch.from_numpy(d).to(DEV), near_plane=near,
                                 far_plane=far, render_step_size=dt)
    assert ri2.dtype == torch.int64 and t02.dtype == torch.float32
    same((ri2.cpu().numpy(), t02.cpu().numpy(), t12.cpu().numpy(), 0), ref, "sampling")


def test_checkerboard():
    o, d, aabb, res, binaries, near, far, dt = R.checkerboard_case()
    est = estimator(aabb, res, binaries)
    ref = R.march_ref(o, d, aabb, res, binaries, near, far, dt)
    same(march_guarded(est, o, d, near, far, dt), ref, "checkerboard")


@pytest.mark.parametrize("n_rays", [0, 1])
def test_few_rays(n_rays):
    o, d, aabb, res, binaries, near, far, dt = R.checkerboard_case()
    est = estimator(aabb, res, binaries)
    o, d = o[5:5 + n_rays], d[5:5 + n_rays]
    ref = R.march_ref(o, d, aabb, res, binaries, near, far, dt)
    same(march_guarded(est, o, d, near, far, dt), ref, f"{n_rays} rays")
    out = est.sampling(torch.from_numpy(o).to(DEV), torch.from_numpy(d).to(DEV), near_plane=near, far_plane=far,
                       render_step_size=dt)
    assert out[0].numel() == ref[0].size and (n_rays == 0 or ref[0].size > 0)


def test_ray_reaches_the_step_limit():
    """One ray whose chord holds more than NERF_OCC_MAX_STEPS steps: status bit 0, exactly 8192 steps
    considered (all kept: the grid is full), next to a ray that stays below the limit."""
    aabb, res, binaries = [0.0, 0.0, 0.0, 1.0, 1.0, 1.0], (4, 4, 4), np.ones((4, 4, 4), dtype=bool)
    o = np.array([[-1.0, 0.5, 0.5], [-1.0, 0.25, 0.75]], dtype=np.float32)
    d = np.array([[1.0, 0.0, 0.0], [4.0, 0.0, 0.0]], dtype=np.float32)
    dt = 1.0 / 10000
    est = estimator(aabb, res, binaries)
    ref = R.march_ref(o, d, aabb, res, binaries, 0.0, 1e9, dt)
    assert ref[3] == 1 and list(ref[4]) == [R.MAX_STEPS, 2500]
    got = march_guarded(est, o, d, 0.0, 1e9, dt)
    same(got, ref, "step limit")
    assert got[3] == 1 and list(got[4]) == [R.MAX_STEPS, 2500]


def test_stratified_with_a_fixed_seed():
    from nerf_amd.model_interpolation import _rng_seed
    o, d, aabb, res, binaries, near, far, dt = R.checkerboard_case()
    est = estimator(aabb, res, binaries)
    torch.manual_seed(77)
    seed = _rng_seed()
    ref = R.march_ref(o, d, aabb, res, binaries, near, far, dt, stratified=True, seed=seed)
    plain = R.march_ref(o, d, aabb, res, binaries, near, far, dt)
    assert not np.array_equal(ref[1][:8], plain[1][:8])
    same(march_guarded(est, o, d, near, far, dt, stratified=True, seed=seed), ref, "stratified")
    torch.manual_seed(77)                                   # sampling draws the same seed itself
    ri, t0, t1 = est.sampling(torch.from_numpy(o).to(DEV), torch.from_numpy(d).to(DEV), near_plane=near,
                              far_plane=far, render_step_size=dt, stratified=True)
    same((ri.cpu().numpy(), t0.cpu().numpy(), t1.cpu().numpy(), 0), ref, "stratified sampling")


def test_packed_bits_follow_the_grid():
    """The kernel's bit-packed copy is rebuilt after an in-place write, load_state_dict and .to()."""
    o, d, aabb, res, binaries, near, far, dt = R.checkerboard_case()
    od = (torch.from_numpy(o).to(DEV), torch.from_numpy(d).to(DEV))
    kw = dict(near_plane=near, far_plane=far, render_step_size=dt)
    est = estimator(aabb, res, np.zeros_like(binaries))
    assert est.sampling(*od, **kw)[0].numel() == 0
    est.binaries.copy_(torch.from_numpy(binaries).reshape(est.binaries.shape))
    ref = R.march_ref(o, d, aabb, res, binaries, near, far, dt)
    assert est.sampling(*od, **kw)[0].numel() == ref[0].size
    from nerf_amd import OccGridEstimator
    other = OccGridEstimator(aabb, resolution=list(res))
    other.grid_bits()
    other.load_state_dict(est.state_dict())
    other = other.to(DEV)
    got = other.sampling(*od, **kw)
    same(tuple(x.cpu().numpy() for x in got) + (0,), ref, "after load_state_dict and .to()")


def test_visibility_filter():
    """sampling with sigma_fn, alpha_thre and early_stop_eps keeps exactly the samples the same filter
    keeps on the restatement's output (alpha and transmittance from the fp64 packed restatement; the
    thresholds are placed in gaps of the reference values wider than the kernels' 2e-6 bar, so the
    fp32 and fp64 decisions agree), and alpha_fn gives the same selection as its sigma_fn."""
    o, d, aabb, res, binaries, near, far, dt = R.checkerboard_case()
    est = estimator(aabb, res, binaries)
    ref = R.march_ref(o, d, aabb, res, binaries, near, far, dt)
    ri, t0, t1 = (torch.from_numpy(x) for x in ref[:3])
    sigma_of = lambda a, b: 8.0 + 6.0 * torch.sin(7.0 * (a + b))
    seg = torch.searchsorted(ri, torch.arange(65))
    _, _, _, _, trans, alphas, _, _ = R.packed_composite_ref64(sigma_of(t0, t1), None, t0, t1, seg)

    def gap_threshold(values, target):
        v = torch.sort(values).values
        i = int(torch.searchsorted(v, torch.tensor(target, dtype=v.dtype)))
        for j in range(i, v.numel() - 1):
            if v[j + 1] - v[j] > 1e-4 * max(target, 1e-3) + 1e-5:
                return float((v[j] + v[j + 1]) / 2)
        raise AssertionError("no gap")

    alpha_thre = gap_threshold(alphas, 0.1)
    eps = gap_threshold(trans, 0.05)
    keep = ((alphas >= alpha_thre) & (trans >= eps)).numpy()
    assert 0.1 < keep.mean() < 0.9
    od = (torch.from_numpy(o).to(DEV), torch.from_numpy(d).to(DEV))
    kw = dict(near_plane=near, far_plane=far, render_step_size=dt, early_stop_eps=eps, alpha_thre=alpha_thre)
    got = est.sampling(*od, sigma_fn=lambda a, b, r: sigma_of(a, b), **kw)
    want = (ref[0][keep], ref[1][keep], ref[2][keep], 0)
    same(tuple(x.cpu().numpy() for x in got) + (0,), want, "sigma_fn filter")
    got = est.sampling(*od, alpha_fn=lambda a, b, r: 1.0 - torch.exp(-sigma_of(a, b) * (b - a)), **kw)
    same(tuple(x.cpu().numpy() for x in got) + (0,), want, "alpha_fn filter")
