"""Cascaded occupancy-grid marching (csrc/occgrid_cascade.hip: nerf_occ_cascade_count /
nerf_occ_cascade_write), nerf_amd.CascadedOccGridEstimator.sampling and OccGridRenderer(cone_angle=...)
against the numpy fp32 restatement of the cascaded marching contract, tests/_occgrid_cascade_ref.py::
march_cascade_ref: ray_indices, t_starts, t_ends and status bit for bit, no case left out.  The C-ABI
calls write into buffers guarded by a NaN pattern (tests/_guarded.py): no store may land outside the
N samples the counts name.
"""
import numpy as np
import pytest
import torch
from torch import nn

import _occgrid_cascade_ref as C
import _occgrid_ref as R
from _guarded import GUARD, SENTINEL, Guarded

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def _lib():
    import nerf_amd
    nerf_amd._lib.load()  # fail loudly if the HIP library is missing
    yield


def estimator(roi, res, binaries):
    """The estimator over region of interest roi with binaries [levels, rx, ry, rz]."""
    from nerf_amd import CascadedOccGridEstimator
    binaries = np.asarray(binaries)
    est = CascadedOccGridEstimator(roi, resolution=list(res), levels=binaries.shape[0]).to(DEV)
    est.binaries.copy_(torch.from_numpy(binaries))
    assert est.aabbs.device.type == "cuda"
    return est


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype=F32)).to(DEV)


def march_guarded(est, o, d, near, far, dt, cone=0.0, t_lo=None, t_hi=None, stratified=False, seed=0,
                  mask_words=None):
    """Both passes through the C calls with guarded outputs: (ray_indices, t_starts, t_ends, status,
    counts) on the host."""
    import nerf_amd
    from nerf_amd import kernels as K
    lib = nerf_amd._lib.load()
    o, d = dev(o), dev(d)
    n = o.shape[0]
    words = mask_words or K.occ_mask_words(near, far, dt)
    nbytes = K.occ_march_workspace_bytes(n, words)
    ws = Guarded((nbytes + 3) // 4, dtype=torch.int32)
    # the guard sits 4096 bytes into a torch allocation: the body is 256-byte aligned
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    counts = K.occ_cascade_count(o, d, est.aabbs.tolist(), est.resolution, est.grid_bits(), near, far, dt, cone,
                                 stratified, seed, words, ws.body, status, dev(t_lo), dev(t_hi))
    offsets = torch.cumsum(counts, 0)
    total = int(offsets[-1]) if n else 0
    ri, t0, t1 = Guarded(total, dtype=torch.int64), Guarded(total), Guarded(total)
    st = lib.nerf_occ_cascade_write(n, dt, cone, words, ws.ptr(), nbytes, offsets.data_ptr() if n else None, total,
                                    ri.ptr(), t0.ptr(), t1.ptr(), torch.cuda.current_stream().cuda_stream)
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


def host(out):
    return tuple(x.cpu().numpy() for x in out) + (0,)


ROI = [-0.5, -0.5, -0.5, 0.5, 0.5, 0.5]
_REFS = {}


def cascade_with_misses():
    o, d, aabbs, res, binaries, near, far, dt = C.cascade_case()
    o, d = np.concatenate([o, C.MISSING_RAYS[0]]), np.concatenate([d, C.MISSING_RAYS[1]])
    return o, d, aabbs, res, binaries, near, far, dt


def cascade_ref(cone):
    """The restatement on the cascade case plus the four missing rays, computed once per cone."""
    if cone not in _REFS:
        _REFS[cone] = C.march_cascade_ref(*cascade_with_misses(), cone=cone)
    return _REFS[cone]


@pytest.mark.parametrize("cone", [0.0, 0.01])
def test_cascade_case(cone):
    o, d, aabbs, res, binaries, near, far, dt = cascade_with_misses()
    est = estimator(ROI, res, binaries)
    assert np.array_equal(est.aabbs.cpu().numpy(), aabbs)
    ref = cascade_ref(cone)
    assert ref[0].size == (6634 if cone else 9515) and ref[0].max() == 63
    got = march_guarded(est, o, d, near, far, dt, cone)
    same(got, ref, f"cascade, cone {cone}")
    assert list(got[4][64:]) == [0, 0, 0, 0]
    # the estimator's own call returns the same bits
    out = est.sampling(dev(o), dev(d), near_plane=near, far_plane=far, render_step_size=dt, cone_angle=cone)
    assert out[0].dtype == torch.int64 and out[1].dtype == torch.float32
    same(host(out), ref, "sampling")
    assert int(est.status().item()) == 0


@pytest.mark.parametrize("cone", [0.0, 0.01])
@pytest.mark.parametrize("n_rays", [0, 1])
def test_few_rays(n_rays, cone):
    o, d, aabbs, res, binaries, near, far, dt = C.cascade_case()
    est = estimator(ROI, res, binaries)
    o, d = o[5:5 + n_rays], d[5:5 + n_rays]
    ref = C.march_cascade_ref(o, d, aabbs, res, binaries, near, far, dt, cone)
    assert n_rays == 0 or ref[0].size > 0
    same(march_guarded(est, o, d, near, far, dt, cone), ref, f"{n_rays} rays")
    out = est.sampling(dev(o).reshape(-1, 3), dev(d).reshape(-1, 3), near_plane=near, far_plane=far,
                       render_step_size=dt, cone_angle=cone)
    same(host(out), ref, f"sampling, {n_rays} rays")


def test_cone_count_construction():
    """All sixteen (m, t_max) of the recurrence's count construction in one call, t_max per ray:
    exactly m samples each, abutting bitwise, the last ending at its t_max."""
    o, d, aabbs, res, binaries, near, far, dt, cone = C.cone_count_case()
    chain, bounds = C.cone_count_bounds()
    t_hi = np.array([b[1] for b in bounds], dtype=F32)
    o, d = np.repeat(o, len(bounds), 0), np.repeat(d, len(bounds), 0)
    est = estimator(aabbs[0].tolist(), res, binaries)
    ref = C.march_cascade_ref(o, d, aabbs, res, binaries, near, far, dt, cone, t_hi=t_hi)
    got = march_guarded(est, o, d, near, far, dt, cone, t_hi=t_hi)
    same(got, ref, "cone count construction")
    assert list(got[4]) == [b[0] for b in bounds]
    ri, t0, t1 = got[:3]
    inner = ri[:-1] == ri[1:]
    assert np.array_equal(t1[:-1][inner].view(np.uint32), t0[1:][inner].view(np.uint32))
    last = np.append(~inner, True)
    assert np.array_equal(t1[last].view(np.uint32), t_hi.view(np.uint32))
    # the unbounded ray: 404 steps from 1 to 5
    got = march_guarded(est, o[:1], d[:1], near, far, dt, cone)
    assert got[0].size == 404 and got[1][0] == 1.0 and got[2][-1] == 5.0
    assert np.array_equal(got[1].view(np.uint32), chain[:-1].view(np.uint32))


def test_one_level_is_the_one_level_kernel():
    """levels 1, cone 0, no ray bounds: the outputs and counts of nerf_occ_march_count / _write."""
    from nerf_amd import OccGridEstimator
    o, d, aabb, res, binaries, near, far, dt = R.checkerboard_case()
    est = estimator(aabb, res, binaries[None])
    got = march_guarded(est, o, d, near, far, dt)
    old = OccGridEstimator(aabb, resolution=list(res)).to(DEV)
    old.binaries.copy_(torch.from_numpy(binaries).reshape(old.binaries.shape))
    want = old.sampling(dev(o), dev(d), near_plane=near, far_plane=far, render_step_size=dt)
    assert want[0].numel() == 4092
    same(got, host(want), "one level against the one-level kernels")
    torch.manual_seed(5)
    want = old.sampling(dev(o), dev(d), near_plane=near, far_plane=far, render_step_size=dt, stratified=True)
    torch.manual_seed(5)
    out = est.sampling(dev(o), dev(d), near_plane=near, far_plane=far, render_step_size=dt, stratified=True)
    same(host(out), host(want), "one level, stratified")


@pytest.mark.parametrize("cone", [0.0, 0.01])
def test_ray_bounds(cone):
    """Seeded t_min / t_max per ray, inside and outside [near, far], a quarter of the rays with
    t_min > t_max; one of them absent in turn."""
    o, d, aabbs, res, binaries, near, far, dt = C.cascade_case()
    rng = np.random.default_rng(99)
    t_lo = rng.uniform(-1.0, 4.0, size=64).astype(F32)
    t_hi = (t_lo + rng.uniform(0.1, 4.0, size=64)).astype(F32)        # up to 8 > far
    t_lo[::4], t_hi[::4] = t_hi[::4].copy(), t_lo[::4].copy()
    assert (t_lo < near).any() and (t_hi > far).any() and (t_lo > t_hi).sum() == 16
    est = estimator(ROI, res, binaries)
    plain = C.march_cascade_ref(o, d, aabbs, res, binaries, near, far, dt, cone)
    for lo, hi in ((t_lo, t_hi), (t_lo, None), (None, t_hi)):
        ref = C.march_cascade_ref(o, d, aabbs, res, binaries, near, far, dt, cone, t_lo=lo, t_hi=hi)
        assert 0 < ref[0].size < plain[0].size
        same(march_guarded(est, o, d, near, far, dt, cone, t_lo=lo, t_hi=hi), ref, f"ray bounds, cone {cone}")
    ref = C.march_cascade_ref(o, d, aabbs, res, binaries, near, far, dt, cone, t_lo=t_lo, t_hi=t_hi)
    assert np.all(np.bincount(ref[0], minlength=64)[::4] == 0)
    out = est.sampling(dev(o), dev(d), near_plane=near, far_plane=far, render_step_size=dt, cone_angle=cone,
                       t_min=dev(t_lo), t_max=dev(t_hi))
    same(host(out), ref, "sampling with ray bounds")


def test_recurrence_reaches_the_step_limit():
    """A chain of more than NERF_OCC_MAX_STEPS steps: status bit 0 and exactly 8192 samples (the grid is
    full), next to a ray that stays below the limit; cut at a smaller mask capacity: bit 1."""
    o, _, aabbs, res, binaries, near, far, _, _ = C.cone_count_case()
    o = np.repeat(o, 2, 0)
    d = np.array([[1e-4, 0.0, 0.0], [1e-2, 0.0, 0.0]], dtype=F32)
    est = estimator(aabbs[0].tolist(), res, binaries)
    ref = C.march_cascade_ref(o, d, aabbs, res, binaries, near, far, 1.0, 1e-6)
    assert ref[3] == 1 and list(ref[4]["considered"]) == [C.MAX_STEPS, 400]
    got = march_guarded(est, o, d, near, far, 1.0, 1e-6)
    same(got, ref, "step limit")
    assert got[3] == 1 and list(got[4]) == [C.MAX_STEPS, 400]
    ref = C.march_cascade_ref(o, d, aabbs, res, binaries, near, far, 1.0, 1e-6, mask_words=3)
    got = march_guarded(est, o, d, near, far, 1.0, 1e-6, mask_words=3)
    same(got, ref, "mask capacity")
    assert got[3] == 2 and list(got[4]) == [192, 192]


def test_stratified_with_a_fixed_seed():
    from nerf_amd.model_interpolation import _rng_seed
    o, d, aabbs, res, binaries, near, far, dt = C.cascade_case()
    est = estimator(ROI, res, binaries)
    torch.manual_seed(77)
    seed = _rng_seed()
    ref = C.march_cascade_ref(o, d, aabbs, res, binaries, near, far, dt, 0.01, stratified=True, seed=seed)
    assert not np.array_equal(ref[1][:8], cascade_ref(0.01)[1][:8])
    same(march_guarded(est, o, d, near, far, dt, 0.01, stratified=True, seed=seed), ref, "stratified")
    torch.manual_seed(77)                                   # sampling draws the same seed itself
    out = est.sampling(dev(o), dev(d), near_plane=near, far_plane=far, render_step_size=dt, stratified=True,
                       cone_angle=0.01)
    same(host(out), ref, "stratified sampling")


class BallField(nn.Module):
    """The analytic field of tests/test_gpu_occ_render.py: density 20 inside the ball of radius 0.5, a
    smooth colour of position plus a two-layer head."""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(0)
        self.l1, self.l2 = nn.Linear(6, 16), nn.Linear(16, 3)
        with torch.no_grad():
            for p in self.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * 0.5)
        self.calls = []

    def forward(self, pos, dirs):
        self.calls.append(pos.detach())
        density = 20.0 * (pos.detach().float().norm(dim=-1) < 0.5).to(pos.dtype)
        head = self.l2(torch.tanh(self.l1(torch.cat([pos, dirs], dim=-1))))
        return torch.sigmoid(torch.sin(3.0 * pos) + head), density


def test_renderer_with_cone_angle():
    """OccGridRenderer(cone_angle=0.01) over three full levels of 16^3 around [-1, 1]^3: the samples are
    the restatement's, the field sees bitwise their midpoints, rgb is `rendering` on the same samples,
    and the backward reaches the field's parameters."""
    import nerf_amd
    o, d, _, _, _, near, far, dt = R.checkerboard_case()
    roi, res = [-1.0, -1.0, -1.0, 1.0, 1.0, 1.0], (16, 16, 16)
    binaries = np.ones((3, 16, 16, 16), dtype=bool)
    est = estimator(roi, res, binaries)
    field = BallField().to(DEV)
    bkgd = torch.tensor([0.1, 0.6, 0.3])
    ren = nerf_amd.OccGridRenderer(field, est, near, far, dt, early_stop_eps=0.0, render_bkgd=bkgd,
                                   cone_angle=0.01).to(DEV)
    od = dev(o), dev(d)
    rgb, op, dep, ex = ren(*od, stratified=False)
    ref = C.march_cascade_ref(o, d, C.cascade_aabbs(roi, 3), res, binaries, near, far, dt, 0.01)
    assert ref[4]["cone_step"].any() and not ref[4]["cone_step"].all() and set(ref[4]["level"]) == {0, 1, 2}
    same(host((ex["ray_indices"], ex["t_starts"], ex["t_ends"])), ref, "renderer samples")
    assert len(field.calls) == 1
    pos = C.points_ref(o, d, *ref[:3])
    assert torch.equal(field.calls[0].cpu().view(torch.int32), torch.from_numpy(pos).view(torch.int32))
    pts = nerf_amd.packed_points(*od, ex["ray_indices"], ex["t_starts"], ex["t_ends"], 64)[0]
    assert torch.equal(pts.cpu().view(torch.int32), torch.from_numpy(pos).view(torch.int32))

    def rgb_sigma_fn(ts, te, idx):
        p, dirs = nerf_amd.packed_points(*od, idx, ts, te, 64)
        c, sigma = field(p, dirs)
        return c, sigma.reshape(-1)
    want = nerf_amd.rendering(ex["t_starts"], ex["t_ends"], ex["ray_indices"], 64, rgb_sigma_fn, bkgd.to(DEV))
    assert torch.equal(rgb, want[0]) and torch.equal(op, want[1]) and torch.equal(dep, want[2])
    assert float(op.detach().max()) > 0.99 and float(op.detach().min()) == 0.0
    rgb.sum().backward()
    grads = [p.grad for p in field.parameters()]
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads) and float(grads[0].abs().max()) > 0
    # with the visibility filter (the defaults) strictly fewer samples, the same picture within the bars
    ren2 = nerf_amd.OccGridRenderer(field, est, near, far, dt, render_bkgd=bkgd, cone_angle=0.01).to(DEV)
    rgb2, _, _, ex2 = ren2(*od, stratified=False)
    assert 0 < ex2["ray_indices"].numel() < ref[0].size
    assert float((rgb2 - rgb).detach().abs().max()) <= 1e-4 + 2e-6     # early_stop_eps = 1e-4 of transmittance left out
    # a one-level estimator behind the same renderer class is called without cone_angle, as before
    one = nerf_amd.OccGridEstimator(roi, resolution=16).to(DEV)
    one.binaries.fill_(True)
    plain = nerf_amd.OccGridRenderer(field, one, near, far, dt, early_stop_eps=0.0).to(DEV)
    ref1 = R.march_ref(o, d, roi, res, binaries[0], near, far, dt)
    ex1 = plain(*od, stratified=False)[3]
    same(host((ex1["ray_indices"], ex1["t_starts"], ex1["t_ends"])), ref1[:4], "one-level renderer")
