"""nerf_amd.OccGridRenderer: estimator -> packed points -> field -> packed compositing -> grid update.

The field is analytic: density 20 inside the ball of radius 0.5, a smooth colour of position plus a
two-layer head (so there are parameters).  Scene: the 64 rays of tests/_occgrid_ref.py::
checkerboard_case, grids over [-1, 1]^3, dt = 1/64, near / far 0.05 / 6.  Bars: the compositing bars,
2e-6 for outputs and 2e-5 + 1e-5 rel for gradients (tests/test_gpu_composite_packed.py).  Measured
distances are printed.
"""
import copy

import numpy as np
import pytest
import torch
from torch import nn

import _occgrid_ref as R
import _packed_train_ref as P

pytestmark = pytest.mark.gpu

DEV = "cuda"
AABB = [-1.0, -1.0, -1.0, 1.0, 1.0, 1.0]
NEAR, FAR, DT = 0.05, 6.0, 1.0 / 64
RADIUS = 0.5


class BallField(nn.Module):
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
        density = 20.0 * (pos.detach().float().norm(dim=-1) < RADIUS).to(pos.dtype)
        head = self.l2(torch.tanh(self.l1(torch.cat([pos, dirs], dim=-1))))
        return torch.sigmoid(torch.sin(3.0 * pos) + head), density


@pytest.fixture(scope="module", autouse=True)
def _lib():
    import nerf_amd
    nerf_amd._lib.load()  # fail loudly if the HIP library is missing
    yield


@pytest.fixture(scope="module")
def rays():
    o, d = R.checkerboard_case()[:2]
    return torch.from_numpy(o), torch.from_numpy(d)


def estimator(res, binaries=None):
    import nerf_amd
    est = nerf_amd.OccGridEstimator(AABB, resolution=res).to(DEV)
    if binaries is not None:
        est.binaries.copy_(binaries.view_as(est.binaries))
    return est


def superset_cells(res):
    """Every cell whose centre lies within a cell diagonal of the ball: a superset of the cells the
    ball touches (a point is within half a diagonal of its cell's centre)."""
    c = (torch.arange(res, dtype=torch.float64) + 0.5) / res * 2 - 1
    dist = (c[:, None, None] ** 2 + c[None, :, None] ** 2 + c[None, None, :] ** 2).sqrt()
    return dist < RADIUS + (2.0 / res) * 3 ** 0.5


def renderer(field, est, **kw):
    import nerf_amd
    return nerf_amd.OccGridRenderer(field, est, NEAR, FAR, DT, **kw).to(DEV)


def within(got, ref, what, grad=False, atol=2e-6):
    atol, rtol = (2e-5, 1e-5) if grad else (atol, 0.0)
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    err = (got - ref).abs()
    print(f"{what}: max |err| = {float(err.max()) if err.numel() else 0.0:.3e} (largest value {float(ref.abs().max()):.3f})")
    assert torch.all(err <= atol + rtol * ref.abs()), what


def test_superset_grid_against_full_grid(rays):
    """Samples outside the ball have density exactly 0 and change nothing: a grid that covers the ball
    renders what the full grid renders, from strictly fewer samples (visibility filter on: the
    defaults)."""
    o, d = rays[0].to(DEV), rays[1].to(DEV)
    g = torch.Generator().manual_seed(4)
    g_c, g_o, g_d = (torch.randn(64, k, generator=g).to(DEV) for k in (3, 1, 1))
    bkgd = torch.tensor([0.1, 0.6, 0.3])
    outs = []
    for cells in (torch.ones(16, 16, 16, dtype=torch.bool), superset_cells(16)):
        field = BallField().to(DEV)
        ren = renderer(field, estimator(16, cells), render_bkgd=bkgd)
        assert ren.render_bkgd.device.type == "cuda"
        rgb, op, dep, ex = ren(o, d, stratified=False)
        assert rgb.shape == (64, 3) and op.shape == (64, 1) and dep.shape == (64, 1)
        assert set(ex) == {"weights", "trans", "sigmas", "rgbs", "alphas", "ray_indices", "t_starts", "t_ends"}
        assert len(field.calls) == 2                    # the filter's density pass, then the field proper
        ((rgb * g_c).sum() + (op * g_o).sum() + (dep * g_d).sum()).backward()
        outs.append((rgb, op, dep, [p.grad for p in field.parameters()], ex))
    full, sup = outs
    assert 0 < sup[4]["ray_indices"].numel() < full[4]["ray_indices"].numel()
    assert float(full[1].detach().max()) > 0.99 and float(full[1].detach().min()) == 0.0     # rays through and past the ball
    for name, a, b in zip(("rgb", "opacity", "depth"), sup, full):
        within(a, b, name)
    for i, (a, b) in enumerate(zip(sup[3], full[3])):
        assert float(b.abs().max()) > 0
        within(a, b, f"parameter gradient {i}", grad=True)


def test_filter_runs_only_when_asked(rays):
    o, d = rays[0].to(DEV), rays[1].to(DEV)
    field = BallField().to(DEV)
    ren = renderer(field, estimator(16, superset_cells(16)), early_stop_eps=0.0)
    _, _, _, ex = ren(o, d, stratified=False)
    assert len(field.calls) == 1
    ri, t0, t1, _, _ = R.march_ref(rays[0].numpy(), rays[1].numpy(), AABB, (16,) * 3, superset_cells(16).numpy(), NEAR,
                                   FAR, DT)
    assert np.array_equal(ex["ray_indices"].cpu().numpy(), ri) and np.array_equal(ex["t_starts"].cpu().numpy(), t0)
    # the field saw bitwise the marched midpoints
    pos, _ = P.points_ref32(rays[0].numpy(), rays[1].numpy(), ri, t0, t1)
    assert torch.equal(field.calls[0].cpu().view(torch.int32), torch.from_numpy(pos).view(torch.int32))
    # stratified defaults to self.training
    a = ren(o, d)[3]["t_starts"]
    ren.eval()
    b, c = ren(o, d)[3]["t_starts"], ren(o, d)[3]["t_starts"]
    assert torch.equal(b, c) and torch.equal(b, ex["t_starts"])
    assert a.shape != b.shape or not torch.equal(a, b)
    ren2 = renderer(field, estimator(16, superset_cells(16)), early_stop_eps=0.0, alpha_thre=1e-3)
    n = len(field.calls)
    kept = ren2(o, d, stratified=False)[3]
    assert len(field.calls) == n + 2 and 0 < kept["ray_indices"].numel() < ri.size
    assert float(kept["alphas"].min()) >= 1e-3


def test_ray_gradients_and_distortion_loss(rays):
    """Gradients to rays_o / rays_d (the pose gradient) against the fp64 torch-indexing restatement of
    the same samples, bitwise equal across two runs; distortion_loss(extras) against the direct sum."""
    g = torch.Generator().manual_seed(6)
    g_c, g_o, g_d = (torch.randn(64, k, generator=g) for k in (3, 1, 1))
    bkgd = torch.tensor([0.1, 0.6, 0.3])
    field = BallField()
    runs = []
    for _ in range(2):
        f = copy.deepcopy(field).to(DEV)
        ren = renderer(f, estimator(16, superset_cells(16)), early_stop_eps=0.0, render_bkgd=bkgd)
        o, d = rays[0].to(DEV).requires_grad_(True), rays[1].to(DEV).requires_grad_(True)
        rgb, op, dep, ex = ren(o, d, stratified=False)
        dist = ren.distortion_loss(ex)
        ((rgb * g_c.to(DEV)).sum() + (op * g_o.to(DEV)).sum() + (dep * g_d.to(DEV)).sum() + 3.0 * dist).backward()
        runs.append((o.grad, d.grad, rgb, op, dep, ex, dist, [p.grad for p in f.parameters()]))
    assert torch.equal(runs[0][0].view(torch.int32), runs[1][0].view(torch.int32))
    assert torch.equal(runs[0][1].view(torch.int32), runs[1][1].view(torch.int32))
    o_grad, d_grad, rgb, op, dep, ex, dist, p_grads = runs[0]
    ri, t0, t1 = (ex[k].cpu() for k in ("ray_indices", "t_starts", "t_ends"))
    f64 = copy.deepcopy(field).double()
    o64, d64 = rays[0].double().requires_grad_(True), rays[1].double().requires_grad_(True)
    r_rgb, r_op, r_dep, r_w = P.render_ref64(f64, o64, d64, ri, t0, t1, bkgd)
    seg = torch.searchsorted(ri, torch.arange(65))
    # the loss of the restatement's own fp64 weights, differentiated through them
    w, m, delta = r_w, ((t0 + t1) * 0.5).double(), t1.double() - t0.double()
    r_dist = torch.stack([(w[a:b, None] * w[None, a:b] * (m[a:b, None] - m[None, a:b]).abs()).sum()
                          + (w[a:b] ** 2 * delta[a:b]).sum() / 3 for a, b in zip(seg[:-1].tolist(), seg[1:].tolist())])
    ((r_rgb * g_c).sum() + (r_op * g_o).sum() + (r_dep * g_d).sum() + 3.0 * r_dist.mean()).backward()
    within(op, r_op, "opacity")
    within(dep, r_dep, "depth", atol=2e-6 * FAR)             # the depth bar of test_gpu_composite_packed.py
    within(dist, r_dist.mean(), "distortion loss")
    direct, _ = P.distortion_direct64(ex["weights"].detach().cpu(), t0, t1, seg)
    within(dist, direct.mean(), "distortion loss of the device's weights")
    assert float(direct.mean()) > 1e-4
    assert float(o64.grad.abs().max()) > 1e-3 and float(d64.grad.abs().max()) > 1e-3
    within(o_grad, o64.grad, "rays_o.grad", grad=True)
    within(d_grad, d64.grad, "rays_d.grad", grad=True)
    for i, (a, b) in enumerate(zip(p_grads, f64.parameters())):
        within(a, b.grad, f"parameter gradient {i}", grad=True)


def test_update_grid_and_the_next_forward(rays):
    o, d = rays[0].to(DEV), rays[1].to(DEV)
    field = BallField().to(DEV)
    est = estimator(8)
    ren = renderer(field, est, early_stop_eps=0.0)
    _, _, _, ex = ren(o, d, stratified=False)
    assert ex["ray_indices"].numel() == 0 and not field.calls       # nothing set yet
    ren.update_grid(1, n=16)
    assert not field.calls and not bool(est.binaries.any())
    torch.manual_seed(123)
    ren.update_grid(0, n=16)
    assert len(field.calls) == 1 and field.calls[0].shape == (512, 3)
    # the same occ_eval_fn replayed under the same seed
    torch.manual_seed(123)
    idx = torch.arange(512, device=DEV)
    coords = torch.stack([idx // 64, (idx // 8) % 8, idx % 8], dim=-1).float()
    x = (coords + torch.rand_like(coords)) / torch.tensor([8, 8, 8], device=DEV, dtype=torch.float32)
    pts = torch.tensor(AABB[:3], device=DEV) + x * (torch.tensor(AABB[3:], device=DEV) - torch.tensor(AABB[:3], device=DEV))
    assert torch.equal(pts, field.calls[0])
    n_calls = len(field.calls)
    occ = field(pts, torch.tensor([0.0, 0.0, 1.0], device=DEV).expand(512, 3))[1] * DT
    del field.calls[n_calls:]
    expect = pts.norm(dim=-1) < RADIUS
    assert torch.equal(occ > 0.01, expect) and 0 < int(expect.sum()) < 512
    assert torch.equal(est.binaries.reshape(-1), expect)
    _, op, _, ex = ren(o, d, stratified=False)
    ri, t0, t1, _, _ = R.march_ref(rays[0].numpy(), rays[1].numpy(), AABB, (8,) * 3, expect.cpu().numpy(), NEAR, FAR, DT)
    assert ri.size > 0 and np.array_equal(ex["ray_indices"].cpu().numpy(), ri)
    assert np.array_equal(ex["t_starts"].cpu().numpy(), t0) and np.array_equal(ex["t_ends"].cpu().numpy(), t1)
    assert float(op.detach().max()) > 0.5


def test_all_empty_grid_gives_background_without_calling_the_field(rays):
    o, d = rays[0].to(DEV).requires_grad_(True), rays[1].to(DEV)
    field = BallField().to(DEV)
    bkgd = torch.tensor([0.2, 0.5, 0.9])
    for kw in ({}, {"early_stop_eps": 0.0}):
        ren = renderer(field, estimator(8), render_bkgd=bkgd, **kw)
        rgb, op, dep, ex = ren(o, d)
        assert not field.calls
        assert torch.equal(rgb, bkgd.to(DEV).expand(64, 3)) and not rgb.requires_grad
        assert torch.all(op == 0) and torch.all(dep == 0) and op.shape == (64, 1) and dep.shape == (64, 1)
        assert ex["weights"].shape == (0,) and ex["rgbs"].shape == (0, 3) and ex["ray_indices"].dtype == torch.int64
        assert float(ren.distortion_loss(ex)) == 0.0
    rgb = renderer(field, estimator(8))(o, d)[0]
    assert torch.all(rgb == 0)
