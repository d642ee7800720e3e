"""Sample points of packed samples (csrc/packed_points.hip: nerf_packed_points_fwd / _bwd) and
nerf_amd.packed_points against tests/_packed_train_ref.py.

Forward: bitwise against the numpy fp32 restatement of the points contract (each operation rounded
alone) on the marching restatement's output, so the points are the midpoints whose cells the marching
tested.  Backward: the fp64 segment sums of the restatement within the project's gradient bar
(2e-5 + 1e-5 rel); the kernel sums in fp64 and rounds once, so the measured distance is half an ulp of
the result (printed; on the MI355X 1.8e-6 on g_o up to 55 and 6.6e-6 on g_d up to 224, against
bars of 5.7e-4 and 2.3e-3 there), and two runs give the same bits.  Every
output is written into a buffer guarded by a NaN pattern (tests/_guarded.py); positions and dirs
with a row stride of 4, whose pad column must keep the pattern.
"""
import numpy as np
import pytest
import torch

import _occgrid_ref as R
import _packed_train_ref as P
from _guarded import Guarded, SENTINEL

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _lib():
    import nerf_amd
    nerf_amd._lib.load()  # fail loudly if the HIP library is missing
    yield


def stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def lib():
    import nerf_amd
    return nerf_amd._lib.load()


def _marched(o, d, aabb, res, binaries, near, far, dt):
    ri, t0, t1, _, _ = R.march_ref(o, d, aabb, res, binaries, near, far, dt)
    return o, d, ri, t0, t1


@pytest.fixture(scope="module")
def cases():
    """(rays_o, rays_d, ray_indices, t_starts, t_ends) of the marching restatement, computed once."""
    out = {"checkerboard": _marched(*R.checkerboard_case())}
    for m in R.COUNT_M:
        out[f"count{m}"] = _marched(*R.count_construction(m))
    return out


def forward_guarded(o, d, ri, t0, t1, want_dirs=True, n_rays=None, n_samples=None):
    """The raw entry point into stride-4 guarded rows; returns (positions, dirs) Guarded and the status."""
    N = ri.numel() if n_samples is None else n_samples
    cols = (torch.arange(4 * ri.numel()) % 4) < 3
    pos, dirs = Guarded(4 * ri.numel(), named=cols), Guarded(4 * ri.numel(), named=cols)
    st = lib().nerf_packed_points_fwd(o.data_ptr(), d.data_ptr(), o.shape[0] if n_rays is None else n_rays,
                                      ri.data_ptr(), t0.data_ptr(), t1.data_ptr(), N, pos.ptr(), 4,
                                      dirs.ptr() if want_dirs else None, 4, stream())
    return pos, dirs, st


def bits(x):
    return torch.as_tensor(np.ascontiguousarray(x)).view(torch.int32)


def test_forward_is_bitwise_the_marched_midpoints(cases):
    for name, (o, d, ri, t0, t1) in cases.items():
        assert ri.size > 0, name
        ref_p, ref_d = P.points_ref32(o, d, ri, t0, t1)
        dev = [torch.from_numpy(x).to(DEV) for x in (o, d, ri, t0, t1)]
        pos, dirs, st = forward_guarded(*dev)
        assert st == 0
        pos.check(f"{name} positions")
        dirs.check(f"{name} dirs")
        got_p = pos.body.view(-1, 4)[:, :3].cpu().contiguous().view(torch.int32)
        got_d = dirs.body.view(-1, 4)[:, :3].cpu().contiguous().view(torch.int32)
        assert torch.equal(got_p, bits(ref_p)), name
        assert torch.equal(got_d, bits(ref_d)), name
        pos2, dirs2, st = forward_guarded(*dev, want_dirs=False)
        assert st == 0
        dirs2.check(f"{name} dirs skipped", written=False)
        assert torch.equal(pos2.body.view(torch.int32), pos.body.view(torch.int32))


def test_out_of_range_index_gives_a_nan_row(cases):
    o, d, ri, t0, t1 = cases["checkerboard"]
    ri = ri.copy()
    k, k2 = ri.size // 2, ri.size - 1
    ri[k], ri[k2] = o.shape[0], -1
    ref_p, ref_d = P.points_ref32(o, d, ri, t0, t1)
    assert np.isnan(ref_p[k]).all() and np.isnan(ref_p[k2]).all() and np.isnan(ref_p).sum() == 6
    pos, dirs, st = forward_guarded(*[torch.from_numpy(x).to(DEV) for x in (o, d, ri, t0, t1)])
    assert st == 0
    pos.check("positions")
    dirs.check("dirs")
    for buf, ref in ((pos, ref_p), (dirs, ref_d)):
        got = buf.body.view(-1, 4)[:, :3].cpu()
        assert torch.isnan(got[k]).all() and torch.isnan(got[k2]).all()
        assert torch.all(got[k].view(torch.int32) != SENTINEL)
        rest = np.ones(ri.size, dtype=bool)
        rest[[k, k2]] = False
        assert torch.equal(got[torch.from_numpy(rest)].contiguous().view(torch.int32), bits(ref[rest]))


def test_zero_rays_and_zero_samples_launch_nothing(cases):
    from nerf_amd import packed_points
    o, d, ri, t0, t1 = [torch.from_numpy(x).to(DEV) for x in cases["count2"]]
    for kw in ({"n_rays": 0}, {"n_samples": 0}):
        pos, dirs, st = forward_guarded(o, d, ri, t0, t1, **kw)
        torch.cuda.synchronize()
        assert st == 0
        pos.check("positions", written=False)
        dirs.check("dirs", written=False)
    g = Guarded(3)
    st = lib().nerf_packed_points_bwd(None, 1, None, None, 0, None, 3, None, 3, g.ptr(), g.ptr(), stream())
    assert st == 0
    g.check("g_o", written=False)
    # the public function: empty outputs, and zero gradients for rays without samples
    e = torch.zeros(0, device=DEV)
    oo = o.clone().requires_grad_(True)
    p, dd = packed_points(oo, d, torch.zeros(0, dtype=torch.int64, device=DEV), e, e)
    assert p.shape == (0, 3) and dd.shape == (0, 3)
    (p.sum() + dd.sum()).backward()
    assert torch.all(oo.grad == 0) and oo.grad.shape == o.shape
    none_o = torch.zeros(0, 3, device=DEV)
    p, _ = packed_points(none_o, none_o, ri, t0, t1)      # no rays: every index is out of range
    assert torch.isnan(p).all()


@pytest.fixture(scope="module")
def bwd_case():
    g = torch.Generator().manual_seed(31)
    N = sum(P.LENGTHS)
    t0 = torch.rand(N, generator=g) * 5
    t1 = t0 + torch.rand(N, generator=g) * 0.1 + 1e-3
    g_pos, g_dirs = torch.randn(N, 3, generator=g), torch.randn(N, 3, generator=g)
    seg = R.segments_of(P.LENGTHS)
    ref = {True: P.points_bwd_ref64(seg.numpy(), t0.numpy(), t1.numpy(), g_pos.numpy(), g_dirs.numpy()),
           False: P.points_bwd_ref64(seg.numpy(), t0.numpy(), t1.numpy(), g_pos.numpy())}
    return seg, t0, t1, g_pos, g_dirs, ref


def close_grad(got, ref, what):
    got = got.detach().cpu().double().numpy()
    err = np.abs(got - ref)
    print(f"{what}: max |err| = {err.max():.3e} (largest value {np.abs(ref).max():.3f})")
    np.testing.assert_allclose(got, ref, atol=2e-5, rtol=1e-5, err_msg=what)


@pytest.mark.parametrize("with_dirs", [True, False])
def test_backward_on_ragged_segments(bwd_case, with_dirs):
    seg, t0, t1, g_pos, g_dirs, ref = bwd_case
    Rn, N = len(P.LENGTHS), t0.numel()
    d = [x.to(DEV) for x in (seg, t0, t1, g_pos, g_dirs)]
    runs = []
    for _ in range(2):
        g_o, g_d = Guarded(3 * Rn), Guarded(3 * Rn)
        st = lib().nerf_packed_points_bwd(d[0].data_ptr(), Rn, d[1].data_ptr(), d[2].data_ptr(), N, d[3].data_ptr(), 3,
                                          d[4].data_ptr() if with_dirs else None, 3, g_o.ptr(), g_d.ptr(), stream())
        assert st == 0
        g_o.check("g_o")
        g_d.check("g_d")
        runs.append((g_o.body.view(Rn, 3).clone(), g_d.body.view(Rn, 3).clone()))
    close_grad(runs[0][0], ref[with_dirs][0], "g_o")
    close_grad(runs[0][1], ref[with_dirs][1], "g_d")
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))       # the same bits twice
    empty = [i for i, L in enumerate(P.LENGTHS) if L == 0]
    assert torch.all(runs[0][0][empty].view(torch.int32) == 0) and torch.all(runs[0][1][empty].view(torch.int32) == 0)


def test_public_function_forward_and_gradients(cases, bwd_case):
    """nerf_amd.packed_points: the raw kernel's bits, None for want_dirs=False, and one autograd node
    whose gradients to rays_o / rays_d are the restatement's (positions alone, and positions + dirs)."""
    from nerf_amd import packed_points
    o, d, ri, t0, t1 = cases["checkerboard"]
    ref_p, ref_d = P.points_ref32(o, d, ri, t0, t1)
    dev = [torch.from_numpy(x).to(DEV) for x in (o, d, ri, t0, t1)]
    g = torch.Generator().manual_seed(9)
    g_pos, g_dirs = torch.randn(ri.size, 3, generator=g), torch.randn(ri.size, 3, generator=g)
    seg = np.searchsorted(ri, np.arange(o.shape[0] + 1))
    for want_dirs in (True, False):
        oo, dd = dev[0].clone().requires_grad_(True), dev[1].clone().requires_grad_(True)
        pos, dirs = packed_points(oo, dd, *dev[2:], n_rays=o.shape[0], want_dirs=want_dirs)
        assert torch.equal(pos.detach().cpu().view(torch.int32), bits(ref_p))
        assert pos.grad_fn is not None
        loss = (pos * g_pos.to(DEV)).sum()
        if want_dirs:
            assert torch.equal(dirs.detach().cpu().view(torch.int32), bits(ref_d)) and dirs.grad_fn is pos.grad_fn
            loss = loss + (dirs * g_dirs.to(DEV)).sum()
        else:
            assert dirs is None
        loss.backward()
        r_o, r_d = P.points_bwd_ref64(seg, t0, t1, g_pos.numpy(), g_dirs.numpy() if want_dirs else None)
        close_grad(oo.grad, r_o, "rays_o.grad")
        close_grad(dd.grad, r_d, "rays_d.grad")
    # only rays_d requires grad, only dirs is used: g_positions is absent
    dd = dev[1].clone().requires_grad_(True)
    _, dirs = packed_points(dev[0], dd, *dev[2:])
    dirs.sum().backward()
    counts = np.diff(seg).astype(np.float64)
    close_grad(dd.grad, np.repeat(counts[:, None], 3, axis=1), "rays_d.grad from dirs alone")
