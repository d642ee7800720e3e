"""The cascaded occupancy grid without a GPU: the numpy fp32 restatement of the cascaded marching
contract (tests/_occgrid_cascade_ref.py) against the one-level restatement and on constructions
whose answer is known, the C ABI's argument validation, and the host side of
nerf_amd.CascadedOccGridEstimator (boxes, buffers, the grid update in plain torch ops).
"""
import ctypes

import numpy as np
import pytest
import torch

import _occgrid_cascade_ref as C
import _occgrid_ref as R

F32 = np.float32


def bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_one_level_is_the_one_level_contract():
    o, d, aabb, res, binaries, near, far, dt = R.checkerboard_case()
    want = R.march_ref(o, d, aabb, res, binaries, near, far, dt)
    got = C.march_cascade_ref(o, d, C.cascade_aabbs(aabb, 1), res, binaries[None], near, far, dt)
    assert want[0].size == 4092 and np.array_equal(got[0], want[0])
    assert bits_equal(got[1], want[1]) and bits_equal(got[2], want[2]) and got[3] == want[3] == 0
    assert np.array_equal(got[4]["considered"], want[4])
    assert np.array_equal(C.cascade_aabbs(aabb, 1), np.array([aabb], dtype=F32))


@pytest.mark.parametrize("cone, samples, per_level, dt_steps, cone_steps",
                         [(0.0, 9515, (827, 3351, 5337), 9515, 0), (0.01, 6634, (546, 2294, 3794), 3105, 3529)])
def test_cascade_case(cone, samples, per_level, dt_steps, cone_steps):
    """The sample totals and the split by level are those of an independent prototype of the contract.
    The split by step rule counts the branch h_k took (w_k > dt); the prototype's 3115 / 3519 at cone
    0.01 is the split by interval length (t1 - t0 at most dt, or longer), which moves ten cone-rule
    steps that t_max clipped to no more than dt: the last samples of their rays, checked below."""
    case = C.cascade_case()
    assert np.array_equal(case[2], np.array([[-h] * 3 + [h] * 3 for h in (0.5, 1.0, 2.0)], dtype=F32))
    ri, t0, t1, status, info = C.march_cascade_ref(*case, cone=cone)
    assert ri.size == samples and status == 0
    assert tuple(np.bincount(info["level"], minlength=3)) == per_level
    assert np.bincount(ri, minlength=64).min() > 0, "no ray is empty"
    assert int((~info["cone_step"]).sum()) == dt_steps and int(info["cone_step"].sum()) == cone_steps
    assert np.all(np.diff(ri) >= 0) and np.all(t0 < t1)
    if cone:
        short = t1.astype(np.float64) - t0 <= case[7] * (1 + 1e-5)
        assert int(short.sum()) == 3115 and int((~short).sum()) == 3519
        moved = info["cone_step"] & short                   # cone-rule steps clipped at t_max to at most dt
        last_of_ray = np.append(ri[1:] != ri[:-1], True)
        assert int(moved.sum()) == 10 and last_of_ray[moved].all()


def test_cone_steps_grow_and_abut():
    o, d, aabbs, res, binaries, near, far, dt, cone = C.cone_count_case()
    ri, t0, t1, status, info = C.march_cascade_ref(o, d, aabbs, res, binaries, near, far, dt, cone)
    assert ri.size == 404 and status == 0 and t0[0] == 1.0 and t1[-1] == 5.0
    assert bits_equal(t1[:-1], t0[1:]), "consecutive steps abut bitwise"
    assert info["cone_step"].all() and np.all(np.diff(t1 - t0)[:-1] >= 0)
    assert info["chain"].size == 405 and bits_equal(info["chain"][:-1], t0)


@pytest.mark.parametrize("m", R.COUNT_M)
def test_cone_count_construction(m):
    o, d, aabbs, res, binaries, near, far, dt, cone = C.cone_count_case()
    chain, bounds = C.cone_count_bounds()
    for mm, t_max, clipped in bounds:
        if mm != m:
            continue
        ri, t0, t1, status, _ = C.march_cascade_ref(o, d, aabbs, res, binaries, near, far, dt, cone,
                                                    t_hi=np.array([t_max], dtype=F32))
        assert ri.size == m and status == 0
        assert bits_equal(t0, chain[:m]) and bits_equal(t1[:-1], chain[1:m]) and t1[-1] == t_max
        assert (t_max < chain[m]) == clipped and chain[m - 1] < t_max


def test_ray_bounds_and_cut_in_the_restatement():
    o, d, aabbs, res, binaries, near, far, dt, cone = C.cone_count_case()
    run = lambda **kw: C.march_cascade_ref(o, d, aabbs, res, binaries, near, far, dt, **kw)
    f = lambda v: np.array([v], dtype=F32)
    # bounds narrow [near, far] and never widen it; t_lo >= t_hi leaves nothing
    assert run(t_lo=f(2.0), t_hi=f(3.0))[1][0] == 2.0 and run(t_lo=f(2.0), t_hi=f(3.0))[2][-1] == 3.0
    assert run(t_lo=f(-5.0), t_hi=f(50.0))[0].size == run()[0].size == 4096
    assert run(t_lo=f(3.0), t_hi=f(2.0))[0].size == 0 and run(t_lo=f(3.0), t_hi=f(3.0))[0].size == 0
    assert run(cone=cone, t_lo=f(4.5))[1][0] == 4.5
    # the recurrence is cut at the mask capacity (bit 1) or at NERF_OCC_MAX_STEPS (bit 0)
    ri, _, _, status, info = run(cone=cone, mask_words=2)
    assert ri.size == 128 and status == 2 and info["considered"][0] == 128
    slow = np.array([[1e-4, 0.0, 0.0]], dtype=F32)
    ri, t0, t1, status, info = C.march_cascade_ref(o, slow, aabbs, res, binaries, near, far, 1.0, 1e-6)
    assert ri.size == C.MAX_STEPS and status == 1 and bits_equal(t1[:-1], t0[1:])


def test_capi_argument_validation_without_launch():
    from nerf_amd import _lib
    lib = _lib.load()
    boxes = (ctypes.c_float * 12)(0, 0, 0, 1, 1, 1, -1, -1, -1, 2, 2, 2)
    res = (ctypes.c_int32 * 3)(8, 8, 8)
    W = lib.nerf_occ_march_workspace
    count = lambda o=256, d=256, n=4, bx=boxes, lv=2, rs=res, bits=256, lo=None, hi=None, dt=0.1, cone=0.0, words=2, \
        ws=256, nb=1 << 20, st=256: lib.nerf_occ_cascade_count(o, d, n, bx, lv, rs, bits, lo, hi, 0.0, 1.0, dt, cone, 0,
                                                                0, 0, words, ws, nb, st, None)
    assert count(n=0, o=None, d=None, bits=None, ws=None, st=None) == 0
    assert count(n=0, cone=0.004, lo=256, hi=256) == 0
    assert count(o=None) == -1 and count(d=None) == -1 and count(bits=None) == -1 and count(ws=None) == -1
    assert count(st=None) == -1 and count(bx=None) == -1 and count(rs=None) == -1
    assert count(o=258) == -1 and count(ws=384) == -1 and count(st=257) == -1          # misaligned
    assert count(lo=258) == -1 and count(hi=257) == -1 and count(bits=254) == -1
    assert count(lv=0) == -1 and count(lv=9) == -1 and count(lv=-1) == -1
    assert count(dt=0.0) == -1 and count(dt=float("nan")) == -1 and count(dt=float("inf")) == -1
    assert count(cone=-0.01) == -1 and count(cone=float("nan")) == -1 and count(cone=float("inf")) == -1
    assert count(words=0) == -1 and count(words=129) == -1 and count(n=-1) == -1
    assert count(bx=(ctypes.c_float * 12)(0, 0, 0, 1, 1, 1, -1, -1, -1, 2, -1, 2)) == -1   # level 1 is empty
    assert count(rs=(ctypes.c_int32 * 3)(8, 0, 8)) == -1
    assert count(nb=W(4, 2) - 1) == -4
    write = lambda n=4, dt=0.1, cone=0.0, words=2, ws=256, nb=1 << 20, cum=256, N=10, ri=256, t0=256, t1=256: \
        lib.nerf_occ_cascade_write(n, dt, cone, words, ws, nb, cum, N, ri, t0, t1, None)
    assert write(n=0, ws=None, cum=None) == 0 and write(N=0, ri=None, t0=None, t1=None) == 0
    assert write(ws=None) == -1 and write(cum=None) == -1 and write(ri=None) == -1 and write(t0=None) == -1
    assert write(t1=None) == -1
    assert write(cum=260) == -1 and write(ri=260) == -1 and write(t0=258) == -1 and write(ws=320) == -1
    assert write(N=-1) == -1 and write(n=-1) == -1 and write(words=200) == -1 and write(dt=-1.0) == -1
    assert write(cone=-1.0) == -1 and write(cone=float("nan")) == -1
    assert write(nb=100) == -4
    # additive: the binding's arity is the header's, and the ABI version did not move
    assert len(_lib._SIGNATURES["nerf_occ_cascade_count"][1]) == 21
    assert len(_lib._SIGNATURES["nerf_occ_cascade_write"][1]) == 12
    assert _lib.NERF_OCC_MAX_LEVELS == 8
    assert lib.nerf_abi_version() == 10


def ball(x):
    return (x.norm(dim=-1) < 0.6).float()


def test_estimator_boxes_buffers_and_refusals():
    import nerf_amd
    from nerf_amd import CascadedOccGridEstimator, OccGridEstimator
    from nerf_amd.occ_grid import pack_grid_bits
    est = nerf_amd.CascadedOccGridEstimator([0.0, 0.0, 0.0, 1.0, 1.0, 1.0], levels=2)     # the base class refuses
    assert isinstance(est, OccGridEstimator) and est.binaries.shape == (2, 128, 128, 128)
    roi = [-0.3, 0.1, -1.0, 0.7, 0.2, 3.0]
    est = CascadedOccGridEstimator(roi, resolution=(4, 5, 6), levels=3)
    assert est.aabbs.dtype == torch.float32 and np.array_equal(est.aabbs.numpy(), C.cascade_aabbs(roi, 3))
    sd = est.state_dict()
    assert set(sd) == {"occs", "binaries"}
    assert sd["occs"].shape == (3 * 120,) and sd["occs"].dtype == torch.float32
    assert sd["binaries"].shape == (3, 4, 5, 6) and sd["binaries"].dtype == torch.bool
    est.binaries[2, 3, 4, 5] = True
    est.binaries[1, 0, 0, 1] = True
    bits = est.grid_bits().numpy().view(np.uint32)
    flat = ((bits[:, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(-1)
    assert list(np.nonzero(flat)[0]) == [120 + 1, 3 * 120 - 1]      # bit l * cells + cell of the flat packing
    other = CascadedOccGridEstimator(roi, resolution=(4, 5, 6), levels=3)
    other.load_state_dict(sd)
    assert torch.equal(other.grid_bits(), pack_grid_bits(est.binaries))
    with pytest.raises(ValueError):
        CascadedOccGridEstimator(roi, levels=0)
    with pytest.raises(ValueError):
        CascadedOccGridEstimator(roi, levels=9)
    with pytest.raises(ValueError):
        est.sampling(torch.zeros(1, 3), torch.ones(1, 3), cone_angle=-0.1)
    with pytest.raises(RuntimeError):                       # no CPU path
        est.sampling(torch.zeros(1, 3), torch.ones(1, 3), cone_angle=0.01)


def test_update_marks_the_ball_on_every_level():
    """The one-level test's criterion per level: cells whose farthest corner is in the ball are set,
    cells whose nearest point is outside are not; level l spans [-2^l, 2^l]^3."""
    from nerf_amd import CascadedOccGridEstimator
    torch.manual_seed(0)
    est = CascadedOccGridEstimator([-1.0, -1.0, -1.0, 1.0, 1.0, 1.0], resolution=16, levels=3)
    est.update_every_n_steps(3, ball)                     # not a multiple of n: nothing happens
    assert not est.binaries.any()
    axes = lambda v: torch.stack(torch.meshgrid(v, v, v, indexing="ij"), -1)

    def criterion(l):
        edges = torch.linspace(-2.0 ** l, 2.0 ** l, 17)
        lo, hi = edges[:-1], edges[1:]
        near1 = torch.where((lo <= 0) & (hi >= 0), torch.zeros(16), torch.minimum(lo.abs(), hi.abs()))
        far1 = torch.maximum(lo.abs(), hi.abs())
        return axes(far1).norm(dim=-1) < 0.6, axes(near1).norm(dim=-1) > 0.6

    def check():
        for l in range(3):
            inside, outside = criterion(l)
            assert outside.sum() > 1000 and (l == 2 or inside.sum() > 0)
            assert est.binaries[l][inside].all() and not est.binaries[l][outside].any(), l
        assert est.binaries[0].sum() > 100 and est.binaries[1].sum() >= 8 and est.binaries[2].sum() >= 1

    est.update_every_n_steps(0, ball)                     # warm-up: every cell of every level
    check()
    est.update_every_n_steps(512, ball)                   # past warm-up: a quarter plus occupied, per level
    check()
    assert est.occs.shape == (3 * 4096,) and float(est.occs.max()) == 1.0
