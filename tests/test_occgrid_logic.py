"""Occupancy-grid sampler and packed compositing, without a GPU: the numpy fp32 restatement of the
marching contract (tests/_occgrid_ref.py) on constructions whose answer is known, the grid update
rule of nerf_amd.occ_grid.OccGridEstimator (plain torch ops, so it runs on the CPU), the C ABI's
argument validation, and the distance between an fp32 and the fp64 evaluation of the packed
compositing contract, which sets the margin of the GPU tests' bars.

Bars of the GPU tests (tests/test_gpu_composite_packed.py): colours, opacity, weights 2e-6 abs,
gradients 2e-5 abs + 1e-5 rel (the project's compositing bars, tests/test_gpu_parity.py); depth
2e-6 * far_plane, a weight sum with coefficients of at most far.  Measured here on the GPU tests'
inputs (segments [0, 1, 63, 64, 65, 0, 0, 128, 129, 1500, 2, 0], far 6): the fp32 torch evaluation
lies within 2.5e-7 (colours), 5.3e-7 (opacity), 4.6e-8 (weights), 6.7e-7 (depth, bar 1.2e-5) of the
fp64 restatement and within 0.4 % of the gradient bar, so each bar leaves a factor above three and the
depth bar is not widened.
"""
import ctypes

import numpy as np
import pytest
import torch

import _occgrid_ref as R

F32 = np.float32
LENGTHS = [0, 1, 63, 64, 65, 0, 0, 128, 129, 1500, 2, 0]
FAR = 6.0


@pytest.mark.parametrize("m", R.COUNT_M)
def test_count_construction(m):
    o, d, aabb, res, binaries, near, far, dt = R.count_construction(m)
    ri, t0, t1, status, considered = R.march_ref(o, d, aabb, res, binaries, near, far, dt)
    assert ri.size == m and status == 0 and np.all(ri == 0)
    assert np.array_equal(t1[:-1].view(np.uint32), t0[1:].view(np.uint32)), "consecutive steps abut bitwise"
    assert np.all(t0 < t1) and considered[0] >= m


def test_misses_and_zero_direction_components():
    aabb, res, occ = [0.0, 0.0, 0.0, 1.0, 1.0, 1.0], (4, 4, 4), np.ones((4, 4, 4), dtype=bool)
    run = lambda o, d, near=0.0, far=1e9, dt=0.125: R.march_ref([o], [d], aabb, res, occ, near, far, dt)
    # points away from the box; passes beside it
    assert run([-1, 0.5, 0.5], [-1, 0, 0])[0].size == 0
    assert run([-1, 2.5, 0.5], [1, 0, 0])[0].size == 0
    # zero components inside the slab: a full chord of 8 steps; on the upper face (hi is outside), below lo
    assert run([-1, 0.5, 0.5], [1, 0, 0])[0].size == 8
    assert run([-1, 1.0, 0.5], [1, 0, 0])[0].size == 0
    assert run([-1, 0.0, 0.5], [1, 0, 0])[0].size == 8
    assert run([-1, -1e-6, 0.5], [1, 0, 0])[0].size == 0
    # all components zero, origin inside: t in [near, far], every step at the origin's cell
    ri, t0, t1, status, considered = run([0.5, 0.5, 0.5], [0, 0, 0], near=1.0, far=2.0)
    assert ri.size == 8 and t0[0] == 1.0 and t1[-1] == 2.0
    # t_min >= t_max: the box lies before near, or behind far
    assert run([-1, 0.5, 0.5], [1, 0, 0], near=2.0)[0].size == 0
    assert run([-1, 0.5, 0.5], [1, 0, 0], near=0.0, far=1.0)[0].size == 0
    assert run([-1, 0.5, 0.5], [1, 0, 0], near=1.5, far=1.5)[0].size == 0
    # the last step is clipped to t_max
    ri, t0, t1, _, _ = run([-1, 0.5, 0.5], [1, 0, 0], dt=0.3)
    assert ri.size == 4 and t1[-1] == 2.0 and t0[0] == 1.0


def test_empty_cells_are_skipped_and_truncation_is_flagged():
    aabb, res = [0.0, 0.0, 0.0, 1.0, 1.0, 1.0], (4, 1, 1)
    occ = np.array([True, False, True, False]).reshape(4, 1, 1)
    ri, t0, t1, status, _ = R.march_ref([[-1, 0.5, 0.5]], [[1, 0, 0]], aabb, res, occ, 0.0, 1e9, 0.125)
    assert np.array_equal(t0, np.array([1.0, 1.125, 1.5, 1.625], dtype=F32)) and status == 0
    ri, t0, t1, status, considered = R.march_ref([[-1, 0.5, 0.5]], [[1, 0, 0]], aabb, res, occ, 0.0, 1e9, 1e-5)
    assert status == 1 and considered[0] == R.MAX_STEPS and ri.size == R.MAX_STEPS


def test_checkerboard_case_is_not_degenerate():
    ri, t0, t1, status, considered = R.march_ref(*R.checkerboard_case())
    counts = np.bincount(ri, minlength=64)
    assert status == 0 and (counts > 0).sum() >= 48 and counts.max() > 64 and len(set(counts)) > 16
    assert np.all(np.diff(ri) >= 0) and np.all(t0 < t1)


def ball(x):
    return (x.norm(dim=-1) < 0.6).float()


def test_update_marks_the_ball_and_state_dict_round_trips():
    from nerf_amd import OccGridEstimator
    from nerf_amd.occ_grid import pack_grid_bits
    torch.manual_seed(0)
    est = OccGridEstimator([-1.0, -1.0, -1.0, 1.0, 1.0, 1.0], resolution=16)
    assert est.occs.shape == (4096,) and est.binaries.shape == (1, 16, 16, 16) and est.binaries.dtype == torch.bool
    est.update_every_n_steps(3, ball)                     # not a multiple of n: nothing happens
    assert not est.binaries.any()
    est.update_every_n_steps(0, ball)                     # warm-up: every cell, at a jittered point
    edges = torch.linspace(-1, 1, 17)
    lo, hi = edges[:-1], edges[1:]
    near1 = torch.where((lo <= 0) & (hi >= 0), torch.zeros(16), torch.minimum(lo.abs(), hi.abs()))
    far1 = torch.maximum(lo.abs(), hi.abs())
    axes = lambda v: torch.stack(torch.meshgrid(v, v, v, indexing="ij"), -1)
    inside = axes(far1).norm(dim=-1) < 0.6                # the cell's farthest corner is in the ball
    outside = axes(near1).norm(dim=-1) > 0.6              # its nearest point is not
    b = est.binaries[0]
    assert inside.sum() > 100 and outside.sum() > 1000
    assert b[inside].all() and not b[outside].any()
    # past warm-up: a quarter of the cells plus occupied ones; the ball stays marked
    est.update_every_n_steps(512, ball)
    assert est.binaries[0][inside].all() and not est.binaries[0][outside].any()
    # state_dict carries both buffers; the packed copy follows the loaded grid
    sd = est.state_dict()
    assert set(sd) == {"occs", "binaries"}
    other = OccGridEstimator([-1.0, -1.0, -1.0, 1.0, 1.0, 1.0], resolution=16)
    assert not other.grid_bits().any()
    other.load_state_dict(sd)
    assert torch.equal(other.binaries, est.binaries) and torch.equal(other.occs, est.occs)
    assert torch.equal(other.grid_bits(), pack_grid_bits(est.binaries))
    bits = other.grid_bits().numpy().view(np.uint32)
    flat = est.binaries.reshape(-1).numpy()
    assert np.array_equal(((bits[:, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(-1).astype(bool), flat)


def test_constructor_and_sampling_refusals():
    from nerf_amd import OccGridEstimator
    with pytest.raises(NotImplementedError):
        OccGridEstimator([0, 0, 0, 1, 1, 1], levels=2)
    est = OccGridEstimator([0, 0, 0, 1, 1, 1], resolution=(4, 5, 6))
    assert est.binaries.shape == (1, 4, 5, 6)
    with pytest.raises(NotImplementedError):
        est.sampling(torch.zeros(1, 3), torch.ones(1, 3), cone_angle=0.01)


def test_capi_argument_validation_without_launch():
    from nerf_amd import _lib
    lib = _lib.load()
    box = (ctypes.c_float * 6)(0, 0, 0, 1, 1, 1)
    res = (ctypes.c_int32 * 3)(8, 8, 8)
    W = lib.nerf_occ_march_workspace
    assert W(0, 1) == 0 and W(-1, 1) == 0 and W(5, 0) == 0 and W(5, 129) == 0
    assert W(5, 2) == 256 + 5 * 2 * 8 and W(13, 128) == 512 + 13 * 128 * 8
    count = lambda o=256, d=256, n=4, bx=box, rs=res, bits=256, dt=0.1, words=2, ws=256, nb=1 << 20, st=256: \
        lib.nerf_occ_march_count(o, d, n, bx, rs, bits, 0.0, 1.0, dt, 0, 0, 0, words, ws, nb, st, None)
    assert count(n=0, o=None, d=None, bits=None, ws=None, st=None) == 0
    assert count(o=None) == -1 and count(bits=None) == -1 and count(ws=None) == -1 and count(st=None) == -1
    assert count(o=258) == -1 and count(ws=384) == -1 and count(st=257) == -1          # misaligned
    assert count(dt=0.0) == -1 and count(dt=float("nan")) == -1 and count(words=0) == -1 and count(words=129) == -1
    assert count(n=-1) == -1
    assert count(bx=(ctypes.c_float * 6)(0, 0, 0, 1, 0, 1)) == -1
    assert count(rs=(ctypes.c_int32 * 3)(8, 0, 8)) == -1
    assert count(nb=W(4, 2) - 1) == -4
    write = lambda n=4, dt=0.1, words=2, ws=256, nb=1 << 20, cum=256, N=10, ri=256, t0=256, t1=256: \
        lib.nerf_occ_march_write(n, dt, words, ws, nb, cum, N, ri, t0, t1, None)
    assert write(n=0, ws=None, cum=None) == 0 and write(N=0, ri=None, t0=None, t1=None) == 0
    assert write(ws=None) == -1 and write(cum=None) == -1 and write(ri=None) == -1 and write(t1=None) == -1
    assert write(cum=260) == -1 and write(ri=260) == -1 and write(t0=258) == -1 and write(ws=320) == -1
    assert write(N=-1) == -1 and write(words=200) == -1 and write(dt=-1.0) == -1
    assert write(nb=100) == -4
    fwd = lambda s=256, ss=1, c=256, cs=3, t0=256, t1=256, seg=256, R_=4, N=10, col=256, w=256: \
        lib.nerf_composite_packed_fwd(s, ss, c, cs, t0, t1, seg, R_, N, col, 256, 256, w, 256, 256, None)
    assert fwd(R_=0, s=None, seg=None) == 0
    assert fwd(seg=None) == -1 and fwd(s=None) == -1 and fwd(t1=None) == -1 and fwd(R_=-1) == -1 and fwd(N=-1) == -1
    assert fwd(seg=260) == -1 and fwd(s=258) == -1 and fwd(w=257) == -1 and fwd(cs=2) == -1 and fwd(ss=0) == -1
    bwd = lambda s=256, c=256, seg=256, R_=4, N=10, w=256, T=256, gs=256, gss=1, gc=256, gcs=3: \
        lib.nerf_composite_packed_bwd(s, 1, c, 3, 256, 256, seg, R_, N, w, T, 256, 256, 256, 256, gs, gss, gc, gcs,
                                      None)
    assert bwd(R_=0, s=None, seg=None) == 0 and bwd(N=0, s=None) == 0
    assert bwd(seg=None) == -1 and bwd(s=None) == -1 and bwd(w=None) == -1 and bwd(T=None) == -1
    assert bwd(seg=252) == -1 and bwd(T=258) == -1 and bwd(gs=257) == -1 and bwd(gcs=2) == -1 and bwd(gss=0) == -1
    assert bwd(c=None) == -1                               # a colour gradient needs the colours
    assert lib.nerf_abi_version() == 10


def test_packed_restatement_agrees_with_a_direct_evaluation():
    """packed_composite_ref64 (composite_ref64 per segment, opacity and depth gradients folded into the
    weight gradient) against the contract written out with autograd through every output, with and
    without colours."""
    args = R.packed_inputs(LENGTHS, 11, FAR)
    for a in (args, (args[0], None) + args[2:]):
        for x, y in zip(R.packed_composite_ref64(*a), R.packed_composite_direct64(*a)):
            assert (x is None) == (y is None)
            assert x is None or float((x - y).abs().max()) < 1e-13


def test_fp32_evaluation_stays_within_a_third_of_each_bar():
    """The fp32 torch evaluation of the packed contract against the fp64 restatement on the GPU tests'
    inputs.  Measured: colours 2.5e-7, opacity 5.3e-7 (27 % of its bar, the largest share), weights
    4.6e-8, depth 6.7e-7 (bar 2e-6 * 6 = 1.2e-5), gradients at most 0.4 % of 2e-5 + 1e-5 |ref|: all
    below a third, no bar widened."""
    args = R.packed_inputs(LENGTHS, 11, FAR)
    ref = R.packed_composite_ref64(*args)
    got = R.packed_composite_fp32(*args)
    names = ("colours", "opacity", "depth", "weights", "trans", "alphas", "d sigma", "d rgb")
    bars = (2e-6, 2e-6, 2e-6 * FAR, 2e-6, 2e-6, 2e-6, None, None)
    for name, g, r, bar in zip(names, got, ref, bars):
        err = (g.double() - r).abs()
        if bar is None:
            share = float((err / (2e-5 + 1e-5 * r.abs())).max())
        else:
            share = float(err.max()) / bar
        print(f"{name}: max |fp32 - fp64| = {float(err.max()):.3e}, {100 * share:.1f} % of the bar")
        assert share < 1 / 3, name
    # empty rays give zeros
    empty = [i for i, L in enumerate(LENGTHS) if L == 0]
    assert torch.all(ref[0][empty] == 0) and torch.all(ref[1][empty] == 0) and torch.all(ref[2][empty] == 0)
