"""CPU checks of tests/_hashgrid3d_ref.py, the restatements tests/test_gpu_hashgrid_edges.py holds the
3-D hash-grid kernels to: the fixed-point table gradient against the fp64 oracle within the rule's own
roundings, the shift rule's guarantees, the sensitivity of the restatement to small mutations of the
rule (so that "bitwise" means something), the position gradient's bound being far below the values it
guards, and — through the library's host-side sizing — the kernel path every config is named for."""
import math

import numpy as np
import pytest

import _hashgrid3d_ref as R
from oracle import hashgrid_oracle as O

TAGS = list(R.CONFIGS)


def _shift_of(g, n):
    return R.fixed_shift(n, float(np.abs(g).max()))


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("n", [1, 257, 4097])
def test_restatement_within_its_own_roundings_of_the_fp64_oracle(tag, n):
    """Each of a row's `hits` contributions is rounded once to the grid 2^-s (half a step each), and the
    sum once to fp32: |fixed - fp64| <= hits 2^-(s+1) + 2^-24 |ref| per entry."""
    res, T, F, primes, normalize = R.cfg_args(tag)
    x, g = R.points(tag, n), R.grads(tag, n, wide=True)
    got = R.table_grad_fixed(x, g, res, T, F, primes, normalize)
    ref, hits = R.table_grad64(x, g, res, T, F, primes, normalize)
    s = _shift_of(g, n)
    tol = hits[:, None] * math.ldexp(1.0, -(s + 1)) + R.U * np.abs(ref)
    err = np.abs(got.astype(np.float64) - ref)
    print(f"{tag} n={n}: s={s} max err {err.max():.3e} = {err.max() / np.abs(ref).max():.2e} of the largest entry")
    assert got.shape == ref.shape == (sum(O.level_rows(r, T) for r in res), F)
    assert (err <= tol).all()
    assert not got[hits == 0].any() and np.abs(ref).max() > 0


def test_shift_rule():
    one_below = float(np.float32(1.0) - np.float32(2.0 ** -24))
    for n in (1, 2, 63, 255, 256, 257, 4097, 1 << 20, (1 << 31) - 1):
        for gmax in (one_below, 1.0, 1e-3, 3.0, 1e30, 1e-20, float(np.finfo(np.float32).max),
                     float(np.finfo(np.float32).tiny)):
            s = R.fixed_shift(n, gmax)
            # no accumulator can overflow: a row takes at most 8 n contributions of at most gmax 2^s
            assert 8.0 * n * gmax * math.ldexp(1.0, s) < 2.0 ** 62, (n, gmax)
            # from 256 samples on every contribution is below 2^51, where rint_fixed equals llrint
            if n >= 256:
                assert gmax * math.ldexp(1.0, s) < 2.0 ** 51, (n, gmax)
            if s < 120:
                assert 8.0 * n * gmax * math.ldexp(1.0, s + 1) >= 2.0 ** 62, (n, gmax)   # the largest such s
    assert R.fixed_shift(256, one_below) == 51 and one_below * 2.0 ** 51 < 2.0 ** 51
    assert R.fixed_shift(256, 1.0) == 50
    assert R.fixed_shift(257, 1e-30) == 120                   # the cap
    assert R.fixed_shift(257, 0.0) == 60
    assert R.fixed_shift(257, float("inf")) is None and R.fixed_shift(257, float("nan")) is None
    res, T, F, primes, normalize = R.cfg_args("A")
    x, g = R.points("A", 65), R.grads("A", 65)
    g[3, 1] = np.inf
    assert np.isnan(R.table_grad_fixed(x, g, res, T, F, primes, normalize)).all()
    assert not R.table_grad_fixed(x, np.zeros_like(g), res, T, F, primes, normalize).any()
    assert R.table_grad_fixed(x[:0], g[:0], res, T, F, primes, normalize).shape == (125 + 3 * 1024, 2)


def _swapped_yz(x, r, T, primes=O.PRIMES, normalize=True):
    """level_corners with the y and z strides of a bijective level exchanged."""
    idx, w = O.level_corners(x, r, T, primes, normalize)
    if (r + 1) ** 3 <= T:
        u = O.normalised(x) if normalize else x.astype(np.float32)
        base = np.floor(u * np.float32(r)).astype(np.int64)
        for k, off in enumerate(O.CORNERS_3D):
            c = np.clip(base + np.array(off, dtype=np.int64), 0, r)
            idx[:, k] = c[:, 0] + (r + 1) * c[:, 2] + (r + 1) * (r + 1) * c[:, 1]
    return idx, w


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_is_sensitive_to_the_rule(tag):
    res, T, F, primes, normalize = R.cfg_args(tag)
    n = 257
    x, g = R.points(tag, n), R.grads(tag, n, wide=True)
    want = R.table_grad_fixed(x, g, res, T, F, primes, normalize)
    mutations = dict(last_corner_dropped=dict(n_corners=7), truncated=dict(rnd=np.trunc), coarser_grid=dict(shift=-1))
    if any((r + 1) ** 3 <= T for r in res):                   # (G has no bijective level to swap)
        mutations["yz_swapped"] = dict(corners=_swapped_yz)
    else:
        assert tag == "G"
    for name, kw in mutations.items():
        got = R.table_grad_fixed(x, g, res, T, F, primes, normalize, **kw)
        assert not np.array_equal(got.view(np.int32), want.view(np.int32)), name
    base = np.random.default_rng(1).standard_normal(want.shape).astype(np.float32)
    assert np.array_equal(R.table_grad_fixed(x, g, res, T, F, primes, normalize, accumulate=base), base + want)


@pytest.mark.parametrize("tag", TAGS)
def test_position_bound_is_far_below_the_values(tag):
    """Not a measurement: the condition that keeps the derived bound from being vacuous.  Its largest
    element is at most 1e-4 of the tensor's largest reference entry, and finite on every edge row."""
    res, T, F, primes, normalize = R.cfg_args(tag)
    tabs = R.tables(tag)
    for n in R.SIZES[1:]:
        x, g = R.points(tag, n), R.grads(tag, n)
        ref, bound = R.pos_grad64_with_bound(x, tabs, res, T, g, primes, normalize)
        ratio = bound.max() / np.abs(ref).max()
        print(f"{tag} n={n}: largest bound {bound.max():.3e} = {ratio:.2e} of the largest entry {np.abs(ref).max():.3e}")
        assert np.isfinite(bound).all() and np.isfinite(ref).all()
        assert 0 < ratio <= 1e-4, (tag, n, ratio)
        e = min(n, R.edge_rows(tag).shape[0])
        assert np.array_equal(x[:e], R.edge_rows(tag)[:e])


def test_ray_positions_are_the_fp32_expression():
    o, d, t0, t1 = R.rays("A", 5, 3, n=14)
    for query in (0, 1):
        pos = R.ray_positions(o, d, t0, t1, 3, query)
        assert pos.dtype == np.float32 and pos.shape == (14, 3)
        tq = t0 if query == 0 else (t0 + t1) / np.float32(2)
        for i in (0, 2, 3, 13):
            want = o[i // 3] + (tq[i] * d[i // 3]).astype(np.float32)
            assert np.array_equal(pos[i], want.astype(np.float32))


def _r256(v):
    return (v + 255) // 256 * 256


# levels the bucketed passes' region of nerf_hashgrid_workspace_n is sized for.  The sizing formula
# looks at the level layout and the part count only, not at F: D (F = 3) and H (F = 8) get a region
# that nerf_hashgrid_bwd never uses (the bucketed passes exist for F = 1, 2 and 4), so for them this
# asserts what the formula gives; their kernel path is the walk whatever the workspace.
BUCKETED_LEVELS = {"A": 3, "B": 2, "C": 1, "D": 3, "E": 0, "G": 3, "H": 30}


@pytest.mark.parametrize("tag", TAGS)
def test_configs_reach_the_paths_they_are_named_for(tag):
    from nerf_amd import kernels as K
    res, T, F, primes, normalize = R.cfg_args(tag)
    L = len(res)
    p = K.make_hashgrid_params(L, T, F, res, primes=primes, normalize=normalize)
    hashed = [(r + 1) ** 3 > T for r in res]
    trailing = next((i for i, h in enumerate(reversed(hashed)) if not h), L)
    assert trailing == BUCKETED_LEVELS[tag]
    for n in (65, 257, 4097):
        base = _r256(K.hashgrid_workspace_bytes(p)) + _r256(n * 16 + n * L * F * 4)
        region = K.hashgrid_workspace_bytes(p, n) - base
        nparts = -(-T // (10240 // F))
        nb = trailing * nparts * 16
        cap = ((8 * n * 5 // 4) // (nparts * 16) + 4096 + 63) // 64 * 64
        want = _r256(nb * 4) + 2 * _r256(nb * cap * 4) if trailing else 0
        assert region == want, (tag, n, region, want)
    assert K.hashgrid_workspace_bytes(p, 0) == _r256(K.hashgrid_workspace_bytes(p))      # an empty batch: no region
    # what the names promise
    if tag == "E":
        assert not any(hashed)
    if tag == "G":
        assert all(hashed)                                    # no part left for the walk launch
    if tag == "C":
        assert hashed == [True, False, True, False, True]
    if tag == "B":
        assert T & (T - 1) != 0 and not normalize
    if tag in ("D", "H"):
        assert F not in (1, 2, 4) and (tag == "H" or (L * F) % 4 != 0)
    assert max(O.level_rows(r, T) for r in res) <= 4096
