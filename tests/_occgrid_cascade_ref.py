"""CPU restatement of the cascaded marching contract of include/nerf_amd.h
(csrc/occgrid_cascade.hip) in numpy fp32, shared by tests/test_occgrid_cascade_logic.py (CPU) and
test_gpu_occgrid_cascade.py.  No GPU, no HIP library.  Every operation is rounded to fp32 on its
own, in the kernel's order, nothing contracted; min / max are the comparisons the contract spells out.
"""
import numpy as np

import _occgrid_ref as R1
from oracle import nerf_oracle as O

F32 = np.float32
MAX_STEPS = R1.MAX_STEPS


def cascade_aabbs(roi_aabb, levels):
    """The host's boxes, fp32 [levels, 6]: c = (lo + hi) * 0.5, h = (hi - lo) * 0.5,
    lo_l = c - h * 2^l, hi_l = c + h * 2^l."""
    lo = np.asarray(roi_aabb[:3], dtype=F32)
    hi = np.asarray(roi_aabb[3:], dtype=F32)
    c = ((lo + hi).astype(F32) * F32(0.5)).astype(F32)
    h = ((hi - lo).astype(F32) * F32(0.5)).astype(F32)
    out = np.zeros((levels, 6), dtype=F32)
    for l in range(levels):
        e = (h * F32(2.0 ** l)).astype(F32)
        out[l, :3] = (c - e).astype(F32)
        out[l, 3:] = (c + e).astype(F32)
    return out


def march_cascade_ref(rays_o, rays_d, aabbs, res, binaries, near, far, dt, cone=0.0, t_lo=None, t_hi=None,
                      stratified=False, seed=0, counter=0, mask_words=MAX_STEPS // 64):
    """(ray_indices int64 [N], t_starts fp32 [N], t_ends fp32 [N], status int, info).  aabbs: fp32
    [levels, 6]; binaries: bool [levels, rx, ry, rz] (or flat).  info: 'considered' steps per ray [R],
    'level' of each sample [N], 'cone_step' (the step's length was s * cone, not dt) [N], 'chain' the
    (s_k) of the last ray marched by the recurrence, s_n included."""
    rays_o = np.asarray(rays_o, dtype=F32).reshape(-1, 3)
    rays_d = np.asarray(rays_d, dtype=F32).reshape(-1, 3)
    aabbs = np.asarray(aabbs, dtype=F32).reshape(-1, 6)
    levels = aabbs.shape[0]
    res = [int(r) for r in res]
    cells = res[0] * res[1] * res[2]
    flat = np.asarray(binaries, dtype=bool).reshape(-1)
    assert flat.size == levels * cells
    near, far, dt, cone = F32(near), F32(far), F32(dt), F32(cone)
    lo_o, hi_o = aabbs[-1, :3], aabbs[-1, 3:]
    limit = min(MAX_STEPS, 64 * mask_words)
    out_r, out_0, out_1, out_l, out_c, considered = [], [], [], [], [], []
    chain = None
    status = 0
    with np.errstate(all="ignore"):
        for r in range(rays_o.shape[0]):
            o, d = rays_o[r], rays_d[r]
            tn, tf = F32(-np.inf), F32(np.inf)
            hit = True
            for a in range(3):
                if d[a] == 0:
                    if not (lo_o[a] <= o[a] < hi_o[a]):
                        hit = False
                else:
                    inv = F32(F32(1.0) / d[a])
                    ta = F32(F32(lo_o[a] - o[a]) * inv)
                    tb = F32(F32(hi_o[a] - o[a]) * inv)
                    mn = ta if ta < tb else tb
                    mx = tb if ta < tb else ta
                    tn = mn if mn > tn else tn
                    tf = mx if mx < tf else tf
            t_min = near if near > tn else tn
            if t_lo is not None:
                t_min = F32(t_lo[r]) if F32(t_lo[r]) > t_min else t_min
            t_max = far if far < tf else tf
            if t_hi is not None:
                t_max = F32(t_hi[r]) if F32(t_hi[r]) < t_max else t_max
            if not (hit and bool(t_min < t_max)):
                considered.append(0)
                continue
            if stratified:
                u = O.philox_uniform(seed, counter, np.array([r], dtype=np.uint64))[0]
                t_min = F32(t_min + F32(u * dt))
            if cone == 0:
                x = np.ceil(F32(F32(t_max - t_min) / dt))
                if x > MAX_STEPS:
                    status |= 1
                n = (int(x) if x < MAX_STEPS else MAX_STEPS) if x >= 1 else 0
                if n > 64 * mask_words:
                    status |= 2
                    n = 64 * mask_words
                k = np.arange(n)
                t0 = (t_min + (k.astype(F32) * dt).astype(F32)).astype(F32)
                e1 = (t_min + ((k + 1).astype(F32) * dt).astype(F32)).astype(F32)
                by_cone = np.zeros(n, dtype=bool)
            else:
                s, ss, by = t_min, [], []
                while s < t_max and len(by) < limit:
                    w = F32(s * cone)
                    ss.append(s)
                    by.append(bool(w > dt))
                    s = F32(s + (w if w > dt else dt))
                if s < t_max:                   # cut: at NERF_OCC_MAX_STEPS bit 0, at the mask capacity bit 1
                    status |= 1 if limit == MAX_STEPS else 2
                ss.append(s)
                chain = np.asarray(ss, dtype=F32)
                n = len(by)
                t0, e1 = chain[:-1], chain[1:]
                by_cone = np.asarray(by, dtype=bool)
            considered.append(n)
            if n == 0:
                continue
            t1 = np.where(e1 < t_max, e1, t_max).astype(F32)
            keep = t0 < t1
            tm = ((t0 + t1).astype(F32) * F32(0.5)).astype(F32)
            p = [(o[a] + (tm * d[a]).astype(F32)).astype(F32) for a in range(3)]
            level = np.full(n, -1, dtype=np.int64)
            for l in range(levels - 1, -1, -1):     # the smallest containing level wins
                inside = np.ones(n, dtype=bool)
                for a in range(3):
                    inside &= (aabbs[l, a] <= p[a]) & (p[a] < aabbs[l, 3 + a])
                level[inside] = l
            keep &= level >= 0
            lv = np.where(level >= 0, level, 0)
            cell = np.zeros(n, dtype=np.int64)
            for a in range(3):
                lo_a, hi_a = aabbs[lv, a], aabbs[lv, 3 + a]
                ext = (hi_a - lo_a).astype(F32)
                c = np.floor((((p[a] - lo_a).astype(F32) / ext).astype(F32) * F32(res[a])).astype(F32))
                keep &= (c >= 0) & (c < res[a])
                cell = cell * res[a] + np.where(keep, c, 0).astype(np.int64)
            keep &= flat[np.where(keep, lv * cells + cell, 0)]
            out_r.append(np.full(int(keep.sum()), r, dtype=np.int64))
            out_0.append(t0[keep])
            out_1.append(t1[keep])
            out_l.append(level[keep])
            out_c.append(by_cone[keep])
    cat = lambda xs, dt_: np.concatenate(xs).astype(dt_) if xs else np.zeros(0, dtype=dt_)
    info = {"considered": np.asarray(considered, dtype=np.int64), "level": cat(out_l, np.int64),
            "cone_step": cat(out_c, bool), "chain": chain}
    return cat(out_r, np.int64), cat(out_0, F32), cat(out_1, F32), status, info


def cascade_case():
    """The rays, dt and near / far of _occgrid_ref.checkerboard_case() through three levels (halves
    0.5, 1, 2) of 8^3 cells around [-0.5, 0.5]^3, binaries[l][i, j, k] = (i + j + k + l) % 2.
    Returns (o, d, aabbs, res, binaries, near, far, dt)."""
    o, d, _, res, _, near, far, dt = R1.checkerboard_case()
    l, i, j, k = np.meshgrid(np.arange(3), np.arange(8), np.arange(8), np.arange(8), indexing="ij")
    binaries = ((i + j + k + l) % 2).astype(bool)
    return o, d, cascade_aabbs([-0.5, -0.5, -0.5, 0.5, 0.5, 0.5], 3), res, binaries, near, far, dt


MISSING_RAYS = (np.array([[5.0, 5.0, 5.0], [-3.0, 0.0, 0.0], [0.0, 2.5, 0.0], [0.0, 0.0, -4.0]], dtype=F32),
                np.array([[1.0, 0.0, 0.0], [-1.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], dtype=F32))
"""Four rays that miss the outermost box [-2, 2]^3 of cascade_case()."""


def cone_count_case():
    """The recurrence count construction: o = (-1, .3, .6), d = (1, 0, 0) through [0, 0, 0, 4, 1, 1],
    one level of 8^3 cells all set, near 0, far 1e9, dt 1/1024, cone 0.004: 404 steps from t = 1 to 5.
    Returns (o, d, aabbs, res, binaries, near, far, dt, cone)."""
    o = np.array([[-1.0, 0.3, 0.6]], dtype=F32)
    d = np.array([[1.0, 0.0, 0.0]], dtype=F32)
    aabbs = np.array([[0.0, 0.0, 0.0, 4.0, 1.0, 1.0]], dtype=F32)
    return o, d, aabbs, (8, 8, 8), np.ones((1, 8, 8, 8), dtype=bool), 0.0, 1e9, 1.0 / 1024, 0.004


def cone_count_bounds():
    """Per m of COUNT_M the two t_max of the construction: s_m itself (exactly m samples), and the
    fp32 midpoint of s_{m-1} and s_m (m samples, the last clipped to it).  Returns (chain, [(m, t_max,
    clipped)])."""
    o, d, aabbs, res, binaries, near, far, dt, cone = cone_count_case()
    chain = march_cascade_ref(o, d, aabbs, res, binaries, near, far, dt, cone)[4]["chain"]
    bounds = []
    for m in R1.COUNT_M:
        bounds.append((m, chain[m], False))
        bounds.append((m, F32(F32(chain[m - 1] + chain[m]) * F32(0.5)), True))
    return chain, bounds


def points_ref(rays_o, rays_d, ri, t0, t1):
    """The points contract of include/nerf_amd.h in numpy fp32: o + ((t0 + t1) * 0.5) * d."""
    tm = ((t0 + t1).astype(F32) * F32(0.5)).astype(F32)
    return (rays_o[ri] + (tm[:, None] * rays_d[ri]).astype(F32)).astype(F32)
