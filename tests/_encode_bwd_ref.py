"""fp64 restatement of the encoding backward kernels (csrc/encode.hip: nerf_encode_bwd,
nerf_encode_bwd_integrated, nerf_encode_bwd_rays) with a derived per-output error bound, and the
cases the CPU self-check (test_encode_bwd_ref.py) and the GPU tests (test_gpu_encode_bwd_edges.py)
share.  CPU, torch, vectorised; nothing here touches a device.

The gradient (include/nerf_amd.h, encode.hip's comment above encode_bwd_integrated_kernel), per
sample, coordinate d and level k, a = pm_d s_k, s_k = fp32(scale) 2^k, w = exp(-(vb_d 4^k) / 2)
(1 for kind 0), m_k the mask:

    g_pm_d  = g_id_d + sum_k m_k s_k w (-g_cos sin a + g_sin cos a)
    g_vb_d  =          sum_k m_k w (-(4^k / 2)) (g_cos cos a + g_sin sin a)
    g_dir_j = g_pm_j mu_diff
              + [diagonal variance] 2 d_j (st - sr / S) g_vb_j + d_j (2 sr / S^2) sum_d g_vb_d d_d^2
    d_origs = sum_s g_pm,   d_dirs = sum_s (tq g_pm + g_dir)

Per-sample quantities (tq, pos, mu_diff, pm, st, sr, S, vb, and the argument a) are formed in fp32,
one rounding per operation, in the order of load_pos_dir / ipe_sample (csrc/encode_common.h), and
promoted to fp64: the gradient is ill-conditioned in them (one ulp of a 1e5 argument is 0.008 rad),
and the kernel, not the rounding of its inputs, is what is measured.  The one operation that cannot
be mirrored is td^4 = powf(td, 4), restated as td2 * td2.  exact=True forms all of them in fp64, for
the comparison with fp64 autograd of the oracle.

Bound.  bound = sum_i eps_i |T_i| + floor, |T_i| = term i with |sin| = |cos| = 1 (the own-coordinate
variance term split into its st and its sr / S piece, the cross term into one piece per coordinate).
eps_i = 2e-7 (the shared sin / cos, test_gpu_sincos_range.py's figure)
      + n_ops 2^-24 (the fp32 operations on the term's path, counted below per kernel)
      + [kind 1] (2 + N_VB x_i) 2^-23, x_i = vb_d 4^k / 2 (two ulps of expf; vb's own difference
        carried through the exponential)
      + [terms that carry st or sr as a factor] N_ST 2^-23.
floor = 2^-125 times the term's factors other than w and g: a product below 2^-126 (w underflows from
x = 87 on) may be flushed to zero.

N_VB = 9 ulps.  The kernel and this file run the same correctly rounded fp32 operations on the same
values except td^4: powf is within 1 ulp of td^4, td2 * td2 within 1.5 (td2's half ulp doubled, the
product's half), so the two td4 differ by up to 2.5 ulps; each of the at most 6 fp32 operations from
td4 to vb (ipe_sample: the product with (12 tm2 - td2), the division, the subtraction from td2 / 3,
the sigma term's addition, st * d2 or the division by 3, the final addition; as many on sr's side)
rounds a slightly different value and can add one more: 8.5, rounded up.  N_ST = 7: the same up to
st / sr (4 operations after td4).

n_ops, in units of 2^-24 (one fp32 rounding), counted from csrc/encode.hip:

nerf_encode_bwd (fourier_grad): a term is ((-(g m) sin) + (g m) cos) s: g m, the product with sin or
  cos, the addition of the pair, the product with s: 4.  The coordinate's sum is accumulated in fp32,
  L terms on g_id: (L + 1) more on every term and on g_id.

nerf_encode_bwd_integrated (ipe_grad): g m, the product with sin / cos, the pair's addition, w, s: 5,
  + (L + 1) for apm's accumulation: dx.  g_vb: g m, the trig product, the pair's addition, w (the
  product with -(4^k / 2) is exact): 4, + (L + 1).  ddir: position term 5 + (L + 1) + 1 (mu_diff) + 2
  (the two additions that assemble gdd[j]); own-coordinate st piece 4 + (L + 1) + 1 (the subtraction
  st - sr / S) + 2 (the products with g_vb and with 2 d_j) + 2; its sr / S piece one more (the
  division); cross 4 + (L + 1) + 2 (d_d^2, its product with g_vb) + 2 (the sum over d) + 3 (S S, the
  division, the product) + 1 (d_j) + 2.

nerf_encode_bwd_rays: per column, g m, the trig product, w, s: 4 (d_origs; an identity column: 0).
  d_dirs: + 1 for tq cpos, + 1 for cpos mu_diff (each rounded, then added in fp64): 5 (identity
  columns 1).  cvb: g m, trig, w: 3; own-coordinate st piece 3 + 1 (subtraction) + 2 (products): 6,
  sr / S piece 7; cross 3 + 2 (d^2, product) + 3 (S S, division, product): 8.  The accumulation, the
  wave reduction and cross d_j are fp64 (1e-16, not counted); the result is rounded to fp32 once:
  2^-24 |ref|.

A ratio err / bound above 1 on the device is a finding: a bug, or a rounding this count missed."""
import math
from dataclasses import dataclass

import numpy as np
import torch

from oracle import nerf_oracle as O

U = 2.0 ** -24          # one fp32 rounding
SINCOS = 2e-7
N_VB = 9
N_ST = 7
FLOOR = 2.0 ** -125


@dataclass(frozen=True)
class Case:
    name: str
    kind: int
    levels: int
    identity: bool
    n_rays: int = 1          # rays (ray mode) or samples (per-sample kernels)
    samples: int = 1
    query: int = 1
    scale: float = 1.0
    alpha: float | None = None        # BARF mask (oracle.barf_mask), None: no mask
    sigma: float = 0.0
    distribute: bool = False
    pw_mode: int = 0
    t_end_null: bool = False
    wide: bool = True                 # pixel widths in [0.02, 0.3]; False: 1 / 555
    seed: int = 0

    @property
    def out_dim(self):
        return 3 * (2 * self.levels + int(self.identity))

    def mask(self):
        return None if self.alpha is None else O.barf_mask(self.alpha, self.levels).tolist()

    def sigma32(self):
        return float(np.float32(self.sigma))


def _levels_identity():
    return [(1, True), (1, False), (10, True), (10, False), (11, True), (11, False), (16, True), (16, False),
            (0, True)]


# nerf_encode_bwd_rays.  Rays {1, 3, 4, 5, 9} (last block with 1, 3, 0, 1, 1 live waves), samples {1, 2, 65}.
RAY_CASES = [
    Case("k0_L1_id_q1", 0, 1, True, 1, 1, query=1, seed=1),
    Case("k0_L1_q0", 0, 1, False, 3, 2, query=0, scale=2 * math.pi, seed=2),
    Case("k0_L10_id_mask", 0, 10, True, 4, 65, query=1, alpha=6.4, seed=3),
    Case("k0_L10_q0_null", 0, 10, False, 5, 2, query=0, t_end_null=True, seed=4),
    Case("k0_L11_id_q0", 0, 11, True, 9, 65, query=0, seed=5),
    Case("k0_L11_mask", 0, 11, False, 5, 1, query=1, alpha=7.3, scale=2 * math.pi, seed=6),
    Case("k0_L16_id_mask", 0, 16, True, 3, 65, query=1, alpha=12.3, scale=2 * math.pi, seed=7),
    Case("k0_L16", 0, 16, False, 9, 2, query=1, seed=8),
    Case("k0_L0_id_q0_null", 0, 0, True, 5, 2, query=0, t_end_null=True, seed=9),
    Case("k1_diag_s0_L10_id_pw0", 1, 10, True, 9, 2, pw_mode=0, seed=11),
    Case("k1_diag_s07_L16_pw1", 1, 16, False, 9, 65, sigma=0.7, pw_mode=1, seed=12),
    Case("k1_dist_s0_L11_id_pw2", 1, 11, True, 5, 2, distribute=True, pw_mode=2, seed=13),
    Case("k1_dist_s07_L1_pw0", 1, 1, False, 4, 1, distribute=True, sigma=0.7, pw_mode=0, seed=14),
    Case("k1_diag_s07_L11_mask_pw2", 1, 11, False, 9, 2, sigma=0.7, alpha=3.5, pw_mode=2, seed=15),
    Case("k1_diag_s0_L16_id_pw1", 1, 16, True, 9, 2, pw_mode=1, seed=16),
    Case("k1_diag_s0_L10_id_narrow", 1, 10, True, 3, 65, wide=False, pw_mode=0, seed=17),
    Case("k1_diag_s0_L0_id", 1, 0, True, 1, 2, pw_mode=0, seed=18),
    Case("k1_diag_s07_L1_id_S1", 1, 1, True, 9, 1, sigma=0.7, pw_mode=0, seed=19),
    Case("k1_diag_s0_L10_pw2_twopi", 1, 10, False, 9, 2, scale=2 * math.pi, pw_mode=2, seed=20),
    Case("k1_dist_s07_L10_id_mask_pw1", 1, 10, True, 3, 2, distribute=True, sigma=0.7, alpha=5.5, pw_mode=1, seed=21),
    Case("k1_diag_s07_L10_id_pw0", 1, 10, True, 9, 2, sigma=0.7, pw_mode=0, seed=22),
    Case("k1_diag_s07_L11_id_S65_pw2", 1, 11, True, 9, 65, sigma=0.7, pw_mode=2, seed=23),
    Case("k1_diag_s0_L1_pw1", 1, 1, False, 9, 2, pw_mode=1, seed=24),
    Case("k1_diag_s07_L16_id_mask_pw0", 1, 16, True, 9, 2, sigma=0.7, alpha=9.6, pw_mode=0, seed=25),
]

# nerf_encode_bwd_integrated: the level / identity set, the four variance forms in turn, sample counts
# around the 256-thread block.
_VAR = [(False, 0.0), (False, 0.7), (True, 0.0), (True, 0.7)]
INTEGRATED_CASES = [
    Case(f"L{L}_{'id' if ident else 'noid'}_{'dist' if _VAR[i % 4][0] else 'diag'}_s{_VAR[i % 4][1]:g}_n{n}", 1, L,
         ident, n, 1, distribute=_VAR[i % 4][0], sigma=_VAR[i % 4][1], pw_mode=2, seed=40 + i,
         alpha=4.4 if i == 5 else None)
    for i, ((L, ident), n) in enumerate(zip(_levels_identity(), [257, 1, 256, 255, 257, 256, 255, 257, 1]))
]

# nerf_encode_bwd: 3 n threads straddle a 256-thread block at n = 85 / 86.
FOURIER_CASES = [
    Case("L0_id_n86", 0, 0, True, 86, 1, seed=60),
    Case("L1_id_n1", 0, 1, True, 1, 1, scale=2 * math.pi, seed=61),
    Case("L1_noid_n85", 0, 1, False, 85, 1, alpha=0.4, seed=62),
    Case("L11_id_mask_n86", 0, 11, True, 86, 1, alpha=7.3, scale=2 * math.pi, seed=63),
    Case("L11_noid_n85", 0, 11, False, 85, 1, seed=64),
]


def by_name(cases):
    return {c.name: c for c in cases}


def expand_pw(pw, mode, n_rays, samples):
    """The per-sample pixel width [n_rays * samples] the header's pw_mode addresses: 0 pw[ray],
    1 pw[n % n_rays], 2 pw[n]."""
    n = torch.arange(n_rays * samples)
    if mode == 0:
        return pw[n // samples]
    if mode == 1:
        return pw[n % n_rays]
    return pw[n]


def _directions(rng, n):
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d *= rng.uniform(0.3, 3.0, (n, 1))
    d[0] = [0.0, 0.0, -1.7]                    # axis-aligned
    if n > 1:
        d[1, 1] = 0.0                          # one zero component
    return d


def ray_inputs(c: Case):
    """fp32 CPU inputs of a ray-mode case: origins in [-1, 1]^3, |d| in [0.3, 3] (ray 0 axis-aligned,
    ray 1 with a zero component), contiguous intervals over t in [2, 6.25] with one empty interval
    (t_end == t_start), pixel widths in [0.02, 0.3] or 1 / 555, a seeded normal grad_out."""
    rng = np.random.RandomState(1000 + c.seed)
    B, S = c.n_rays, c.samples
    o = rng.uniform(-1, 1, (B, 3))
    d = _directions(rng, B)
    edges = np.sort(rng.uniform(0, 1, (B, S)), axis=1) * 4.25 + 2.0
    t0 = edges
    t1 = np.concatenate((edges[:, 1:], np.full((B, 1), 6.25)), axis=1)
    t0 = t0.astype(np.float32)
    t1 = t1.astype(np.float32)
    t1[B // 2, S // 2] = t0[B // 2, S // 2]
    n_pw = B * S if c.pw_mode == 2 else B
    pw = rng.uniform(0.02, 0.3, n_pw) if c.wide else np.full(n_pw, 1 / 555.0)
    g = rng.normal(size=(B * S, c.out_dim))
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return {"o": f(o), "d": f(d), "t0": f(t0), "t1": f(t1), "pw": f(pw), "g": f(g)}


def sample_inputs(c: Case):
    """fp32 CPU inputs of a per-sample case: positions in [-6, 6]^3, and for kind 1 the directions,
    intervals and pixel widths of ray_inputs, one per sample."""
    rng = np.random.RandomState(2000 + c.seed)
    n = c.n_rays
    x = rng.uniform(-6, 6, (n, 3))
    d = _directions(rng, n)
    t0 = rng.uniform(2.0, 6.0, n).astype(np.float32)
    t1 = (t0 + rng.uniform(0.01, 1.0, n)).astype(np.float32)
    t1[n // 2] = t0[n // 2]
    pw = rng.uniform(0.02, 0.3, n)
    g = rng.normal(size=(n, c.out_dim))
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return {"x": f(x), "d": f(d), "t0": f(t0), "t1": f(t1), "pw": f(pw), "g": f(g)}


# ------------------------------------------------------------------------- per-sample quantities
def _ipe(c: Case, pos, dv, t0, t1, pw, dt):
    """ipe_sample (csrc/encode_common.h) in dtype dt, one rounding per operation, its order."""
    k = lambda v: torch.tensor(v, dtype=dt)
    t0, t1, pw = t0.unsqueeze(1), t1.unsqueeze(1), pw.unsqueeze(1)
    tm = (t0 + t1) / k(2.0)
    td = (t1 - t0) / k(2.0)
    tm2, td2 = tm * tm, td * td
    td4 = td2 * td2
    q3 = (k(3.0) * tm2) + td2
    mu = ((k(2.0) * tm) * td2) / q3
    pm = pos + mu * dv
    r_dot = (pw * k(2.0)) / k(3.4641016151377544)
    st = (td2 / k(3.0)) - (((k(4.0) * td4) * ((k(12.0) * tm2) - td2)) / (k(15.0) * (q3 * q3)))
    sr = (r_dot * r_dot) * (((tm2 / k(4.0)) + ((k(5.0) * td2) / k(12.0))) - ((k(4.0) * td4) / (k(15.0) * q3)))
    if np.float32(c.sigma) > np.float32(0.25):
        as_ = (k(c.sigma32()) * pw) * tm
        add = as_ * as_
        st = st + add
        sr = sr + add
    d2 = dv * dv
    S = ((d2[:, 0] + d2[:, 1]) + d2[:, 2]).unsqueeze(1)
    if c.distribute:
        vb = ((st + sr * k(2.0)) / k(3.0)).expand(-1, 3)
    else:
        vb = (st * d2) + (sr * (k(1.0) - (d2 / S)))
    return {"mu": mu, "pm": pm, "st": st, "sr": sr, "S": S, "vb": vb}


def _scales(c: Case, dt):
    return (torch.tensor(c.scale, dtype=torch.float32) * 2.0 ** torch.arange(c.levels, dtype=torch.float32)).to(dt)


class Terms:
    """The gradient's terms of N samples in fp64 from the per-sample quantities q (dtype dt: the
    argument a = pm s is formed in dt too).  gpm, gvb [N, 3]; Apos, Avb [N, 3, L] = |T| of the
    position / variance terms with w in; Kpos, Kvb = the same without w and g (the underflow floor);
    x [N, 3, L]."""

    def __init__(self, c: Case, pm, vb, g, dt):
        N, L = pm.shape[0], c.levels
        idn = 3 if c.identity else 0
        g = g.double()
        s = _scales(c, dt)
        a = (pm.to(dt).unsqueeze(2) * s.view(1, 1, L)).double()
        s = s.double().view(1, 1, L)
        m = torch.ones(L, dtype=torch.float64) if c.alpha is None else torch.tensor(c.mask(),
                                                                                     dtype=torch.float32).double()
        m = m.view(1, 1, L)
        p4 = (4.0 ** torch.arange(L, dtype=torch.float64)).view(1, 1, L)
        if c.kind == 1:
            self.x = vb.double().unsqueeze(2) * p4 / 2
            w = torch.exp(-self.x)
        else:
            self.x = torch.zeros(N, 3, L, dtype=torch.float64)
            w = torch.ones(N, 3, L, dtype=torch.float64)
        self.g_id = g[:, :3] if idn else torch.zeros(N, 3, dtype=torch.float64)
        gc = g[:, idn:idn + 3 * L].reshape(N, 3, L)
        gs = g[:, idn + 3 * L:idn + 6 * L].reshape(N, 3, L)
        sn, cs = torch.sin(a), torch.cos(a)
        self.gpm = self.g_id + (m * s * w * (-gc * sn + gs * cs)).sum(2)
        self.gvb = (m * w * (-(p4 / 2)) * (gc * cs + gs * sn)).sum(2)
        G = m * (gc.abs() + gs.abs())
        self.Kpos, self.Kvb = s.expand(N, 3, L), (p4 / 2).expand(N, 3, L)
        self.Apos, self.Avb = s * w * G, (p4 / 2) * w * G
        self.unmasked = (m != 0).expand(N, 3, L)

    def eps(self, c: Case, n_ops, st=False):
        e = SINCOS + n_ops * U
        if c.kind == 1:
            e = e + (2 + N_VB * self.x) * 2 * U + (N_ST * 2 * U if st else 0.0)
        return e if torch.is_tensor(e) else torch.full_like(self.x, e)


@dataclass
class RayRef:
    d_o: torch.Tensor
    d_o_bound: torch.Tensor
    d_o_sum: torch.Tensor          # sum_i |T_i|
    d_d: torch.Tensor
    d_d_bound: torch.Tensor
    d_d_sum: torch.Tensor
    share_pos: torch.Tensor        # each group's share of d_d_sum, [n_rays, 3]
    share_own: torch.Tensor
    share_cross: torch.Tensor
    pm: torch.Tensor               # the (mean-shifted) position as formed, [N, 3]
    pos: torch.Tensor
    tq: torch.Tensor
    x: torch.Tensor                # vb 4^k / 2, [N, 3, L]
    unmasked: torch.Tensor


def rays_ref(c: Case, inp, exact=False) -> RayRef:
    """Reference and bound of nerf_encode_bwd_rays."""
    dt = torch.float64 if exact else torch.float32
    B, S = c.n_rays, c.samples
    o, d = inp["o"].to(dt), inp["d"].to(dt)
    t0 = inp["t0"].to(dt).reshape(-1)
    tq = t0 if c.query == 0 else (t0 + inp["t1"].to(dt).reshape(-1)) / torch.tensor(2.0, dtype=dt)
    dv = d.repeat_interleave(S, dim=0)
    pos = o.repeat_interleave(S, dim=0) + tq.unsqueeze(1) * dv
    if c.kind == 1:
        pw = expand_pw(inp["pw"], c.pw_mode, B, S).to(dt)
        q = _ipe(c, pos, dv, t0, inp["t1"].to(dt).reshape(-1), pw, dt)
        pm, vb = q["pm"], q["vb"]
    else:
        pm, vb = pos, None
    T = Terms(c, pm, vb, inp["g"], dt)
    seg = lambda v: v.reshape(B, S, *v.shape[1:]).sum(1)
    tq64, dv64 = tq.double().unsqueeze(1), dv.double()
    e4, e5 = T.eps(c, 4), T.eps(c, 5)
    d_o = seg(T.gpm)
    d_o_sum = seg(T.g_id.abs() + T.Apos.sum(2))
    d_o_bound = seg((e4 * T.Apos + FLOOR * T.Kpos).sum(2))
    lever = tq64.abs()
    g_d = tq64 * T.gpm
    if c.kind == 1:
        mu = q["mu"].double()
        g_d = g_d + mu * T.gpm
        lever = lever + mu.abs()
    pos_sum = lever * (T.g_id.abs() + T.Apos.sum(2))
    bound = lever * (U * T.g_id.abs() + (e5 * T.Apos + FLOOR * T.Kpos).sum(2))
    own_sum = torch.zeros_like(pos_sum)
    cross_sum = torch.zeros_like(pos_sum)
    if c.kind == 1 and not c.distribute:
        st, sr, Sd = q["st"].double(), q["sr"].double(), q["S"].double()
        d2 = dv64 * dv64
        g_d = g_d + 2 * dv64 * (st - sr / Sd) * T.gvb + dv64 * (2 * sr / (Sd * Sd)) * (T.gvb * d2).sum(1, keepdim=True)
        c_st, c_sr = 2 * dv64.abs() * st.abs(), 2 * dv64.abs() * (sr / Sd).abs()
        own_sum = (c_st + c_sr) * T.Avb.sum(2)
        bound = bound + c_st * (T.eps(c, 6, True) * T.Avb + FLOOR * T.Kvb).sum(2) \
            + c_sr * (T.eps(c, 7, True) * T.Avb + FLOOR * T.Kvb).sum(2)
        c_x = dv64.abs() * (2 * sr / (Sd * Sd)).abs()
        cross_sum = c_x * (d2 * T.Avb.sum(2)).sum(1, keepdim=True)
        bound = bound + c_x * (d2 * (T.eps(c, 8, True) * T.Avb + FLOOR * T.Kvb).sum(2)).sum(1, keepdim=True)
    d_d = seg(g_d)
    d_d_sum = seg(pos_sum + own_sum + cross_sum)
    share = lambda v: seg(v) / d_d_sum
    return RayRef(d_o, d_o_bound + U * d_o.abs(), d_o_sum, d_d, seg(bound) + U * d_d.abs(), d_d_sum, share(pos_sum),
                  share(own_sum), share(cross_sum), pm, pos, tq, T.x, T.unmasked)


@dataclass
class SampleRef:
    dx: torch.Tensor
    dx_bound: torch.Tensor
    dx_sum: torch.Tensor
    ddir: torch.Tensor | None = None
    ddir_bound: torch.Tensor | None = None
    ddir_sum: torch.Tensor | None = None


def integrated_ref(c: Case, x, dv, t0, t1, pw, g, exact=False) -> SampleRef:
    """Reference and bound of nerf_encode_bwd_integrated (dx, ddir [N, 3])."""
    dt = torch.float64 if exact else torch.float32
    x, dv = x.to(dt), dv.to(dt)
    q = _ipe(c, x, dv, t0.to(dt).reshape(-1), t1.to(dt).reshape(-1), pw.to(dt).reshape(-1), dt)
    T = Terms(c, q["pm"], q["vb"], g, dt)
    L1 = c.levels + 1
    dv64, mu = dv.double(), q["mu"].double()
    dx_sum = T.g_id.abs() + T.Apos.sum(2)
    dx_bound = L1 * U * T.g_id.abs() + (T.eps(c, 5 + L1) * T.Apos + FLOOR * T.Kpos).sum(2)
    ddir = mu * T.gpm
    ddir_sum = mu.abs() * dx_sum
    ddir_bound = mu.abs() * ((L1 + 3) * U * T.g_id.abs() + (T.eps(c, 8 + L1) * T.Apos + FLOOR * T.Kpos).sum(2))
    if not c.distribute:
        st, sr, Sd = q["st"].double(), q["sr"].double(), q["S"].double()
        d2 = dv64 * dv64
        ddir = ddir + 2 * dv64 * (st - sr / Sd) * T.gvb + dv64 * (2 * sr / (Sd * Sd)) * (T.gvb * d2).sum(1, keepdim=True)
        c_st, c_sr = 2 * dv64.abs() * st.abs(), 2 * dv64.abs() * (sr / Sd).abs()
        c_x = dv64.abs() * (2 * sr / (Sd * Sd)).abs()
        ddir_sum = ddir_sum + (c_st + c_sr) * T.Avb.sum(2) + c_x * (d2 * T.Avb.sum(2)).sum(1, keepdim=True)
        ddir_bound = ddir_bound + c_st * (T.eps(c, 9 + L1, True) * T.Avb + FLOOR * T.Kvb).sum(2) \
            + c_sr * (T.eps(c, 10 + L1, True) * T.Avb + FLOOR * T.Kvb).sum(2) \
            + c_x * (d2 * (T.eps(c, 14 + L1, True) * T.Avb + FLOOR * T.Kvb).sum(2)).sum(1, keepdim=True)
    return SampleRef(T.gpm, dx_bound, dx_sum, ddir, ddir_bound, ddir_sum)


def fourier_ref(c: Case, x, g, exact=False) -> SampleRef:
    """Reference and bound of nerf_encode_bwd (dx [N, 3])."""
    dt = torch.float64 if exact else torch.float32
    T = Terms(c, x.to(dt), None, g, dt)
    L1 = c.levels + 1
    dx_sum = T.g_id.abs() + T.Apos.sum(2)
    dx_bound = L1 * U * T.g_id.abs() + (T.eps(c, 4 + L1) * T.Apos + FLOOR * T.Kpos).sum(2)
    return SampleRef(T.gpm, dx_bound, dx_sum)


# ------------------------------------------------------------------ fp64 autograd of the oracle
def _oracle_encode(c: Case, pos, dirs, pw, t0, t1):
    if c.kind == 0:
        if c.alpha is None:
            pe = O.fourier_features(pos, c.levels, c.scale)
            return torch.cat((pos, pe), dim=1) if c.identity else pe
        return O.barf_pe(pos, c.levels, c.alpha, c.identity, c.scale)
    mask = None if c.alpha is None else O.barf_mask(c.alpha, c.levels).double()
    return O.integrated_pe(pos, dirs, pw.view(-1, 1), t0.view(-1, 1), t1.view(-1, 1), c.levels, c.scale, c.identity,
                           c.distribute, c.sigma32(), mask)


def rays_autograd(c: Case, inp):
    """(d_origs, d_dirs) by fp64 autograd of the oracle's encoding over compute_positions."""
    o = inp["o"].double().requires_grad_(True)
    d = inp["d"].double().requires_grad_(True)
    t0, t1 = inp["t0"].double(), inp["t1"].double()
    pos, dirs = O.compute_positions(o, d, t0, t1, "left" if c.query == 0 else "middle")
    pw = expand_pw(inp["pw"], c.pw_mode, c.n_rays, c.samples).double()
    pe = _oracle_encode(c, pos.reshape(-1, 3), dirs.reshape(-1, 3), pw, t0.reshape(-1), t1.reshape(-1))
    (pe * inp["g"].double()).sum().backward()
    return o.grad, d.grad


def samples_autograd(c: Case, inp):
    """(dx, ddir) by fp64 autograd of the oracle's encoding of explicit positions."""
    x = inp["x"].double().requires_grad_(True)
    d = inp["d"].double().requires_grad_(True)
    pe = _oracle_encode(c, x, d, inp["pw"].double(), inp["t0"].double(), inp["t1"].double())
    (pe * inp["g"].double()).sum().backward()
    return x.grad, (d.grad if d.grad is not None else torch.zeros_like(x))
