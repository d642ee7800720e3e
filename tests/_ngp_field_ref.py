"""Restatements of the NGP radiance field's per-sample pieces that the tests and tools/ngp_field_bench.py
run against (test infrastructure only; no kernels):

* ``sh32`` / ``unit_cube32`` — numpy fp32, the two numbered contracts of include/nerf_amd.h operation by
  operation, each rounded alone; ``sh64`` / ``unit_cube64`` — the same formulas in fp64.
* ``sh_jac64`` / ``unit_cube_jac64`` — the hand-derived Jacobians in fp64; ``sh_bwd64`` /
  ``unit_cube_bwd64`` — their products with an output gradient.
* ``sh_torch`` / ``unit_cube_torch`` — the eager torch forms (any dtype, differentiable), in the
  contracts' operation order.
* ``sphere_quadrature`` — Gauss-Legendre x uniform-phi nodes and weights on the unit sphere.
* ``field_points`` — the seeded points of the distance measurement: a third inside the box, a third
  with 1 < m < 4, the rest with m up to 1e6.
* ``ref_field`` — NGPRadianceField.forward in eager torch from the module's state_dict (hash grid:
  oracle/hashgrid_oracle.py's rows, torch weights added corner by corner in the oracle's order).
* ``field_bounds`` — first-order forward-error bounds, per element, of one run of the field at
  per-product error eps, by the method of tests/test_gpu_ingp2d.py::_bounds.
"""
from __future__ import annotations

import math

import numpy as np
import torch as th

from oracle import hashgrid_oracle as O

C = (0.28209479177387814, 0.48860251190291987, 1.0925484305920792, 0.94617469575755997, 0.31539156525251999,
     0.54627421529603959, 0.59004358992664352, 2.8906114426405538, 0.45704579946446572, 0.3731763325901154,
     1.4453057213202769)


# ----------------------------------------------------------------------------- spherical harmonics
def _sh(x, y, z, degree, c, three, five, one):
    """The contract's operation order on arrays of one dtype (c: the constants in that dtype)."""
    out = [np.full_like(x, c[0])]
    if degree >= 2:
        out += [(-c[1]) * y, c[1] * z, (-c[1]) * x]
    if degree >= 3:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        out += [c[2] * xy, (-c[2]) * yz, c[3] * zz - c[4], (-c[2]) * xz, c[5] * (xx - yy)]
    if degree >= 4:
        w = one - five * zz
        out += [(c[6] * y) * ((-three) * xx + yy), (c[7] * xy) * z, (c[8] * y) * w, (c[9] * z) * (five * zz - three),
                (c[8] * x) * w, (c[10] * z) * (xx - yy), (c[6] * x) * ((-xx) + three * yy)]
    return np.stack(out, axis=1)


def sh32(d: np.ndarray, degree: int = 4) -> np.ndarray:
    d = d.astype(np.float32)
    f = np.float32
    return _sh(d[:, 0], d[:, 1], d[:, 2], degree, [f(v) for v in C], f(3), f(5), f(1))


def sh64(d: np.ndarray, degree: int = 4) -> np.ndarray:
    d = d.astype(np.float64)
    return _sh(d[:, 0], d[:, 1], d[:, 2], degree, C, 3.0, 5.0, 1.0)


def sh_jac64(d: np.ndarray, degree: int = 4) -> np.ndarray:
    """[N, degree^2, 3]: dY_c / dd_a of the polynomials, by hand."""
    d = d.astype(np.float64)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    J = np.zeros((d.shape[0], 16, 3))
    c = C
    J[:, 1, 1], J[:, 2, 2], J[:, 3, 0] = -c[1], c[1], -c[1]
    J[:, 4, 0], J[:, 4, 1] = c[2] * y, c[2] * x
    J[:, 5, 1], J[:, 5, 2] = -c[2] * z, -c[2] * y
    J[:, 6, 2] = 2 * c[3] * z
    J[:, 7, 0], J[:, 7, 2] = -c[2] * z, -c[2] * x
    J[:, 8, 0], J[:, 8, 1] = 2 * c[5] * x, -2 * c[5] * y
    J[:, 9, 0], J[:, 9, 1] = -6 * c[6] * x * y, 3 * c[6] * (y * y - x * x)
    J[:, 10, 0], J[:, 10, 1], J[:, 10, 2] = c[7] * y * z, c[7] * x * z, c[7] * x * y
    J[:, 11, 1], J[:, 11, 2] = c[8] * (1 - 5 * z * z), -10 * c[8] * y * z
    J[:, 12, 2] = c[9] * (15 * z * z - 3)
    J[:, 13, 0], J[:, 13, 2] = c[8] * (1 - 5 * z * z), -10 * c[8] * x * z
    J[:, 14, 0], J[:, 14, 1], J[:, 14, 2] = 2 * c[10] * x * z, -2 * c[10] * y * z, c[10] * (x * x - y * y)
    J[:, 15, 0], J[:, 15, 1] = 3 * c[6] * (y * y - x * x), 6 * c[6] * x * y
    return J[:, :degree * degree]


def sh_bwd64(d: np.ndarray, g: np.ndarray, degree: int = 4) -> np.ndarray:
    return np.einsum("nc,nca->na", g[:, :degree * degree].astype(np.float64), sh_jac64(d, degree))


def sh_torch(d: th.Tensor, degree: int = 4) -> th.Tensor:
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    c = C
    out = [th.full_like(x, c[0])]
    if degree >= 2:
        out += [(-c[1]) * y, c[1] * z, (-c[1]) * x]
    if degree >= 3:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        out += [c[2] * xy, (-c[2]) * yz, c[3] * zz - c[4], (-c[2]) * xz, c[5] * (xx - yy)]
    if degree >= 4:
        w = 1 - 5 * zz
        out += [(c[6] * y) * (-3 * xx + yy), (c[7] * xy) * z, (c[8] * y) * w, (c[9] * z) * (5 * zz - 3),
                (c[8] * x) * w, (c[10] * z) * (xx - yy), (c[6] * x) * (-xx + 3 * yy)]
    return th.stack(out, dim=1)


def sphere_quadrature(n_theta: int = 24, n_phi: int = 48):
    """(directions [n, 3], weights [n]) integrating polynomials of degree < min(2 n_theta, n_phi) exactly;
    the weights sum to 4 pi."""
    mu, wm = np.polynomial.legendre.leggauss(n_theta)
    phi = 2 * np.pi * np.arange(n_phi) / n_phi
    s = np.sqrt(1 - mu ** 2)
    d = np.stack([np.outer(s, np.cos(phi)), np.outer(s, np.sin(phi)), np.outer(mu, np.ones(n_phi))], axis=-1)
    w = np.outer(wm, np.full(n_phi, 2 * np.pi / n_phi))
    return d.reshape(-1, 3), w.reshape(-1)


# ----------------------------------------------------------------------------- position map
def _unit_cube(x, aabb, mode, f):
    lo, hi = aabb[:3], aabb[3:]
    e = hi - lo
    v = (x - lo) / e
    if mode == 0:
        u = v
    else:
        c = v * f(2) - f(1)
        with np.errstate(invalid="ignore"):
            m = np.fmax(np.fmax(np.abs(c[:, 0]), np.abs(c[:, 1])), np.abs(c[:, 2]))[:, None]
            far = m > f(1)
            ms = np.where(far, m, f(1))
            s = f(2) - f(1) / ms
            c = np.where(far, s * (c / ms), c)
        u = c / f(4) + f(0.5)
    with np.errstate(invalid="ignore"):
        inside = ((u > 0) & (u < 1)).all(axis=1)
    return u, inside.astype(x.dtype)


def unit_cube32(x: np.ndarray, aabb, mode: int):
    """(u [N, 3], inside [N]) in fp32, each operation rounded alone."""
    return _unit_cube(x.astype(np.float32), np.asarray(aabb, dtype=np.float32), mode, np.float32)


def unit_cube64(x: np.ndarray, aabb, mode: int):
    """The same formulas in fp64 on the fp32 inputs (the box as its fp32 values)."""
    return _unit_cube(x.astype(np.float64), np.asarray(aabb, dtype=np.float32).astype(np.float64), mode, np.float64)


def contraction_m(x: np.ndarray, aabb) -> np.ndarray:
    """m = max_a |2 v_a - 1| of the contract, fp64."""
    a = np.asarray(aabb, dtype=np.float32).astype(np.float64)
    c = (x.astype(np.float64) - a[:3]) / (a[3:] - a[:3]) * 2 - 1
    return np.abs(c).max(axis=1)


def unit_cube_jac64(x: np.ndarray, aabb, mode: int) -> np.ndarray:
    """[N, 3 (j), 3 (i)]: du_j / dx_i by hand (k = the lowest index attaining m)."""
    a = np.asarray(aabb, dtype=np.float32).astype(np.float64)
    e = a[3:] - a[:3]
    n = x.shape[0]
    J = np.zeros((n, 3, 3))
    eye = np.eye(3)
    if mode == 0:
        J[:] = eye / e
        return J
    c = (x.astype(np.float64) - a[:3]) / e * 2 - 1
    m = np.abs(c).max(axis=1)
    k = np.argmax(np.abs(c) == m[:, None], axis=1)
    far = m > 1
    ms = np.where(far, m, 1.0)
    s = 2 - 1 / ms
    dy = (s / ms)[:, None, None] * eye                                     # [N, j, i]
    sg = np.sign(c[np.arange(n), k])
    dy[np.arange(n), :, k] += c * (sg * (2 - 2 * ms) / ms ** 3)[:, None]
    dy = np.where(far[:, None, None], dy, eye)
    return dy / (2 * e)[None, None, :]


def unit_cube_bwd64(x: np.ndarray, aabb, mode: int, g: np.ndarray) -> np.ndarray:
    return np.einsum("nj,nji->ni", g.astype(np.float64), unit_cube_jac64(x, aabb, mode))


def unit_cube_torch(x: th.Tensor, aabb: th.Tensor, mode: int):
    """(u, inside) in eager torch, the contract's operation order (differentiable in x)."""
    lo, hi = aabb[:3], aabb[3:]
    v = (x - lo) / (hi - lo)
    if mode == 0:
        u = v
    else:
        c = v * 2 - 1
        m = c.abs().amax(dim=1, keepdim=True)
        far = m > 1
        ms = th.where(far, m, th.ones_like(m))
        u = th.where(far, (2 - 1 / ms) * (c / ms), c) / 4 + 0.5
    inside = ((u > 0) & (u < 1)).all(dim=1).to(x.dtype)
    return u, inside


def field_points(n: int, seed: int = 0):
    """(x [n, 3] fp32, aabb [6] fp32): extents in [1, 4]; a third of the points inside the box, a third
    with 1 < m < 4, the rest with m log-uniform up to 1e6 (m = max_a |2 v_a - 1|)."""
    rng = np.random.default_rng(seed)
    lo = rng.uniform(-2, 0, 3)
    ext = rng.uniform(1, 4, 3)
    aabb = np.concatenate([lo, lo + ext]).astype(np.float32)
    c = rng.uniform(-1, 1, (n, 3))
    c /= np.abs(c).max(axis=1, keepdims=True)                               # m = 1
    third = n // 3
    m = np.concatenate([rng.uniform(0, 1, third), rng.uniform(1, 4, third),
                        10 ** rng.uniform(math.log10(4), 6, n - 2 * third)])
    c *= m[:, None]
    a = aabb.astype(np.float64)
    x = ((c + 1) / 2 * (a[3:] - a[:3]) + a[:3]).astype(np.float32)
    return x, aabb


def unit_dirs(n: int, seed: int = 1) -> np.ndarray:
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((n, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


# ----------------------------------------------------------------------------- the field in eager torch
def _corner_rows(c: th.Tensor, r: int, T: int) -> th.Tensor:
    """oracle/hashgrid_oracle.py::corner_index in torch int64 (wrapping products, non-negative remainder)."""
    if (r + 1) ** 3 <= T:
        cc = c.clamp(0, r)
        return cc[:, 0] + (r + 1) * cc[:, 1] + (r + 1) * (r + 1) * cc[:, 2]
    h = (c[:, 0] * O.PRIMES[0]) ^ (c[:, 1] * O.PRIMES[1]) ^ (c[:, 2] * O.PRIMES[2])
    return th.remainder(h, T)


def hash_features_torch(u: th.Tensor, tables, res, T: int, u32: th.Tensor | None = None) -> th.Tensor:
    """[N, L * F]: per level the eight corners' w * row added in the oracle's order from 0; rows and
    floor are constants of the fp32 u (u32: the fp32 run's own coordinates, for an fp64 u that may round
    into a neighbouring cell), the weights (1 - |x_hat - c|) products differentiable in u."""
    u32 = u.detach().to(th.float32) if u32 is None else u32
    outs = []
    for t, r in zip(tables, res):
        r = int(r)
        base32 = th.floor(u32 * r)
        base_i = base32.to(th.int64)
        base = base32.to(u.dtype)
        xh = u * r
        acc = th.zeros(u.shape[0], t.shape[1], dtype=u.dtype, device=u.device)
        for off in O.CORNERS_3D:
            o = th.tensor(off, device=u.device)
            d = 1 - th.abs(xh - (base + o.to(u.dtype)))
            acc = acc + t[_corner_rows(base_i + o, r, T)] * ((d[:, 0] * d[:, 1]) * d[:, 2]).unsqueeze(1)
        outs.append(acc)
    return th.cat(outs, dim=1)


class RefNGPField(th.nn.Module):
    """ref_field as a module holding its own copy of an NGPRadianceField's state: the eager torch path
    the fit test's step count was chosen on (any device)."""

    def __init__(self, field):
        super().__init__()
        self.cfg = field_cfg(field)
        sd = field.state_dict()
        self.names = [k for k in sd if k != "aabb"]
        self.values = th.nn.ParameterList([th.nn.Parameter(sd[k].detach().clone()) for k in self.names])
        self.register_buffer("aabb", sd["aabb"].detach().clone())

    def _sd(self):
        return {**dict(zip(self.names, self.values)), "aabb": self.aabb}

    def forward(self, positions, directions):
        return ref_field(self._sd(), self.cfg, positions, directions)

    def query_density(self, x):
        d = x.new_tensor([0.0, 0.0, 1.0]).expand(x.shape[0], 3)
        return ref_field(self._sd(), self.cfg, x, d)[1]


def field_cfg(field) -> dict:
    return dict(n_levels=field.n_levels, log2_hashmap_size=field.log2_hashmap_size, unbounded=field.unbounded,
                resolutions=list(field.position_encoding.resolutions), use_viewdirs=field.use_viewdirs)


class TruncExpRef(th.autograd.Function):
    """The definition: exp(x) forward, g * exp(clamp(x, max=15)) backward."""

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return th.exp(x)

    @staticmethod
    def backward(ctx, g):
        return g * th.exp(th.clamp(ctx.saved_tensors[0], max=15))


def ref_field(sd: dict, cfg: dict, positions: th.Tensor, directions: th.Tensor, dtype=th.float32, keep=None,
              cells=None):
    """(rgb [N, 3], density [N, 1]) of NGPRadianceField(**cfg) holding state_dict sd, in eager torch on
    the CPU in `dtype`; the parameters are taken as given (pass leaves that require grad to
    differentiate).  keep: a dict that receives the intermediate tensors.  cells: (u fp32, inside) of the
    fp32 contract, which an fp64 run takes its grid cells and selector from."""
    L = cfg["n_levels"]
    res = cfg["resolutions"]
    T = 2 ** cfg["log2_hashmap_size"]
    aabb = sd["aabb"].to(dtype)
    u, inside = unit_cube_torch(positions, aabb, 1 if cfg["unbounded"] else 0)
    tables = [sd[f"position_encoding.encodings.{l}.table"] for l in range(L)]
    if cells is not None:
        u = u + (cells[0].to(dtype) - u).detach()       # evaluated at the fp32 run's coordinates, gradient kept
        inside = cells[1].to(dtype)
    feat = hash_features_torch(u, tables, res, T, None if cells is None else cells[0])
    h = th.relu(th.nn.functional.linear(feat, sd["mlp_base.0.weight"], sd["mlp_base.0.bias"]))
    z = th.nn.functional.linear(h, sd["mlp_base.2.weight"], sd["mlp_base.2.bias"])
    dens = TruncExpRef.apply(z[:, 0] - 1) * inside
    views = cfg.get("use_viewdirs", True)
    sh = sh_torch(directions, 4) if views else z.new_zeros(z.shape[0], 0)
    a0 = th.cat([sh, z[:, 1:]], dim=1)
    h1 = th.relu(th.nn.functional.linear(a0, sd["mlp_head.0.weight"], sd["mlp_head.0.bias"]))
    h2 = th.relu(th.nn.functional.linear(h1, sd["mlp_head.2.weight"], sd["mlp_head.2.bias"]))
    head = th.nn.functional.linear(h2, sd["mlp_head.4.weight"], sd["mlp_head.4.bias"])
    rgb = th.sigmoid(head)
    if keep is not None:
        keep.update(u=u, inside=inside, feat=feat, h=h, z=z, sh=sh, a0=a0, h1=h1, h2=h2, head=head)
    return rgb, dens.unsqueeze(1)


def field_loss(rgb: th.Tensor, dens: th.Tensor, g_rgb: th.Tensor, g_dens: th.Tensor) -> th.Tensor:
    """A fixed linear functional of the outputs: every gradient path carries a known seed."""
    return ((rgb * g_rgb).sum() + (dens.reshape(-1) * g_dens).sum()) / rgb.shape[0]


def _corner_slopes(u32: np.ndarray, r: int) -> np.ndarray:
    """[N, 8, 3]: |dw_k / dx_hat_a| of the eight corners in stacking order: the product of the other two
    axes' factors (1 - |x_hat - c|)."""
    xh = u32.astype(np.float32) * np.float32(r)
    frac = (xh - np.floor(xh)).astype(np.float64)
    out = np.empty((u32.shape[0], 8, 3))
    for k, off in enumerate(O.CORNERS_3D):
        d = np.where(np.array(off) == 1, frac, 1 - frac)                    # [N, 3]
        out[:, k] = np.stack([d[:, 1] * d[:, 2], d[:, 0] * d[:, 2], d[:, 0] * d[:, 1]], axis=1)
    return out


def field_bounds(sd64: dict, cfg: dict, x: np.ndarray, dirs: np.ndarray, g_rgb: np.ndarray, g_dens: np.ndarray,
                 eps: float) -> dict:
    """First-order error bounds, **per element**, of one fp32 run of the field and of field_loss's
    gradients at per-product error eps in the GEMMs (the forward-error method of
    tests/test_gpu_ingp2d.py::_bounds carried element by element, so that a bound stays under the value
    it guards): element (n, j) of a GEMM output over K terms carries (eps + K u) sum_k |a_nk w_jk| (+ |b_j|)
    of its own plus sum_k E_nk |w_jk| of the incoming error E; ReLU is 1-Lipschitz and passes the error
    of live units only in the backward; the sigmoid's slope is rgb (1 - rgb); exp carries 6 u relative
    beside its argument's error.  A weight gradient sums N products: (eps + N u) sum_n |d a| + sum_n (E_d |a|
    + |d| E_a).  A table entry sums w d over the corners that land on it; the position gradient sums
    r d t dw/dx_hat over levels, features and corners and passes through the map's Jacobian.  The
    unit-cube coordinates, hash features and SH values are the same bits in both runs (checked by the
    caller), so they enter with error 0.  Magnitudes from the fp64 run of ref_field on sd64.
    Returns {'rgb' [N, 3], 'density' [N, 1], 'loss' scalar, 'grad': {name: array of the tensor's shape}}."""
    u = 2.0 ** -24
    N = x.shape[0]
    eff = lambda K: eps + K * u
    P = {k: v.detach().numpy() for k, v in sd64.items()}
    keep = {}
    xt = th.tensor(x.astype(np.float64), requires_grad=True)
    dt = th.tensor(dirs.astype(np.float64), requires_grad=True)
    u32, in32 = unit_cube32(x, P["aabb"], 1 if cfg["unbounded"] else 0)      # the cells both fp32 runs use
    rgb, dens = ref_field(sd64, cfg, xt, dt, th.float64, keep, cells=(th.from_numpy(u32), th.from_numpy(in32)))
    K_ = {k: v.detach().numpy() for k, v in keep.items()}
    rgb, dens = rgb.detach().numpy(), dens.detach().numpy().reshape(-1)
    n_sh = K_["sh"].shape[1]

    def fwd(a, E_a, W, b):
        return eff(W.shape[1]) * (np.abs(a) @ np.abs(W).T + np.abs(b)) + E_a @ np.abs(W).T
    E_h = fwd(K_["feat"], np.zeros_like(K_["feat"]), P["mlp_base.0.weight"], P["mlp_base.0.bias"])
    E_z = fwd(K_["h"], E_h, P["mlp_base.2.weight"], P["mlp_base.2.bias"])
    E_a0 = np.concatenate([np.zeros((N, n_sh)), E_z[:, 1:]], axis=1)
    E_h1 = fwd(K_["a0"], E_a0, P["mlp_head.0.weight"], P["mlp_head.0.bias"])
    E_h2 = fwd(K_["h1"], E_h1, P["mlp_head.2.weight"], P["mlp_head.2.bias"])
    E_head = fwd(K_["h2"], E_h2, P["mlp_head.4.weight"], P["mlp_head.4.bias"])
    slope = rgb * (1 - rgb)
    E_rgb = slope * E_head + 2 * u
    E_dens = dens * (E_z[:, 0] + 6 * u)
    out = {"rgb": E_rgb, "density": E_dens[:, None],
           "loss": ((np.abs(g_rgb) * E_rgb).sum() + (np.abs(g_dens) * E_dens).sum()
                    + 8 * u * (np.abs(rgb * g_rgb).sum() + np.abs(dens * g_dens).sum())) / N,
           "grad": {}}

    def bwd(name, d, E_d, a, E_a, W):
        """Records the layer's weight / bias bounds; returns (d W, its error) at the layer's input."""
        out["grad"][name + ".weight"] = eff(N) * (np.abs(d).T @ np.abs(a)) + E_d.T @ np.abs(a) + np.abs(d).T @ E_a
        out["grad"][name + ".bias"] = eff(N) * np.abs(d).sum(0) + E_d.sum(0)
        return d @ W, eff(W.shape[0]) * (np.abs(d) @ np.abs(W)) + E_d @ np.abs(W)

    d = g_rgb / N * slope
    E_d = np.abs(g_rgb) / N * np.abs(1 - 2 * rgb) * E_rgb + 4 * u * np.abs(d)
    d, E_d = bwd("mlp_head.4", d, E_d, K_["h2"], E_h2, P["mlp_head.4.weight"])
    live = K_["h2"] > 0
    d, E_d = bwd("mlp_head.2", d * live, E_d * live, K_["h1"], E_h1, P["mlp_head.2.weight"])
    live = K_["h1"] > 0
    d, E_d = bwd("mlp_head.0", d * live, E_d * live, K_["a0"], E_a0, P["mlp_head.0.weight"])
    d_sh, E_dsh = d[:, :n_sh], E_d[:, :n_sh]
    # the raw density's seed: g_dens / N * exp(min(z0 - 1, 15)) * inside
    raw = K_["z"][:, 0] - 1
    d_z0 = g_dens / N * np.exp(np.minimum(raw, 15)) * K_["inside"]
    E_dz0 = np.abs(d_z0) * (E_z[:, 0] + 6 * u)
    d = np.concatenate([d_z0[:, None], d[:, n_sh:]], axis=1)
    E_d = np.concatenate([E_dz0[:, None], E_d[:, n_sh:]], axis=1)
    d, E_d = bwd("mlp_base.2", d, E_d, K_["h"], E_h, P["mlp_base.2.weight"])
    live = K_["h"] > 0
    d, E_d = bwd("mlp_base.0", d * live, E_d * live, K_["feat"], np.zeros_like(K_["feat"]), P["mlp_base.0.weight"])
    T, F = 2 ** cfg["log2_hashmap_size"], 2
    A, E_u = np.zeros((N, 3)), np.zeros((N, 3))
    for l, r in enumerate(cfg["resolutions"]):
        idx, w = O.level_corners(u32, int(r), T, normalize=False)
        t = P[f"position_encoding.encodings.{l}.table"]
        dl, El = np.abs(d[:, l * F:(l + 1) * F]), E_d[:, l * F:(l + 1) * F]
        cnt = np.zeros(t.shape[0])
        np.add.at(cnt, idx.reshape(-1), 1.0)
        e_t, s_t = np.zeros_like(t), np.zeros_like(t)
        for k in range(8):
            wk = np.abs(w[:, k:k + 1]).astype(np.float64)
            np.add.at(e_t, idx[:, k], wk * El)
            np.add.at(s_t, idx[:, k], wk * dl)
        out["grad"][f"position_encoding.encodings.{l}.table"] = e_t + (cnt[:, None] + 4) * u * s_t
        # d u_a = sum_l r_l sum_f d_f sum_k t_kf dw_k/dx_hat_a (x_hat = u r)
        slopes = _corner_slopes(u32, int(r))                                # [N, 8, 3]
        ts = np.einsum("nkf,nka->nfa", np.abs(t[idx]), slopes)              # [N, F, 3]
        A += r * np.einsum("nf,nfa->na", dl, ts)
        E_u += r * np.einsum("nf,nfa->na", El, ts)
    n_terms = 8 * F * len(cfg["resolutions"])
    E_u += (n_terms + 8) * u * A
    J = np.abs(unit_cube_jac64(x, P["aabb"], 1 if cfg["unbounded"] else 0))  # [N, j, i]
    out["grad"]["positions"] = np.einsum("nj,nji->ni", E_u + 16 * u * A, J)
    Js = np.abs(sh_jac64(dirs, 4))[:, :n_sh]
    out["grad"]["directions"] = (np.einsum("nc,nca->na", E_dsh, Js)
                                 + 24 * u * np.einsum("nc,nca->na", np.abs(d_sh), Js))
    return out
