"""fp64 references, fp32 restatements and input rows for the proposal-sampler kernels
(csrc/propnet.hip: nerf_prop_cdf / nerf_prop_sample / nerf_prop_loss).  The references evaluate
oracle/nerfacc_oracle.py's formulas in float64 on the fp32 inputs the kernels get; comparisons of
fp32 values (bucket searches) are exact either way.  Shared by tests/test_adam_prop_logic.py (CPU)
and tests/test_gpu_prop_edges.py."""
import numpy as np
import torch

from oracle import nerf_oracle as O
from oracle import nerfacc_oracle as NO

U = 2.0 ** -24
S_BAR_ULPS = 8.0                   # |s - ref| <= 8u max(|v_b|, |v_b+1|)
NEAR, FAR = 2.0, 7.0
TRANSFORMS = ("uniform", "lindisp")
PATTERNS = 5                       # every row builder below knows five kinds of row


def _rng(*key):
    return np.random.default_rng([17, *key])


# ----------------------------------------------------------------------------- cdf
CDF_K = (1, 2, 63, 64, 65, 128, 129, 511)
CDF_R = (1, 3, 4, 5)


def cdf_weights(K, R, shift):
    """[R, K] fp32 weights, row i of kind (i + shift) % 5: 0.5 then 2^-26 each (a running fp32 sum
    drops them); all zero; all mass in the last bin; magnitudes 0.5 down to 1e-30; random."""
    rng = _rng(1, K, R, shift)
    w = np.zeros((R, K), np.float64)
    for i in range(R):
        kind = (i + shift) % PATTERNS
        if kind == 0:
            w[i] = 2.0 ** -26
            w[i, 0] = 0.5
        elif kind == 2:
            w[i, K - 1] = 1.0
        elif kind == 3:
            row = 10.0 ** np.linspace(np.log10(0.5), -30.0, K)
            w[i] = row / max(1.0, row.sum() * 1.001)
        elif kind == 4:
            row = rng.random(K) ** 3
            w[i] = row / (row.sum() * 1.3 + 1e-6)
    return w.astype(np.float32)


def cdf_ref64(w):
    """[R, K] fp32 -> [R, K+1] float64: 0, exclusive fp64 sums, 1."""
    w = np.asarray(w, np.float32).astype(np.float64)
    R = w.shape[0]
    return np.concatenate([np.zeros((R, 1)), np.cumsum(w, axis=1)[:, :-1], np.ones((R, 1))], axis=1)


# ----------------------------------------------------------------------------- sample
SAMPLE_EDGES = [(E, Q) for E in (2, 65, 512) for Q in (2, 64, 65, 512)]      # (K + 1, n + 1)
SAMPLE_R = (1, 5)
STRATIFIED = dict(E=65, Q=512, R=5, seed=0x1234ABCD5678, counter=3)


def sorted_edges(rng, R, K):
    """[R, K+1] increasing fp32 edges over [0, 1], no two closer than 0.2 / K."""
    v = (np.arange(K + 1)[None, :] + rng.uniform(-0.4, 0.4, (R, K + 1))) / K
    v[:, 0], v[:, -1] = 0.0, 1.0
    return v.astype(np.float32)


def sample_rows(K, R, shift):
    """(vals, cdf) [R, K+1] fp32, row i's cdf of kind (i + shift) % 5: random with a flat stretch;
    no mass (0 .. 0 1); a single-bin jump; edges at j / K exactly (quantiles land on them); random."""
    rng = _rng(2, K, R, shift)
    vals = sorted_edges(rng, R, K)
    cdf = np.zeros((R, K + 1), np.float32)
    for i in range(R):
        kind = (i + shift) % PATTERNS
        if kind in (0, 4):
            w = rng.random(K) ** 3
            if kind == 0:
                w[K // 3:K // 2] = 0.0
            w = (w / (w.sum() * 1.3 + 1e-6)).astype(np.float32)
            cdf[i] = cdf_ref64(w[None])[0].astype(np.float32)
        elif kind == 2:
            cdf[i, K // 2 + 1:] = 1.0
        elif kind == 3:
            cdf[i] = np.arange(K + 1, dtype=np.float32) / np.float32(K)
        cdf[i, K] = 1.0
    return vals, cdf


def stratified_rows():
    """The stratified set's (vals, cdf): sample_rows with the last ray a copy of the first, so only
    the random stream tells the two apart."""
    vals, cdf = sample_rows(STRATIFIED["E"] - 1, STRATIFIED["R"], 0)
    vals[-1], cdf[-1] = vals[0], cdf[0]
    return vals, cdf


def quantiles(R, n, stratified=False, seed=0, counter=0):
    """u [R, n+1] fp32 as the kernel forms it: 0, 1 and i / n, or ((i - 1/2) + U) / n with U the
    Philox stream's element r (n + 1) + i."""
    i = np.arange(n + 1, dtype=np.float32)
    if stratified:
        idx = np.arange(R, dtype=np.uint64)[:, None] * np.uint64(n + 1) + np.arange(n + 1, dtype=np.uint64)[None, :]
        rnd = O.philox_uniform(seed, counter, idx).astype(np.float32)
        u = ((i[None, :] - np.float32(0.5)) + rnd) / np.float32(n)
    else:
        u = np.broadcast_to(i / np.float32(n), (R, n + 1)).copy()
    u[:, 0], u[:, n] = 0.0, 1.0
    assert u.dtype == np.float32
    return u


def _t(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def sample_ref64(vals, cdf, u, transform):
    """(s, t, s_bar) float64: NO.invert_cdf / NO.stot in fp64 on the fp32 inputs; s_bar = 8u times the
    larger edge of the bucket the (exact) search chooses."""
    K = vals.shape[1] - 1
    v, c, q = _t(vals, torch.float64), _t(cdf, torch.float64), _t(u, torch.float64)
    s = NO.invert_cdf(v, c, q)
    b = (torch.searchsorted(c, q, right=True) - 1).clamp(0, K - 1)
    bar = S_BAR_ULPS * U * torch.maximum(v.gather(1, b).abs(), v.gather(1, b + 1).abs())
    return s.numpy(), NO.stot(s, transform, NEAR, FAR).numpy(), bar.numpy()


def sample_fp32(vals, cdf, u):
    """The same inversion operation by operation in fp32 (torch CPU: no fused multiply-add)."""
    return NO.invert_cdf(_t(vals, torch.float32), _t(cdf, torch.float32), _t(u, torch.float32)).numpy()


# ----------------------------------------------------------------------------- loss
LOSS_SHAPES = [(1, 1), (1, 511), (511, 1), (511, 511), (64, 65)]              # (n, K)
LOSS_R = (1, 5)
LOSS_EPS = 1e-7


def loss_rows(n, K, R, shift):
    """(q_vals, q_cdf [R, n+1], k_vals, k_cdf [R, K+1]) fp32; the keys carry half the queries' mass so
    most intervals are penalised.  Row i of kind (i + shift) % 5: every query interval inside one key
    interval; one query interval covering every key (the others outside the keys' range); query
    edges exactly on key edges; query weights with zeros; random."""
    rng = _rng(3, n, K, R, shift)
    kv = sorted_edges(rng, R, K)
    qv = sorted_edges(rng, R, n)
    kw = rng.random((R, K)) ** 2 + 0.05
    qw = rng.random((R, n)) ** 2 + 0.05
    for i in range(R):
        kind = (i + shift) % PATTERNS
        if kind == 0:
            c = K // 2
            lo, hi = float(kv[i, c]), float(kv[i, c + 1])
            qv[i] = (lo + (hi - lo) * np.linspace(0.1, 0.9, n + 1)).astype(np.float32)
            kw[i, c] *= 0.01
        elif kind == 1:
            j0 = n // 2
            qv[i] = np.concatenate([np.linspace(-0.3, -0.01, j0 + 1), np.linspace(1.01, 1.3, n - j0)])
        elif kind == 2:
            take = min(n + 1, K + 1)
            on = kv[i, np.sort(rng.choice(K + 1, take, replace=False))]
            qv[i] = np.sort(np.concatenate([on, rng.random(n + 1 - take).astype(np.float32)]))
        elif kind == 3:
            qw[i, rng.random(n) < 0.5] = 0.0
            qw[i, n // 3:n // 2 + 1] = 0.0
    kw = (kw / kw.sum(axis=1, keepdims=True) * 0.5).astype(np.float32)
    qw = (qw / (qw.sum(axis=1, keepdims=True) * 1.01 + 1e-9)).astype(np.float32)
    assert np.all(np.diff(qv, axis=1) >= 0) and np.all(np.diff(kv, axis=1) > 0)
    return qv, cdf_ref64(qw).astype(np.float32), kv, cdf_ref64(kw).astype(np.float32)


def loss_ref64(qv, qc, kv, kc, grad_scale):
    """(loss_ray [R], grad_k_w [R, K]) float64: NO.pdf_loss in fp64 on the fp32 inputs; the gradient
    from autograd with respect to the given key cdf (a leaf: the kinks stay where the fp32 cdf puts
    them), dkw[j] = sum_{i=j+1}^{K-1} dkc[i]."""
    K = kv.shape[1] - 1
    gs = float(np.float32(grad_scale))
    leaf = _t(kc, torch.float64).requires_grad_(True)
    per = NO.pdf_loss(_t(qv, torch.float64), _t(qc, torch.float64), _t(kv, torch.float64), leaf,
                      float(np.float32(LOSS_EPS)))
    (per.sum() * gs).backward()
    dkc = leaf.grad.numpy()
    dkw = np.zeros((kv.shape[0], K))
    for j in range(K):
        dkw[:, j] = dkc[:, j + 1:K].sum(axis=1)
    return per.detach().sum(dim=1).numpy(), dkw


def loss_fp32(qv, qc, kv, kc, grad_scale):
    """The kernel's arithmetic restated: per interval in fp32, operation by operation; the sums over
    intervals in fp64, as the kernel's are."""
    R, K = kv.shape[0], kv.shape[1] - 1
    eps, gs = np.float32(LOSS_EPS), np.float32(grad_scale)
    loss, dkw = np.zeros(R), np.zeros((R, K))
    for r in range(R):
        cnt = np.searchsorted(kv[r], qv[r], side="right")
        right = np.minimum(cnt[1:], K)
        left = np.clip(cnt[:-1] - 1, 0, K)
        w = qc[r, 1:] - qc[r, :-1]
        wo = kc[r][right] - kc[r][left]
        d = np.maximum(w - wo, np.float32(0))
        den = w + eps
        assert d.dtype == np.float32 and den.dtype == np.float32
        loss[r] = ((d * d) / den).astype(np.float64).sum()
        cj = (-(np.float32(2) * d / den) * gs).astype(np.float64)
        dcdf = np.zeros(K + 1)
        np.add.at(dcdf, right, cj)
        np.add.at(dcdf, left, -cj)
        for j in range(K):
            dkw[r, j] = dcdf[j + 1:K].sum()
    return loss, dkw


def loss_bars(loss_ref, dkw_ref):
    """(per-ray loss bar [R], gradient bar [R, 1]): 1e-5 relative + 1e-12; 1e-5 of the row's largest
    reference magnitude."""
    return 1e-5 * np.abs(loss_ref) + 1e-12, 1e-5 * np.abs(dkw_ref).max(axis=1, keepdims=True)
