"""References and input sets for the fused Adam kernel (csrc/adam.hip, include/nerf_amd.h):

  g' = g (+ weight_decay * p);  m' = m + (1-beta1) * (g' - m);  v' = v * beta2 + ((1-beta2) * g') * g'
  p' = p + step_size * (m' / (sqrt(v') / bc2_sqrt + eps))

`adam_ref64` evaluates it in float64, `adam_ref32` operation by operation in float32 in the kernel's
order without fused multiply-add; both on the fp32 arrays and the fp32-rounded scalars the C struct
carries.  The input sets below are shared by tests/test_adam_prop_logic.py (CPU: the fp32
restatement against the bar) and tests/test_gpu_adam_edges.py (the kernel against both)."""
import numpy as np

U = 2.0 ** -24
P_REL, P_UPD = 4.0, 16.0          # the constants of the p bar (test_adam_prop_logic.py measures them)


def f32(x):
    return np.float32(x)


def adam_ref64(p, g, m, v, step_size, bc2_sqrt, weight_decay, one_minus_beta1, beta2, one_minus_beta2, eps):
    """(p', m', v', bar) in float64; bar is the elementwise bound on |p' - ref|:
    4u |ref| + 16u |step| (|m'| + |g'|) / denom + 1e-45."""
    p, g, m, v = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (p, g, m, v))
    step, bc2, wd, omb1, b2, omb2, e = (np.float64(np.float32(s)) for s in
                                        (step_size, bc2_sqrt, weight_decay, one_minus_beta1, beta2,
                                         one_minus_beta2, eps))
    with np.errstate(all="ignore"):
        gv = g + wd * p if wd != 0.0 else g
        mv = m + omb1 * (gv - m)
        vv = v * b2 + (omb2 * gv) * gv
        denom = np.sqrt(vv) / bc2 + e
        pv = p + step * (mv / denom)
        bar = P_REL * U * np.abs(pv) + P_UPD * U * np.abs(step) * (np.abs(mv) + np.abs(gv)) / denom + 1e-45
    return pv, mv, vv, bar


def adam_ref32(p, g, m, v, step_size, bc2_sqrt, weight_decay, one_minus_beta1, beta2, one_minus_beta2, eps):
    """(p', m', v') in float32: every operation of the kernel rounded once, in its order."""
    p, g, m, v = (np.asarray(a, dtype=np.float32) for a in (p, g, m, v))
    step, bc2, wd, omb1, b2, omb2, e = (np.float32(s) for s in (step_size, bc2_sqrt, weight_decay, one_minus_beta1,
                                                                beta2, one_minus_beta2, eps))
    with np.errstate(all="ignore"):
        gv = g
        if wd != np.float32(0.0):
            t = wd * p
            gv = g + t
        d = gv - m
        d = omb1 * d
        mv = m + d
        a = v * b2
        c = omb2 * gv
        c = c * gv
        vv = a + c
        s = np.sqrt(vv)
        s = s / bc2
        denom = s + e
        q = mv / denom
        q = step * q
        pv = p + q
    for a in (pv, mv, vv):
        assert a.dtype == np.float32
    return pv, mv, vv


class Case:
    """One launch's worth of inputs (or, for the chunked sets, several launches' worth): the batch
    scalars as Python floats and per tensor (p, g, m, v, step_size, bc2_sqrt, weight_decay)."""

    def __init__(self, name, beta1, beta2, eps, tensors):
        self.name, self.beta1, self.beta2, self.eps, self.tensors = name, beta1, beta2, eps, tensors

    def scalars(self):
        # as ctypes rounds what kernels.adam_step assigns: 1 - beta in double, then to fp32
        return dict(one_minus_beta1=f32(1 - self.beta1), beta2=f32(self.beta2), one_minus_beta2=f32(1 - self.beta2),
                    eps=f32(self.eps))

    def refs(self):
        """Per tensor ((p', m', v', bar) float64, (p', m', v') float32)."""
        out = []
        for p, g, m, v, step, bc2, wd in self.tensors:
            args = (p, g, m, v, step, bc2, wd)
            out.append((adam_ref64(*args, **self.scalars()), adam_ref32(*args, **self.scalars())))
        return out


def _tensor(rng, n, t, lr, beta1, beta2, wd):
    """Plausible state after t steps: g ~ N(0, 1) * 10^k, m of g's size, v of its square."""
    scale = 10.0 ** rng.integers(-3, 3)
    p = rng.standard_normal(n).astype(np.float32)
    g = (rng.standard_normal(n) * scale).astype(np.float32)
    m = (rng.standard_normal(n) * scale * 0.5).astype(np.float32)
    v = ((rng.standard_normal(n) * scale) ** 2 * rng.uniform(0.2, 1.0)).astype(np.float32)
    return (p, g, m, v, -lr / (1 - beta1 ** t), (1 - beta2 ** t) ** 0.5, wd)


def _table(name, sizes, seed, beta1=0.9, beta2=0.999, eps=1e-5):
    """Every tensor with its own step count (so its own step_size and bc2_sqrt), learning rate and
    weight decay; every third decay is zero."""
    rng = np.random.default_rng(seed)
    tensors = []
    for i, n in enumerate(sizes):
        wd = 0.0 if i % 3 == 0 else 0.01 * (1 + i % 5)
        tensors.append(_tensor(rng, n, 1 + i, 1e-3 * (1 + i % 7), beta1, beta2, wd))
    return Case(name, beta1, beta2, eps, tensors)


GEOMETRY_SIZES = [0, 1, 255, 256, 257, 2047, 2048, 2049, 0, 4096, 4097, 6145, 3, 0]
FULL_SIZES = [(1, 2048, 2049, 300)[i % 4] for i in range(48)]
CHUNK_SIZES = (1, 7, 2049, 300, 2048)


def geometry_case():
    return _table("geometry", GEOMETRY_SIZES, 101)


def full_table_case():
    return _table("full table", FULL_SIZES, 102, beta2=0.99)


def chunk_case(n_entries):
    return _table(f"{n_entries} entries", [CHUNK_SIZES[i % len(CHUNK_SIZES)] for i in range(n_entries)],
                  200 + n_entries, beta1=0.8)


VALUE_N = 4097


def value_case(eps):
    """One 4,097-element tensor: [0, 1024) g = m = v = 0; [1024, 2048) v = 0, g = 0, m != 0 (the
    denominator is eps alone); [2048, 4097) |g| log-spaced over 1e-30 .. 1e18 with random signs, m of
    g's size, v of its square (v' underflows at the small end and the denominator is eps again)."""
    rng = np.random.default_rng(103)
    n = VALUE_N
    p = rng.standard_normal(n).astype(np.float32)
    g, m, v = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)
    m[1024:2048] = (rng.standard_normal(1024) * 10.0 ** rng.integers(-6, 3, 1024)).astype(np.float32)
    k = n - 2048
    mag = 10.0 ** np.linspace(-30.0, 18.0, k)
    g[2048:] = (mag * rng.choice([-1.0, 1.0], k)).astype(np.float32)
    m[2048:] = (mag * rng.standard_normal(k)).astype(np.float32)
    v[2048:] = ((mag * rng.uniform(0.1, 2.0, k)) ** 2).astype(np.float32)
    t, lr, b1, b2 = 7, 5e-4, 0.9, 0.999
    return Case(f"values eps={eps:g}", b1, b2, eps, [(p, g, m, v, -lr / (1 - b1 ** t), (1 - b2 ** t) ** 0.5, 0.0)])


NONFINITE = {5: np.nan, 255: np.inf, 256: -np.inf, 2047: np.nan, 2048: np.inf, 2049: -np.inf, 4096: np.nan}


def nonfinite_case():
    """A plausible 4,097-element tensor whose gradient is NaN or +-inf at NONFINITE's indices (block
    and wave boundaries among them)."""
    rng = np.random.default_rng(104)
    b1, b2 = 0.9, 0.999
    p, g, m, v, step, bc2, _ = _tensor(rng, VALUE_N, 3, 1e-3, b1, b2, 0.0)
    for i, x in NONFINITE.items():
        g[i] = x
    return Case("non-finite gradients", b1, b2, 1e-5, [(p, g, m, v, step, bc2, 0.02)])


def all_cases():
    return [geometry_case(), full_table_case(), chunk_case(49), chunk_case(97), value_case(1e-5), value_case(1e-8),
            nonfinite_case()]
