"""The proposal-sampler kernels (csrc/propnet.hip) at their edge shapes, through the C ABI: rows of
NERF_PROP_MAX_EDGES edges, the 64-lane chunk boundaries of the cdf scan, blocks with dead waves
(R < 4, R = 5), row strides larger than the rows, and guarded buffers (tests/_guarded.py) whose pad
columns no call may touch.  References: tests/_prop_ref.py, fp64 on the same fp32 inputs.

Bars: cdf 2^-24 absolute; s 8u max(|v_b|, |v_b+1|) with u = 2^-24; t 1e-5 relative; per-ray loss
1e-5 relative + 1e-12; gradient 1e-5 of the row's largest reference magnitude.  The fp32 restatements
use at most 13 % (s), 2 % (t) and 1 % (loss, gradient) of them (tests/test_adam_prop_logic.py)."""
import numpy as np
import pytest
import torch

import _prop_ref as P
from _guarded import GUARD, SENTINEL, Guarded

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def lib():
    import nerf_amd
    return nerf_amd._lib.load()  # fail loudly if the HIP library is missing


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _named(R, C, ld):
    return (torch.arange(R * ld) % ld) < C


def rows_in(a, ld):
    """Guarded [R][ld] holding a's [R, C] columns; the pad columns keep the NaN pattern."""
    R, C = a.shape
    buf = Guarded(R * ld, named=_named(R, C, ld))
    buf.body.view(R, ld)[:, :C] = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    assert int((buf.flat[:GUARD] != SENTINEL).sum()) == 0 and int((buf.flat[-GUARD:] != SENTINEL).sum()) == 0
    return buf


def rows_out(R, C, ld):
    return Guarded(R * ld, named=_named(R, C, ld))


def read(buf, R, C, ld):
    return buf.body.view(R, ld)[:, :C].cpu().numpy()


def unread(buf, what):
    """A buffer the call only reads: returns the check that no word of it, guards and pad columns
    included, changed (Guarded.check(written=False) is for a buffer that holds the pattern alone)."""
    before = buf.flat.clone()

    def check():
        assert torch.equal(before, buf.flat), f"{what}: a word of a read-only buffer or its guards changed"

    return check


def shifts(R):
    """Five kinds of row: a call with fewer rays is repeated so that every kind gets every slot."""
    return range(P.PATTERNS) if R < P.PATTERNS else (0,)


# ----------------------------------------------------------------------------- nerf_prop_cdf
@pytest.mark.parametrize("R", P.CDF_R)
@pytest.mark.parametrize("K", P.CDF_K)
def test_cdf_edges(lib, K, R):
    """ld_w = K + 3, ld_cdf = K + 6.  Rows: 0.5 followed by 2^-26 each, all zero, all mass in the last
    bin, 0.5 down to 1e-30, random."""
    ldw, ldc = K + 3, K + 6
    for shift in shifts(R):
        w = P.cdf_weights(K, R, shift)
        wb, cb = rows_in(w, ldw), rows_out(R, K + 1, ldc)
        same = unread(wb, "weights")
        assert lib.nerf_prop_cdf(wb.ptr(), ldw, R, K, cb.ptr(), ldc, _stream()) == 0
        torch.cuda.synchronize()
        cb.check(f"cdf K={K} R={R} shift={shift}")
        same()
        got, ref = read(cb, R, K + 1, ldc), P.cdf_ref64(w)
        assert np.all(got[:, 0] == 0.0) and np.all(got[:, K] == 1.0)
        err = np.abs(got.astype(np.float64) - ref)
        assert err.max() <= 2.0 ** -24, f"K={K} R={R} shift={shift}: cdf off by {err.max():.3e} at {np.argwhere(err == err.max())[0]}"


# ----------------------------------------------------------------------------- nerf_prop_sample
def run_sample(lib, vals, cdf, n, stratified, seed, counter, transform):
    R, E = vals.shape
    ldv, ldc, ldo = E + 3, E + 5, n + 1 + 7
    vb, cb = rows_in(vals, ldv), rows_in(cdf, ldc)
    sb, tb = rows_out(R, n + 1, ldo), rows_out(R, n + 1, ldo)
    same = unread(vb, "vals"), unread(cb, "cdf")
    st = lib.nerf_prop_sample(vb.ptr(), ldv, cb.ptr(), ldc, R, E - 1, n, int(stratified), seed, counter,
                              P.TRANSFORMS.index(transform), P.NEAR, P.FAR, sb.ptr(), tb.ptr(), ldo, _stream())
    assert st == 0
    torch.cuda.synchronize()
    sb.check("s_out")
    tb.check("t_out")
    for f in same:
        f()
    return read(sb, R, n + 1, ldo), read(tb, R, n + 1, ldo)


def check_sample(what, got, vals, cdf, u, transform):
    s, t = got
    s64, t64, bar = P.sample_ref64(vals, cdf, u, transform)
    es = np.abs(s.astype(np.float64) - s64) / bar
    assert es.max() <= 1.0, f"{what}: s misses its bar {es.max():.2f}-fold at {np.argwhere(es == es.max())[0]}"
    et = np.abs(t.astype(np.float64) - t64) / (1e-5 * np.abs(t64))
    assert et.max() <= 1.0, f"{what}: t misses its bar {et.max():.2f}-fold at {np.argwhere(et == et.max())[0]}"
    assert np.all(s[:, 1:] >= s[:, :-1]), f"{what}: s decreases"
    assert np.all(s[:, 0] == vals[np.arange(len(s)), _first_bucket(cdf)]), f"{what}: u = 0 is not on its edge"
    return float(es.max()), float(et.max())


def _first_bucket(cdf):
    """The bucket of u = 0: the last edge whose cdf is 0, at most K - 1."""
    K = cdf.shape[1] - 1
    return np.minimum((cdf <= 0).sum(axis=1) - 1, K - 1)


@pytest.mark.parametrize("transform", P.TRANSFORMS)
@pytest.mark.parametrize("R", P.SAMPLE_R)
@pytest.mark.parametrize("E,Q", P.SAMPLE_EDGES)
def test_sample_edges(lib, E, Q, R, transform):
    """K + 1 = E edges per ray, n + 1 = Q quantiles at i / n; strided vals, cdf and outputs.  Rows:
    a flat stretch, no mass, a single-bin jump, cdf edges at j / K exactly, random."""
    for shift in shifts(R):
        vals, cdf = P.sample_rows(E - 1, R, shift)
        got = run_sample(lib, vals, cdf, Q - 1, False, 0, 0, transform)
        check_sample(f"K+1={E} n+1={Q} R={R} shift={shift} {transform}", got, vals, cdf, P.quantiles(R, Q - 1), transform)


@pytest.mark.parametrize("transform", P.TRANSFORMS)
def test_sample_stratified_matches_host_quantiles(lib, transform):
    """Stratified, K + 1 = 65, n + 1 = 512, R = 5 with a fixed seed and a non-zero counter: the host
    forms u from the same Philox stream; two rays with equal rows get different samples."""
    st = P.STRATIFIED
    vals, cdf = P.stratified_rows()
    n = st["Q"] - 1
    u = P.quantiles(st["R"], n, True, st["seed"], st["counter"])
    got = run_sample(lib, vals, cdf, n, True, st["seed"], st["counter"], transform)
    check_sample(f"stratified {transform}", got, vals, cdf, u, transform)
    s = got[0]
    assert np.array_equal(vals[0], vals[-1]) and np.array_equal(cdf[0], cdf[-1])
    assert np.mean(s[0, 1:-1] != s[-1, 1:-1]) > 0.9, "two rays drew the same offsets"
    again = run_sample(lib, vals, cdf, n, True, st["seed"], st["counter"], transform)
    other = run_sample(lib, vals, cdf, n, True, st["seed"], st["counter"] + 1, transform)
    assert np.array_equal(s, again[0]) and np.mean(s[:, 1:-1] != other[0][:, 1:-1]) > 0.9


def test_sample_wrapper_refuses_more_than_the_limit():
    from nerf_amd import kernels as Kn
    vals = torch.linspace(0, 1, 65, device=DEV).expand(3, 65).contiguous()
    with pytest.raises(ValueError):
        Kn.prop_sample(vals, vals, 512, False, 0, 0, 2.0, 7.0)             # n + 1 = 513
    big = torch.linspace(0, 1, 513, device=DEV).expand(3, 513).contiguous()
    with pytest.raises(ValueError):
        Kn.prop_sample(big, big, 64, False, 0, 0, 2.0, 7.0)                # K + 1 = 513
    with pytest.raises(ValueError):
        Kn.prop_loss(big, big, vals, vals, 1e-7)
    with pytest.raises(ValueError):
        Kn.prop_loss(vals, vals, big, big, 1e-7)


# ----------------------------------------------------------------------------- nerf_prop_loss
@pytest.mark.parametrize("R", P.LOSS_R)
@pytest.mark.parametrize("n,K", P.LOSS_SHAPES)
def test_loss_edges(lib, n, K, R):
    """Loss only, gradient only and both, with ld_q = n + 4, ld_k = K + 6, ld_gw = K + 2; a null
    output's buffer keeps its pattern.  Rows: every query interval inside one key interval; one
    query interval over every key; query edges on key edges; w = 0 (eps = 1e-7 divides alone); random."""
    ldq, ldk, ldg = n + 1 + 3, K + 1 + 5, K + 2
    gs = 1.0 / (R * n)
    for shift in shifts(R):
        qv, qc, kv, kc = P.loss_rows(n, K, R, shift)
        lref, gref = P.loss_ref64(qv, qc, kv, kc, gs)
        lbar, gbar = P.loss_bars(lref, gref)
        ins = [rows_in(a, ld) for a, ld in ((qv, ldq), (qc, ldq), (kv, ldk), (kc, ldk))]
        same = [unread(b, name) for b, name in zip(ins, ("q_vals", "q_cdf", "k_vals", "k_cdf"))]
        for want_loss, want_grad in ((True, False), (False, True), (True, True)):
            what = f"n={n} K={K} R={R} shift={shift} loss={want_loss} grad={want_grad}"
            lb, gb = Guarded(R), rows_out(R, K, ldg)
            st = lib.nerf_prop_loss(ins[0].ptr(), ins[1].ptr(), ldq, ins[2].ptr(), ins[3].ptr(), ldk, R, n, K,
                                    P.LOSS_EPS, lb.ptr() if want_loss else None, gs,
                                    gb.ptr() if want_grad else None, ldg if want_grad else 0, _stream())
            assert st == 0, what
            torch.cuda.synchronize()
            lb.check(f"{what}: loss_ray", written=want_loss)
            gb.check(f"{what}: grad_k_w", written=want_grad)
            for f in same:
                f()
            if want_loss:
                err = np.abs(lb.body.cpu().numpy().astype(np.float64) - lref) / lbar
                assert err.max() <= 1.0, f"{what}: loss misses its bar {err.max():.2f}-fold in ray {int(np.argmax(err))}"
            if want_grad:
                err = np.abs(read(gb, R, K, ldg).astype(np.float64) - gref)
                over = err > gbar
                assert not over.any(), (f"{what}: gradient misses its bar at {np.argwhere(over)[0]}: "
                                        f"{err[over][0]:.3e} > {np.broadcast_to(gbar, err.shape)[over][0]:.3e}")
