"""CPU checks of the references behind tests/test_gpu_adam_edges.py and tests/test_gpu_prop_edges.py:
the fp32 restatements of the kernels' arithmetic must stay within a third of each bar on every input
set the GPU tests use, so a kernel that misses a bar is wrong and not merely rounding differently.

Measured (restatement error / bar, the largest over all input sets; every one at most 1/3):
  Adam p      0.249  (97 entries and non-finite gradients; 0.245 geometry, 0.241 both value sets; the constants
                     4 and 16 of the bar are kept)
  sample s    0.125  (8u max(|v_b|, |v_b+1|) is kept, no fall-back to 2e-6)
  sample t    0.019  of 1e-5 relative
  loss        0.008  of 1e-5 relative + 1e-12
  gradient    0.007  of 1e-5 of the row's largest magnitude
Adam's m' and v' are not bars: the kernel must equal the restatement bit for bit.
"""
import numpy as np

import _adam_ref as A
import _prop_ref as P


def test_adam_restatement_matches_a_scalar_walk():
    """adam_ref32 / adam_ref64 on hand-picked numbers, worked step by step."""
    f = np.float32
    p, g, m, v = f(1.5), f(0.25), f(-0.125), f(0.0625)
    step, bc2, wd, b1, b2, eps = -1e-2, 0.5, 0.5, 0.5, 0.75, 0.25
    p32, m32, v32 = A.adam_ref32([p], [g], [m], [v], step, bc2, wd, 1 - b1, b2, 1 - b2, eps)
    gv = 0.25 + 0.5 * 1.5                                  # 1.0
    mv = -0.125 + 0.5 * (gv + 0.125)                       # 0.4375
    vv = 0.0625 * 0.75 + (0.25 * gv) * gv                  # 0.296875
    want = 1.5 + step * (mv / (vv ** 0.5 / 0.5 + 0.25))
    assert m32[0] == f(mv) and v32[0] == f(vv)             # exact in fp32
    assert abs(float(p32[0]) - want) <= 2 * A.U * 1.5
    p64, m64, v64, bar = A.adam_ref64([p], [g], [m], [v], step, bc2, wd, 1 - b1, b2, 1 - b2, eps)
    assert m64[0] == mv and v64[0] == vv and abs(p64[0] - want) < 1e-9      # step is rounded to fp32
    assert bar[0] > 4 * A.U * 1.4
    # no weight decay: the parameter does not enter the gradient
    _, m0, _ = A.adam_ref32([p], [g], [m], [v], step, bc2, 0.0, 1 - b1, b2, 1 - b2, eps)
    assert m0[0] == f(-0.125 + 0.5 * (0.25 + 0.125))


def test_adam_input_sets_cover_the_edges():
    geo = A.geometry_case()
    assert [t[0].size for t in geo.tensors] == [0, 1, 255, 256, 257, 2047, 2048, 2049, 0, 4096, 4097, 6145, 3, 0]
    for case in (geo, A.full_table_case(), A.chunk_case(49), A.chunk_case(97)):
        own = {(float(np.float32(t[4])), float(np.float32(t[5])), t[6]) for t in case.tensors}
        assert len(own) == len(case.tensors), "every tensor has its own step_size, bc2_sqrt and weight_decay"
        decays = [t[6] for t in case.tensors]
        assert 0.0 in decays and any(w > 0 for w in decays)
    full = A.full_table_case()
    assert len(full.tensors) == 48 and full.tensors[47][0].size == 300
    val = A.value_case(1e-5).tensors[0]
    mag = np.abs(val[1][2048:])
    assert val[0].size == 4097 and mag.min() == np.float32(1e-30) and mag.max() == np.float32(1e18)
    assert np.all(val[1][:2048] == 0) and np.all(val[3][:2048] == 0) and np.all(val[2][1024:2048] != 0)


def test_adam_fp32_restatement_stays_within_a_third_of_the_p_bar():
    """Largest |p32 - p64| / bar over every finite element of every input set.  Measured: geometry
    0.245, full table 0.246, 49 entries 0.246, 97 entries 0.249, values 0.241 at both eps, non-finite
    gradients 0.249: all below a third, the bar's constants 4 and 16 stay."""
    shares = {}
    for case in A.all_cases():
        for (p64, m64, v64, bar), (p32, m32, v32) in case.refs():
            if p64.size == 0:
                continue
            fin = np.isfinite(p64)
            assert np.array_equal(fin, np.isfinite(p32)), case.name
            share = float((np.abs(p32[fin].astype(np.float64) - p64[fin]) / bar[fin]).max())
            shares[case.name] = max(shares.get(case.name, 0.0), share)
    for name, share in shares.items():
        print(f"{name}: |p32 - p64| at most {share:.3f} of the bar")
    assert len(shares) == 7 and max(shares.values()) <= 1 / 3


def test_adam_nonfinite_rows_of_the_restatement():
    (p64, m64, v64, _), (p32, m32, v32) = A.nonfinite_case().refs()[0]
    bad = np.zeros(A.VALUE_N, bool)
    bad[list(A.NONFINITE)] = True
    for a in (p64, m64, v64, p32, m32, v32):
        assert np.array_equal(~np.isfinite(a), bad)
    for i, x in A.NONFINITE.items():
        if np.isinf(x):
            assert m32[i] == x and v32[i] == np.inf and np.isnan(p32[i])


def test_cdf_reference_keeps_what_a_float_sum_drops():
    w = P.cdf_weights(511, 5, 0)
    ref = P.cdf_ref64(w)
    assert ref.shape == (5, 512) and np.all(ref[:, 0] == 0) and np.all(ref[:, -1] == 1)
    assert np.all(np.diff(ref[:, :-1], axis=1) >= 0) and float(ref[:, :-1].max()) < 1.0
    run = np.cumsum(w[0], dtype=np.float32)
    assert run[-1] == np.float32(0.5) and ref[0, 510] == 0.5 + 509 * 2.0 ** -26
    assert abs(float(np.float32(ref[0, 510])) - 0.5) > 100 * 2.0 ** -26          # far beyond the 2^-24 bar
    assert np.all(ref[1, :-1] == 0) and np.all(ref[2, :-1] == 0)
    assert float(w[3].max()) == np.float32(0.5 / max(1.0, (10.0 ** np.linspace(np.log10(0.5), -30, 511)).sum() * 1.001))
    assert 0 < float(w[3].min()) < 1e-29
    w2 = P.cdf_weights(2, 4, 3)                                              # kinds 3, 4, 0, 1
    assert w2[0, 0] == np.float32(0.5) and w2[0, 1] == np.float32(1e-30)


def _sample_sets():
    for E, Q in P.SAMPLE_EDGES:
        for R in P.SAMPLE_R:
            for shift in (range(P.PATTERNS) if R < P.PATTERNS else (0,)):
                vals, cdf = P.sample_rows(E - 1, R, shift)
                yield f"K+1={E} n+1={Q} R={R} shift={shift}", vals, cdf, P.quantiles(R, Q - 1)
    s = P.STRATIFIED
    vals, cdf = P.stratified_rows()
    yield "stratified", vals, cdf, P.quantiles(s["R"], s["Q"] - 1, True, s["seed"], s["counter"])


def test_sample_fp32_restatement_stays_within_a_third_of_each_bar():
    """Measured: s at most 0.125 of 8u max(|v_b|, |v_b+1|); t (fp32 stot of the fp32 s) at most 0.019
    of 1e-5 relative, over the twelve edge pairs, R = 1 and 5, every kind of row and the stratified set."""
    import torch
    from oracle import nerfacc_oracle as NO
    worst_s = worst_t = 0.0
    for name, vals, cdf, u in _sample_sets():
        assert np.all(np.diff(u, axis=1) >= 0) and u.min() == 0.0 and u.max() == 1.0, name
        s32 = P.sample_fp32(vals, cdf, u)
        for tr in P.TRANSFORMS:
            s64, t64, bar = P.sample_ref64(vals, cdf, u, tr)
            worst_s = max(worst_s, float((np.abs(s32 - s64) / bar).max()))
            t32 = NO.stot(torch.from_numpy(s32), tr, P.NEAR, P.FAR).numpy()
            worst_t = max(worst_t, float((np.abs(t32 - t64) / (1e-5 * np.abs(t64))).max()))
    print(f"s: {worst_s:.3f} of its bar; t: {worst_t:.3f} of its bar")
    assert worst_s <= 1 / 3 and worst_t <= 1 / 3


def test_sample_rows_hold_the_named_kinds():
    vals, cdf = P.sample_rows(64, 5, 0)
    u = P.quantiles(5, 64)
    assert np.any(np.diff(cdf[0, :-1]) == 0) and np.all(cdf[1, :-1] == 0) and set(np.unique(cdf[2])) == {0.0, 1.0}
    assert np.array_equal(cdf[3], u[3])                                      # quantiles exactly on the edges
    s64, _, _ = P.sample_ref64(vals, cdf, u, "uniform")
    assert np.array_equal(s64[3], vals[3].astype(np.float64))
    # no mass before the last edge: every quantile falls into the last bucket, linear in u
    last = float(vals[1, 63])
    assert s64[1, 0] == last and s64[1, -1] == 1.0 and np.allclose(s64[1], last + u[1] * (1.0 - last), atol=1e-12)
    st = P.STRATIFIED
    us = P.quantiles(2, 511, True, st["seed"], st["counter"])
    i = np.arange(1, 511)
    assert np.all(us[:, 1:511] >= (i - 0.5) / 511 - 1e-7) and np.all(us[:, 1:511] <= (i + 0.5) / 511 + 1e-7)
    assert not np.array_equal(us[0], us[1])


def _loss_sets():
    for n, K in P.LOSS_SHAPES:
        for R in P.LOSS_R:
            for shift in (range(P.PATTERNS) if R < P.PATTERNS else (0,)):
                yield f"n={n} K={K} R={R} shift={shift}", P.loss_rows(n, K, R, shift), 1.0 / (R * n)


def test_loss_fp32_restatement_stays_within_a_third_of_each_bar():
    """Measured: per-ray loss at most 0.008 of 1e-5 relative + 1e-12; gradient at most 0.007 of 1e-5 of
    the row's largest magnitude (rows whose reference gradient is zero must be exactly zero)."""
    worst_l = worst_g = 0.0
    for name, rows, gs in _loss_sets():
        lref, gref = P.loss_ref64(*rows, gs)
        l32, g32 = P.loss_fp32(*rows, gs)
        lbar, gbar = P.loss_bars(lref, gref)
        worst_l = max(worst_l, float((np.abs(l32 - lref) / lbar).max()))
        zero = gbar[:, 0] == 0
        assert np.all(g32[zero] == 0), name
        if np.any(~zero):
            worst_g = max(worst_g, float((np.abs(g32 - gref)[~zero] / gbar[~zero]).max()))
    print(f"loss: {worst_l:.3f} of its bar; gradient: {worst_g:.3f} of its bar")
    assert worst_l <= 1 / 3 and worst_g <= 1 / 3


def test_loss_rows_hold_the_named_kinds():
    n, K = 64, 65
    qv, qc, kv, kc = P.loss_rows(n, K, 5, 0)
    cnt = np.stack([np.searchsorted(kv[r], qv[r], side="right") for r in range(5)])
    assert len(set(cnt[0])) == 1 and 0 < cnt[0, 0] <= K                      # all inside one key interval
    spans = (cnt[1, :-1] == 0) & (cnt[1, 1:] == K + 1)
    assert spans.sum() == 1 and set(cnt[1]) == {0, K + 1}                    # one interval over every key
    assert np.isin(qv[2], kv[2]).all()                                       # query edges on key edges
    assert np.sum(np.diff(qc[3]) == 0) > n // 4                              # w = 0 (eps alone divides)
    lref, gref = P.loss_ref64(qv, qc, kv, kc, 0.25)
    assert np.all(lref > 0) and np.all(gref[1] == 0) and gref[0].min() < 0
    # gradient against central differences of the loss in the key weights (row 4, fp64 throughout)
    w = np.diff(kc[4].astype(np.float64))

    def total(wk):
        c = np.concatenate([[0.0], np.cumsum(wk)[:-1], [1.0]])[None]
        import torch
        from oracle import nerfacc_oracle as NO
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()
        return float(NO.pdf_loss(t(qv[4:5]), t(qc[4:5]), t(kv[4:5]), t(c), float(np.float32(P.LOSS_EPS))).sum()) * 0.25

    for j in (0, 17, K - 2, K - 1):
        e = np.zeros(K)
        e[j] = 1e-7
        fd = (total(w + e) - total(w - e)) / 2e-7
        assert abs(fd - gref[4, j]) <= 1e-4 * np.abs(gref[4]).max() + 1e-9, j
