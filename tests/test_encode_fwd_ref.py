"""The fp64 restatement of the encoding forward kernels (_encode_fwd_ref.py) checks itself, on the
CPU: against the oracle's encodings evaluated in fp64 for every case the GPU tests use, torch's fp32
evaluation of the same row against the derived bound, the size of that bound, and the conditions on
the inputs that make the GPU comparison able to see a wrong weight, a wrong level index or a wrong
thread mapping."""
import pytest
import torch

import _encode_fwd_ref as F
from _encode_bwd_ref import _oracle_encode
from oracle import nerf_oracle as O

RAYS = F.by_name(F.RAY_CASES)
SAMPLES = F.by_name(F.SAMPLE_CASES)


def _oracle_rays(c, inp):
    o, d, t0, t1 = (inp[k].double() for k in ("o", "d", "t0", "t1"))
    pos, dirs = O.compute_positions(o, d, t0, t1, "left" if c.query == 0 else "middle")
    pw = F.expand_pw(inp["pw"], c.pw_mode, c.n_rays, c.samples).double()
    return _oracle_encode(c, pos.reshape(-1, 3), dirs.reshape(-1, 3), pw, t0.reshape(-1), t1.reshape(-1))


def _oracle_samples(c, inp):
    return _oracle_encode(c, inp["x"].double(), inp["d"].double(), inp["pw"].double(), inp["t0"].double(),
                          inp["t1"].double())


def _both(name):
    if name in RAYS:
        c = RAYS[name]
        inp = F.ray_inputs(c)
        return c, inp, F.ray_quantities, _oracle_rays
    c = SAMPLES[name]
    return c, F.sample_inputs(c), F.sample_quantities, _oracle_samples


ALL = list(RAYS) + list(SAMPLES)


def test_case_names_are_distinct():
    assert len(set(ALL)) == len(F.RAY_CASES) + len(F.SAMPLE_CASES)


@pytest.mark.parametrize("name", ALL)
def test_exact_matches_oracle(name):
    """Every quantity formed in fp64: the row is the oracle's fourier_features / barf_pe /
    integrated_pe on fp64 inputs, to 1e-12 per column."""
    c, inp, quantities, oracle = _both(name)
    ref = F.fwd_ref(c, quantities(c, inp, exact=True))
    want = oracle(c, inp)
    assert ref.ref.shape == want.shape == (c.n_rays * c.samples, c.out_dim)
    err = (ref.ref - want).abs().max().item()
    print(f"{name}: max |restatement - oracle| = {err:.2e}")
    assert err <= 1e-12


@pytest.mark.parametrize("name", ALL)
def test_fp32_evaluation_within_bound(name):
    """torch's fp32 evaluation of the same row, operation by operation: cos / sin columns within the
    bound, masked columns exactly zero, identity columns bit-equal; the bound below 1e-6 wherever
    m_k w > 0."""
    c, inp, quantities, _ = _both(name)
    q = quantities(c, inp)
    ref = F.fwd_ref(c, q)
    got = F.fwd_fp32(c, q)
    assert got.dtype == torch.float32 and torch.isfinite(got).all()
    err = (got.double() - ref.ref).abs()
    zero = ref.bound == 0
    assert (err[zero] == 0).all()
    ratio = torch.where(zero, torch.zeros_like(err), err / ref.bound).max().item()
    live = ref.bound[~zero]
    print(f"{name}: fp32 evaluation max err / bound {ratio:.3f}; largest bound "
          f"{live.max().item() if live.numel() else 0.0:.2e}")
    assert ratio <= 1.0
    if live.numel():
        assert live.max().item() < 1e-6
    if c.identity:
        assert ref.ident.dtype == torch.float32
        assert torch.equal(got[:, :3].view(torch.int32), ref.ident.view(torch.int32))
    if c.alpha is not None and c.levels:
        dead = (~ref.unmasked).reshape(-1, 3 * c.levels)
        idn = 3 if c.identity else 0
        for blk in (0, 1):
            cols = got[:, idn + blk * 3 * c.levels: idn + (blk + 1) * 3 * c.levels]
            assert (cols[dead] == 0).all()
            assert (ref.bound[:, idn + blk * 3 * c.levels: idn + (blk + 1) * 3 * c.levels][dead] == 0).all()


def test_the_weight_matters():
    """Over the kind-1 cases of each list some unmasked column carries a weight strictly between 0.01
    and 0.99, and another a weight that has underflowed to zero in fp32: a weight with 2^k in place
    of 4^k, or taken at another level, moves columns by far more than their bound."""
    for cases, build in ((F.RAY_CASES, F.ray_case), (F.SAMPLE_CASES, F.sample_case)):
        mid = gone = 0
        x_lo, x_hi = float("inf"), 0.0
        for c in cases:
            if c.kind != 1 or c.levels == 0:
                continue
            _, ref = build(c)
            w, x = ref.w[ref.unmasked], ref.x[ref.unmasked]
            mid += int(((w > 0.01) & (w < 0.99)).sum())
            gone += int((w < 2.0 ** -149).sum())
            x_lo, x_hi = min(x_lo, x.min().item()), max(x_hi, x.max().item())
            # the damped columns are seen at their own size: the bound follows w down
            live = (ref.mw > 0) & (ref.mw < 1e-3)
            if live.any():
                idn = 3 if c.identity else 0
                b = ref.bound[:, idn:idn + 3 * c.levels].reshape(-1, 3, c.levels)
                assert (b[live] < 1e-8).all()
        print(f"unmasked columns with w in (0.01, 0.99): {mid}, with w = 0 in fp32: {gone}; x from {x_lo:.2e} to "
              f"{x_hi:.2e}")
        assert mid >= 100 and gone >= 100


def test_both_sincos_branches_occur():
    """The 16-level cases hold arguments on both sides of the shared sin / cos's 2^19 limit, in one
    row."""
    for c, quantities, inputs in ((RAYS["k0_L16_id_mask"], F.ray_quantities, F.ray_inputs),
                                  (RAYS["k0_L16"], F.ray_quantities, F.ray_inputs)) + tuple(
            (s, F.sample_quantities, F.sample_inputs) for s in F.SAMPLE_CASES
            if s.levels == 16 and s.scale > 1.0):
        q = quantities(c, inputs(c))
        a = (q.pm.unsqueeze(2) * F._scales(c, torch.float32).view(1, 1, -1)).abs().reshape(q.pm.shape[0], -1)
        both = ((a >= 2.0 ** 19).any(1) & (a < 2.0 ** 19).any(1)).sum().item()
        print(f"{c.name}: largest argument {a.max().item():.2e}, rows with both branches {both}")
        if c.name != "k0_L16":
            assert both > 0
        else:
            assert a.max().item() > 4e5


def test_sample_cases_cover_the_tiles_and_forms():
    rows = {c.n_rays for c in F.SAMPLE_CASES}
    assert rows == {1, 63, 64, 65, 129}
    for kind in (0, 1):
        mine = [c for c in F.SAMPLE_CASES if c.kind == kind]
        assert {(c.levels, c.identity) for c in mine} == set(F._levels_identity())
        assert sum(c.alpha is not None for c in mine) == 1
    assert {(c.distribute, c.sigma) for c in F.SAMPLE_CASES if c.kind == 1} == set(F._VAR)
    # the 64-thread mapping of the LDS kernel (3 L > 32) with rows on both sides of a tile
    assert {c.n_rays for c in F.SAMPLE_CASES if c.levels >= 11} >= {63, 64, 65, 129}
