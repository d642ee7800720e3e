"""GPU tests of the 2-D hash grid (nerf_hashgrid2d_fwd / _bwd) and nerf_amd.model_ingp2d.

Kernels: bitwise against oracle/hashgrid_oracle.py::encode_2d (forward) and the numpy int64
restatement of the fixed-point rule, tests/_ingp2d_ref.py::table_grad_fixed (table gradient).

Model against the reference's own run (tests/golden/ingp2d.npz): features bitwise; for everything
behind a GEMM the bound is derived, not fitted (``_bounds`` below): a GEMM output z = sum_k a_k w_k + b
over K terms carries at most (eps + K 2^-24) * max sum_k |a_k w_k| of its own error — eps the
per-product error, 2^-24 for the fp32 MFMA path ("highest"), 2^-17 for the 3 x bf16 split ("high"),
K 2^-24 the fp32 accumulation — plus the incoming activation error times the weight matrix's largest
absolute row sum; ReLU is 1-Lipschitz, the sigmoid's slope is at most 1/4.  The backward runs the same
recurrence on d = dL/dz (K = the layer's width for the input gradient, K = 503 samples for the weight
and bias gradients), and a table entry sums w * d over its corners, so its error is at most the
error of d times the row's largest sum of weights.  All magnitudes come from the fixture (fp64 on the
CPU); the reference's own fp32 run carries the same bound with eps = 2^-24, so the tolerance is
bound(eps) + bound(2^-24).  Adam: the first steps move a weight by lr g / (|g| + 1e-8), whose
derivative in g is at most 1 / (|g| + 1e-8), so three steps differ by at most
3 lr min(2, E_g / (max(|g| - E_g, 0) + 1e-8)) per element (E_g the gradient's bound, |g| the
fixture's first gradient) plus the rounding of three fp32 updates.
Derived bounds and the errors measured on an MI355X (configuration A / B; gradients: the tensor
with the largest measured error, error and bound relative to its largest reference entry):
    highest  rgb        bound 7.3e-06 / 3.9e-07   measured 6.0e-08 / 6.0e-08
             loss       bound 7.4e-06 / 4.7e-07   measured 7.5e-09 / 7.5e-09
             gradients  bound 4.4e-03 / 4.2e-04   measured 6.2e-07 / 2.3e-07
    high     rgb        bound 2.7e-05 / 9.5e-07   measured 1.2e-07 / 1.2e-07
             loss       bound 2.8e-05 / 1.1e-06   measured 7.5e-09 / 7.5e-09
             gradients  bound 1.2e+00 / 5.3e-04   measured 1.2e-05 / 4.6e-07
The bounds are worst-case sums of absolute values carried through every layer, so they are loose
where the chain is long: configuration A's coarsest table at "high" is bounded only by 1.2 of its
largest entry (three layers of absolute row sums, then 80 samples' weights per row), configuration
B's single layer to 5e-4.  Three FusedAdam steps: largest parameter error 2.6e-06 (A, "high"), every
element inside its bound.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ingp2d_ref as R  # noqa: E402
from oracle import hashgrid_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
CONFIGS = {"A": dict(enc=(64, 4, 2 ** 8, 2, 5), n_hidden=2), "B": dict(enc=(100, 3, 1000, 4, 4), n_hidden=0)}
MAIN = dict(res=R.schedule(2048, 16, 16), T=2 ** 16, F=2)


@pytest.fixture(scope="module", autouse=True)
def _lib():
    import nerf_amd
    nerf_amd._lib.load()
    yield


def _tables(res, T, F, seed=0, scale=1.0):
    rng = np.random.default_rng(seed)
    return [((rng.random((R.level_rows(r, T), F)) * 2 - 1) * scale).astype(np.float32) for r in res]


def _params(res, T, F, primes=R.PRIMES):
    from nerf_amd import kernels as K
    return K.make_hashgrid_params(len(res), T, F, res, 0, primes=(primes[0], primes[1], 0), normalize=False)


def _fwd(x, tables, res, T, F, primes=R.PRIMES, ld=None, guard=64):
    """(features [n, L F], status) from nerf_hashgrid2d_fwd with NaN canary rows around the table (a
    stray read poisons the output), a NaN-filled [n + 3, ld] output (pad columns and rows beyond n
    must stay NaN) and a status word."""
    from nerf_amd import kernels as K
    n, cols = x.shape[0], len(res) * F
    ld = cols if ld is None else ld
    packed = np.concatenate(tables, axis=0)
    buf = torch.full((packed.shape[0] + 2 * guard, F), float("nan"), device=DEV)
    buf[guard:guard + packed.shape[0]] = torch.from_numpy(packed).to(DEV)
    out = torch.full((n + 3, ld), float("nan"), device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    K.hashgrid2d_fwd(_params(res, T, F, primes), buf[guard:guard + packed.shape[0]], out,
                     torch.from_numpy(np.ascontiguousarray(x)).to(DEV), n, status)
    o = out.cpu().numpy()
    assert np.isnan(o[n:]).all() and np.isnan(o[:n, cols:]).all(), "store outside the [n, L F] block"
    assert torch.isnan(buf[:guard]).all() and torch.isnan(buf[guard + packed.shape[0]:]).all()
    return o[:n, :cols], int(status.item())


def _bwd(x, g, res, T, F, primes=R.PRIMES, accumulate=None, seed=1, guard=64):
    """Packed table gradient from nerf_hashgrid2d_bwd out of a garbage-filled workspace, with canary
    rows around the gradient buffer."""
    from nerf_amd import kernels as K
    p = _params(res, T, F, primes)
    rows = K.hashgrid2d_table_rows(p)
    gen = torch.Generator(device=DEV).manual_seed(seed)
    ws = torch.randint(-2 ** 62, 2 ** 62, ((K.hashgrid2d_workspace_bytes(p) + 7) // 8,), dtype=torch.int64, device=DEV,
                       generator=gen)
    buf = torch.full((rows + 2 * guard, F), -7.5, device=DEV)
    gt = buf[guard:guard + rows]
    if accumulate is not None:
        gt.copy_(torch.from_numpy(accumulate).to(DEV))
    K.hashgrid2d_bwd(p, torch.from_numpy(g).to(DEV), gt, ws, torch.from_numpy(np.ascontiguousarray(x)).to(DEV),
                     x.shape[0], accumulate=accumulate is not None)
    assert (buf[:guard] == -7.5).all() and (buf[guard + rows:] == -7.5).all(), "store outside the gradient"
    return gt.cpu().numpy()


# ----------------------------------------------------------------------------- forward
@pytest.mark.parametrize("tag", ["A", "B"])
def test_forward_fixture_points_bitwise(golden, tag):
    g = golden("ingp2d")
    T, F = CONFIGS[tag]["enc"][2], CONFIGS[tag]["enc"][3]
    res = [int(r) for r in g[f"{tag}.res"]]
    tables = [g[f"{tag}.sd.position_encoder.encodings.{l}.table"] for l in range(len(res))]
    got, status = _fwd(g["x"], tables, res, T, F)
    assert status == 0
    assert np.array_equal(got, O.encode_2d(g["x"], tables, res, T))
    assert np.array_equal(got, g[f"{tag}.features"])


def test_forward_main_shape_bitwise():
    res, T, F = MAIN["res"], MAIN["T"], MAIN["F"]
    rng = np.random.default_rng(2)
    x = rng.random((20000, 2), dtype=np.float32)
    x[:3] = [[0.0, 0.0], [1 - 2.0 ** -24, 1 - 2.0 ** -24], [0.999999, 0.5]]
    tables = _tables(res, T, F)
    got, status = _fwd(x, tables, res, T, F)
    assert status == 0 and np.array_equal(got, O.encode_2d(x, tables, res, T))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_forward_batch_sizes_and_wide_rows(n):
    res, T, F = R.schedule(100, 3, 4), 1000, 2
    x = np.random.default_rng(n).random((n, 2), dtype=np.float32)
    tables = _tables(res, T, F, seed=n)
    got, status = _fwd(x, tables, res, T, F, ld=len(res) * F + 5)
    assert status == 0 and np.array_equal(got, O.encode_2d(x, tables, res, T))


@pytest.mark.parametrize("F", [1, 4, 8])
def test_forward_feature_counts(F):
    res, T = R.schedule(300, 5, 7), 2 ** 10
    x = np.random.default_rng(F).random((193, 2), dtype=np.float32)
    tables = _tables(res, T, F, seed=F)
    got, status = _fwd(x, tables, res, T, F, ld=64)
    assert status == 0 and np.array_equal(got, O.encode_2d(x, tables, res, T))


def test_forward_custom_primes_and_32_levels():
    x = np.random.default_rng(9).random((130, 2), dtype=np.float32)
    for res, T, primes in ((R.schedule(500, 4, 6), 2 ** 9, (73856093, 19349663)),
                           (R.schedule(500, 4, 6), 777, (-3, 2 ** 40 + 17)),
                           (R.schedule(4000, 2, 32), 2 ** 8, R.PRIMES)):
        tables = _tables(res, T, 2, seed=T)
        got, status = _fwd(x, tables, res, T, 2, primes=primes)
        want, st = R.encode(x, tables, res, T, primes)
        assert status == 0 and st == 0 and np.array_equal(got, want)
        if primes == R.PRIMES:
            assert np.array_equal(got, O.encode_2d(x, tables, res, T))


# ----------------------------------------------------------------------------- domain
OUTSIDE = np.array([[-0.25, 0.5], [0.5, 1.0], [1.5, 0.25], [1.0, 1.0], [1e9, 0.5], [0.5, -1e9]], dtype=np.float32)


def test_points_outside_the_unit_square():
    """Out-of-range corners of bijective levels are dropped (forward and backward) and flagged, hashed
    levels follow the formula, and nothing outside the table or the gradient is touched (the NaN and
    -7.5 canaries of _fwd / _bwd)."""
    res, T, F = R.schedule(100, 3, 4), 1000, 4              # 3, 9 bijective; 31, 100 hashed
    inside = np.random.default_rng(3).random((70, 2), dtype=np.float32)
    x = np.concatenate((inside[:35], OUTSIDE, inside[35:]))
    tables = _tables(res, T, F)
    got, status = _fwd(x, tables, res, T, F)
    want, st = R.encode(x, tables, res, T)
    assert st == 1 and status & 1
    assert np.array_equal(got, want)
    hashed = slice(2 * F, 4 * F)
    assert np.array_equal(got[:, hashed], O.encode_2d(x, tables[2:], res[2:], T))
    _, status_in = _fwd(inside, tables, res, T, F)
    assert status_in == 0
    # a power-of-two table: the hashed levels' 32-bit form and its 64-bit form beyond |x_hat| = 2^30
    res2, T2 = R.schedule(64, 4, 5), 2 ** 8
    tables2 = _tables(res2, T2, 2)
    got2, status2 = _fwd(x, tables2, res2, T2, 2)
    want2, _ = R.encode(x, tables2, res2, T2)
    assert status2 & 1 and np.array_equal(got2, want2)
    # table gradient: bitwise the restatement, and the dropped corners add nothing to any row
    g = np.random.default_rng(4).standard_normal((x.shape[0], len(res) * F)).astype(np.float32)
    grad = _bwd(x, g, res, T, F)
    assert np.array_equal(grad, R.table_grad_fixed(x, g, res, T, F))
    only = np.zeros_like(g)
    only[35:35 + len(OUTSIDE)] = g[35:35 + len(OUTSIDE)]
    assert np.array_equal(_bwd(x, only, res, T, F), R.table_grad_fixed(x, only, res, T, F))
    bij_rows = 16 + 100
    all_out = np.array([[-0.25, 1.5], [1.5, -3.0], [2.0, 2.0]], dtype=np.float32)      # every corner dropped
    assert not _bwd(all_out, g[:3], res, T, F)[:bij_rows].any()


# ----------------------------------------------------------------------------- table gradient
def _grad_case(name):
    rng = np.random.default_rng(5)
    if name == "main":
        res, T, F, n = MAIN["res"], MAIN["T"], MAIN["F"], 20000
        x = rng.random((n, 2), dtype=np.float32)
    elif name == "B":
        res, T, F, n = R.schedule(100, 3, 4), 1000, 4, 257
        x = rng.random((n, 2), dtype=np.float32)
    else:
        res, T, F, n = R.schedule(64, 4, 5), 256, 8, 4096
        x = np.tile(np.array([[0.3183, 0.7071]], dtype=np.float32), (n, 1))
    g = rng.standard_normal((n, len(res) * F)).astype(np.float32)
    return x, g, res, T, F


@pytest.mark.parametrize("name", ["main", "B", "contended"])
def test_table_gradient_bitwise_and_deterministic(name):
    x, g, res, T, F = _grad_case(name)
    first = _bwd(x, g, res, T, F, seed=1)
    again = _bwd(x, g, res, T, F, seed=2)
    assert np.array_equal(first, again)
    want = R.table_grad_fixed(x, g, res, T, F)
    assert first.shape == want.shape and (name != "main" or first.shape[0] == 554051)
    assert np.array_equal(first, want)


def test_table_gradient_small_scales_accumulate_nan_and_empty():
    x, g, res, T, F = _grad_case("B")
    want = R.table_grad_fixed(x, g, res, T, F)
    base = np.random.default_rng(6).standard_normal(want.shape).astype(np.float32)
    assert np.array_equal(_bwd(x, g, res, T, F, accumulate=base), base + want)
    # fewer than 512 points take llrint, tiny gradients the capped exponent, a wide g_ld the row stride
    tiny = (g * np.float32(1e-30)).astype(np.float32)
    assert np.array_equal(_bwd(x, tiny, res, T, F), R.table_grad_fixed(x, tiny, res, T, F))
    wide = np.concatenate((g, np.full((g.shape[0], 3), 1e30, np.float32)), axis=1)
    assert np.array_equal(_bwd(x, wide, res, T, F), want)
    assert not _bwd(x, np.zeros_like(g), res, T, F).any()
    bad = g.copy()
    bad[100, 7] = np.nan
    assert np.isnan(_bwd(x, bad, res, T, F)).all()
    bad[100, 7] = np.inf
    assert np.isnan(_bwd(x, bad, res, T, F)).all()
    empty_x, empty_g = np.zeros((0, 2), np.float32), np.zeros((0, len(res) * F), np.float32)
    assert not _bwd(empty_x, empty_g, res, T, F).any()
    assert np.array_equal(_bwd(empty_x, empty_g, res, T, F, accumulate=base), base)
    feats, status = _fwd(empty_x, _tables(res, T, F), res, T, F)
    assert feats.shape == (0, len(res) * F) and status == 0


# ----------------------------------------------------------------------------- model vs fixture
@pytest.fixture(params=["highest", "high"])
def matmul_precision(request):
    old = torch.get_float32_matmul_precision()
    torch.set_float32_matmul_precision(request.param)
    yield request.param
    torch.set_float32_matmul_precision(old)


def _bounds(g, tag, eps):
    """First-order error bounds of one run at per-product error eps (the module docstring): dict with
    'rgb', 'loss' and 'grad' {parameter name: absolute bound}."""
    u = 2.0 ** -24
    T, F = CONFIGS[tag]["enc"][2], CONFIGS[tag]["enc"][3]
    res = [int(r) for r in g[f"{tag}.res"]]
    keys = [str(k) for k in g[f"{tag}.keys"]]
    wk = [k for k in keys if k.endswith("weight")]
    Ws = [g[f"{tag}.sd.{k}"].astype(np.float64) for k in wk]
    bs = [g[f"{tag}.sd.{k[:-6]}bias"].astype(np.float64) for k in wk]
    y = g["y"].astype(np.float64)
    N = y.shape[0]
    eff = lambda K: eps + K * u
    acts, errs = [g[f"{tag}.features"].astype(np.float64)], [0.0]         # the features are bitwise: no error
    for i, (W, b) in enumerate(zip(Ws, bs)):
        a = acts[-1]
        z = a @ W.T + b
        S = np.abs(a) @ np.abs(W).T + np.abs(b)
        e = eff(W.shape[1]) * S.max() + errs[-1] * np.abs(W).sum(1).max()
        acts.append(np.maximum(z, 0) if i < len(Ws) - 1 else z)
        errs.append(e)
    rgb = 1 / (1 + np.exp(-acts[-1]))
    e_rgb = errs[-1] / 4 + 2 * u
    loss = ((rgb - y) ** 2).mean()
    out = {"rgb": e_rgb, "loss": 2 * np.abs(rgb - y).max() * e_rgb + 4 * u * loss, "grad": {}}
    c = 2.0 / (3 * N)
    d = c * (rgb - y) * rgb * (1 - rgb)
    e_d = c * 1.25 * e_rgb + 4 * u * np.abs(d).max()
    for i in reversed(range(len(Ws))):
        a, e_a, W = acts[i], errs[i], Ws[i]
        out["grad"][wk[i]] = (eff(N) * (np.abs(d).T @ np.abs(a)).max() + e_d * np.abs(a).sum(0).max()
                              + e_a * np.abs(d).sum(0).max())
        out["grad"][wk[i][:-6] + "bias"] = eff(N) * np.abs(d).sum(0).max() + N * e_d
        e_d = eff(W.shape[0]) * (np.abs(d) @ np.abs(W)).max() + e_d * np.abs(W).sum(0).max()
        d = (d @ W) * (a > 0 if i > 0 else 1.0)
    # a table entry = sum over its corners of w d (fixed point: exact sums, one rounding back to fp32)
    for l, r in enumerate(res):
        idx, w, _ = R.level_corners(g["x"], r, T)
        wsum = np.zeros(R.level_rows(r, T))
        np.add.at(wsum, idx.reshape(-1), w.reshape(-1).astype(np.float64))
        ref = g[f"{tag}.grad.position_encoder.encodings.{l}.table"]
        out["grad"][f"position_encoder.encodings.{l}.table"] = e_d * wsum.max() + 2 * u * np.abs(ref).max()
    return out


@pytest.mark.parametrize("tag", ["A", "B"])
def test_model_vs_reference(golden, matmul_precision, tag):
    from nerf_amd import model_ingp2d as M
    g = golden("ingp2d")
    eps = 2.0 ** -24 if matmul_precision == "highest" else 2.0 ** -17
    ours, theirs = _bounds(g, tag, eps), _bounds(g, tag, 2.0 ** -24)
    torch.manual_seed(0)
    model = M.Gigapixel(CONFIGS[tag]["n_hidden"], 64, M.INGPEncoding(*CONFIGS[tag]["enc"]))
    model.load_state_dict({str(k): torch.from_numpy(g[f"{tag}.sd.{k}"]) for k in g[f"{tag}.keys"]})
    model = model.to(DEV)
    x, y = torch.from_numpy(g["x"]).to(DEV), torch.from_numpy(g["y"]).to(DEV)
    feat = model.position_encoder(x)
    assert np.array_equal(feat.detach().cpu().numpy(), g[f"{tag}.features"])
    assert int(model.position_encoder.last_status.item()) == 0
    rgb = model(x)
    tol = ours["rgb"] + theirs["rgb"]
    err = np.abs(rgb.detach().cpu().numpy() - g[f"{tag}.rgb"]).max()
    print(f"{tag} {matmul_precision}: rgb err {err:.3e} bound {tol:.3e}")
    assert err <= tol
    loss = model.training_step((x, y))
    ltol = ours["loss"] + theirs["loss"]
    lerr = abs(loss.item() - float(g[f"{tag}.loss"]))
    print(f"{tag} {matmul_precision}: loss err {lerr:.3e} bound {ltol:.3e}")
    assert lerr <= ltol
    loss.backward()
    worst = (0.0, 0.0)
    gtol = {}
    for k, p in model.named_parameters():
        ref = g[f"{tag}.grad.{k}"]
        gtol[k] = ours["grad"][k] + theirs["grad"][k]
        gerr = np.abs(p.grad.cpu().numpy() - ref).max()
        scale = np.abs(ref).max()
        print(f"{tag} {matmul_precision}: grad {k} err/max {gerr / scale:.3e} bound/max {gtol[k] / scale:.3e}")
        worst = max(worst, (gerr / scale, gtol[k] / scale))
        assert gerr <= gtol[k], k
    print(f"{tag} {matmul_precision}: worst gradient err/max {worst[0]:.3e} (bound/max {worst[1]:.3e})")
    # three FusedAdam steps
    model.zero_grad()
    opt = model.configure_optimizers()["optimizer"]
    assert type(opt).__name__ == "FusedAdam"
    for _ in range(3):
        opt.zero_grad()
        model.training_step((x, y)).backward()
        opt.step()
    lr, u = 1e-3, 2.0 ** -24
    for k, v in model.state_dict().items():
        ref, g1 = g[f"{tag}.adam3.{k}"], np.abs(g[f"{tag}.grad.{k}"])
        bound = 3 * lr * np.minimum(2.0, gtol[k] / (np.maximum(g1 - gtol[k], 0) + 1e-8)) + 3 * 4 * u * (np.abs(ref) + lr)
        perr = np.abs(v.cpu().numpy() - ref)
        print(f"{tag} {matmul_precision}: adam3 {k} err {perr.max():.3e} (largest bound {bound.max():.3e})")
        assert (perr <= bound).all(), k


# ----------------------------------------------------------------------------- fit and render
def test_fit_vs_restatement_and_render():
    """40 full-batch steps on a procedural 64 x 64 image in "highest" against the torch restatement
    with torch Adam from the same init: final losses within 1 % (Nerf2d's criterion)."""
    from nerf_amd import model_ingp2d as M
    res = 64
    loc = M.pixel_centres(res)
    img = torch.stack((0.5 + 0.5 * torch.sin(6 * loc[:, 0]), 0.5 + 0.5 * torch.cos(9 * loc[:, 1]),
                       loc[:, 0] * loc[:, 1]), dim=1)
    torch.manual_seed(0)
    enc = M.INGPEncoding(64, 4, 2 ** 8, 2, 5)
    model = M.Gigapixel(2, 64, enc)
    ref = R.RefGigapixel(2, 64, R.RefEncoding(enc.resolutions, 2 ** 8, 2))
    ref.load_state_dict({k: v.clone() for k, v in model.state_dict().items()})
    prev = torch.get_float32_matmul_precision()
    torch.set_float32_matmul_precision("highest")
    try:
        model = model.to(DEV)
        opt = model.configure_optimizers()["optimizer"]
        xg, yg = loc.to(DEV), img.to(DEV)
        first = model.validation_step((xg, yg)).item()
        for _ in range(40):
            opt.zero_grad()
            model.training_step((xg, yg)).backward()
            opt.step()
        gpu_loss = model.validation_step((xg, yg)).item()
        picture = model.render(res)
        with torch.no_grad():
            flat = model(M.pixel_centres(res, DEV))
        chunked = model.render(res, chunk=1000)
    finally:
        torch.set_float32_matmul_precision(prev)
    opt_c = torch.optim.Adam(ref.parameters(), lr=1e-3)
    for _ in range(40):
        opt_c.zero_grad()
        torch.nn.functional.mse_loss(ref(loc), img).backward()
        opt_c.step()
    with torch.no_grad():
        cpu_loss = torch.nn.functional.mse_loss(ref(loc), img).item()
    print(f"fit: loss {first:.5f} -> {gpu_loss:.6f} (restatement {cpu_loss:.6f})")
    assert math.isfinite(gpu_loss) and gpu_loss < first
    assert abs(gpu_loss - cpu_loss) <= 0.01 * cpu_loss, (gpu_loss, cpu_loss)
    assert picture.shape == (res, res, 3)
    assert torch.equal(picture, flat.view(res, res, 3).permute(1, 0, 2))
    torch.testing.assert_close(chunked, picture, atol=1e-6, rtol=0)
    assert int(model.position_encoder.last_status.item()) == 0
