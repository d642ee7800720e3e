"""GPU parity of SIREN's sine (csrc/param_act.hip nerf_sine_act_*, the epilogues of
nerf_linear_sine_x3; the epilogue-against-separate-pass test also runs its siblings, the Gaussian, Gabor and Sarf) and of LinearSine / NerfModel / NerfSiren (nerf_amd/model_siren.py) against the
reference's fixture (tests/golden/siren.npz).

Bounds.  The sine alone: 2e-7 absolute on y (sincos_enc's stated ~1e-7 plus one rounding), and
2e-7 |g| plus one fp32 ulp of dz on dz.  The networks: the sibling families' bounds
(test_gpu_gabor_sarf.py): outputs atol = rtol = 1e-4 at "highest" (fp32 MFMA) and 2e-3 at "high"
(3 x bf16 split), gradients 10 x those; parameter gradients by digest and by sampled entries,
relative to each tensor's largest entry; input gradients (dx, dpos, ddir) with atol = rtol = 10 x the
output bound, as the siblings' are.  Every bound is checked against the fixture's error yardstick
(dev.*: the reference in fp32 and its 3 x bf16 split restatement, both against fp64): the recorded
deviation must sit below one tenth of the bound, so a bound never hides the restatement's error.

One tensor has no tenfold room in absolute terms: dx of the first-layer LinearSine (3 -> 256,
scale = 32) at "high".  That layer multiplies its input by 32, so dx = 32 * (W^T dz) reaches 260, and
the split restatement's own error on it is 8.95e-3 absolute: 0.45 of the 2e-2 bound, 3.4e-5 of the
tensor's maximum.  The comparison keeps the 2e-2 bound; for this one tensor the yardstick assertion is
made in the units of the bounds' own justification (deviation relative to the tensor's largest
entry against a tenth of the tolerance) and the absolute ratio is printed (YARDSTICK_RELATIVE).
"""
import math

import numpy as np
import pytest
import torch

import _siren_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = 0xA5


def g2d(a):
    return torch.from_numpy(np.asarray(a)).to(DEV)


@pytest.fixture(scope="module", autouse=True)
def _lib():
    import nerf_amd
    nerf_amd._lib.load()
    yield


@pytest.fixture(params=["highest", "high"])
def matmul_precision(request):
    old = torch.get_float32_matmul_precision()
    torch.set_float32_matmul_precision(request.param)
    yield request.param
    torch.set_float32_matmul_precision(old)


def _tol(precision):
    return 1e-4 if precision == "highest" else 2e-3


# (tensor, precision) whose yardstick is taken relative to the tensor's largest entry (module docstring)
YARDSTICK_RELATIVE = {("ls0.dx", "high")}


def _yardstick_ok(g, key, precision, bound_abs):
    """The fixture's own deviation for this tensor (fp32 at "highest", split at "high") sits below
    one tenth of the absolute bound used for it."""
    d32, dsplit, big = g[f"dev.{key}"]
    dev = d32 if precision == "highest" else max(d32, dsplit)
    print(f"{key} [{precision}]: fixture deviation {dev:.3e}, bound {bound_abs:.3e}, ratio {dev / bound_abs:.3f}")
    if (key, precision) in YARDSTICK_RELATIVE:
        print(f"{key} [{precision}]: relative to the tensor's largest entry {big:.3e}: {dev / big:.3e}")
        dev = dev / big
    assert dev <= bound_abs / 10, (key, dev, bound_abs)


def _guarded(rows, ld, guard_rows=3):
    """A [rows + guard_rows, ld] fp32 buffer whose every byte holds the sentinel."""
    return torch.full(((rows + guard_rows) * ld * 4,), SENT, dtype=torch.uint8, device=DEV).view(torch.float32) \
        .view(rows + guard_rows, ld)


def _guards_untouched(buf, M, N):
    b = buf.view(torch.uint8).view(buf.shape[0], buf.shape[1], 4)
    return bool((b[M:] == SENT).all()) and bool((b[:, N:] == SENT).all())


# ------------------------------------------------------------------------------- the sine alone
def test_sine_act_vs_fp64():
    """nerf_sine_act_fwd / _bwd on [257, 260] with ragged row strides: z uniform in [-30, 30] plus
    0, +-pi/2, +-pi; against fp64 sin / cos of the same fp32 z."""
    from nerf_amd import kernels as K
    M, N = 257, 260
    gen = torch.Generator().manual_seed(31)
    z = torch.rand(M, N, generator=gen) * 60 - 30
    z[0, :5] = torch.tensor([0.0, math.pi / 2, -math.pi / 2, math.pi, -math.pi])
    gy = torch.randn(M, N, generator=gen)
    zb, yb, gb, dzb, ab = _guarded(M, 263), _guarded(M, 261), _guarded(M, 267), _guarded(M, 262), _guarded(M, 267)
    zb[:M, :N] = z.to(DEV)
    gb[:M, :N] = gy.to(DEV)
    ab[:M, :N] = gy.to(DEV)
    K.sine_act_fwd(zb[:M], N, yb[:M])
    K.sine_act_bwd(gb[:M], zb[:M], N, dzb[:M])
    K.sine_act_bwd(ab[:M], zb[:M], N, ab[:M])                   # grad_z aliases grad_y
    torch.cuda.synchronize()
    for buf in (yb, dzb, ab, zb, gb):
        assert _guards_untouched(buf, M, N)
    assert torch.equal(gb[:M, :N].cpu(), gy) and torch.equal(zb[:M, :N].cpu(), z)      # inputs unchanged
    y, dz = yb[:M, :N].cpu(), dzb[:M, :N].cpu()
    assert torch.equal(ab[:M, :N].cpu(), dz)                    # in place: the same bits
    z64, g64 = z.double(), gy.double()
    err_y = (y.double() - torch.sin(z64)).abs()
    ref_dz = g64 * torch.cos(z64)
    r32 = ref_dz.float().abs()
    ulp = (torch.nextafter(r32, torch.full_like(r32, float("inf"))) - r32).double()
    over = (dz.double() - ref_dz).abs() - (2e-7 * g64.abs() + ulp)
    print(f"sine: max|y - sin| = {err_y.max().item():.3e}, dz over its bound by {over.max().item():.3e}")
    assert err_y.max().item() <= 2e-7
    assert over.max().item() <= 0


def test_sine_act_empty():
    from nerf_amd import kernels as K
    z = torch.empty(0, 8, device=DEV)
    K.sine_act_fwd(z, 8, torch.empty(0, 8, device=DEV))
    K.sine_act_bwd(z, z, 8, torch.empty(0, 8, device=DEV))


FAMILY = ["gauss", "gabor", "sarf"]            # the sine's siblings: the activations with parameters


def _act_params(act, n):
    """Parameters of `act` for n channels in the reference's init ranges (inverse std / frequency in
    [0.5, 2), spread in [0, 2 pi)), as nn.Parameters on the device."""
    gen = torch.Generator().manual_seed(34)
    ps = [torch.rand(n, generator=gen) * 1.5 + 0.5]
    if act == "gabor":
        ps.append(torch.rand(n, generator=gen) * 2 * math.pi)
    return tuple(torch.nn.Parameter(p.to(DEV)) for p in ps)


@pytest.mark.parametrize("act", FAMILY)
def test_act_empty(act):
    """M = 0 for the sine's siblings: nothing to do, and the backward (accumulate = 0) zeroes the
    parameter gradients."""
    lp = _layer(8, 4, act)
    z = torch.empty(0, 8, device=DEV)
    lp.act_fwd(z, torch.empty(0, 8, device=DEV))
    grads = [torch.full((8,), float("nan"), device=DEV) for _ in lp.pact]
    lp.act_bwd(z, z, torch.empty(0, 8, device=DEV), grads)
    for g in grads:
        assert torch.equal(g, torch.zeros(8, device=DEV))


# --------------------------------------------------------------------- epilogue = separate passes
def _layer(n_out, k_in, act="sine"):
    from nerf_amd._lib import NERF_ACT_GABOR, NERF_ACT_SARF
    from nerf_amd.mlp import LayerPlan, Source
    torch.manual_seed(7)
    lin = torch.nn.Linear(k_in, n_out).to(DEV)
    srcs = [Source("pos", 4, 32)] if k_in == 4 else [Source("pos", 256, 256), Source("dir", 4, 32)]
    if act == "sine":
        lp = LayerPlan(lin, srcs, False, sine=True)
    elif act == "gauss":
        lp = LayerPlan(lin, srcs, False, gauss=_act_params(act, n_out)[0])
    else:
        lp = LayerPlan(lin, srcs, False, act=(NERF_ACT_GABOR if act == "gabor" else NERF_ACT_SARF,
                                               _act_params(act, n_out)))
    lp.finalize(torch.device(DEV))
    lp.pack("x3")
    return lp


def _epilogue_and_separate(lp, n_out, k_in, z_range):
    """One layer (M = 257: one full 256-row tile and one ragged row; K = 4, one segment, or 256 + 4,
    two) through the GEMM epilogue and through the GEMM followed by the stand-alone pass.  Asserts
    that z, y and dz of the two routes are bitwise equal and that the parameter gradients agree up
    to the fp64 summation order (rtol 1e-5, atol 1e-6: the bounds of
    test_garf_gauss_epilogue_matches_separate_passes and of the Gabor / Sarf
    test_epilogue_matches_separate_passes).  Gabor's and Sarf's backward epilogue must be refused
    for n_out > 128; the separate pass then runs alone.  Returns (z, y, dz) of the epilogue route,
    dz of the separate pass where the epilogue was refused."""
    from nerf_amd import kernels as K
    from nerf_amd._lib import NERF_EPI_BIAS
    M = 257
    gen = torch.Generator().manual_seed(32)
    a_main = (torch.rand(M, 256, generator=gen) * 2 - 1).to(DEV)
    a_tail = (torch.rand(M, 4, generator=gen) * 2 - 1).to(DEV)
    segs = [(a_tail, 4, 1)] if k_in == 4 else [(a_main, 256, 1), (a_tail, 4, 1)]
    bias = lp.module.bias
    # forward
    z1, y1, z2, y2 = (torch.empty(M, n_out, device=DEV) for _ in range(4))
    assert lp.linear_act_x3(segs, M, lp.Wpx, lp.Kp, n_out, z1, bias=bias, y=y1)
    K.linear_fwd_x3(segs, M, lp.Wpx, lp.Kp, n_out, bias, z2, NERF_EPI_BIAS)
    lp.act_fwd(z2, y2)
    assert torch.equal(z1, z2) and torch.equal(y1, y2)
    # backward: out = act'(z) (A W^T) with a pre-activation of the layer's range
    zpre = ((torch.rand(M, n_out, generator=gen) * 2 - 1) * z_range).to(DEV)
    dz1, g2, dz2 = (torch.empty(M, n_out, device=DEV) for _ in range(3))
    gr1 = [torch.full((n_out,), float("nan"), device=DEV) for _ in lp.pact]
    gr2 = [torch.full((n_out,), float("nan"), device=DEV) for _ in lp.pact]
    fused = lp.linear_act_x3(segs, M, lp.Wpx, lp.Kp, n_out, dz1, z=zpre, grads=gr1)
    assert fused == (lp.act is None or n_out <= 128)
    K.linear_fwd_x3(segs, M, lp.Wpx, lp.Kp, n_out, None, g2, 0)
    lp.act_bwd(g2, zpre, dz2, gr2)
    assert dz2.abs().max().item() > 0 and all(torch.isfinite(g).all() for g in gr2)
    if fused:
        assert torch.equal(dz1, dz2)
        for a, b in zip(gr1, gr2):
            torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6)
    return z1, y1, dz1 if fused else dz2


@pytest.mark.parametrize("k_in", [4, 260])
@pytest.mark.parametrize("n_out", [128, 256, 260])
def test_epilogue_equals_separate_passes(n_out, k_in):
    """nerf_linear_sine_x3, forward and backward, against nerf_linear_fwd_x3 followed by
    nerf_sine_act_*: the same GEMM and the same element function, so bitwise equal.  M = 257: one
    full 256-row tile and one ragged row; K = 4 (one segment) and 256 + 4 (two).  The 256-column
    backward epilogue shipped (no scratch, no spills), so it is tested like the 128-column one;
    N = 260 takes two column blocks (256 + 4) in both modes."""
    z1, y1, dz1 = _epilogue_and_separate(_layer(n_out, k_in), n_out, k_in, 30.0)
    assert (y1 - torch.sin(z1.double()).float()).abs().max().item() <= 2e-7
    assert dz1.abs().max().item() > 0


@pytest.mark.parametrize("k_in", [4, 260])
@pytest.mark.parametrize("n_out", [128, 256, 260])
@pytest.mark.parametrize("act", FAMILY)
def test_epilogue_equals_separate_passes_family(act, n_out, k_in):
    """The same for the Gaussian (nerf_linear_gauss_x3 against nerf_gauss_act_*) and for Gabor and
    Sarf (nerf_linear_act_x3 against nerf_param_act_*), whose backward epilogue exists for
    N <= 128 only: at 256 and 260 it must be refused."""
    _epilogue_and_separate(_layer(n_out, k_in, act), n_out, k_in, 2.0)


def _model_run(m, pos, d, w):
    p = pos.clone().requires_grad_(True)
    dd = d.clone().requires_grad_(True)
    density, rgb = m(p, dd)
    (w * (density + rgb.sum(dim=1))).sum().backward()
    grads = {k: v.grad.clone() for k, v in m.named_parameters()}
    for v in m.parameters():
        v.grad = None
    return density.detach(), rgb.detach(), p.grad, dd.grad, grads


def test_model_epilogue_route_runs_and_equals_separate_passes(golden):
    """NerfModel at "high": every sine layer's forward and backward ran in a GEMM epilogue (all 8,
    the 256-column backward included), and the result is bitwise the separate-pass route's; two
    identical passes are bitwise equal (no atomics anywhere on the route)."""
    from nerf_amd import kernels as K
    from nerf_amd import mlp as mlp_mod
    from nerf_amd import model_siren
    g = golden("siren")
    pos, d, w = g2d(g["model.pos"]), g2d(g["model.dir"]), g2d(g["model.w"])
    prev = torch.get_float32_matmul_precision()
    torch.set_float32_matmul_precision("high")
    calls = []
    orig = K.linear_sine_x3

    def counting(*a, **k):
        ok = orig(*a, **k)
        calls.append(("fwd" if k.get("y") is not None else "bwd", ok))
        return ok
    K.linear_sine_x3 = counting
    try:
        torch.manual_seed(0)
        m = model_siren.NerfModel(32).to(DEV)
        runs = [_model_run(m, pos, d, w), _model_run(m, pos, d, w)]
        fused_calls = list(calls)
        mlp_mod.GAUSS_EPILOGUE = False
        runs.append(_model_run(m, pos, d, w))
    finally:
        K.linear_sine_x3 = orig
        mlp_mod.GAUSS_EPILOGUE = True
        torch.set_float32_matmul_precision(prev)
    assert len(calls) == len(fused_calls) == 32 and all(ok for _, ok in calls)
    assert sum(1 for wh, _ in calls if wh == "fwd") == 16 and sum(1 for wh, _ in calls if wh == "bwd") == 16
    for other in runs[1:]:
        for a, b in zip(runs[0][:4], other[:4]):
            assert torch.equal(a, b)
        for k in runs[0][4]:
            assert torch.equal(runs[0][4][k], other[4][k]), k


# ------------------------------------------------------------------------ against the fixture
def _check_rows(got, g, key, atol, rtol):
    """A [257, n] result against the fixture's stored rows and fp64 row / column sums."""
    rows = R.stored_rows()
    np.testing.assert_allclose(got[rows].cpu().numpy(), g[key], atol=atol, rtol=rtol, err_msg=key)
    n_r, n_c = got.shape
    np.testing.assert_allclose(got.double().sum(dim=1).cpu().numpy(), g[key + ".rowsum"], atol=atol * n_c, rtol=rtol)
    np.testing.assert_allclose(got.double().sum(dim=0).cpu().numpy(), g[key + ".colsum"], atol=atol * n_r, rtol=rtol)


def _check_param_grad(got, g, key, tol):
    """Digest and sampled entries, relative to the tensor's largest entry; 10 x the output bound."""
    big = float(g[key + ".max"])
    ref_sum, ref_abs = g[key + ".digest"]
    assert abs(got.double().abs().sum().item() - ref_abs) <= 10 * tol * ref_abs + 1e-6, key
    assert abs(got.double().sum().item() - ref_sum) <= 10 * tol * ref_abs + 1e-6, key
    sample = got.reshape(-1)[R.sample_idx(got.numel()).to(got.device)].cpu().numpy()
    assert np.abs(sample - g[key + ".sample"]).max() <= 10 * tol * max(big, 1e-30), key
    assert abs(got.abs().max().item() - big) <= 10 * tol * big, key


@pytest.mark.parametrize("case", R.LS_CASES, ids=[c[0] for c in R.LS_CASES])
def test_linear_sine_vs_fixture(golden, case, matmul_precision):
    from nerf_amd import LinearSine
    g = golden("siren")
    key, k, n, first = case
    tol = _tol(matmul_precision)
    torch.manual_seed(0)
    m = LinearSine(k, n, scale=R.linear_sine_scale(key), first_layer=first).to(DEV)
    x = R.linear_sine_input(key, k).to(DEV).requires_grad_(True)
    y = m(x)
    assert y.shape == (R.ROWS, n)
    (y * R.upstream(n).to(DEV)).sum().backward()
    _yardstick_ok(g, f"{key}.y", matmul_precision, tol)
    _yardstick_ok(g, f"{key}.dx", matmul_precision, 10 * tol)
    _yardstick_ok(g, f"{key}.dW", matmul_precision, 10 * tol * float(g[f"{key}.dW.max"]))
    _yardstick_ok(g, f"{key}.db", matmul_precision, 10 * tol * max(1.0, float(np.abs(g[f"{key}.db"]).max())))
    _check_rows(y.detach(), g, f"{key}.y", tol, tol)
    _check_rows(x.grad, g, f"{key}.dx", 10 * tol, 10 * tol)
    _check_param_grad(m.linear.weight.grad, g, f"{key}.dW", tol)
    db = g[f"{key}.db"]
    np.testing.assert_allclose(m.linear.bias.grad.cpu().numpy(), db, atol=10 * tol * max(1.0, np.abs(db).max()),
                               rtol=10 * tol)


def test_model_vs_fixture(golden, matmul_precision):
    from nerf_amd import model_siren
    g = golden("siren")
    tol = _tol(matmul_precision)
    torch.manual_seed(0)
    m = model_siren.NerfModel(32).to(DEV)
    density, rgb, dpos, ddir, grads = _model_run(m, g2d(g["model.pos"]), g2d(g["model.dir"]), g2d(g["model.w"]))
    assert density.shape == (R.ROWS,) and rgb.shape == (R.ROWS, 3)
    for key, bound in (("density", tol), ("rgb", tol), ("dpos", 10 * tol), ("ddir", 10 * tol)):
        _yardstick_ok(g, f"model.{key}", matmul_precision, bound)
    np.testing.assert_allclose(density.cpu().numpy(), g["model.density"], atol=tol, rtol=tol)
    np.testing.assert_allclose(rgb.cpu().numpy(), g["model.rgb"], atol=tol, rtol=tol)
    np.testing.assert_allclose(dpos.cpu().numpy(), g["model.dpos"], atol=10 * tol, rtol=10 * tol)
    np.testing.assert_allclose(ddir.cpu().numpy(), g["model.ddir"], atol=10 * tol, rtol=10 * tol)
    assert sorted(grads) == sorted(str(k) for k in g["model.params"])
    for k, got in grads.items():
        _yardstick_ok(g, f"model.grad.{k}", matmul_precision, 10 * tol * float(g[f"model.grad.{k}.max"]))
        _check_param_grad(got, g, f"model.grad.{k}", tol)


def _siren(g):
    from nerf_amd import NerfSiren
    near, far, fine, coarse = g["siren.args"]
    torch.manual_seed(0)
    return NerfSiren(float(near), float(far), int(fine), int(coarse)).to(DEV)


def test_nerf_siren_vs_fixture(golden, matmul_precision):
    """With the stored t_coarse: t_fine, rgb_coarse and rgb_fine.  A ray whose integer fine-sample
    counts came out differently (a weight within rounding of a .5 boundary) has discretely different
    t_fine: such rays are left out of the rgb_fine comparison and counted; at most 2 of 64."""
    g = golden("siren")
    tol = _tol(matmul_precision)
    m = _siren(g)
    t_coarse = g2d(g["siren.t_coarse"])
    m._sample_t_coarse = lambda batch_size: t_coarse.clone()
    kept = {}
    sample_fine = m._sample_t_fine

    def keep_fine(*a, **k):
        kept["t_fine"] = sample_fine(*a, **k)
        return kept["t_fine"]
    m._sample_t_fine = keep_fine
    with torch.no_grad():
        rgb_fine, rgb_coarse = m(g2d(g["siren.origins"]), g2d(g["siren.dirs"]))
    for key in ("rgb_coarse", "rgb_fine", "t_fine"):
        _yardstick_ok(g, f"siren.{key}", matmul_precision, tol)
    np.testing.assert_allclose(rgb_coarse.cpu().numpy(), g["siren.rgb_coarse"], atol=tol, rtol=tol)
    t_fine = kept["t_fine"].cpu().numpy()
    assert t_fine.shape == g["siren.t_fine"].shape
    # a changed count moves samples by a fraction of a coarse bin (>= 1e-3 here); rounding by ~1e-7
    moved = np.abs(t_fine - g["siren.t_fine"]).max(axis=1) > 1e-4
    print(f"rays with different fine-sample counts: {int(moved.sum())} of {moved.size}")
    assert moved.sum() <= 2
    np.testing.assert_allclose(t_fine[~moved], g["siren.t_fine"][~moved], atol=tol, rtol=tol)
    np.testing.assert_allclose(rgb_fine.cpu().numpy()[~moved], g["siren.rgb_fine"][~moved], atol=tol, rtol=tol)


def test_nerf_siren_training_step(golden):
    """training_loss + backward + one Adam step: every parameter of both networks receives a
    gradient and stays finite; the scheduler steps."""
    g = golden("siren")
    m = _siren(g)
    o, d = g2d(g["siren.origins"]), g2d(g["siren.dirs"])
    colors = torch.rand(o.shape[0], 3, generator=torch.Generator().manual_seed(33)).to(DEV)
    cfg = m.configure_optimizers()
    opt, sched = cfg["optimizer"], cfg["lr_scheduler"]
    before = {k: v.detach().clone() for k, v in m.named_parameters()}
    loss, parts = m.training_loss(o, d, colors)
    assert set(parts) == {"loss_coarse", "loss_fine"} and torch.isfinite(loss)
    opt.zero_grad()
    loss.backward()
    assert len(before) == 40
    for k, v in m.named_parameters():
        assert v.grad is not None and torch.isfinite(v.grad).all(), k
    opt.step()
    sched.step()
    assert opt.param_groups[0]["lr"] == pytest.approx(1e-4 * 0.5)
    changed = 0
    for k, v in m.named_parameters():
        assert torch.isfinite(v).all(), k
        changed += int(not torch.equal(v, before[k]))
    assert changed > 0
