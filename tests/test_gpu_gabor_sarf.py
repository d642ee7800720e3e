"""GPU parity of the Gabor / Sarf activations (csrc/param_act.hip, the epilogues of
nerf_linear_act_x3) and the GaborF / SARF field networks against the reference's fixtures
(tests/golden/gaborf.npz, sarf.npz) and an fp64 restatement of the formulas (_gabor_sarf_ref.py).

Bounds: the activation alone is held to the reference's own fp32 error on the same inputs
(4 x max|ref fp32 - ref fp64| + 1e-7 of scale, both from the fixture: sincos_enc's ~1e-7 absolute
error against libm's ulp, expf ulps and another operation order); the networks to the GARF bounds
(1e-4 fp32 MFMA / 2e-3 3 x bf16 split on outputs, 10 x on gradients).
"""
import copy
import functools
import math

import numpy as np
import pytest
import torch

from _gabor_sarf_ref import INIT, KINDS, PARAMS, TorchAct, act_bwd, act_fwd, modules

pytestmark = pytest.mark.gpu

DEV = "cuda"
FAMILIES = ["gaborf", "sarf"]
RAGGED = FAMILIES + ["garf"]          # the ragged multi-slab launch also runs GARF's Gaussian (same kernels)


def _gauss_fwd(z, s):
    return torch.exp((-(z * z)) * (s * s + 1e-6))


def _gauss_bwd(g, z, s):
    """garf/gaussian.py:8-31 and the backward of s ** 2: (dz, ds)."""
    v = s * s + 1e-6
    ge = g * torch.exp((-(z * z)) * v)
    return -ge * 2 * z * v, (-ge * z * z).sum(0) * (2 * s)


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


def _net(family, name, *extra):
    mod, _ = modules(family)
    return getattr(mod, "RadianceNetwork" if name == "radiance" else "ProposalNetwork")(*INIT[family], *extra)


@pytest.mark.parametrize("family", FAMILIES)
def test_activation_vs_fixture(golden, family):
    """Forward and every gradient, every element, against the reference run in fp64; the bound is
    the reference's own fp32 error on these inputs (read from the fixture)."""
    _, act_cls = modules(family)
    g = golden(family)
    act = act_cls(48, 0.5, 2.0).to(DEV)
    with torch.no_grad():
        for p in PARAMS[family]:
            getattr(act, p).copy_(g2d(g[f"act.{p}"]))
    z = g2d(g["act.z"]).requires_grad_(True)
    y = act(z)
    (y * g2d(g["act.gy"])).sum().backward()
    got = {"y": y.detach(), "dz": z.grad}
    got.update({f"d_{p}": getattr(act, p).grad for p in PARAMS[family]})
    for n, t in got.items():
        ref64 = g[f"act.{n}.f64"]
        ref_err = np.abs(g[f"act.{n}"].astype(np.float64) - ref64).max()
        err = np.abs(t.cpu().numpy().astype(np.float64) - ref64).max()
        bound = 4 * ref_err + 1e-7 * np.abs(ref64).max()
        print(f"{family} {n}: max|HIP - f64| = {err:.3e}, reference fp32 error {ref_err:.3e}, bound {bound:.3e}")
        assert err <= bound, (n, err, bound)
    if family == "sarf":
        zc = g["act.z"]
        assert (zc[0, :2] == 0).all()
        assert (z.grad[0, :2] == 0).all()          # sign(+-0) = 0: exactly zero


@functools.lru_cache(maxsize=None)
def _ragged(family):
    """Computed once per family (Gabor, Sarf, and GARF's Gaussian through nerf_gauss_act_*), shared
    by the two tests below.  M = 33,281 = 65 x 512 + 1 rows:
    the kernels cut them into ceil(M / 512) = 66 slabs of ceil(M / 66) = 505 rows, the last one of
    456 (no one-row slab is launched), which is more than 64 slabs, so the
    reduction takes its second level with two chunks.  N = 37: one ragged column block, no multiple
    of 4.  Padded buffers (ld = 40) with NaN guard rows and columns, backward in place, two
    backward runs.  z, grad_y = randn as in GaussAct's large test;
    parameters in the reference's init ranges (inverse std / frequency in [0.5, 2), spread in
    [0, 2 pi)).  Checks the guards and the run-to-run bit-identity; returns the results, the fp64
    restatement and the restatement evaluated by torch in fp32."""
    from nerf_amd import kernels as K
    torch.manual_seed(12)
    M, N, LD, GR = 33_281, 37, 40, 3
    z = torch.randn(M, N)
    gy = torch.randn(M, N)
    if family == "gaborf":
        ps = [torch.rand(N) * 1.5 + 0.5, torch.rand(N) * 2 * math.pi]
    else:
        ps = [torch.rand(N) * 1.5 + 0.5]
    psd = [p.to(DEV) for p in ps]
    nan = float("nan")
    zb = torch.full((M + GR, LD), nan, device=DEV)
    zb[:M, :N] = z.to(DEV)
    yb = torch.full((M + GR, LD), nan, device=DEV)
    if family == "garf":
        fwd = lambda z_, y_: K.gauss_act_fwd(z_, N, psd[0], y_)
        bwd = lambda g_, z_, dz_, gr: K.gauss_act_bwd(g_, z_, N, psd[0], dz_, gr[0])
        ref_fwd, ref_bwd = _gauss_fwd, _gauss_bwd
    else:
        fwd = lambda z_, y_: K.param_act_fwd(KINDS[family], z_, N, psd, y_)
        bwd = lambda g_, z_, dz_, gr: K.param_act_bwd(KINDS[family], g_, z_, N, psd, dz_, gr)
        ref_fwd, ref_bwd = functools.partial(act_fwd, family), functools.partial(act_bwd, family)
    fwd(zb[:M], yb[:M])
    runs = []
    for _ in range(2):
        gb = torch.full((M + GR, LD), nan, device=DEV)
        gb[:M, :N] = gy.to(DEV)
        grads = [torch.empty(N, device=DEV) for _ in ps]
        bwd(gb[:M], zb[:M], gb[:M], grads)                              # grad_z == grad_y
        runs.append((gb, grads))
    for buf in (yb, runs[0][0], runs[1][0]):
        assert torch.isnan(buf[M:]).all() and torch.isnan(buf[:, N:]).all()      # guards untouched
        assert torch.isfinite(buf[:M, :N]).all()
    assert torch.equal(runs[0][0][:M, :N], runs[1][0][:M, :N])
    for a, b in zip(runs[0][1], runs[1][1]):
        assert torch.equal(a, b)                   # fixed-order reduction: bit-identical
    z64, g64, p64 = z.double(), gy.double(), [p.double() for p in ps]
    ref = (ref_fwd(z64, *p64),) + tuple(ref_bwd(g64, z64, *p64))
    ref32 = (ref_fwd(z, *ps),) + tuple(ref_bwd(gy, z, *ps))
    got = (yb[:M, :N].cpu(), runs[0][0][:M, :N].cpu()) + tuple(t.cpu() for t in runs[0][1])
    return got, ref, ref32


@pytest.mark.parametrize("family", FAMILIES)
def test_ragged_multi_slab_guards_determinism_and_fp32_yardstick(family):
    """Ragged and multi-slab launch: NaN guard rows / columns untouched, in-place backward, two runs
    bit-identical (all asserted in _ragged), and every output within the yardstick of
    test_activation_vs_fixture, here against torch's fp32 evaluation of the same formulas:
    max|HIP - f64| <= 4 x max|torch fp32 - f64| + 1e-7 of scale."""
    got, ref, ref32 = _ragged(family)
    for n, a, b, b32 in zip(["y", "dz"] + [f"d_{p}" for p in PARAMS[family]], got, ref, ref32):
        err = (a.double() - b).abs().max().item()
        bound = 4 * (b32.double() - b).abs().max().item() + 1e-7 * b.abs().max().item()
        assert err <= bound, (n, err, bound)


@pytest.mark.parametrize("family", RAGGED)
def test_ragged_multi_slab(family):
    """The same launch against the fp64 restatement with GaussAct's large-test bounds
    (test_gpu_garf_ipe.py:119-121: y 1e-7 + 1e-6 rel, dz 1e-6 + 1e-5 rel, parameter gradients
    1e-3 + 1e-4 rel).  A plain fp32 evaluation of these formulas misses the y / dz bounds (torch's
    fp32 run of the reference's own expressions is over them by up to 5.8e-7 / 8.8e-6, printed below):
    one fp32 ulp of the cos / sin argument (p z up to ~25, f / q up to ~8) enters y undamped.  The
    kernels therefore carry the argument's rounding error along (csrc/param_act.h, sincos_arg)."""
    got, ref, ref32 = _ragged(family)
    names = ["y", "dz"] + [f"d_{p}" for p in PARAMS.get(family, ("inv_standard_deviation",))]
    tols = [(1e-7, 1e-6), (1e-6, 1e-5)] + [(1e-3, 1e-4)] * (len(names) - 2)
    worst = []
    for n, a, b, b32, (atol, rtol) in zip(names, got, ref, ref32, tols):
        over = ((a.double() - b).abs() - (atol + rtol * b.abs())).max().item()
        over32 = ((b32.double() - b).abs() - (atol + rtol * b.abs())).max().item()
        print(f"{family} {n}: max|HIP - f64| = {(a.double() - b).abs().max().item():.3e} "
              f"(torch fp32: {(b32.double() - b).abs().max().item():.3e}), over the bound by {over:.3e} "
              f"(torch fp32: {over32:.3e})")
        worst.append((n, over))
    for n, over in worst:
        assert over <= 0, (n, over)


@pytest.mark.parametrize("name", ["radiance", "proposal"])
@pytest.mark.parametrize("family", FAMILIES)
def test_networks_vs_fixture(golden, family, name, matmul_precision):
    mod, _ = modules(family)
    g = golden(family)
    torch.manual_seed(0)
    m = _net(family, name)
    ref_key = dict(zip(mod.strip_compile_prefix({str(k): None for k in g[f"{name}.keys"]}).keys(),
                       (str(k) for k in g[f"{name}.keys"])))
    for k, v in m.state_dict().items():
        ref = g[f"{name}.sdsum.{ref_key[k]}"]
        assert abs(v.double().abs().sum().item() - ref[1]) <= 1e-9 * max(1.0, ref[1]), k
    m = m.to(DEV)
    tol = 1e-4 if matmul_precision == "highest" else 2e-3
    pos = g2d(g["pos"]).requires_grad_(True)
    if name == "radiance":
        d = g2d(g["dir"]).requires_grad_(True)
        rgb, dens = m(pos, d)
        np.testing.assert_allclose(rgb.detach().cpu().numpy(), g["radiance.rgb"], atol=tol, rtol=tol)
        np.testing.assert_allclose(dens.detach().cpu().numpy(), g["radiance.density"], atol=tol, rtol=tol)
        ((rgb * g2d(g["radiance.gc"])).sum() + (dens * g2d(g["radiance.gd"])).sum()).backward()
        np.testing.assert_allclose(d.grad.cpu().numpy(), g["radiance.ddir"], atol=10 * tol, rtol=10 * tol)
    else:
        dens = m(pos)
        assert dens.shape == (pos.shape[0], 1)
        np.testing.assert_allclose(dens.detach().cpu().numpy(), g["proposal.density"], atol=tol, rtol=tol)
        (dens * g2d(g["proposal.gd"])).sum().backward()
    np.testing.assert_allclose(pos.grad.cpu().numpy(), g[f"{name}.dpos"], atol=10 * tol, rtol=10 * tol)
    for k, prm in m.named_parameters():
        s = g[f"{name}.gradsum.{ref_key[k]}"]
        assert abs(prm.grad.double().abs().sum().item() - s[1]) <= 10 * tol * s[1] + 1e-6, k
        key = f"{name}.grad.{ref_key[k]}"
        if key in g:
            np.testing.assert_allclose(prm.grad.cpu().numpy(), g[key],
                                       atol=10 * tol * max(1.0, np.abs(g[key]).max()), rtol=10 * tol)


@pytest.mark.parametrize("name", ["radiance", "proposal"])
@pytest.mark.parametrize("family", FAMILIES)
def test_epilogue_matches_separate_passes(family, name):
    """The activation fused into the split-precision GEMM epilogues (forward: every eligible layer,
    the 1024- and 512-wide ones in 256-column blocks; backward: the layers of <= 128 outputs with one
    consumer) against the separate nerf_param_act passes on the same GEMMs: outputs, dpos and every
    Linear gradient bit-identical, activation-parameter gradients equal up to the fp64 summation
    order.  M = 8,321 = 65 x 128 + 1: ragged 256-row tiles and two reduction chunks."""
    from nerf_amd import kernels as K
    from nerf_amd import mlp as mlp_mod
    torch.manual_seed(3)
    M = 8_321
    pos = (torch.rand(M, 3) * 2 - 1).to(DEV)
    d = torch.nn.functional.normalize(torch.randn(M, 3), dim=-1).to(DEV)
    gc, gd = torch.randn(M, 3).to(DEV), torch.randn(M, 1).to(DEV)
    prev = torch.get_float32_matmul_precision()
    torch.set_float32_matmul_precision("high")
    results = []
    calls = []
    orig = K.linear_act_x3

    def counting(*a, **k):
        ok = orig(*a, **k)
        calls.append(("fwd" if k.get("y") is not None else "bwd", ok))
        return ok
    K.linear_act_x3 = counting
    try:
        for fused in (True, False):
            mlp_mod.GAUSS_EPILOGUE = fused
            torch.manual_seed(0)
            m = _net(family, name).to(DEV)
            p = pos.clone().requires_grad_(True)
            if name == "radiance":
                rgb, dens = m(p, d)
                loss = (rgb * gc).sum() + (dens * gd).sum()
                outs = [rgb.detach(), dens.detach()]
            else:
                dens = m(p)
                loss = (dens * gd).sum()
                outs = [dens.detach()]
            loss.backward()
            results.append((outs, p.grad.clone(), {k: v.grad.clone() for k, v in m.named_parameters()}))
            if fused:
                n_fused = list(calls)
    finally:
        K.linear_act_x3 = orig
        mlp_mod.GAUSS_EPILOGUE = True
        torch.set_float32_matmul_precision(prev)
    # the fused route ran (and only when switched on): every activation layer forward, some backward
    assert len(calls) == len(n_fused)
    assert sum(1 for w, ok in n_fused if w == "fwd" and ok) == (8 if name == "radiance" else 3)
    assert any(w == "bwd" and ok for w, ok in n_fused)
    (o1, dp1, g1), (o2, dp2, g2) = results
    for a, b in zip(o1, o2):
        assert torch.equal(a, b)
    assert torch.equal(dp1, dp2)
    for k in g1:
        if k.rsplit(".", 1)[1] in PARAMS[family]:
            torch.testing.assert_close(g1[k], g2[k], rtol=1e-5, atol=1e-6, msg=k)
        else:
            assert torch.equal(g1[k], g2[k]), k


def _torch_radiance(family, m):
    """The radiance network as plain fp64 torch modules over the restated activation."""
    _, act_cls = modules(family)
    seqs = []
    for seq in (m.model_density_1, m.model_density_2, m.model_color):
        seqs.append(torch.nn.Sequential(*[
            TorchAct(family, [getattr(x, p) for p in PARAMS[family]]) if isinstance(x, act_cls) else copy.deepcopy(x)
            for x in seq]).double())
    net = torch.nn.ModuleList(seqs)

    def forward(pos, d):
        z1 = seqs[0](pos)
        z2 = seqs[1](torch.cat((z1, pos), dim=1))
        density = torch.nn.functional.softplus(z2[:, 128] - 1, threshold=8)
        return seqs[2](torch.cat((z1[:, :128] + z2[:, :128], d), dim=1)), density
    return net, forward


def test_training_direction(matmul_precision):
    """Three Adam steps (FusedAdam) on the Gabor radiance network, M = 1,024 in two half batches
    whose gradients accumulate in .grad, against the same steps of torch.optim.Adam on an fp64 torch
    copy with the restated activation: the loss sequences agree within the network bound."""
    from nerf_amd import FusedAdam
    torch.manual_seed(0)
    m = _net("gaborf", "radiance")
    net, ref_forward = _torch_radiance("gaborf", m)
    m = m.to(DEV)
    g = torch.Generator().manual_seed(5)
    M = 1_024
    pos = torch.rand(M, 3, generator=g) * 2 - 1
    d = torch.nn.functional.normalize(torch.randn(M, 3, generator=g), dim=1)
    target = torch.rand(M, 3, generator=g)
    w = torch.rand(M, generator=g) * 0.1

    def loss_of(forward, sl, dev, dt):
        rgb, dens = forward(pos[sl].to(dev, dt), d[sl].to(dev, dt))
        return ((rgb - target[sl].to(dev, dt)) ** 2).sum() / M + (dens.reshape(-1) * w[sl].to(dev, dt)).sum() / M

    halves = (slice(0, M // 2), slice(M // 2, M))
    seqs = []
    for forward, params, opt_cls, dev, dt in ((m, list(m.parameters()), FusedAdam, DEV, torch.float32),
                                              (ref_forward, list(net.parameters()), torch.optim.Adam, "cpu",
                                               torch.float64)):
        opt = opt_cls(params, lr=5e-4, eps=1e-5)
        losses = []
        for _ in range(3):
            opt.zero_grad(set_to_none=False)
            total = 0.0
            for sl in halves:
                loss = loss_of(forward, sl, dev, dt)
                loss.backward()
                total += loss.item()
            opt.step()
            losses.append(total)
        seqs.append(losses)
    tol = 1e-4 if matmul_precision == "highest" else 2e-3
    print("losses", seqs)
    assert seqs[0][0] != seqs[0][2]
    np.testing.assert_allclose(seqs[0], seqs[1], atol=tol, rtol=tol)
