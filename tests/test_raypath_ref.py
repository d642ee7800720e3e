"""CPU checks of tests/_raypath_ref.py, the restatements that the GPU edge tests of the stand-alone
compositing and sampling kernels compare against: the references are pinned to the oracle and to
the reference's golden vectors before any kernel is measured with them."""
import numpy as np
import pytest
import torch

from _raypath_ref import (activate32, composite_inputs, composite_ref64, resample_fallback_ref,
                          sample_uniform_ref)
from oracle import nerf_oracle as O


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


@pytest.mark.parametrize("S", [1, 2, 63, 64, 65, 200, 385, 513, 1024])
@pytest.mark.parametrize("sa,sb,shift", [(3.0, 7.0, 0.0), (1.0, 1.0, 1.5)])
def test_composite_ref64_vs_fp32_oracle(S, sa, sb, shift):
    """The fp32 oracle (O.render_rays on fp32 activations) lies within the project's compositing
    bars of the fp64 restatement on the edge tests' inputs: 2e-6 on rgb and weights, 2e-5 + 1e-5 rel
    on the raw-input gradients.  Measured over every S from 1 to 129 and the larger S of the GPU
    sweep: rgb within 5.2e-7, weights within 8.5e-8, gradients within 0.7 % of their bar, so the
    fp32 rounding of the reference alone leaves the kernels a margin of more than three."""
    head, dist, g_rgb, g_w = composite_inputs(9, S, 100 + S)
    rgb, w, d_sigma, d_color = composite_ref64(head, dist, sa, sb, 1, shift, g_rgb, g_w)
    h = head.clone().requires_grad_(True)
    rr, ww = O.render_rays(O.softplus8(h[..., 3] - shift), torch.sigmoid(h[..., :3]), dist, sa, sb)
    np.testing.assert_allclose(rr.detach().numpy(), rgb.numpy(), atol=2e-6, rtol=0)
    np.testing.assert_allclose(ww.detach().numpy(), w.numpy(), atol=2e-6, rtol=0)
    ((rr * g_rgb).sum() + (ww * g_w).sum()).backward()
    ref = torch.cat((d_color, d_sigma.unsqueeze(-1)), dim=-1)
    np.testing.assert_allclose(h.grad.numpy(), ref.numpy(), atol=2e-5, rtol=1e-5)
    # act = 0 on the activated values: the same rgb and weights
    sig, col = activate32(head, shift)
    rgb0, w0, _, _ = composite_ref64((sig, col), dist, sa, sb, 0)
    np.testing.assert_allclose(rgb0.numpy(), rgb.numpy(), atol=2e-6, rtol=0)
    np.testing.assert_allclose(w0.numpy(), w.numpy(), atol=2e-6, rtol=0)


@pytest.mark.parametrize("S", [64, 128, 192])
def test_composite_ref64_vs_golden(golden, S):
    """The reference's own outputs and gradients (tests/golden/composite.npz), at the tolerances
    tests/test_oracle_golden.py holds the fp32 oracle to."""
    g = golden("composite")
    k = f"S{S}"
    t = torch.from_numpy
    rgb, w, d_sigma, d_color = composite_ref64((t(g[f"{k}_sigma"]), t(g[f"{k}_color"])), t(g[f"{k}_dist"]), 3.0,
                                               1 / 3, 0, 0.0, t(g[f"{k}_grgb"]), t(g[f"{k}_gw"]))
    np.testing.assert_allclose(rgb.numpy(), g[f"{k}_rgb"], atol=1e-6, rtol=0)
    np.testing.assert_allclose(w.numpy(), g[f"{k}_w"], atol=1e-6, rtol=0)
    np.testing.assert_allclose(d_sigma.numpy(), g[f"{k}_dsigma"], atol=1e-5, rtol=1e-5)
    np.testing.assert_allclose(d_color.numpy(), g[f"{k}_dcolor"], atol=1e-6, rtol=0)


def test_composite_ref64_threshold_branch_has_finite_gradients():
    """A raw density of 1e4 takes the identity branch of the softplus without a NaN from the
    discarded one; nothing behind that wall receives a gradient."""
    head, dist, g_rgb, g_w = composite_inputs(2, 20, 3)
    head[0, 10:, 3] = 1e4
    dist[0] = dist[0].clamp(min=0.01)
    rgb, w, d_sigma, d_color = composite_ref64(head, dist, 3.0, 7.0, 1, 0.0, g_rgb, g_w)
    for x in (rgb, w, d_sigma, d_color):
        assert torch.isfinite(x).all()
    assert torch.all(d_sigma[0, 11:] == 0) and torch.all(d_color[0, 11:] == 0)


@pytest.mark.parametrize("S", [1, 2, 3, 64, 65, 100, 128, 257, 1000])
def test_sample_uniform_ref_vs_linspace_oracle(S):
    """The equidistant samples against O.linspace_t (torch.linspace of Python doubles, as the
    reference forms them): bit-equal for (near, far) = (2, 8) and (0, 1), which are fp32 values; for
    (0.1, 1/3) within one fp32 ulp of far.  Cause of what remains: the reference forms the last
    sample's position far - D (D = (far - near) / S) from Python doubles, and the kernel's ABI takes
    near and far as fp32, so its double far - D starts from the rounded 1/3 (0.1 rounds the same way
    in both, as torch.linspace's start).

    Before this test the kernel formed far - D in fp32 and rounded step * idx on its own; torch
    fuses start + step * idx into one multiply-add.  That restatement differed from O.linspace_t
    in 8 of 65 and 36 of 257 samples for (2, 8) (by half an ulp of far), and in 2 of 3 for (0, 1)."""
    for near, far in ((2.0, 8.0), (0.0, 1.0)):
        t0, t1 = sample_uniform_ref(5, S, near, far, False, 0.0, 1, 0)
        np.testing.assert_array_equal(t0, O.linspace_t(near, far, S).expand(5, S).numpy())
        assert np.all(t1[:, -1] == np.float32(far)) and np.array_equal(t1[:, :-1], t0[:, 1:])
    near, far = 0.1, 1 / 3
    t0, _ = sample_uniform_ref(5, S, near, far, False, 0.0, 1, 0)
    diff = np.abs(t0.astype(np.float64) - O.linspace_t(near, far, S).expand(5, S).numpy().astype(np.float64))
    assert diff.max() <= ulp32(far)


def test_sample_uniform_ref_streams():
    """Stratified draws stay inside their interval; the per-ray offset is one value per ray, from a
    stream other than the stratified one; the fallback is the offset -1 of the same stream."""
    B, S = 7, 65
    base, _ = sample_uniform_ref(B, S, 2.0, 8.0, False, 0.0, 5, 0)
    D = np.float32(6.0) / np.float32(S)
    t0, _ = sample_uniform_ref(B, S, 2.0, 8.0, True, 0.0, 5, 0)
    u = (t0.astype(np.float64) - base) / D
    assert u.min() > -1e-5 and u.max() < 1 + 1e-5 and u.std() > 0.2
    off, _ = sample_uniform_ref(B, S, 2.0, 8.0, False, 1.0, 5, 0)
    v = (off.astype(np.float64) - base) / D
    assert np.abs(v - v[:, :1]).max() < 1e-4 and len(np.unique(np.round(v[:, 0], 4))) == B
    assert np.abs(v[:, 0] - u[:, 0]).max() > 1e-3
    fb0, fb1 = resample_fallback_ref(B, S, 2.0, 8.0, 5, 0)
    neg, neg1 = sample_uniform_ref(B, S, 2.0, 8.0, False, -1.0, 5, 0)
    np.testing.assert_array_equal(fb0, neg)
    np.testing.assert_array_equal(fb1, neg1)
