"""Packed compositing (csrc/composite_packed.hip: nerf_composite_packed_fwd / _bwd) and the packed
path of nerf_amd.prop_sampler.rendering against the fp64 restatement tests/_occgrid_ref.py::
packed_composite_ref64 (tests/_raypath_ref.py's composite_ref64 per segment).

Bars: colours, opacity, weights (trans, alphas) 2e-6 abs and gradients 2e-5 abs + 1e-5 rel, the
project's compositing bars (tests/test_gpu_parity.py); depth 2e-6 * far_plane (far = 6), a weight sum
with coefficients of at most far.  tests/test_occgrid_logic.py shows the fp32 torch evaluation of the
same inputs within a third of each of them (depth: 6.7e-7 against 1.2e-5, so that bar is not
widened).  Every output is written into a buffer guarded by a NaN pattern (tests/_guarded.py).
"""
import numpy as np
import pytest
import torch

import _occgrid_ref as R
from _guarded import Guarded

pytestmark = pytest.mark.gpu

DEV = "cuda"
LENGTHS = [0, 1, 63, 64, 65, 0, 0, 128, 129, 1500, 2, 0]
FAR = 6.0
BAR = {"colours": 2e-6, "opacity": 2e-6, "depth": 2e-6 * FAR, "weights": 2e-6, "trans": 2e-6, "alphas": 2e-6}


@pytest.fixture(scope="module", autouse=True)
def _lib():
    import nerf_amd
    nerf_amd._lib.load()  # fail loudly if the HIP library is missing
    yield


@pytest.fixture(scope="module")
def case():
    """The inputs and their fp64 reference, computed once and left unchanged."""
    args = R.packed_inputs(LENGTHS, 11, FAR)
    return args, R.packed_composite_ref64(*args)


def stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def close(got, ref, what, grad=False):
    atol, rtol = (2e-5, 1e-5) if grad else (BAR[what], 0.0)
    got, ref = got.detach().cpu().double().numpy(), ref.numpy()
    err = np.abs(got - ref.reshape(got.shape))
    print(f"{what}: max |err| = {err.max() if err.size else 0.0:.3e}")
    np.testing.assert_allclose(got, ref.reshape(got.shape), atol=atol, rtol=rtol, err_msg=what)


def forward_guarded(sigma, rgb, t0, t1, seg):
    import nerf_amd
    Rn, N = seg.numel() - 1, sigma.numel()
    out = {"colours": Guarded(3 * Rn, named=None if rgb is not None else torch.zeros(3 * Rn, dtype=torch.bool)),
           "opacity": Guarded(Rn), "depth": Guarded(Rn), "weights": Guarded(N), "trans": Guarded(N),
           "alphas": Guarded(N)}
    st = nerf_amd._lib.load().nerf_composite_packed_fwd(
        sigma.data_ptr(), 1, rgb.data_ptr() if rgb is not None else None, 3, t0.data_ptr(), t1.data_ptr(),
        seg.data_ptr(), Rn, N, out["colours"].ptr() if rgb is not None else None, out["opacity"].ptr(),
        out["depth"].ptr(), out["weights"].ptr(), out["trans"].ptr(), out["alphas"].ptr(), stream())
    assert st == 0
    return out


def test_forward_and_backward_on_ragged_segments(case):
    import nerf_amd
    (sigma, rgb, t0, t1, seg, g_rgb, g_op, g_dep, g_w), ref = case
    d = [x.to(DEV) for x in (sigma, rgb, t0, t1, seg)]
    out = forward_guarded(*d)
    Rn, N = len(LENGTHS), sigma.numel()
    for (name, buf), r in zip(out.items(), ref[:6]):
        buf.check(name)
        close(buf.body.view(Rn, 3) if name == "colours" else buf.body, r, name)
    empty = [i for i, L in enumerate(LENGTHS) if L == 0]
    assert torch.all(out["colours"].body.view(Rn, 3)[empty] == 0) and torch.all(out["opacity"].body[empty] == 0)
    assert torch.all(out["depth"].body[empty] == 0)
    first = seg[:-1][torch.tensor(LENGTHS) > 0]
    assert torch.all(out["trans"].body[first.to(DEV)] == 1)
    gs, gc = Guarded(N), Guarded(3 * N)
    g = [x.to(DEV) for x in (g_rgb, g_op, g_dep, g_w)]     # kept alive across the call
    st = nerf_amd._lib.load().nerf_composite_packed_bwd(
        d[0].data_ptr(), 1, d[1].data_ptr(), 3, d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(), Rn, N,
        out["weights"].ptr(), out["trans"].ptr(), g[0].data_ptr(), g[1].data_ptr(), g[2].data_ptr(),
        g[3].data_ptr(), gs.ptr(), 1, gc.ptr(), 3, stream())
    assert st == 0
    gs.check("d sigma")
    gc.check("d rgb")
    close(gs.body, ref[6], "d sigma", grad=True)
    close(gc.body.view(N, 3), ref[7], "d rgb", grad=True)


def test_weights_only_mode(case):
    """rgb = NULL: colours are not touched, the other outputs hold the bits of the full call, and the
    backward gives the density gradient of the opacity / depth / weight terms alone."""
    from nerf_amd import kernels as K
    (sigma, rgb, t0, t1, seg, g_rgb, g_op, g_dep, g_w), _ = case
    d = [x.to(DEV) for x in (sigma, rgb, t0, t1, seg)]
    full = forward_guarded(*d)
    wo = forward_guarded(d[0], None, d[2], d[3], d[4])
    wo["colours"].check("colours", written=False)
    for name in ("opacity", "depth", "weights", "trans", "alphas"):
        wo[name].check(name)
        assert torch.equal(wo[name].body, full[name].body), name
    ref = R.packed_composite_ref64(sigma, None, t0, t1, seg, g_rgb, g_op, g_dep, g_w)
    d_sigma, d_rgb = K.composite_packed_bwd(d[0], None, d[2], d[3], d[4], wo["weights"].body, wo["trans"].body, None,
                                            g_op.to(DEV), g_dep.to(DEV), g_w.to(DEV))
    assert d_rgb is None
    close(d_sigma, ref[6], "d sigma", grad=True)


@pytest.mark.parametrize("n_rays", [0, 3])
def test_no_samples(n_rays):
    """N == 0: every ray is empty and renders zeros; nothing else is stored.  n_rays == 0: no launch."""
    import nerf_amd
    seg = torch.zeros(n_rays + 1, dtype=torch.int64, device=DEV)
    empty = torch.zeros(0, device=DEV)
    out = forward_guarded(empty, torch.zeros(0, 3, device=DEV), empty, empty, seg)
    torch.cuda.synchronize()
    for name, buf in out.items():
        buf.check(name)
        assert torch.all(buf.body == 0)
    st = nerf_amd._lib.load().nerf_composite_packed_bwd(None, 1, None, 3, None, None, seg.data_ptr(), n_rays, 0, None,
                                                        None, None, None, None, None, None, 1, None, 3, stream())
    assert st == 0


def _field(t_starts, t_ends, ray_indices, table):
    """A differentiable per-sample field: rows of `table` [N, 4] -> (rgbs [N, 3], sigmas [N])."""
    rows = table.reshape(-1, 4)
    return torch.sigmoid(rows[:, :3]).reshape(*t_starts.shape, 3), torch.nn.functional.softplus(rows[:, 3]).reshape(
        t_starts.shape)


def test_rendering_accepts_ray_indices_and_matches_the_batched_path():
    """rendering(ray_indices=...) no longer raises (it did before the packed path existed); on equal-
    length segments it agrees with the batched rendering of the same intervals within the forward
    bars (both lie within them of the fp64 value, so twice the bar apart at most; asserted at one
    bar), and its gradients within the gradient bar."""
    from nerf_amd.prop_sampler import rendering
    Rn, S = 37, 70
    g = torch.Generator().manual_seed(5)
    edges = 1.0 + torch.cumsum(torch.rand(Rn, S + 1, generator=g) * 3.2 / S, dim=1)
    t0, t1 = edges[:, :-1].contiguous().to(DEV), edges[:, 1:].contiguous().to(DEV)
    assert float(edges.max()) < FAR
    table = (torch.randn(Rn * S, 4, generator=g) * 2).to(DEV)
    bkgd = torch.tensor([0.2, 0.5, 0.9], device=DEV)
    ray_indices = torch.arange(Rn, device=DEV).repeat_interleave(S)
    g_c, g_o, g_d = (torch.randn(Rn, k, generator=g).to(DEV) for k in (3, 1, 1))
    g_w = torch.randn(Rn, S, generator=g).to(DEV)
    outs = []
    for packed in (False, True):
        tab = table.clone().requires_grad_(True)
        fn = lambda a, b, ri: _field(a, b, ri, tab)
        if packed:
            colors, op, dep, ex = rendering(t0.reshape(-1), t1.reshape(-1), ray_indices, Rn, fn, bkgd)
            assert ex["weights"].shape == (Rn * S,) and ex["rgbs"].shape == (Rn * S, 3)
        else:
            colors, op, dep, ex = rendering(t0, t1, None, None, fn, bkgd)
        assert colors.shape == (Rn, 3) and op.shape == (Rn, 1) and dep.shape == (Rn, 1)
        assert set(ex) == {"weights", "trans", "sigmas", "rgbs", "alphas"} and not ex["trans"].requires_grad
        loss = (colors * g_c).sum() + (op * g_o).sum() + (dep * g_d).sum() + (ex["weights"].reshape(Rn, S) * g_w).sum()
        loss.backward()
        outs.append((colors, op, dep, ex["weights"].reshape(Rn, S), ex["trans"].reshape(Rn, S),
                     ex["alphas"].reshape(Rn, S), tab.grad))
    names = ("colours", "opacity", "depth", "weights", "trans", "alphas")
    for name, a, b in zip(names, outs[0], outs[1]):
        err = float((a - b).detach().abs().max())
        print(f"{name}: batched vs packed max |diff| = {err:.3e}")
        assert err <= BAR[name], name
    ga, gb = outs[0][6], outs[1][6]
    print(f"gradient: max |diff| = {float((ga - gb).abs().max()):.3e}")
    assert torch.all((ga - gb).abs() <= 2e-5 + 1e-5 * ga.abs())


def test_render_weight_from_density_packed_and_batched(case):
    from nerf_amd.prop_sampler import render_weight_from_density
    (sigma, rgb, t0, t1, seg, *_), ref = case
    ri = torch.repeat_interleave(torch.arange(len(LENGTHS)), torch.tensor(LENGTHS)).to(DEV)
    w, T, al = render_weight_from_density(t0.to(DEV), t1.to(DEV), sigma.to(DEV), ri, len(LENGTHS))
    close(w, ref[3], "weights")
    close(T, ref[4], "trans")
    close(al, ref[5], "alphas")
    a, b = int(seg[9]), int(seg[10])                     # the 1500-sample ray as a [3, 500] batch
    args = [x[a:b].reshape(3, 500).to(DEV) for x in (t0, t1, sigma)]
    wb, Tb, _ = render_weight_from_density(*args)
    ref3 = R.packed_composite_ref64(sigma[a:b], None, t0[a:b], t1[a:b], torch.tensor([0, 500, 1000, 1500]))
    close(wb.reshape(-1), ref3[3], "weights")
    close(Tb.reshape(-1), ref3[4], "trans")
    with pytest.raises(ValueError, match="n_rays"):
        render_weight_from_density(t0.to(DEV), t1.to(DEV), sigma.to(DEV), ri)
