"""Distortion loss (csrc/distortion.hip: nerf_distortion_fwd / _bwd) and nerf_amd.distortion against
the fp64 direct double sum tests/_packed_train_ref.py::distortion_direct64.

Inputs: the fp32-rounded weights of the packed compositing restatement on packed_inputs(LENGTHS, 7)
with its intervals (all below far = 6).  Bars: loss per ray 2e-6, the compositing bar; gradient
2e-5 + 1e-5 rel, the project's gradient bar.  The contract (fp64 accumulation rounded once to fp32)
lies within 1.4e-8 and 1.2e-7 of the direct sum for these inputs (values up to 0.40 and 2.7;
tests/test_packed_train_logic.py), more than an order of magnitude inside both; the distances measured
on the MI355X are printed (loss 1.4e-8, gradient 1.1e-7).  Outputs go into buffers guarded by a NaN
pattern (tests/_guarded.py).
"""
import numpy as np
import pytest
import torch

import _packed_train_ref as P
from _guarded import Guarded

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _lib():
    import nerf_amd
    nerf_amd._lib.load()  # fail loudly if the HIP library is missing
    yield


@pytest.fixture(scope="module")
def case():
    """The inputs and their fp64 reference, computed once and left unchanged."""
    w, t0, t1, seg, g_loss = P.distortion_case()
    return (w, t0, t1, seg, g_loss), P.distortion_direct64(w, t0, t1, seg, g_loss)


def stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def close(got, ref, what, grad=False):
    atol, rtol = (2e-5, 1e-5) if grad else (2e-6, 0.0)
    got, ref = got.detach().cpu().double().numpy(), ref.numpy()
    err = np.abs(got - ref)
    print(f"{what}: max |err| = {err.max() if err.size else 0.0:.3e} (largest value {np.abs(ref).max():.3f})")
    np.testing.assert_allclose(got, ref, atol=atol, rtol=rtol, err_msg=what)


def test_loss_and_gradient_on_ragged_segments(case):
    import nerf_amd
    (w, t0, t1, seg, g_loss), (ref_loss, ref_grad) = case
    Rn, N = len(P.LENGTHS), w.numel()
    d = [x.to(DEV) for x in (w, t0, t1, seg, g_loss)]
    lib = nerf_amd._lib.load()
    loss, grad = Guarded(Rn), Guarded(N)
    st = lib.nerf_distortion_fwd(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), Rn, N,
                                 loss.ptr(), stream())
    assert st == 0
    loss.check("loss")
    close(loss.body, ref_loss, "loss")
    empty = [i for i, L in enumerate(P.LENGTHS) if L == 0]
    assert torch.all(loss.body[empty].view(torch.int32) == 0)
    st = lib.nerf_distortion_bwd(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), Rn, N,
                                 d[4].data_ptr(), grad.ptr(), stream())
    assert st == 0
    grad.check("d weights")
    close(grad.body, ref_grad, "d weights", grad=True)


def test_public_function_packed(case):
    """nerf_amd.distortion with ray_indices: the raw kernels' values, differentiable in weights only."""
    from nerf_amd import distortion
    (w, t0, t1, seg, g_loss), (ref_loss, ref_grad) = case
    ri = P.ray_indices_of(P.LENGTHS).to(DEV)
    wd = w.to(DEV).requires_grad_(True)
    ts = t0.to(DEV).requires_grad_(True)
    loss = distortion(wd, ts, t1.to(DEV), ri, len(P.LENGTHS))
    assert loss.shape == (len(P.LENGTHS),)
    close(loss, ref_loss, "loss")
    (loss * g_loss.to(DEV)).sum().backward()
    close(wd.grad, ref_grad, "d weights", grad=True)
    assert ts.grad is None


@pytest.mark.parametrize("S", [1, 64, 65])
def test_batched_call_equals_the_packed_call_on_equal_segments(case, S):
    from nerf_amd import distortion
    (w, t0, t1, seg, _), _ = case
    a = int(seg[9])                                        # inside the 1500-sample ray
    Rn = 5
    sl = slice(a, a + Rn * S)
    flat = [x[sl].contiguous().to(DEV) for x in (w, t0, t1)]
    ri = torch.arange(Rn, device=DEV).repeat_interleave(S)
    seg_eq = torch.arange(Rn + 1) * S
    g = torch.randn(Rn, generator=torch.Generator().manual_seed(S)).to(DEV)
    outs = []
    for batched in (True, False):
        wd = flat[0].clone().requires_grad_(True)
        if batched:
            loss = distortion(wd.view(Rn, S), flat[1].view(Rn, S), flat[2].view(Rn, S))
        else:
            loss = distortion(wd, flat[1], flat[2], ri, Rn)
        (loss * g).sum().backward()
        outs.append((loss.detach(), wd.grad))
    assert outs[0][0].shape == (Rn,)
    assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32))
    assert torch.equal(outs[0][1].view(torch.int32), outs[1][1].view(torch.int32))
    ref_loss, ref_grad = P.distortion_direct64(w[sl], t0[sl], t1[sl], seg_eq, g.cpu())
    close(outs[0][0], ref_loss, f"S = {S} loss")
    close(outs[0][1], ref_grad, f"S = {S} d weights", grad=True)


@pytest.mark.parametrize("n_rays", [0, 3])
def test_no_samples(n_rays):
    """N == 0: no launch; the raw entry points store nothing, the public function gives zeros."""
    import nerf_amd
    from nerf_amd import distortion
    lib = nerf_amd._lib.load()
    seg = torch.zeros(n_rays + 1, dtype=torch.int64, device=DEV)
    loss = Guarded(n_rays)
    assert lib.nerf_distortion_fwd(None, None, None, seg.data_ptr(), n_rays, 0, loss.ptr(), stream()) == 0
    assert lib.nerf_distortion_bwd(None, None, None, seg.data_ptr(), n_rays, 0, None, None, stream()) == 0
    torch.cuda.synchronize()
    loss.check("loss", written=False)
    e = torch.zeros(0, device=DEV, requires_grad=True)
    out = distortion(e, e.detach(), e.detach(), torch.zeros(0, dtype=torch.int64, device=DEV), n_rays)
    assert out.shape == (n_rays,) and torch.all(out == 0)
    out.sum().backward()
    assert e.grad.shape == (0,)
