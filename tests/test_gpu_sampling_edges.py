"""The sampling kernels (csrc/sampling.hip: nerf_sample_uniform, nerf_resample_pdf modes 0 and 1 and
the batch-wide fallback) at their edge shapes, bit for bit against the fp32 restatements in
tests/_raypath_ref.py and the oracle's resample (oracle.nerf_oracle.sample_t_pdf_weighted).

Nothing here has a tolerance except the comparison of the equidistant samples with the reference's
torch.linspace of Python doubles: equal when near and far are fp32 values ((2, 8)), within one fp32
ulp of far for (0.1, 1/3), whose double 1/3 the fp32 ABI cannot carry
(tests/test_raypath_ref.py::test_sample_uniform_ref_vs_linspace_oracle states the cause).
"""
import functools

import numpy as np
import pytest
import torch

from _raypath_ref import resample_fallback_ref, sample_uniform_ref
from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"
STREAMS = [(5, 0), (2 ** 40 + 3, 2 ** 33 + 1)]   # (seed, counter): the second reaches Philox's high words
KN = [(1, 1), (1, 9), (2, 130), (17, 17), (17, 100), (32, 96), (63, 191), (64, 64), (64, 65), (64, 320),
      (33, 1024)]
FAMILIES = ["sparse", "equal", "onehot", "ties"]


@pytest.fixture(scope="module", autouse=True)
def _lib():
    import nerf_amd
    nerf_amd._lib.load()  # fail loudly if the HIP library is missing
    yield


# ----------------------------------------------------------------------------- sample_uniform
@pytest.mark.parametrize("near,far", [(2.0, 8.0), (0.1, 1 / 3)])
@pytest.mark.parametrize("S", [1, 2, 3, 64, 65, 257])
def test_sample_uniform_bitexact(S, near, far):
    """t_start and t_end of every (stratified, offset_size, seed, counter) combination equal
    sample_uniform_ref: the Philox draws, the per-ray offset's own stream counter ^ 2^63, S = 1."""
    from nerf_amd import kernels as K
    B = 33
    for seed, counter in STREAMS:
        for stratified in (False, True):
            for offset in (0.0, 1.0, -1.0, 0.5):
                t0, t1 = K.sample_uniform(B, S, near, far, stratified, offset, seed, counter, DEV)
                r0, r1 = sample_uniform_ref(B, S, near, far, stratified, offset, seed, counter)
                what = f"stratified={stratified} offset={offset} seed={seed} counter={counter}"
                np.testing.assert_array_equal(t0.cpu().numpy(), r0, err_msg="t_start " + what)
                np.testing.assert_array_equal(t1.cpu().numpy(), r1, err_msg="t_end " + what)


@pytest.mark.parametrize("near,far", [(2.0, 8.0), (0.1, 1 / 3)])
@pytest.mark.parametrize("S", [1, 2, 3, 64, 65, 257])
def test_sample_uniform_vs_reference_linspace(S, near, far):
    from nerf_amd import kernels as K
    B = 33
    t0, t1 = K.sample_uniform(B, S, near, far, False, 0.0, 5, 0, DEV)
    ref = O.linspace_t(near, far, S).expand(B, S).numpy()
    if (near, far) == (2.0, 8.0):
        np.testing.assert_array_equal(t0.cpu().numpy(), ref)
    else:
        diff = np.abs(t0.cpu().numpy().astype(np.float64) - ref.astype(np.float64)).max()
        print(f"S={S}: max |t - linspace| = {diff:.3e}, one ulp of far = {np.spacing(np.float32(far)):.3e}")
        assert diff <= float(np.spacing(np.float32(far)))
    assert torch.all(t1[:, -1] == np.float32(far))


def test_sample_uniform_counters_differ():
    from nerf_amd import kernels as K
    for stratified, offset in ((True, 0.0), (False, 1.0)):
        a, _ = K.sample_uniform(33, 65, 2.0, 8.0, stratified, offset, 5, 0, DEV)
        b, _ = K.sample_uniform(33, 65, 2.0, 8.0, stratified, offset, 5, 1, DEV)
        assert (a != b).float().mean() > 0.9


# ----------------------------------------------------------------------------- resample, modes 0 and 1
def resample_case(Kb, N, family, mode, B=41):
    g = torch.Generator().manual_seed(1000 * Kb + N + 7 * FAMILIES.index(family) + mode)
    tc = torch.sort(2 + torch.rand(B, Kb, generator=g) * 6, dim=1).values
    dist = torch.diff(tc, dim=1, append=torch.full((B, 1), 8.0))
    if family == "sparse":      # as test_gpu_parity.py::test_resample_random_vs_oracle
        w = torch.nn.functional.softplus(torch.randn(B, Kb, generator=g) * 2) * (torch.rand(B, Kb, generator=g) < 0.5)
        w[:, 0] += 1e-3
    elif family == "equal":
        w = torch.full((B, Kb), 0.25)
    elif family == "onehot":
        w = torch.zeros(B, Kb)
        w[torch.arange(B), torch.randint(0, Kb, (B,), generator=g)] = 1.0
    else:                        # small integers: exact ties among the fractional parts
        w = torch.randint(0, 4, (B, Kb), generator=g).float()
        w[:, 0] += (w.sum(dim=1) == 0).float()
    if mode == 1:                # compositing weights: row sums in (0.3, 1]
        target = 1.0 - 0.7 * torch.rand(B, 1, generator=g)
        w = w * (target / w.sum(dim=1, keepdim=True))
    return tc, w, dist


@functools.lru_cache(maxsize=None)
def resample_oracle(Kb, N, family, mode):
    tc, w, dist = resample_case(Kb, N, family, mode)
    r0, r1, ok = O.sample_t_pdf_weighted(tc, w, dist, N, 8.0, mode)
    assert ok and torch.isfinite(r0).all()
    return r0.numpy(), r1.numpy()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("Kb,N", KN)
def test_resample_bitexact(Kb, N, family, mode):
    """Fewer than 64 bins (inactive lanes, rank loops cut at K), no fine samples (N = K), N not a
    multiple of 64, exact ties of the fractional parts: the oracle's t, bit for bit, status 0."""
    from nerf_amd import kernels as K
    tc, w, dist = resample_case(Kb, N, family, mode)
    r0, r1 = resample_oracle(Kb, N, family, mode)
    t0, t1, st = K.resample_pdf(tc.to(DEV), w.to(DEV), dist.to(DEV), N, mode, 2.0, 8.0, 3, 0)
    assert int(st.item()) == 0
    np.testing.assert_array_equal(t0.cpu().numpy(), r0)
    np.testing.assert_array_equal(t1.cpu().numpy(), r1)


# ----------------------------------------------------------------------------- fallback
@pytest.mark.parametrize("bad", ["zero_row", "nan", "inf"])
@pytest.mark.parametrize("seed,counter", STREAMS)
def test_fallback_value_for_value(bad, seed, counter):
    """One ray the reference's validity check rejects sends the whole batch to equidistant samples
    with the per-ray offset -(U' D): status bit 0, and every t as resample_fallback_ref."""
    from nerf_amd import kernels as K
    B, Kb, N = 9, 17, 100
    tc, w, dist = resample_case(Kb, N, "sparse", 0, B=B)
    if bad == "zero_row":
        w[4] = 0
    else:
        w[4, 5] = float(bad)
    t0, t1, st = K.resample_pdf(tc.to(DEV), w.to(DEV), dist.to(DEV), N, 0, 2.0, 8.0, seed, counter)
    assert int(st.item()) == 1
    r0, r1 = resample_fallback_ref(B, N, 2.0, 8.0, seed, counter)
    np.testing.assert_array_equal(t0.cpu().numpy(), r0)
    np.testing.assert_array_equal(t1.cpu().numpy(), r1)


def test_status_bit_1_alone_is_no_fallback():
    from nerf_amd import kernels as K
    Kb, N = 17, 100
    tc, w, dist = resample_case(Kb, N, "sparse", 0)
    r0, r1 = resample_oracle(Kb, N, "sparse", 0)
    status = torch.full((1,), 2, device=DEV, dtype=torch.int32)
    t0, t1, st = K.resample_pdf(tc.to(DEV), w.to(DEV), dist.to(DEV), N, 0, 2.0, 8.0, 3, 0, status=status)
    assert int(st.item()) == 2
    np.testing.assert_array_equal(t0.cpu().numpy(), r0)
    np.testing.assert_array_equal(t1.cpu().numpy(), r1)


# ----------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("Kb,N,mode", [(65, 130, 0), (65, 130, 1), (64, 513, 2)])
def test_refusals(Kb, N, mode):
    """More than 64 bins, or more than 512 samples of the multinomial mode: NERF_ERR_UNSUPPORTED."""
    from nerf_amd import kernels as K
    from nerf_amd._lib import NERF_ERR_UNSUPPORTED
    tc, w, dist = resample_case(Kb, N, "sparse", 0, B=5)
    with pytest.raises(RuntimeError, match=f"status {NERF_ERR_UNSUPPORTED}"):
        K.resample_pdf(tc.to(DEV), w.to(DEV), dist.to(DEV), N, mode, 2.0, 8.0, 3, 0)
