"""The fp64 restatement of the encoding backward kernels (_encode_bwd_ref.py) checks itself, on the
CPU: against fp64 autograd of the oracle's encodings for every case the GPU tests use, fp32-formed
against fp64-formed per-sample quantities, and the conditions on the inputs that make the GPU
comparison able to see a mis-weighted variance term."""
import pytest
import torch

import _encode_bwd_ref as R

RAYS = R.by_name(R.RAY_CASES)
INTEGRATED = R.by_name(R.INTEGRATED_CASES)
FOURIER = R.by_name(R.FOURIER_CASES)

# Cases whose gradient is well enough conditioned in the per-sample quantities for the fp32-formed and
# the fp64-formed restatement to be comparable at 1e-5: one fp32 rounding of a position of size p moves
# the argument p s_k by p s_k 2^-24, and the term it belongs to by as much relative to itself, so the
# levels that carry weight must keep p s_k below about a hundred: few levels, or levels damped by the
# integrated encoding's weight (wide pixels) or by the mask.
WELL_CONDITIONED_RAYS = ["k0_L1_id_q1", "k0_L0_id_q0_null", "k1_diag_s0_L10_id_pw0", "k1_diag_s07_L16_pw1",
                         "k1_dist_s0_L11_id_pw2", "k1_dist_s07_L1_pw0", "k1_diag_s07_L11_mask_pw2",
                         "k1_diag_s0_L16_id_pw1", "k1_diag_s0_L0_id", "k1_diag_s07_L1_id_S1",
                         "k1_dist_s07_L10_id_mask_pw1", "k1_diag_s07_L10_id_pw0", "k1_diag_s07_L11_id_S65_pw2",
                         "k1_diag_s0_L1_pw1", "k1_diag_s07_L16_id_mask_pw0"]
WIDE_DIAGONAL = [c for c in R.RAY_CASES if c.kind == 1 and not c.distribute and c.wide and c.levels > 0]


def _worst(a, b, scale):
    return ((a - b).abs() / scale.clamp_min(1e-300)).max().item()


@pytest.mark.parametrize("name", list(RAYS))
def test_rays_exact_matches_autograd(name):
    """exact=True against fp64 autograd of oracle barf_pe / integrated_pe over compute_positions: at
    most 1e-12 of sum |T_i| per output."""
    c = RAYS[name]
    inp = R.ray_inputs(c)
    ref = R.rays_ref(c, inp, exact=True)
    a_o, a_d = R.rays_autograd(c, inp)
    r_o, r_d = _worst(ref.d_o, a_o, ref.d_o_sum), _worst(ref.d_d, a_d, ref.d_d_sum)
    print(f"{name}: d_origs {r_o:.2e}, d_dirs {r_d:.2e} of sum |T|")
    assert r_o <= 1e-12 and r_d <= 1e-12
    share = ref.share_pos + ref.share_own + ref.share_cross
    assert torch.allclose(share, torch.ones_like(share), atol=1e-12)
    assert (ref.d_o_bound > 0).all() and (ref.d_d_bound > 0).all()


@pytest.mark.parametrize("name", list(INTEGRATED))
def test_integrated_exact_matches_autograd(name):
    c = INTEGRATED[name]
    inp = R.sample_inputs(c)
    ref = R.integrated_ref(c, inp["x"], inp["d"], inp["t0"], inp["t1"], inp["pw"], inp["g"], exact=True)
    a_x, a_d = R.samples_autograd(c, inp)
    r_x, r_d = _worst(ref.dx, a_x, ref.dx_sum), _worst(ref.ddir, a_d, ref.ddir_sum)
    print(f"{name}: dx {r_x:.2e}, ddir {r_d:.2e} of sum |T|")
    assert r_x <= 1e-12 and r_d <= 1e-12


@pytest.mark.parametrize("name", list(FOURIER))
def test_fourier_exact_matches_autograd(name):
    c = FOURIER[name]
    inp = R.sample_inputs(c)
    ref = R.fourier_ref(c, inp["x"], inp["g"], exact=True)
    a_x, _ = R.samples_autograd(c, inp)
    r_x = _worst(ref.dx, a_x, ref.dx_sum)
    print(f"{name}: dx {r_x:.2e} of sum |T|")
    assert r_x <= 1e-12


@pytest.mark.parametrize("name", WELL_CONDITIONED_RAYS)
def test_fp32_formed_matches_fp64_formed(name):
    """The default mode (per-sample quantities formed in fp32) and exact=True are the same formula:
    within 1e-5 of the largest gradient of each output."""
    c = RAYS[name]
    inp = R.ray_inputs(c)
    r32, r64 = R.rays_ref(c, inp), R.rays_ref(c, inp, exact=True)
    e_o = ((r32.d_o - r64.d_o).abs().max() / r64.d_o.abs().max()).item()
    e_d = ((r32.d_d - r64.d_d).abs().max() / r64.d_d.abs().max()).item()
    print(f"{name}: fp32-formed against fp64-formed: d_origs {e_o:.2e}, d_dirs {e_d:.2e}")
    assert e_o <= 1e-5 and e_d <= 1e-5
    # the bound is that of the formula, not of the forming: the two agree closely
    assert torch.allclose(r32.d_d_bound, r64.d_d_bound, rtol=1e-3)


def test_bound_is_tight():
    """The bound stays a small multiple of 1e-6 of sum |T_i| wherever the weight has not underflowed:
    about a thousand times below the 2e-3 the integrated backward was held to."""
    for c in R.RAY_CASES:
        ref = R.rays_ref(c, R.ray_inputs(c))
        worst = max((ref.d_o_bound / ref.d_o_sum).max().item(), (ref.d_d_bound / ref.d_d_sum).max().item())
        print(f"{c.name}: max bound / sum |T| = {worst:.2e}")
        assert worst < 2e-5


def test_wide_pixel_inputs_exercise_the_variance_terms():
    """In the wide-pixel diagonal-variance cases the own-coordinate and the cross group each hold at
    least 1 % of sum |T_i| (over all three groups) in at least 100 d_dirs outputs, and x = vb 4^k / 2
    over unmasked levels exceeds 20 in some sample and stays below 1 in another."""
    own = cross = 0
    x_max = []
    for c in WIDE_DIAGONAL:
        ref = R.rays_ref(c, R.ray_inputs(c))
        own += int((ref.share_own >= 0.01).sum())
        cross += int((ref.share_cross >= 0.01).sum())
        x = torch.where(ref.unmasked, ref.x, torch.zeros_like(ref.x))
        x_max.append(x.amax(dim=(1, 2)))
        print(f"{c.name}: median share own {ref.share_own.median().item():.3f}, cross "
              f"{ref.share_cross.median().item():.3f}; max x per sample {x_max[-1].min().item():.2e} .. "
              f"{x_max[-1].max().item():.2e}")
    x_max = torch.cat(x_max)
    print(f"outputs with own >= 1 %: {own}, cross >= 1 %: {cross}")
    assert own >= 100 and cross >= 100
    assert x_max.max().item() > 20 and x_max.min().item() < 1


def test_narrow_pixels_hide_the_variance_terms():
    """Why the wide pixels: at 1 / 555 the cross group is below 1e-3 of the sum everywhere."""
    c = RAYS["k1_diag_s0_L10_id_narrow"]
    ref = R.rays_ref(c, R.ray_inputs(c))
    assert ref.share_cross.max().item() < 1e-3


def test_pw_modes():
    pw = torch.arange(6.0)
    assert R.expand_pw(pw, 0, 3, 2).tolist() == [0, 0, 1, 1, 2, 2]
    assert R.expand_pw(pw, 1, 3, 2).tolist() == [0, 1, 2, 0, 1, 2]
    assert R.expand_pw(pw, 2, 3, 2).tolist() == [0, 1, 2, 3, 4, 5]
