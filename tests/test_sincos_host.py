"""Host sweep of sincos_enc (csrc/common.h), the one sine / cosine of every hot path (the encodings of
encode.hip / encode_common.h / mlp_fused.hip, Gabor and Sarf through param_act.h, SIREN's sine and its
GEMM epilogue).  CPU only: hipcc compiles the function's own source (`__host__ __device__`) into the
stand-alone tests/host/sincos_sweep.hip, which runs here; nothing touches a GPU.  The fast path is
rintf, fmaf and fp32 multiplies only, so the device computes the same bits.

What is walked: EVERY fp32 bit pattern of [2^12, T), T = kSincosFastMax, the limit of the fast path
(7 binades, 5.9e7 values, none left out; split over up to 8 threads, a few seconds per variant with the
compile), and every 61st pattern of (0, 2^12), subnormals included; each with its negative.  Both
reductions (the default three-term fp32 Cody-Waite and -DNERF_SINCOS_FP64_REDUCTION).

Bounds: 1e-7 absolute on sin and on cos against fp64, the figure common.h and DESIGN.md state, with no
input excluded; sincos_enc(-x) = (-s, c) bit for bit for every value walked; |x| >= T, +-inf and NaN
give sincosf's own bits.

The same program runs sincos_arg (csrc/param_act.h: the Gabor / Sarf argument carried as hi + lo) on
1.4e6 seeded exact products and as many fp64 arguments with magnitudes from 2^-4 to 2^40, against fp64
sin / cos of the exact argument.  Its bound is sincos_enc's swept 9.5e-8, plus half an fp32 ulp of a
result in [0.5, 1] for the rounding of the first-order FMA (2^-24 = 6.0e-8), plus the second-order term
lo^2 / 2 <= 7.5e-9: 1.62e-7, on the first-order path (|a| < 4096) and on the fp64-wrapped one alike
(measured: 1.14e-7 and 1.18e-7); no result exceeds 1 in magnitude; past 2^40 and for non-finite
arguments it is sincosf of the fp32 argument."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "nerf-experiments_amd")
HIPCC = "/opt/rocm/bin/hipcc"
BOUND = 1e-7
ARG_BOUND = 9.5e-8 + 2.0 ** -24 + 7.5e-9


def _build_and_run(tmp_path, variant, defines):
    exe = str(tmp_path / f"sincos_sweep_{variant}")
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "include"), "-I",
           os.path.join(PKG, "csrc"), *defines, os.path.join(ROOT, "tests", "host", "sincos_sweep.hip"), "-o", exe,
           "-pthread"]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    out = subprocess.run([exe], check=True, capture_output=True, timeout=600, text=True).stdout
    print(out)
    return out


def _parse(out):
    r = {"edges": []}
    for ln in out.splitlines():
        f = ln.split()
        if f[0] in ("exhaustive", "strided"):
            if f[1] in ("max_sin_err", "max_cos_err"):
                r[f"{f[0]}.{f[1]}"] = (float(f[2]), f[4], float(f[5]))
            else:
                r[f"{f[0]}.{f[1]}"] = int(f[2])
        elif f[0] == "arg":
            r[f"arg.{f[1]}"] = float(f[2])
        elif f[0] == "T":
            r["T"], r["T.bits"] = float(f[1]), int(f[2], 16)
        elif f[0] == "edge":
            r["edges"].append((f[1], float(f[3]), f[4]))
        else:
            r[f[0]] = f[1]
    return r


@pytest.mark.parametrize("variant,defines", [("fp32", []), ("fp64", ["-DNERF_SINCOS_FP64_REDUCTION"])])
def test_sincos_enc_host_sweep(tmp_path, variant, defines):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    r = _parse(_build_and_run(tmp_path, variant, defines))
    assert r["reduction"] == variant
    T = r["T"]
    assert T >= 2.0 ** 15                                         # the sweep is not emptied by a small limit
    # every value was visited: each bit pattern of [2^12, T), every 61st of the 0x45800000 - 1 below
    assert r["exhaustive.n"] == r["T.bits"] - 0x45800000
    assert r["strided.n"] == (0x45800000 - 1 + 60) // 61
    for part in ("exhaustive", "strided"):
        for which in ("max_sin_err", "max_cos_err"):
            err, bits, x = r[f"{part}.{which}"]
            assert err <= BOUND, f"{part} {which} = {err:.3e} at x = {x!r} ({bits})"
        assert r[f"{part}.asymmetric"] == 0
        assert r[f"{part}.unbounded"] == 0
    assert r["arg.n"] == 43 * 2 ** 15
    for k in ("first_order_product", "first_order_fp64", "wrapped_product", "wrapped_fp64"):
        assert 0 < r[f"arg.{k}"] <= ARG_BOUND, k
    assert r["arg.unbounded"] == 0 and r["arg.far_not_libm"] == 0
    edges = r["edges"]
    assert len([e for e in edges if e[0] == "below_T"]) == 8
    assert len([e for e in edges if e[0] == "above_T"]) == 16 + 5 + 2
    assert len([e for e in edges if e[0] == "nonfinite"]) == 3
    for what, x, path in edges:
        if what == "below_T":
            assert abs(x) < T
        else:
            assert path == "libm", (what, x, path)                # |x| >= T, +-inf, NaN: sincosf's own bits
            assert not abs(x) < T
