// Per-element formulas of the per-channel activations, one functor each (load, fwd, bwd, kParams):
//   Gauss  garf/gaussian.py:8-63  (GaussActivation autograd, GaussAct; copy in barf/gaussian.py)
//   Gabor  gaborf/gabor.py:8-64   (GaborActivation autograd, GaborAct)
//   Sarf   sarf/activation.py:40-65 (SarfAct.forward, the cos * exp form it returns)
//   Sine   nerf-siren/linear_sine.py:44-45  (the activation of LinearSine; no parameters)
// The stand-alone kernels (param_act.hip) and the GEMM epilogues (linear_x3.hip) call the same
// functions, so the two routes differ only in the summation order of the column partials.
//
// Gauss, v = s^2 + 1e-6 (s = inv_standard_deviation):
//   forward   y  = exp((-(z*z)) * v)
//   backward  ge = g * exp((-(z*z)) * v)
//             dz = (((-ge) * 2) * z) * v
//             dv_n = sum_m (-ge) * z^2               ds_n = dv_n * (2 * s_n)
// Gabor, v = s^2 + 1e-6 (s = inv_standard_deviation, p = spread):
//   forward   y  = exp((-(z*z)) * v) * cos(p*z)
//   backward  go = (-exp((-(z*z)) * v)) * g
//             dz = go * (((2*cos(pz)) * v) * z + p * sin(pz))
//             dv_n = sum_m (go * z^2) * cos(pz)      ds_n = dv_n * (2 * s_n)
//             dp_n = sum_m (go * z) * sin(pz)
// Sarf, t = |z| + 1e-4, u = t^2, q = u + 1/(f*f), a = f/q (f = frequency, f != 0):
//   forward   y  = cos(a) * exp(-u)
//   backward  dz = g * (exp(-u) * ((sin(a)*f)/(q*q) - cos(a))) * (2 * t * sign(z)),  sign(+-0) = 0
//             df_n = sum_m g * ((-sin(a)) * exp(-u)) * (1/q + 2/((f*f)*(q*q)))
// f == 0 is outside the contract (1/(f*f) is infinite; the reference's own gradient is not
// finite there).  sin / cos through sincos_enc (common.h), exp through expf, IEEE divisions.
//
// The sin / cos argument carries its rounding error along (sincos_arg): one fp32 ulp of p z (up to
// ~25 near initialisation) or of f / q (up to ~8) is 5e-7 .. 2e-6, and it enters y undamped, where
// the Gaussian has a single exp whose argument error is relative to y.  Gabor takes the exact
// product p z as hi + lo (one FMA); Sarf forms t, q and f / q in fp64 and splits the quotient.
// Arguments of 4096 and more (a grown spread or frequency) are wrapped into [-pi, pi] in fp64
// first.  Everything else is fp32 arithmetic in the order written above.
//
// kChain: the first parameter is s of v = s^2 + 1e-6, so its column sum (dv) is finished with the
// chain-rule factor 2 s (param_reduce).
#pragma once
#include "common.h"

namespace nerf {

// sin and cos of hi + lo, |lo| <= 2^-13: sincos_enc(hi) and the first-order term in lo (the
// second-order term lo^2 / 2 is below 7.5e-9).
__host__ __device__ __forceinline__ void sincos_hi_lo(float hi, float lo, float* s, float* c) {
    float s0, c0;
    sincos_enc(hi, &s0, &c0);
    *s = __builtin_fmaf(c0, lo, s0);
    *c = __builtin_fmaf(-s0, lo, c0);
}

// Arguments of 4096 and more.  Below, |lo| <= ulp(hi) / 2 <= 2^-13 and sincos_hi_lo serves as it
// is (every argument of a network near its initialisation).  A spread or a frequency that has
// grown takes the argument further (p z without limit, f / q up to f^3), where lo is no longer
// small (0.03 at 2^19, 128 at 2^31) and a first-order term in it is simply wrong.  There the
// argument, exact in fp64, is first taken into [-pi, pi]: a - k 2pi with k = rint(a / 2pi) and
// 2pi in two fp64 terms under fused multiply-adds (k 2pi_hi exact inside its FMA, the second
// term's error below 1e-20 for |a| < 2^40), and the remainder is split into hi + lo again.
// wrap_2pi returns false for |a| >= 2^40 and for non-finite a: the caller then takes sincos_enc
// of the fp32 argument alone (sincosf: NaN for +-inf and NaN).
constexpr float kSincosArgMax = 4096.0f;

__host__ __device__ __forceinline__ bool wrap_2pi(double* a) {
    if (!(fabs(*a) < 1099511627776.0)) return false;
    const double k = rint(*a * 0.15915494309189535);
    double r = __builtin_fma(k, -6.283185307179586, *a);
    r = __builtin_fma(k, -2.4492935982947064e-16, r);
    *a = r;
    return true;
}

// sin and cos of hi + lo, |lo| <= ulp(hi) / 2 (hi + lo an exact product or quotient)
__host__ __device__ __forceinline__ void sincos_arg(float hi, float lo, float* s, float* c) {
    if (!(fabsf(hi) < kSincosArgMax)) {
        double a = (double)hi + (double)lo;
        if (wrap_2pi(&a)) {
            hi = (float)a;
            lo = (float)(a - (double)hi);
        } else {
            lo = 0.0f;
        }
    }
    sincos_hi_lo(hi, lo, s, c);
}

// the same of an fp64 argument
__host__ __device__ __forceinline__ void sincos_arg(double a, float* s, float* c) {
    bool split = true;
    if (!(fabs(a) < (double)kSincosArgMax)) split = wrap_2pi(&a);
    const float hi = (float)a;
    sincos_hi_lo(hi, split ? (float)(a - (double)hi) : 0.0f, s, c);
}

// GARF's Gaussian.  kKind is the tile GEMM's template value 0; no public `kind` takes it.
struct GaussFn {
    static constexpr int kKind = 0;
    static constexpr int kParams = 1;
    static constexpr bool kChain = true;
    struct P { float v; };
    static __device__ __forceinline__ P load(const float* p0, const float*, int n) {
#pragma clang fp contract(off)
        const float sv = p0[n];
        return P{sv * sv + 1e-6f};
    }
    static __device__ __forceinline__ float fwd(float z, P k) {
#pragma clang fp contract(off)
        return expf((-(z * z)) * k.v);
    }
    static __device__ __forceinline__ float bwd(float g, float z, P k, double& a0, double&) {
#pragma clang fp contract(off)
        const float z2 = z * z;
        const float ge = g * expf((-z2) * k.v);
        a0 += (double)((-ge) * z2);
        return (((-ge) * 2.0f) * z) * k.v;
    }
};

struct GaborFn {
    static constexpr int kKind = NERF_ACT_GABOR;
    static constexpr int kParams = 2;
    static constexpr bool kChain = true;
    struct P { float v, p; };
    static __device__ __forceinline__ P load(const float* p0, const float* p1, int n) {
#pragma clang fp contract(off)
        const float sv = p0[n];
        return P{sv * sv + 1e-6f, p1[n]};
    }
    static __device__ __forceinline__ float fwd(float z, P k) {
#pragma clang fp contract(off)
        float s, c;
        const float a = k.p * z;
        sincos_arg(a, __builtin_fmaf(k.p, z, -a), &s, &c);
        return expf((-(z * z)) * k.v) * c;
    }
    static __device__ __forceinline__ float bwd(float g, float z, P k, double& a0, double& a1) {
#pragma clang fp contract(off)
        float s, c;
        const float a = k.p * z;
        sincos_arg(a, __builtin_fmaf(k.p, z, -a), &s, &c);
        const float z2 = z * z;
        const float go = (-expf((-z2) * k.v)) * g;
        a0 += (double)((go * z2) * c);
        a1 += (double)((go * z) * s);
        return go * ((((2.0f * c) * k.v) * z) + k.p * s);
    }
};

struct SarfFn {
    static constexpr int kKind = NERF_ACT_SARF;
    static constexpr int kParams = 1;
    static constexpr bool kChain = false;
    struct P { float f, r; double rd; };          // frequency, 1 / (f * f) in fp32 and in fp64
    static __device__ __forceinline__ P load(const float* p0, const float*, int n) {
#pragma clang fp contract(off)
        const float f = p0[n];
        return P{f, 1.0f / (f * f), 1.0 / ((double)f * (double)f)};
    }
    // sin and cos of a = f / ((|z| + 1e-4)^2 + 1 / f^2), the quotient formed in fp64
    static __device__ __forceinline__ void sincos_a(float z, P k, float* s, float* c) {
#pragma clang fp contract(off)
        const double td = (double)fabsf(z) + 1e-4;
        const double ad = (double)k.f / (td * td + k.rd);
        sincos_arg(ad, s, c);
    }
    static __device__ __forceinline__ float fwd(float z, P k) {
#pragma clang fp contract(off)
        const float t = fabsf(z) + 1e-4f;
        const float u = t * t;
        float s, c;
        sincos_a(z, k, &s, &c);
        return c * expf(-u);
    }
    static __device__ __forceinline__ float bwd(float g, float z, P k, double& a0, double&) {
#pragma clang fp contract(off)
        const float t = fabsf(z) + 1e-4f;
        const float u = t * t;
        const float q = u + k.r;
        const float q2 = q * q;
        float s, c;
        sincos_a(z, k, &s, &c);
        const float e = expf(-u);
        const float sg = z > 0.0f ? 1.0f : (z < 0.0f ? -1.0f : 0.0f);
        a0 += (double)(g * (((-s) * e) * (1.0f / q + 2.0f / ((k.f * k.f) * q2))));
        return (g * (e * ((s * k.f) / q2 - c))) * ((2.0f * t) * sg);
    }
};

// SIREN's sine (nerf-siren/linear_sine.py:44-45): y = sin(z), dz = g * cos(z), no learnable
// parameter (no column sums, no partial planes).  z is a GEMM output, not an exact product, so
// the argument carries no rounding error of its own to keep: plain sincos_enc.  kKind is an
// internal template value of the tile GEMM; no public entry point takes it as a kind.
struct SineFn {
    static constexpr int kKind = 3;
    static constexpr int kParams = 0;
    static constexpr bool kChain = false;
    struct P {};
    static __device__ __forceinline__ P load(const float*, const float*, int) { return P{}; }
    static __device__ __forceinline__ float fwd(float z, P) {
        float s, c;
        sincos_enc(z, &s, &c);
        return s;
    }
    static __device__ __forceinline__ float bwd(float g, float z, P, double&, double&) {
#pragma clang fp contract(off)
        float s, c;
        sincos_enc(z, &s, &c);
        return g * c;
    }
};

// Column sums of per-slab fp64 partials [slabs][N], in a fixed order (chunks of slabs in parallel,
// 4 strided runs each combined in order, then the chunks in order): dp_n (+)= (float)(sum_i
// partial[i][n]), times (2 * s_n) when s is given (the gradient of s from that of v = s^2 + 1e-6).
// scratch holds param_reduce_scratch(N) bytes.
size_t param_reduce_scratch(int N);
int param_reduce(const double* partial, int64_t slabs, int N, const float* s, float* dp, int accumulate,
                 double* scratch, hipStream_t stream);

// All `params` parameter gradients of one activation from its partial planes (plane p at
// partial + p * plane); chain: the first one takes the factor 2 * p0.
int param_act_reduce(int params, bool chain, const double* partial, int64_t plane, int64_t slabs, int N,
                     const float* p0, float* const* grad, int accumulate, double* scratch, hipStream_t stream);

}  // namespace nerf
