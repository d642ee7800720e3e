// Alpha compositing of packed samples: rays own segments [seg[r], seg[r+1]) of any length of one flat
// sample list (the output of an occupancy-grid sampler), forward and backward.
//
// The arithmetic is composite.hip's with density factor 1 and no activation:
//   b_i = -sigma_i * (t_end_i - t_start_i),  T_i = exp(sum of b over the ray's earlier samples)
//   (fp64 prefix, rounded to fp32; 1 for the ray's first sample),  alpha_i = -expm1(b_i),
//   w_i = T_i * alpha_i;  colors = sum w c, opacity = sum w, depth = sum w (t_start + t_end) / 2.
// alpha is formed with expm1f, not as 1 - expf(b): a marched ray has many thin samples (|b| ~ 1e-3),
// where 1 - expf(b) keeps an absolute error of an ulp of 1 per sample; summed over the 1500 samples of
// one ray that put the opacity 2.2e-6 from the fp64 value on the device (bar 2e-6), expm1f keeps it
// relative to alpha.
// One 64-lane wavefront per ray walks its segment in 64-sample chunks: one fp64 DPP wave scan per
// chunk plus the running fp64 total of the earlier chunks.  The backward walks the chunks in reverse
// with a running fp64 suffix sum of g_w * w and reads the saved weights and transmittances.  No LDS,
// no atomics; a ray without samples gets zeros.  Segment bounds are clamped to [0, n_samples], so a
// malformed seg cannot take an access outside the sample arrays.
#include "common.h"
#include "composite_common.h"

using namespace nerf;

namespace {

struct PackedArgs {
    const float* sigma; int64_t ss;
    const float* rgb; int64_t cs;          // rgb may be null: weights only
    const float* t0; const float* t1;
    const int64_t* seg;
    int64_t n_rays, n_samples;
};

__device__ __forceinline__ void segment(const PackedArgs& a, int64_t ray, int64_t& s0, int64_t& s1) {
    s0 = a.seg[ray];
    s1 = a.seg[ray + 1];
    s0 = s0 < 0 ? 0 : (s0 > a.n_samples ? a.n_samples : s0);
    s1 = s1 < s0 ? s0 : (s1 > a.n_samples ? a.n_samples : s1);
}

__global__ __launch_bounds__(256) void composite_packed_fwd_kernel(PackedArgs a, float* __restrict__ colors,
                                                                   float* __restrict__ opacity,
                                                                   float* __restrict__ depth,
                                                                   float* __restrict__ weights,
                                                                   float* __restrict__ trans,
                                                                   float* __restrict__ alphas) {
#pragma clang fp contract(off)
    const int lane = lane_id();
    const int64_t ray = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ray >= a.n_rays) return;        // wave-uniform
    int64_t s0, s1;
    segment(a, ray, s0, s1);
    float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f, acco = 0.f, accd = 0.f;
    double carry = 0.0;                 // sum of b over the ray's earlier chunks
    for (int64_t cb = s0; cb < s1; cb += NERF_WAVE) {
        const int64_t i = cb + lane;
        const bool ok = i < s1;
        float sig = 0.f, ts = 0.f, te = 0.f, c0 = 0.f, c1 = 0.f, c2 = 0.f;
        if (ok) {
            sig = a.sigma[i * a.ss];
            ts = a.t0[i];
            te = a.t1[i];
            if (a.rgb) {
                const float* cp = a.rgb + i * a.cs;
                c0 = cp[0]; c1 = cp[1]; c2 = cp[2];
            }
        }
        float bb = (-sig) * (te - ts);
        if (!ok) bb = 0.f;
        const double incl = wave_inclusive_scan_dpp((double)bb);
        const double ex = carry + (incl - (double)bb);      // exclusive prefix
        carry += wave_last_d(incl);
        const float T = (i == s0) ? 1.0f : comp_exp((float)ex);
        const float al = -expm1f(bb);
        const float w = T * al;
        if (ok) {
            if (weights) weights[i] = w;
            if (trans) trans[i] = T;
            if (alphas) alphas[i] = al;
            acc0 += w * c0;
            acc1 += w * c1;
            acc2 += w * c2;
            acco += w;
            accd += w * ((ts + te) * 0.5f);
        }
    }
    const float r0 = wave_sum_f(acc0), r1 = wave_sum_f(acc1), r2 = wave_sum_f(acc2);
    const float ro = wave_sum_f(acco), rd = wave_sum_f(accd);
    if (lane == 0) {
        if (colors) {
            colors[ray * 3 + 0] = r0;
            colors[ray * 3 + 1] = r1;
            colors[ray * 3 + 2] = r2;
        }
        if (opacity) opacity[ray] = ro;
        if (depth) depth[ray] = rd;
    }
}

// With g_w(i) = <g_colors, c_i> + g_weights(i) + g_opacity + g_depth * tm_i:
//   dL/db_k = -g_w(k) * T_k * exp(b_k) + sum_{i>k} g_w(i) * w_i
//   dL/dsigma_k = dL/db_k * (-(delta_k)) ;  dL/dc_k = w_k * g_colors
__global__ __launch_bounds__(256) void composite_packed_bwd_kernel(PackedArgs a, const float* __restrict__ weights,
                                                                   const float* __restrict__ trans,
                                                                   const float* __restrict__ g_colors,
                                                                   const float* __restrict__ g_opacity,
                                                                   const float* __restrict__ g_depth,
                                                                   const float* __restrict__ g_weights,
                                                                   float* __restrict__ gd, int64_t gds,
                                                                   float* __restrict__ gc, int64_t gcs) {
#pragma clang fp contract(off)
    const int lane = lane_id();
    const int64_t ray = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ray >= a.n_rays) return;
    int64_t s0, s1;
    segment(a, ray, s0, s1);
    if (s0 >= s1) return;
    float g0 = 0.f, g1 = 0.f, g2 = 0.f;
    if (g_colors) { g0 = g_colors[ray * 3 + 0]; g1 = g_colors[ray * 3 + 1]; g2 = g_colors[ray * 3 + 2]; }
    const float go = g_opacity ? g_opacity[ray] : 0.f;
    const float gdep = g_depth ? g_depth[ray] : 0.f;
    double later = 0.0;                 // sum of g_w * w over the chunks behind this one
    const int64_t chunks = (s1 - s0 + NERF_WAVE - 1) / NERF_WAVE;
    for (int64_t ch = chunks - 1; ch >= 0; --ch) {
        const int64_t i = s0 + ch * NERF_WAVE + lane;
        const bool ok = i < s1;
        float sig = 0.f, ts = 0.f, te = 0.f, c0 = 0.f, c1 = 0.f, c2 = 0.f, w = 0.f, T = 0.f, gw = 0.f;
        if (ok) {
            sig = a.sigma[i * a.ss];
            ts = a.t0[i];
            te = a.t1[i];
            w = weights[i];
            T = trans[i];
            if (a.rgb) {
                const float* cp = a.rgb + i * a.cs;
                c0 = cp[0]; c1 = cp[1]; c2 = cp[2];
            }
            gw = g0 * c0 + g1 * c1 + g2 * c2;
            if (g_weights) gw += g_weights[i];
            gw += go;
            gw += gdep * ((ts + te) * 0.5f);
        }
        const float del = te - ts;
        const float e = comp_exp((-sig) * del);
        const double q = ok ? (double)gw * (double)w : 0.0;
        const double qi = wave_inclusive_scan_dpp(q);
        const double qtot = wave_last_d(qi);
        const double suffix = later + (qtot - qi);
        later += qtot;
        if (ok) {
            const float dldb = (float)((double)(-gw * T * e) + suffix);
            if (gd) gd[i * gds] = -(dldb * del);
            if (gc) {
                float* gp = gc + i * gcs;
                gp[0] = w * g0; gp[1] = w * g1; gp[2] = w * g2;
            }
        }
    }
}

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

extern "C" int nerf_composite_packed_fwd(const float* sigma, int64_t sigma_stride, const float* rgb,
                                         int64_t rgb_stride, const float* t_starts, const float* t_ends,
                                         const int64_t* seg, int64_t n_rays, int64_t n_samples, float* colors,
                                         float* opacity, float* depth, float* weights, float* trans, float* alphas,
                                         void* stream) {
    NERF_REQUIRE(n_rays >= 0 && n_samples >= 0);
    if (n_rays == 0) return NERF_OK;
    NERF_REQUIRE(seg && aligned(seg, 8));
    NERF_REQUIRE(n_samples == 0 || (sigma && t_starts && t_ends && sigma_stride >= 1));
    NERF_REQUIRE(!rgb || rgb_stride >= 3);
    NERF_REQUIRE(aligned(sigma, 4) && aligned(rgb, 4) && aligned(t_starts, 4) && aligned(t_ends, 4));
    NERF_REQUIRE(aligned(colors, 4) && aligned(opacity, 4) && aligned(depth, 4) && aligned(weights, 4) &&
                 aligned(trans, 4) && aligned(alphas, 4));
    NERF_REQUIRE((n_rays + 3) / 4 < (1ll << 31));
    PackedArgs a{sigma, sigma_stride, rgb, rgb_stride, t_starts, t_ends, seg, n_rays, n_samples};
    dim3 grid((unsigned)((n_rays + 3) / 4)), block(256);
    hipLaunchKernelGGL(composite_packed_fwd_kernel, grid, block, 0, as_stream(stream), a, colors, opacity, depth,
                       weights, trans, alphas);
    NERF_CHECK_LAUNCH();
    return NERF_OK;
}

extern "C" int nerf_composite_packed_bwd(const float* sigma, int64_t sigma_stride, const float* rgb,
                                         int64_t rgb_stride, const float* t_starts, const float* t_ends,
                                         const int64_t* seg, int64_t n_rays, int64_t n_samples, const float* weights,
                                         const float* trans, const float* g_colors, const float* g_opacity,
                                         const float* g_depth, const float* g_weights, float* grad_sigma,
                                         int64_t gs_stride, float* grad_rgb, int64_t gc_stride, void* stream) {
    NERF_REQUIRE(n_rays >= 0 && n_samples >= 0);
    if (n_rays == 0 || n_samples == 0) return NERF_OK;
    NERF_REQUIRE(seg && aligned(seg, 8));
    NERF_REQUIRE(sigma && t_starts && t_ends && weights && trans && sigma_stride >= 1);
    NERF_REQUIRE(!rgb || rgb_stride >= 3);
    NERF_REQUIRE(!grad_sigma || gs_stride >= 1);
    NERF_REQUIRE(!grad_rgb || (rgb && gc_stride >= 3));
    NERF_REQUIRE(aligned(sigma, 4) && aligned(rgb, 4) && aligned(t_starts, 4) && aligned(t_ends, 4) &&
                 aligned(weights, 4) && aligned(trans, 4));
    NERF_REQUIRE(aligned(g_colors, 4) && aligned(g_opacity, 4) && aligned(g_depth, 4) && aligned(g_weights, 4) &&
                 aligned(grad_sigma, 4) && aligned(grad_rgb, 4));
    NERF_REQUIRE((n_rays + 3) / 4 < (1ll << 31));
    PackedArgs a{sigma, sigma_stride, rgb, rgb_stride, t_starts, t_ends, seg, n_rays, n_samples};
    dim3 grid((unsigned)((n_rays + 3) / 4)), block(256);
    hipLaunchKernelGGL(composite_packed_bwd_kernel, grid, block, 0, as_stream(stream), a, weights, trans, g_colors,
                       g_opacity, g_depth, g_weights, grad_sigma, gs_stride, grad_rgb, gc_stride);
    NERF_CHECK_LAUNCH();
    return NERF_OK;
}
