// Sample points of packed samples (the output of an occupancy-grid sampler) and their gradient to
// the rays: the step between OccGridEstimator.sampling and the field.
//
// Forward, one thread per sample i of ray r = ray_indices[i]:
//   tm = (t_starts_i + t_ends_i) * 0.5f,  p_a = o[r]_a + tm * d[r]_a,  dirs_i = d[r]
// every operation rounded to fp32 on its own (steps 8-9 of the marching contract, include/nerf_amd.h),
// so a kept sample is evaluated bitwise at the point whose grid cell the marching tested.  A ray
// index outside [0, n_rays) gives a NaN row and reads nothing.
// Backward, one 64-lane wavefront per ray over its segment [seg[r], seg[r+1]) in 64-sample chunks:
//   g_o[r] = sum g_pos_i,  g_d[r] = sum (tm_i * g_pos_i + g_dir_i)
// each lane sums its samples of the successive chunks in fp64, then one xor-butterfly over the lanes:
// a fixed order, no atomics, bitwise reproducible.  Segment bounds are clamped to [0, n_samples].
#include "common.h"

using namespace nerf;

namespace {

__global__ __launch_bounds__(256) void packed_points_fwd_kernel(const float* __restrict__ rays_o,
                                                                const float* __restrict__ rays_d, int64_t n_rays,
                                                                const int64_t* __restrict__ ray_indices,
                                                                const float* __restrict__ t0,
                                                                const float* __restrict__ t1, int64_t n_samples,
                                                                float* __restrict__ pos, int64_t ps,
                                                                float* __restrict__ dirs, int64_t ds) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_samples) return;
    const int64_t r = ray_indices[i];
    float* pp = pos + i * ps;
    float* dp = dirs ? dirs + i * ds : nullptr;
    if (r < 0 || r >= n_rays) {
        const float nan = __builtin_nanf("");
        pp[0] = nan; pp[1] = nan; pp[2] = nan;
        if (dp) { dp[0] = nan; dp[1] = nan; dp[2] = nan; }
        return;
    }
    const float* o = rays_o + r * 3;
    const float* d = rays_d + r * 3;
    const float d0 = d[0], d1 = d[1], d2 = d[2];
    const float tm = (t0[i] + t1[i]) * 0.5f;
    pp[0] = o[0] + tm * d0;
    pp[1] = o[1] + tm * d1;
    pp[2] = o[2] + tm * d2;
    if (dp) { dp[0] = d0; dp[1] = d1; dp[2] = d2; }
}

__global__ __launch_bounds__(256) void packed_points_bwd_kernel(const int64_t* __restrict__ seg, int64_t n_rays,
                                                                const float* __restrict__ t0,
                                                                const float* __restrict__ t1, int64_t n_samples,
                                                                const float* __restrict__ gp, int64_t gps,
                                                                const float* __restrict__ gd, int64_t gds,
                                                                float* __restrict__ g_o, float* __restrict__ g_d) {
#pragma clang fp contract(off)
    const int lane = lane_id();
    const int64_t ray = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ray >= n_rays) return;          // wave-uniform
    int64_t s0 = seg[ray], s1 = seg[ray + 1];
    s0 = s0 < 0 ? 0 : (s0 > n_samples ? n_samples : s0);
    s1 = s1 < s0 ? s0 : (s1 > n_samples ? n_samples : s1);
    double ao0 = 0.0, ao1 = 0.0, ao2 = 0.0, ad0 = 0.0, ad1 = 0.0, ad2 = 0.0;
    for (int64_t cb = s0; cb < s1; cb += NERF_WAVE) {
        const int64_t i = cb + lane;
        if (i < s1) {
            const float tm = (t0[i] + t1[i]) * 0.5f;        // the forward's fp32 midpoint
            const float* g = gp + i * gps;
            const double x0 = g[0], x1 = g[1], x2 = g[2];
            ao0 += x0; ao1 += x1; ao2 += x2;
            double y0 = (double)tm * x0, y1 = (double)tm * x1, y2 = (double)tm * x2;
            if (gd) {
                const float* h = gd + i * gds;
                y0 += (double)h[0]; y1 += (double)h[1]; y2 += (double)h[2];
            }
            ad0 += y0; ad1 += y1; ad2 += y2;
        }
    }
    ao0 = wave_sum(ao0); ao1 = wave_sum(ao1); ao2 = wave_sum(ao2);
    ad0 = wave_sum(ad0); ad1 = wave_sum(ad1); ad2 = wave_sum(ad2);
    if (lane == 0) {
        g_o[ray * 3 + 0] = (float)ao0; g_o[ray * 3 + 1] = (float)ao1; g_o[ray * 3 + 2] = (float)ao2;
        g_d[ray * 3 + 0] = (float)ad0; g_d[ray * 3 + 1] = (float)ad1; g_d[ray * 3 + 2] = (float)ad2;
    }
}

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

extern "C" int nerf_packed_points_fwd(const float* rays_o, const float* rays_d, int64_t n_rays,
                                      const int64_t* ray_indices, const float* t_starts, const float* t_ends,
                                      int64_t n_samples, float* positions, int64_t pos_stride, float* dirs,
                                      int64_t dirs_stride, void* stream) {
    NERF_REQUIRE(n_rays >= 0 && n_samples >= 0);
    if (n_rays == 0 || n_samples == 0) return NERF_OK;
    NERF_REQUIRE(rays_o && rays_d && ray_indices && t_starts && t_ends && positions);
    NERF_REQUIRE(pos_stride >= 3 && (!dirs || dirs_stride >= 3));
    NERF_REQUIRE(aligned(ray_indices, 8));
    NERF_REQUIRE(aligned(rays_o, 4) && aligned(rays_d, 4) && aligned(t_starts, 4) && aligned(t_ends, 4) &&
                 aligned(positions, 4) && aligned(dirs, 4));
    NERF_REQUIRE((n_samples + 255) / 256 < (1ll << 31));
    dim3 grid((unsigned)((n_samples + 255) / 256)), block(256);
    hipLaunchKernelGGL(packed_points_fwd_kernel, grid, block, 0, as_stream(stream), rays_o, rays_d, n_rays,
                       ray_indices, t_starts, t_ends, n_samples, positions, pos_stride, dirs, dirs_stride);
    NERF_CHECK_LAUNCH();
    return NERF_OK;
}

extern "C" int nerf_packed_points_bwd(const int64_t* seg, int64_t n_rays, const float* t_starts, const float* t_ends,
                                      int64_t n_samples, const float* g_positions, int64_t gp_stride,
                                      const float* g_dirs, int64_t gd_stride, float* g_o, float* g_d, void* stream) {
    NERF_REQUIRE(n_rays >= 0 && n_samples >= 0);
    if (n_rays == 0 || n_samples == 0) return NERF_OK;
    NERF_REQUIRE(seg && t_starts && t_ends && g_positions && g_o && g_d);
    NERF_REQUIRE(gp_stride >= 3 && (!g_dirs || gd_stride >= 3));
    NERF_REQUIRE(aligned(seg, 8));
    NERF_REQUIRE(aligned(t_starts, 4) && aligned(t_ends, 4) && aligned(g_positions, 4) && aligned(g_dirs, 4) &&
                 aligned(g_o, 4) && aligned(g_d, 4));
    NERF_REQUIRE((n_rays + 3) / 4 < (1ll << 31));
    dim3 grid((unsigned)((n_rays + 3) / 4)), block(256);
    hipLaunchKernelGGL(packed_points_bwd_kernel, grid, block, 0, as_stream(stream), seg, n_rays, t_starts, t_ends,
                       n_samples, g_positions, gp_stride, g_dirs, gd_stride, g_o, g_d);
    NERF_CHECK_LAUNCH();
    return NERF_OK;
}
