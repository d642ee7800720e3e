// Per-sample pieces of the Instant-NGP radiance field (nerf_amd/model_ngp.py) behind the occupancy
// grid: the degree <= 4 real spherical-harmonics direction encoding, and the position map from scene
// coordinates to the hash grid's unit cube (normalise to the box, or nerfacc's contract_to_unisphere
// with the inf-norm) with its in-box selector.  nerfacc and tiny-cuda-nn are restated from their
// published behaviour, parity unpinned.
//
// Four kernels, one thread per sample, no atomics, no LDS, no inline assembly; every operation is
// rounded to fp32 on its own (no contraction) in the order of the two numbered contracts in
// include/nerf_amd.h, which tests/_ngp_field_ref.py restates.  No store at or past row n and none to
// a column the contracts do not name.
#include "common.h"

using namespace nerf;

namespace {

// the 16 constants, rounded to fp32 once
constexpr float C0 = 0.28209479177387814f;
constexpr float C1 = 0.48860251190291987f;
constexpr float C2 = 1.0925484305920792f;
constexpr float C3 = 0.94617469575755997f;
constexpr float C4 = 0.31539156525251999f;
constexpr float C5 = 0.54627421529603959f;
constexpr float C6 = 0.59004358992664352f;
constexpr float C7 = 2.8906114426405538f;
constexpr float C8 = 0.45704579946446572f;
constexpr float C9 = 0.3731763325901154f;
constexpr float C10 = 1.4453057213202769f;

__global__ __launch_bounds__(256) void sh_encode_fwd_kernel(const float* __restrict__ dirs, int64_t ds, int64_t n,
                                                            int degree, float* __restrict__ out, int64_t ld) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float* d = dirs + i * ds;
    const float x = d[0], y = d[1], z = d[2];
    float* o = out + i * ld;
    o[0] = C0;
    if (degree <= 1) return;
    o[1] = -C1 * y;
    o[2] = C1 * z;
    o[3] = -C1 * x;
    if (degree <= 2) return;
    const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
    o[4] = C2 * xy;
    o[5] = -C2 * yz;
    o[6] = C3 * zz - C4;
    o[7] = -C2 * xz;
    o[8] = C5 * (xx - yy);
    if (degree <= 3) return;
    const float w = 1.0f - 5.0f * zz;
    o[9] = (C6 * y) * (-3.0f * xx + yy);
    o[10] = (C7 * xy) * z;
    o[11] = (C8 * y) * w;
    o[12] = (C9 * z) * (5.0f * zz - 3.0f);
    o[13] = (C8 * x) * w;
    o[14] = (C10 * z) * (xx - yy);
    o[15] = (C6 * x) * (-xx + 3.0f * yy);
}

__global__ __launch_bounds__(256) void sh_encode_bwd_kernel(const float* __restrict__ dirs, int64_t ds, int64_t n,
                                                            int degree, const float* __restrict__ g_out, int64_t gld,
                                                            float* __restrict__ g_dirs, int64_t gds) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float* d = dirs + i * ds;
    const float x = d[0], y = d[1], z = d[2];
    const float* g = g_out + i * gld;
    // c = 0 is constant; the sums run over c ascending
    float gx = 0.0f, gy = 0.0f, gz = 0.0f;
    if (degree >= 2) {
        gy += g[1] * -C1;
        gz += g[2] * C1;
        gx += g[3] * -C1;
    }
    if (degree >= 3) {
        const float g4 = g[4], g5 = g[5], g6 = g[6], g7 = g[7], g8 = g[8];
        gx += g4 * (C2 * y);             gy += g4 * (C2 * x);
        gy += g5 * (-C2 * z);            gz += g5 * (-C2 * y);
        gz += g6 * ((2.0f * C3) * z);
        gx += g7 * (-C2 * z);            gz += g7 * (-C2 * x);
        gx += g8 * ((2.0f * C5) * x);    gy += g8 * ((-2.0f * C5) * y);
    }
    if (degree >= 4) {
        const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
        const float w = 1.0f - 5.0f * zz, e = yy - xx;
        const float g9 = g[9], g10 = g[10], g11 = g[11], g12 = g[12], g13 = g[13], g14 = g[14], g15 = g[15];
        gx += g9 * ((-6.0f * C6) * xy);   gy += g9 * ((3.0f * C6) * e);
        gx += g10 * (C7 * yz);            gy += g10 * (C7 * xz);             gz += g10 * (C7 * xy);
        gy += g11 * (C8 * w);             gz += g11 * ((-10.0f * C8) * yz);
        gz += g12 * (C9 * (15.0f * zz - 3.0f));
        gx += g13 * (C8 * w);             gz += g13 * ((-10.0f * C8) * xz);
        gx += g14 * ((2.0f * C10) * xz);  gy += g14 * ((-2.0f * C10) * yz);  gz += g14 * (C10 * (xx - yy));
        gx += g15 * ((3.0f * C6) * e);    gy += g15 * ((6.0f * C6) * xy);
    }
    float* o = g_dirs + i * gds;
    o[0] = gx; o[1] = gy; o[2] = gz;
}

struct Box {
    float lo[3], hi[3];
};

// fmaxf: a NaN operand is ignored
__device__ __forceinline__ float inf_norm(const float* c) { return fmaxf(fmaxf(fabsf(c[0]), fabsf(c[1])), fabsf(c[2])); }

__global__ __launch_bounds__(256) void unit_cube_fwd_kernel(const float* __restrict__ x, int64_t xs, int64_t n, Box box,
                                                            int mode, float* __restrict__ u, int64_t us,
                                                            float* __restrict__ inside) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float* p = x + i * xs;
    float c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float e = box.hi[a] - box.lo[a];
        c[a] = (p[a] - box.lo[a]) / e;
    }
    if (mode == 1) {
#pragma unroll
        for (int a = 0; a < 3; ++a) c[a] = c[a] * 2.0f - 1.0f;
        const float m = inf_norm(c);
        if (m > 1.0f) {
            const float s = 2.0f - 1.0f / m;
#pragma unroll
            for (int a = 0; a < 3; ++a) c[a] = s * (c[a] / m);
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) c[a] = c[a] / 4.0f + 0.5f;
    }
    float* o = u + i * us;
    o[0] = c[0]; o[1] = c[1]; o[2] = c[2];
    if (inside) {
        const bool in = c[0] > 0.0f && c[0] < 1.0f && c[1] > 0.0f && c[1] < 1.0f && c[2] > 0.0f && c[2] < 1.0f;
        inside[i] = in ? 1.0f : 0.0f;
    }
}

__global__ __launch_bounds__(256) void unit_cube_bwd_kernel(const float* __restrict__ x, int64_t xs, int64_t n, Box box,
                                                            int mode, const float* __restrict__ g_u, int64_t gus,
                                                            float* __restrict__ g_x, int64_t gxs) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float* p = x + i * xs;
    const float* g = g_u + i * gus;
    float* o = g_x + i * gxs;
    float e[3], gc[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        e[a] = box.hi[a] - box.lo[a];
        gc[a] = g[a];
    }
    if (mode == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) o[a] = gc[a] / e[a];
        return;
    }
    float c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) c[a] = ((p[a] - box.lo[a]) / e[a]) * 2.0f - 1.0f;
    const float m = inf_norm(c);
    if (m > 1.0f) {
        // y = (2m - 1) c / m^2:  dy_j/dc_i = (s/m) delta_ij + c_j sgn(c_k) delta_ik (2 - 2m) / m^3
        const int k = fabsf(c[0]) == m ? 0 : (fabsf(c[1]) == m ? 1 : 2);
        const float s = 2.0f - 1.0f / m;
        const float dot = (gc[0] * c[0] + gc[1] * c[1]) + gc[2] * c[2];
        const float t = ((2.0f - 2.0f * m) / m) / (m * m);
        const float sm = s / m;
        const float ck = k == 0 ? c[0] : (k == 1 ? c[1] : c[2]);
        const float extra = (ck < 0.0f ? -t : t) * dot;
#pragma unroll
        for (int a = 0; a < 3; ++a) gc[a] = sm * gc[a] + (a == k ? extra : 0.0f);
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) o[a] = gc[a] / (2.0f * e[a]);
}

bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

bool grid_ok(int64_t n) { return (n + 255) / 256 < (1ll << 31); }

}  // namespace

extern "C" int nerf_sh_encode_fwd(const float* dirs, int64_t dirs_stride, int64_t n, int degree, float* out,
                                  int64_t out_ld, void* stream) {
    NERF_REQUIRE(n >= 0 && degree >= 1 && degree <= 4);
    if (n == 0) return NERF_OK;
    NERF_REQUIRE(dirs && out && aligned4(dirs) && aligned4(out));
    NERF_REQUIRE(dirs_stride >= 3 && out_ld >= (int64_t)degree * degree && grid_ok(n));
    dim3 grid((unsigned)((n + 255) / 256)), block(256);
    hipLaunchKernelGGL(sh_encode_fwd_kernel, grid, block, 0, as_stream(stream), dirs, dirs_stride, n, degree, out,
                       out_ld);
    NERF_CHECK_LAUNCH();
    return NERF_OK;
}

extern "C" int nerf_sh_encode_bwd(const float* dirs, int64_t dirs_stride, int64_t n, int degree,
                                  const float* grad_out, int64_t g_ld, float* grad_dirs, int64_t gd_stride,
                                  void* stream) {
    NERF_REQUIRE(n >= 0 && degree >= 1 && degree <= 4);
    if (n == 0) return NERF_OK;
    NERF_REQUIRE(dirs && grad_out && grad_dirs && aligned4(dirs) && aligned4(grad_out) && aligned4(grad_dirs));
    NERF_REQUIRE(dirs_stride >= 3 && g_ld >= (int64_t)degree * degree && gd_stride >= 3 && grid_ok(n));
    dim3 grid((unsigned)((n + 255) / 256)), block(256);
    hipLaunchKernelGGL(sh_encode_bwd_kernel, grid, block, 0, as_stream(stream), dirs, dirs_stride, n, degree,
                       grad_out, g_ld, grad_dirs, gd_stride);
    NERF_CHECK_LAUNCH();
    return NERF_OK;
}

extern "C" int nerf_unit_cube_fwd(const float* x, int64_t x_stride, int64_t n, const float* aabb, int mode, float* u,
                                  int64_t u_stride, float* inside, void* stream) {
    NERF_REQUIRE(n >= 0 && (mode == 0 || mode == 1) && aabb);
    if (n == 0) return NERF_OK;
    NERF_REQUIRE(x && u && aligned4(x) && aligned4(u) && aligned4(inside));
    NERF_REQUIRE(x_stride >= 3 && u_stride >= 3 && grid_ok(n));
    Box box;
    for (int a = 0; a < 3; ++a) { box.lo[a] = aabb[a]; box.hi[a] = aabb[3 + a]; }
    dim3 grid((unsigned)((n + 255) / 256)), block(256);
    hipLaunchKernelGGL(unit_cube_fwd_kernel, grid, block, 0, as_stream(stream), x, x_stride, n, box, mode, u, u_stride,
                       inside);
    NERF_CHECK_LAUNCH();
    return NERF_OK;
}

extern "C" int nerf_unit_cube_bwd(const float* x, int64_t x_stride, int64_t n, const float* aabb, int mode,
                                  const float* grad_u, int64_t gu_stride, float* grad_x, int64_t gx_stride,
                                  void* stream) {
    NERF_REQUIRE(n >= 0 && (mode == 0 || mode == 1) && aabb);
    if (n == 0) return NERF_OK;
    NERF_REQUIRE(x && grad_u && grad_x && aligned4(x) && aligned4(grad_u) && aligned4(grad_x));
    NERF_REQUIRE(x_stride >= 3 && gu_stride >= 3 && gx_stride >= 3 && grid_ok(n));
    Box box;
    for (int a = 0; a < 3; ++a) { box.lo[a] = aabb[a]; box.hi[a] = aabb[3 + a]; }
    dim3 grid((unsigned)((n + 255) / 256)), block(256);
    hipLaunchKernelGGL(unit_cube_bwd_kernel, grid, block, 0, as_stream(stream), x, x_stride, n, box, mode, grad_u,
                       gu_stride, grad_x, gx_stride);
    NERF_CHECK_LAUNCH();
    return NERF_OK;
}
