// Gabor and Sarf activations with learnable per-channel parameters (GaborF / SARF field MLPs):
// element formulas in param_act.h (gaborf/gabor.py:8-64, sarf/activation.py:40-65).
//
// Layout and mapping as gauss.hip: z, y, g, dz are [M][N] row-major with their own row strides;
// 64 consecutive lanes on 64 consecutive columns of one row, 4 row groups per block, slabs of
// ~512 rows.  The backward keeps one fp64 column partial per thread and learnable parameter
// (Gabor: 2, Sarf: 1), reduces the 4 row groups through LDS and writes one partial row per slab
// and parameter (plane p at partial + p * slabs * N); the slabs are then summed in a fixed order
// (nerf::gauss_reduce for Gabor's s, whose final * (2 s) is the same chain rule as GARF's;
// nerf::param_reduce_plain for spread / frequency).  Deterministic, no atomics.
//
// SIREN's sine (nerf_sine_act_fwd / _bwd, nerf-siren/linear_sine.py:44-45) uses the same mapping
// with SineFn: no parameter, so no partials, no reduce and no workspace.
#include "param_act.h"

using namespace nerf;

namespace {

constexpr int kCols = 64;     // columns per block
constexpr int kRowGroups = 4; // row groups per block (blockDim = 256)
constexpr int kMaxChunks = 64;

template <class Act>
__global__ __launch_bounds__(256) void param_act_fwd_kernel(const float* __restrict__ z, int64_t ldz,
                                                            const float* __restrict__ p0,
                                                            const float* __restrict__ p1, int64_t M, int N,
                                                            float* __restrict__ y, int64_t ldy,
                                                            int64_t rows_per_block) {
    const int n = blockIdx.y * kCols + (threadIdx.x & (kCols - 1));
    if (n >= N) return;
    const typename Act::P k = Act::load(p0, p1, n);
    const int64_t m0 = (int64_t)blockIdx.x * rows_per_block;
    const int64_t m1 = m0 + rows_per_block < M ? m0 + rows_per_block : M;
    for (int64_t m = m0 + (threadIdx.x >> 6); m < m1; m += kRowGroups) y[m * ldy + n] = Act::fwd(z[m * ldz + n], k);
}

// grad_z may alias grad_y (in-place): each element is read and then written by one thread.
template <class Act>
__global__ __launch_bounds__(256) void param_act_bwd_kernel(const float* g, int64_t ldg,
                                                            const float* __restrict__ z, int64_t ldz,
                                                            const float* __restrict__ p0,
                                                            const float* __restrict__ p1, int64_t M, int N, float* dz,
                                                            int64_t lddz, int64_t rows_per_block,
                                                            double* __restrict__ partial, int64_t plane) {
    __shared__ double red[Act::kParams][kRowGroups][kCols];
    const int c = threadIdx.x & (kCols - 1);
    const int rg = threadIdx.x >> 6;
    const int n = blockIdx.y * kCols + c;
    double acc0 = 0.0, acc1 = 0.0;
    if (n < N) {
        const typename Act::P k = Act::load(p0, p1, n);
        const int64_t m0 = (int64_t)blockIdx.x * rows_per_block;
        const int64_t m1 = m0 + rows_per_block < M ? m0 + rows_per_block : M;
        for (int64_t m = m0 + rg; m < m1; m += kRowGroups)
            dz[m * lddz + n] = Act::bwd(g[m * ldg + n], z[m * ldz + n], k, acc0, acc1);
    }
    red[0][rg][c] = acc0;
    if (Act::kParams > 1) red[Act::kParams - 1][rg][c] = acc1;
    __syncthreads();
    if (rg == 0 && n < N) {
#pragma unroll
        for (int p = 0; p < Act::kParams; ++p)
            partial[p * plane + (int64_t)blockIdx.x * N + n] =
                ((red[p][0][c] + red[p][1][c]) + red[p][2][c]) + red[p][3][c];
    }
}

// SIREN's sine backward: the same mapping, no column sums (SineFn has no parameters).
// grad_z may alias grad_y, as above.
__global__ __launch_bounds__(256) void sine_act_bwd_kernel(const float* g, int64_t ldg, const float* __restrict__ z,
                                                           int64_t ldz, int64_t M, int N, float* dz, int64_t lddz,
                                                           int64_t rows_per_block) {
    const int n = blockIdx.y * kCols + (threadIdx.x & (kCols - 1));
    if (n >= N) return;
    const int64_t m0 = (int64_t)blockIdx.x * rows_per_block;
    const int64_t m1 = m0 + rows_per_block < M ? m0 + rows_per_block : M;
    double unused0 = 0.0, unused1 = 0.0;
    for (int64_t m = m0 + (threadIdx.x >> 6); m < m1; m += kRowGroups)
        dz[m * lddz + n] = SineFn::bwd(g[m * ldg + n], z[m * ldz + n], SineFn::P{}, unused0, unused1);
}

// the two levels of gauss.hip's column reduction, finished without a factor
__global__ __launch_bounds__(256) void param_reduce_chunks_kernel(const double* __restrict__ partial, int64_t slabs,
                                                                  int N, int64_t chunk, double* __restrict__ out2) {
    __shared__ double red[kRowGroups][kCols];
    const int c = threadIdx.x & (kCols - 1);
    const int rg = threadIdx.x >> 6;
    const int n = blockIdx.x * kCols + c;
    const int64_t i0 = (int64_t)blockIdx.y * chunk;
    const int64_t i1 = i0 + chunk < slabs ? i0 + chunk : slabs;
    double acc = 0.0;
    if (n < N)
        for (int64_t i = i0 + rg; i < i1; i += kRowGroups) acc += partial[i * N + n];
    red[rg][c] = acc;
    __syncthreads();
    if (rg == 0 && n < N) out2[(int64_t)blockIdx.y * N + n] = ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
}

__global__ __launch_bounds__(256) void param_reduce_final_kernel(const double* __restrict__ out2, int chunks, int N,
                                                                 float* __restrict__ dp, int accumulate) {
#pragma clang fp contract(off)
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    double t = 0.0;
    for (int i = 0; i < chunks; ++i) t += out2[(int64_t)i * N + n];
    const float r = (float)t;
    dp[n] = accumulate ? dp[n] + r : r;
}

int64_t slabs_for(int64_t M) {
    // ~512 rows per slab, at most 1024 slabs (as gauss.hip)
    int64_t slabs = (M + 511) / 512;
    if (slabs > 1024) slabs = 1024;
    if (slabs < 1) slabs = 1;
    return slabs;
}

bool kind_ok(int kind) { return kind == NERF_ACT_GABOR || kind == NERF_ACT_SARF; }
int n_params(int kind) { return kind == NERF_ACT_GABOR ? 2 : 1; }

}  // namespace

int nerf::param_reduce_plain(const double* partial, int64_t slabs, int N, float* dp, int accumulate, double* scratch,
                             hipStream_t st) {
    int64_t chunks = (slabs + 63) / 64;
    chunks = chunks < 1 ? 1 : (chunks > kMaxChunks ? kMaxChunks : chunks);
    const int64_t chunk = (slabs + chunks - 1) / chunks;
    chunks = (slabs + chunk - 1) / chunk;
    hipLaunchKernelGGL(param_reduce_chunks_kernel, dim3((unsigned)((N + kCols - 1) / kCols), (unsigned)chunks),
                       dim3(256), 0, st, partial, slabs, N, chunk, scratch);
    if (hipGetLastError() != hipSuccess) return NERF_ERR_LAUNCH;
    hipLaunchKernelGGL(param_reduce_final_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, scratch,
                       (int)chunks, N, dp, accumulate);
    if (hipGetLastError() != hipSuccess) return NERF_ERR_LAUNCH;
    return NERF_OK;
}

int nerf::param_act_reduce(int kind, const double* partial, int64_t plane, int64_t slabs, int N, const float* p0,
                           float* grad_p0, float* grad_p1, int accumulate, double* scratch, hipStream_t st) {
    if (kind == NERF_ACT_GABOR) {
        const int rc = nerf::gauss_reduce(partial, slabs, N, p0, grad_p0, accumulate, scratch, st);
        if (rc != NERF_OK) return rc;
        return nerf::param_reduce_plain(partial + plane, slabs, N, grad_p1, accumulate, scratch, st);
    }
    return nerf::param_reduce_plain(partial, slabs, N, grad_p0, accumulate, scratch, st);
}

extern "C" size_t nerf_param_act_workspace(int32_t kind, int64_t M, int32_t N) {
    if (!kind_ok(kind) || M <= 0 || N <= 0) return 0;
    return (size_t)n_params(kind) * (size_t)slabs_for(M) * (size_t)N * sizeof(double) + nerf::gauss_reduce_scratch(N);
}

extern "C" int nerf_param_act_fwd(int32_t kind, const float* z, int64_t ld_z, const float* p0, const float* p1,
                                  int64_t M, int32_t N, float* y, int64_t ld_y, void* stream) {
    NERF_REQUIRE(kind_ok(kind) && M >= 0 && N >= 0);
    if (M == 0 || N == 0) return NERF_OK;
    NERF_REQUIRE(z && p0 && (p1 || kind != NERF_ACT_GABOR) && y && ld_z >= N && ld_y >= N);
    const int64_t slabs = slabs_for(M);
    const int64_t rows = (M + slabs - 1) / slabs;
    dim3 grid((unsigned)slabs, (unsigned)((N + kCols - 1) / kCols));
    if (kind == NERF_ACT_GABOR)
        hipLaunchKernelGGL(param_act_fwd_kernel<GaborFn>, grid, dim3(256), 0, as_stream(stream), z, ld_z, p0, p1, M, N,
                           y, ld_y, rows);
    else
        hipLaunchKernelGGL(param_act_fwd_kernel<SarfFn>, grid, dim3(256), 0, as_stream(stream), z, ld_z, p0, p1, M, N,
                           y, ld_y, rows);
    NERF_CHECK_LAUNCH();
    return NERF_OK;
}

extern "C" int nerf_param_act_bwd(int32_t kind, const float* grad_y, int64_t ld_g, const float* z, int64_t ld_z,
                                  const float* p0, const float* p1, int64_t M, int32_t N, float* grad_z,
                                  int64_t ld_dz, float* grad_p0, float* grad_p1, int32_t accumulate, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    NERF_REQUIRE(kind_ok(kind) && M >= 0 && N >= 0);
    if (N == 0) return NERF_OK;
    const bool two = kind == NERF_ACT_GABOR;
    NERF_REQUIRE(p0 && grad_p0 && (!two || (p1 && grad_p1)));
    hipStream_t st = as_stream(stream);
    if (M == 0) {
        if (!accumulate) {
            if (hipMemsetAsync(grad_p0, 0, (size_t)N * sizeof(float), st) != hipSuccess) return NERF_ERR_LAUNCH;
            if (two && hipMemsetAsync(grad_p1, 0, (size_t)N * sizeof(float), st) != hipSuccess)
                return NERF_ERR_LAUNCH;
        }
        return NERF_OK;
    }
    NERF_REQUIRE(grad_y && z && grad_z && ld_g >= N && ld_z >= N && ld_dz >= N);
    if (!workspace || workspace_bytes < nerf_param_act_workspace(kind, M, N) ||
        (reinterpret_cast<uintptr_t>(workspace) & 7) != 0)
        return NERF_ERR_WORKSPACE;
    const int64_t slabs = slabs_for(M);
    const int64_t rows = (M + slabs - 1) / slabs;
    const int64_t plane = slabs * N;
    double* partial = reinterpret_cast<double*>(workspace);
    dim3 grid((unsigned)slabs, (unsigned)((N + kCols - 1) / kCols));
    if (two)
        hipLaunchKernelGGL(param_act_bwd_kernel<GaborFn>, grid, dim3(256), 0, st, grad_y, ld_g, z, ld_z, p0, p1, M, N,
                           grad_z, ld_dz, rows, partial, plane);
    else
        hipLaunchKernelGGL(param_act_bwd_kernel<SarfFn>, grid, dim3(256), 0, st, grad_y, ld_g, z, ld_z, p0, p1, M, N,
                           grad_z, ld_dz, rows, partial, plane);
    NERF_CHECK_LAUNCH();
    return nerf::param_act_reduce(kind, partial, plane, slabs, N, p0, grad_p0, grad_p1, accumulate,
                                  partial + n_params(kind) * plane, st);
}

// ---------------------------------------------------------------------------- SIREN's sine
extern "C" int nerf_sine_act_fwd(const float* z, int64_t ld_z, int64_t M, int32_t N, float* y, int64_t ld_y,
                                 void* stream) {
    NERF_REQUIRE(M >= 0 && N >= 0);
    if (M == 0 || N == 0) return NERF_OK;
    NERF_REQUIRE(z && y && ld_z >= N && ld_y >= N);
    const int64_t slabs = slabs_for(M);
    const int64_t rows = (M + slabs - 1) / slabs;
    dim3 grid((unsigned)slabs, (unsigned)((N + kCols - 1) / kCols));
    hipLaunchKernelGGL(param_act_fwd_kernel<SineFn>, grid, dim3(256), 0, as_stream(stream), z, ld_z,
                       (const float*)nullptr, (const float*)nullptr, M, N, y, ld_y, rows);
    NERF_CHECK_LAUNCH();
    return NERF_OK;
}

extern "C" int nerf_sine_act_bwd(const float* grad_y, int64_t ld_g, const float* z, int64_t ld_z, int64_t M,
                                 int32_t N, float* grad_z, int64_t ld_dz, void* stream) {
    NERF_REQUIRE(M >= 0 && N >= 0);
    if (M == 0 || N == 0) return NERF_OK;
    NERF_REQUIRE(grad_y && z && grad_z && ld_g >= N && ld_z >= N && ld_dz >= N);
    const int64_t slabs = slabs_for(M);
    const int64_t rows = (M + slabs - 1) / slabs;
    dim3 grid((unsigned)slabs, (unsigned)((N + kCols - 1) / kCols));
    hipLaunchKernelGGL(sine_act_bwd_kernel, grid, dim3(256), 0, as_stream(stream), grad_y, ld_g, z, ld_z, M, N,
                       grad_z, ld_dz, rows);
    NERF_CHECK_LAUNCH();
    return NERF_OK;
}
