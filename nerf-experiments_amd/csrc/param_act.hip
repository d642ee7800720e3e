// The per-channel activations as stand-alone passes: GARF's Gaussian, Gabor and Sarf (learnable
// per-channel parameters) and SIREN's sine (none); element formulas in param_act.h
// (garf/gaussian.py:8-63, gaborf/gabor.py:8-64, sarf/activation.py:40-65, nerf-siren/linear_sine.py:44-45).
//
// Layout: z, y, g, dz are [M][N] row-major with their own row strides (the MLP's padded activation
// buffers).  Both kernels map 64 consecutive lanes to 64 consecutive columns of one row, so every
// load / store is a coalesced 256-byte wave access; 4 row groups per block, slabs of ~512 rows.
// The backward keeps one fp64 column partial per thread and learnable parameter (Gabor: 2, Gauss
// and Sarf: 1, sine: 0 - no LDS, no partials, no reduce, no workspace), reduces the 4 row groups
// through LDS and writes one partial row per slab and parameter (plane p at partial + p * slabs * N);
// nerf::param_reduce then sums the slabs in a fixed order (deterministic, no atomics), with the
// chain-rule factor 2 s for the s of Gauss and Gabor.  The same reduction serves the activation
// epilogues of linear_x3.hip.
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
    if constexpr (Act::kParams > 0) {
        __shared__ double red[Act::kParams][kRowGroups][kCols];
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
}

// Column sums of the slab partials in two fixed-order levels: block (column group, chunk) sums
// its chunk's slabs (4 row groups, each a strided run, combined in order), then one thread per
// column sums the chunks in order.
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

// s: null for a plain sum, else the chain-rule factor 2 s_n of v = s^2 + 1e-6
__global__ __launch_bounds__(256) void param_reduce_final_kernel(const double* __restrict__ out2, int chunks, int N,
                                                                 const float* __restrict__ s, float* __restrict__ dp,
                                                                 int accumulate) {
#pragma clang fp contract(off)
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    double t = 0.0;
    for (int i = 0; i < chunks; ++i) t += out2[(int64_t)i * N + n];
    const float r = s ? ((float)t) * (2.0f * s[n]) : (float)t;
    dp[n] = accumulate ? dp[n] + r : r;
}

struct Slabs {
    int64_t n, rows;          // slabs of `rows` rows
    dim3 grid;
    Slabs(int64_t M, int N) {
        // ~512 rows per slab, at most 1024 slabs (the partials stay tiny: slabs * N * 8 bytes)
        n = (M + 511) / 512;
        n = n > 1024 ? 1024 : (n < 1 ? 1 : n);
        rows = (M + n - 1) / n;
        grid = dim3((unsigned)n, (unsigned)((N + kCols - 1) / kCols));
    }
};

size_t act_workspace(int params, int64_t M, int N) {
    if (params <= 0 || M <= 0 || N <= 0) return 0;
    return (size_t)params * (size_t)Slabs(M, N).n * (size_t)N * sizeof(double) + nerf::param_reduce_scratch(N);
}

template <class Act>
int act_fwd(const float* z, int64_t ld_z, const float* p0, const float* p1, int64_t M, int N, float* y, int64_t ld_y,
            void* stream) {
    NERF_REQUIRE(M >= 0 && N >= 0);
    if (M == 0 || N == 0) return NERF_OK;
    NERF_REQUIRE(z && (p0 || Act::kParams < 1) && (p1 || Act::kParams < 2) && y && ld_z >= N && ld_y >= N);
    const Slabs sl(M, N);
    hipLaunchKernelGGL(param_act_fwd_kernel<Act>, sl.grid, dim3(256), 0, as_stream(stream), z, ld_z, p0, p1, M, N, y,
                       ld_y, sl.rows);
    NERF_CHECK_LAUNCH();
    return NERF_OK;
}

// backward + the parameter gradients' reduce; M == 0 zeroes the gradients unless accumulate
template <class Act>
int act_bwd(const float* grad_y, int64_t ld_g, const float* z, int64_t ld_z, const float* p0, const float* p1,
            int64_t M, int N, float* grad_z, int64_t ld_dz, float* grad_p0, float* grad_p1, int accumulate,
            void* workspace, size_t workspace_bytes, void* stream) {
    constexpr int KP = Act::kParams;
    NERF_REQUIRE(M >= 0 && N >= 0);
    if (N == 0) return NERF_OK;
    float* const grad[2] = {grad_p0, grad_p1};
    NERF_REQUIRE(((p0 && grad_p0) || KP < 1) && ((p1 && grad_p1) || KP < 2));
    hipStream_t st = as_stream(stream);
    if (M == 0) {
        for (int p = 0; p < KP && !accumulate; ++p)
            if (hipMemsetAsync(grad[p], 0, (size_t)N * sizeof(float), st) != hipSuccess) return NERF_ERR_LAUNCH;
        return NERF_OK;
    }
    NERF_REQUIRE(grad_y && z && grad_z && ld_g >= N && ld_z >= N && ld_dz >= N);
    if (KP > 0 && (!workspace || workspace_bytes < act_workspace(KP, M, N) ||
                   (reinterpret_cast<uintptr_t>(workspace) & 7) != 0))
        return NERF_ERR_WORKSPACE;
    const Slabs sl(M, N);
    const int64_t plane = sl.n * N;
    double* partial = reinterpret_cast<double*>(workspace);
    hipLaunchKernelGGL(param_act_bwd_kernel<Act>, sl.grid, dim3(256), 0, st, grad_y, ld_g, z, ld_z, p0, p1, M, N,
                       grad_z, ld_dz, sl.rows, partial, plane);
    NERF_CHECK_LAUNCH();
    return nerf::param_act_reduce(KP, Act::kChain, partial, plane, sl.n, N, p0, grad, accumulate, partial + KP * plane,
                                  st);
}

bool kind_ok(int kind) { return kind == NERF_ACT_GABOR || kind == NERF_ACT_SARF; }

}  // namespace

size_t nerf::param_reduce_scratch(int N) { return (size_t)kMaxChunks * (size_t)(N > 0 ? N : 0) * sizeof(double); }

int nerf::param_reduce(const double* partial, int64_t slabs, int N, const float* s, float* dp, int accumulate,
                       double* scratch, hipStream_t st) {
    int64_t chunks = (slabs + 63) / 64;
    chunks = chunks < 1 ? 1 : (chunks > kMaxChunks ? kMaxChunks : chunks);
    const int64_t chunk = (slabs + chunks - 1) / chunks;
    chunks = (slabs + chunk - 1) / chunk;
    hipLaunchKernelGGL(param_reduce_chunks_kernel, dim3((unsigned)((N + kCols - 1) / kCols), (unsigned)chunks),
                       dim3(256), 0, st, partial, slabs, N, chunk, scratch);
    if (hipGetLastError() != hipSuccess) return NERF_ERR_LAUNCH;
    hipLaunchKernelGGL(param_reduce_final_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, scratch,
                       (int)chunks, N, s, dp, accumulate);
    if (hipGetLastError() != hipSuccess) return NERF_ERR_LAUNCH;
    return NERF_OK;
}

int nerf::param_act_reduce(int params, bool chain, const double* partial, int64_t plane, int64_t slabs, int N,
                           const float* p0, float* const* grad, int accumulate, double* scratch, hipStream_t st) {
    for (int p = 0; p < params; ++p) {
        const int rc = nerf::param_reduce(partial + p * plane, slabs, N, p == 0 && chain ? p0 : nullptr, grad[p],
                                          accumulate, scratch, st);
        if (rc != NERF_OK) return rc;
    }
    return NERF_OK;
}

// ------------------------------------------------------------------------- GARF's Gaussian
extern "C" size_t nerf_gauss_act_workspace(int64_t M, int32_t N) { return act_workspace(GaussFn::kParams, M, N); }

extern "C" int nerf_gauss_act_fwd(const float* z, int64_t ld_z, const float* inv_std, int64_t M, int32_t N, float* y,
                                  int64_t ld_y, void* stream) {
    return act_fwd<GaussFn>(z, ld_z, inv_std, nullptr, M, N, y, ld_y, stream);
}

extern "C" int nerf_gauss_act_bwd(const float* grad_y, int64_t ld_g, const float* z, int64_t ld_z,
                                  const float* inv_std, int64_t M, int32_t N, float* grad_z, int64_t ld_dz,
                                  float* grad_inv_std, int32_t accumulate, void* workspace, size_t workspace_bytes,
                                  void* stream) {
    return act_bwd<GaussFn>(grad_y, ld_g, z, ld_z, inv_std, nullptr, M, N, grad_z, ld_dz, grad_inv_std, nullptr,
                            accumulate, workspace, workspace_bytes, stream);
}

// ---------------------------------------------------------------------------- Gabor / Sarf
extern "C" size_t nerf_param_act_workspace(int32_t kind, int64_t M, int32_t N) {
    return kind_ok(kind) ? act_workspace(kind == NERF_ACT_GABOR ? 2 : 1, M, N) : 0;
}

extern "C" int nerf_param_act_fwd(int32_t kind, const float* z, int64_t ld_z, const float* p0, const float* p1,
                                  int64_t M, int32_t N, float* y, int64_t ld_y, void* stream) {
    NERF_REQUIRE(kind_ok(kind));
    return kind == NERF_ACT_GABOR ? act_fwd<GaborFn>(z, ld_z, p0, p1, M, N, y, ld_y, stream)
                                  : act_fwd<SarfFn>(z, ld_z, p0, p1, M, N, y, ld_y, stream);
}

extern "C" int nerf_param_act_bwd(int32_t kind, const float* grad_y, int64_t ld_g, const float* z, int64_t ld_z,
                                  const float* p0, const float* p1, int64_t M, int32_t N, float* grad_z,
                                  int64_t ld_dz, float* grad_p0, float* grad_p1, int32_t accumulate, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    NERF_REQUIRE(kind_ok(kind));
    return kind == NERF_ACT_GABOR
               ? act_bwd<GaborFn>(grad_y, ld_g, z, ld_z, p0, p1, M, N, grad_z, ld_dz, grad_p0, grad_p1, accumulate,
                                  workspace, workspace_bytes, stream)
               : act_bwd<SarfFn>(grad_y, ld_g, z, ld_z, p0, p1, M, N, grad_z, ld_dz, grad_p0, grad_p1, accumulate,
                                 workspace, workspace_bytes, stream);
}

// ---------------------------------------------------------------------------- SIREN's sine
extern "C" int nerf_sine_act_fwd(const float* z, int64_t ld_z, int64_t M, int32_t N, float* y, int64_t ld_y,
                                 void* stream) {
    return act_fwd<SineFn>(z, ld_z, nullptr, nullptr, M, N, y, ld_y, stream);
}

extern "C" int nerf_sine_act_bwd(const float* grad_y, int64_t ld_g, const float* z, int64_t ld_z, int64_t M,
                                 int32_t N, float* grad_z, int64_t ld_dz, void* stream) {
    return act_bwd<SineFn>(grad_y, ld_g, z, ld_z, nullptr, nullptr, M, N, grad_z, ld_dz, nullptr, nullptr, 0, nullptr,
                           0, stream);
}
