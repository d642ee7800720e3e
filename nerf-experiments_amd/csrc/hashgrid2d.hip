// 2-D multiresolution hash-grid encoding: INGPTable / INGPEncoding of the reference's
// 2d-ingp/model.py:13-115 (the Gigapixel image fit), as oracle/hashgrid_oracle.py::level_corners_2d /
// encode_2d restate it and tests/golden/hashgrid2d.npz, ingp2d.npz pin it.  Contract in
// include/nerf_amd.h (nerf_hashgrid2d_*).  New entry points only: the 3-D file, its kernels and
// hashgrid_common.h are untouched (this file includes the header for hash_row alone; the gmax, shift
// and finish helpers are duplicated here with 4 corners for 8, so no 3-D kernel is recompiled from
// different text).
//
// Table layout = the reference's parameters: one [rows_l][F] table per level, rows_l = (r+1)^2 for a
// bijective level ((r+1)^2 <= T), T otherwise, packed back to back.
//
// Forward, per level in fp32 with contraction off: x_hat = x r; corners floor(x_hat) + (0,0), (0,1),
// (1,0), (1,1) in that order; row = cx + (r+1) cy on the unclipped corner (bijective) or
// ((cx pi1) ^ (cy pi2)) mod T in int64 (hash_row with a zero third coordinate); weight
// (1 - |x_hat_0 - cx|) (1 - |x_hat_1 - cy|); out = sum_k w_k table[row_k], products rounded, then
// added in corner order.  The corner coordinates as floats are floor(x_hat) and floor(x_hat) + 1.0f:
// the reference converts its int64 corners back to fp32 for the weights, and both are the correctly
// rounded value of the same integer.
//
// Domain: a bijective-level corner with cx or cy outside [0, r] (a point outside [0,1)^2, or NaN)
// is dropped — no load, no add, forward and backward — and sets bit 0 of *status.  Hashed levels are
// in range by construction.
//
// Backward (table gradient only): as hashgrid.hip, every contribution w g rounded to a 64-bit
// fixed-point integer at 2^s, s from the batch's max |g| with 4 n gmax 2^s < 2^62, added with integer
// atomics (order-independent), then scaled back.  A level is cut into parts of PART_ENTRIES
// accumulators held in LDS; one workgroup per (part, slab of samples) adds the corners that fall in
// its part with LDS atomics and flushes the part with one contiguous pass of global atomics.  A level
// of at most PART_ENTRIES accumulators (every bijective level up to r = 100 at F = 2) is one part:
// its thousands of adders per row at image-sized batches never leave the chip.  For the larger levels
// the alternative, 64-bit global atomics straight from one thread per (sample, level), measured 980
// against 217 us per call at n = 2^18 (36 against 25 us at n = 2560), so they take the
// same per-part walk.
#include "common.h"
#include "hashgrid_common.h"

namespace {
using namespace nerf;

struct Hash2Args {
    nerf_hashgrid_params p;
    int64_t off[NERF_HASHGRID_MAX_LEVELS];          // first row of each level in the packed table
    const float* x;                                 // [n][2]
    int64_t n;
    int32_t* status;                                // optional
};

struct Corners2 {
    int idx[4];           // table rows (< T < 2^31); -1: out of the bijective level's domain
    float w[4];
    bool oob;             // some corner was dropped
};

// rows of a level's table: (r+1)^2 when bijective, else T
__host__ __device__ inline int64_t level_rows2(int r, int T) {
    const int64_t r1 = r + 1;
    return r1 * r1 <= T ? r1 * r1 : T;
}

template <typename PR>
__device__ __forceinline__ Corners2 level_corners2(float px, float py, int r, int T, const PR& primes) {
#pragma clang fp contract(off)
    Corners2 c;
    c.oob = false;
    const float xh0 = px * (float)r, xh1 = py * (float)r;
    const float f0 = floorf(xh0), f1 = floorf(xh1);
    const float wx[2] = {1.0f - fabsf(xh0 - f0), 1.0f - fabsf(xh0 - (f0 + 1.0f))};
    const float wy[2] = {1.0f - fabsf(xh1 - f1), 1.0f - fabsf(xh1 - (f1 + 1.0f))};
#pragma unroll
    for (int k = 0; k < 4; ++k) c.w[k] = wx[k >> 1] * wy[k & 1];
    const int r1 = r + 1;
    if ((long long)r1 * r1 <= (long long)T) {
        bool okx[2], oky[2];
        int qx[2], qy[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const float vx = e ? f0 + 1.0f : f0, vy = e ? f1 + 1.0f : f1;
            okx[e] = vx >= 0.0f && vx <= (float)r;          // false for NaN
            oky[e] = vy >= 0.0f && vy <= (float)r;
            qx[e] = okx[e] ? (int)vx : 0;
            qy[e] = oky[e] ? r1 * (int)vy : 0;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool ok = okx[k >> 1] && oky[k & 1];
            c.idx[k] = ok ? qx[k >> 1] + qy[k & 1] : -1;
            c.oob = c.oob || !ok;
        }
        return c;
    }
    const bool pow2 = (T & (T - 1)) == 0;
    const bool small = fabsf(xh0) < 1073741824.0f && fabsf(xh1) < 1073741824.0f;
    if (pow2 && small) {
        // modulo a power of two only the low 32 bits of corners and primes matter
        const unsigned pr0 = (unsigned)(long long)primes[0], pr1 = (unsigned)(long long)primes[1];
        const int b0 = (int)f0, b1 = (int)f1;
        const unsigned hx[2] = {(unsigned)b0 * pr0, (unsigned)(b0 + 1) * pr0};
        const unsigned hy[2] = {(unsigned)b1 * pr1, (unsigned)(b1 + 1) * pr1};
#pragma unroll
        for (int k = 0; k < 4; ++k) c.idx[k] = (int)((hx[k >> 1] ^ hy[k & 1]) & (unsigned)(T - 1));
        return c;
    }
    const long long b0 = (long long)f0, b1 = (long long)f1;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long long cc[3] = {(long long)((unsigned long long)b0 + (unsigned)(k >> 1)),
                                 (long long)((unsigned long long)b1 + (unsigned)(k & 1)), 0};
        c.idx[k] = hash_row(cc, (long long)primes[0], (long long)primes[1], 0, T, pow2);
    }
    return c;
}

// one atomic OR per wave that saw a dropped corner
__device__ __forceinline__ void flag_oob(int32_t* status, bool oob) {
    if (status == nullptr) return;
    const unsigned long long m = __ballot(oob);
    if (oob && lane_id() == __builtin_ctzll(m)) atomicOr(status, 1);
}

// Forward: 64 samples per workgroup, one wave per level (levels beyond the workgroup's waves in
// further trips), so a wave's gathers hit one level's table and neighbouring samples (pixel centres
// in image order) neighbouring rows; the workgroup's features are staged in LDS and written as whole
// [64][L F] output rows (scattered per-level row pieces amplify writes, see hashgrid.hip).  All four
// rows of a corner set are loaded before the sums (F = 2: as 8-byte loads when the table is 8-byte
// aligned).  The one-thread-per-(sample, level) form was built and timed against this one: equal at
// the training batch and on a render chunk, 74 against 68 us at 2^18 random points.
constexpr int TILE_SAMPLES = 64;
template <int F>
__global__ __launch_bounds__(1024) void hashgrid2d_fwd_tile_kernel(Hash2Args a, const float* __restrict__ table,
                                                                   float* __restrict__ out, int64_t ld, int vec2) {
#pragma clang fp contract(off)
    __shared__ float rows[TILE_SAMPLES * (NERF_HASHGRID_MAX_LEVELS * F + 1)];
    const int L = a.p.levels, T = a.p.table_size, cols = L * F, rld = cols + 1;
    const int nw = (int)(blockDim.x >> 6), wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    const int64_t n0 = (int64_t)blockIdx.x * TILE_SAMPLES;
    const int64_t n = n0 + lane;
    if (n < a.n) {
        const float px = a.x[n * 2 + 0], py = a.x[n * 2 + 1];
        for (int l = wave; l < L; l += nw) {
            const Corners2 c = level_corners2(px, py, a.p.res[l], T, a.p.primes);
            const float* tab = table + a.off[l] * F;
            float v[4][F];
            if (F == 2 && vec2) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float2 q = c.idx[k] >= 0 ? *reinterpret_cast<const float2*>(tab + (int64_t)c.idx[k] * 2)
                                                   : make_float2(0.0f, 0.0f);
                    v[k][0] = q.x;
                    v[k][F - 1] = q.y;
                }
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
#pragma unroll
                    for (int f = 0; f < F; ++f) v[k][f] = c.idx[k] >= 0 ? tab[(int64_t)c.idx[k] * F + f] : 0.0f;
            }
            float acc[F];
#pragma unroll
            for (int f = 0; f < F; ++f) acc[f] = 0.0f;
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int f = 0; f < F; ++f) acc[f] = c.idx[k] >= 0 ? acc[f] + c.w[k] * v[k][f] : acc[f];
#pragma unroll
            for (int f = 0; f < F; ++f) rows[lane * rld + l * F + f] = acc[f];
            flag_oob(a.status, c.oob);
        }
    }
    __syncthreads();
    const int64_t left = a.n - n0;
    const int nr = left < TILE_SAMPLES ? (int)left : TILE_SAMPLES;
    for (int e = threadIdx.x; e < nr * cols; e += blockDim.x) {
        const int r = e / cols, cc = e - r * cols;
        out[(n0 + r) * ld + cc] = rows[r * rld + cc];
    }
}

template <int F>
void launch_fwd_tile(hipStream_t s, const Hash2Args& a, const float* table, float* out, int64_t ld, int vec2) {
    const int waves = a.p.levels < 16 ? a.p.levels : 16;
    hipLaunchKernelGGL(hashgrid2d_fwd_tile_kernel<F>, dim3((unsigned)((a.n + TILE_SAMPLES - 1) / TILE_SAMPLES)),
                       dim3(64 * waves), 0, s, a, table, out, ld, vec2);
}

// max |grad_out| over the batch as the bits of a non-negative float (order-preserving as uint32);
// non-finite values land above every finite one
template <int V>
__global__ __launch_bounds__(256) void hashgrid2d_gmax_kernel(const float* __restrict__ g, int64_t ld, int64_t n,
                                                              int cols, unsigned* __restrict__ gmax) {
    const int cv = cols / V;
    const int64_t total = n * cv;
    unsigned m = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / cv;
        const float* p = g + r * ld + (i - r * cv) * V;
        float v[V];
        if constexpr (V == 4) {
            const float4 q = *reinterpret_cast<const float4*>(p);
            v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
        } else {
            v[0] = p[0];
        }
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const unsigned b = __float_as_uint(fabsf(v[j]));
            m = b > m ? b : m;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned o = __shfl_xor(m, off, 64);
        m = o > m ? o : m;
    }
    // one atomic per block (same-address atomics serialise at the memory side)
    __shared__ unsigned wm[4];
    if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = wm[0] > wm[1] ? wm[0] : wm[1];
        m = m > wm[2] ? m : wm[2];
        m = m > wm[3] ? m : wm[3];
        if (m != 0) atomicMax(gmax, m);
    }
}

// fixed-point exponent s with 4 * n * gmax * 2^s < 2^62 (no entry can overflow); -1000 flags a
// non-finite gradient
__device__ __forceinline__ int fixed_shift2(unsigned gmax_bits, int64_t n) {
    const float gm = __uint_as_float(gmax_bits);
    if (!(gm < INFINITY)) return -1000;
    if (gm == 0.0f) return 60;
    const double bound = 4.0 * (double)n * (double)gm;
    int e;
    frexp(bound, &e);                       // bound < 2^e
    const int s = 62 - e;
    return s > 120 ? 120 : s;
}

constexpr int PART_ENTRIES = 20480;         // all 160 KiB of LDS as int64 accumulators
constexpr int BWD_THREADS = 1024;
constexpr int BWD_UNROLL = 4;               // samples per thread and trip, their loads issued together

struct Bwd2Plan {
    int start[NERF_HASHGRID_MAX_LEVELS + 1];        // prefix of parts per level
    int rows_per_part;
    int parts;                                      // parts of all levels (workgroups per slab)
    int64_t slab;                                   // samples per slab
};

// round-to-nearest-even of |x| < 2^51 to int64 (llrint's value), see hashgrid.hip
__device__ __forceinline__ long long rint_fixed2(double x) {
#pragma clang fp contract(off)
    const double m = 6755399441055744.0;
    return __builtin_bit_cast(long long, x + m) - __builtin_bit_cast(long long, m);
}

// One workgroup per (part, slab).  SMALL: n >= 512, so that every contribution |w g 2^s| <= gmax 2^s
// < 2^62 / (4 n) <= 2^51 rounds with rint_fixed2.
template <int F, bool SMALL>
__device__ __forceinline__ void walk_part2(const Hash2Args& a, int l, int64_t row0, int prow, double scale,
                                           int64_t n_begin, int64_t n_end, const float* __restrict__ g, int64_t ld,
                                           unsigned long long* part) {
#pragma clang fp contract(off)
    const int res = a.p.res[l], T = a.p.table_size;
    for (int64_t base = n_begin; base < n_end; base += BWD_UNROLL * BWD_THREADS) {
        const int64_t nb = base + threadIdx.x;
        float px[BWD_UNROLL], py[BWD_UNROLL], gv[BWD_UNROLL][F];
        // loads first (indices clamped into the range, so every load is in bounds)
#pragma unroll
        for (int u = 0; u < BWD_UNROLL; ++u) {
            const int64_t n = nb + u * BWD_THREADS < n_end ? nb + u * BWD_THREADS : n_end - 1;
            px[u] = a.x[n * 2 + 0];
            py[u] = a.x[n * 2 + 1];
#pragma unroll
            for (int f = 0; f < F; ++f) gv[u][f] = g[n * ld + (int64_t)l * F + f];
        }
#pragma unroll
        for (int u = 0; u < BWD_UNROLL; ++u) {
            if (nb + u * BWD_THREADS >= n_end) continue;
            const Corners2 c = level_corners2(px[u], py[u], res, T, a.p.primes);
            // w g 2^s = w (g 2^s): both products exact in fp64 (24-bit mantissas, power-of-two scale)
            double gs[F];
#pragma unroll
            for (int f = 0; f < F; ++f) gs[f] = (double)gv[u][f] * scale;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                // a dropped corner (-1) is below every part
                const int64_t rel = (int64_t)c.idx[k] - row0;
                if ((uint64_t)rel < (uint64_t)prow) {
                    const double wk = (double)c.w[k];
#pragma unroll
                    for (int f = 0; f < F; ++f) {
                        const double x = wk * gs[f];
                        const long long q = SMALL ? rint_fixed2(x) : llrint(x);
                        atomicAdd(&part[(int)rel * F + f], (unsigned long long)q);
                    }
                }
            }
        }
    }
}

template <int F>
__global__ __launch_bounds__(BWD_THREADS) void hashgrid2d_bwd_kernel(Hash2Args a, Bwd2Plan pl,
                                                                     const float* __restrict__ g, int64_t ld,
                                                                     const unsigned* __restrict__ gmax,
                                                                     unsigned long long* __restrict__ acc) {
    __shared__ unsigned long long part[PART_ENTRIES];
    const int w = (int)(blockIdx.x % (unsigned)pl.parts);
    const int64_t slab = blockIdx.x / (unsigned)pl.parts;
    int l = 0;
    while (w >= pl.start[l + 1]) ++l;
    const int64_t row0 = (int64_t)(w - pl.start[l]) * pl.rows_per_part;
    const int64_t rows = level_rows2(a.p.res[l], a.p.table_size) - row0;
    const int prow = (int)(rows < pl.rows_per_part ? rows : pl.rows_per_part);
    const int s = fixed_shift2(*gmax, a.n);
    if (s == -1000) return;                         // uniform: the finish pass writes NaN
    const double scale = ldexp(1.0, s);
    for (int e = threadIdx.x; e < prow * F; e += BWD_THREADS) part[e] = 0ull;
    __syncthreads();
    const int64_t n0 = slab * pl.slab;
    const int64_t n1 = n0 + pl.slab < a.n ? n0 + pl.slab : a.n;
    if (a.n >= 512)
        walk_part2<F, true>(a, l, row0, prow, scale, n0, n1, g, ld, part);
    else
        walk_part2<F, false>(a, l, row0, prow, scale, n0, n1, g, ld, part);
    __syncthreads();
    // the part's accumulators out to the global ones: one contiguous pass of atomics
    unsigned long long* dst = acc + (a.off[l] + row0) * F;
    for (int e = threadIdx.x; e < prow * F; e += BWD_THREADS) {
        const unsigned long long v = part[e];
        if (v != 0ull) atomicAdd(dst + e, v);
    }
}

template <int F>
void launch_bwd(hipStream_t s, int64_t blocks, const Hash2Args& a, const Bwd2Plan& pl, const float* g, int64_t ld,
                const unsigned* gmax, unsigned long long* acc) {
    if (blocks > 0)
        hipLaunchKernelGGL(hashgrid2d_bwd_kernel<F>, dim3((unsigned)blocks), dim3(BWD_THREADS), 0, s, a, pl, g, ld, gmax,
                           acc);
}

// table gradient = accumulator * 2^-s (or NaN after a non-finite gradient)
__global__ __launch_bounds__(256) void hashgrid2d_finish_kernel(const unsigned long long* __restrict__ acc,
                                                                int64_t count, const unsigned* __restrict__ gmax,
                                                                int64_t n, float* __restrict__ grad, int accumulate) {
    const int s = fixed_shift2(*gmax, n);
    const double inv = s == -1000 ? 0.0 : ldexp(1.0, -s);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) {
        const long long q = (long long)acc[i];
        const float v = s == -1000 ? NAN : (float)((double)q * inv);
        grad[i] = accumulate ? grad[i] + v : v;
    }
}

int num_cus() {
    static int n = 0;
    if (n == 0) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
            n = 256;
    }
    return n;
}

bool valid_params(const nerf_hashgrid_params* p) {
    if (p == nullptr || p->levels < 1 || p->levels > NERF_HASHGRID_MAX_LEVELS) return false;
    if (p->features < 1 || p->features > NERF_HASHGRID_MAX_FEATURES || p->table_size < 1) return false;
    if ((int64_t)p->levels * p->table_size * p->features >= ((int64_t)1 << 31)) return false;
    for (int l = 0; l < p->levels; ++l)
        if (p->res[l] < 1 || p->res[l] > (1 << 20)) return false;
    return p->normalize == 0;
}

int64_t total_rows(const nerf_hashgrid_params* p) {
    int64_t rows = 0;
    for (int l = 0; l < p->levels; ++l) rows += level_rows2(p->res[l], p->table_size);
    return rows;
}

Hash2Args make_args(const nerf_hashgrid_params* p, const float* x, int64_t n, int32_t* status) {
    Hash2Args a{};
    a.p = *p;
    int64_t r = 0;
    for (int l = 0; l < p->levels; ++l) {
        a.off[l] = r;
        r += level_rows2(p->res[l], p->table_size);
    }
    a.x = x, a.n = n, a.status = status;
    return a;
}

}  // namespace

extern "C" int64_t nerf_hashgrid2d_table_rows(const nerf_hashgrid_params* params, int32_t level) {
    if (!valid_params(params) || level >= params->levels) return -1;
    return level < 0 ? total_rows(params) : level_rows2(params->res[level], params->table_size);
}

extern "C" int nerf_hashgrid2d_fwd(const nerf_hashgrid_params* params, const float* x, int64_t n, const float* table,
                                   float* out, int64_t out_ld, int32_t* status, void* stream) {
    NERF_REQUIRE(valid_params(params) && n >= 0);
    NERF_REQUIRE(out_ld >= (int64_t)params->levels * params->features);
    if (n == 0) return NERF_OK;
    NERF_REQUIRE(x != nullptr && table != nullptr && out != nullptr);
    const Hash2Args a = make_args(params, x, n, status);
    const int vec2 = (reinterpret_cast<uintptr_t>(table) & 7) == 0;
    hipStream_t st = as_stream(stream);
    NERF_REQUIRE((n + TILE_SAMPLES - 1) / TILE_SAMPLES < (1ll << 31));
    switch (params->features) {
        case 1: launch_fwd_tile<1>(st, a, table, out, out_ld, vec2); break;
        case 2: launch_fwd_tile<2>(st, a, table, out, out_ld, vec2); break;
        case 3: launch_fwd_tile<3>(st, a, table, out, out_ld, vec2); break;
        case 4: launch_fwd_tile<4>(st, a, table, out, out_ld, vec2); break;
        case 5: launch_fwd_tile<5>(st, a, table, out, out_ld, vec2); break;
        case 6: launch_fwd_tile<6>(st, a, table, out, out_ld, vec2); break;
        case 7: launch_fwd_tile<7>(st, a, table, out, out_ld, vec2); break;
        default: launch_fwd_tile<8>(st, a, table, out, out_ld, vec2); break;
    }
    NERF_CHECK_LAUNCH();
    return NERF_OK;
}

// [256-byte header: the max |grad_out| bits][accumulators: rows x F int64]
extern "C" size_t nerf_hashgrid2d_workspace(const nerf_hashgrid_params* params) {
    if (!valid_params(params)) return 0;
    return 256 + (size_t)total_rows(params) * params->features * sizeof(unsigned long long);
}

extern "C" int nerf_hashgrid2d_bwd(const nerf_hashgrid_params* params, const float* x, int64_t n, const float* grad_out,
                                   int64_t g_ld, float* grad_table, int32_t accumulate, void* workspace,
                                   size_t workspace_bytes, void* stream) {
    NERF_REQUIRE(valid_params(params) && n >= 0);
    NERF_REQUIRE(g_ld >= (int64_t)params->levels * params->features);
    NERF_REQUIRE(n == 0 || (x != nullptr && grad_out != nullptr && grad_table != nullptr && workspace != nullptr));
    if (workspace != nullptr) {
        if (workspace_bytes < nerf_hashgrid2d_workspace(params)) return NERF_ERR_WORKSPACE;
        NERF_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0);
    }
    const int64_t count = total_rows(params) * params->features;
    hipStream_t s = as_stream(stream);
    if (n == 0) {
        // nothing to add: a plain gradient is zero, an accumulated one unchanged (no kernel)
        if (!accumulate && grad_table != nullptr &&
            hipMemsetAsync(grad_table, 0, (size_t)count * sizeof(float), s) != hipSuccess)
            return NERF_ERR_LAUNCH;
        return NERF_OK;
    }
    const int F = params->features, cols = params->levels * F;
    Bwd2Plan pl{};
    pl.rows_per_part = PART_ENTRIES / F;
    for (int l = 0; l < params->levels; ++l) {
        const int64_t rows = level_rows2(params->res[l], params->table_size);
        pl.start[l + 1] = pl.start[l] + (int)((rows + pl.rows_per_part - 1) / pl.rows_per_part);
    }
    pl.parts = pl.start[params->levels];
    // One 1024-thread workgroup (160 KiB of LDS) runs per CU: about one round of workgroups, slabs of
    // at least one 4096-sample trip (every slab flushes its parts, so no more slabs than fill the card)
    const int64_t G = num_cus(), most = (n + BWD_UNROLL * BWD_THREADS - 1) / (BWD_UNROLL * BWD_THREADS);
    int64_t slabs = pl.parts > 0 ? (G + pl.parts / 2) / pl.parts : 1;
    slabs = slabs < 1 ? 1 : (slabs > most ? most : slabs);
    pl.slab = (n + slabs - 1) / slabs;
    slabs = (n + pl.slab - 1) / pl.slab;
    NERF_REQUIRE(slabs * pl.parts < (1ll << 31));
    unsigned* gmax = static_cast<unsigned*>(workspace);
    unsigned long long* acc = reinterpret_cast<unsigned long long*>(static_cast<char*>(workspace) + 256);
    // header and accumulators zeroed by every call (no state carried between calls)
    if (hipMemsetAsync(workspace, 0, 256 + (size_t)count * sizeof(unsigned long long), s) != hipSuccess)
        return NERF_ERR_LAUNCH;
    const Hash2Args a = make_args(params, x, n, nullptr);
    const bool vec = cols % 4 == 0 && g_ld % 4 == 0 && (reinterpret_cast<uintptr_t>(grad_out) & 15) == 0;
    int64_t blocks = (n * (vec ? cols / 4 : cols) + 255) / 256;
    blocks = blocks < 1024 ? blocks : 1024;
    if (vec)
        hipLaunchKernelGGL(hashgrid2d_gmax_kernel<4>, dim3((unsigned)blocks), dim3(256), 0, s, grad_out, g_ld, n, cols,
                           gmax);
    else
        hipLaunchKernelGGL(hashgrid2d_gmax_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, s, grad_out, g_ld, n, cols,
                           gmax);
    NERF_CHECK_LAUNCH();
    const int64_t wg = slabs * pl.parts;
    switch (F) {
        case 1: launch_bwd<1>(s, wg, a, pl, grad_out, g_ld, gmax, acc); break;
        case 2: launch_bwd<2>(s, wg, a, pl, grad_out, g_ld, gmax, acc); break;
        case 3: launch_bwd<3>(s, wg, a, pl, grad_out, g_ld, gmax, acc); break;
        case 4: launch_bwd<4>(s, wg, a, pl, grad_out, g_ld, gmax, acc); break;
        case 5: launch_bwd<5>(s, wg, a, pl, grad_out, g_ld, gmax, acc); break;
        case 6: launch_bwd<6>(s, wg, a, pl, grad_out, g_ld, gmax, acc); break;
        case 7: launch_bwd<7>(s, wg, a, pl, grad_out, g_ld, gmax, acc); break;
        default: launch_bwd<8>(s, wg, a, pl, grad_out, g_ld, gmax, acc); break;
    }
    NERF_CHECK_LAUNCH();
    int64_t fb = (count + 255) / 256;
    fb = fb < 4096 ? fb : 4096;
    hipLaunchKernelGGL(hashgrid2d_finish_kernel, dim3((unsigned)fb), dim3(256), 0, s, acc, count, gmax, n, grad_table,
                       accumulate);
    NERF_CHECK_LAUNCH();
    return NERF_OK;
}
