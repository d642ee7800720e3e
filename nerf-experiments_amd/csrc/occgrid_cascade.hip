// Cascaded occupancy-grid ray marching for unbounded scenes: `levels` nested boxes of one resolution,
// each twice the size of the one inside it, a step that grows with distance (cone_angle) and
// optional per-ray bounds.  nerfacc's OccGridEstimator(levels=L).sampling(cone_angle=...,
// t_min=..., t_max=...) restated (parity unpinned); the cascaded marching contract is the one in
// include/nerf_amd.h, which tests/_occgrid_cascade_ref.py restates in numpy fp32 bit for bit.  With one
// level, cone 0 and no ray bounds the outputs are those of occgrid.hip.
//
// Design: that of occgrid.hip, one 64-lane wavefront per ray and two passes around the caller's
// prefix sum, over the same workspace.  With cone == 0 lane l tests steps k = 64 j + l of the
// lattice.  With cone > 0 the steps are a recurrence, s_{k+1} = s_k + max(s_k * cone, dt): per chunk
// every lane runs the serial chain from the chunk's first s (three dependent operations per step,
// plus a compare and a select that stop lane l after l steps, at its own s_k), the last lane's
// s_{k+1} is the next chunk's first s; the cell test with its three divisions then runs one step per
// lane as before, the levels probed from the innermost until one holds the point.  Pass 2 reruns
// the identical chain (the same bits) and never tests the grid.  Every chunk loop is bounded by
// mask_words, every grid read follows the cell's range test, every store is guarded by the output's
// length.  No atomics except the OR into the status word, no LDS.
#include "occgrid_common.h"

using namespace nerf;

namespace {

struct OccCascade {
    float box[NERF_OCC_MAX_LEVELS][6];      // per level lo[3], hi[3]
    int res[3];
    int levels;
};

// s_{k+1} of the recurrence.  fmaxf is the contract's w > dt ? w : dt on every input that reaches it
// (dt is finite and positive; a NaN w gives dt either way) as one instruction.
__device__ __forceinline__ float chain_step(float s, float dt, float cone) {
#pragma clang fp contract(off)
    const float w = s * cone;
    return s + fmaxf(w, dt);
}

// One chunk of the recurrence from s = s_{64 j} (the same in every lane): lane l advances l times,
// so it ends at its own step's t0 = s_{64 j + l}; one more step gives e1, and lane 63's e1 is the
// next chunk's s.
__device__ __forceinline__ void chain_chunk(float& s, float dt, float cone, int lane, float& t0, float& e1) {
    float t = s;
#pragma unroll 16
    for (int i = 0; i < NERF_WAVE - 1; ++i) {
        const float nx = chain_step(t, dt, cone);
        t = lane > i ? nx : t;
    }
    t0 = t;
    e1 = chain_step(t, dt, cone);
    s = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, e1), NERF_WAVE - 1));
}

__device__ __forceinline__ bool wave_uniform(bool v) { return __builtin_amdgcn_readfirstlane((int)v) != 0; }

template <bool CONE>
__global__ __launch_bounds__(256) void occ_cascade_count_kernel(
    const float* __restrict__ rays_o, const float* __restrict__ rays_d, int64_t n_rays, OccCascade g,
    const uint32_t* __restrict__ bits, const float* __restrict__ t_lo, const float* __restrict__ t_hi, float near_,
    float far_, float dt, float cone, int stratified, uint64_t seed, uint64_t counter, int words, OccWorkspace ws,
    int32_t* __restrict__ status) {
#pragma clang fp contract(off)
    const int lane = lane_id();
    const int64_t ray = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ray >= n_rays) return;          // wave-uniform
    float o[3], d[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        o[a] = rays_o[ray * 3 + a];
        d[a] = rays_d[ray * 3 + a];
    }
    // slab test against the outermost box (every lane computes the same values)
    const float* outer = g.box[g.levels - 1];
    float tn = -INFINITY, tf = INFINITY;
    bool hit = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float lo = outer[a], hi = outer[3 + a];
        if (d[a] == 0.0f) {
            if (!(lo <= o[a] && o[a] < hi)) hit = false;
        } else {
            const float inv = 1.0f / d[a];
            const float ta = (lo - o[a]) * inv;
            const float tb = (hi - o[a]) * inv;
            const float mn = ta < tb ? ta : tb;
            const float mx = ta < tb ? tb : ta;
            tn = mn > tn ? mn : tn;
            tf = mx < tf ? mx : tf;
        }
    }
    float t_min = near_ > tn ? near_ : tn;
    float t_max = far_ < tf ? far_ : tf;
    if (t_lo) {
        const float b = t_lo[ray];
        t_min = b > t_min ? b : t_min;
    }
    if (t_hi) {
        const float b = t_hi[ray];
        t_max = b < t_max ? b : t_max;
    }
    hit = hit && (t_min < t_max);
    if (hit && stratified) t_min = t_min + philox_uniform(seed, counter, (uint64_t)ray) * dt;
    int n = 0;                          // steps considered: the lattice's n, or the chain's steps below t_max
    if (!CONE && hit) {
        const float x = ceilf((t_max - t_min) / dt);
        const float cap = (float)NERF_OCC_MAX_STEPS;
        if (x > cap && lane == 0) atomicOr(status, 1);
        n = x >= 1.0f ? (x < cap ? (int)x : NERF_OCC_MAX_STEPS) : 0;
        if (n > words * NERF_WAVE) {    // the caller's mask capacity is below the ray's step count
            if (lane == 0) atomicOr(status, 2);
            n = words * NERF_WAVE;
        }
    }
    const int64_t cells = (int64_t)g.res[0] * g.res[1] * g.res[2];
    unsigned long long* mrow = ws.masks + ray * words;
    int64_t count = 0;
    float s = t_min;                    // the chain's carry
    for (int j = 0; j < words; ++j) {
        float t0 = 0.0f, e1 = 0.0f;
        bool exists;
        if (CONE) {
            if (!wave_uniform(hit && s < t_max)) break;
            chain_chunk(s, dt, cone, lane, t0, e1);
            exists = t0 < t_max;
            n += __popcll(__ballot(exists));
        } else {
            if (j * NERF_WAVE >= n) break;
            const int k = j * NERF_WAVE + lane;
            exists = k < n;
            t0 = t_min + (float)k * dt;
            e1 = t_min + (float)(k + 1) * dt;
        }
        const float t1 = e1 < t_max ? e1 : t_max;
        const float tm = (t0 + t1) * 0.5f;
        const float p[3] = {o[0] + tm * d[0], o[1] + tm * d[1], o[2] + tm * d[2]};
        bool pending = exists && t0 < t1;   // no level found yet
        bool keep = false;
        for (int l = 0; l < g.levels && __ballot(pending) != 0ull; ++l) {
            const float* b = g.box[l];
            if (pending && b[0] <= p[0] && p[0] < b[3] && b[1] <= p[1] && p[1] < b[4] && b[2] <= p[2] && p[2] < b[5]) {
                pending = false;        // the smallest level that holds the point decides
                float c[3];
                bool in = true;
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    c[a] = floorf(((p[a] - b[a]) / (b[3 + a] - b[a])) * (float)g.res[a]);
                    in = in && (c[a] >= 0.0f) && (c[a] < (float)g.res[a]);
                }
                if (in) {               // the grid is read only for a cell inside it
                    const int64_t cell =
                        l * cells + ((int64_t)c[0] * g.res[1] + (int64_t)c[1]) * g.res[2] + (int64_t)c[2];
                    keep = (bits[cell >> 5] >> (cell & 31)) & 1u;
                }
            }
        }
        const unsigned long long m = __ballot(keep);
        if (lane == 0) mrow[j] = m;
        count += __popcll(m);
    }
    // a chain that stops below t_max was cut: at NERF_OCC_MAX_STEPS (bit 0) or at the mask capacity (bit 1)
    if (CONE && hit && s < t_max && lane == 0) atomicOr(status, words * NERF_WAVE >= NERF_OCC_MAX_STEPS ? 1 : 2);
    if (lane == 0) {
        ws.counts[ray] = count;
        ws.tmin[ray] = t_min;
        ws.tmax[ray] = t_max;
        ws.nsteps[ray] = n;
    }
}

template <bool CONE>
__global__ __launch_bounds__(256) void occ_cascade_write_kernel(int64_t n_rays, float dt, float cone, int words,
                                                                OccWorkspace ws, const int64_t* __restrict__ cum,
                                                                int64_t n_samples, int64_t* __restrict__ ray_indices,
                                                                float* __restrict__ t_starts,
                                                                float* __restrict__ t_ends) {
#pragma clang fp contract(off)
    const int lane = lane_id();
    const int64_t ray = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ray >= n_rays) return;
    const int64_t count = ws.counts[ray];
    if (count <= 0) return;
    int64_t base = cum[ray] - count;
    int n = ws.nsteps[ray];
    n = n < words * NERF_WAVE ? n : words * NERF_WAVE;
    const float t_min = ws.tmin[ray], t_max = ws.tmax[ray];
    const unsigned long long* mrow = ws.masks + ray * words;
    const unsigned long long below = (1ull << lane) - 1ull;
    float s = t_min;
    for (int j = 0; j * NERF_WAVE < n; ++j) {
        const unsigned long long m = mrow[j];
        float t0 = 0.0f, e1 = 0.0f;
        if (CONE) {
            chain_chunk(s, dt, cone, lane, t0, e1);
        } else {
            const int k = j * NERF_WAVE + lane;
            t0 = t_min + (float)k * dt;
            e1 = t_min + (float)(k + 1) * dt;
        }
        const int64_t slot = base + __popcll(m & below);
        if (((m >> lane) & 1ull) && slot >= 0 && slot < n_samples) {
            ray_indices[slot] = ray;
            t_starts[slot] = t0;
            t_ends[slot] = e1 < t_max ? e1 : t_max;
        }
        base += __popcll(m);
    }
}

bool valid_cone(float cone) { return cone >= 0.0f && cone < INFINITY; }

}  // namespace

extern "C" int nerf_occ_cascade_count(const float* rays_o, const float* rays_d, int64_t n_rays, const float* aabbs,
                                      int32_t levels, const int32_t* resolution, const uint32_t* grid_bits,
                                      const float* t_lo, const float* t_hi, float near_plane, float far_plane,
                                      float step_size, float cone_angle, int32_t stratified, uint64_t seed,
                                      uint64_t counter, int32_t mask_words, void* workspace, size_t workspace_bytes,
                                      int32_t* status, void* stream) {
    NERF_REQUIRE(n_rays >= 0 && occ_valid_words(mask_words) && aabbs && resolution);
    NERF_REQUIRE(levels >= 1 && levels <= NERF_OCC_MAX_LEVELS);
    NERF_REQUIRE(step_size > 0.0f && step_size < INFINITY && valid_cone(cone_angle));
    OccCascade g = {};
    g.levels = levels;
    int64_t cells = 1;
    for (int a = 0; a < 3; ++a) {
        g.res[a] = resolution[a];
        NERF_REQUIRE(g.res[a] >= 1 && g.res[a] <= 4096);
        cells *= g.res[a];
    }
    NERF_REQUIRE(cells <= (1ll << 31));
    for (int l = 0; l < levels; ++l)
        for (int a = 0; a < 3; ++a) {
            const float lo = aabbs[l * 6 + a], hi = aabbs[l * 6 + 3 + a];
            NERF_REQUIRE(lo < hi && hi - lo < INFINITY);
            g.box[l][a] = lo;
            g.box[l][3 + a] = hi;
        }
    if (n_rays == 0) return NERF_OK;
    NERF_REQUIRE(rays_o && rays_d && grid_bits && workspace && status);
    NERF_REQUIRE(occ_aligned(rays_o, 4) && occ_aligned(rays_d, 4) && occ_aligned(grid_bits, 4) &&
                 occ_aligned(status, 4) && occ_aligned(t_lo, 4) && occ_aligned(t_hi, 4));
    NERF_REQUIRE((n_rays + 3) / 4 < (1ll << 31));
    if (workspace_bytes < occ_workspace_bytes(n_rays, mask_words)) return NERF_ERR_WORKSPACE;
    NERF_REQUIRE(occ_aligned(workspace, 256));
    dim3 grid((unsigned)((n_rays + 3) / 4)), block(256);
    auto kernel = cone_angle > 0.0f ? occ_cascade_count_kernel<true> : occ_cascade_count_kernel<false>;
    hipLaunchKernelGGL(kernel, grid, block, 0, as_stream(stream), rays_o, rays_d, n_rays, g, grid_bits, t_lo, t_hi,
                       near_plane, far_plane, step_size, cone_angle, stratified, seed, counter, mask_words,
                       occ_carve(workspace, n_rays), status);
    NERF_CHECK_LAUNCH();
    return NERF_OK;
}

extern "C" int nerf_occ_cascade_write(int64_t n_rays, float step_size, float cone_angle, int32_t mask_words,
                                      const void* workspace, size_t workspace_bytes, const int64_t* offsets_incl,
                                      int64_t n_samples, int64_t* ray_indices, float* t_starts, float* t_ends,
                                      void* stream) {
    NERF_REQUIRE(n_rays >= 0 && n_samples >= 0 && occ_valid_words(mask_words));
    NERF_REQUIRE(step_size > 0.0f && step_size < INFINITY && valid_cone(cone_angle));
    if (n_rays == 0 || n_samples == 0) return NERF_OK;
    NERF_REQUIRE(workspace && offsets_incl && ray_indices && t_starts && t_ends);
    NERF_REQUIRE(occ_aligned(offsets_incl, 8) && occ_aligned(ray_indices, 8) && occ_aligned(t_starts, 4) &&
                 occ_aligned(t_ends, 4));
    NERF_REQUIRE((n_rays + 3) / 4 < (1ll << 31));
    if (workspace_bytes < occ_workspace_bytes(n_rays, mask_words)) return NERF_ERR_WORKSPACE;
    NERF_REQUIRE(occ_aligned(workspace, 256));
    dim3 grid((unsigned)((n_rays + 3) / 4)), block(256);
    auto kernel = cone_angle > 0.0f ? occ_cascade_write_kernel<true> : occ_cascade_write_kernel<false>;
    hipLaunchKernelGGL(kernel, grid, block, 0, as_stream(stream), n_rays, step_size, cone_angle, mask_words,
                       occ_carve(const_cast<void*>(workspace), n_rays), offsets_incl, n_samples, ray_indices,
                       t_starts, t_ends);
    NERF_CHECK_LAUNCH();
    return NERF_OK;
}
