// Occupancy-grid ray marching (empty-space skipping): a fixed-step lattice along each ray, kept
// where the step's midpoint falls in a set cell of a one-level binary grid.  nerfacc's
// OccGridEstimator.sampling restated (parity unpinned); the marching contract is the one in
// include/nerf_amd.h, which tests/_occgrid_ref.py restates in numpy fp32 bit for bit.
//
// Design: one 64-lane wavefront per ray, lane l tests steps k = 64 j + l.  Pass 1 (count) stores
// each chunk's 64-bit ballot mask, the ray's kept count and its (t_min, t_max, n) in the caller's
// workspace; the caller turns the counts into offsets (an inclusive prefix sum); pass 2 (write)
// derives every slot from the stored masks by a popcount of the lower lanes.  Pass 2 never tests
// the grid again, so the two passes cannot disagree on what is kept.  Every loop is bounded by
// n <= 64 * mask_words <= NERF_OCC_MAX_STEPS, every grid read follows the cell's range test, every
// store is guarded by the output's length.  No atomics except the OR into the status word, no LDS.
#include "occgrid_common.h"

using namespace nerf;

namespace {

struct OccGrid {
    float lo[3], hi[3];
    int res[3];
};

__global__ __launch_bounds__(256) void occ_march_count_kernel(const float* __restrict__ rays_o,
                                                              const float* __restrict__ rays_d, int64_t n_rays,
                                                              OccGrid g, const uint32_t* __restrict__ bits,
                                                              float near_, float far_, float dt, int stratified,
                                                              uint64_t seed, uint64_t counter, int words,
                                                              OccWorkspace ws, int32_t* __restrict__ status) {
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
    // slab test (every lane computes the same values)
    float tn = -INFINITY, tf = INFINITY;
    bool hit = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (d[a] == 0.0f) {
            if (!(g.lo[a] <= o[a] && o[a] < g.hi[a])) hit = false;
        } else {
            const float inv = 1.0f / d[a];
            const float ta = (g.lo[a] - o[a]) * inv;
            const float tb = (g.hi[a] - o[a]) * inv;
            const float mn = ta < tb ? ta : tb;
            const float mx = ta < tb ? tb : ta;
            tn = mn > tn ? mn : tn;
            tf = mx < tf ? mx : tf;
        }
    }
    float t_min = near_ > tn ? near_ : tn;
    const float t_max = far_ < tf ? far_ : tf;
    hit = hit && (t_min < t_max);
    int n = 0;
    if (hit) {
        if (stratified) t_min = t_min + philox_uniform(seed, counter, (uint64_t)ray) * dt;
        const float x = ceilf((t_max - t_min) / dt);
        const float cap = (float)NERF_OCC_MAX_STEPS;
        if (x > cap && lane == 0) atomicOr(status, 1);
        n = x >= 1.0f ? (x < cap ? (int)x : NERF_OCC_MAX_STEPS) : 0;
        if (n > words * NERF_WAVE) {    // the caller's mask capacity is below the ray's step count
            if (lane == 0) atomicOr(status, 2);
            n = words * NERF_WAVE;
        }
    }
    unsigned long long* mrow = ws.masks + ray * words;
    int64_t count = 0;
    const float ext[3] = {g.hi[0] - g.lo[0], g.hi[1] - g.lo[1], g.hi[2] - g.lo[2]};
    for (int j = 0; j * NERF_WAVE < n; ++j) {
        const int k = j * NERF_WAVE + lane;
        bool keep = false;
        if (k < n) {
            const float t0 = t_min + (float)k * dt;
            const float e1 = t_min + (float)(k + 1) * dt;
            const float t1 = e1 < t_max ? e1 : t_max;
            if (t0 < t1) {
                const float tm = (t0 + t1) * 0.5f;
                float c[3];
                bool in = true;
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const float p = o[a] + tm * d[a];
                    c[a] = floorf(((p - g.lo[a]) / ext[a]) * (float)g.res[a]);
                    in = in && (c[a] >= 0.0f) && (c[a] < (float)g.res[a]);
                }
                if (in) {               // the grid is read only for a cell inside it
                    const int64_t cell = ((int64_t)c[0] * g.res[1] + (int64_t)c[1]) * g.res[2] + (int64_t)c[2];
                    keep = (bits[cell >> 5] >> (cell & 31)) & 1u;
                }
            }
        }
        const unsigned long long m = __ballot(keep);
        if (lane == 0) mrow[j] = m;
        count += __popcll(m);
    }
    if (lane == 0) {
        ws.counts[ray] = count;
        ws.tmin[ray] = t_min;
        ws.tmax[ray] = t_max;
        ws.nsteps[ray] = n;
    }
}

__global__ __launch_bounds__(256) void occ_march_write_kernel(int64_t n_rays, float dt, int words, OccWorkspace ws,
                                                              const int64_t* __restrict__ cum, int64_t n_samples,
                                                              int64_t* __restrict__ ray_indices,
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
    for (int j = 0; j * NERF_WAVE < n; ++j) {
        const unsigned long long m = mrow[j];
        const int k = j * NERF_WAVE + lane;
        const int64_t slot = base + __popcll(m & below);
        if (((m >> lane) & 1ull) && slot >= 0 && slot < n_samples) {
            const float e1 = t_min + (float)(k + 1) * dt;
            ray_indices[slot] = ray;
            t_starts[slot] = t_min + (float)k * dt;
            t_ends[slot] = e1 < t_max ? e1 : t_max;
        }
        base += __popcll(m);
    }
}

}  // namespace

extern "C" size_t nerf_occ_march_workspace(int64_t n_rays, int32_t mask_words) {
    if (n_rays < 0 || !occ_valid_words(mask_words)) return 0;
    return occ_workspace_bytes(n_rays, mask_words);
}

extern "C" int nerf_occ_march_count(const float* rays_o, const float* rays_d, int64_t n_rays, const float* aabb,
                                    const int32_t* resolution, const uint32_t* grid_bits, float near_plane,
                                    float far_plane, float step_size, int32_t stratified, uint64_t seed,
                                    uint64_t counter, int32_t mask_words, void* workspace, size_t workspace_bytes,
                                    int32_t* status, void* stream) {
    NERF_REQUIRE(n_rays >= 0 && occ_valid_words(mask_words) && aabb && resolution);
    NERF_REQUIRE(step_size > 0.0f && step_size < INFINITY);
    OccGrid g;
    int64_t cells = 1;
    for (int a = 0; a < 3; ++a) {
        g.lo[a] = aabb[a]; g.hi[a] = aabb[3 + a]; g.res[a] = resolution[a];
        NERF_REQUIRE(g.lo[a] < g.hi[a] && g.hi[a] - g.lo[a] < INFINITY);
        NERF_REQUIRE(g.res[a] >= 1 && g.res[a] <= 4096);
        cells *= g.res[a];
    }
    NERF_REQUIRE(cells <= (1ll << 31));
    if (n_rays == 0) return NERF_OK;
    NERF_REQUIRE(rays_o && rays_d && grid_bits && workspace && status);
    NERF_REQUIRE(occ_aligned(rays_o, 4) && occ_aligned(rays_d, 4) && occ_aligned(grid_bits, 4) &&
                 occ_aligned(status, 4));
    NERF_REQUIRE((n_rays + 3) / 4 < (1ll << 31));
    if (workspace_bytes < nerf_occ_march_workspace(n_rays, mask_words)) return NERF_ERR_WORKSPACE;
    NERF_REQUIRE(occ_aligned(workspace, 256));
    dim3 grid((unsigned)((n_rays + 3) / 4)), block(256);
    hipLaunchKernelGGL(occ_march_count_kernel, grid, block, 0, as_stream(stream), rays_o, rays_d, n_rays, g, grid_bits,
                       near_plane, far_plane, step_size, stratified, seed, counter, mask_words,
                       occ_carve(workspace, n_rays), status);
    NERF_CHECK_LAUNCH();
    return NERF_OK;
}

extern "C" int nerf_occ_march_write(int64_t n_rays, float step_size, int32_t mask_words, const void* workspace,
                                    size_t workspace_bytes, const int64_t* offsets_incl, int64_t n_samples,
                                    int64_t* ray_indices, float* t_starts, float* t_ends, void* stream) {
    NERF_REQUIRE(n_rays >= 0 && n_samples >= 0 && occ_valid_words(mask_words));
    NERF_REQUIRE(step_size > 0.0f && step_size < INFINITY);
    if (n_rays == 0 || n_samples == 0) return NERF_OK;
    NERF_REQUIRE(workspace && offsets_incl && ray_indices && t_starts && t_ends);
    NERF_REQUIRE(occ_aligned(offsets_incl, 8) && occ_aligned(ray_indices, 8) && occ_aligned(t_starts, 4) &&
                 occ_aligned(t_ends, 4));
    NERF_REQUIRE((n_rays + 3) / 4 < (1ll << 31));
    if (workspace_bytes < nerf_occ_march_workspace(n_rays, mask_words)) return NERF_ERR_WORKSPACE;
    NERF_REQUIRE(occ_aligned(workspace, 256));
    dim3 grid((unsigned)((n_rays + 3) / 4)), block(256);
    hipLaunchKernelGGL(occ_march_write_kernel, grid, block, 0, as_stream(stream), n_rays, step_size, mask_words,
                       occ_carve(const_cast<void*>(workspace), n_rays), offsets_incl, n_samples, ray_indices,
                       t_starts, t_ends);
    NERF_CHECK_LAUNCH();
    return NERF_OK;
}
