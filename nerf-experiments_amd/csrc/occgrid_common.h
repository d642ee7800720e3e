// The marching workspace shared by the one-level kernels (occgrid.hip) and the cascaded ones
// (occgrid_cascade.hip): one layout, one size function (nerf_occ_march_workspace).
#pragma once
#include "common.h"

namespace nerf {

constexpr int kOccMaxWords = NERF_OCC_MAX_STEPS / NERF_WAVE;

// workspace: [counts int64 x n][t_min f32 x n][t_max f32 x n][n_steps i32 x n] pad to 256 [masks u64 x n x words]
struct OccWorkspace {
    int64_t* counts; float* tmin; float* tmax; int32_t* nsteps; unsigned long long* masks;
};

inline size_t occ_header_bytes(int64_t n_rays) { return ((size_t)n_rays * 20 + 255) & ~(size_t)255; }

inline size_t occ_workspace_bytes(int64_t n_rays, int32_t words) {
    return occ_header_bytes(n_rays) + (size_t)n_rays * words * sizeof(unsigned long long);
}

inline OccWorkspace occ_carve(void* ws, int64_t n_rays) {
    char* p = static_cast<char*>(ws);
    OccWorkspace w;
    w.counts = reinterpret_cast<int64_t*>(p);
    w.tmin = reinterpret_cast<float*>(p + (size_t)n_rays * 8);
    w.tmax = w.tmin + n_rays;
    w.nsteps = reinterpret_cast<int32_t*>(w.tmax + n_rays);
    w.masks = reinterpret_cast<unsigned long long*>(p + occ_header_bytes(n_rays));
    return w;
}

inline bool occ_aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

inline bool occ_valid_words(int32_t words) { return words >= 1 && words <= kOccMaxWords; }

}  // namespace nerf
