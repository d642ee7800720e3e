// Distortion loss of mip-NeRF 360 (nerfacc.distortion restated) on packed samples, forward and
// backward: rays own segments [seg[r], seg[r+1]) of the flat weights / t_starts / t_ends.
//
// With m_i = (t_starts_i + t_ends_i) / 2 and delta_i = t_ends_i - t_starts_i formed in fp64, and
// W_<i, WM_<i the exclusive fp64 prefix sums of w and w * m in sample order:
//   loss_r   = fp32( sum_i [ w_i^2 delta_i / 3 + 2 w_i (m_i W_<i - WM_<i) ] )
//   grad_w_i = fp32( g_r [ 2/3 w_i delta_i + 2 (m_i W_<i - WM_<i + WM_>i - m_i W_>i) ] )
// which is sum_ij w_i w_j |m_i - m_j| + 1/3 sum w_i^2 delta_i when the midpoints ascend along the ray
// (the contract; marched samples and proposal intervals satisfy it).  The fp32 form of the bracket
// cancels (m W and WM agree to the leading digits), hence fp64.
// One 64-lane wavefront per ray walks its segment in 64-sample chunks: two fp64 DPP wave scans per
// chunk plus the running totals of the earlier chunks, as composite_packed.hip does.  The backward
// first walks the segment for the ray totals (the same scans, so W_>i = W - W_<=i is a difference of
// sums formed alike), then again for the gradient.  No LDS, no atomics; an empty ray gets loss 0.
// Segment bounds are clamped to [0, n_samples].
#include "common.h"

using namespace nerf;

namespace {

struct DistArgs {
    const float* w; const float* t0; const float* t1;
    const int64_t* seg;
    int64_t n_rays, n_samples;
};

__device__ __forceinline__ void segment(const DistArgs& a, int64_t ray, int64_t& s0, int64_t& s1) {
    s0 = a.seg[ray];
    s1 = a.seg[ray + 1];
    s0 = s0 < 0 ? 0 : (s0 > a.n_samples ? a.n_samples : s0);
    s1 = s1 < s0 ? s0 : (s1 > a.n_samples ? a.n_samples : s1);
}

// one chunk's sample of this lane: w, m, delta in fp64 (zeros past the segment)
__device__ __forceinline__ void load_sample(const DistArgs& a, int64_t i, bool ok, double& w, double& m, double& del) {
    w = 0.0; m = 0.0; del = 0.0;
    if (ok) {
        const double ts = (double)a.t0[i], te = (double)a.t1[i];
        w = (double)a.w[i];
        m = (ts + te) * 0.5;
        del = te - ts;
    }
}

__global__ __launch_bounds__(256) void distortion_fwd_kernel(DistArgs a, float* __restrict__ loss) {
#pragma clang fp contract(off)
    const int lane = lane_id();
    const int64_t ray = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ray >= a.n_rays) return;        // wave-uniform
    int64_t s0, s1;
    segment(a, ray, s0, s1);
    double cw = 0.0, cwm = 0.0;         // sums of w and w * m over the ray's earlier chunks
    double acc = 0.0;
    for (int64_t cb = s0; cb < s1; cb += NERF_WAVE) {
        const int64_t i = cb + lane;
        double w, m, del;
        load_sample(a, i, i < s1, w, m, del);
        const double wm = w * m;
        const double iw = wave_inclusive_scan_dpp(w);
        const double iwm = wave_inclusive_scan_dpp(wm);
        const double ew = cw + (iw - w), ewm = cwm + (iwm - wm);    // exclusive prefixes
        cw += wave_last_d(iw);
        cwm += wave_last_d(iwm);
        acc += w * w * del / 3.0 + 2.0 * w * (m * ew - ewm);
    }
    const double tot = wave_sum(acc);
    if (lane == 0) loss[ray] = (float)tot;
}

__global__ __launch_bounds__(256) void distortion_bwd_kernel(DistArgs a, const float* __restrict__ g_loss,
                                                             float* __restrict__ grad_w) {
#pragma clang fp contract(off)
    const int lane = lane_id();
    const int64_t ray = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ray >= a.n_rays) return;
    int64_t s0, s1;
    segment(a, ray, s0, s1);
    if (s0 >= s1) return;
    const double g = (double)g_loss[ray];
    double tw = 0.0, twm = 0.0;         // the ray totals, summed as the prefixes below are
    for (int64_t cb = s0; cb < s1; cb += NERF_WAVE) {
        const int64_t i = cb + lane;
        double w, m, del;
        load_sample(a, i, i < s1, w, m, del);
        tw += wave_last_d(wave_inclusive_scan_dpp(w));
        twm += wave_last_d(wave_inclusive_scan_dpp(w * m));
    }
    double cw = 0.0, cwm = 0.0;
    for (int64_t cb = s0; cb < s1; cb += NERF_WAVE) {
        const int64_t i = cb + lane;
        const bool ok = i < s1;
        double w, m, del;
        load_sample(a, i, ok, w, m, del);
        const double wm = w * m;
        const double iw = wave_inclusive_scan_dpp(w);
        const double iwm = wave_inclusive_scan_dpp(wm);
        const double ew = cw + (iw - w), ewm = cwm + (iwm - wm);    // sums over the earlier samples
        const double lw = tw - (cw + iw), lwm = twm - (cwm + iwm);  // sums over the later samples
        cw += wave_last_d(iw);
        cwm += wave_last_d(iwm);
        if (ok) grad_w[i] = (float)(g * (2.0 / 3.0 * w * del + 2.0 * (m * ew - ewm + lwm - m * lw)));
    }
}

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

extern "C" int nerf_distortion_fwd(const float* weights, const float* t_starts, const float* t_ends,
                                   const int64_t* seg, int64_t n_rays, int64_t n_samples, float* loss, void* stream) {
    NERF_REQUIRE(n_rays >= 0 && n_samples >= 0);
    if (n_rays == 0 || n_samples == 0) return NERF_OK;
    NERF_REQUIRE(weights && t_starts && t_ends && seg && loss);
    NERF_REQUIRE(aligned(seg, 8));
    NERF_REQUIRE(aligned(weights, 4) && aligned(t_starts, 4) && aligned(t_ends, 4) && aligned(loss, 4));
    NERF_REQUIRE((n_rays + 3) / 4 < (1ll << 31));
    DistArgs a{weights, t_starts, t_ends, seg, n_rays, n_samples};
    dim3 grid((unsigned)((n_rays + 3) / 4)), block(256);
    hipLaunchKernelGGL(distortion_fwd_kernel, grid, block, 0, as_stream(stream), a, loss);
    NERF_CHECK_LAUNCH();
    return NERF_OK;
}

extern "C" int nerf_distortion_bwd(const float* weights, const float* t_starts, const float* t_ends,
                                   const int64_t* seg, int64_t n_rays, int64_t n_samples, const float* g_loss,
                                   float* grad_weights, void* stream) {
    NERF_REQUIRE(n_rays >= 0 && n_samples >= 0);
    if (n_rays == 0 || n_samples == 0) return NERF_OK;
    NERF_REQUIRE(weights && t_starts && t_ends && seg && g_loss && grad_weights);
    NERF_REQUIRE(aligned(seg, 8));
    NERF_REQUIRE(aligned(weights, 4) && aligned(t_starts, 4) && aligned(t_ends, 4) && aligned(g_loss, 4) &&
                 aligned(grad_weights, 4));
    NERF_REQUIRE((n_rays + 3) / 4 < (1ll << 31));
    DistArgs a{weights, t_starts, t_ends, seg, n_rays, n_samples};
    dim3 grid((unsigned)((n_rays + 3) / 4)), block(256);
    hipLaunchKernelGGL(distortion_bwd_kernel, grid, block, 0, as_stream(stream), a, g_loss, grad_weights);
    NERF_CHECK_LAUNCH();
    return NERF_OK;
}
