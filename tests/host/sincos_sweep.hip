// Host sweep of nerf::sincos_enc (csrc/common.h, __host__ __device__): the function's own source,
// compiled for the CPU, against fp64 sin / cos.  The fast path is rintf, fmaf and fp32 multiplies
// only, so the device computes the same bits.  Built and run by tests/test_sincos_host.py; no GPU
// is touched.
//
//   exhaustive: every fp32 bit pattern of [2^12, T), T = nerf::kSincosFastMax
//   strided:    every 61st bit pattern of (0, 2^12), subnormals included
//   for each x: |s - sin(x)|, |c - cos(x)| in fp64; sincos_enc(-x) must be (-s, c) bit for bit
//   edges:      the eight fp32 values on either side of T, 2^30's neighbours, FLT_MAX, +-inf, NaN:
//               which path each took, by comparing with a direct sincosf call
//   wide:       nerf::sincos_arg (csrc/param_act.h), the Gabor / Sarf argument hi + lo: seeded exact
//               products p z with |p z| from 2^-4 to 2^40 (the first-order path below 4096, the fp64
//               wrap into [-pi, pi] above) and fp64 arguments of the same range, against fp64 sin /
//               cos of the exact argument; past 2^40 the result must be sincosf of the fp32 argument
//
// Output: "key value..." lines, parsed by the test.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <thread>
#include <vector>

#include "common.h"
#include "param_act.h"

static inline float from_bits(uint32_t b) {
    float f;
    memcpy(&f, &b, 4);
    return f;
}
static inline uint32_t to_bits(float f) {
    uint32_t b;
    memcpy(&b, &f, 4);
    return b;
}

struct Worst {
    double sin_err = 0.0, cos_err = 0.0;
    uint32_t sin_at = 0, cos_at = 0;
    uint64_t n = 0, asym = 0, unbounded = 0;
    uint32_t asym_at = 0;
    void merge(const Worst& o) {
        if (o.sin_err > sin_err) { sin_err = o.sin_err; sin_at = o.sin_at; }
        if (o.cos_err > cos_err) { cos_err = o.cos_err; cos_at = o.cos_at; }
        if (o.asym && !asym) asym_at = o.asym_at;
        n += o.n; asym += o.asym; unbounded += o.unbounded;
    }
};

// bit patterns lo, lo + step, ... below hi
static void sweep(uint32_t lo, uint32_t hi, uint32_t step, Worst* w) {
    for (uint64_t b = lo; b < hi; b += step) {
        const float x = from_bits((uint32_t)b);
        float s, c, sm, cm;
        nerf::sincos_enc(x, &s, &c);
        nerf::sincos_enc(-x, &sm, &cm);
        const double es = fabs((double)s - sin((double)x)), ec = fabs((double)c - cos((double)x));
        // NaN-safe: a NaN error counts as the worst
        if (!(es <= w->sin_err)) { w->sin_err = es == es ? es : INFINITY; w->sin_at = (uint32_t)b; }
        if (!(ec <= w->cos_err)) { w->cos_err = ec == ec ? ec : INFINITY; w->cos_at = (uint32_t)b; }
        if (to_bits(sm) != to_bits(-s) || to_bits(cm) != to_bits(c)) {
            if (!w->asym) w->asym_at = (uint32_t)b;
            ++w->asym;
        }
        if (!(fabsf(s) <= 1.0f) || !(fabsf(c) <= 1.0f)) ++w->unbounded;
        ++w->n;
    }
}

static Worst sweep_threads(uint32_t lo, uint32_t hi, uint32_t step, unsigned nt) {
    // contiguous chunks whose starts stay on the stride
    const uint64_t count = ((uint64_t)hi - lo + step - 1) / step, per = (count + nt - 1) / nt;
    std::vector<Worst> ws(nt);
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; ++t) {
        const uint64_t a = lo + (uint64_t)t * per * step, b = std::min<uint64_t>(hi, a + per * step);
        if (a >= hi) break;
        th.emplace_back(sweep, (uint32_t)a, (uint32_t)b, step, &ws[t]);
    }
    for (auto& t : th) t.join();
    Worst w;
    for (auto& x : ws) w.merge(x);
    return w;
}

static void report(const char* name, const Worst& w) {
    printf("%s n %llu\n", name, (unsigned long long)w.n);
    printf("%s max_sin_err %.6e at 0x%08x %.9g\n", name, w.sin_err, w.sin_at, (double)from_bits(w.sin_at));
    printf("%s max_cos_err %.6e at 0x%08x %.9g\n", name, w.cos_err, w.cos_at, (double)from_bits(w.cos_at));
    printf("%s asymmetric %llu first 0x%08x\n", name, (unsigned long long)w.asym, w.asym_at);
    printf("%s unbounded %llu\n", name, (unsigned long long)w.unbounded);
}

static inline bool same_bits(float a, float b) { return to_bits(a) == to_bits(b) || (a != a && b != b); }

// which path x took: "libm" if both results are sincosf's bits (NaN matching NaN), else "fast"
static void edge(const char* what, float x) {
    float s, c, ls, lc;
    nerf::sincos_enc(x, &s, &c);
    sincosf(x, &ls, &lc);
    const bool same = same_bits(s, ls) && same_bits(c, lc);
    printf("edge %s 0x%08x %.9g %s sin %.9g cos %.9g\n", what, to_bits(x), (double)x, same ? "libm" : "fast",
           (double)s, (double)c);
}

// sincos_arg over seeded arguments with |a| in [2^e, 2^(e + 2)), e = -4 .. 38: the product form
// (hi = fl(p z), lo = p z - hi by one FMA) and the fp64 form
static uint64_t lcg(uint64_t* st) {
    *st = *st * 6364136223846793005ull + 1442695040888963407ull;
    return *st >> 33;
}

static void wide() {
    double worst[2][2] = {{0, 0}, {0, 0}}, at[2][2] = {{0, 0}, {0, 0}};     // [narrow, wide][product, fp64]
    uint64_t st = 20240607, n = 0, unbounded = 0;
    for (int e = -4; e <= 38; ++e) {
        for (int i = 0; i < (1 << 15); ++i) {
            const float p = ldexpf(1.0f + (float)(lcg(&st) & 0x7fffff) / 8388608.0f, e) * ((lcg(&st) & 1) ? -1.f : 1.f);
            const float z = 1.0f + (float)(lcg(&st) & 0x7fffff) / 8388608.0f;
            const float hi = p * z, lo = __builtin_fmaf(p, z, -hi);
            const double a = (double)p * (double)z, b = a / 3.0 + 0.1;
            float s, c;
            nerf::sincos_arg(hi, lo, &s, &c);
            const int w = fabsf(hi) < nerf::kSincosArgMax ? 0 : 1;
            double err = fmax(fabs((double)s - sin(a)), fabs((double)c - cos(a)));
            if (!(err <= worst[w][0])) { worst[w][0] = err == err ? err : INFINITY; at[w][0] = a; }
            if (!(fabsf(s) <= 1.0f) || !(fabsf(c) <= 1.0f)) ++unbounded;
            nerf::sincos_arg(b, &s, &c);
            const int wb = fabs(b) < (double)nerf::kSincosArgMax ? 0 : 1;
            err = fmax(fabs((double)s - sin(b)), fabs((double)c - cos(b)));
            if (!(err <= worst[wb][1])) { worst[wb][1] = err == err ? err : INFINITY; at[wb][1] = b; }
            if (!(fabsf(s) <= 1.0f) || !(fabsf(c) <= 1.0f)) ++unbounded;
            ++n;
        }
    }
    printf("arg n %llu\n", (unsigned long long)n);
    printf("arg first_order_product %.6e at %.17g\n", worst[0][0], at[0][0]);
    printf("arg first_order_fp64 %.6e at %.17g\n", worst[0][1], at[0][1]);
    printf("arg wrapped_product %.6e at %.17g\n", worst[1][0], at[1][0]);
    printf("arg wrapped_fp64 %.6e at %.17g\n", worst[1][1], at[1][1]);
    printf("arg unbounded %llu\n", (unsigned long long)unbounded);
    // past 2^40 and non-finite: sincosf of the fp32 argument, lo dropped
    const float far_[] = {1099511627776.0f, -3.0e12f, 1.0e20f, 3.402823466e+38f, INFINITY, -INFINITY, NAN};
    int bad = 0;
    for (float h : far_) {
        float s, c, ls, lc, s2, c2;
        sincosf(h, &ls, &lc);
        nerf::sincos_arg(h, h * 1e-8f, &s, &c);
        nerf::sincos_arg((double)h, &s2, &c2);
        const bool ok = same_bits(s, ls) && same_bits(c, lc) && same_bits(s2, ls) && same_bits(c2, lc);
        bad += ok ? 0 : 1;
    }
    printf("arg far_not_libm %d\n", bad);
}

int main() {
    const float T = nerf::kSincosFastMax;
    const uint32_t tb = to_bits(T), b12 = to_bits(4096.0f);
    unsigned nt = std::thread::hardware_concurrency();
    nt = nt == 0 ? 1 : std::min(nt, 8u);
#ifdef NERF_SINCOS_FP64_REDUCTION
    printf("reduction fp64\n");
#else
    printf("reduction fp32\n");
#endif
    printf("T %.9g 0x%08x\n", (double)T, tb);
    printf("threads %u\n", nt);
    if (!(T > 4096.0f) || !(T < INFINITY)) {
        printf("bad_T\n");
        return 2;
    }
    report("exhaustive", sweep_threads(b12, tb, 1, nt));
    report("strided", sweep_threads(1, b12, 61, nt));
    for (int i = 8; i >= 1; --i) edge("below_T", from_bits(tb - i));
    for (int i = 0; i < 8; ++i) edge("above_T", from_bits(tb + i));
    for (int i = 0; i < 8; ++i) edge("above_T", -from_bits(tb + i));
    const uint32_t b30 = to_bits(1073741824.0f);
    for (int i = -2; i <= 2; ++i) edge("above_T", from_bits(b30 + i));
    edge("above_T", 3.402823466e+38f);
    edge("above_T", -3.402823466e+38f);
    edge("nonfinite", INFINITY);
    edge("nonfinite", -INFINITY);
    edge("nonfinite", NAN);
    wide();
    return 0;
}
