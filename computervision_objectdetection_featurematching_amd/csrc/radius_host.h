// radius_host.h — the host-callable parts of radius matching (BFMatcher(norm).radiusMatch): the
// argument check, the integer thresholds the kernels compare against, the 64-bit sort key and the merge
// step of the per-query sort.  HIP-free: radius.hip runs radius_merge_place on the device, api.cpp computes the
// thresholds once per call, and a plain C++17 compiler builds tests/cpp/radius_driver.cpp over the same text.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define MIM_RAD_HD __host__ __device__ __forceinline__
#else
#define MIM_RAD_HD inline
#endif

namespace mim {

constexpr int kRadMaxD2 = 128 * 255 * 255;  // 8,323,200: the largest squared distance of two integer 128-D rows
constexpr int kRadHamMax = 8 * 64;          // the largest Hamming distance of two rows of 64 bytes
constexpr int kRadSortCap = 2048;           // keys of one in-LDS sort (16 KiB); a longer list is sorted in runs

// DescriptorMatcher::radiusMatch: CV_Assert(maxDistance > FLT_EPSILON); a NaN fails the compare
inline bool radius_arg_ok(float r) { return r > FLT_EPSILON; }

// Binary rows: the distance is an integer n in [0, 512] carried as a float, and (float)n <= r is
// n <= floor(r) for r >= 0 (n and floor(r) are both exact floats).  -1: nothing passes (r < 0 or a NaN).
inline int radius_ham_threshold(float r) {
    if (!(r >= 0.f)) return -1;
    return r >= (float)kRadHamMax ? kRadHamMax : (int)floorf(r);
}

// Integer 128-D rows: the largest n in [0, kRadMaxD2] with sqrtf((float)n) <= r, -1 if there is none.
// n < 2^24 converts exactly, sqrtf is correctly rounded and so monotone: the n that pass are a prefix
// 0..T2 of the range, and the literal test sqrtf((float)d2) <= r is d2 <= T2.  The search starts at
// fl(r * r), which is within one rounding of r^2, and walks with the literal compare: a step crosses at
// most the few integers between r^2's float neighbours plus one sqrtf class (two integers above 4e6).
inline int radius_int_threshold(float r) {
    if (!(r >= 0.f)) return -1;  // NaN, negative
    if (sqrtf((float)kRadMaxD2) <= r) return kRadMaxD2;
    const float p = r * r;  // r < 2885: no overflow
    int n = p >= (float)kRadMaxD2 ? kRadMaxD2 : (int)p;
    while (n < kRadMaxD2 && sqrtf((float)(n + 1)) <= r) ++n;
    while (n >= 0 && !(sqrtf((float)n) <= r)) --n;
    return n;
}

// Float rows: the largest float T with sqrtf(T) <= r, so that the literal test sqrtf(d2) <= r on a squared
// distance d2 (never negative) is d2 <= T, bit for bit: sqrtf is correctly rounded, hence monotone over the
// non-negative floats, +inf included (sqrtf(+inf) = +inf passes only r = +inf, and then T = +inf), and a NaN d2
// fails both forms.  The walk starts at fl(r * r) and moves by single floats with the literal compare; r^2's
// rounding and the width of one sqrtf class are a few floats at most.  A negative value: nothing passes
// (r < 0 or a NaN).
inline float radius_flt_threshold(float r) {
    if (!(r >= 0.f)) return -1.f;
    const float inf = INFINITY;
    if (r == inf) return inf;
    float t = r * r;
    if (!(t < inf)) t = FLT_MAX;  // r * r overflowed; sqrtf(FLT_MAX) ~ 1.8e19 <= r
    while (t < FLT_MAX && sqrtf(nextafterf(t, inf)) <= r) t = nextafterf(t, inf);
    while (t > 0.f && !(sqrtf(t) <= r)) t = nextafterf(t, 0.f);
    return t;  // t = 0 passes every r >= 0
}

// Sort key of one match: the distance's bits above the train row.  A distance here is never negative and
// never a NaN, so its bits order as its value (+inf last), and unsigned key order is (distance, row) order.
// The keys of one query are distinct (its rows are).
MIM_RAD_HD uint64_t radius_key(float d, int row) {
    uint32_t b;
    memcpy(&b, &d, 4);
    return (uint64_t)b << 32 | (uint32_t)row;
}
MIM_RAD_HD float radius_key_dist(uint64_t key) {
    const uint32_t b = (uint32_t)(key >> 32);
    float d;
    memcpy(&d, &b, 4);
    return d;
}
MIM_RAD_HD int32_t radius_key_row(uint64_t key) { return (int32_t)(uint32_t)key; }

// Merge step: `own` and `other` are ascending runs whose keys are all distinct.  The place of own[i] in the
// ascending union of the two is i plus the number of keys of `other` below it (a binary search).  Calling it
// for every element of both runs fills every place of the union once.
MIM_RAD_HD int64_t radius_merge_place(const uint64_t* own, int64_t i, const uint64_t* other, int64_t n_other) {
    const uint64_t key = own[i];
    int64_t lo = 0, hi = n_other;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (other[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return i + lo;
}

// One merge pass over a list of n keys made of sorted runs of `width` (the last may be shorter): where
// src[i] goes in dst, runs merged in pairs (an unpaired last run keeps its place).
MIM_RAD_HD int64_t radius_pass_place(const uint64_t* src, int64_t n, int64_t width, int64_t i) {
    const int64_t base = i / (2 * width) * (2 * width);
    const int64_t a1 = base + width < n ? base + width : n, b1 = base + 2 * width < n ? base + 2 * width : n;
    if (i < a1) return base + radius_merge_place(src + base, i - base, src + a1, b1 - a1);
    return base + radius_merge_place(src + a1, i - a1, src + base, a1 - base);
}

}  // namespace mim
