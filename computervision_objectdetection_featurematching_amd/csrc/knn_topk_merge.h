// knn_topk_merge.h — the top-k partial entry and the merge of a query's per-split lists.
// HIP-free: knn_topk.hip runs topk_merge_query on the device, one thread per query, and a plain C++17
// compiler builds tests/cpp/knn_topk_driver.cpp over the same function.
#pragma once
#include <cfloat>
#include <climits>
#include <cstdint>
#include <cstring>
#include <type_traits>

#if defined(__HIPCC__)
#define MIM_TOPK_HD __host__ __device__ __forceinline__
#else
#define MIM_TOPK_HD inline
#endif
#if defined(__clang__)
#define MIM_TOPK_UNROLL _Pragma("unroll")
#else
#define MIM_TOPK_UNROLL
#endif

namespace mim {

// One entry of a top-k partial list: a split's lists are [q_pad][k], ascending in (d, i); an entry past the
// list's end is (FLT_MAX, INT_MAX).  d is the DMatch::distance of the kind, below FLT_MAX, never a NaN.
struct TopkEnt {
    float d;
    int i;
};

// (d, i) order as one unsigned compare: a non-negative float's bits order as its value
MIM_TOPK_HD uint64_t topk_key(TopkEnt e) {
    uint32_t b;
    memcpy(&b, &e.d, 4);
    return (uint64_t)b << 32 | (uint32_t)e.i;
}

constexpr uint64_t kTopkNone = (uint64_t)0x7F7FFFFFu << 32 | (uint32_t)INT_MAX;  // (FLT_MAX, INT_MAX)

// x into the ascending list L where it is below L[KT - 1]; for any other x nothing changes.  Static
// indices only: with KT a template argument the list stays in registers.
template <int KT, class T>
MIM_TOPK_HD void topk_chain(T (&L)[KT], T x) {
MIM_TOPK_UNROLL
    for (int s = KT - 1; s > 0; --s) {
        const T lo = L[s - 1] > x ? L[s - 1] : x;  // max(L[s - 1], x)
        L[s] = L[s] < lo ? L[s] : lo;              // min(L[s], that): the median, L[s - 1] <= L[s]
    }
    L[0] = L[0] < x ? L[0] : x;
}

// Query q's k nearest over the nsplit lists of one problem (parts: its [split][q_pad][k] block), in
// (distance, index) order: rows of distinct splits are distinct, so the keys are, and the k smallest of
// their union do not depend on how the train rows were cut.  A split's list is ascending, so it is left
// at its first entry that is not below the current KT-th key.  Entries past the last finite one are
// written as index -1 and distance FLT_MAX.  KT >= k.
template <int KT>
MIM_TOPK_HD void topk_merge_query(const TopkEnt* parts, int nsplit, int q_pad, int k, int q, int32_t* idx, float* dist) {
    uint64_t L[KT];
MIM_TOPK_UNROLL
    for (int s = 0; s < KT; ++s) L[s] = kTopkNone;
    for (int sp = 0; sp < nsplit; ++sp) {
        const TopkEnt* e = parts + ((long long)sp * q_pad + q) * k;
        for (int s = 0; s < k; ++s) {
            const uint64_t x = topk_key(e[s]);
            if (!(x < L[KT - 1])) break;
            topk_chain<KT>(L, x);
        }
    }
MIM_TOPK_UNROLL
    for (int s = 0; s < KT; ++s)
        if (s < k) {
            const bool ok = L[s] < kTopkNone && (uint32_t)(L[s] >> 32) < 0x7F7FFFFFu;
            const uint32_t b = ok ? (uint32_t)(L[s] >> 32) : 0x7F7FFFFFu;
            float d;
            memcpy(&d, &b, 4);
            idx[s] = ok ? (int32_t)(uint32_t)L[s] : -1;
            dist[s] = d;
        }
}

// the list length a k runs at: k rounded up to 4, 8 or 16
inline int topk_kt(int k) { return k <= 4 ? 4 : k <= 8 ? 8 : 16; }

// f(std::integral_constant<int, topk_kt(k)>{}): the launchers' choice of a kernel's KT
template <class F>
inline void topk_dispatch(int k, F&& f) {
    if (k <= 4) f(std::integral_constant<int, 4>{});
    else if (k <= 8) f(std::integral_constant<int, 8>{});
    else f(std::integral_constant<int, 16>{});
}

}  // namespace mim
