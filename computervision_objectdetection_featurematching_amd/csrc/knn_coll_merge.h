// knn_coll_merge.h — the merge of one query row's partial lists over the images of a train collection
// (mim_knn_collection_dev).  HIP-free: knn_coll.hip runs coll_merge_query on the device, one
// thread per query row, and a plain C++17 compiler builds tests/cpp/knn_coll_driver.cpp over the same function.
#pragma once
#include "knn_topk_merge.h"  // TopkEnt, topk_chain

namespace mim {

constexpr int kCollImgShift = 18;     // BFMatcher's IMGIDX_SHIFT: a train image has fewer than 2^18 rows
constexpr int kCollMaxImages = 8191;  // imgCount << 18 stays below INT_MAX
constexpr uint64_t kCollNone = ~(uint64_t)0;

// The partial lists of one (query set, image) pair.  A 128-D pair has two blocks of lists, one per kernel that
// may own it; the sets' flags words say which one was written.
struct CollPart {
    const TopkEnt* a;    // i8 kernel's lists [na][qa_pad][KT] (two per train split: the lane halves; KT = topk_kt(k)
                         // slots per list, the last k in use, (-1, -1) in front); null: not a 128-D pair
    const TopkEnt* b;    // Hamming / float kernel's lists [nb][qb_pad][k]
    const int* qflags;   // the 128-D sets' integrality flags (SetDev::flags); null with a
    const int* tflags;
    int na, qa_pad;
    int nb, qb_pad;
    int img;             // the image's place in the collection
    int pad_;
};

// (distance, imgIdx, trainIdx) order as one unsigned compare: the bits of a float in [0, FLT_MAX) fit 31,
// img 13 and row 18
MIM_TOPK_HD uint64_t coll_key(float d, int img, int row) {
    uint32_t b;
    memcpy(&b, &d, 4);
    return (uint64_t)b << 31 | (uint64_t)(uint32_t)img << kCollImgShift | (uint32_t)row;
}

// Query row q's k nearest over the images of `parts` (n_parts records in image order), in (distance, imgIdx,
// trainIdx) order.  seed: the rows idx / img / dist hold the lists an earlier group of images left, which take
// part as entries like any other (their images precede this group's, and so do their keys among equal
// distances); else the lists start empty.  The (image, row) pairs are distinct, so the keys are, and the k
// smallest do not depend on how the rows were cut into images' splits, lane halves or groups.  A partial
// list is ascending and ends at its first sentinel (FLT_MAX, INT_MAX); it is left at its first entry that is
// not below the current KT-th key.  Absent entries are written as -1, -1, FLT_MAX.  KT = topk_kt(k).
template <int KT>
MIM_TOPK_HD void coll_merge_query(const CollPart* parts, int n_parts, int k, int q, bool seed, int32_t* idx, int32_t* img,
                                  float* dist) {
    uint64_t L[KT];
MIM_TOPK_UNROLL
    for (int s = 0; s < KT; ++s) L[s] = kCollNone;
    if (seed) {
        for (int s = 0; s < k; ++s) {
            if (idx[s] < 0) break;
            topk_chain<KT>(L, coll_key(dist[s], img[s], idx[s]));
        }
    }
    for (int p = 0; p < n_parts; ++p) {
        const CollPart& P = parts[p];
        const bool i8 = P.a && !(*P.qflags | *P.tflags);
        const TopkEnt* lists = i8 ? P.a : P.b;
        const int n = i8 ? P.na : P.nb;
        const long long q_pad = i8 ? P.qa_pad : P.qb_pad;
        const int stride = i8 ? KT : k, skip = stride - k;
        for (int l = 0; l < n; ++l) {
            const TopkEnt* e = lists + ((long long)l * q_pad + q) * stride + skip;
            for (int s = 0; s < k; ++s) {
                if (e[s].i == INT_MAX) break;
                const uint64_t x = coll_key(e[s].d, P.img, e[s].i);
                if (!(x < L[KT - 1])) break;
                topk_chain<KT>(L, x);
            }
        }
    }
MIM_TOPK_UNROLL
    for (int s = 0; s < KT; ++s)
        if (s < k) {
            const bool ok = L[s] != kCollNone;
            const uint32_t b = ok ? (uint32_t)(L[s] >> 31) : 0x7F7FFFFFu;
            float d;
            memcpy(&d, &b, 4);
            idx[s] = ok ? (int32_t)(L[s] & 0x3FFFFu) : -1;
            img[s] = ok ? (int32_t)((L[s] >> kCollImgShift) & 0x1FFFu) : -1;
            dist[s] = d;
        }
}

}  // namespace mim
