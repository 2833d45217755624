// knn_coll.hip — knnMatch over a train collection (BFMatcher::add + knnMatch(query, k)): the i8
// MFMA top-k kernel for 128-D sets that are integer-valued on both sides, and the kernel that merges every
// image's partial lists into one list per query row with the image in imgIdx.  Binary sets, generic float
// sets and flagged 128-D sets go through the top-k kernels of knn_topk.hip.
//
// knn_topk_i8_kernel is the frame of sweep_i8.h (R = q'.t'' + floor(n2/2), D = 2R + (n2 & 1), d^2 = D + c(q),
// exact) under a rule that keeps, per lane and column tile, an ascending list of (sqrtf(d^2), row) in VGPRs
// (unrolled indices only).  A lane meets its rows in ascending order (accumulator g of lane half h is row
// (g & 3) + 8 (g >> 2) + 4 h of the half tile), so inserting behind a strict < on the float is OpenCV's tie
// rule inside a lane's list.  The two lane halves hold disjoint rows of one query: they are written as two
// lists, and the merge joins them.
//
// The integer filter.  With kK the list's k-th distance (FLT_MAX while it is not full) a pair is inserted iff
// sqrtf((float)d^2) < kK.  thr = nextafterf(fl(kK * kK), +inf) has d^2 > thr => sqrtf(d^2) >= kK (the claim
// proved in knn_topk.hip's header; d^2 < 2^23 is an integer, so (float)d^2 is exact), and for the integer
// d^2 that is d^2 > T = floor(thr).  So only pairs with 2R + p + c(q) <= T can be inserted, and p >= 0 gives
//   R <= lim = floor((T - c(q)) / 2),
// one register per list.  fl(kK * kK) >= 2^23 (above every d^2; the list not full) is lim = INT_MAX: every
// pair is a candidate, the padded train rows (R = 2^30 - 1 + q'.t'') included, so the hit path tests row < nt
// itself.  Candidates are decided by the exact float compare, which then re-derives lim.  A column past the
// query set has lim = INT_MIN.  Only the last k of the KT slots are used: the first KT - k hold (-1, -1),
// below every distance, so the bound is the k-th distance and not the KT-th.
// gfx950, wave64.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>

#include "knn_coll.h"
#include "sweep_i8.h"

namespace mim {

namespace {

// lim of the file header from the list's k-th distance
__device__ __forceinline__ int i8_limit(float kK, int cq) {
    const float p = kK * kK;
    if (!(p < 8388608.f)) return INT_MAX;
    return ((int)__uint_as_float(__float_as_uint(p) + 1u) - cq) >> 1;  // |c(q)| <= 2^22: no overflow
}

template <int KT>
struct TopkI8Rule {
    // an empty split of the schedule (tile0 == tile1) sweeps nothing and writes its sentinel lists
    static constexpr bool kSkipEmpty = false, kFixedLimit = false;
    const CollI8Prob& P;
    const int split, k;
    int lim[kKnnQT];
    float Ld[kKnnQT][KT];
    int Li[kKnnQT][KT];

    __device__ __forceinline__ TopkI8Rule(const CollI8Prob& P_, const KnnWork& w, int k_) : P(P_), split(w.split), k(k_) {}
    __device__ __forceinline__ void init(int u, const I8Col& c) {
        lim[u] = c.valid ? INT_MAX : INT_MIN;
#pragma unroll
        for (int a = 0; a < KT; ++a) {
            Ld[u][a] = FLT_MAX;
            Li[u][a] = INT_MAX;
        }
    }
    // the KT - k unused slots in front: (-1, -1) shifted in one at a time (a loop, not a compare of k per slot)
    __device__ __forceinline__ void begin() {
        for (int j = KT - k; j > 0; --j) {
#pragma unroll
            for (int u = 0; u < kKnnQT; ++u) {
#pragma unroll
                for (int a = KT - 1; a > 0; --a) {
                    Ld[u][a] = Ld[u][a - 1];
                    Li[u][a] = Li[u][a - 1];
                }
                Ld[u][0] = -1.f;
                Li[u][0] = -1;
            }
        }
    }
    __device__ __forceinline__ int limit(int u) const { return lim[u]; }
    __device__ __forceinline__ void row(int u, const I8Col& c, int R, unsigned par, int row, int nt) {
        if (R <= lim[u] && row < nt && c.valid) {  // a padded row's R is under an unbounded lim
            const int D = (int)(((unsigned)R << 1) | par);
            const float d = sqrtf((float)(D + c.cq));
            if (d < Ld[u][KT - 1]) {
                // slot a takes slot a - 1's entry where d is below that too, else d where it is
                // below slot a's (one compare per slot, carried down the list)
                bool here = true;
#pragma unroll
                for (int a = KT - 1; a > 0; --a) {
                    const bool up = d < Ld[u][a - 1];
                    Ld[u][a] = up ? Ld[u][a - 1] : here ? d : Ld[u][a];
                    Li[u][a] = up ? Li[u][a - 1] : here ? row : Li[u][a];
                    here = up;
                }
                Ld[u][0] = here ? d : Ld[u][0];
                Li[u][0] = here ? row : Li[u][0];
                lim[u] = i8_limit(Ld[u][KT - 1], c.cq);  // it only falls
            }
        }
    }
    __device__ __forceinline__ void finish(const I8Col (&col)[kKnnQT], int h, bool active) {
        if (!active) return;
#pragma unroll
        for (int u = 0; u < kKnnQT; ++u) {
            if (!col[u].valid) continue;
            // all KT slots, the unused ones in front included: the merge reads the last k
            TopkEnt* o = P.parts + ((size_t)(2 * split + h) * P.q_pad + col[u].q) * KT;
#pragma unroll
            for (int a = 0; a < KT; ++a) o[a] = TopkEnt{Ld[u][a], Li[u][a]};
        }
    }
};

template <int KT>
__global__ __launch_bounds__(kI8Threads) void knn_topk_i8_kernel(const CollI8Prob* __restrict__ probs,
                                                                 const KnnWork* __restrict__ works,
                                                                 const int* __restrict__ seg_start, int k) {
    i8_sweep<TopkI8Rule<KT>>(probs, works, seg_start, k);
}

// ---------------------------------------------------------------------------------------------------
// Merge and emit: a thread per query row, blockIdx.y the query set
// ---------------------------------------------------------------------------------------------------
constexpr int kMergeThreads = 128;

template <int KT>
__global__ __launch_bounds__(kMergeThreads) void knn_coll_merge_kernel(const CollQuery* __restrict__ queries,
                                                                       const CollPart* __restrict__ parts, int n_parts, int k,
                                                                       bool seed, int32_t* idx, int32_t* img, float* dist) {
    const CollQuery Q = queries[blockIdx.y];
    const int q = blockIdx.x * kMergeThreads + (int)threadIdx.x;
    if (q >= Q.nq) return;
    const long long o = Q.out_off + (long long)q * k;
    coll_merge_query<KT>(parts + (size_t)blockIdx.y * n_parts, n_parts, k, q, seed, idx + o, img + o, dist + o);
}

}  // namespace

void launch_knn_topk_i8(const CollI8Prob* probs, const KnnWork* works, const int* seg_start, int n_blocks, int k,
                        hipStream_t st) {
    if (n_blocks <= 0) return;
    topk_dispatch(k, [&](auto kt) { knn_topk_i8_kernel<decltype(kt)::value><<<n_blocks, kI8Threads, 0, st>>>(probs, works, seg_start, k); });
}

void launch_knn_coll_merge(const CollQuery* queries, int n_queries, const CollPart* parts, int n_parts, int max_nq, int k,
                           bool seed, int32_t* idx, int32_t* img, float* dist, hipStream_t st) {
    if (n_queries <= 0 || max_nq <= 0) return;
    const int gx = (max_nq + kMergeThreads - 1) / kMergeThreads;
    for (int q0 = 0; q0 < n_queries; q0 += 65535) {  // grid.y limit
        const dim3 grid(gx, std::min(n_queries - q0, 65535));
        const CollPart* p = parts + (size_t)q0 * n_parts;
        topk_dispatch(k, [&](auto kt) {
            knn_coll_merge_kernel<decltype(kt)::value><<<grid, kMergeThreads, 0, st>>>(queries + q0, p, n_parts, k, seed, idx, img, dist);
        });
    }
}

}  // namespace mim
