// knn_topk.hip — brute-force k-NN for k = 1..16 over every descriptor kind (BFMatcher(norm).knnMatch(k),
// DESIGN.md §16): a Hamming kernel for binary sets, a float kernel for generic float sets and for the f32
// rows of 128-D sets, and the kernel that merges their per-split lists and writes the knnMatch rows.
// The k = 2 kernels of hamming.hip / knn_float.hip / knn.hip are separate symbols and are not touched.
//
// Both distance kernels keep, per query, an ascending list of KT entries in VGPRs, KT = 4, 8 or 16 = k
// rounded up (one kernel per KT: the same for every block of a launch).  The list is only ever indexed by
// unrolled loop counters, so it stays in registers.  A pair enters the list behind one compare against the
// list's last entry, and the compare-exchange chain runs only where some lane of the wave has an event
// (a ballot branch, as flt_insert of knn_float.hip).
//
// Hamming: the sweep of sweep_hamming.h, packed keys d << 18 | row.  Keys of distinct rows are distinct and unsigned key
// order is (distance, row) order, so the k smallest keys of a query are the same however the rows are
// spread over tiles, waves and splits; the chain is min / max on the keys.
//
// Float: the sweep of sweep_float.h, one query per lane.  A lane meets its rows in
// ascending order, so inserting behind a strict < on the distance is OpenCV's tie rule.  OpenCV ranks on
// d = sqrtf(d2), and distinct d2 share a d, so the list holds d; the sqrt is taken for candidates only:
//   thr = nextafterf(kK * kK, +inf), kK the list's last distance (float product, rounded to nearest).
//   Claim: d2 > thr implies sqrtf(d2) >= kK, i.e. the pair is not inserted.
//   The float nearest to the real kK^2 is p = fl(kK * kK), so kK^2 lies between p's two neighbours and the
//   float after p is not below kK^2: thr >= kK^2 (p = +inf on overflow: thr = +inf, every pair is a
//   candidate; p = 0 on underflow: thr is the least denormal, and kK^2 < 2^-149 is below it).  Then
//   d2 > thr >= kK^2, sqrt is monotone on the reals and so is rounding to nearest: sqrtf(d2) >=
//   fl(sqrt(kK^2)) = fl(kK) = kK.  The candidates (d2 <= thr) are decided by the exact compare d < kK.
//   d2 = +inf (an overflow) is a candidate only while thr = +inf, and sqrtf gives +inf, never below
//   FLT_MAX: not inserted.  A NaN d2 fails d2 <= thr: not inserted.
//
// Output of both: the split's lists [q_pad][k] of TopkEnt (distance, row), (FLT_MAX, INT_MAX) past the end.
// gfx950, wave64.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>

#include "mim_internal.h"
#include "sweep_float.h"
#include "sweep_hamming.h"

namespace mim {

namespace {

// ---------------------------------------------------------------------------------------------------
// Hamming
// ---------------------------------------------------------------------------------------------------
constexpr uint32_t kHamNone = 0xFFFFFFFFu;  // packed-key sentinel: no row

// queries a lane holds: four (every wave holds the block's 256 queries and takes every fourth row of the
// tile) while the rows and lists of four queries fit beside a train row at 128 VGPRs, else two (two pairs
// of waves, each pair holds half of the block's queries and a wave of it takes every second row)
template <int W, int KT>
constexpr int ham_topk_qpt() { return W + KT <= 20 ? 4 : 2; }

// dwords of LDS: the tile, reused for one wave's lists per query group in the merge ([entry][query])
template <int KT>
constexpr int ham_topk_lds() { return kHamTileRows * 16 > KT * kHamBlockQ ? kHamTileRows * 16 : KT * kHamBlockQ; }

template <int KT>
__device__ __forceinline__ void ham_topk_insert(uint32_t (&L)[KT], uint32_t key) {
    if (__builtin_amdgcn_ballot_w64(key < L[KT - 1]) == 0) return;
    topk_chain<KT>(L, key);  // changes nothing in a lane whose key is not below its last entry
}

template <int W, int KT>
__device__ __forceinline__ void ham_topk_work(const TopkHamWork& w, int k, uint32_t* lds) {
    constexpr int QPT = ham_topk_qpt<W, KT>();
    constexpr int WPG = kHamWaves * QPT * kWave / kHamBlockQ;  // waves that share a group's queries
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int grp = wave / WPG, ph = wave % WPG;
    const int slot0 = grp * QPT * kWave + lane;  // slot0 + 64 j: the lane's j-th query within the block
    uint32_t L[QPT][KT];
#pragma unroll
    for (int j = 0; j < QPT; ++j)
#pragma unroll
        for (int s = 0; s < KT; ++s) L[j][s] = kHamNone;

    ham_sweep<W, QPT, WPG>(w.s, lds, [&](int j, uint32_t d, int row) { ham_topk_insert<KT>(L[j], (d << 18) | (uint32_t)row); });

    // the group's waves' lists into its first wave's, one wave at a time through LDS: mg[entry][slot]
    uint32_t* mg = lds;
#pragma unroll
    for (int v = 1; v < WPG; ++v) {
        __syncthreads();
        if (ph == v) {
#pragma unroll
            for (int j = 0; j < QPT; ++j)
#pragma unroll
                for (int s = 0; s < KT; ++s) mg[s * kHamBlockQ + slot0 + j * kWave] = L[j][s];
        }
        __syncthreads();
        if (ph == 0) {
#pragma unroll
            for (int j = 0; j < QPT; ++j)
#pragma unroll
                for (int s = 0; s < KT; ++s) ham_topk_insert<KT>(L[j], mg[s * kHamBlockQ + slot0 + j * kWave]);
        }
    }
    if (ph == 0) {
#pragma unroll
        for (int j = 0; j < QPT; ++j) {
            const int qi = w.s.q0 + slot0 + j * kWave;
            if (qi < w.s.nq) {
                TopkEnt* o = w.out + (size_t)qi * k;
#pragma unroll
                for (int s = 0; s < KT; ++s)
                    if (s < k) {
                        const uint32_t key = L[j][s];
                        o[s] = key == kHamNone ? TopkEnt{FLT_MAX, INT_MAX} : TopkEnt{(float)(key >> 18), (int)(key & 0x3FFFFu)};
                    }
            }
        }
    }
}

template <int KT>
__global__ __launch_bounds__(kHamThreads) void knn_topk_hamming_kernel(const TopkHamWork* __restrict__ works, int k) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[ham_topk_lds<KT>()];
    const TopkHamWork w = works[blockIdx.x];
    if (w.s.wdw == 4) ham_topk_work<4, KT>(w, k, lds);  // block-uniform
    else if (w.s.wdw == 8) ham_topk_work<8, KT>(w, k, lds);
    else ham_topk_work<16, KT>(w, k, lds);
}

// ---------------------------------------------------------------------------------------------------
// Float: the sink of sweep_float.h's sweep
// ---------------------------------------------------------------------------------------------------
template <int KT>
struct FltList {
    const TopkFltWork& w;
    const int k;
    float d[KT];  // ascending distances (sqrt values), FLT_MAX past the end
    int i[KT];    // their rows
    float thr;    // nextafterf(d[KT - 1]^2, +inf): see the file header

    __device__ __forceinline__ FltList(const TopkFltWork& w_, int k_) : w(w_), k(k_) {
#pragma unroll
        for (int a = 0; a < KT; ++a) {
            d[a] = FLT_MAX;
            i[a] = INT_MAX;
        }
        thr = __builtin_inff();
    }

    // The outer test is wave-wide (a scalar branch), as flt_insert's (knn_float.hip).
    __device__ __forceinline__ void pair(float d2, int row) {
        const bool cand = d2 <= thr;
        if (__builtin_amdgcn_ballot_w64(cand) == 0) return;
        if (cand) {
            const float x = sqrtf(d2);
            if (x < d[KT - 1]) {
#pragma unroll
                for (int a = KT - 1; a > 0; --a) {
                    const bool up = x < d[a - 1], here = x < d[a];
                    d[a] = up ? d[a - 1] : here ? x : d[a];
                    i[a] = up ? i[a - 1] : here ? row : i[a];
                }
                const bool first = x < d[0];
                d[0] = first ? x : d[0];
                i[0] = first ? row : i[0];
                const float p = d[KT - 1] * d[KT - 1];  // >= 0, never a NaN
                thr = p < __builtin_inff() ? __uint_as_float(__float_as_uint(p) + 1u) : p;
            }
        }
    }

    __device__ __forceinline__ void finish() {
        const int qi = w.s.q0 + (int)threadIdx.x;
        if (qi >= w.s.nq) return;
        TopkEnt* o = w.out + (size_t)qi * k;
#pragma unroll
        for (int a = 0; a < KT; ++a)
            if (a < k) o[a] = TopkEnt{d[a], i[a]};
    }
};

template <int KT>
__global__ __launch_bounds__(kFltThreads) void knn_topk_float_kernel(const TopkFltWork* __restrict__ works, int k) {
    __shared__ __attribute__((aligned(16))) float lds[kFltLdsFloats];
    const TopkFltWork w = works[blockIdx.x];
    FltList<KT> list(w, k);
    flt_sweep(w.s, lds, list);
}

// ---------------------------------------------------------------------------------------------------
// Merge and emit: a thread per query, blockIdx.y the problem
// ---------------------------------------------------------------------------------------------------
constexpr int kMergeThreads = 128;

template <int KT>
__global__ __launch_bounds__(kMergeThreads) void knn_topk_merge_kernel(const TopkProb* __restrict__ probs, int k) {
    const TopkProb P = probs[blockIdx.y];
    const int q = blockIdx.x * kMergeThreads + (int)threadIdx.x;
    if (q >= P.nq) return;
    topk_merge_query<KT>(P.parts, P.nsplit, P.q_pad, k, q, P.idx + (size_t)q * k, P.dist + (size_t)q * k);
}

}  // namespace

void launch_knn_topk_hamming(const TopkHamWork* works, int n_works, int k, hipStream_t st) {
    if (n_works <= 0) return;
    topk_dispatch(k, [&](auto kt) { knn_topk_hamming_kernel<decltype(kt)::value><<<n_works, kHamThreads, 0, st>>>(works, k); });
}

void launch_knn_topk_float(const TopkFltWork* works, int n_works, int k, hipStream_t st) {
    if (n_works <= 0) return;
    topk_dispatch(k, [&](auto kt) { knn_topk_float_kernel<decltype(kt)::value><<<n_works, kFltThreads, 0, st>>>(works, k); });
}

// probs: n_probs records on the device; max_nq: the most query rows of one of them
void launch_knn_topk_merge(const TopkProb* probs, int n_probs, int max_nq, int k, hipStream_t st) {
    if (n_probs <= 0 || max_nq <= 0) return;
    const int gx = (max_nq + kMergeThreads - 1) / kMergeThreads;
    for (int p0 = 0; p0 < n_probs; p0 += 65535) {  // grid.y limit
        const dim3 grid(gx, std::min(n_probs - p0, 65535));
        topk_dispatch(k, [&](auto kt) { knn_topk_merge_kernel<decltype(kt)::value><<<grid, kMergeThreads, 0, st>>>(probs + p0, k); });
    }
}

}  // namespace mim
