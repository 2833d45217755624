// radius.hip — brute-force radius matching over every descriptor kind (BFMatcher(norm).radiusMatch, DESIGN.md
// §17): for every query row every train row with DMatch::distance <= maxDistance, sorted by (distance, row).
//
// Two passes over the same work items, one kernel template with a kFill flag per kind.  The count pass adds 1
// to its query's count per passing pair (vector atomics; integer sums do not depend on the order), a scan
// turns the counts into offsets, and the fill pass recomputes the same pairs, takes a slot from the query's
// cursor and writes radius_key(distance, row) at offsets[query] + slot, bounds-checked against
// offsets[query + 1].  The keys of one query are distinct, so the sort kernel fixes the result whatever the
// arrival order was.  No partial buffers: a train split only adds to the same counts.
//
// Hamming: the sweep of sweep_hamming.h, the compare d <= floor(r) for a sink.
// Float: the sweep of sweep_float.h; the literal test sqrtf(d2) <= r is the compare d2 <= T with T the largest
//   float whose sqrtf is <= r (radius_flt_threshold: sqrtf is monotone), which spares the count pass the sqrt
//   sequence, about a tenth of a 128-D pair.
// i8 MFMA (128-D sets whose flags say integer-valued on both sides): the frame of sweep_i8.h.  sqrtf((float)d^2)
//   <= r is d^2 <= T2 (radius_int_threshold), per query 2R + p <= tau = T2 - c(q); every accumulator is filtered
//   against floor(tau / 2) (2R + p <= tau implies R <= floor(tau / 2)), and only a wave with a hit reads the
//   parities and decides exactly.
// gfx950, wave64.
#include <hip/hip_runtime.h>

#include <climits>

#include "radius.h"
#include "sweep_float.h"
#include "sweep_hamming.h"
#include "sweep_i8.h"

namespace mim {

namespace {

// the fill pass's write of one match of query gq (numbered over the call)
__device__ __forceinline__ void rad_emit(const RadArgs& a, long long gq, float d, int row) {
    const int slot = atomicAdd(a.cursor + gq, 1);
    const long long pos = a.offsets[gq] + slot;
    if (pos < a.offsets[gq + 1]) a.keys[pos] = radius_key(d, row);
}

// ---------------------------------------------------------------------------------------------------
// Hamming: every wave holds the block's 256 queries, 4 per lane, and takes every 4th row
// ---------------------------------------------------------------------------------------------------
constexpr int kHamQpt = kHamBlockQ / kWave;

template <bool kFill>
struct RadHamSink {
    const RadHamWork& w;
    const RadArgs& a;
    const int q0;  // the lane's j-th query: q0 + 64 j
    int cnt[kHamQpt];
    __device__ __forceinline__ void operator()(int j, uint32_t d, int row) {
        const int qi = q0 + j * kWave;
        const bool hit = d <= (uint32_t)a.ham_t && qi < w.s.nq;  // ham_t >= 0: the entries accept only r > FLT_EPSILON
        if (kFill) {
            if (hit) rad_emit(a, w.qoff + qi, (float)d, row);
        } else {
            cnt[j] += hit;
        }
    }
};

template <int W, bool kFill>
__device__ __forceinline__ void rad_ham_work(const RadHamWork& w, const RadArgs& a, uint32_t* lds) {
    RadHamSink<kFill> sink{w, a, w.s.q0 + (int)(threadIdx.x & 63), {}};
    ham_sweep<W, kHamQpt, kHamWaves>(w.s, lds, sink);
    if (!kFill) {
#pragma unroll
        for (int j = 0; j < kHamQpt; ++j) {
            const int qi = sink.q0 + j * kWave;
            if (qi < w.s.nq && sink.cnt[j] != 0) atomicAdd(a.counts + w.qoff + qi, sink.cnt[j]);
        }
    }
}

template <bool kFill>
__global__ __launch_bounds__(kHamThreads) void radius_hamming_kernel(const RadHamWork* __restrict__ works, RadArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[kHamTileRows * 16];
    const RadHamWork w = works[blockIdx.x];
    if (w.s.wdw == 4) rad_ham_work<4, kFill>(w, a, lds);  // block-uniform
    else if (w.s.wdw == 8) rad_ham_work<8, kFill>(w, a, lds);
    else rad_ham_work<16, kFill>(w, a, lds);
}

// ---------------------------------------------------------------------------------------------------
// Float.  sqrtf(d2) <= r as d2 <= T (radius_flt_threshold: the same pairs, bit for bit; a NaN d2 never passes,
// +inf only r = +inf); the sqrt is taken for the matches the fill pass writes
// ---------------------------------------------------------------------------------------------------
template <bool kFill>
struct RadFltSink {
    const RadFltWork& w;
    const RadArgs& a;
    const int qi;
    int cnt;
    __device__ __forceinline__ void pair(float d2, int row) {
        const bool hit = d2 <= a.flt_t && qi < w.s.nq;
        if (kFill) {
            if (hit) rad_emit(a, w.qoff + qi, sqrtf(d2), row);
        } else {
            cnt += hit;
        }
    }
    __device__ __forceinline__ void finish() {
        if (!kFill && qi < w.s.nq && cnt != 0) atomicAdd(a.counts + w.qoff + qi, cnt);
    }
};

template <bool kFill>
__global__ __launch_bounds__(kFltThreads) void radius_float_kernel(const RadFltWork* __restrict__ works, RadArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[kFltLdsFloats];
    const RadFltWork w = works[blockIdx.x];
    RadFltSink<kFill> sink{w, a, w.s.q0 + (int)threadIdx.x, 0};
    flt_sweep(w.s, lds, sink);
}

// ---------------------------------------------------------------------------------------------------
// i8 MFMA: the rule of sweep_i8.h's frame.  tau = T2 - c(q) of the lane's column in each column tile: c(q)
// lies within +-2^22 and T2 in [-1, 2^23), so tau cannot leave int32.  A column past the set gets the least
// tau: nothing passes, and `valid` bounds it explicitly.  A padded train row's R is never under a
// floor(tau / 2) below 2^23.
// ---------------------------------------------------------------------------------------------------
template <bool kFill>
struct RadI8Rule {
    static constexpr bool kSkipEmpty = true, kFixedLimit = true;
    const RadArgs& a;
    const long long qoff;
    int tau[kKnnQT], hf[kKnnQT], cnt[kKnnQT];

    __device__ __forceinline__ RadI8Rule(const RadI8Prob& P, const KnnWork&, const RadArgs& args) : a(args), qoff(P.qoff) {}
    __device__ __forceinline__ void init(int u, const I8Col& c) {
        tau[u] = c.valid ? a.int_t2 - c.cq : INT_MIN;
        hf[u] = tau[u] >> 1;  // floor(tau / 2)
        cnt[u] = 0;
    }
    __device__ __forceinline__ void begin() {}
    __device__ __forceinline__ int limit(int u) const { return hf[u]; }
    __device__ __forceinline__ void row(int u, const I8Col& c, int R, unsigned par, int row, int nt) {
        // 2R + p without signed overflow (a padded row's wraps and is cut by row < nt)
        const int D = (int)(((unsigned)R << 1) | par);
        const bool hit = D <= tau[u] && row < nt && c.valid;
        if (kFill) {
            if (hit) rad_emit(a, qoff + c.q, sqrtf((float)(D + c.cq)), row);
        } else {
            cnt[u] += hit;
        }
    }
    __device__ __forceinline__ void finish(const I8Col (&col)[kKnnQT], int h, bool) {
        if (kFill) return;
#pragma unroll
        for (int u = 0; u < kKnnQT; ++u) {
            const int c = cnt[u] + __shfl_xor(cnt[u], 32);  // the two halves hold disjoint rows of one query
            if (h == 0 && col[u].valid && c != 0) atomicAdd(a.counts + qoff + col[u].q, c);
        }
    }
};

template <bool kFill>
__global__ __launch_bounds__(kI8Threads) void radius_i8_kernel(const RadI8Prob* __restrict__ probs,
                                                               const KnnWork* __restrict__ works,
                                                               const int* __restrict__ seg_start, RadArgs a) {
    i8_sweep<RadI8Rule<kFill>>(probs, works, seg_start, a);
}

// ---------------------------------------------------------------------------------------------------
// Scan: offsets[i] = the matches before query i.  Two launches over blocks of kScanBlockQ queries: the blocks'
// sums and longest lists into meta[2 + 2 b], meta[3 + 2 b]; then every block adds up the sums before it, scans
// its own counts and clears its cursors, and the last block writes the total and the longest list.
// ---------------------------------------------------------------------------------------------------
constexpr int kScanThreads = 1024, kScanPer = 4, kScanBlockQ = kScanThreads * kScanPer;

// sum over the block (every thread gets it); red: kScanThreads / kWave words, free to reuse after the call
__device__ __forceinline__ long long scan_block_sum(long long v, long long* red) {
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) v += __shfl_xor(v, d);
    __syncthreads();  // earlier reads of red
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    long long t = 0;
    for (int w = 0; w < kScanThreads / kWave; ++w) t += red[w];
    return t;
}
__device__ __forceinline__ long long scan_block_max(long long v, long long* red) {
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) v = max(v, (long long)__shfl_xor(v, d));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    long long t = 0;
    for (int w = 0; w < kScanThreads / kWave; ++w) t = max(t, red[w]);
    return t;
}

__global__ __launch_bounds__(kScanThreads) void radius_scan_sums_kernel(const int* __restrict__ counts, long long n,
                                                                        long long* __restrict__ meta) {
    __shared__ long long red[kScanThreads / kWave];
    const long long i0 = (long long)blockIdx.x * kScanBlockQ + (long long)threadIdx.x * kScanPer;
    long long s = 0, mx = 0;
#pragma unroll
    for (int k = 0; k < kScanPer; ++k) {
        const int c = i0 + k < n ? counts[i0 + k] : 0;
        s += c;
        mx = max(mx, (long long)c);
    }
    s = scan_block_sum(s, red);
    mx = scan_block_max(mx, red);
    if (threadIdx.x == 0) {
        meta[2 + 2 * blockIdx.x] = s;
        meta[3 + 2 * blockIdx.x] = mx;
    }
}

__global__ __launch_bounds__(kScanThreads) void radius_scan_kernel(const int* __restrict__ counts, int* __restrict__ cursor,
                                                                   long long* __restrict__ offsets,
                                                                   long long* __restrict__ offsets_user, long long n,
                                                                   long long* __restrict__ meta) {
    __shared__ long long red[kScanThreads / kWave];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x, nb = gridDim.x;
    long long part = 0;
    for (int v = tid; v < b; v += kScanThreads) part += meta[2 + 2 * v];
    const long long carry = scan_block_sum(part, red);
    const long long i0 = (long long)b * kScanBlockQ + (long long)tid * kScanPer;
    int c[kScanPer];
    long long s = 0;
#pragma unroll
    for (int k = 0; k < kScanPer; ++k) {
        c[k] = i0 + k < n ? counts[i0 + k] : 0;
        s += c[k];
    }
    long long incl = s;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const long long o = __shfl_up(incl, d);
        if (lane >= d) incl += o;
    }
    __syncthreads();  // scan_block_sum's reads of red
    if (lane == kWave - 1) red[wave] = incl;
    __syncthreads();
    long long before = 0, total = 0;
    for (int v = 0; v < kScanThreads / kWave; ++v) {
        before += v < wave ? red[v] : 0;
        total += red[v];
    }
    long long o = carry + before + incl - s;
#pragma unroll
    for (int k = 0; k < kScanPer; ++k) {
        if (i0 + k < n) {
            offsets[i0 + k] = o;
            if (offsets_user) offsets_user[i0 + k] = o;
            cursor[i0 + k] = 0;
        }
        o += c[k];
    }
    if (b == nb - 1) {  // block-uniform
        long long mx = 0;
        for (int v = tid; v < nb; v += kScanThreads) mx = max(mx, meta[3 + 2 * v]);
        mx = scan_block_max(mx, red);
        if (tid == 0) {
            offsets[n] = carry + total;
            if (offsets_user) offsets_user[n] = carry + total;
            meta[0] = carry + total;
            meta[1] = mx;
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// Sort and emit: a block per query list, grid-strided.  A list of up to kRadSortCap keys is padded with
// UINT64_MAX to a power of two and sorted in LDS (bitonic).  A longer list is sorted in runs of kRadSortCap,
// then the runs are merged pairwise in passes between the key buffer and the scratch buffer: each element
// finds its place by its position in its own run plus a binary search in the other (radius_pass_place).
// The list's keys are then split into the caller's idx / dist.  keys / scratch are read after they were
// written by other threads of the block: plain pointers, a barrier between the passes.
// ---------------------------------------------------------------------------------------------------
constexpr int kSortThreads = 256;

__global__ __launch_bounds__(kSortThreads) void radius_sort_kernel(const long long* __restrict__ offsets, long long n_queries,
                                                                   unsigned long long* keys, unsigned long long* scratch,
                                                                   int32_t* __restrict__ idx, float* __restrict__ dist) {
    __shared__ unsigned long long s[kRadSortCap];
    const int tid = threadIdx.x;
    for (long long seg = blockIdx.x; seg < n_queries; seg += gridDim.x) {
        const long long o0 = offsets[seg], L = offsets[seg + 1] - o0;
        if (L <= 0) continue;  // block-uniform
        unsigned long long* K = keys + o0;
        for (long long run0 = 0; run0 < L; run0 += kRadSortCap) {
            const int n = (int)min((long long)kRadSortCap, L - run0);
            int p2 = 2;
            while (p2 < n) p2 <<= 1;
            __syncthreads();  // the previous run's reads of s
            for (int i = tid; i < p2; i += kSortThreads) s[i] = i < n ? K[run0 + i] : ~0ull;
            __syncthreads();
            for (int k = 2; k <= p2; k <<= 1)
                for (int j = k >> 1; j > 0; j >>= 1) {
                    for (int i = tid; i < p2; i += kSortThreads) {
                        const int x = i ^ j;
                        if (x > i) {
                            const unsigned long long va = s[i], vb = s[x];
                            if ((va > vb) == ((i & k) == 0)) {
                                s[i] = vb;
                                s[x] = va;
                            }
                        }
                    }
                    __syncthreads();
                }
            if (L <= kRadSortCap) {
                for (int i = tid; i < n; i += kSortThreads) {
                    idx[o0 + i] = radius_key_row(s[i]);
                    dist[o0 + i] = radius_key_dist(s[i]);
                }
            } else {
                for (int i = tid; i < n; i += kSortThreads) K[run0 + i] = s[i];
            }
        }
        if (L <= kRadSortCap) continue;
        unsigned long long* src = K;
        unsigned long long* dst = scratch + o0;
        for (long long width = kRadSortCap; width < L; width *= 2) {
            __syncthreads();  // the runs (or the previous pass) are written
            for (long long i = tid; i < L; i += kSortThreads)
                dst[radius_pass_place(reinterpret_cast<const uint64_t*>(src), L, width, i)] = src[i];
            unsigned long long* t = src;
            src = dst;
            dst = t;
        }
        __syncthreads();
        for (long long i = tid; i < L; i += kSortThreads) {
            idx[o0 + i] = radius_key_row(src[i]);
            dist[o0 + i] = radius_key_dist(src[i]);
        }
    }
}

}  // namespace

void launch_radius_hamming(const RadHamWork* works, int n_works, const RadArgs& a, bool fill, hipStream_t st) {
    if (n_works <= 0) return;
    if (fill) radius_hamming_kernel<true><<<n_works, kHamThreads, 0, st>>>(works, a);
    else radius_hamming_kernel<false><<<n_works, kHamThreads, 0, st>>>(works, a);
}

void launch_radius_float(const RadFltWork* works, int n_works, const RadArgs& a, bool fill, hipStream_t st) {
    if (n_works <= 0) return;
    if (fill) radius_float_kernel<true><<<n_works, kFltThreads, 0, st>>>(works, a);
    else radius_float_kernel<false><<<n_works, kFltThreads, 0, st>>>(works, a);
}

void launch_radius_i8(const RadI8Prob* probs, const KnnWork* works, const int* seg_start, int n_blocks, const RadArgs& a,
                      bool fill, hipStream_t st) {
    if (n_blocks <= 0) return;
    if (fill) radius_i8_kernel<true><<<n_blocks, kI8Threads, 0, st>>>(probs, works, seg_start, a);
    else radius_i8_kernel<false><<<n_blocks, kI8Threads, 0, st>>>(probs, works, seg_start, a);
}

void launch_radius_scan(const int* counts, int* cursor, long long* offsets, long long* offsets_user, long long n_queries,
                        long long* meta, hipStream_t st) {
    const int nb = radius_scan_blocks(n_queries);
    radius_scan_sums_kernel<<<nb, kScanThreads, 0, st>>>(counts, n_queries, meta);
    radius_scan_kernel<<<nb, kScanThreads, 0, st>>>(counts, cursor, offsets, offsets_user, n_queries, meta);
}

int radius_scan_blocks(long long n_queries) { return (int)std::max<long long>(1, (n_queries + kScanBlockQ - 1) / kScanBlockQ); }

void launch_radius_sort(const long long* offsets, long long n_queries, unsigned long long* keys,
                        unsigned long long* scratch, int32_t* idx, float* dist, hipStream_t st) {
    if (n_queries <= 0) return;
    const int grid = (int)std::min<long long>(n_queries, 1 << 16);
    radius_sort_kernel<<<grid, kSortThreads, 0, st>>>(offsets, n_queries, keys, scratch, idx, dist);
}

}  // namespace mim
