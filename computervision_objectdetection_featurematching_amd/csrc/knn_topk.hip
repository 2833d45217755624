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
// Hamming: the sweep of ham_work (hamming.hip): LDS tile of kHamTileRows rows read at wave-uniform
// addresses, xor + popcount, packed keys d << 18 | row.  Keys of distinct rows are distinct and unsigned key
// order is (distance, row) order, so the k smallest keys of a query are the same however the rows are
// spread over tiles, waves and splits; the chain is min / max on the keys.
//
// Float: the arithmetic of knn_float.hip (knn_float_arith.h), one query per lane.  A lane meets its rows in
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

#include "knn_float_arith.h"  // flt_round, flt_reduce, flt_tail4, flt_tile_rows; fp contraction off
#include "mim_internal.h"

namespace mim {

namespace {

// ---------------------------------------------------------------------------------------------------
// Hamming
// ---------------------------------------------------------------------------------------------------
constexpr int kHamThreads = 256;  // 4 waves
constexpr int kHamWaves = kHamThreads / kWave;
constexpr uint32_t kHamNone = 0xFFFFFFFFu;  // packed-key sentinel: no row

// popcount(x) + acc as the one instruction it is (hamming.hip popc_add)
__device__ __forceinline__ uint32_t popc_add(uint32_t x, uint32_t acc) {
    uint32_t r;
    asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(acc));
    return r;
}

// queries a lane holds: four (ham_work's layout: every wave holds the block's 256 queries and takes every
// fourth row of the tile) while the rows and lists of four queries fit beside a train row at 128 VGPRs,
// else two (two pairs of waves, each pair holds half of the block's queries and a wave of it takes every
// second row)
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
    constexpr int GROUPS = kHamBlockQ / (QPT * kWave);  // query groups of the block
    constexpr int WPG = kHamWaves / GROUPS;             // waves that share a group's queries
    static_assert(GROUPS * WPG == kHamWaves && GROUPS * QPT * kWave == kHamBlockQ, "waves tile the block's queries");
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = wave / WPG, ph = wave % WPG;
    const int slot0 = grp * QPT * kWave + lane;  // slot0 + 64 j: the lane's j-th query within the block
    uint32_t q[QPT][W];
#pragma unroll
    for (int j = 0; j < QPT; ++j) {
        const int qi = w.q0 + slot0 + j * kWave;
        const bool ok = qi < w.nq;
#pragma unroll
        for (int c = 0; c < W; c += 4) {
            const uint4 v = ok ? *reinterpret_cast<const uint4*>(w.q + (size_t)qi * W + c) : make_uint4(0, 0, 0, 0);
            q[j][c] = v.x; q[j][c + 1] = v.y; q[j][c + 2] = v.z; q[j][c + 3] = v.w;
        }
    }
    uint32_t L[QPT][KT];
#pragma unroll
    for (int j = 0; j < QPT; ++j)
#pragma unroll
        for (int s = 0; s < KT; ++s) L[j][s] = kHamNone;

    // train rows [r0, r1): r0 is a multiple of kHamTileRows, and the set's storage is zero rows up to
    // the next multiple past its last row, so a whole tile is always readable
    for (int r = w.r0; r < w.r1; r += kHamTileRows) {
        __syncthreads();
        const uint4* src = reinterpret_cast<const uint4*>(w.t + (size_t)r * W);
        for (int e = tid; e < kHamTileRows * W / 4; e += kHamThreads) reinterpret_cast<uint4*>(lds)[e] = src[e];
        __syncthreads();
        const int rows = min(kHamTileRows, w.r1 - r);
        for (int rr = ph; rr < rows; rr += WPG) {
            uint32_t t[W];
#pragma unroll
            for (int c = 0; c < W; c += 4) {
                const uint4 v = *reinterpret_cast<const uint4*>(lds + rr * W + c);
                t[c] = v.x; t[c + 1] = v.y; t[c + 2] = v.z; t[c + 3] = v.w;
            }
            const uint32_t row = (uint32_t)(r + rr);
#pragma unroll
            for (int j = 0; j < QPT; ++j) {
                uint32_t d = __popc(q[j][0] ^ t[0]);
#pragma unroll
                for (int c = 1; c < W; ++c) d = popc_add(q[j][c] ^ t[c], d);
                ham_topk_insert<KT>(L[j], (d << 18) | row);
            }
        }
    }

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
            const int qi = w.q0 + slot0 + j * kWave;
            if (qi < w.nq) {
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
    if (w.wdw == 4) ham_topk_work<4, KT>(w, k, lds);  // block-uniform
    else if (w.wdw == 8) ham_topk_work<8, KT>(w, k, lds);
    else ham_topk_work<16, KT>(w, k, lds);
}

// ---------------------------------------------------------------------------------------------------
// Float
// ---------------------------------------------------------------------------------------------------
constexpr int kFltThreads = 256;     // 4 waves, a query per lane
constexpr int kFltLdsFloats = 8192;  // 32 KiB train tile
constexpr int kFltR = 4;             // train rows in flight on the streamed path
static_assert(kFltThreads == kFltBlockQ, "one query per thread");
static_assert(kFltRowPad * 128 <= kFltLdsFloats && 16 * kFltMaxDim <= kFltLdsFloats, "tile fits the LDS");

template <int KT>
struct FltList {
    float d[KT];  // ascending distances (sqrt values), FLT_MAX past the end
    int i[KT];    // their rows
    float thr;    // nextafterf(d[KT - 1]^2, +inf): see the file header
};

template <int KT>
__device__ __forceinline__ void flt_list_init(FltList<KT>& s) {
#pragma unroll
    for (int a = 0; a < KT; ++a) {
        s.d[a] = FLT_MAX;
        s.i[a] = INT_MAX;
    }
    s.thr = __builtin_inff();
}

// The outer test is wave-wide (a scalar branch), as flt_insert's (knn_float.hip).
template <int KT>
__device__ __forceinline__ void flt_list_insert(FltList<KT>& s, float d2, int row) {
    const bool cand = d2 <= s.thr;
    if (__builtin_amdgcn_ballot_w64(cand) == 0) return;
    if (cand) {
        const float d = sqrtf(d2);
        if (d < s.d[KT - 1]) {
#pragma unroll
            for (int a = KT - 1; a > 0; --a) {
                const bool up = d < s.d[a - 1], here = d < s.d[a];
                s.d[a] = up ? s.d[a - 1] : here ? d : s.d[a];
                s.i[a] = up ? s.i[a - 1] : here ? row : s.i[a];
            }
            const bool first = d < s.d[0];
            s.d[0] = first ? d : s.d[0];
            s.i[0] = first ? row : s.i[0];
            const float p = s.d[KT - 1] * s.d[KT - 1];  // >= 0, never a NaN
            s.thr = p < __builtin_inff() ? __uint_as_float(__float_as_uint(p) + 1u) : p;
        }
    }
}

template <int KT>
__device__ __forceinline__ void flt_list_store(const TopkFltWork& w, int k, int qi, const FltList<KT>& s) {
    if (qi >= w.nq) return;
    TopkEnt* o = w.out + (size_t)qi * k;
#pragma unroll
    for (int a = 0; a < KT; ++a)
        if (a < k) o[a] = TopkEnt{s.d[a], s.i[a]};
}

// tile [r, r + TR) of the train rows into LDS; rows from nt on are not read (the f32 rows of a 128-D set
// end there) and are staged as zeros
__device__ __forceinline__ void flt_topk_stage(const TopkFltWork& w, int r, int TR, float* lds) {
    const int total = TR * w.dp, have = min(TR, w.nt - r) * w.dp;
    const float* src = w.t + (size_t)r * w.dp;
    if (w.vec) {
        const float4* src4 = reinterpret_cast<const float4*>(src);
        float4* lds4 = reinterpret_cast<float4*>(lds);
        for (int e = threadIdx.x; e < total / 4; e += kFltThreads)
            lds4[e] = e < have / 4 ? src4[e] : make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
        for (int e = threadIdx.x; e < total; e += kFltThreads) lds[e] = e < have ? src[e] : 0.f;
    }
}

// dim = dp = 16 NR <= 128: the query row in 16 NR VGPRs, one train row at a time (flt_resident)
template <int NR, int KT>
__device__ __forceinline__ void flt_topk_resident(const TopkFltWork& w, int k, float* lds) {
    constexpr int DP4 = 4 * NR, TR = 64;
    const int qi = w.q0 + (int)threadIdx.x;
    const float* qp = w.q + (size_t)min(qi, w.nq - 1) * (DP4 * 4);
    float4 q[DP4];
    if (w.vec) {
#pragma unroll
        for (int c = 0; c < DP4; ++c) q[c] = reinterpret_cast<const float4*>(qp)[c];
    } else {
#pragma unroll
        for (int c = 0; c < DP4; ++c) q[c] = make_float4(qp[4 * c], qp[4 * c + 1], qp[4 * c + 2], qp[4 * c + 3]);
    }
    FltList<KT> s;
    flt_list_init(s);
    const float4* lds4 = reinterpret_cast<const float4*>(lds);
    for (int r = w.r0; r < w.r1; r += TR) {
        __syncthreads();
        flt_topk_stage(w, r, TR, lds);
        __syncthreads();
        const int rows = min(TR, w.r1 - r);
        for (int rr = 0; rr < rows; ++rr) {
            f2 acc[8];
#pragma unroll
            for (int a = 0; a < 8; ++a) acc[a] = f2{0.f, 0.f};
            const float4* t = lds4 + rr * DP4;
#pragma unroll
            for (int c = 0; c < NR; ++c) flt_round(acc, q + 4 * c, t + 4 * c);
            flt_list_insert(s, flt_reduce(acc), r + rr);
        }
    }
    flt_list_store(w, k, qi, s);
}

// any dim (generic float sets only: their rows are 16-byte aligned): flt_streamed with the list
template <int KT>
__device__ __forceinline__ void flt_topk_streamed(const TopkFltWork& w, int k, float* lds) {
    const int dp4 = w.dp >> 2, rounds = w.dim >> 4;
    const int TR = flt_tile_rows(w.dp);
    const int qi = w.q0 + (int)threadIdx.x;
    const float4* qrow = reinterpret_cast<const float4*>(w.q + (size_t)min(qi, w.nq - 1) * w.dp);
    FltList<KT> s;
    flt_list_init(s);
    const float4* lds4 = reinterpret_cast<const float4*>(lds);
    for (int r = w.r0; r < w.r1; r += TR) {
        __syncthreads();
        flt_topk_stage(w, r, TR, lds);
        __syncthreads();
        const int rows = min(TR, w.r1 - r);
        for (int rr = 0; rr < rows; rr += kFltR) {  // rr + j < TR: rows past `rows` are computed, not inserted
            f2 acc[kFltR][8];
#pragma unroll
            for (int j = 0; j < kFltR; ++j)
#pragma unroll
                for (int a = 0; a < 8; ++a) acc[j][a] = f2{0.f, 0.f};
            const float4* t = lds4 + rr * dp4;
            for (int c = 0; c < rounds; ++c) {
                float4 qv[4];
#pragma unroll
                for (int v = 0; v < 4; ++v) qv[v] = qrow[4 * c + v];
#pragma unroll
                for (int j = 0; j < kFltR; ++j) flt_round(acc[j], qv, t + j * dp4 + 4 * c);
            }
            float d[kFltR];
#pragma unroll
            for (int j = 0; j < kFltR; ++j) d[j] = flt_reduce(acc[j]);  // all zero without a full round
            for (int c4 = 4 * rounds; c4 < dp4; ++c4) {
                const float4 qv = qrow[c4];
#pragma unroll
                for (int j = 0; j < kFltR; ++j) d[j] = flt_tail4(d[j], qv, t[j * dp4 + c4]);
            }
#pragma unroll
            for (int j = 0; j < kFltR; ++j)
                if (rr + j < rows) flt_list_insert(s, d[j], r + rr + j);
        }
    }
    flt_list_store(w, k, qi, s);
}

template <int KT>
__global__ __launch_bounds__(kFltThreads) void knn_topk_float_kernel(const TopkFltWork* __restrict__ works, int k) {
    __shared__ __attribute__((aligned(16))) float lds[kFltLdsFloats];
    const TopkFltWork w = works[blockIdx.x];
    // collection calls on 128-D sets that are integer-valued on both sides: the i8 kernel's (block-uniform, as
    // radius_float_kernel); null from the other entries
    if (w.qflags && !(*w.qflags | *w.tflags)) return;
    if ((w.dim & 15) == 0 && w.dim <= 128 && w.dp == w.dim) {  // block-uniform
        switch (w.dim >> 4) {
            case 1: flt_topk_resident<1, KT>(w, k, lds); break;
            case 2: flt_topk_resident<2, KT>(w, k, lds); break;
            case 3: flt_topk_resident<3, KT>(w, k, lds); break;
            case 4: flt_topk_resident<4, KT>(w, k, lds); break;
            case 5: flt_topk_resident<5, KT>(w, k, lds); break;
            case 6: flt_topk_resident<6, KT>(w, k, lds); break;
            case 7: flt_topk_resident<7, KT>(w, k, lds); break;
            default: flt_topk_resident<8, KT>(w, k, lds); break;
        }
    } else {
        flt_topk_streamed<KT>(w, k, lds);
    }
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
    if (k <= 4) knn_topk_hamming_kernel<4><<<n_works, kHamThreads, 0, st>>>(works, k);
    else if (k <= 8) knn_topk_hamming_kernel<8><<<n_works, kHamThreads, 0, st>>>(works, k);
    else knn_topk_hamming_kernel<16><<<n_works, kHamThreads, 0, st>>>(works, k);
}

void launch_knn_topk_float(const TopkFltWork* works, int n_works, int k, hipStream_t st) {
    if (n_works <= 0) return;
    if (k <= 4) knn_topk_float_kernel<4><<<n_works, kFltThreads, 0, st>>>(works, k);
    else if (k <= 8) knn_topk_float_kernel<8><<<n_works, kFltThreads, 0, st>>>(works, k);
    else knn_topk_float_kernel<16><<<n_works, kFltThreads, 0, st>>>(works, k);
}

// probs: n_probs records on the device; max_nq: the most query rows of one of them
void launch_knn_topk_merge(const TopkProb* probs, int n_probs, int max_nq, int k, hipStream_t st) {
    if (n_probs <= 0 || max_nq <= 0) return;
    const int gx = (max_nq + kMergeThreads - 1) / kMergeThreads;
    for (int p0 = 0; p0 < n_probs; p0 += 65535) {  // grid.y limit
        const dim3 grid(gx, std::min(n_probs - p0, 65535));
        if (k <= 4) knn_topk_merge_kernel<4><<<grid, kMergeThreads, 0, st>>>(probs + p0, k);
        else if (k <= 8) knn_topk_merge_kernel<8><<<grid, kMergeThreads, 0, st>>>(probs + p0, k);
        else knn_topk_merge_kernel<16><<<grid, kMergeThreads, 0, st>>>(probs + p0, k);
    }
}

}  // namespace mim
