// hamming.hip — brute-force 2-NN over binary descriptors (BFMatcher(NORM_HAMMING).knnMatch, k = 2).
//
// Rows are CV_8U descriptors (ORB, BRIEF, BRISK, FREAK, AKAZE, LATCH) zero-padded to 16, 32 or 64 bytes
// (DESIGN.md "Binary descriptors").  The distance is popcount(q ^ t) summed over the row's dwords, an
// integer <= 512, so everything is exact.  Output: the same Top2 partials [split][q_pad] that
// ratio_compact_kernel / knn_emit_kernel (knn.hip) merge; key = (float)distance, sentinels
// FLT_MAX / INT_MAX.  knn2_hamming_cross_kernel is the same sweep for cross-check batches: it also leaves each
// train row's nearest query row.  gfx950, wave64.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>

#include "mim_internal.h"
#include "sweep_hamming.h"  // kHamThreads, kHamWaves, popc_add

namespace mim {

namespace {

constexpr int kHamQPT = kHamBlockQ / kWave;       // query rows held by one lane
constexpr uint32_t kHamNone = 0xFFFFFFFFu;        // packed-key sentinel: no row
static_assert(kHamQPT * kWave == kHamBlockQ, "a block's queries are whole waves of lanes");
static_assert(kHamTileRows * 64 >= kHamWaves * kHamBlockQ * 8, "the merge scratch reuses the tile's LDS");

// Minimum of x over the wave's 64 lanes, in registers: four row_shr steps leave each 16-lane row's
// minimum in its lane 15, row_bcast:15 carries it into rows 1 and 3, row_bcast:31 into rows 2 and 3;
// lane 63 then holds the wave's, read back as a wave-uniform value.  A lane whose DPP source lies outside
// its row, or whose row the step masks off, takes all ones, the identity of the unsigned minimum, and so
// keeps its own value (no bound_ctrl); with the identity as `old` the move folds into v_min_u32_dpp.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_min_step(uint32_t x) {
    return min(x, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)x, CTRL, ROW_MASK, 0xF, false));
}
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t x) {
    x = dpp_min_step<0x111, 0xF>(x);  // row_shr:1
    x = dpp_min_step<0x112, 0xF>(x);  // row_shr:2
    x = dpp_min_step<0x114, 0xF>(x);  // row_shr:4
    x = dpp_min_step<0x118, 0xF>(x);  // row_shr:8
    x = dpp_min_step<0x142, 0xA>(x);  // row_bcast:15
    x = dpp_min_step<0x143, 0xC>(x);  // row_bcast:31
    return (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
}

// One work item for rows of W dwords.  Every wave holds the same kHamBlockQ queries (lane l: rows
// q0 + l + 64 j, j < kHamQPT, in VGPRs) and takes every kHamWaves-th train row of the staged tile, read
// from LDS at a wave-uniform address (a broadcast: no bank conflicts), so one ds_read_b128 feeds
// 4 dwords x kHamQPT queries of xor + popcount.  Top-2 per query as packed keys d << 18 | row
// (d <= 512, row < 2^18): min/max keep the two smallest keys, and key order is (distance, row) order,
// which is BFMatcher's tie rule (an equal distance never displaces an earlier row).
// CROSS (knn2_hamming_cross_kernel): every pair's distance also enters its train row's column key
// d << 18 | query row (0xFFFFFFFF for the zero-filled lanes past nq, which compute distances too and must
// never win): the lane's minimum over its kHamQPT queries, the wave's over its lanes, one entry of
// colrow[] per tile row (a tile row belongs to one wave), and after the tile an atomicMin into
// colmin[train row].  Unsigned min is commutative and associative, so colmin does not depend on blocks,
// splits or order, and key order is (distance, query row) order: colmin[j] & 0x3FFFF is the lowest query
// row at the least distance from train row j.
template <int W, bool CROSS>
__device__ __forceinline__ void ham_work(const HamWork& w, uint32_t* lds, uint32_t* colrow = nullptr,
                                         uint32_t* colmin = nullptr) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    uint32_t q[kHamQPT][W];
#pragma unroll
    for (int j = 0; j < kHamQPT; ++j) {
        const int qi = w.q0 + j * kWave + lane;
        const bool ok = qi < w.nq;
#pragma unroll
        for (int k = 0; k < W; k += 4) {
            const uint4 v = ok ? *reinterpret_cast<const uint4*>(w.q + (size_t)qi * W + k) : make_uint4(0, 0, 0, 0);
            q[j][k] = v.x; q[j][k + 1] = v.y; q[j][k + 2] = v.z; q[j][k + 3] = v.w;
        }
    }
    uint32_t k1[kHamQPT], k2[kHamQPT];
#pragma unroll
    for (int j = 0; j < kHamQPT; ++j) k1[j] = k2[j] = kHamNone;
    uint32_t qor[kHamQPT];  // CROSS: the low bits of a column key, all ones for a lane without a query
    if constexpr (CROSS) {
#pragma unroll
        for (int j = 0; j < kHamQPT; ++j) {
            const int qi = w.q0 + j * kWave + lane;
            qor[j] = qi < w.nq ? (uint32_t)qi : kHamNone;
        }
    }

    // train rows [r0, r1): r0 is a multiple of kHamTileRows, and the set's storage is zero rows up to
    // the next multiple past its last row, so a whole tile is always readable
    for (int r = w.r0; r < w.r1; r += kHamTileRows) {
        __syncthreads();
        if constexpr (CROSS) {  // the previous tile's column minima (all kHamTileRows rows: only the last tile is short)
            if (r > w.r0 && tid < kHamTileRows) atomicMin(colmin + r - kHamTileRows + tid, colrow[tid]);
        }
        const uint4* src = reinterpret_cast<const uint4*>(w.t + (size_t)r * W);
        for (int e = tid; e < kHamTileRows * W / 4; e += kHamThreads) reinterpret_cast<uint4*>(lds)[e] = src[e];
        __syncthreads();
        const int rows = min(kHamTileRows, w.r1 - r);
        for (int rr = wave; rr < rows; rr += kHamWaves) {
            uint32_t t[W];
#pragma unroll
            for (int k = 0; k < W; k += 4) {
                const uint4 v = *reinterpret_cast<const uint4*>(lds + rr * W + k);
                t[k] = v.x; t[k + 1] = v.y; t[k + 2] = v.z; t[k + 3] = v.w;
            }
            const uint32_t row = (uint32_t)(r + rr);
            uint32_t ck = kHamNone;
#pragma unroll
            for (int j = 0; j < kHamQPT; ++j) {
                uint32_t d = __popc(q[j][0] ^ t[0]);
#pragma unroll
                for (int k = 1; k < W; ++k) d = popc_add(q[j][k] ^ t[k], d);
                const uint32_t key = (d << 18) | row;
                k2[j] = min(k2[j], max(k1[j], key));
                k1[j] = min(k1[j], key);
                if constexpr (CROSS) ck = min(ck, (d << 18) | qor[j]);
            }
            if constexpr (CROSS) {
                ck = wave_min_u32(ck);
                if (lane == 0) colrow[rr] = ck;
            }
        }
    }

    // merge the waves' lists: slot s = 64 j + lane is query q0 + s
    __syncthreads();
    if constexpr (CROSS) {  // the last tile's column minima
        if (w.r1 > w.r0) {
            const int r = w.r0 + (w.r1 - w.r0 - 1) / kHamTileRows * kHamTileRows;
            if (tid < w.r1 - r) atomicMin(colmin + r + tid, colrow[tid]);
        }
    }
    uint2* mg = reinterpret_cast<uint2*>(lds);  // [wave][slot]
#pragma unroll
    for (int j = 0; j < kHamQPT; ++j) mg[wave * kHamBlockQ + j * kWave + lane] = make_uint2(k1[j], k2[j]);
    __syncthreads();
    for (int s = tid; s < kHamBlockQ; s += kHamThreads) {
        uint32_t a1 = kHamNone, a2 = kHamNone;
#pragma unroll
        for (int v = 0; v < kHamWaves; ++v) {
            const uint2 m = mg[v * kHamBlockQ + s];
            a2 = min(a2, max(a1, m.x));
            a1 = min(a1, m.x);
            a2 = min(a2, max(a1, m.y));
            a1 = min(a1, m.y);
        }
        const int qi = w.q0 + s;
        if (qi < w.nq) {
            Top2 o;
            o.k1 = a1 == kHamNone ? FLT_MAX : (float)(a1 >> 18);
            o.i1 = a1 == kHamNone ? INT_MAX : (int)(a1 & 0x3FFFFu);
            o.k2 = a2 == kHamNone ? FLT_MAX : (float)(a2 >> 18);
            o.i2 = a2 == kHamNone ? INT_MAX : (int)(a2 & 0x3FFFFu);
            w.out[qi] = o;
        }
    }
}

__global__ __launch_bounds__(kHamThreads) void knn2_hamming_kernel(const HamWork* __restrict__ works) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[kHamTileRows * 16];
    const HamWork w = works[blockIdx.x];
    if (w.wdw == 4) ham_work<4, false>(w, lds);  // block-uniform
    else if (w.wdw == 8) ham_work<8, false>(w, lds);
    else ham_work<16, false>(w, lds);
}

// The same sweep for cross-check batches: each pair's popcount is taken once and serves
// the query's top-2 and the train row's column minimum.
__global__ __launch_bounds__(kHamThreads) void knn2_hamming_cross_kernel(const HamCrossWork* __restrict__ works) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[kHamTileRows * 16];
    __shared__ uint32_t colrow[kHamTileRows];
    const HamWork w = works[blockIdx.x].w;
    uint32_t* colmin = works[blockIdx.x].colmin;
    if (w.wdw == 4) ham_work<4, true>(w, lds, colrow, colmin);  // block-uniform
    else if (w.wdw == 8) ham_work<8, true>(w, lds, colrow, colmin);
    else ham_work<16, true>(w, lds, colrow, colmin);
}

}  // namespace

void launch_knn_hamming(const HamWork* works, int n_works, hipStream_t st) {
    if (n_works > 0) knn2_hamming_kernel<<<n_works, kHamThreads, 0, st>>>(works);
}

// colmin: the batch's column minima, n_col entries over its fused problems, all ones before the sweep
void launch_knn_hamming_cross(const HamCrossWork* works, int n_works, uint32_t* colmin, long long n_col,
                              hipStream_t st) {
    if (n_col > 0) (void)hipMemsetAsync(colmin, 0xFF, sizeof(uint32_t) * n_col, st);
    if (n_works > 0) knn2_hamming_cross_kernel<<<n_works, kHamThreads, 0, st>>>(works);
}

}  // namespace mim
