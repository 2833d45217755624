// sweep_hamming.h — the Hamming sweep of one work item, written once: every pair of the item's
// queries and train rows [r0, r1), its distance handed to a sink.  The top-k kernel (knn_topk.hip) and the
// radius kernel (radius.hip) are this sweep under their sinks; hamming.hip's k = 2 kernels keep their own loop
// (the fused cross variant) and take popc_add from here.
//
// A block of kHamThreads threads holds the item's kHamBlockQ queries QPT to a lane: kHamBlockQ / (64 QPT)
// query groups, WPG waves to a group.  A tile of kHamTileRows train rows is staged in LDS and read at
// wave-uniform addresses (a broadcast: no bank conflicts); wave `ph` of a group takes rows ph, ph + WPG, ...
// of the tile, so a lane meets the rows of its share in ascending order.  gfx950, wave64.
#pragma once
#include <hip/hip_runtime.h>

#include "mim_internal.h"

namespace mim {

namespace {

constexpr int kHamThreads = 256;  // 4 waves
constexpr int kHamWaves = kHamThreads / kWave;

// popcount(x) + acc as the one instruction it is (left to the compiler, the sums are reassociated into
// popcounts plus separate three-operand adds: 23 instead of 20 VALU instructions per pair at 32 bytes)
__device__ __forceinline__ uint32_t popc_add(uint32_t x, uint32_t acc) {
    uint32_t r;
    asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(acc));
    return r;
}

// sink(j, d, row): the distance d of the lane's j-th query (row w.q0 + slot0 + 64 j of the query set, slot0 =
// (wave / WPG) 64 QPT + lane; it may lie past nq, its words are zeros then) to train row `row`.  lds: at least
// kHamTileRows * 16 dwords; a caller that reuses them afterwards puts a barrier first (the last tile's reads).
template <int W, int QPT, int WPG, class Sink>
__device__ __forceinline__ void ham_sweep(const HamSweepWork& w, uint32_t* lds, Sink&& sink) {
    constexpr int GROUPS = kHamBlockQ / (QPT * kWave);
    static_assert(GROUPS * WPG == kHamWaves && GROUPS * QPT * kWave == kHamBlockQ, "waves tile the block's queries");
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = wave / WPG, ph = wave % WPG;
    const int slot0 = grp * QPT * kWave + lane;
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
#pragma unroll
            for (int j = 0; j < QPT; ++j) {
                uint32_t d = __popc(q[j][0] ^ t[0]);
#pragma unroll
                for (int c = 1; c < W; ++c) d = popc_add(q[j][c] ^ t[c], d);
                sink(j, d, r + rr);
            }
        }
    }
}

}  // namespace

}  // namespace mim
