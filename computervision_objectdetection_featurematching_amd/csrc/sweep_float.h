// sweep_float.h — the float sweep of one work item, written once: the squared L2 distance of
// every pair of the item's queries and train rows [r0, r1) in OpenCV's order (knn_float_arith.h), handed to a
// sink.  The top-k kernel (knn_topk.hip) and the radius kernel (radius.hip) are this sweep under their sinks;
// knn_float.hip's k = 2 kernel keeps its own loop (padded storage, no nt, no vec) and takes the constants.
//
// One query per lane, kFltBlockQ to a block; a tile of train rows is staged in LDS and read at wave-uniform
// addresses.  dim = dp a multiple of 16 up to 128: the query row lives in 16 NR VGPRs, one train row at a time
// (resident).  Any other dim (generic float sets only: their rows are 16-byte aligned): kFltR train rows'
// accumulators are carried through the rounds and the query's floats are streamed from memory once per kFltR
// rows.  A lane meets its rows in ascending order.  gfx950, wave64.
#pragma once
#include <hip/hip_runtime.h>

#include "knn_float_arith.h"  // flt_round, flt_reduce, flt_tail4, flt_tile_rows; fp contraction off
#include "mim_internal.h"

namespace mim {

namespace {

constexpr int kFltThreads = 256;     // 4 waves, a query per lane
constexpr int kFltLdsFloats = 8192;  // 32 KiB train tile
constexpr int kFltR = 4;             // train rows in flight on the streamed path
static_assert(kFltThreads == kFltBlockQ, "one query per thread");
static_assert(kFltRowPad * 128 <= kFltLdsFloats && 16 * kFltMaxDim <= kFltLdsFloats, "tile fits the LDS");

// tile [r, r + TR) of the train rows into LDS; rows from nt on are not read (the f32 rows of a 128-D set
// end there) and are staged as zeros
__device__ __forceinline__ void flt_sweep_stage(const FltSweepWork& w, int r, int TR, float* lds) {
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

template <int NR, class Sink>
__device__ __forceinline__ void flt_sweep_resident(const FltSweepWork& w, float* lds, Sink& sink) {
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
    const float4* lds4 = reinterpret_cast<const float4*>(lds);
    for (int r = w.r0; r < w.r1; r += TR) {
        __syncthreads();
        flt_sweep_stage(w, r, TR, lds);
        __syncthreads();
        const int rows = min(TR, w.r1 - r);
        for (int rr = 0; rr < rows; ++rr) {
            f2 acc[8];
#pragma unroll
            for (int v = 0; v < 8; ++v) acc[v] = f2{0.f, 0.f};
            const float4* t = lds4 + rr * DP4;
#pragma unroll
            for (int c = 0; c < NR; ++c) flt_round(acc, q + 4 * c, t + 4 * c);
            sink.pair(flt_reduce(acc), r + rr);
        }
    }
    sink.finish();
}

template <class Sink>
__device__ __forceinline__ void flt_sweep_streamed(const FltSweepWork& w, float* lds, Sink& sink) {
    const int dp4 = w.dp >> 2, rounds = w.dim >> 4;
    const int TR = flt_tile_rows(w.dp);
    const int qi = w.q0 + (int)threadIdx.x;
    const float4* qrow = reinterpret_cast<const float4*>(w.q + (size_t)min(qi, w.nq - 1) * w.dp);
    const float4* lds4 = reinterpret_cast<const float4*>(lds);
    for (int r = w.r0; r < w.r1; r += TR) {
        __syncthreads();
        flt_sweep_stage(w, r, TR, lds);
        __syncthreads();
        const int rows = min(TR, w.r1 - r);
        for (int rr = 0; rr < rows; rr += kFltR) {  // rr + j < TR: rows past `rows` are computed, not passed on
            f2 acc[kFltR][8];
#pragma unroll
            for (int j = 0; j < kFltR; ++j)
#pragma unroll
                for (int v = 0; v < 8; ++v) acc[j][v] = f2{0.f, 0.f};
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
                if (rr + j < rows) sink.pair(d[j], r + rr + j);
        }
    }
    sink.finish();
}

// The work item of one block.  The sink is the lane's: sink.pair(d2, row) once per train row of [r0, r1), rows
// ascending, d2 the squared distance of the lane's query w.q0 + threadIdx.x (of row nq - 1 where that lies
// past the set: the sink leaves such a lane's results out); sink.finish() once after the last pair.  Neither is
// called for a 128-D item whose sets are both integer-valued: an i8 MFMA kernel owns those pairs.
// lds: kFltLdsFloats floats.
template <class Sink>
__device__ __forceinline__ void flt_sweep(const FltSweepWork& w, float* lds, Sink& sink) {
    if (w.qflags && !(*w.qflags | *w.tflags)) return;          // block-uniform
    if ((w.dim & 15) == 0 && w.dim <= 128 && w.dp == w.dim) {  // block-uniform
        switch (w.dim >> 4) {
            case 1: flt_sweep_resident<1>(w, lds, sink); break;
            case 2: flt_sweep_resident<2>(w, lds, sink); break;
            case 3: flt_sweep_resident<3>(w, lds, sink); break;
            case 4: flt_sweep_resident<4>(w, lds, sink); break;
            case 5: flt_sweep_resident<5>(w, lds, sink); break;
            case 6: flt_sweep_resident<6>(w, lds, sink); break;
            case 7: flt_sweep_resident<7>(w, lds, sink); break;
            default: flt_sweep_resident<8>(w, lds, sink); break;
        }
    } else {
        flt_sweep_streamed(w, lds, sink);
    }
}

}  // namespace

}  // namespace mim
