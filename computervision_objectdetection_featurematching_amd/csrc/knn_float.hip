// knn_float.hip — brute-force 2-NN over float descriptors of any dimension 1..512
// (BFMatcher(NORM_L2).knnMatch, k = 2, on the rows of mim_set_create_f32).
//
// The squared distance of a pair is computed in OpenCV's order (core/src/norm.cpp normL2Sqr_, restated
// in oracle/mim_oracle.c l2sqr_sse_order): full rounds of 16 floats into 16 independent accumulators
// (acc = d * d + acc, the product and the sum rounded separately), the reduction ((a0+a1)+a2)+a3 per
// lane and (s0+s2)+(s1+s3) across lanes, then the dim % 16 tail elements one by one; the distance is
// sqrtf of that.  This file is compiled with fp contraction off, so no product is fused into a sum.
// Two neighbouring accumulators form one float2: the subtraction, the product and the sum are packed
// fp32 operations with IEEE rounding per element (v_pk_add_f32 / v_pk_mul_f32), 1.5 VALU instructions
// per element.
//
// Layout: one query per lane, 256 queries per block; a tile of train rows is staged in LDS and every
// wave reads it at wave-uniform addresses (ds_read_b128 broadcasts, no bank conflicts).
//   dim a multiple of 16 up to 128: the query row lives in VGPRs (templated on the round count);
//   any other dim: the 16 accumulators of kFltR train rows are carried through the rounds and the
//   query's floats are streamed from memory once per kFltR rows.
// Top-2: OpenCV inserts on the sqrt values with a strict <, so an equal distance keeps the lower row.
// The sqrt is taken only when d^2 <= m2sq, the d^2 that produced the current second best (d^2 > m2sq
// implies sqrtf(d^2) >= k2: not inserted); ranking on d^2 alone would be wrong, since distinct d^2
// share a sqrtf.  Output: the same Top2 partials [split][q_pad] that ratio_compact_kernel /
// knn_emit_kernel (knn.hip) merge; sentinels FLT_MAX / INT_MAX.  gfx950, wave64.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>

#include "mim_internal.h"
#include "sweep_float.h"  // kFltThreads, kFltLdsFloats, kFltR; the arithmetic of knn_float_arith.h, fp contraction off

namespace mim {

namespace {

struct FltTop {
    float k1, k2;      // the two smallest distances (sqrt values)
    float m1sq, m2sq;  // the d^2 they came from
    int i1, i2;
};

__device__ __forceinline__ FltTop flt_top_init() {
    return FltTop{FLT_MAX, FLT_MAX, __builtin_inff(), __builtin_inff(), INT_MAX, INT_MAX};
}

// rows arrive in ascending order, so the strict compares are OpenCV's tie rule; +inf (an overflowed
// d^2) is never below FLT_MAX and is not inserted.  The outer test is wave-wide (a scalar branch): left
// per lane, the compiler turns the whole insertion, sqrt included, into selects that every pair pays.
__device__ __forceinline__ void flt_insert(FltTop& s, float d2, int row) {
    const bool cand = d2 <= s.m2sq;
    if (__builtin_amdgcn_ballot_w64(cand) == 0) return;
    if (cand) {
        const float d = sqrtf(d2);
        if (d < s.k2) {
            if (d < s.k1) {
                s.k2 = s.k1; s.i2 = s.i1; s.m2sq = s.m1sq;
                s.k1 = d; s.i1 = row; s.m1sq = d2;
            } else {
                s.k2 = d; s.i2 = row; s.m2sq = d2;
            }
        }
    }
}

// whole tile [r, r + tile rows) of the train set into LDS: the set's storage has zero rows up to the
// next multiple of kFltRowPad, and r0 is such a multiple, so every tile is readable without a test
__device__ __forceinline__ void flt_stage(const FltWork& w, int r, int n4, float4* lds4) {
    const float4* src = reinterpret_cast<const float4*>(w.t + (size_t)r * w.dp);
    for (int e = threadIdx.x; e < n4; e += kFltThreads) lds4[e] = src[e];
}

__device__ __forceinline__ void flt_store(const FltWork& w, int qi, const FltTop& s) {
    if (qi < w.nq) w.out[qi] = Top2{s.k1, s.i1, s.k2, s.i2};
}

// dim = 16 NR <= 128: the query row in 16 NR VGPRs, one train row at a time (two rows in flight
// spill: the 128-float query leaves no room for a second set of operands at two waves per SIMD)
template <int NR>
__device__ __forceinline__ void flt_resident(const FltWork& w, float4* lds4) {
    constexpr int DP4 = 4 * NR, TR = 64;
    const int qi = w.q0 + (int)threadIdx.x;
    const float4* qrow = reinterpret_cast<const float4*>(w.q + (size_t)min(qi, w.nq - 1) * (DP4 * 4));
    float4 q[DP4];
#pragma unroll
    for (int k = 0; k < DP4; ++k) q[k] = qrow[k];
    FltTop s = flt_top_init();
    for (int r = w.r0; r < w.r1; r += TR) {
        __syncthreads();
        flt_stage(w, r, TR * DP4, lds4);
        __syncthreads();
        const int rows = min(TR, w.r1 - r);
        for (int rr = 0; rr < rows; ++rr) {
            f2 acc[8];
#pragma unroll
            for (int a = 0; a < 8; ++a) acc[a] = f2{0.f, 0.f};
            const float4* t = lds4 + rr * DP4;
#pragma unroll
            for (int k = 0; k < NR; ++k) flt_round(acc, q + 4 * k, t + 4 * k);
            flt_insert(s, flt_reduce(acc), r + rr);
        }
    }
    flt_store(w, qi, s);
}

// any dim: kFltR train rows' accumulators carried through the rounds in order, the query's floats
// streamed from memory once per kFltR rows; then the tail (dp - 16 rounds floats, the zero fill
// included: 0 * 0 added to a non-negative sum changes nothing)
__device__ __forceinline__ void flt_streamed(const FltWork& w, float4* lds4) {
    const int dp4 = w.dp >> 2, rounds = w.dim >> 4;
    const int TR = flt_tile_rows(w.dp);
    const int qi = w.q0 + (int)threadIdx.x;
    const float4* qrow = reinterpret_cast<const float4*>(w.q + (size_t)min(qi, w.nq - 1) * w.dp);
    FltTop s = flt_top_init();
    for (int r = w.r0; r < w.r1; r += TR) {
        __syncthreads();
        flt_stage(w, r, TR * dp4, lds4);
        __syncthreads();
        const int rows = min(TR, w.r1 - r);
        for (int rr = 0; rr < rows; rr += kFltR) {  // rr + j < TR: rows past `rows` are computed, not inserted
            f2 acc[kFltR][8];
#pragma unroll
            for (int j = 0; j < kFltR; ++j)
#pragma unroll
                for (int a = 0; a < 8; ++a) acc[j][a] = f2{0.f, 0.f};
            const float4* t = lds4 + rr * dp4;
            for (int k = 0; k < rounds; ++k) {
                float4 qv[4];
#pragma unroll
                for (int v = 0; v < 4; ++v) qv[v] = qrow[4 * k + v];
#pragma unroll
                for (int j = 0; j < kFltR; ++j) flt_round(acc[j], qv, t + j * dp4 + 4 * k);
            }
            float d[kFltR];
#pragma unroll
            for (int j = 0; j < kFltR; ++j) d[j] = flt_reduce(acc[j]);  // all zero without a full round
            for (int k4 = 4 * rounds; k4 < dp4; ++k4) {
                const float4 qv = qrow[k4];
#pragma unroll
                for (int j = 0; j < kFltR; ++j) d[j] = flt_tail4(d[j], qv, t[j * dp4 + k4]);
            }
#pragma unroll
            for (int j = 0; j < kFltR; ++j)
                if (rr + j < rows) flt_insert(s, d[j], r + rr + j);
        }
    }
    flt_store(w, qi, s);
}

__global__ __launch_bounds__(kFltThreads) void knn2_float_kernel(const FltWork* __restrict__ works) {
    __shared__ __attribute__((aligned(16))) float lds[kFltLdsFloats];
    const FltWork w = works[blockIdx.x];
    float4* lds4 = reinterpret_cast<float4*>(lds);
    if ((w.dim & 15) == 0 && w.dim <= 128) {  // block-uniform
        switch (w.dim >> 4) {
            case 1: flt_resident<1>(w, lds4); break;
            case 2: flt_resident<2>(w, lds4); break;
            case 3: flt_resident<3>(w, lds4); break;
            case 4: flt_resident<4>(w, lds4); break;
            case 5: flt_resident<5>(w, lds4); break;
            case 6: flt_resident<6>(w, lds4); break;
            case 7: flt_resident<7>(w, lds4); break;
            default: flt_resident<8>(w, lds4); break;
        }
    } else {
        flt_streamed(w, lds4);
    }
}

}  // namespace

void launch_knn_float(const FltWork* works, int n_works, hipStream_t st) {
    if (n_works > 0) knn2_float_kernel<<<n_works, kFltThreads, 0, st>>>(works);
}

}  // namespace mim
