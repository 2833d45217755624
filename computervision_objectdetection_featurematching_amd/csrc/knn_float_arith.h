// knn_float_arith.h — the squared L2 distance of float rows in OpenCV's order (core/src/norm.cpp normL2Sqr_,
// restated in oracle/mim_oracle.c l2sqr_sse_order), shared by knn_float.hip and knn_topk.hip: full rounds of
// 16 floats into 16 independent accumulators (acc = d * d + acc, the product and the sum rounded
// separately), the reduction ((a0+a1)+a2)+a3 per lane and (s0+s2)+(s1+s3) across lanes, then the dim % 16
// tail elements one by one.  Files that include this are compiled with fp contraction off, so no product
// is fused into a sum.  Two neighbouring accumulators form one float2: the subtraction, the product and the
// sum are packed fp32 operations with IEEE rounding per element (v_pk_add_f32 / v_pk_mul_f32).
#pragma once
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

namespace mim {

namespace {

typedef float f2 __attribute__((ext_vector_type(2)));

// MIM_FLT_PACKED=0 (with -fno-slp-vectorize): the same arithmetic as scalar fp32 instructions, the build
// that DESIGN.md §14 measures the packed one against
#ifndef MIM_FLT_PACKED
#define MIM_FLT_PACKED 1
#endif

// one round: 16 floats of the query (q[0..3]) against 16 of a train row (t[0..3], LDS, wave-uniform)
// acc[2 v + h] holds lanes 2h, 2h + 1 of accumulator v
__device__ __forceinline__ void flt_round(f2 (&acc)[8], const float4* q, const float4* t) {
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        const float4 tv = t[v], qv = q[v];
#if MIM_FLT_PACKED
        const f2 d0 = f2{qv.x, qv.y} - f2{tv.x, tv.y};
        const f2 d1 = f2{qv.z, qv.w} - f2{tv.z, tv.w};
        acc[2 * v] = d0 * d0 + acc[2 * v];
        acc[2 * v + 1] = d1 * d1 + acc[2 * v + 1];
#else
        const float e0 = qv.x - tv.x, e1 = qv.y - tv.y, e2 = qv.z - tv.z, e3 = qv.w - tv.w;
        acc[2 * v].x = e0 * e0 + acc[2 * v].x;
        acc[2 * v].y = e1 * e1 + acc[2 * v].y;
        acc[2 * v + 1].x = e2 * e2 + acc[2 * v + 1].x;
        acc[2 * v + 1].y = e3 * e3 + acc[2 * v + 1].y;
#endif
    }
}

__device__ __forceinline__ float flt_reduce(const f2 (&acc)[8]) {
    const f2 s01 = ((acc[0] + acc[2]) + acc[4]) + acc[6];  // s0, s1
    const f2 s23 = ((acc[1] + acc[3]) + acc[5]) + acc[7];  // s2, s3
    const f2 t = s01 + s23;                                // s0 + s2, s1 + s3
    return t.x + t.y;
}

// four tail elements, one by one
__device__ __forceinline__ float flt_tail4(float d, const float4 qv, const float4 tv) {
    float e = qv.x - tv.x;
    d = d + e * e;
    e = qv.y - tv.y;
    d = d + e * e;
    e = qv.z - tv.z;
    d = d + e * e;
    e = qv.w - tv.w;
    d = d + e * e;
    return d;
}

// train rows per staged tile at a row stride of dp floats: divides kFltRowPad, a multiple of kFltR
__device__ __forceinline__ int flt_tile_rows(int dp) { return dp <= 128 ? 64 : dp <= 256 ? 32 : 16; }

}  // namespace

}  // namespace mim
