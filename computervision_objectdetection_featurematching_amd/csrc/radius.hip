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
// Hamming: the sweep of ham_work (hamming.hip), the compare d <= floor(r) in place of the top-2 upkeep.
// Float: flt_resident / flt_streamed of knn_float.hip with the arithmetic of knn_float_arith.h; the literal test
//   sqrtf(d2) <= r is the compare d2 <= T with T the largest float whose sqrtf is <= r (radius_flt_threshold:
//   sqrtf is monotone), which spares the count pass the sqrt sequence, about a tenth of a 128-D pair.
// i8 MFMA (128-D sets whose flags say integer-valued on both sides): the fragment tiles and norm blocks of
//   prep_batch_kernel (knn.hip).  A wave keeps the q' fragments of two 32-query column tiles in VGPRs and takes
//   the train tiles 64 rows at a time, 16 v_mfma_i32_32x32x32_i8 per tile, accumulators seeded with floor(n2/2):
//   R = q'.t'' + floor(n2/2), d^2 = 2R + (n2 & 1) + c(q).  sqrtf((float)d^2) <= r is d^2 <= T2
//   (radius_int_threshold), per query 2R + p <= tau = T2 - c(q); every accumulator is filtered against
//   floor(tau / 2) (2R + p <= tau implies R <= floor(tau / 2)), one min3 chain per 16 values, and only a
//   wave with a hit reads the parities and decides exactly.  Train fragments are staged by LDS-DMA.
// gfx950, wave64.
#include <hip/hip_runtime.h>

#include <climits>

#include "knn_float_arith.h"  // flt_round, flt_reduce, flt_tail4, flt_tile_rows; fp contraction off
#include "radius.h"

namespace mim {

namespace {

typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(16))) int i32x16;
typedef const __attribute__((address_space(1))) i32x4 gi32x4;  // global (not flat) loads
typedef const __attribute__((address_space(1))) int gint;

// the fill pass's write of one match of query gq (numbered over the call)
__device__ __forceinline__ void rad_emit(const RadArgs& a, long long gq, float d, int row) {
    const int slot = atomicAdd(a.cursor + gq, 1);
    const long long pos = a.offsets[gq] + slot;
    if (pos < a.offsets[gq + 1]) a.keys[pos] = radius_key(d, row);
}

// ---------------------------------------------------------------------------------------------------
// Hamming
// ---------------------------------------------------------------------------------------------------
constexpr int kHamThreads = 256;  // 4 waves: each holds the block's 256 queries, 4 per lane, and takes every 4th row
constexpr int kHamWaves = kHamThreads / kWave;
constexpr int kHamQpt = kHamBlockQ / kWave;

// popcount(x) + acc as the one instruction it is (hamming.hip popc_add)
__device__ __forceinline__ uint32_t popc_add(uint32_t x, uint32_t acc) {
    uint32_t r;
    asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(acc));
    return r;
}

template <int W, bool kFill>
__device__ __forceinline__ void rad_ham_work(const RadHamWork& w, const RadArgs& a, uint32_t* lds) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t T = (uint32_t)a.ham_t;  // >= 0: the entries accept only r > FLT_EPSILON
    uint32_t q[kHamQpt][W];
    int cnt[kHamQpt];
#pragma unroll
    for (int j = 0; j < kHamQpt; ++j) {
        const int qi = w.q0 + lane + j * kWave;
        const bool ok = qi < w.nq;
        cnt[j] = 0;
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
        for (int rr = wave; rr < rows; rr += kHamWaves) {
            uint32_t t[W];
#pragma unroll
            for (int c = 0; c < W; c += 4) {
                const uint4 v = *reinterpret_cast<const uint4*>(lds + rr * W + c);
                t[c] = v.x; t[c + 1] = v.y; t[c + 2] = v.z; t[c + 3] = v.w;
            }
#pragma unroll
            for (int j = 0; j < kHamQpt; ++j) {
                uint32_t d = __popc(q[j][0] ^ t[0]);
#pragma unroll
                for (int c = 1; c < W; ++c) d = popc_add(q[j][c] ^ t[c], d);
                const int qi = w.q0 + lane + j * kWave;
                const bool hit = d <= T && qi < w.nq;
                if (kFill) {
                    if (hit) rad_emit(a, w.qoff + qi, (float)d, r + rr);
                } else {
                    cnt[j] += hit;
                }
            }
        }
    }
    if (!kFill) {
#pragma unroll
        for (int j = 0; j < kHamQpt; ++j) {
            const int qi = w.q0 + lane + j * kWave;
            if (qi < w.nq && cnt[j] != 0) atomicAdd(a.counts + w.qoff + qi, cnt[j]);
        }
    }
}

template <bool kFill>
__global__ __launch_bounds__(kHamThreads) void radius_hamming_kernel(const RadHamWork* __restrict__ works, RadArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[kHamTileRows * 16];
    const RadHamWork w = works[blockIdx.x];
    if (w.wdw == 4) rad_ham_work<4, kFill>(w, a, lds);  // block-uniform
    else if (w.wdw == 8) rad_ham_work<8, kFill>(w, a, lds);
    else rad_ham_work<16, kFill>(w, a, lds);
}

// ---------------------------------------------------------------------------------------------------
// Float
// ---------------------------------------------------------------------------------------------------
constexpr int kFltThreads = 256;     // 4 waves, a query per lane
constexpr int kFltLdsFloats = 8192;  // 32 KiB train tile
constexpr int kFltR = 4;             // train rows in flight on the streamed path
static_assert(kFltThreads == kFltBlockQ, "one query per thread");
static_assert(kFltRowPad * 128 <= kFltLdsFloats && 16 * kFltMaxDim <= kFltLdsFloats, "tile fits the LDS");

// sqrtf(d2) <= r as d2 <= T (radius_flt_threshold: the same pairs, bit for bit; a NaN d2 never passes, +inf
// only r = +inf); the sqrt is taken for the matches the fill pass writes
template <bool kFill>
__device__ __forceinline__ void rad_flt_pair(const RadFltWork& w, const RadArgs& a, int qi, float d2, int row, int& cnt) {
    const bool hit = d2 <= a.flt_t && qi < w.nq;
    if (kFill) {
        if (hit) rad_emit(a, w.qoff + qi, sqrtf(d2), row);
    } else {
        cnt += hit;
    }
}

// tile [r, r + TR) of the train rows into LDS; rows from nt on are not read (the f32 rows of a 128-D set
// end there) and are staged as zeros
__device__ __forceinline__ void rad_flt_stage(const RadFltWork& w, int r, int TR, float* lds) {
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
template <int NR, bool kFill>
__device__ __forceinline__ void rad_flt_resident(const RadFltWork& w, const RadArgs& a, float* lds) {
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
    int cnt = 0;
    const float4* lds4 = reinterpret_cast<const float4*>(lds);
    for (int r = w.r0; r < w.r1; r += TR) {
        __syncthreads();
        rad_flt_stage(w, r, TR, lds);
        __syncthreads();
        const int rows = min(TR, w.r1 - r);
        for (int rr = 0; rr < rows; ++rr) {
            f2 acc[8];
#pragma unroll
            for (int v = 0; v < 8; ++v) acc[v] = f2{0.f, 0.f};
            const float4* t = lds4 + rr * DP4;
#pragma unroll
            for (int c = 0; c < NR; ++c) flt_round(acc, q + 4 * c, t + 4 * c);
            rad_flt_pair<kFill>(w, a, qi, flt_reduce(acc), r + rr, cnt);
        }
    }
    if (!kFill && qi < w.nq && cnt != 0) atomicAdd(a.counts + w.qoff + qi, cnt);
}

// any dim (generic float sets only: their rows are 16-byte aligned): flt_streamed
template <bool kFill>
__device__ __forceinline__ void rad_flt_streamed(const RadFltWork& w, const RadArgs& a, float* lds) {
    const int dp4 = w.dp >> 2, rounds = w.dim >> 4;
    const int TR = flt_tile_rows(w.dp);
    const int qi = w.q0 + (int)threadIdx.x;
    const float4* qrow = reinterpret_cast<const float4*>(w.q + (size_t)min(qi, w.nq - 1) * w.dp);
    int cnt = 0;
    const float4* lds4 = reinterpret_cast<const float4*>(lds);
    for (int r = w.r0; r < w.r1; r += TR) {
        __syncthreads();
        rad_flt_stage(w, r, TR, lds);
        __syncthreads();
        const int rows = min(TR, w.r1 - r);
        for (int rr = 0; rr < rows; rr += kFltR) {  // rr + j < TR: rows past `rows` are computed, not tested
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
                if (rr + j < rows) rad_flt_pair<kFill>(w, a, qi, d[j], r + rr + j, cnt);
        }
    }
    if (!kFill && qi < w.nq && cnt != 0) atomicAdd(a.counts + w.qoff + qi, cnt);
}

template <bool kFill>
__global__ __launch_bounds__(kFltThreads) void radius_float_kernel(const RadFltWork* __restrict__ works, RadArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[kFltLdsFloats];
    const RadFltWork w = works[blockIdx.x];
    // 128-D sets that are integer-valued on both sides: the MFMA kernel's (block-uniform, as knn2_f32_kernel)
    if (w.qflags && !(*w.qflags | *w.tflags)) return;
    if ((w.dim & 15) == 0 && w.dim <= 128 && w.dp == w.dim) {  // block-uniform
        switch (w.dim >> 4) {
            case 1: rad_flt_resident<1, kFill>(w, a, lds); break;
            case 2: rad_flt_resident<2, kFill>(w, a, lds); break;
            case 3: rad_flt_resident<3, kFill>(w, a, lds); break;
            case 4: rad_flt_resident<4, kFill>(w, a, lds); break;
            case 5: rad_flt_resident<5, kFill>(w, a, lds); break;
            case 6: rad_flt_resident<6, kFill>(w, a, lds); break;
            case 7: rad_flt_resident<7, kFill>(w, a, lds); break;
            default: rad_flt_resident<8, kFill>(w, a, lds); break;
        }
    } else {
        rad_flt_streamed<kFill>(w, a, lds);
    }
}

// ---------------------------------------------------------------------------------------------------
// i8 MFMA.  Block = kKnnWaves waves = kKnnBlockQ queries, a wave = kKnnQT 32-query column tiles (the
// KnnWork unit of knn_schedule_static: block b runs works[seg_start[b] .. seg_start[b + 1])).
// Train fragments stream HBM -> LDS by LDS-DMA (global_load_lds_dwordx4, as knn2_i8_kernel's stage_dma) in
// stages of kI8Stage 64-row tiles, double buffered, one barrier per stage: one wave-instruction writes 64
// lanes x 16 contiguous bytes at a wave-uniform LDS base, which a fragment of the fragment-major tile already
// is; the train half of the tile's norm block (floor(n2/2), the parity mask) follows it as two 256-byte pieces.
// A wave then reads a half tile's four fragments as conflict-free ds_read_b128 and its seeds and parity word
// from the same stage: the sweep's only vector-memory operations are the DMA, so nothing in it waits for one
// but the stage's end.  A wave whose queries all lie past the set (the last block of a problem) still stages
// and waits at the barriers, and computes nothing.
// Accumulator g of lane (h = lane >> 5, r = lane & 31) of a 32-row half tile is train row
// (g & 3) + 8 (g >> 2) + 4 h against query column r (the layout block_mfma of knn.hip reads its seeds by).
// ---------------------------------------------------------------------------------------------------
constexpr int kI8Threads = 64 * kKnnWaves;
constexpr int kI8Stage = 2;                      // 64-row train tiles per LDS stage (per barrier)
constexpr int kI8Frags = kTileBytes / 1024;      // 1 KiB wave loads per tile
constexpr int kI8LdsTile = kTileBytes + 512;     // fragments + the train half of the norm block
static_assert((kI8Stage * kI8Frags) % kKnnWaves == 0, "the waves share a stage's fragments evenly");

template <bool kFill>
__global__ __launch_bounds__(kI8Threads) void radius_i8_kernel(const RadI8Prob* __restrict__ probs,
                                                               const KnnWork* __restrict__ works,
                                                               const int* __restrict__ seg_start, RadArgs a) {
    constexpr int QT = kKnnQT;
    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * kI8Stage * kI8LdsTile];
    const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, r = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int si_end = seg_start[blockIdx.x + 1];
    for (int si = seg_start[blockIdx.x]; si < si_end; ++si) {
        const KnnWork w = works[si];
        const RadI8Prob* P = probs + w.problem;
        if (*P->q.flags | *P->t.flags) continue;  // not integer-valued: the float kernel's (block-uniform)
        if (w.tile0 >= w.tile1) continue;         // an empty split of the schedule (block-uniform)
        const int nq = P->q.n, nt = P->t.n;
        const int qbase = w.q0 + wave * 32 * QT;
        const bool active = qbase < nq;  // wave-uniform
        const uint4* tsrc = reinterpret_cast<const uint4*>(P->t.frag);
        const int* tnorm = P->t.norm;

        // query fragments q' = ~t'' and tau = T2 - c(q) of the lane's column in each column tile.  c(q) =
        // |q - 128|^2 + 2 sum(q - 128) lies within +-2^22 and T2 in [-1, 2^23): tau cannot leave int32.
        // A column past the set gets the least tau: nothing passes, and `valid` bounds it explicitly.
        i32x4 B[QT][4];
        int tau[QT], hf[QT], cq[QT], cnt[QT];
        bool valid[QT];
#pragma unroll
        for (int u = 0; u < QT; ++u) {
            const int qr = qbase + 32 * u, qt = qr >> 6, qh = (qr >> 5) & 1;
            const int qtc = qt < P->q.n_tiles ? qt : 0;  // tiles past the set: tile 0's, never counted
            const gi32x4* qsrc = (const gi32x4*)(P->q.frag) + (size_t)qtc * 512;
#pragma unroll
            for (int s = 0; s < 4; ++s) B[u][s] = ~qsrc[(qh * 4 + s) * 64 + lane];
            const int q = qr + r;
            valid[u] = q < nq;
            cq[u] = valid[u] ? ((const gint*)P->q.norm)[(size_t)(q >> 6) * kNormWords + 128 + (q & 63)] : 0;
            tau[u] = valid[u] ? a.int_t2 - cq[u] : INT_MIN;
            hf[u] = tau[u] >> 1;  // floor(tau / 2)
            cnt[u] = 0;
        }

        // tiles [t0, t0 + kI8Stage) below tile1 into buffer buf; fragment f of the stage is wave f % kKnnWaves'
        auto stage_dma = [&](int t0, int buf) {
#pragma unroll
            for (int f = wave; f < kI8Stage * kI8Frags; f += kKnnWaves) {
                const int tt = f / kI8Frags, fr = f % kI8Frags;
                if (t0 + tt < w.tile1)
                    __builtin_amdgcn_global_load_lds((const void*)(tsrc + (size_t)(t0 + tt) * 512 + fr * 64 + lane),
                                                     (__attribute__((address_space(3))) void*)(smem + (buf * kI8Stage + tt) * kI8LdsTile + fr * 1024),
                                                     16, 0, 0);
            }
#pragma unroll
            for (int p = wave; p < 2 * kI8Stage; p += kKnnWaves) {  // piece p: tile p >> 1, norm words 64 (p & 1) ..
                const int tt = p >> 1;
                if (t0 + tt < w.tile1)
                    __builtin_amdgcn_global_load_lds((const void*)(tnorm + (size_t)(t0 + tt) * kNormWords + 64 * (p & 1) + lane),
                                                     (__attribute__((address_space(3))) void*)(smem + (buf * kI8Stage + tt) * kI8LdsTile + kTileBytes + 256 * (p & 1)),
                                                     4, 0, 0);
            }
        };
        // (the previous work item's last LDS read lies before its last barrier)
        stage_dma(w.tile0, 0);
        __builtin_amdgcn_s_waitcnt(0);  // the prologue loads, q' fragments included
        __syncthreads();

        for (int st = w.tile0; st < w.tile1; st += kI8Stage) {
            const int buf = ((st - w.tile0) / kI8Stage) & 1;
            if (st + kI8Stage < w.tile1) stage_dma(st + kI8Stage, buf ^ 1);
            const int ht_end = active ? 2 * min(st + kI8Stage, w.tile1) : 0;
            for (int ht = 2 * st; ht < ht_end; ++ht) {  // 32-row half tiles
                const int tile = ht >> 1, u2 = ht & 1, row0 = 32 * ht;
                const unsigned char* tb = smem + (buf * kI8Stage + (tile - st)) * kI8LdsTile;
                const i32x4* A = reinterpret_cast<const i32x4*>(tb);
                const int* tn = reinterpret_cast<const int*>(tb + kTileBytes);
                // bit (g & 3) + 8 (g >> 2): n2 & 1 of the lane's row g
                const unsigned pw = (unsigned)tn[64 + u2] >> (4 * h);
                i32x16 acc[QT];
#pragma unroll
                for (int gg = 0; gg < 4; ++gg) {
                    const i32x4 n = *reinterpret_cast<const i32x4*>(tn + 32 * u2 + 4 * h + 8 * gg);
                    acc[0][4 * gg + 0] = n.x; acc[0][4 * gg + 1] = n.y; acc[0][4 * gg + 2] = n.z; acc[0][4 * gg + 3] = n.w;
                }
#pragma unroll
                for (int u = 1; u < QT; ++u) acc[u] = acc[0];
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const i32x4 av = A[(u2 * 4 + s) * 64 + lane];
#pragma unroll
                    for (int u = 0; u < QT; ++u) acc[u] = __builtin_amdgcn_mfma_i32_32x32x32_i8(av, B[u][s], acc[u], 0, 0, 0);
                }
#pragma unroll
                for (int u = 0; u < QT; ++u) {
                    const i32x16& p = acc[u];
                    int m = min(min(p[0], p[1]), p[2]);
#pragma unroll
                    for (int g = 3; g < 15; g += 2) m = min(min(m, p[g]), p[g + 1]);
                    m = min(m, p[15]);
                    // a padded train row's R is 2^30 - 1 + q'.t'': never under a floor(tau / 2) below 2^23
                    if (__builtin_amdgcn_ballot_w64(m <= hf[u]) == 0) continue;
                    // the rows some lane has under its filter (independent compares into SGPR pairs), then a
                    // scalar test per row: at 8 matches per query one row in five has a hit somewhere in the wave
                    unsigned long long hm[16];
#pragma unroll
                    for (int g = 0; g < 16; ++g) hm[g] = __builtin_amdgcn_ballot_w64(p[g] <= hf[u]);
#pragma unroll
                    for (int g = 0; g < 16; ++g) {
                        if (hm[g] == 0) continue;
                        const int pos = (g & 3) + 8 * (g >> 2), row = row0 + pos + 4 * h;
                        // 2R + p without signed overflow (a padded row's wraps and is cut by row < nt)
                        const int D = (int)(((unsigned)p[g] << 1) | ((pw >> pos) & 1u));
                        const bool hit = D <= tau[u] && row < nt && valid[u];
                        if (kFill) {
                            if (hit) rad_emit(a, P->qoff + qbase + 32 * u + r, sqrtf((float)(D + cq[u])), row);
                        } else {
                            cnt[u] += hit;
                        }
                    }
                }
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's DMA into the next buffer landed
            __syncthreads();
        }
        if (!kFill) {
#pragma unroll
            for (int u = 0; u < QT; ++u) {
                const int c = cnt[u] + __shfl_xor(cnt[u], 32);  // the two halves hold disjoint rows of one query
                if (h == 0 && valid[u] && c != 0) atomicAdd(a.counts + P->qoff + qbase + 32 * u + r, c);
            }
        }
    }
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
