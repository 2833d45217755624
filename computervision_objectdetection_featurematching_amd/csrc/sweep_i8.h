// sweep_i8.h — the i8 MFMA sweep over 128-D sets that are integer-valued on both sides, written once
// (DESIGN.md §19).  radius_i8_kernel (radius.hip) and knn_topk_i8_kernel (knn_coll.hip) are this frame under
// their rules; knn.hip's hand-scheduled knn2_i8_kernel is its own.
//
// Block = kKnnWaves waves = kKnnBlockQ queries, a wave = kKnnQT 32-query column tiles whose q' fragments stay
// in VGPRs (the KnnWork unit of knn_schedule_static: block b runs works[seg_start[b] .. seg_start[b + 1])).
// Train fragments (the fragment tiles and norm blocks of prep_batch_kernel, knn.hip) stream HBM -> LDS by
// LDS-DMA (global_load_lds_dwordx4) in stages of kI8Stage 64-row tiles, double buffered, one barrier per
// stage: one wave-instruction writes 64 lanes x 16 contiguous bytes at a wave-uniform LDS base, which a
// fragment of the fragment-major tile already is; the train half of the tile's norm block (floor(n2/2), the
// parity mask) follows it as two 256-byte pieces.  A wave then reads a half tile's four fragments as
// conflict-free ds_read_b128 and its seeds and parity word from the same stage: the sweep's only vector-memory
// operations are the DMA, so nothing in it waits for one but the stage's end.  A wave whose queries all lie
// past the set (the last block of a problem) still stages and waits at the barriers, and computes nothing.
//
// 16 v_mfma_i32_32x32x32_i8 per 64-row tile, accumulators seeded with floor(n2/2):
//   R = q'.t'' + floor(n2/2),  D = 2R + (n2 & 1),  d^2 = D + c(q), exact.
// Accumulator g of lane (h = lane >> 5, r = lane & 31) of a 32-row half tile is train row
// (g & 3) + 8 (g >> 2) + 4 h against query column r (the layout block_mfma of knn.hip reads its seeds by).
// Every accumulator is filtered against the rule's limit on R, one min3 chain per 16 values and one ballot;
// only a wave with a value under some lane's limit enters the row loop, which hands single rows to the rule.
// A padded train row's R is 2^30 - 1 + q'.t''.  gfx950, wave64.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>

#include "mim_internal.h"

namespace mim {

namespace {

typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(16))) int i32x16;
typedef const __attribute__((address_space(1))) i32x4 gi32x4;  // global (not flat) loads
typedef const __attribute__((address_space(1))) int gint;

constexpr int kI8Threads = 64 * kKnnWaves;
constexpr int kI8Stage = 2;                      // 64-row train tiles per LDS stage (per barrier)
constexpr int kI8Frags = kTileBytes / 1024;      // 1 KiB wave loads per tile
constexpr int kI8LdsTile = kTileBytes + 512;     // fragments + the train half of the norm block
static_assert((kI8Stage * kI8Frags) % kKnnWaves == 0, "the waves share a stage's fragments evenly");

// The lane's query column in one column tile.
struct I8Col {
    int q;       // the query row within its set
    int cq;      // c(q) = |q - 128|^2 + 2 sum(q - 128), within +-2^22; 0 past the set
    bool valid;  // q < nq
};

// A Rule holds the per-column state of one work item (kKnnQT columns, unrolled indices only) and provides
//   static constexpr bool kSkipEmpty   an empty split of the schedule (tile0 >= tile1) is left out altogether
//   Rule(prob, w, args)                 from the problem record (its q and t are the SetDev), the unit, the kernel's arguments
//   init(u, col)                        column tile u's state before the sweep
//   begin()                             once after every init
//   limit(u)                            the filter: no row with R above it can matter to column tile u
//   static constexpr bool kFixedLimit   limit(u) does not change during the sweep
//   row(u, col, R, par, row, nt)        one row of a half tile that some lane of the wave has under its limit (this
//                                       lane's R may lie above it): R, par = n2 & 1.  Rows from nt on are padding.
//   finish(col, h, active)              the epilogue; active: some column of the wave is valid (wave-uniform)
// The row loop stands here and not in the rule: as a function of its own it is unrolled before it is inlined
// into the loop over the column tiles, and what its 16 rows share between the column tiles (the row numbers,
// row < nt, the parities) is then hoisted out of the hit path into the MFMA block, 47 VALU instructions and 30
// VGPRs that every half tile pays.
template <class Rule, class Prob, class Args>
__device__ __forceinline__ void i8_sweep(const Prob* __restrict__ probs, const KnnWork* __restrict__ works,
                                         const int* __restrict__ seg_start, const Args& args) {
    constexpr int QT = kKnnQT;
    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * kI8Stage * kI8LdsTile];
    const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, r = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int si_end = seg_start[blockIdx.x + 1];
    for (int si = seg_start[blockIdx.x]; si < si_end; ++si) {
        const KnnWork w = works[si];
        const Prob* P = probs + w.problem;
        if (*P->q.flags | *P->t.flags) continue;  // not integer-valued: the float kernel's (block-uniform)
        if (Rule::kSkipEmpty && w.tile0 >= w.tile1) continue;  // (block-uniform)
        const int nq = P->q.n, nt = P->t.n;
        const int qbase = w.q0 + wave * 32 * QT;
        const bool active = qbase < nq;  // wave-uniform
        const uint4* tsrc = reinterpret_cast<const uint4*>(P->t.frag);
        const int* tnorm = P->t.norm;

        // query fragments q' = ~t'' and c(q) of the lane's column in each column tile
        i32x4 B[QT][4];
        I8Col col[QT];
        Rule rule(*P, w, args);
#pragma unroll
        for (int u = 0; u < QT; ++u) {
            const int qr = qbase + 32 * u, qt = qr >> 6, qh = (qr >> 5) & 1;
            const int qtc = qt < P->q.n_tiles ? qt : 0;  // tiles past the set: tile 0's, never valid
            const gi32x4* qsrc = (const gi32x4*)(P->q.frag) + (size_t)qtc * 512;
#pragma unroll
            for (int s = 0; s < 4; ++s) B[u][s] = ~qsrc[(qh * 4 + s) * 64 + lane];
            const int q = qr + r;
            col[u].q = q;
            col[u].valid = q < nq;
            col[u].cq = col[u].valid ? ((const gint*)P->q.norm)[(size_t)(q >> 6) * kNormWords + 128 + (q & 63)] : 0;
            rule.init(u, col[u]);
        }
        rule.begin();

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
                    if (__builtin_amdgcn_ballot_w64(m <= rule.limit(u)) == 0) continue;
                    // A fixed limit: the rows some lane has under it first (independent compares into SGPR pairs),
                    // then a scalar test per row: at 8 matches per query one row in five has a hit somewhere in the
                    // wave.  A limit that falls: row by row, against the limit as the rows before left it.
                    unsigned long long hm[16];
                    if (Rule::kFixedLimit) {
#pragma unroll
                        for (int g = 0; g < 16; ++g) hm[g] = __builtin_amdgcn_ballot_w64(p[g] <= rule.limit(u));
                    }
#pragma unroll
                    for (int g = 0; g < 16; ++g) {
                        if ((Rule::kFixedLimit ? hm[g] : __builtin_amdgcn_ballot_w64(p[g] <= rule.limit(u))) == 0) continue;
                        const int pos = (g & 3) + 8 * (g >> 2);
                        rule.row(u, col[u], p[g], (pw >> pos) & 1u, row0 + pos + 4 * h, nt);
                    }
                }
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's DMA into the next buffer landed
            __syncthreads();
        }
        rule.finish(col, h, active);
    }
}

}  // namespace

}  // namespace mim
