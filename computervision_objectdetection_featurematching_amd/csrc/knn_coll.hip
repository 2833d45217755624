// knn_coll.hip — knnMatch over a train collection (BFMatcher::add + knnMatch(query, k)): the i8
// MFMA top-k kernel for 128-D sets that are integer-valued on both sides, and the kernel that merges every
// image's partial lists into one list per query row with the image in imgIdx.  Binary sets, generic float
// sets and flagged 128-D sets go through the top-k kernels of knn_topk.hip.
//
// knn_topk_i8_kernel has the frame of radius_i8_kernel (radius.hip): KnnWork units of knn_schedule_static, a
// block of kKnnWaves waves, a wave = kKnnQT 32-query column tiles whose q' fragments stay in VGPRs, train
// tiles and the train half of their norm blocks staged HBM -> LDS by LDS-DMA, double buffered, one barrier per
// stage, 16 v_mfma_i32_32x32x32_i8 per 64-row tile, accumulators seeded with floor(n2/2):
//   R = q'.t'' + floor(n2/2),  D = 2R + (n2 & 1),  d^2 = D + c(q), exact.
// In place of the radius threshold a lane keeps, per column tile, an ascending list of (sqrtf(d^2), row) in
// VGPRs (unrolled indices only).  A lane meets its rows in ascending order (accumulator g of lane half h is row
// (g & 3) + 8 (g >> 2) + 4 h of the half tile), so inserting behind a strict < on the float is OpenCV's tie
// rule inside a lane's list.  The two lane halves hold disjoint rows of one query: they are written as two
// lists, and the merge joins them.
//
// The integer filter.  With kK the list's k-th distance (FLT_MAX while it is not full) a pair is inserted iff
// sqrtf((float)d^2) < kK.  thr = nextafterf(fl(kK * kK), +inf) has d^2 > thr => sqrtf(d^2) >= kK (the claim
// proved in knn_topk.hip's header; d^2 < 2^23 is an integer, so (float)d^2 is exact), and for the integer
// d^2 that is d^2 > T = floor(thr).  So only pairs with 2R + p + c(q) <= T can be inserted, and p >= 0 gives
//   R <= lim = floor((T - c(q)) / 2),
// one register per list as hf of radius_i8_kernel.  fl(kK * kK) >= 2^23 (above every d^2; the list not full)
// is lim = INT_MAX: every pair is a candidate, the padded train rows (R = 2^30 - 1 + q'.t'') included, so the
// hit path tests row < nt itself.  Candidates are decided by the exact float compare, which then re-derives
// lim.  A column past the query set has lim = INT_MIN.  Only the last k of the KT slots are used: the first
// KT - k hold (-1, -1), below every distance, so the bound is the k-th distance and not the KT-th.
// gfx950, wave64.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>

#include "knn_coll.h"

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

// lim of the file header from the list's k-th distance
__device__ __forceinline__ int i8_limit(float kK, int cq) {
    const float p = kK * kK;
    if (!(p < 8388608.f)) return INT_MAX;
    return ((int)__uint_as_float(__float_as_uint(p) + 1u) - cq) >> 1;  // |c(q)| <= 2^22: no overflow
}

template <int KT>
__global__ __launch_bounds__(kI8Threads) void knn_topk_i8_kernel(const CollI8Prob* __restrict__ probs,
                                                                 const KnnWork* __restrict__ works,
                                                                 const int* __restrict__ seg_start, int k) {
    constexpr int QT = kKnnQT;
    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * kI8Stage * kI8LdsTile];
    const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, r = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int si_end = seg_start[blockIdx.x + 1];
    for (int si = seg_start[blockIdx.x]; si < si_end; ++si) {
        const KnnWork w = works[si];
        const CollI8Prob* P = probs + w.problem;
        if (*P->q.flags | *P->t.flags) continue;  // not integer-valued: the float kernel's (block-uniform)
        // an empty split of the schedule (tile0 == tile1) sweeps nothing and writes its sentinel lists
        const int nq = P->q.n, nt = P->t.n;
        const int qbase = w.q0 + wave * 32 * QT;
        const bool active = qbase < nq;  // wave-uniform
        const uint4* tsrc = reinterpret_cast<const uint4*>(P->t.frag);
        const int* tnorm = P->t.norm;

        // query fragments q' = ~t'' and c(q) of the lane's column in each column tile; the empty lists
        i32x4 B[QT][4];
        int lim[QT], cq[QT];
        bool valid[QT];
        float Ld[QT][KT];
        int Li[QT][KT];
#pragma unroll
        for (int u = 0; u < QT; ++u) {
            const int qr = qbase + 32 * u, qt = qr >> 6, qh = (qr >> 5) & 1;
            const int qtc = qt < P->q.n_tiles ? qt : 0;  // tiles past the set: tile 0's, never inserted
            const gi32x4* qsrc = (const gi32x4*)(P->q.frag) + (size_t)qtc * 512;
#pragma unroll
            for (int s = 0; s < 4; ++s) B[u][s] = ~qsrc[(qh * 4 + s) * 64 + lane];
            const int q = qr + r;
            valid[u] = q < nq;
            cq[u] = valid[u] ? ((const gint*)P->q.norm)[(size_t)(q >> 6) * kNormWords + 128 + (q & 63)] : 0;
            lim[u] = valid[u] ? INT_MAX : INT_MIN;
#pragma unroll
            for (int a = 0; a < KT; ++a) {
                Ld[u][a] = FLT_MAX;
                Li[u][a] = INT_MAX;
            }
        }
        // the KT - k unused slots in front: (-1, -1) shifted in one at a time (a loop, not a compare of k per slot)
        for (int j = KT - k; j > 0; --j) {
#pragma unroll
            for (int u = 0; u < QT; ++u) {
#pragma unroll
                for (int a = KT - 1; a > 0; --a) {
                    Ld[u][a] = Ld[u][a - 1];
                    Li[u][a] = Li[u][a - 1];
                }
                Ld[u][0] = -1.f;
                Li[u][0] = -1;
            }
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
                    if (__builtin_amdgcn_ballot_w64(m <= lim[u]) == 0) continue;
                    // a scalar test per row against the limits as the rows before it left them (lim only falls)
#pragma unroll
                    for (int g = 0; g < 16; ++g) {
                        if (__builtin_amdgcn_ballot_w64(p[g] <= lim[u]) == 0) continue;
                        const int pos = (g & 3) + 8 * (g >> 2), row = row0 + pos + 4 * h;
                        if (p[g] <= lim[u] && row < nt && valid[u]) {  // a padded row's R is under an unbounded lim
                            const int D = (int)(((unsigned)p[g] << 1) | ((pw >> pos) & 1u));
                            const float d = sqrtf((float)(D + cq[u]));
                            if (d < Ld[u][KT - 1]) {
                                // slot a takes slot a - 1's entry where d is below that too, else d where it is
                                // below slot a's (one compare per slot, carried down the list)
                                bool here = true;
#pragma unroll
                                for (int a = KT - 1; a > 0; --a) {
                                    const bool up = d < Ld[u][a - 1];
                                    Ld[u][a] = up ? Ld[u][a - 1] : here ? d : Ld[u][a];
                                    Li[u][a] = up ? Li[u][a - 1] : here ? row : Li[u][a];
                                    here = up;
                                }
                                Ld[u][0] = here ? d : Ld[u][0];
                                Li[u][0] = here ? row : Li[u][0];
                                lim[u] = i8_limit(Ld[u][KT - 1], cq[u]);
                            }
                        }
                    }
                }
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's DMA into the next buffer landed
            __syncthreads();
        }

        if (active) {
#pragma unroll
            for (int u = 0; u < QT; ++u) {
                if (!valid[u]) continue;
                // all KT slots, the unused ones in front included: the merge reads the last k
                TopkEnt* o = P->parts + ((size_t)(2 * w.split + h) * P->q_pad + (qbase + 32 * u + r)) * KT;
#pragma unroll
                for (int a = 0; a < KT; ++a) o[a] = TopkEnt{Ld[u][a], Li[u][a]};
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// Merge and emit: a thread per query row, blockIdx.y the query set
// ---------------------------------------------------------------------------------------------------
constexpr int kMergeThreads = 128;

template <int KT>
__global__ __launch_bounds__(kMergeThreads) void knn_coll_merge_kernel(const CollQuery* __restrict__ queries,
                                                                       const CollPart* __restrict__ parts, int n_parts, int k,
                                                                       bool seed, int32_t* idx, int32_t* img, float* dist) {
    const CollQuery Q = queries[blockIdx.y];
    const int q = blockIdx.x * kMergeThreads + (int)threadIdx.x;
    if (q >= Q.nq) return;
    const long long o = Q.out_off + (long long)q * k;
    coll_merge_query<KT>(parts + (size_t)blockIdx.y * n_parts, n_parts, k, q, seed, idx + o, img + o, dist + o);
}

}  // namespace

void launch_knn_topk_i8(const CollI8Prob* probs, const KnnWork* works, const int* seg_start, int n_blocks, int k,
                        hipStream_t st) {
    if (n_blocks <= 0) return;
    if (k <= 4) knn_topk_i8_kernel<4><<<n_blocks, kI8Threads, 0, st>>>(probs, works, seg_start, k);
    else if (k <= 8) knn_topk_i8_kernel<8><<<n_blocks, kI8Threads, 0, st>>>(probs, works, seg_start, k);
    else knn_topk_i8_kernel<16><<<n_blocks, kI8Threads, 0, st>>>(probs, works, seg_start, k);
}

void launch_knn_coll_merge(const CollQuery* queries, int n_queries, const CollPart* parts, int n_parts, int max_nq, int k,
                           bool seed, int32_t* idx, int32_t* img, float* dist, hipStream_t st) {
    if (n_queries <= 0 || max_nq <= 0) return;
    const int gx = (max_nq + kMergeThreads - 1) / kMergeThreads;
    for (int q0 = 0; q0 < n_queries; q0 += 65535) {  // grid.y limit
        const dim3 grid(gx, std::min(n_queries - q0, 65535));
        const CollPart* p = parts + (size_t)q0 * n_parts;
        if (k <= 4) knn_coll_merge_kernel<4><<<grid, kMergeThreads, 0, st>>>(queries + q0, p, n_parts, k, seed, idx, img, dist);
        else if (k <= 8) knn_coll_merge_kernel<8><<<grid, kMergeThreads, 0, st>>>(queries + q0, p, n_parts, k, seed, idx, img, dist);
        else knn_coll_merge_kernel<16><<<grid, kMergeThreads, 0, st>>>(queries + q0, p, n_parts, k, seed, idx, img, dist);
    }
}

}  // namespace mim
