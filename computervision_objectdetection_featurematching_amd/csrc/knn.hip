// knn.hip — brute-force NORM_L2 k=2 matching + Lowe ratio test on gfx950.
//
// Replaces BFMatcher(NORM_L2).knnMatch(view, scene, m, 2) and the ratio-test loop of
// /root/reference/src/TestsDetector.cpp:36,60,66-72 (OpenCV: matchers.cpp knnMatchImpl ->
// batch_distance.cpp batchDistance(K=2) -> normL2Sqr_).
//
// Exact path (SIFT rows: integers in [0,255]): a set is stored once as t'' = 127 - t in [-128,127]
// (exact in i8); as a query the same bytes give q' = q - 128 = ~t''.  Then q - t = q' + t'' + 1 and
//   |q - t|^2 = n2(t) + 2 q'.t'' + c(q),   n2(t) = |t - 128|^2,  c(q) = |q - 128|^2 + 2 sum(q - 128),
// with q'.t'' on the i8 MFMA (v_mfma_i32_32x32x32_i8, i32 accumulate: 2x the bf16 rate).  Every
// distance is an exact integer, so d = sqrtf(d^2) is bit-identical to OpenCV's sqrt(normL2Sqr_)
// (SURVEY.md Appendix B).  The accumulator starts at floor(n2/2), so the MFMA yields
// R = q'.t'' + floor(n2/2) and D = d^2 - c(q) = 2R + (n2 & 1) (one v_lshl_add_u32).
// Top-2 selection: OpenCV orders by the float distance sqrtf(d^2) (ties -> lower train index).  The
// sweep keeps, branch-free, the two smallest (D, index) per query.  sqrtf is monotone and, below
// 2^22, injective on integers, so that pair is OpenCV's top-2 whenever the 2nd d^2 < 4e6 (equal d^2
// keep the lower index); other queries are rescanned exactly by knn2_rescan_kernel.
//
// Generic path (any other float rows): per-pair fp32 arithmetic in OpenCV's SSE normL2Sqr_ order
// (4 accumulators x 4 lanes, no FMA), bit-identical to oracle/mim_oracle.c l2sqr_sse_order.
#include "mim_internal.h"
#include <float.h>
#include <limits.h>

namespace mim {

typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(16))) int i32x16;
typedef const __attribute__((address_space(1))) i32x4 gi32x4;  // global (not flat) loads
typedef const __attribute__((address_space(1))) int gint;

// ------------------------------------------------------------------------------------------------
// prep: fp32 rows -> i8 fragment-major tiles of 127 - d + norms + integrality flag.
// Fragment-major: a tile of 64 rows is [u 0..1][kstep s 0..3][lane 0..63][j 0..15] with
// row = 32u + (lane & 31), col = 32s + 16(lane >> 5) + j — the per-lane operand of
// v_mfma_i32_32x32x32_i8 (query and train use the same k order, so the product is k-order free);
// one 1 KiB wave load = one fragment, fully coalesced.
// Norm block per tile (kNormWords): [64] floor(n2/2), [2] the 64 values n2 & 1 as a bit mask + [62]
// zero (the train side, staged to LDS as is), [64] c (the query side), [64] the early-phase key
// addends K = 2^28 + 128 (n2 & 1) + row (train side, staged for the early tiles only); padded rows
// floor(n2/2) = 2^30 - 1, n2 & 1 = 1, so D = INT_MAX, and K = 255, so their early key is UINT_MAX.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void prep_tile(const float* __restrict__ src, int n, int8_t* __restrict__ frag,
                                          int* __restrict__ norm, int* __restrict__ flags, int tile) {
    // per row: n2 and sum(t - 128) in 4 partials (one per 32-column block = one per wave), summed by
    // the first wave; every row is read once, by the fragment pass (integer sums: exact in any order)
    __shared__ int2 part[4][64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int bad = 0;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int ci = k * 256 + tid;  // output chunk (16 B) within the tile: u = k, s = w
        const int row = tile * 64 + 32 * k + (lane & 31);
        const int col = 32 * w + 16 * (lane >> 5);
        uint32_t o[4] = {0, 0, 0, 0};
        int n2 = 0, sum = 0;
        if (row < n) {
            const float4* p = reinterpret_cast<const float4*>(src + (size_t)row * kDim + col);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float4 a = p[c];
                const float v[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    bad |= !(v[j] >= 0.f && v[j] <= 255.f && v[j] == rintf(v[j]));
                    const int d = (int)v[j] - 128;  // garbage for non-integer rows (flagged, unused)
                    n2 += d * d;
                    sum += d;
                    o[c] |= (uint32_t)((127 - (int)v[j]) & 0xff) << (8 * j);
                }
            }
        }
        reinterpret_cast<uint4*>(frag)[(size_t)tile * 512 + ci] = make_uint4(o[0], o[1], o[2], o[3]);
        n2 += __shfl_xor(n2, 32);  // the other 16 columns of the row's 32-column block
        sum += __shfl_xor(sum, 32);
        if (lane < 32) part[w][32 * k + lane] = make_int2(n2, sum);
    }
    __syncthreads();
    if (tid < 64) {
        const int row = tile * 64 + tid;
        int n2 = 0, sum = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            n2 += part[q][tid].x;
            sum += part[q][tid].y;
        }
        int* nb = norm + (size_t)tile * kNormWords;
        nb[tid] = row < n ? n2 >> 1 : (1 << 30) - 1;
        // the 64 parities as one bit mask (row i = bit i) in words 64, 65; words 66..127 zero
        const unsigned long long pm = __ballot(row < n ? n2 & 1 : 1);  // tid < 64: wave 0, all lanes
        nb[64 + tid] = tid < 2 ? (int)(uint32_t)(pm >> (32 * tid)) : 0;
        nb[128 + tid] = n2 + 2 * sum;
        nb[192 + tid] = row < n ? (1 << 28) + ((n2 & 1) << 7) + tid : 255;
    }
    if (__any(bad) && (tid & 63) == 0) atomicOr(flags, 1);
}

// Every set created since the last batch in one launch: block b preps tile b - tile0 of the last
// job with tile0 <= b (jobs ascending in tile0; sets without rows own no tile).
__global__ __launch_bounds__(256) void prep_batch_kernel(const PrepJob* __restrict__ jobs, int njobs) {
    int lo = 0, hi = njobs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].tile0 <= (int)blockIdx.x) lo = mid;
        else hi = mid - 1;
    }
    const PrepJob J = jobs[lo];
    prep_tile(J.src, J.n, J.frag, J.norm, J.flags, (int)blockIdx.x - J.tile0);
}

// ------------------------------------------------------------------------------------------------
// Running top-2 of one query in the exact integer domain D = d^2 - c(q).  Candidates of one
// selection arrive in increasing train index: strict `<` keeps the earlier of equal D.
// ------------------------------------------------------------------------------------------------
struct LaneSel {
    int m1, m2;  // two smallest D (INT_MAX = absent)
    int i1, i2;  // their train indices (INT_MAX = absent)
};

__device__ __forceinline__ void sel_init(LaneSel& s) {
    s.m1 = s.m2 = INT_MAX;
    s.i1 = s.i2 = INT_MAX;
}

// branch-free insertion of (v, idx): 7 VALU
__device__ __forceinline__ void sel_push(LaneSel& s, int v, int idx) {
    const bool c1 = v < s.m1, c2 = v < s.m2;
    s.m2 = max(min(s.m1, s.m2), min(max(s.m1, s.m2), v));  // med3 (one v_med3_i32)
    s.i2 = c2 ? (c1 ? s.i1 : idx) : s.i2;
    s.m1 = min(s.m1, v);
    s.i1 = c1 ? idx : s.i1;
}

__device__ __forceinline__ bool dlt(int da, int ia, int db, int ib) { return da < db || (da == db && ia < ib); }

// union of two selections over disjoint rows: two smallest (D, index)
__device__ __forceinline__ LaneSel sel_merge(LaneSel a, const LaneSel& b) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int w = k ? b.m2 : b.m1;
        const int iw = k ? b.i2 : b.i1;
        const bool l1 = dlt(w, iw, a.m1, a.i1), l2 = dlt(w, iw, a.m2, a.i2);
        a.m2 = l1 ? a.m1 : (l2 ? w : a.m2);
        a.i2 = l1 ? a.i1 : (l2 ? iw : a.i2);
        a.m1 = l1 ? w : a.m1;
        a.i1 = l1 ? iw : a.i1;
    }
    return a;
}

// Ratio mode (knn2_i8_kernel<true>): the two smallest D as values and the index of the smallest
// only.  Which of two equal minima gives i1 does not matter: a query whose two smallest are equal
// fails every ratio test below 1.
__device__ __forceinline__ void sel_push_r(LaneSel& s, int v, int idx) {
    const bool c1 = v < s.m1;
    s.m2 = max(min(s.m1, s.m2), min(max(s.m1, s.m2), v));
    s.m1 = min(s.m1, v);
    s.i1 = c1 ? idx : s.i1;
}

__device__ __forceinline__ LaneSel sel_merge_r(const LaneSel& a, const LaneSel& b) {
    LaneSel r;
    const bool l = b.m1 < a.m1;
    r.m1 = l ? b.m1 : a.m1;
    r.i1 = l ? b.i1 : a.i1;
    r.m2 = min(max(a.m1, b.m1), min(a.m2, b.m2));  // 2nd smallest of {a.m1 <= a.m2, b.m1 <= b.m2}
    r.i2 = INT_MAX;
    return r;
}

__device__ __forceinline__ bool key_less(float ka, int ia, float kb, int ib) {
    return ka < kb || (ka == kb && ia < ib);
}

struct T2 {
    float k1; int i1; float k2; int i2;
};

__device__ __forceinline__ T2 top2_merge(T2 a, float k, int i) {
    const bool l1 = key_less(k, i, a.k1, a.i1);
    const bool l2 = key_less(k, i, a.k2, a.i2);
    T2 r;
    r.k1 = l1 ? k : a.k1;
    r.i1 = l1 ? i : a.i1;
    r.k2 = l1 ? a.k1 : (l2 ? k : a.k2);
    r.i2 = l1 ? a.i1 : (l2 ? i : a.i2);
    return r;
}

constexpr int kRescan = -2;  // Top2::i2 marker: the split's top-2 needs the exact rescan

// Accumulator value g of a 32x32 MFMA tile is train row (g&3) + 8(g>>2) + 4h of its 32-row block.
// Indices are stored without the lane's 4h (uniform, scalar) and corrected at the end.
//   early tiles (the top-2 still changes often): every D = 2R + p inserted branch-free;
//   later tiles: the min of a lane's 16 R is tested against the lane's threshold on R (a superset of
//     the rows that can enter the top-2); the exact insertion runs only for the 4-row groups in
//     which some lane of the wave has a candidate.
#ifndef MIM_KNN_EARLY
#define MIM_KNN_EARLY 4
#endif
constexpr int kEarlyTiles = MIM_KNN_EARLY;
#ifndef MIM_KNN_LATE_UNROLL
#define MIM_KNN_LATE_UNROLL 1
#endif
// timing probes (diagnostic builds only, results wrong): 1 late tiles without the insertion events,
// 2 without the min filter too, 3 and with zero accumulator seeds (no seed LDS reads)
#ifndef MIM_KNN_PROBE
#define MIM_KNN_PROBE 0
#endif
// parity word of a late half tile waited for with the seeds, before the MFMAs (1) or after them (0)
#ifndef MIM_KNN_PW_EARLY
#define MIM_KNN_PW_EARLY 0
#endif
// s_setprio 1 for waves 4-7 (the younger half of each SIMD's pair)
#ifndef MIM_KNN_PRIO
#define MIM_KNN_PRIO 0
#endif


// Threshold on R of a lane in the late tiles.  Lanes l, l ^ 32 hold the same query over disjoint
// row halves; the union of their two top-2 lists always contains the query's top-2 so far.  A new
// row can enter that top-2 only if D <= Dc, the 2nd smallest of the pair's four D (an equal D may
// still win on the lower index), and a row that does enters its own lane's list, so the filter
// keeps the invariant.  D = 2R + p with p in {0,1} gives R <= floor(Dc/2).
// o1 <= o2: the partner lane's m1, m2 (exchanged by permlane32_swap at each refresh; the partner's
// values only decrease, so a stale copy gives a threshold >= the exact one: still a superset).
__device__ __forceinline__ int late_threshold(const LaneSel& s, int o1, int o2) {
    return min(max(s.m1, o1), min(s.m2, o2)) >> 1;  // 2nd smallest of {m1 <= m2, o1 <= o2}, halved
}
// Ratio mode: 1st and 2nd smallest of the lane pair's four D (partner copy o1 <= o2, stale = larger)
__device__ __forceinline__ int pair_first(const LaneSel& s, int o1) { return min(s.m1, o1); }
__device__ __forceinline__ int pair_second(const LaneSel& s, int o1, int o2) {
    return min(max(s.m1, o1), min(s.m2, o2));
}
// rows with D < v: D = 2R + p <= v - 1 gives R <= floor((v - 1) / 2)
__device__ __forceinline__ int below_threshold(int v) { return (v - 1) >> 1; }
__device__ __forceinline__ int dval(int R, int p) { return (R << 1) | p; }  // v_lshl_or_b32

// v_med3_u32 (the compiler rewrites the max/min form of a top-2 update into a max and two mins)
__device__ __forceinline__ unsigned med3_u32(unsigned a, unsigned b, unsigned c) {
    unsigned r;
    asm("v_med3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

__device__ __forceinline__ int med3_i32(int a, int b, int c) {
    int r;
    asm("v_med3_i32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// insertion events of the late tiles: 0 a ballot per row of a hit row group and an out-of-line push per
// hit row; 1 the group's two smallest (R, row) keys branch-free, the first pushed in every lane, the
// second only when some lane can still take it, the rest of the group by rows after that (rare)
#ifndef MIM_KNN_EVENT
#define MIM_KNN_EVENT 0
#endif
// waves 4-7 (the second wave of each SIMD's pair in a block) defer the filter and events of each
// stage's last half tile past the stage barrier, so a SIMD's two waves of one block do not filter at
// the same time (MI355X_MICROARCH.md, "try a stagger")
#ifndef MIM_KNN_STAGGER
#define MIM_KNN_STAGGER 0
#endif
// refresh schedule of the late loop: every stage for the first MIM_KNN_REFRESH_DENSE late stages of a
// sweep, after that on every MIM_KNN_REFRESH_EVERY-th late stage, counted from the first late stage (so a
// work item starting at any tile behaves the same).  EVERY = 1: every stage, the code without a schedule.
#ifndef MIM_KNN_REFRESH_DENSE
#define MIM_KNN_REFRESH_DENSE 8
#endif
#ifndef MIM_KNN_REFRESH_EVERY
#define MIM_KNN_REFRESH_EVERY 4
#endif
constexpr int kRefreshDense = MIM_KNN_REFRESH_DENSE, kRefreshEvery = MIM_KNN_REFRESH_EVERY;
static_assert(kRefreshDense >= 0 && kRefreshEvery >= 1, "refresh schedule");
// MFMA order inside a 32-row block: 0 k-step major (both column tiles' chains end together), 1 column-tile
// major (the four k-steps of column tile 0, then those of tile 1: tile 0's filter can start under them)
#ifndef MIM_KNN_MFMA_ORDER
#define MIM_KNN_MFMA_ORDER 0
#endif
// a wave whose queries all lie past the set (qbase >= nq) only stages and keeps the barriers; 0: it
// runs the whole sweep on padding, as every wave did before
#ifndef MIM_KNN_SKIP_PAD
#define MIM_KNN_SKIP_PAD 1
#endif

// ------------------------------------------------------------------------------------------------
// Exact distance kernel.  Block = kKnnWaves waves = kKnnBlockQ queries (each wave: kKnnQT 32-query
// MFMA column tiles, their q' fragments held in VGPRs for the whole sweep).  Train rows stream
// HBM -> LDS by LDS-DMA in stages of kKnnStage 64-row tiles (double buffer, one barrier per stage);
// per tile a wave reads the 8 KiB of fragments as 8 conflict-free ds_read_b128 and issues 8 kKnnQT
// i8 MFMAs.
// ------------------------------------------------------------------------------------------------
constexpr int kLdsTile = kTileBytes + 768;  // fragments + the train half of the norm block + the key addends
constexpr int kStage = kKnnStage;
constexpr int kThreads = 64 * kKnnWaves;
constexpr int kStageChunks = kStage * kTileBytes / 16 / kThreads;  // 16-B fragment chunks per thread
static_assert(kStageChunks * 16 * kThreads == kStage * kTileBytes, "stage split");

#ifndef MIM_KNN_OCC
#define MIM_KNN_OCC 4
#endif

// Verdict mode stores a value doubled with a mark in bit 0: 2 D for a row pushed exactly, 4 R + 3 for a
// row that was tracked (its R is known, its parity is not): it orders after both exact values it could be.
// e_hi: the largest D the value can stand for (D itself, or 2 R + 1).
__device__ __forceinline__ int e_hi(int e) { return e >> 1; }
// an mn that tracks nothing: 4 kNoTrack + 3 lies above every real value and below INT_MAX
constexpr int kNoTrack = 1 << 28;

// The ratio argument of the distance kernel: kappa alone for the exact and the ratio mode, (kappa, ratio)
// for the verdict mode, which evaluates the ratio kernel's own test at the end of the sweep.
template <int MODE>
struct KnnRatioArg {
    using type = float;
    static __device__ __forceinline__ float kappa(float a) { return a; }
    static __device__ __forceinline__ float ratio(float) { return 0.f; }
};
template <>
struct KnnRatioArg<2> {
    using type = float2;
    static __device__ __forceinline__ float kappa(float2 a) { return a.x; }
    static __device__ __forceinline__ float ratio(float2 a) { return a.y; }
};
//
// Ratio mode (RATIO, kappa in (0, 1)): the batch path reads the top-2 only through the ratio test
// k1 < ratio * k2 and i1 where it passes, so a lane pair that fails the test needs less than its exact
// 2nd neighbour.  kappa >= ratio^2 (1 + 2^-18): d1^2 >= kappa d2^2 makes the float test false, and a
// smaller d2^2 keeps it false.  Q1 <= Q2 are the two smallest of the pair's four list values, G1 <= G2
// the two smallest D of all rows so far.  Invariant: Q1 = G1, Q2 >= G2, and Q2 = G2 or F(Q1, Q2), where
// F(a, b) is the float test (a + c) >= kappa (b + c), monotone in b.  A refresh sets a lane's limit to
// v = Q1 when F(Q1, Q2) holds (failing), else v = Q2 (candidate); a row with D >= v is ignored.
//   Inserting a row keeps the invariant: Q1, Q2 become the two smallest of {Q1, Q2, D}; with Q2 > G2
//   and D < Q1 the new second is the old G1, exact again; with Q1 <= D < Q2, F(Q1, D) follows from F(Q1, Q2).
//   Ignoring a row under a candidate limit (D >= Q2 >= G2) changes nothing.
//   Ignoring a row under a failing limit v = Q1r (the refresh's pair Q1r, Q2r, F(Q1r, Q2r)): while Q1 is
//   still Q1r, D >= G1 can only lower G2, and F(Q1r, Q2) holds as Q2 <= Q2r; once an insertion has lowered
//   Q1, Q2 <= Q1r <= D and the row changes nothing.  Partner values are stale, that is larger: limits only
//   grow.  After an insertion the limit becomes min(limit, candidate limit of the fresh pair): for a
//   failing lane that is a change only when Q1 fell, and then Q2 <= Q1r.
// So a failing pair takes an event only for a new minimum, not for every row that enters its top-2.
// At the end the split emits (Q1, i1, Q2): exact, or failing with Q2 too large, which fails the test as
// the true pair does; merged with other splits' pairs the same invariant holds (the minimum is exact,
// the second too large only behind F).  Equal minima fail the test, so i1 and the rescan's index order do
// not matter.  Thresholds are on R: D < v is R <= floor((v - 1) / 2).
//
// Verdict mode (MODE 2; whole sweeps of one split only, so the work item's verdict is final): a failing
// pair does not take an event for a new minimum either.  A list value is 2 D (exact, pushed with its index)
// or 4 R + 3 (tracked: the row's R without its parity; D is 2 R or 2 R + 1 = e_hi).  After the event test
// of a half tile every lane pushes 4 mn + 3 of its smallest row into its two values, unless an event has
// just pushed that very row exactly, so every value is a row of its own.  This alone gives, per lane and
// so per pair: (V1) R(Q1) is the smallest R of all rows so far, (V2) e_hi(Q1) >= G1 and e_hi(Q2) >= G2.
// A refresh calls a pair surely failing when F(2 R(Q1), e_hi(Q2)): F then holds for G1, G2 whatever the
// parities.  Its limit is the flip limit, every R with not F(2 R, e_hi(Q1)): the rows that could pass
// against the pair's first value.  Every other pair gets the candidate limit, rows with D < e_hi(Q2).  A lane
// with a row at or under its limit takes the candidate limit of its current values before the event's
// pushes (a failing lane that hits is a candidate lane from then on; its partner half stays at the flip
// limit until the next refresh); after an event limits only fall, to the fresh candidate limit.
//   (V3) The stored pair surely fails, or R(Q2) = R(G2).  A row ignored under a candidate limit has
//   D >= e_hi(Q2) >= G2 and changes nothing.  A row W ignored (tracked) under a flip limit taken at Q1r has
//   F(2 R(W), e_hi(Q1r)); the lane has not hit since, so the stored pair surely failed before W, and after
//   it: W under Q1 makes Q2 the old Q1 <= Q1r, W between them makes Q2 = W <= the old Q2, and F stays
//   true as its second argument falls; W above Q2 leaves the pair as it was.  An exact push from another
//   lane's hit into such a lane is the same three cases.  Two tracked rows of one lane and half tile: only
//   the smaller is recorded, the other lies above the flip limit as well, same argument.
//   (V4) If the true pair passes, its nearest row X took an event and Q1 = 2 G1 with X's index: under a
//   candidate limit D(X) < G2 <= e_hi(Q2); under a flip limit not F(D(X), G2) and G2 <= G1 before X
//   <= e_hi(Q1r) give not F(2 R(X), e_hi(Q1r)).  No later value lies under it (V2: every value is at least 2 D
//   of its row).  When X enters, the old Q1, right up to its parity by V1, becomes Q2 in X's lane, or is the
//   other half's first value (a flip in one half, the old minimum tracked in the other): R(Q2) = R(G2),
//   also with further rows under the old minimum in the same half tile, which the lane, a candidate
//   lane by then, pushes as well, or the other half tracks.
//   (V5) If the stored pair passes with Q1 exact, so does the true one up to Q2's parity: Q2 too large
//   needs an ignored row under it, which V3 allows only while the stored pair surely fails.
// End of the sweep: the ratio kernel's own test at the most favourable bounds (Q1 at 2 R, Q2 at e_hi) and at
// the least favourable (Q1 at e_hi, Q2 at the even value under e_hi: an exact odd Q2 may stand where an
// unrecorded row of the same R and even parity is the true second).  Failing at the first: the true pair
// fails by V2, V4; a failing record (k1 = k2) is written.  Passing at both with Q1 exact: passes by V5,
// i1 by V4.  Anything else (the two differ, or a passing first value is tracked) is marked for
// knn2_rescan_kernel, which rewrites the record from the fp32 rows.  Padded rows (R = 2^30 - 1) are never
// under a limit, and their tile caps mn before the shift; a lane half has real rows from the early tiles.
// (A padded row is still pushed, in every mode, when another lane hits its accumulator slot of the last
// tile: its D = INT_MAX never displaces a real value, and the verdict mode's push caps it before doubling.)
//
// Refresh schedule (MIM_KNN_REFRESH_DENSE, MIM_KNN_REFRESH_EVERY): a stage off the schedule exchanges
// nothing and computes no limit; o1c, o2c and T[u] stay what the last refresh and the events since left.
// Nothing above depends on when a refresh happens, only on what a limit was taken from:
//   exact mode: a lane's own values change only in events, which recompute T from them and the partner
//   copy; the copy is stale upwards, so T is at least the exact threshold: a superset, for any staleness.
//   ratio mode: a failing limit v = Q1r is justified row by row from the refresh's pair (Q1r, Q2r) for as
//   long as the lane is not refreshed again, however many stages that is; a candidate limit only falls, in
//   events, and a stale partner copy only raises it.  The invariant is kept by every row, so it holds at the
//   end of the sweep whichever stages refreshed.
//   verdict mode: V1 and V2 come from the tracked push of every half tile, which no schedule skips.  V3's
//   flip-limit case runs from the refresh that took Q1r to the lane's next hit, over any number of stages; a
//   candidate limit taken earlier stands for a larger e_hi(Q2) than the current one (tracked rows lower the
//   values without an event), so it only admits more rows, which are pushed exactly.  V4 needs X under its
//   lane's limit: D(X) < G2 <= e_hi(Q2) now <= e_hi(Q2) then, and under a flip limit the same inequality
//   against Q1r.  V5 follows from V3.
// What a skipped refresh costs is events, never a verdict: a pair that turned surely failing since the last
// refresh keeps its candidate limit until the next one (a failing lane that hits turns candidate in the event
// itself, so the reverse needs no refresh).  The first late stage of a work item always refreshes.
template <int MODE>  // 0 exact, 1 ratio mode, 2 verdict mode
__global__ __launch_bounds__(kThreads, MIM_KNN_OCC) void knn2_i8_kernel(  // OCC = waves per SIMD
    const ProbDev* __restrict__ probs, const KnnWork* __restrict__ works, const int* __restrict__ seg_start,
    Top2* __restrict__ parts, int* __restrict__ dyn_ctr, typename KnnRatioArg<MODE>::type karg) {
    constexpr bool RATIO = MODE != 0, FLIP = MODE == 2;
    const float kappa = KnnRatioArg<MODE>::kappa(karg);
    constexpr int QT = kKnnQT;
    // ratio mode: c(q) of the work item's queries behind the two stage buffers (read once per stage)
    constexpr int kCqOff = 2 * kStage * kLdsTile;
    __shared__ __attribute__((aligned(16))) unsigned char smem[kCqOff + (RATIO ? 4 * kKnnBlockQ : 0)];
    __shared__ int s_item;
    // static: block b runs works[seg_start[b] .. seg_start[b + 1]); dynamic (dyn_ctr != null): the works
    // are 8 lists (seg_start[0..8]), block b pulls items from list b mod 8 (its XCD's) with an atomic
    // counter, then from the other lists, so a block that starts late (its CU held by another batch's
    // kernel) takes less
    int si = dyn_ctr ? 0 : seg_start[blockIdx.x];
    const int si_end = dyn_ctr ? 0 : seg_start[blockIdx.x + 1];
    int list = blockIdx.x & 7, lists_done = 0;
  for (;;) {
    if (dyn_ctr) {
        int idx = -1;
        while (lists_done < 8) {
            if (threadIdx.x == 0) s_item = atomicAdd(dyn_ctr + list, 1);
            __syncthreads();
            const int k = s_item;
            __syncthreads();
            if (k < seg_start[list + 1] - seg_start[list]) {
                idx = seg_start[list] + k;
                break;
            }
            list = (list + 1) & 7;
            ++lists_done;
        }
        if (idx < 0) break;
        si = idx;
    } else if (si >= si_end) {
        break;
    }
    const KnnWork w = works[si];
    ++si;
    const ProbDev* P = probs + w.problem;
    if (*P->q.flags | *P->t.flags) continue;  // not integer-valued: generic kernel handles it
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, h = lane >> 5, r = lane & 31;
    const int nq = P->q.n;
    const uint4* __restrict__ tsrc = reinterpret_cast<const uint4*>(P->t.frag);
    const int* __restrict__ tnorm = P->t.norm;

    // ---- query fragments q': column tile u = query rows qbase + 32u .. + 31 ----
    const int qbase = w.q0 + wave * 32 * QT;
    // a wave of padding only (wave-uniform, decided on the scalar unit): no fragments, tiles, refreshes
    // or epilogue; it stages its share of every stage and meets every barrier
    const bool live = !MIM_KNN_SKIP_PAD || w.q0 + __builtin_amdgcn_readfirstlane(wave) * 32 * QT < nq;
    i32x4 B[QT][4];
    if (live) {
#pragma unroll
        for (int u = 0; u < QT; ++u) {
            const int qr = qbase + 32 * u, qt = qr >> 6, qh = (qr >> 5) & 1;
            const bool ok = qt < P->q.n_tiles;
            const int qtc = ok ? qt : 0;  // rows past the set: loaded from tile 0, never written out
            const gi32x4* qsrc = (const gi32x4*)(P->q.frag) + (size_t)qtc * 512;
#pragma unroll
            for (int s = 0; s < 4; ++s) B[u][s] = ~qsrc[(qh * 4 + s) * 64 + lane];  // q' = ~t''
        }
    }
    LaneSel st[QT];
    int T[QT];  // late-tile thresholds on R
    // the partner lane's (l ^ 32) m1, m2 as of the last refresh (the schedule above): between refreshes an
    // insertion recomputes the threshold from its own fresh pair and these (the partner's values only
    // decrease, so a stale copy gives a threshold >= the exact one: a superset, no exchange per event)
    int o1c[QT], o2c[QT];
    const int* cq = reinterpret_cast<const int*>(smem + kCqOff) + wave * 32 * QT + r;  // ratio mode
#pragma unroll
    for (int u = 0; u < QT; ++u) {
        sel_init(st[u]);
        T[u] = INT_MAX;
    }
    if (RATIO) {
        // (the previous work item's last read of these words lies before its last stage barrier)
        for (int k = tid; k < kKnnBlockQ; k += kThreads) {
            const int q = w.q0 + k, qt = q >> 6;
            const int qtc = qt < P->q.n_tiles ? qt : 0;  // as the fragments: never written out
            reinterpret_cast<int*>(smem + kCqOff)[k] = ((const gint*)P->q.norm)[(size_t)qtc * kNormWords + 128 + (q & 63)];
        }
    }
    // threshold after an insertion.  Ratio mode: never above the one set at the last refresh (a
    // failing pair keeps its lower threshold through other lanes' events, see the proof above)
    auto event_threshold = [&](int u) {
        if (FLIP) T[u] = min(T[u], below_threshold(e_hi(pair_second(st[u], o1c[u], o2c[u]))));
        else if (RATIO) T[u] = min(T[u], below_threshold(pair_second(st[u], o1c[u], o2c[u])));
        else T[u] = late_threshold(st[u], o1c[u], o2c[u]);
    };
    auto push = [&](int u, int v, int idx) {
        // exact values are stored as 2 D.  A padded row (D = INT_MAX) is pushed too when another lane hits
        // the same accumulator slot of the last tile: capped so that doubling it cannot wrap to -2, which
        // would become the minimum of every query of the column tile whose other lane half holds it
        if (FLIP) sel_push_r(st[u], min(v, INT_MAX >> 1) << 1, idx);
        else if (RATIO) sel_push_r(st[u], v, idx);
        else sel_push(st[u], v, idx);
    };

    // ---- staging: LDS-DMA (global_load_lds_dwordx4 / _dword), double buffered, one barrier per
    // stage of kStage 64-row tiles.  One wave-instruction writes 64 lanes x size contiguous bytes at a
    // wave-uniform LDS base, which the fragment-major tile already is; the norm half of the tile's
    // norm block (floor(n2/2), parity mask) is two 256-B pieces.  No staging VGPRs, no ds_write pass.
    // LDS stage layout: kStage x [8 KiB fragments | 512 B norms]; tiles past the work item's range
    // are not loaded.  (Every LDS read is an ext-vector or int access of the one smem array: with the
    // seeds read as a struct type the waitcnt pass could not tell them from the DMA's target and
    // waited for the next stage's DMA before each tile.)
    const int wv = __builtin_amdgcn_readfirstlane(wave);
    if (MIM_KNN_PRIO && wv >= 4) __builtin_amdgcn_s_setprio(1);
    auto stage_dma = [&](int t0, int buf, bool keys) {
        unsigned char* base = smem + buf * kStage * kLdsTile;
#pragma unroll
        for (int c = 0; c < kStageChunks; ++c) {
            const int cw = c * kThreads + wv * 64, tt = cw >> 9;  // the wave's first chunk: uniform
            if (kStage == 1 || t0 + tt < w.tile1)
                __builtin_amdgcn_global_load_lds((const void*)(tsrc + (size_t)t0 * 512 + cw + lane),
                                                 (__attribute__((address_space(3))) void*)(base + tt * kLdsTile + (cw & 511) * 16),
                                                 16, 0, 0);
        }
#pragma unroll
        for (int p = wv; p < 2 * kStage; p += kKnnWaves) {  // piece p: tile p >> 1, norm words 64 (p & 1) ..
            const int tt = p >> 1;
            if (kStage == 1 || t0 + tt < w.tile1)
                __builtin_amdgcn_global_load_lds((const void*)(tnorm + (size_t)(t0 + tt) * kNormWords + 64 * (p & 1) + lane),
                                                 (__attribute__((address_space(3))) void*)(base + tt * kLdsTile + kTileBytes + 256 * (p & 1)),
                                                 4, 0, 0);
        }
        if (keys) {  // early stages: the key addends (norm words 192..255) of each tile
#pragma unroll
            for (int tt = wv; tt < kStage; tt += kKnnWaves)
                if (kStage == 1 || t0 + tt < w.tile1)
                    __builtin_amdgcn_global_load_lds((const void*)(tnorm + (size_t)(t0 + tt) * kNormWords + 192 + lane),
                                                     (__attribute__((address_space(3))) void*)(base + tt * kLdsTile + kTileBytes + 512),
                                                     4, 0, 0);
        }
    };

    const int tile_e = min(w.tile1, w.tile0 + (kEarlyTiles + kStage - 1) / kStage * kStage);
    if (w.tile0 < w.tile1) stage_dma(w.tile0, 0, w.tile0 < tile_e);
    // retire every prologue load (q' fragments included) here: with one still pending at the loop
    // entry the waitcnt pass keeps a vmcnt(0) in the loop
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();

    // the 32x32 block u2 of a tile: accumulators start at floor(n2/2) (LDS), R = q'.t'' + floor(n2/2)
    auto block_mfma = [&](const unsigned char* tb, int u2, i32x16 (&acc)[QT]) {
        const i32x4* A = reinterpret_cast<const i32x4*>(tb);
        const int* tnu = reinterpret_cast<const int*>(tb + kTileBytes) + 32 * u2 + 4 * h;
#pragma unroll
        for (int gg = 0; gg < 4; ++gg) {
            const i32x4 n = MIM_KNN_PROBE >= 3 ? i32x4{0, 0, 0, 0} : *reinterpret_cast<const i32x4*>(tnu + 8 * gg);
            acc[0][4 * gg + 0] = n.x; acc[0][4 * gg + 1] = n.y; acc[0][4 * gg + 2] = n.z; acc[0][4 * gg + 3] = n.w;
        }
#pragma unroll
        for (int u = 1; u < QT; ++u) acc[u] = acc[0];
        if (MIM_KNN_MFMA_ORDER == 1) {
            i32x4 a[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) a[s] = A[(u2 * 4 + s) * 64 + lane];
#pragma unroll
            for (int u = 0; u < QT; ++u)
#pragma unroll
                for (int s = 0; s < 4; ++s) acc[u] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[s], B[u][s], acc[u], 0, 0, 0);
            return;
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const i32x4 a = A[(u2 * 4 + s) * 64 + lane];
#pragma unroll
            for (int u = 0; u < QT; ++u) acc[u] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, B[u][s], acc[u], 0, 0, 0);
        }
    };
    // early tiles: every value enters a branch-free top-2 of 32-bit keys
    //   key = (R << 8) + K = 128 D + row + 2^28  (K = 2^28 + 128 (n2 & 1) + row from the tile's norm block)
    // ordered as (D, row): R in [-2^20.1, 2^22] keeps real keys in (0, 2^31); a padded row (R = 2^30 - 1,
    // K = 255) wraps to exactly UINT_MAX and never enters.  Three VALU per value (v_lshl_add_u32,
    // v_med3_u32, v_min_u32); the tile's two keys per lane and column tile are decoded and merged into the
    // (D, index) lists at the tile's end.
    auto tile_early = [&](const unsigned char* tb, int tile) {
        const int* tk = reinterpret_cast<const int*>(tb + kTileBytes + 512) + 4 * h;
        unsigned k1[QT], k2[QT];
#pragma unroll
        for (int u = 0; u < QT; ++u) k1[u] = k2[u] = 0xFFFFFFFFu;
#pragma unroll
        for (int u2 = 0; u2 < 2; ++u2) {
            i32x16 acc[QT];
            block_mfma(tb, u2, acc);
#pragma unroll
            for (int gg = 0; gg < 4; ++gg) {
                const i32x4 kv = *reinterpret_cast<const i32x4*>(tk + 32 * u2 + 8 * gg);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
#pragma unroll
                    for (int u = 0; u < QT; ++u) {
                        const unsigned key = ((unsigned)acc[u][4 * gg + k] << 8) + (unsigned)kv[k];
                        k2[u] = med3_u32(k1[u], k2[u], key);  // = max(k1, min(k2, key)) as k1 <= k2
                        k1[u] = min(k1[u], key);
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < QT; ++u) {
            LaneSel t;
            // D = (key - 2^28) >> 7, row = key & 127 (with the lane's 4h, which the lists store without)
            t.m1 = k1[u] == 0xFFFFFFFFu ? INT_MAX : ((int)(k1[u] - (1u << 28)) >> 7) << (FLIP ? 1 : 0);
            t.i1 = k1[u] == 0xFFFFFFFFu ? INT_MAX : tile * 64 + (int)(k1[u] & 127) - 4 * h;
            t.m2 = k2[u] == 0xFFFFFFFFu ? INT_MAX : ((int)(k2[u] - (1u << 28)) >> 7) << (FLIP ? 1 : 0);
            t.i2 = RATIO || k2[u] == 0xFFFFFFFFu ? INT_MAX : tile * 64 + (int)(k2[u] & 127) - 4 * h;
            st[u] = RATIO ? sel_merge_r(st[u], t) : sel_merge(st[u], t);
        }
    };
    // late tiles: one min over a lane's 16 R per column tile against its threshold, the exact
    // insertion only in groups some lane hits.  half_filter: the 32-row half tile starting at row0
    // (accumulators acc, parity word pw); keyed: keys (R << 3 | g) cannot overflow (no padded row)
    auto half_filter = [&](const i32x16 (&acc)[QT], unsigned pw, int row0, bool keyed) {
        // a lane's 16 R as two row groups (g 0-7, 8-15): the group minima cost one v_min more
        // than a single min chain and let an event compare the rows of the hit groups only
        int mn[QT], gmn[QT][2];
        unsigned long long bm[QT], any = 0;  // wave masks of the lanes with a candidate (SGPR pairs)
#pragma unroll
        for (int u = 0; u < QT; ++u) {
            const i32x16& p = acc[u];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                int a = min(min(p[8 * i], p[8 * i + 1]), p[8 * i + 2]);
                a = min(min(a, p[8 * i + 3]), p[8 * i + 4]);
                a = min(min(a, p[8 * i + 5]), p[8 * i + 6]);
                gmn[u][i] = min(a, p[8 * i + 7]);
            }
            mn[u] = min(gmn[u][0], gmn[u][1]);
            bm[u] = __ballot(mn[u] <= T[u]);
            any |= bm[u];
        }
        // the masks are tested on the scalar unit (re-evaluating the compare as a ballot made the
        // compiler rebuild each one with a v_cndmask + v_cmp pair per event)
        if (MIM_KNN_PROBE == 1) asm volatile("" ::"s"(any));
        if (MIM_KNN_PROBE != 1 && __builtin_expect(any != 0, 0)) {  // ~1 insertion per wave and half tile
#pragma unroll
            for (int u = 0; u < QT; ++u) {
                if (bm[u] != 0) {
                    // verdict mode: a lane that hits takes the candidate limit of its current values before
                    // its rows are pushed (a surely failing lane becomes a candidate lane: the rows between
                    // its flip limit and its second value now count; a candidate lane's limit only falls)
                    if (FLIP) T[u] = mn[u] <= T[u] ? below_threshold(e_hi(pair_second(st[u], o1c[u], o2c[u]))) : T[u];
                    // per row of a hit group: one compare (the ballot) and, if some lane has the row
                    // under its threshold, an unconditional insertion in every lane (the lane lists
                    // stay the exact top-2 of the rows pushed, a superset of the filtered ones); the
                    // row ballots of a group first (independent compares into SGPR pairs), then a
                    // not-taken scalar test per row: the insertion code sits out of line
                    unsigned long long gb[2];
#pragma unroll
                    for (int i = 0; i < 2; ++i) gb[i] = __ballot(gmn[u][i] <= T[u]);
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        if (gb[i] != 0) {
                            // rows of group i in this lane: pos = (g & 3) + 8 (g >> 2) + 16 i (without 4h),
                            // ascending with g; the parity of the row is bit pos of pw
                            int k2 = INT_MAX;
                            if (MIM_KNN_EVENT == 1 && keyed) {
                                // the group's two smallest (R, row) keys: every lane pushes its own
                                // smallest row (pushing rows beyond the filter keeps a lane list the
                                // exact top-2 of the rows pushed into it); the second only if some lane
                                // can still take it once the first is in; further rows by row ballots
                                int k1 = INT_MAX;
#pragma unroll
                                for (int g = 0; g < 8; ++g) {
                                    const int key = (acc[u][8 * i + g] << 3) | g;
                                    k2 = med3_i32(k1, k2, key);
                                    k1 = min(k1, key);
                                }
                                const int pos1 = (k1 & 3) + 8 * ((k1 >> 2) & 1) + 16 * i;
                                push(u, dval(k1 >> 3, (pw >> pos1) & 1), row0 + pos1);
                                if (FLIP) mn[u] = (k1 >> 3) == mn[u] ? kNoTrack : mn[u];
                                event_threshold(u);
                                if (__builtin_expect(__ballot((k2 >> 3) <= T[u]) == 0, 1)) continue;
                                const int pos2 = (k2 & 3) + 8 * ((k2 >> 2) & 1) + 16 * i;
                                push(u, dval(k2 >> 3, (pw >> pos2) & 1), row0 + pos2);
                                if (FLIP) mn[u] = (k2 >> 3) == mn[u] ? kNoTrack : mn[u];
                                event_threshold(u);
                            }
                            // rows in index order (keyed: only those after the second key, all of which
                            // have a larger D than the two pushed rows' or an equal D and a larger row)
                            unsigned long long hm[8];
#pragma unroll
                            for (int g = 0; g < 8; ++g)
                                hm[g] = __ballot(acc[u][8 * i + g] <= T[u] &&
                                                 (MIM_KNN_EVENT != 1 || !keyed || ((acc[u][8 * i + g] << 3) | g) > k2));
#pragma unroll
                            for (int g = 8 * i; g < 8 * i + 8; ++g) {
                                if (__builtin_expect(hm[g - 8 * i] != 0, 0)) {
                                    push(u, dval(acc[u][g], (pw >> ((g & 3) + 8 * (g >> 2))) & 1),
                                         row0 + (g & 3) + 8 * (g >> 2));
                                    // verdict mode: the lane's smallest row is in its list now, exactly
                                    if (FLIP) mn[u] = acc[u][g] == mn[u] ? kNoTrack : mn[u];
                                }
                            }
                        }
                    }
                    event_threshold(u);
                }
            }
        }
        if (FLIP) {
            // the half tile's smallest row of the lane enters its list as a tracked value, without an event
            // and after the events: a lane whose smallest row has just been pushed exactly has no mn left
            // (kNoTrack), so no row is counted twice.  Three VALU per column tile: v_lshl_or_b32,
            // v_med3_i32, v_min_i32.  The padded tile (R = 2^30 - 1 would overflow the shift) caps mn first,
            // in a branch of its own (the asm keeps it a branch).
            if (__builtin_expect(!keyed, 0)) {
                asm volatile("; padded tile");
#pragma unroll
                for (int u = 0; u < QT; ++u) mn[u] = min(mn[u], kNoTrack);
            }
#pragma unroll
            for (int u = 0; u < QT; ++u) {
                const int tv = (mn[u] << 2) | 3;
                st[u].m2 = med3_i32(st[u].m1, st[u].m2, tv);  // = max(m1, min(m2, tv)) as m1 <= m2
                st[u].m1 = min(st[u].m1, tv);
            }
        }
    };
    // deferred half tile (MIM_KNN_STAGGER, waves 4-7): its accumulators, parity word and first row
    i32x16 dacc[QT];
    unsigned dpw = 0;
    int drow0 = -1;
    bool dkeyed = false;
    const bool stagger = MIM_KNN_STAGGER && wv >= 4;
    // the last set tile holds padded rows (R ~ 2^30): no keyed events there
    const int pad_tile = (P->t.n & 63) ? P->t.n_tiles - 1 : INT_MAX;
    auto tile_late = [&](const unsigned char* tb, int tile, bool defer) {
        const int* tn = reinterpret_cast<const int*>(tb + kTileBytes);
#pragma unroll
        for (int u2 = 0; u2 < 2; ++u2) {
            const int row0 = tile * 64 + 32 * u2;
            const unsigned pw = (unsigned)tn[64 + u2] >> (4 * h);  // bit 8j + k: n2 & 1 of the lane's row
            i32x16 acc[QT];
            if (MIM_KNN_PW_EARLY) asm volatile("" ::"v"(pw));
            block_mfma(tb, u2, acc);
            // the parity word is read with the seeds (its LDS latency hidden behind the MFMAs), not
            // inside the rare insertion path where the compiler would sink it: one LDS round trip per event
            if (!MIM_KNN_PW_EARLY) asm volatile("" ::"v"(pw));
            if (MIM_KNN_PROBE >= 2) {
#pragma unroll
                for (int u = 0; u < QT; ++u) asm volatile("" ::"v"(acc[u]));
                continue;
            }
            if (defer && u2 == 1) {
#pragma unroll
                for (int u = 0; u < QT; ++u) dacc[u] = acc[u];
                dpw = pw;
                drow0 = row0;
                dkeyed = tile != pad_tile;
                continue;
            }
            half_filter(acc, pw, row0, tile != pad_tile);
        }
    };
    auto flush_deferred = [&]() {
        if (stagger && drow0 >= 0) {
            half_filter(dacc, dpw, drow0, dkeyed);
            drow0 = -1;
        }
    };

    int stage = w.tile0;
    for (; stage < tile_e; stage += kStage) {
        const int buf = ((stage - w.tile0) / kStage) & 1;
        const bool more = stage + kStage < w.tile1;
        if (more) stage_dma(stage + kStage, buf ^ 1, stage + kStage < tile_e);
        const unsigned char* sb = smem + buf * kStage * kLdsTile;
#pragma unroll
        for (int ts = 0; ts < kStage; ++ts)
            if (live && (kStage == 1 || stage + ts < w.tile1)) tile_early(sb + ts * kLdsTile, stage + ts);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's DMA into the next buffer landed
        __syncthreads();
    }
    for (int ls = 0; stage < w.tile1; stage += kStage, ++ls) {  // ls: the sweep's late stages, counted from 0
        const int buf = ((stage - w.tile0) / kStage) & 1;
        const bool more = stage + kStage < w.tile1;
        // a stage off the refresh schedule skips what only feeds refresh(): the c(q) read, the exchange
        // (o1c, o2c keep their last values) and the limit arithmetic; T[u] stays as the last refresh and
        // the events since left it.  The first late stage (ls = 0) always refreshes.
        const bool fresh = kRefreshEvery == 1 || ls < kRefreshDense || ls % kRefreshEvery == 0;
        // c(q) for the refresh, read before the next stage's DMA is issued: an LDS read after it
        // would wait for that DMA (the waitcnt pass cannot tell the words apart)
        int cqv[QT];
        if (live && fresh) {
#pragma unroll
            for (int u = 0; u < QT; ++u) cqv[u] = RATIO ? cq[32 * u] : 0;
        }
        if (more) stage_dma(stage + kStage, buf ^ 1, false);
        const unsigned char* sb = smem + buf * kStage * kLdsTile;
        auto refresh = [&]() {  // thresholds from the partner lane's current m1, m2 (every tile: slower, r03bd)
#pragma unroll
            for (int u = 0; u < QT; ++u) {
                const auto a = __builtin_amdgcn_permlane32_swap(st[u].m1, st[u].m1, false, false);
                const auto b = __builtin_amdgcn_permlane32_swap(st[u].m2, st[u].m2, false, false);
                o1c[u] = (tid & 32) ? (int)a[0] : (int)a[1];
                o2c[u] = (tid & 32) ? (int)b[0] : (int)b[1];
                if (FLIP) {
                    // surely failing: the test fails for the smallest first and the largest second value
                    // the pair's two values can stand for.  Its limit is the flip limit: a row passes against
                    // the first value only if (float)(2 R + p + c) < tf, so R <= (ceil(tf) - c) >> 1 holds
                    // every such row (d^2 < 2^24 is exact in float); never above the rows under the minimum
                    const int e1 = pair_first(st[u], o1c[u]), e2 = pair_second(st[u], o1c[u], o2c[u]);
                    const int c = cqv[u];
                    const float tf = kappa * (float)(e_hi(e1) + c);
                    const bool fail = e2 != INT_MAX && (float)((e_hi(e1) & ~1) + c) >= kappa * (float)(e_hi(e2) + c);
                    const int flip = min(((int)ceilf(tf) - c) >> 1, below_threshold(e_hi(e1)));
                    T[u] = fail ? flip : below_threshold(e_hi(e2));
                } else if (RATIO) {
                    // the pair's two smallest D, both halves fresh: exact or failing (invariant above)
                    const int q1 = pair_first(st[u], o1c[u]), q2 = pair_second(st[u], o1c[u], o2c[u]);
                    const int c = cqv[u];
                    const bool fail = q2 != INT_MAX && (float)(q1 + c) >= kappa * (float)(q2 + c);
                    T[u] = below_threshold(fail ? q1 : q2);
                } else {
                    T[u] = late_threshold(st[u], o1c[u], o2c[u]);
                }
            }
        };
        if (live) {
            flush_deferred();  // the previous stage's last half tile (waves 4-7 with MIM_KNN_STAGGER)
            if (fresh) refresh();
            // rolled by default (unrolling measured no faster; the late tile is ~3 KiB of code)
#pragma unroll MIM_KNN_LATE_UNROLL
            for (int ts = 0; ts < kStage; ++ts)
                if (kStage == 1 || stage + ts < w.tile1)
                    tile_late(sb + ts * kLdsTile, stage + ts, stagger && (ts == kStage - 1 || stage + ts + 1 == w.tile1));
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's DMA into the next buffer landed
        __syncthreads();
    }
    flush_deferred();

    // ---- merge the two lane halves (disjoint train rows of the same query), keys ----
    if (!live) continue;  // nothing to store (q >= nq in every lane); the next item's barriers come after
#pragma unroll
    for (int u = 0; u < QT; ++u) {
        LaneSel m = st[u];
        if (m.i1 != INT_MAX) m.i1 += 4 * h;
        if (!RATIO && m.i2 != INT_MAX) m.i2 += 4 * h;
        LaneSel o;
        o.m1 = __shfl_xor(m.m1, 32); o.m2 = __shfl_xor(m.m2, 32);
        o.i1 = __shfl_xor(m.i1, 32); o.i2 = RATIO ? INT_MAX : __shfl_xor(m.i2, 32);
        if (RATIO) {
            m = sel_merge_r(m, o);
            m.i2 = m.m2 == INT_MAX ? INT_MAX : m.i1;  // any valid index: only k2 is read downstream
        } else {
            m = sel_merge(m, o);
        }
        const int q = qbase + 32 * u + r;
        if (h == 0 && q < nq) {
            // c(q), read here rather than held in a register for the whole sweep
            const int qq = ((const gint*)P->q.norm)[(size_t)(q >> 6) * kNormWords + 128 + (q & 63)];
            Top2 t;
            // exact d^2 = D + c(q) (< 2^23); verdict mode: the largest d^2 the values can stand for
            const int d1 = (FLIP ? e_hi(m.m1) : m.m1) + qq, d2 = (FLIP ? e_hi(m.m2) : m.m2) + qq;
            t.k1 = m.i1 == INT_MAX ? FLT_MAX : sqrtf((float)d1);
            t.k2 = m.i2 == INT_MAX ? FLT_MAX : sqrtf((float)d2);
            t.i1 = m.i1;
            t.i2 = m.i2;
            if (FLIP && m.i2 != INT_MAX) {
                // the ratio kernel's test at the bounds of what the two values can stand for: the first at
                // its lower bound (a tracked 2 R + 1 may be 2 R), the second at its upper bound and at the
                // even value under it (a row of the same R and even parity may have gone by unrecorded)
                const float ratio = KnnRatioArg<MODE>::ratio(karg);
                const int h1 = d1, l1 = max(h1 - (m.m1 & 1), 0), h2 = d2, l2 = max(h2 - (e_hi(m.m2) & 1), 0);
                const bool p_opt = sqrtf((float)l1) < ratio * sqrtf((float)h2);
                const bool p_pes = sqrtf((float)h1) < ratio * sqrtf((float)l2);
                t.k1 = sqrtf((float)h1);
                t.k2 = sqrtf((float)l2);
                if (!p_opt) t.k2 = t.k1;                                 // fails whatever the parities: k1 >= k2
                else if (!p_pes || (m.m1 & 1)) t.i2 = kRescan;           // undecided here: the exact rescan decides
            }
            // d^2 >= 4e6: distinct integers may share a key (sqrt class), where the lower index
            // wins: rescan exactly.  Below, equal keys mean equal d^2, already in index order.
            // (ratio mode: the test reads the two smallest keys as values, and those are the keys of
            // the two smallest d^2 in any sqrt class: no rescan)
            if (!RATIO && t.i2 != INT_MAX && d2 >= 4000000) t.i2 = kRescan;
            parts[P->part_off + (long long)w.split * P->q_pad + q] = t;
        }
    }
  }
}


// ------------------------------------------------------------------------------------------------
// Exact rescan of the queries the distance kernel marked (kRescan): one wave per query over the
// work item's train rows, fp32 distances of integer rows (exact in any order), keys sqrtf(d^2),
// (key, index) order.  Rare: the marked queries have a 3rd row in the 2nd key's sqrt class.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void knn2_rescan_kernel(const ProbDev* __restrict__ probs,
                                                          const KnnWork* __restrict__ works,
                                                          Top2* __restrict__ parts) {
    const KnnWork w = works[blockIdx.x];
    const ProbDev* P = probs + w.problem;
    if (*P->q.flags | *P->t.flags) return;  // generic kernel's parts are exact already
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int nq = P->q.n, nt = P->t.n;
    Top2* out = parts + P->part_off + (long long)w.split * P->q_pad;
    const int r0 = w.tile0 * 64, r1 = min(w.tile1 * 64, nt);
    for (int k = 0; k < kKnnBlockQ; k += 64) {
        const int q = w.q0 + k + lane;
        const bool marked = q < nq && out[q].i2 == kRescan;
        unsigned long long m = __ballot(marked);
        // a marked query belongs to the wave its position names.  (Not round-robin over the marks a wave
        // sees: the waves read the marks at different times, and one that has already rewritten a record
        // clears that mark for the waves behind it, which then counted differently and left a query to
        // nobody.)
        while (m) {
            const int b = __builtin_ctzll(m);
            m &= m - 1;
            if ((b & 3) != wave) continue;
            const int qq = w.q0 + k + b;
            const float* qv = P->q.f32 + (size_t)qq * kDim;
            T2 t{FLT_MAX, INT_MAX, FLT_MAX, INT_MAX};
            for (int row = r0 + lane; row < r1; row += 64) {
                const float* tv = P->t.f32 + (size_t)row * kDim;
                float d2 = 0.f;
                for (int c = 0; c < kDim; ++c) {
                    const float d = qv[c] - tv[c];
                    d2 = fmaf(d, d, d2);  // integer terms, partial sums < 2^24: exact
                }
                t = top2_merge(t, sqrtf(d2), row);
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const float ok1 = __shfl_xor(t.k1, off), ok2 = __shfl_xor(t.k2, off);
                const int oi1 = __shfl_xor(t.i1, off), oi2 = __shfl_xor(t.i2, off);
                t = top2_merge(t, ok1, oi1);
                t = top2_merge(t, ok2, oi2);
            }
            if (lane == 0) out[qq] = Top2{t.k1, t.i1, t.k2, t.i2};
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Generic fp32 path: one thread per query, train rows broadcast from LDS, OpenCV SSE summation
// order (core/src/norm.cpp normL2Sqr_: 4 accumulators x 4 lanes, v_reduce_sum (a0+a2)+(a1+a3)).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float l2sqr_sse_order(const float* q, const float* t) {
    float acc[4][4];
#pragma unroll
    for (int v = 0; v < 4; ++v)
#pragma unroll
        for (int l = 0; l < 4; ++l) acc[v][l] = 0.f;
#pragma unroll
    for (int j = 0; j < kDim; j += 16) {
#pragma unroll
        for (int v = 0; v < 4; ++v)
#pragma unroll
            for (int l = 0; l < 4; ++l) {
                const float d = q[j + 4 * v + l] - t[j + 4 * v + l];
                acc[v][l] = __fadd_rn(__fmul_rn(d, d), acc[v][l]);
            }
    }
    float s[4];
#pragma unroll
    for (int l = 0; l < 4; ++l) s[l] = ((acc[0][l] + acc[1][l]) + acc[2][l]) + acc[3][l];
    return (s[0] + s[2]) + (s[1] + s[3]);
}

__global__ __launch_bounds__(256) void knn2_f32_kernel(const ProbDev* __restrict__ probs,
                                                       const KnnWork* __restrict__ works,
                                                       Top2* __restrict__ parts, int n_works) {
    __shared__ __attribute__((aligned(16))) float tl[kTileRows * kDim];
    // grid-stride over the work items: the grid is capped (knn_launch), since nearly every item is
    // integer-valued and exits at the flag test; one early-exit block per item (32 KiB of LDS, 128
    // query VGPRs) cost ~0.12 ms of dispatch per C3 batch
  for (int wi = blockIdx.x; wi < n_works; wi += gridDim.x) {
    const KnnWork w = works[wi];
    const ProbDev* P = probs + w.problem;
    if (!(*P->q.flags | *P->t.flags)) continue;  // integer-valued: exact MFMA kernel handles it (block-uniform)
    const int tid = threadIdx.x;
    const int nq = P->q.n, nt = P->t.n;
  for (int qo = 0; qo < kKnnBlockQ; qo += 256) {  // the work item's queries, 256 per pass
    const int q = w.q0 + qo + tid;
    float qv[kDim];
    const bool qvalid = q < nq;
#pragma unroll
    for (int c = 0; c < kDim; c += 4) {
        float4 v = qvalid ? *reinterpret_cast<const float4*>(P->q.f32 + (size_t)q * kDim + c)
                          : make_float4(0.f, 0.f, 0.f, 0.f);
        qv[c] = v.x; qv[c + 1] = v.y; qv[c + 2] = v.z; qv[c + 3] = v.w;
    }
    float k1 = FLT_MAX, k2 = FLT_MAX;
    int i1 = INT_MAX, i2 = INT_MAX;
    for (int tile = w.tile0; tile < w.tile1; ++tile) {
        __syncthreads();
        for (int e = tid; e < kTileRows * kDim / 4; e += 256) {
            const int row = tile * 64 + e / (kDim / 4);
            float4 v = row < nt ? reinterpret_cast<const float4*>(P->t.f32)[(size_t)tile * 64 * (kDim / 4) + e]
                                : make_float4(0.f, 0.f, 0.f, 0.f);
            reinterpret_cast<float4*>(tl)[e] = v;
        }
        __syncthreads();
        const int rows = min(64, nt - tile * 64);
        for (int rr = 0; rr < rows; ++rr) {
            const float d = sqrtf(l2sqr_sse_order(qv, tl + rr * kDim));
            // OpenCV compares the bit patterns as int: for non-negative floats that is float order;
            // NaN (> FLT_MAX bits) and values >= FLT_MAX are never inserted.
            if (d < k2) {
                const int j = tile * 64 + rr;
                if (d < k1) { k2 = k1; i2 = i1; k1 = d; i1 = j; }
                else { k2 = d; i2 = j; }
            }
        }
    }
    if (qvalid) parts[P->part_off + (long long)w.split * P->q_pad + q] = Top2{k1, i1, k2, i2};
  }
    __syncthreads();  // the next work item's first tile load overwrites tl
  }
}

// ------------------------------------------------------------------------------------------------
// Merge train splits, emit knnMatch rows, Lowe ratio test and ordered compaction
// (TestsDetector.cpp:62-72): survivors keep ascending query order — the order findHomography's
// point lists and inlier mask are indexed by.  One 1024-thread block per problem.
// Output pts[k] = (objPt.x, objPt.y, scenePt.x, scenePt.y) of the k-th good match.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void ratio_compact_kernel(const ProbDev* __restrict__ probs,
                                                            const Top2* __restrict__ parts, float ratio,
                                                            int32_t* __restrict__ good_q,
                                                            int32_t* __restrict__ good_t,
                                                            float4* __restrict__ pts,
                                                            int* __restrict__ n_good,
                                                            int32_t* __restrict__ knn_idx,
                                                            float* __restrict__ knn_dist) {
    __shared__ int wsum[16];
    __shared__ int wbase[17];
    const ProbDev* P = probs + blockIdx.x;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int nq = P->q.n;
    int running = 0;
    for (int base = 0; base < nq; base += 1024) {
        const int q = base + tid;
        T2 m{FLT_MAX, INT_MAX, FLT_MAX, INT_MAX};
        if (q < nq) {
            for (int sp = 0; sp < P->nsplit; ++sp) {
                const Top2 t = parts[P->part_off + (long long)sp * P->q_pad + q];
                m = top2_merge(m, t.k1, t.i1);
                m = top2_merge(m, t.k2, t.i2);
            }
        }
        const float k1 = m.k1, k2 = m.k2;
        const int i1 = m.i1, i2 = m.i2;
        if (q < nq) {
            if (knn_idx) {
                knn_idx[2 * q] = i1 == INT_MAX ? -1 : i1;
                knn_idx[2 * q + 1] = i2 == INT_MAX ? -1 : i2;
                knn_dist[2 * q] = k1;
                knn_dist[2 * q + 1] = k2;
            }
        }
        const bool good = q < nq && i1 != INT_MAX && i2 != INT_MAX && k1 < ratio * k2;
        const unsigned long long bal = __ballot(good);
        const int within = __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32),
                                                     __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0));
        if (lane == 0) wsum[wave] = __popcll(bal);
        __syncthreads();
        if (tid == 0) {
            int acc = 0;
            for (int i = 0; i < 16; ++i) { wbase[i] = acc; acc += wsum[i]; }
            wbase[16] = acc;
        }
        __syncthreads();
        if (good) {
            const long long o = P->good_off + running + wbase[wave] + within;
            good_q[o] = q;
            good_t[o] = i1;
            const float2 a = P->q.kp[q], b = P->t.kp[i1];
            pts[o] = make_float4(a.x, a.y, b.x, b.y);
        }
        running += wbase[16];
        __syncthreads();
    }
    if (tid == 0) n_good[blockIdx.x] = running;
}

// ------------------------------------------------------------------------------------------------
// Cross-check filter (BFMatcher(norm, crossCheck = true).match) in the shape of
// ratio_compact_kernel: per query, merge the forward splits, look up the reverse nearest row of its
// nearest train row i1 (the shadow problem's partials at row i1, or the fused Hamming kernel's column
// minimum), keep the pair iff that is the query itself (filter 1), and the ratio test holds as well
// (filter 2); then the same ordered compaction, point gather and n_good.  match_idx / match_dist
// (mim_match_cross_sets): per query the matched train row or -1, its distance or FLT_MAX.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void cross_compact_kernel(const ProbDev* __restrict__ probs,
                                                            const CrossDev* __restrict__ cross,
                                                            const Top2* __restrict__ parts, float ratio,
                                                            int filter, int32_t* __restrict__ good_q,
                                                            int32_t* __restrict__ good_t,
                                                            float4* __restrict__ pts,
                                                            int* __restrict__ n_good,
                                                            int32_t* __restrict__ match_idx,
                                                            float* __restrict__ match_dist) {
    __shared__ int wsum[16];
    __shared__ int wbase[17];
    const ProbDev* P = probs + blockIdx.x;
    const CrossDev X = cross[blockIdx.x];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int nq = P->q.n;
    int running = 0;
    for (int base = 0; base < nq; base += 1024) {
        const int q = base + tid;
        T2 m{FLT_MAX, INT_MAX, FLT_MAX, INT_MAX};
        if (q < nq) {
            for (int sp = 0; sp < P->nsplit; ++sp) {
                const Top2 t = parts[P->part_off + (long long)sp * P->q_pad + q];
                m = top2_merge(m, t.k1, t.i1);
                m = top2_merge(m, t.k2, t.i2);
            }
        }
        const float k1 = m.k1, k2 = m.k2;
        const int i1 = m.i1, i2 = m.i2;
        int back = -1;  // the lowest query row nearest to train row i1
        if (q < nq && i1 != INT_MAX) {
            if (X.colmin) {
                const uint32_t key = X.colmin[i1];
                back = key == 0xFFFFFFFFu ? -1 : (int)(key & 0x3FFFFu);
            } else {
                const ProbDev* S = probs + X.shadow;
                T2 r{FLT_MAX, INT_MAX, FLT_MAX, INT_MAX};
                for (int sp = 0; sp < S->nsplit; ++sp) {
                    const Top2 t = parts[S->part_off + (long long)sp * S->q_pad + i1];
                    r = top2_merge(r, t.k1, t.i1);
                    r = top2_merge(r, t.k2, t.i2);
                }
                back = r.i1 == INT_MAX ? -1 : r.i1;
            }
        }
        const bool good = q < nq && i1 != INT_MAX && back == q && (filter == 1 || (i2 != INT_MAX && k1 < ratio * k2));
        if (q < nq && match_idx) {
            match_idx[q] = good ? i1 : -1;
            match_dist[q] = good ? k1 : FLT_MAX;
        }
        const unsigned long long bal = __ballot(good);
        const int within = __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32),
                                                     __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0));
        if (lane == 0) wsum[wave] = __popcll(bal);
        __syncthreads();
        if (tid == 0) {
            int acc = 0;
            for (int i = 0; i < 16; ++i) { wbase[i] = acc; acc += wsum[i]; }
            wbase[16] = acc;
        }
        __syncthreads();
        if (good) {
            const long long o = P->good_off + running + wbase[wave] + within;
            good_q[o] = q;
            good_t[o] = i1;
            const float2 a = P->q.kp[q], b = P->t.kp[i1];
            pts[o] = make_float4(a.x, a.y, b.x, b.y);
        }
        running += wbase[16];
        __syncthreads();
    }
    if (tid == 0) n_good[blockIdx.x] = running;
}

// ------------------------------------------------------------------------------------------------
// knnMatch rows alone (mim_knn2_l2 / mim_knn2_sets_dev): merge the train splits of every query of
// one problem, one thread per query over the whole grid (no ratio test, no compaction).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void knn_emit_kernel(const ProbDev* __restrict__ probs,
                                                      const Top2* __restrict__ parts,
                                                      int32_t* __restrict__ knn_idx, float* __restrict__ knn_dist) {
    const ProbDev* P = probs;
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= P->q.n) return;
    T2 m{FLT_MAX, INT_MAX, FLT_MAX, INT_MAX};
    for (int sp = 0; sp < P->nsplit; ++sp) {
        const Top2 t = parts[P->part_off + (long long)sp * P->q_pad + q];
        m = top2_merge(m, t.k1, t.i1);
        m = top2_merge(m, t.k2, t.i2);
    }
    reinterpret_cast<int2*>(knn_idx)[q] = make_int2(m.i1 == INT_MAX ? -1 : m.i1, m.i2 == INT_MAX ? -1 : m.i2);
    reinterpret_cast<float2*>(knn_dist)[q] = make_float2(m.k1, m.k2);
}

// ------------------------------------------------------------------------------------------------
// allUnfilteredScenePts of a batch (TestsDetector.cpp:87-94): for every accepted problem, the scene
// keypoints of its RANSAC inliers in mask order, divided by the problem's scale in float when it is
// not 1 (scalePoints, :48-55), at offs[i] (the host's prefix sum of the accepted problems' n_inl).
// One 256-thread block per problem; ordered compaction by wave ballots.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void inlier_gather_kernel(const ProbDev* __restrict__ probs,
                                                          const mim_result* __restrict__ res,
                                                          const int32_t* __restrict__ good_t,
                                                          const uint8_t* __restrict__ masks,
                                                          const long long* __restrict__ offs,
                                                          const float* __restrict__ scales,
                                                          float2* __restrict__ out) {
    __shared__ int wsum[4];
    const int i = blockIdx.x;
    if (res[i].status != MIM_ACCEPTED) return;  // block-uniform
    const ProbDev* P = probs + i;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int ng = res[i].n_good;
    const float s = scales ? scales[i] : 1.0f;
    long long o = offs[i];
    for (int base = 0; base < ng; base += 256) {
        const int k = base + tid;
        const bool in = k < ng && masks[P->good_off + k] != 0;
        const unsigned long long bal = __ballot(in);
        const int within = __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0));
        if (lane == 0) wsum[wave] = __popcll(bal);
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            before += w < wave ? wsum[w] : 0;
            all += wsum[w];
        }
        if (in) {
            float2 p = P->t.kp[good_t[P->good_off + k]];
            if (s != 1.0f) {  // pt.x /= scale; pt.y /= scale (IEEE float division)
                p.x = __fdiv_rn(p.x, s);
                p.y = __fdiv_rn(p.y, s);
            }
            out[o + before + within] = p;
        }
        o += all;
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------
// host-side launchers (called from api.cpp)
// ------------------------------------------------------------------------------------------------
void launch_prep_batch(const PrepJob* jobs, int njobs, int total_tiles, hipStream_t st) {
    if (njobs > 0 && total_tiles > 0) prep_batch_kernel<<<total_tiles, 256, 0, st>>>(jobs, njobs);
}

// Both kernels are enqueued; each block reads its problem's integrality flags (set by prep on the
// device) and only the matching kernel does the work, so no host round trip is needed.
int knn_blocks_per_cu() {
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, knn2_i8_kernel<0>, kThreads, 0) != hipSuccess) nb = 1;
    return nb;
}

void launch_knn(const ProbDev* probs, const KnnWork* works, int n_works, const int* seg_start, int n_blocks,
                Top2* parts, int* dyn_ctr, float kappa, float flip_ratio, hipStream_t st) {
    if (n_works <= 0) return;
    if (dyn_ctr) (void)hipMemsetAsync(dyn_ctr, 0, 8 * sizeof(int), st);
    // kappa in (0, 1): the ratio-mode instantiation (its parts feed ratio_compact_kernel only and
    // mark nothing for the rescan); otherwise the exact top-2
    // flip_ratio > 0 (whole sweeps of one split only): the verdict-mode instantiation, whose records are
    // final verdicts; the few it leaves undecided are marked for the rescan
    if (kappa > 0.f && kappa < 1.f && flip_ratio > 0.f) {
        knn2_i8_kernel<2><<<n_blocks, kThreads, 0, st>>>(probs, works, seg_start, parts, dyn_ctr,
                                                         make_float2(kappa, flip_ratio));
        knn2_rescan_kernel<<<n_works, 256, 0, st>>>(probs, works, parts);
    } else if (kappa > 0.f && kappa < 1.f) {
        knn2_i8_kernel<1><<<n_blocks, kThreads, 0, st>>>(probs, works, seg_start, parts, dyn_ctr, kappa);
    } else {
        knn2_i8_kernel<0><<<n_blocks, kThreads, 0, st>>>(probs, works, seg_start, parts, dyn_ctr, 0.f);
        knn2_rescan_kernel<<<n_works, 256, 0, st>>>(probs, works, parts);
    }
    knn2_f32_kernel<<<std::min(n_works, 2048), 256, 0, st>>>(probs, works, parts, n_works);
}

void launch_inlier_gather(const ProbDev* probs, int n, const mim_result* res, const int32_t* good_t,
                          const uint8_t* masks, const long long* offs, const float* scales, float2* out, hipStream_t st) {
    if (n > 0) inlier_gather_kernel<<<n, 256, 0, st>>>(probs, res, good_t, masks, offs, scales, out);
}

void launch_knn_emit(const ProbDev* probs, int nq, const Top2* parts, int32_t* knn_idx, float* knn_dist,
                     hipStream_t st) {
    if (nq > 0) knn_emit_kernel<<<(nq + 255) / 256, 256, 0, st>>>(probs, parts, knn_idx, knn_dist);
}

void launch_ratio(const ProbDev* probs, int n_probs, const Top2* parts, float ratio, int32_t* good_q,
                  int32_t* good_t, float4* pts, int* n_good, int32_t* knn_idx, float* knn_dist,
                  hipStream_t st) {
    if (n_probs > 0)
        ratio_compact_kernel<<<n_probs, 1024, 0, st>>>(probs, parts, ratio, good_q, good_t, pts, n_good,
                                                       knn_idx, knn_dist);
}

void launch_cross(const ProbDev* probs, const CrossDev* cross, int n_probs, const Top2* parts, float ratio, int filter,
                  int32_t* good_q, int32_t* good_t, float4* pts, int* n_good, int32_t* match_idx, float* match_dist,
                  hipStream_t st) {
    if (n_probs > 0)
        cross_compact_kernel<<<n_probs, 1024, 0, st>>>(probs, cross, parts, ratio, filter, good_q, good_t, pts, n_good,
                                                       match_idx, match_dist);
}

}  // namespace mim
