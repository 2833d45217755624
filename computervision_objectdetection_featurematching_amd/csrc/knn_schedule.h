// knn_schedule.h — the distance kernels' work lists as a pure function of a few integers per problem.
// Host only and HIP-free (a plain C++17 compiler builds tests/cpp/knn_schedule_driver.cpp over it);
// mim_internal.h includes it, so the kernels see the same KnnWork and block constants.
#pragma once
#include <algorithm>
#include <vector>

namespace mim {

#ifndef MIM_KNN_QT
#define MIM_KNN_QT 2
#endif

#ifndef MIM_KNN_WAVES
#define MIM_KNN_WAVES 8
#endif
constexpr int kKnnQT = MIM_KNN_QT;             // 32-query MFMA column tiles per wave (distance kernel)
constexpr int kKnnWaves = MIM_KNN_WAVES;       // waves per distance-kernel block
constexpr int kKnnMinChunk = 8;                // fewest train tiles per distance-kernel block
#ifndef MIM_KNN_SUB_TILES
#define MIM_KNN_SUB_TILES -1
#endif
constexpr int kKnnSubTiles = MIM_KNN_SUB_TILES;  // distance schedule's sub-chunk target (knn_schedule_static)
constexpr int kKnnBlockQ = kKnnWaves * 32 * kKnnQT;  // queries per distance-kernel work item

// Segment of the distance kernel: kKnnBlockQ queries x a train tile range of one problem, written
// to train split `split`.  A block runs the segments seg_start[b] .. seg_start[b + 1] - 1
// (knn_schedule_static: one balanced chunk of the batch's tiles per resident block).
struct KnnWork {
    int problem;
    int q0;        // first query row (multiple of kKnnBlockQ)
    int tile0;     // train tiles [tile0, tile1)
    int tile1;
    int split;
};

constexpr int kHamBlockQ = 256;    // queries per Hamming work item
constexpr int kHamTileRows = 128;  // train rows per LDS stage

constexpr int kFltBlockQ = 256;  // queries per generic-float work item (one per lane, 4 waves)
constexpr int kFltRowPad = 64;   // a generic-float set's stored rows are a multiple of this; split unit
constexpr int kFltMaxDim = 512;  // widest generic-float row

// What the schedule knows of one problem.
struct KnnSchedProblem {
    int nq;       // query rows
    int nt;       // train rows
    int n_tiles;  // train tiles (SetDev::n_tiles)
    bool bin;     // binary descriptors: the Hamming work list, not the i8 schedule
    int fdim = 0; // generic float rows of this dim (mim_set_create_f32): the float work list, not the i8 schedule
    bool shadow = false;  // reverse direction of a cross-check problem (knn_cross_problems): distance stage only
};

// problems of the i8 schedule: neither binary nor generic-float
inline bool knn_is_i8(const KnnSchedProblem& p) { return !p.bin && p.fdim == 0; }

// MIM_KNN_SUB, MIM_KNN_DYN and MIM_KNN_TAIL, read by the caller.
struct KnnSchedKnobs {
    int sub_target = kKnnSubTiles;
    int dyn = -1;  // -1: decide from the sweep count; 0 / 1: forced
    bool tail = false;
};

// A problem's share of the batch's buffers (ProbDev's fields of the same names).
struct KnnSchedSlot {
    int nsplit = 0;
    int q_pad = 0;
    long long part_off = 0, good_off = 0, it_off = 0;
};

// Work item of the Hamming kernel without its pointers: kHamBlockQ queries from q0 x train rows
// [r0, r1) of one problem, written to train split `split`.
struct HamPiece {
    int problem, q0, r0, r1, split;
};

// Work item of the generic-float kernel without its pointers: kFltBlockQ queries from q0 x train rows
// [r0, r1) of one problem (r0 a multiple of kFltRowPad), written to train split `split`.
struct FltPiece {
    int problem, q0, r0, r1, split;
};

struct KnnSchedule {
    std::vector<KnnSchedSlot> slots;  // per problem
    std::vector<KnnWork> works;
    std::vector<int> seg;  // static: the blocks' first work items (n_blocks + 1); dynamic: the 8 lists' (9)
    int n_blocks = 0;      // distance-kernel blocks to launch
    bool dyn = false;
    long long part = 0, good = 0;  // Top2 partials and good-match slots over the batch
    std::vector<HamPiece> ham;
    std::vector<FltPiece> flt;
};

inline int knn_query_blocks(int nq) { return (nq + kKnnBlockQ - 1) / kKnnBlockQ; }

// Balanced distance schedule.  The (problem, query block, train tile) units are cut into equal
// sub-chunks, every resident block of the single wave of blocks doing the same number of tiles
// (no tail wave).  A query block cut into k pieces gets k train splits (partial top-2 lists merged
// by the ratio kernel); a problem's split count is the largest over its query blocks, and the
// missing splits of the others are empty work items (sentinel lists).
// L2 locality (MIM_KNN_SUB = s > 0, tiles): with the chunk of a block longer than s, the block
// does R = ceil(chunk / s) sub-chunks of ~s tiles in rounds, and a problem's train tiles are
// ordered in segments of <= s tiles (units: problem, segment, query block, tile), so the blocks
// running at one time on an XCD sweep the same few segments of the same one or two problems.
// Placement: workgroups are dispatched round-robin over the 8 XCDs (block b on XCD b % 8), and
// XCD x gets the x-th eighth of the sub-chunks.  MIM_KNN_SUB = 0: segments of <= chunk tiles, one
// round; < 0: whole query-block sweeps, one round.
inline void knn_schedule_static(const std::vector<KnnSchedProblem>& in, long long G, int sub_target, KnnSchedule& S) {
    const int n = (int)in.size();
    long long units = 0;
    for (int i = 0; i < n; ++i)
        if (knn_is_i8(in[i])) units += (long long)knn_query_blocks(in[i].nq) * in[i].n_tiles;
    const long long chunk = std::max<long long>(kKnnMinChunk, (units + G - 1) / G);
    const long long R = (sub_target > 0 && chunk > sub_target) ? (chunk + sub_target - 1) / sub_target : 1;
    const long long sub = std::max<long long>(kKnnMinChunk, (chunk + R - 1) / R);
    const long long NS = std::max<long long>(1, (units + sub - 1) / sub);  // sub-chunks
    const long long per_x = (NS + 7) / 8;
    const int m = (int)std::max<long long>(1, (per_x + R - 1) / R);  // blocks per XCD
    const int nphys = NS < 8 ? (int)NS : 8 * m;
    auto owner = [&](long long j) -> int {
        if (NS < 8) return (int)j;
        const long long x = j / per_x, jj = j % per_x;
        return (int)(8 * (jj % m) + x);
    };
    std::vector<std::vector<KnnWork>> blk(nphys);
    long long pos = 0;
    struct Piece { int b, t0, t1, k, owner; };
    std::vector<Piece> pieces;
    std::vector<int> cnt, last_owner;
    for (int i = 0; i < n; ++i) {
        if (!knn_is_i8(in[i])) continue;
        const int qb = knn_query_blocks(in[i].nq), nt = in[i].n_tiles;
        const int nseg = (sub_target >= 0 && nt > sub) ? (int)((nt + sub - 1) / sub) : 1;
        const int lseg = nseg > 1 ? (nt + nseg - 1) / nseg : nt;
        pieces.clear();
        cnt.assign(qb, 0);
        last_owner.assign(qb, owner(std::min(NS - 1, pos / sub)));
        for (int sg = 0; sg < nseg; ++sg) {
            const int s0 = sg * lseg, s1 = std::min(nt, s0 + lseg);
            for (int b = 0; b < qb && s0 < s1; ++b) {
                const long long u0 = pos, u1 = pos + (s1 - s0);
                for (long long a = u0; a < u1;) {
                    const long long e = std::min(u1, (a / sub + 1) * sub);
                    const int o = owner(std::min(NS - 1, a / sub));
                    pieces.push_back(Piece{b, s0 + (int)(a - u0), s0 + (int)(e - u0), cnt[b]++, o});
                    last_owner[b] = o;
                    a = e;
                }
                pos = u1;
            }
        }
        int nsplit = 1;
        for (int b = 0; b < qb; ++b) nsplit = std::max(nsplit, cnt[b]);
        S.slots[i].nsplit = nsplit;
        S.slots[i].q_pad = qb * kKnnBlockQ;
        for (const Piece& pc : pieces) blk[pc.owner].push_back(KnnWork{i, pc.b * kKnnBlockQ, pc.t0, pc.t1, pc.k});
        for (int b = 0; b < qb; ++b)
            for (int k = cnt[b]; k < nsplit; ++k)
                blk[last_owner[b]].push_back(KnnWork{i, b * kKnnBlockQ, nt, nt, k});  // empty split
    }
    S.seg.assign(nphys + 1, 0);
    for (int b = 0; b < nphys; ++b) {
        S.seg[b] = (int)S.works.size();
        S.works.insert(S.works.end(), blk[b].begin(), blk[b].end());
    }
    S.seg[nphys] = (int)S.works.size();
    S.n_blocks = nphys;
}

// MIM_KNN_DYN=1: whole query-block sweeps (one split per problem), in unit order, as 8 contiguous
// lists of about equal work (one per XCD); the resident blocks pull them (knn2_i8_kernel).
// The tail: when the sweeps do not fill the last round of the G resident blocks (a per-GPU shard
// of 32 C4 problems is 640 sweeps over 512 blocks: two rounds, the second a quarter full), the
// trailing problems covering that remainder are cut into k train-tile pieces per query block
// (k ~ G / their sweeps, <= 8), which every list holds after its whole sweeps: the blocks
// that finish early pull pieces and the kernel ends near sweeps / G rounds instead of the
// ceiling (each piece repeats the keyed early tiles and the prologue, a few per cent of a
// sweep; partial top-2 lists merged by the ratio kernel).  Opt-in (MIM_KNN_TAIL=1): it shortens a
// batch alone (32-problem shard: 0.48 -> 0.45 ms) but costs throughput once batches overlap (the
// pieces' extra early tiles and merge work: 32-problem shard with 12 in flight 26.8k -> 25.5k
// problems/s, profiles/r05i_*), and the bench keeps batches in flight.
inline void knn_schedule_dynamic(const std::vector<KnnSchedProblem>& in, long long G, long long n_sweeps, bool tail_on,
                                 KnnSchedule& S) {
    const int n = (int)in.size();
    const long long rem = n_sweeps % G;
    int tail_from = n, ksplit = 1;
    if (tail_on && n_sweeps > G && rem > 0) {
        long long ts = 0;
        while (tail_from > 0 && ts < rem) {
            --tail_from;
            if (knn_is_i8(in[tail_from])) ts += knn_query_blocks(in[tail_from].nq);
        }
        ksplit = (int)std::max<long long>(2, std::min<long long>(8, (G + ts / 2) / ts));
    }
    std::vector<KnnWork> works, tail;
    long long total = 0, total_t = 0;
    for (int i = 0; i < n; ++i) {  // pieces in (problem, tile range, query block) order
        if (!knn_is_i8(in[i])) continue;
        const int qb = knn_query_blocks(in[i].nq), nt = in[i].n_tiles;
        const int k = i < tail_from ? 1 : std::min(ksplit, std::max(nt, 1));
        S.slots[i].nsplit = k;
        S.slots[i].q_pad = qb * kKnnBlockQ;
        if (i < tail_from) {
            for (int b = 0; b < qb; ++b) works.push_back(KnnWork{i, b * kKnnBlockQ, 0, nt, 0});
            total += (long long)qb * nt;
        } else {
            for (int j = 0; j < k; ++j)
                for (int b = 0; b < qb; ++b) tail.push_back(KnnWork{i, b * kKnnBlockQ, j * nt / k, (j + 1) * nt / k, j});
            total_t += (long long)qb * nt;
        }
    }
    // 8 lists, each [its eighth of the whole sweeps | its eighth of the pieces], equal work per part
    auto cuts = [&](const std::vector<KnnWork>& v, long long tot) {
        std::vector<int> cut(9, (int)v.size());
        cut[0] = 0;
        long long acc = 0;
        int x = 1;
        for (size_t k = 0; k < v.size() && x < 8; ++k) {
            acc += v[k].tile1 - v[k].tile0;
            while (x < 8 && acc * 8 >= tot * x) cut[x++] = (int)k + 1;
        }
        return cut;
    };
    const std::vector<int> cw = cuts(works, total), ct = cuts(tail, total_t);
    S.works.reserve(works.size() + tail.size());
    S.seg.assign(9, 0);
    for (int x = 0; x < 8; ++x) {
        S.seg[x] = (int)S.works.size();
        S.works.insert(S.works.end(), works.begin() + cw[x], works.begin() + cw[x + 1]);
        S.works.insert(S.works.end(), tail.begin() + ct[x], tail.begin() + ct[x + 1]);
    }
    S.seg[8] = (int)S.works.size();
    S.n_blocks = (int)std::min<long long>(G, std::max<size_t>(S.works.size(), 8));
    S.n_blocks = std::max(8, S.n_blocks / 8 * 8);
}

// Hamming work list of the binary problems: (problem, query block, train row range of one split)
inline void knn_hamming_plan(const std::vector<KnnSchedProblem>& in, int n_cu, KnnSchedule& S) {
    const int n = (int)in.size();
    long long ham_qb = 0;  // their query blocks
    for (int i = 0; i < n; ++i)
        if (in[i].bin) ham_qb += (in[i].nq + kHamBlockQ - 1) / kHamBlockQ;
    for (int i = 0; i < n; ++i) {
        if (!in[i].bin) continue;
        KnnSchedSlot& P = S.slots[i];
        // Train rows are cut into splits only while the query blocks alone would leave CUs idle (one
        // 64 x 70,000 problem must not run on one block): about four work items per CU over the
        // batch's binary problems, a split no shorter than four tiles.
        const int hq = (in[i].nq + kHamBlockQ - 1) / kHamBlockQ;
        const int tiles = (in[i].nt + kHamTileRows - 1) / kHamTileRows;
        const long long want = (4LL * n_cu + ham_qb - 1) / std::max<long long>(ham_qb, 1);
        P.nsplit = (int)std::max<long long>(1, std::min<long long>(want, tiles / 4));
        P.q_pad = std::max(hq, 1) * kHamBlockQ;
        for (int sp = 0; sp < P.nsplit; ++sp) {
            const int r0 = (int)((long long)sp * tiles / P.nsplit) * kHamTileRows;
            const int r1 = std::min(in[i].nt, (int)((long long)(sp + 1) * tiles / P.nsplit) * kHamTileRows);
            for (int b = 0; b < hq; ++b) S.ham.push_back(HamPiece{i, b * kHamBlockQ, r0, std::max(r0, r1), sp});
        }
    }
}

// Work list of the generic-float problems (knn_float.hip): (problem, query block, train row range of one
// split).  Train rows are cut into splits of whole kFltRowPad-row units only while the query blocks alone
// would leave CUs idle (fewer than four per CU over the batch's generic-float problems), a split no
// shorter than four units.  The kernel is VALU-bound, so a CU finishes its blocks one after another
// however many are resident: the common split count w is the one with the least
// ceil(items / CUs) x (rows of the longest item + kFltItemRows), the time of the CU with the most items
// (one 10,000 x 10,000 problem, 40 query blocks on 256 CUs: w = 32, 1,280 items in 5 even rounds, where
// 26 splits would leave a sixth round of 16 items).
constexpr int kFltItemRows = 24;  // an item's fixed cost in train rows (query load, first tile's insertions, launch)
inline void knn_float_plan(const std::vector<KnnSchedProblem>& in, int n_cu, KnnSchedule& S) {
    const int n = (int)in.size();
    long long flt_qb = 0;  // their query blocks
    int max_units = 0;
    for (int i = 0; i < n; ++i)
        if (in[i].fdim) {
            flt_qb += (in[i].nq + kFltBlockQ - 1) / kFltBlockQ;
            if (in[i].nq > 0) max_units = std::max(max_units, (in[i].nt + kFltRowPad - 1) / kFltRowPad);
        }
    int w_best = 1;
    if (flt_qb < 4LL * n_cu && max_units >= 8) {
        const int w_max = (int)std::min<long long>(max_units / 4, 4LL * n_cu);
        long long best = -1;
        for (int w = 1; w <= w_max; ++w) {
            long long items = 0;
            for (int i = 0; i < n; ++i)
                if (in[i].fdim) {
                    const int units = (in[i].nt + kFltRowPad - 1) / kFltRowPad;
                    items += (long long)((in[i].nq + kFltBlockQ - 1) / kFltBlockQ) * std::max(1, std::min(w, units / 4));
                }
            const long long rows = (long long)((max_units + w - 1) / w) * kFltRowPad + kFltItemRows;
            const long long cost = (items + n_cu - 1) / n_cu * rows;
            if (best < 0 || cost < best) {
                best = cost;
                w_best = w;
            }
        }
    }
    for (int i = 0; i < n; ++i) {
        if (!in[i].fdim) continue;
        KnnSchedSlot& P = S.slots[i];
        const int fq = (in[i].nq + kFltBlockQ - 1) / kFltBlockQ;
        const int units = (in[i].nt + kFltRowPad - 1) / kFltRowPad;
        P.nsplit = std::max(1, std::min(w_best, units / 4));
        P.q_pad = std::max(fq, 1) * kFltBlockQ;
        for (int sp = 0; sp < P.nsplit; ++sp) {
            const int r0 = (int)((long long)sp * units / P.nsplit) * kFltRowPad;
            const int r1 = std::min(in[i].nt, (int)((long long)(sp + 1) * units / P.nsplit) * kFltRowPad);
            for (int b = 0; b < fq; ++b) S.flt.push_back(FltPiece{i, b * kFltBlockQ, r0, std::max(r0, r1), sp});
        }
    }
}

// The problems' shares of the partials ([split][q_pad] each), the good-match arrays and the
// per-iteration arrays, in problem order; after the split counts are known.
inline void knn_layout_offsets(const std::vector<KnnSchedProblem>& in, int max_iters, KnnSchedule& S) {
    long long part = 0, good = 0, it = 0;
    for (size_t i = 0; i < in.size(); ++i) {
        KnnSchedSlot& P = S.slots[i];
        P.part_off = part;
        part += (long long)P.nsplit * P.q_pad;
        if (in[i].shadow) {  // partials only: no good-match or iteration capacity
            P.good_off = good;
            P.it_off = it;
            continue;
        }
        P.good_off = good;
        good += (std::max(in[i].nq, 1) + 31) & ~31;  // 32-aligned: the MFMA bound's point tiles
        P.it_off = it;
        it += std::max(max_iters, 1);
    }
    S.part = part;
    S.good = good;
}

// Cross-check batches: the problems followed by their shadows, a shadow being the same
// pair with the two sets swapped (nq x nt becomes nt x nq), which goes through the distance stage like any
// problem of its kind and so leaves the reverse top-2 partials [nsplit][pad(nt)].  shadow_of[i] is
// problem i's shadow in the returned list, -1 where it has none: a binary problem under `fused`, whose
// reverse nearest rows come from the one-pass kernel's column minima (hamming.hip) instead.
inline std::vector<KnnSchedProblem> knn_cross_problems(const std::vector<KnnSchedProblem>& in, bool fused,
                                                       std::vector<int>& shadow_of) {
    std::vector<KnnSchedProblem> out(in);
    shadow_of.assign(in.size(), -1);
    for (size_t i = 0; i < in.size(); ++i) {
        if (in[i].bin && fused) continue;
        KnnSchedProblem s = in[i];
        s.nq = in[i].nt;
        s.nt = in[i].nq;
        s.n_tiles = (in[i].nq + 63) / 64;  // SetDev::n_tiles of the query set
        s.shadow = true;
        shadow_of[i] = (int)out.size();
        out.push_back(s);
    }
    return out;
}

// Top-k entries (mim_knn_batch_dev): where each problem's partial lists and output rows start,
// in entries, after knn_hamming_plan / knn_float_plan set the slots' nsplit and q_pad.  A problem's partials
// are [nsplit][q_pad][k] entries in a buffer of their own; its output rows start at k times the query rows
// before it.
struct KnnTopkLayout {
    std::vector<long long> part_off, out_off;  // per problem
    long long part = 0, out = 0;               // totals
};
inline KnnTopkLayout knn_topk_offsets(const std::vector<KnnSchedProblem>& in, const std::vector<KnnSchedSlot>& slots,
                                      int k) {
    KnnTopkLayout Lo;
    Lo.part_off.resize(in.size());
    Lo.out_off.resize(in.size());
    for (size_t i = 0; i < in.size(); ++i) {
        Lo.part_off[i] = Lo.part;
        Lo.out_off[i] = Lo.out;
        Lo.part += (long long)slots[i].nsplit * slots[i].q_pad * k;
        Lo.out += (long long)std::max(in[i].nq, 0) * k;
    }
    return Lo;
}

// Train collections (mim_knn_collection_dev).  The problems of a group of images are the
// (query set, image) pairs, query set major: pair qi * n_images + j.  A pair's Hamming / float lists are
// [nsplit][q_pad][k] entries as in knn_topk_offsets; a 128-D pair also has the i8 kernel's lists,
// [2 nsplit8][q_pad8][kt] (slots8: the slots knn_schedule_static filled; two lists per split, one per lane
// half; kt = k rounded up to 4, 8 or 16, the slots of the kernel's list), behind them.  Query set qi's output rows start at k times the query rows before it, whatever the group.
struct KnnCollLayout {
    std::vector<long long> part_off;   // per pair: its Hamming / float lists
    std::vector<long long> part8_off;  // per pair: its i8 lists (with slots8)
    std::vector<long long> out_off;    // per query set
    long long part = 0, out = 0;       // totals, in entries
};
inline KnnCollLayout knn_coll_offsets(const std::vector<int>& nq, int n_images, const std::vector<KnnSchedSlot>& slots,
                                      const std::vector<KnnSchedSlot>* slots8, int k) {
    KnnCollLayout Lo;
    const int kt = k <= 4 ? 4 : k <= 8 ? 8 : 16;
    const size_t n = nq.size() * (size_t)n_images;
    Lo.part_off.resize(n);
    Lo.part8_off.assign(n, -1);
    Lo.out_off.resize(nq.size());
    for (size_t qi = 0; qi < nq.size(); ++qi) {
        Lo.out_off[qi] = Lo.out;
        Lo.out += (long long)std::max(nq[qi], 0) * k;
        for (int j = 0; j < n_images; ++j) {
            const size_t i = qi * n_images + j;
            Lo.part_off[i] = Lo.part;
            Lo.part += (long long)slots[i].nsplit * slots[i].q_pad * k;
            if (slots8) {
                Lo.part8_off[i] = Lo.part;
                Lo.part += 2LL * (*slots8)[i].nsplit * (*slots8)[i].q_pad * kt;
            }
        }
    }
    return Lo;
}

// The most entries the lists of one (query set, image) pair can take under any plan: knn_hamming_plan and
// knn_float_plan cut at most units / 4 splits (units of kHamTileRows or kFltRowPad rows), and
// knn_schedule_static cuts a query block's n_tiles at multiples of a sub-chunk of at least kKnnMinChunk tiles:
// at most n_tiles / kKnnMinChunk + 2 pieces.
inline long long knn_coll_pair_bound(int nq, int nt, bool bin, bool sift, int k) {
    const int unit = bin ? kHamTileRows : kFltRowPad, blockq = bin ? kHamBlockQ : kFltBlockQ;
    const long long splits = std::max(1, (nt + unit - 1) / unit / 4);
    long long e = splits * std::max((nq + blockq - 1) / blockq, 1) * blockq * k;
    if (sift) e += 2LL * ((nt + 63) / 64 / kKnnMinChunk + 2) * knn_query_blocks(nq) * kKnnBlockQ * (k <= 4 ? 4 : k <= 8 ? 8 : 16);
    return e;
}

// Images in groups whose partial lists fit `budget` bytes by that bound (8 bytes per entry), so that the
// partial buffer does not grow with the collection: group g is images [start[g], start[g + 1]).  An image
// that alone exceeds the budget is a group of its own.
inline std::vector<int> knn_coll_groups(const std::vector<int>& nq, const std::vector<int>& nt, bool bin, bool sift, int k,
                                        long long budget) {
    std::vector<int> start{0};
    long long used = 0;
    for (size_t j = 0; j < nt.size(); ++j) {
        long long e = 0;
        for (int q : nq) e += knn_coll_pair_bound(q, nt[j], bin, sift, k);
        if (used > 0 && (used + e) * 8 > budget) {
            start.push_back((int)j);
            used = 0;
        }
        used += e;
    }
    start.push_back((int)nt.size());
    return start;
}

// G: resident distance-kernel blocks of the device.
inline KnnSchedule knn_schedule(const std::vector<KnnSchedProblem>& in, int G, int n_cu, int max_iters,
                                const KnnSchedKnobs& knobs) {
    KnnSchedule S;
    S.slots.assign(in.size(), KnnSchedSlot{});
    // binary problems (both sets binary, one width) are known here, on the host: they stay out of the
    // i8 schedule below and get the Hamming work list after it; so are generic-float problems (both
    // sets registered with mim_set_create_f32, one dim), which get the float work list

    // Dynamic mode (whole sweeps pulled from per-XCD lists) when the batch has at least one query-block
    // sweep per resident block: fewer pieces (no early tiles and prologue per split) and a block that
    // starts late under other batches' kernels takes less (measured: C3 isolated kNN 1.39 -> 1.32 ms,
    // pipelined C3 +2.5 %, 32-problem shards +3.8 %, C4 even; profiles/r03_knn_variants.txt, r03ac).
    // Fewer sweeps than blocks (C5's one problem, a scene's small views): the static balanced chunks.
    // MIM_KNN_DYN=0 / 1 forces either.
    long long n_sweeps = 0;
    for (const KnnSchedProblem& p : in)
        if (knn_is_i8(p)) n_sweeps += knn_query_blocks(p.nq);
    S.dyn = knobs.dyn >= 0 ? knobs.dyn != 0 : n_sweeps >= G;
    if (S.dyn)
        knn_schedule_dynamic(in, G, n_sweeps, knobs.tail, S);
    else
        knn_schedule_static(in, G, knobs.sub_target, S);
    knn_hamming_plan(in, n_cu, S);
    knn_float_plan(in, n_cu, S);
    knn_layout_offsets(in, max_iters, S);
    return S;
}

}  // namespace mim

