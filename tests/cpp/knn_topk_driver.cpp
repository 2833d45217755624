// Host driver of the top-k entries' host-callable parts, for the cases read from stdin:
//   offsets k n_cu n, then per problem: nq nt bin fdim
//     the Hamming and float work lists as mim_knn_batch_dev plans them (a 128-D set is given as fdim 128) and
//     knn_topk_offsets (csrc/knn_schedule.h): per problem "slot i nsplit q_pad part_off out_off", then the
//     totals and the pieces.
//   merge k nsplit q_pad nq, then per split and query row q < nq: k entries "distance-bits(hex) index"
//     topk_merge_query (csrc/knn_topk_merge.h, the function the merge kernel runs per query) at the KT of k,
//     on a buffer of exactly nsplit * q_pad * k entries: per query "row q", then k pairs "index
//     distance-bits(hex)".
// Host only, like knn_schedule_driver.cpp.
#include <cstdio>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "../../computervision_objectdetection_featurematching_amd/csrc/knn_schedule.h"
#include "../../computervision_objectdetection_featurematching_amd/csrc/knn_topk_merge.h"

static int run_offsets() {
    int k, n_cu, n;
    if (!(std::cin >> k >> n_cu >> n)) return 2;
    std::vector<mim::KnnSchedProblem> in;
    for (int i = 0; i < n; ++i) {
        int nq, nt, bin, fdim;
        if (!(std::cin >> nq >> nt >> bin >> fdim)) return 2;
        mim::KnnSchedProblem p{nq, nt, (nt + 63) / 64, bin != 0};
        p.fdim = fdim;
        in.push_back(p);
    }
    mim::KnnSchedule S;
    S.slots.assign(in.size(), mim::KnnSchedSlot{});
    mim::knn_hamming_plan(in, n_cu, S);
    mim::knn_float_plan(in, n_cu, S);
    const mim::KnnTopkLayout Lo = mim::knn_topk_offsets(in, S.slots, k);
    for (size_t i = 0; i < in.size(); ++i)
        printf("slot %zu %d %d %lld %lld\n", i, S.slots[i].nsplit, S.slots[i].q_pad, Lo.part_off[i], Lo.out_off[i]);
    printf("total %lld %lld\n", Lo.part, Lo.out);
    for (const mim::HamPiece& h : S.ham) printf("ham %d %d %d %d %d\n", h.problem, h.q0, h.r0, h.r1, h.split);
    for (const mim::FltPiece& f : S.flt) printf("flt %d %d %d %d %d\n", f.problem, f.q0, f.r0, f.r1, f.split);
    printf("end\n");
    return 0;
}

static int run_merge() {
    int k, nsplit, q_pad, nq;
    if (!(std::cin >> k >> nsplit >> q_pad >> nq) || k < 1 || k > 16 || nq > q_pad) return 2;
    std::vector<mim::TopkEnt> parts((size_t)nsplit * q_pad * k, mim::TopkEnt{-1.f, -2});  // rows past nq: never read
    for (int sp = 0; sp < nsplit; ++sp)
        for (int q = 0; q < nq; ++q)
            for (int s = 0; s < k; ++s) {
                unsigned bits;
                int idx;
                if (!(std::cin >> std::hex >> bits >> std::dec >> idx)) return 2;
                mim::TopkEnt e;
                memcpy(&e.d, &bits, 4);
                e.i = idx;
                parts[((size_t)sp * q_pad + q) * k + s] = e;
            }
    std::vector<int32_t> idx(k);
    std::vector<float> dist(k);
    for (int q = 0; q < nq; ++q) {
        const int kt = mim::topk_kt(k);
        if (kt == 4) mim::topk_merge_query<4>(parts.data(), nsplit, q_pad, k, q, idx.data(), dist.data());
        else if (kt == 8) mim::topk_merge_query<8>(parts.data(), nsplit, q_pad, k, q, idx.data(), dist.data());
        else mim::topk_merge_query<16>(parts.data(), nsplit, q_pad, k, q, idx.data(), dist.data());
        printf("row %d", q);
        for (int s = 0; s < k; ++s) {
            unsigned bits;
            memcpy(&bits, &dist[s], 4);
            printf(" %d %x", idx[s], bits);
        }
        printf("\n");
    }
    printf("end\n");
    return 0;
}

int main() {
    std::string cmd;
    while (std::cin >> cmd) {
        const int r = cmd == "offsets" ? run_offsets() : cmd == "merge" ? run_merge() : 2;
        if (r != 0) {
            fprintf(stderr, "bad input at '%s'\n", cmd.c_str());
            return r;
        }
    }
    return 0;
}
