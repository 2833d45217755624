// Prints the distance schedule (csrc/knn_schedule.h) of the cases read from stdin, as text.
// Input, whitespace separated, per case:
//   name G n_cu max_iters sub_target dyn tail n_problems, then per problem: nq nt n_tiles bin
// (sub_target "default" = the built-in target; dyn -1 = decided from the sweep count).
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "../../computervision_objectdetection_featurematching_amd/csrc/knn_schedule.h"

int main() {
    std::string name, sub;
    int G, n_cu, max_iters, dyn, tail, n;
    while (std::cin >> name >> G >> n_cu >> max_iters >> sub >> dyn >> tail >> n) {
        mim::KnnSchedKnobs knobs;
        if (sub != "default") knobs.sub_target = atoi(sub.c_str());
        knobs.dyn = dyn;
        knobs.tail = tail != 0;
        std::vector<mim::KnnSchedProblem> in(n);
        for (auto& p : in) {
            int bin;
            if (!(std::cin >> p.nq >> p.nt >> p.n_tiles >> bin)) {
                fprintf(stderr, "case %s: truncated problem list\n", name.c_str());
                return 2;
            }
            p.bin = bin != 0;
        }
        const mim::KnnSchedule S = mim::knn_schedule(in, G, n_cu, max_iters, knobs);
        printf("case %s\n", name.c_str());
        printf("block_q %d ham_block_q %d ham_tile_rows %d\n", mim::kKnnBlockQ, mim::kHamBlockQ, mim::kHamTileRows);
        printf("n_blocks %d dyn %d part %lld good %lld\n", S.n_blocks, (int)S.dyn, S.part, S.good);
        for (size_t i = 0; i < S.slots.size(); ++i)
            printf("slot %zu %d %d %lld %lld %lld\n", i, S.slots[i].nsplit, S.slots[i].q_pad, S.slots[i].part_off,
                   S.slots[i].good_off, S.slots[i].it_off);
        for (const mim::KnnWork& w : S.works) printf("work %d %d %d %d %d\n", w.problem, w.q0, w.tile0, w.tile1, w.split);
        printf("seg");
        for (int v : S.seg) printf(" %d", v);
        printf("\n");
        for (const mim::HamPiece& h : S.ham) printf("ham %d %d %d %d %d\n", h.problem, h.q0, h.r0, h.r1, h.split);
        printf("end\n");
    }
    if (!std::cin.eof()) {
        fprintf(stderr, "bad case header\n");
        return 2;
    }
    return 0;
}
