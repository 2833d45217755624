// Host driver of the collection entry's host-callable parts, for the cases read from stdin:
//   offsets k n_cu grid kind nQ nI, then nQ query row counts and nI image row counts
//     kind 0: binary sets, 1: generic float sets (dim 64), 2: 128-D sets.  The pairs (query set major) planned as
//     mim_knn_collection_dev plans one group (knn_hamming_plan / knn_float_plan, and knn_schedule_static for
//     128-D sets) and knn_coll_offsets (csrc/knn_schedule.h): per pair "pair i nsplit q_pad part_off nsplit8
//     q_pad8 part8_off bound", per query set "out qi off", then "total part out".
//   groups k kind budget nQ nI, then the row counts: knn_coll_groups' "group start" lines.
//   merge k seed n_parts, then (seed = 1) k triples "index image distance-bits(hex)", then per part
//     "img qflag tflag na nb" followed by na i8 lists and nb float lists of k entries "distance-bits(hex) index"
//     coll_merge_query (csrc/knn_coll_merge.h, the function the merge kernel runs per query row) at the KT of
//     k, for query row 1 of lists padded to 3 rows (the other rows are poison), the i8 lists in their KT-slot
//     form, on buffers of exactly the stated sizes: "row", then k triples "index image distance-bits(hex)".
// Host only, like knn_topk_driver.cpp.
#include <cstdio>
#include <cstring>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#include "../../computervision_objectdetection_featurematching_amd/csrc/knn_coll_merge.h"
#include "../../computervision_objectdetection_featurematching_amd/csrc/knn_schedule.h"

static bool read_counts(int nQ, int nI, std::vector<int>& nq, std::vector<int>& nt) {
    nq.resize(nQ);
    nt.resize(nI);
    for (int& v : nq)
        if (!(std::cin >> v)) return false;
    for (int& v : nt)
        if (!(std::cin >> v)) return false;
    return true;
}

static int run_offsets() {
    int k, n_cu, grid, kind, nQ, nI;
    std::vector<int> nq, nt;
    if (!(std::cin >> k >> n_cu >> grid >> kind >> nQ >> nI) || !read_counts(nQ, nI, nq, nt)) return 2;
    std::vector<mim::KnnSchedProblem> in;
    for (int qi = 0; qi < nQ; ++qi)
        for (int j = 0; j < nI; ++j) {
            mim::KnnSchedProblem p{nq[qi], nt[j], (nt[j] + 63) / 64, kind == 0};
            p.fdim = kind == 1 ? 64 : kind == 2 ? 128 : 0;
            in.push_back(p);
        }
    mim::KnnSchedule S, S8;
    S.slots.assign(in.size(), mim::KnnSchedSlot{});
    mim::knn_hamming_plan(in, n_cu, S);
    mim::knn_float_plan(in, n_cu, S);
    if (kind == 2) {
        for (mim::KnnSchedProblem& p : in) p.fdim = 0;
        S8.slots.assign(in.size(), mim::KnnSchedSlot{});
        mim::knn_schedule_static(in, grid, -1, S8);
    }
    const mim::KnnCollLayout Lo = mim::knn_coll_offsets(nq, nI, S.slots, kind == 2 ? &S8.slots : nullptr, k);
    for (size_t i = 0; i < in.size(); ++i)
        printf("pair %zu %d %d %lld %d %d %lld %lld\n", i, S.slots[i].nsplit, S.slots[i].q_pad, Lo.part_off[i],
               kind == 2 ? S8.slots[i].nsplit : 0, kind == 2 ? S8.slots[i].q_pad : 0, Lo.part8_off[i],
               mim::knn_coll_pair_bound(in[i].nq, in[i].nt, kind == 0, kind == 2, k));
    for (int qi = 0; qi < nQ; ++qi) printf("out %d %lld\n", qi, Lo.out_off[qi]);
    printf("total %lld %lld\n", Lo.part, Lo.out);
    for (const mim::KnnWork& w : S8.works) printf("i8 %d %d %d %d %d\n", w.problem, w.q0, w.tile0, w.tile1, w.split);
    printf("end\n");
    return 0;
}

static int run_groups() {
    int k, kind, nQ, nI;
    long long budget;
    std::vector<int> nq, nt;
    if (!(std::cin >> k >> kind >> budget >> nQ >> nI) || !read_counts(nQ, nI, nq, nt)) return 2;
    for (int s : mim::knn_coll_groups(nq, nt, kind == 0, kind == 2, k, budget)) printf("group %d\n", s);
    printf("end\n");
    return 0;
}

static bool read_ent(mim::TopkEnt& e) {
    unsigned bits;
    if (!(std::cin >> std::hex >> bits >> std::dec >> e.i)) return false;
    memcpy(&e.d, &bits, 4);
    return true;
}

static int run_merge() {
    int k, seed, n_parts;
    if (!(std::cin >> k >> seed >> n_parts) || k < 1 || k > 16) return 2;
    const int kt = mim::topk_kt(k), q_pad = 3, q = 1;
    // exactly k entries each: an access past them is the sanitizer's to find
    std::unique_ptr<int32_t[]> idx(new int32_t[k]), img(new int32_t[k]);
    std::unique_ptr<float[]> dist(new float[k]);
    for (int s = 0; s < k; ++s) {
        idx[s] = img[s] = -9;
        dist[s] = -9.f;
    }
    if (seed)
        for (int s = 0; s < k; ++s) {
            unsigned bits;
            if (!(std::cin >> idx[s] >> img[s] >> std::hex >> bits >> std::dec)) return 2;
            memcpy(&dist[s], &bits, 4);
        }
    std::vector<mim::CollPart> parts(n_parts);
    std::vector<std::vector<mim::TopkEnt>> bufs;
    std::vector<std::unique_ptr<int>> flags;
    for (int p = 0; p < n_parts; ++p) {
        int im, qf, tf, na, nb;
        if (!(std::cin >> im >> qf >> tf >> na >> nb)) return 2;
        const mim::TopkEnt poison{-3.f, -4};
        std::vector<mim::TopkEnt> a((size_t)na * q_pad * kt, poison), b((size_t)nb * q_pad * k, poison);
        for (int l = 0; l < na; ++l) {
            mim::TopkEnt* e = a.data() + ((size_t)l * q_pad + q) * kt;
            for (int s = 0; s < kt - k; ++s) e[s] = mim::TopkEnt{-1.f, -1};
            for (int s = 0; s < k; ++s)
                if (!read_ent(e[kt - k + s])) return 2;
        }
        for (int l = 0; l < nb; ++l)
            for (int s = 0; s < k; ++s)
                if (!read_ent(b[((size_t)l * q_pad + q) * k + s])) return 2;
        bufs.push_back(std::move(a));
        bufs.push_back(std::move(b));
        flags.emplace_back(new int(qf));
        flags.emplace_back(new int(tf));
        mim::CollPart& P = parts[p];
        P = mim::CollPart{};
        P.img = im;
        if (na > 0) {
            P.na = na;
            P.qa_pad = q_pad;
            P.qflags = flags[flags.size() - 2].get();
            P.tflags = flags[flags.size() - 1].get();
        }
        P.nb = nb;
        P.qb_pad = q_pad;
    }
    for (int p = 0; p < n_parts; ++p) {  // the buffers no longer move
        if (parts[p].na > 0) parts[p].a = bufs[2 * p].data();
        parts[p].b = bufs[2 * p + 1].data();
    }
    if (kt == 4) mim::coll_merge_query<4>(parts.data(), n_parts, k, q, seed != 0, idx.get(), img.get(), dist.get());
    else if (kt == 8) mim::coll_merge_query<8>(parts.data(), n_parts, k, q, seed != 0, idx.get(), img.get(), dist.get());
    else mim::coll_merge_query<16>(parts.data(), n_parts, k, q, seed != 0, idx.get(), img.get(), dist.get());
    printf("row");
    for (int s = 0; s < k; ++s) {
        unsigned bits;
        memcpy(&bits, &dist[s], 4);
        printf(" %d %d %x", idx[s], img[s], bits);
    }
    printf("\nend\n");
    return 0;
}

int main() {
    std::string cmd;
    while (std::cin >> cmd) {
        const int r = cmd == "offsets" ? run_offsets() : cmd == "groups" ? run_groups() : cmd == "merge" ? run_merge() : 2;
        if (r != 0) {
            fprintf(stderr, "bad input at '%s'\n", cmd.c_str());
            return r;
        }
    }
    return 0;
}
