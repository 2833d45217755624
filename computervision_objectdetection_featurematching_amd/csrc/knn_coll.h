// knn_coll.h — what knn_coll.hip and its launcher in api.cpp share (mim_knn_collection_dev):
// the problem record of the i8 MFMA top-k kernel and the tables of the collection merge.
#pragma once
#include "knn_coll_merge.h"
#include "mim_internal.h"

namespace mim {

// One (query set, image) pair of the i8 top-k kernel, whose work items are the KnnWork units of
// knn_schedule_static.  Split s of the pair writes lists 2 s (lane half 0) and 2 s + 1 of parts.
struct CollI8Prob {
    SetDev q, t;
    TopkEnt* parts;  // [2 nsplit][q_pad][KT], KT = topk_kt(k)
    int q_pad;
    int pad_;
};

// One query set of the merge: its rows and where its output rows start (entries).
struct CollQuery {
    long long out_off;
    int nq;
    int pad_;
};

void launch_knn_topk_i8(const CollI8Prob* probs, const KnnWork* works, const int* seg_start, int n_blocks, int k,
                        hipStream_t st);
// parts: [n_queries][n_parts] records, a query set's in image order; seed: the outputs hold an earlier group's lists
void launch_knn_coll_merge(const CollQuery* queries, int n_queries, const CollPart* parts, int n_parts, int max_nq, int k,
                           bool seed, int32_t* idx, int32_t* img, float* dist, hipStream_t st);

}  // namespace mim
