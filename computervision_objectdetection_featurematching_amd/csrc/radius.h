// radius.h — what radius.hip and its launcher in api.cpp share: the call's arrays and the
// work items of the three distance kernels.  Queries are numbered over all problems of a call in order; a
// problem's first query is its `qoff`.
#pragma once
#include "mim_internal.h"
#include "radius_host.h"

namespace mim {

// The arrays of one mim_radius_count call and of the fills that follow it.
struct RadArgs {
    int* counts;               // [queries] matches per query (count pass)
    int* cursor;               // [queries] slots handed out so far (fill pass)
    const long long* offsets;  // [queries + 1] exclusive scan of counts
    unsigned long long* keys;  // [offsets[queries]] radius_key of every match, a query's in arrival order
    float flt_t;               // radius_flt_threshold(r): the float kernel's bound on the squared distance
    int ham_t;                 // radius_ham_threshold(r)
    int int_t2;                // radius_int_threshold(r)
    int pad_;
};

// Work items of the Hamming and float kernels: the piece of knn_hamming_plan / knn_float_plan and the problem's
// first query.  A 128-D problem's float pieces carry the sets' flags.
struct RadHamWork {
    HamSweepWork s;
    long long qoff;
};
struct RadFltWork {
    FltSweepWork s;
    long long qoff;
};

// One problem of the i8 MFMA kernel, whose work items are the KnnWork units of knn_schedule_static.
struct RadI8Prob {
    SetDev q, t;
    long long qoff;
};

void launch_radius_hamming(const RadHamWork* works, int n_works, const RadArgs& a, bool fill, hipStream_t st);
void launch_radius_float(const RadFltWork* works, int n_works, const RadArgs& a, bool fill, hipStream_t st);
void launch_radius_i8(const RadI8Prob* probs, const KnnWork* works, const int* seg_start, int n_blocks, const RadArgs& a,
                      bool fill, hipStream_t st);
// counts -> offsets (and offsets_user, device, may be null), cursor cleared; meta: 2 + 2 radius_scan_blocks()
// words, of which meta[0] = the total and meta[1] = the longest list
int radius_scan_blocks(long long n_queries);
void launch_radius_scan(const int* counts, int* cursor, long long* offsets, long long* offsets_user, long long n_queries,
                        long long* meta, hipStream_t st);
// every query's keys sorted, then split into idx / dist; scratch: as many keys as `keys` when a list is
// longer than kRadSortCap, else unused
void launch_radius_sort(const long long* offsets, long long n_queries, unsigned long long* keys,
                        unsigned long long* scratch, int32_t* idx, float* dist, hipStream_t st);

}  // namespace mim
