// api.cpp — the C ABI of include/mim.h: context, descriptor sets, batch orchestration.
//
// Host side of the drop-in boundary for TestsDetector.cpp:58-95.  Everything numeric runs in the
// HIP kernels of knn.hip / ransac.hip; this file only allocates, builds problem tables and
// enqueues launches on the ctx stream.  There is no CPU compute path: a missing device or a
// failed launch is reported as MIM_EDEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/mim.h"
#include "../../include/mim_detect.hpp"
#include "knn_coll.h"
#include "mim_internal.h"
#include "radius.h"

namespace mim {
void launch_prep_batch(const PrepJob* jobs, int njobs, int total_tiles, hipStream_t st);
void launch_knn(const ProbDev* probs, const KnnWork* works, int n_works, const int* seg_start, int n_blocks, Top2* parts,
                int* dyn_ctr, float kappa, float flip_ratio, hipStream_t st);
int knn_blocks_per_cu();
void launch_knn_hamming(const HamWork* works, int n_works, hipStream_t st);
void launch_knn_hamming_cross(const HamCrossWork* works, int n_works, uint32_t* colmin, long long n_col,
                              hipStream_t st);
void launch_knn_float(const FltWork* works, int n_works, hipStream_t st);
void launch_knn_topk_hamming(const TopkHamWork* works, int n_works, int k, hipStream_t st);
void launch_knn_topk_float(const TopkFltWork* works, int n_works, int k, hipStream_t st);
void launch_knn_topk_merge(const TopkProb* probs, int n_probs, int max_nq, int k, hipStream_t st);
void launch_cross(const ProbDev* probs, const CrossDev* cross, int n_probs, const Top2* parts, float ratio, int filter,
                  int32_t* good_q, int32_t* good_t, float4* pts, int* n_good, int32_t* match_idx, float* match_dist,
                  hipStream_t st);
void launch_ratio(const ProbDev* probs, int n_probs, const Top2* parts, float ratio, int32_t* good_q,
                  int32_t* good_t, float4* pts, int* n_good, int32_t* knn_idx, float* knn_dist,
                  hipStream_t st);
void launch_knn_emit(const ProbDev* probs, int nq, const Top2* parts, int32_t* knn_idx, float* knn_dist,
                     hipStream_t st);
void launch_inlier_gather(const ProbDev* probs, int n, const mim_result* res, const int32_t* good_t,
                          const uint8_t* masks, const long long* offs, const float* scales, float2* out, hipStream_t st);
size_t ransac_chain_bytes();
void launch_rng_stream(const unsigned long long* seg_state, uint32_t* out, long long len, int seg, int n_seg,
                       hipStream_t s);
void ransac_enqueue(const RansacParams& prm, int n_probs, const ProbDev* probs, const float4* pts,
                    const int* n_good, const RansacBufs& b, uint8_t* masks, mim_result* results, int raw,
                    hipStream_t s, void (*mark)(void*, const char*, hipStream_t), void* mark_ctx, int exact_all);
}  // namespace mim

using namespace mim;

namespace {

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        size_t want = std::max(bytes, (size_t)4096);
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    template <class T> T* as() const { return static_cast<T*>(p); }
};

// Bump arena for per-set device storage; mim_sets_clear() rewinds it without freeing.
struct Arena {
    std::vector<std::pair<char*, size_t>> chunks;
    size_t chunk_i = 0, off = 0;
    hipError_t alloc(size_t bytes, void** out) {
        bytes = (bytes + 255) & ~size_t(255);
        while (chunk_i < chunks.size() && off + bytes > chunks[chunk_i].second) {
            ++chunk_i;
            off = 0;
        }
        if (chunk_i == chunks.size()) {
            size_t sz = std::max(bytes, (size_t)256 << 20);
            char* p = nullptr;
            hipError_t e = hipMalloc(&p, sz);
            if (e != hipSuccess) return e;
            chunks.push_back({p, sz});
            off = 0;
        }
        *out = chunks[chunk_i].first + off;
        off += bytes;
        return hipSuccess;
    }
    void rewind() { chunk_i = 0; off = 0; }
    struct Mark {
        size_t chunk_i, off;
        bool operator<(const Mark& o) const { return chunk_i < o.chunk_i || (chunk_i == o.chunk_i && off < o.off); }
    };
    Mark pos() const { return Mark{chunk_i, off}; }
    void seek(Mark m) { chunk_i = m.chunk_i; off = m.off; }
    void release() {
        for (auto& c : chunks) (void)hipFree(c.first);
        chunks.clear();
        rewind();
    }
};

struct SetRec {
    SetDev d;
    Arena::Mark mark;  // the arena before the set's storage (mim_sets_truncate)
    int bin_pad = 0;   // binary set: bytes per padded row (16, 32 or 64); 0: a float set
    int bin_width = 0; // binary set: the caller's bytes per row
    int fdim = 0;      // generic float set (mim_set_create_f32): floats per row, 1..kFltMaxDim; 0: not one
    int fpad = 0;      // generic float set: floats per stored row (fdim rounded up to a multiple of 4)
    // the kind, and what the float kernels read of a generic float or a 128-D set (no caller decodes the fields)
    bool is_bin() const { return bin_pad != 0; }
    bool is_f32() const { return fdim != 0; }
    bool is_sift() const { return !bin_pad && !fdim; }  // the 128-D set of mim_set_create, with its prep job
    int flt_dim() const { return fdim ? fdim : kDim; }
    int flt_stride() const { return fdim ? fpad : kDim; }
};

// Pinned staging for the per-batch tables, two generations: a batch's host->device table copies
// are stream-ordered, so the host never waits for the previous batch; a generation is rewritten
// only after the event of its last copy (two batches back) has completed.
struct PinnedStage {
    char* p[2] = {nullptr, nullptr};
    size_t cap[2] = {0, 0};
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool used[2] = {false, false};
    int par = 0;
    hipError_t acquire(size_t bytes, char** out) {
        par ^= 1;
        if (used[par]) {
            hipError_t e = hipEventSynchronize(ev[par]);
            if (e != hipSuccess) return e;
        }
        if (!ev[par]) {
            hipError_t e = hipEventCreateWithFlags(&ev[par], hipEventDisableTiming);
            if (e != hipSuccess) return e;
        }
        if (bytes > cap[par]) {
            if (p[par]) (void)hipHostFree(p[par]);
            p[par] = nullptr;
            cap[par] = 0;
            hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&p[par]), std::max(bytes, (size_t)1 << 16));
            if (e != hipSuccess) return e;
            cap[par] = std::max(bytes, (size_t)1 << 16);
        }
        *out = p[par];
        return hipSuccess;
    }
    hipError_t release_after(hipStream_t s) {  // the copies from the current generation are enqueued
        used[par] = true;
        return hipEventRecord(ev[par], s);
    }
    void destroy() {
        for (int i = 0; i < 2; ++i) {
            if (ev[i]) (void)hipEventSynchronize(ev[i]);
            if (p[i]) (void)hipHostFree(p[i]);
            if (ev[i]) (void)hipEventDestroy(ev[i]);
            p[i] = nullptr;
            ev[i] = nullptr;
        }
    }
};

template <class T> size_t vec_bytes(const std::vector<T>& v) { return sizeof(T) * v.size(); }

// One call's table uploads through a PinnedStage generation of `total` bytes: put() copies a table into the
// stage behind the last one and enqueues its host->device copy, done() lets the generation go after them.
// The first error sticks, so only done()'s result needs a check.
struct StageWriter {
    PinnedStage& ps;
    hipStream_t s;
    char* p = nullptr;
    size_t off = 0;
    hipError_t err;
    StageWriter(PinnedStage& ps_, size_t total, hipStream_t s_) : ps(ps_), s(s_) { err = ps.acquire(total, &p); }
    // b: a second table that lies behind the first on the device too (one copy for both)
    void put(void* dst, const void* a, size_t ab, const void* b = nullptr, size_t bb = 0) {
        if (err != hipSuccess || ab + bb == 0) return;
        if (ab) memcpy(p + off, a, ab);
        if (bb) memcpy(p + off + ab, b, bb);
        err = hipMemcpyAsync(dst, p + off, ab + bb, hipMemcpyHostToDevice, s);
        off += ab + bb;
    }
    template <class T> void put(const DevBuf& dst, const std::vector<T>& v) { put(dst.p, v.data(), vec_bytes(v)); }
    hipError_t done() { return err != hipSuccess ? err : ps.release_after(s); }
};

}  // namespace

namespace mim {
// RANSAC workspace (definition shared with ransac.hip through this layout)
struct RansacWs {
    DevBuf state, samples, hyp, counts, bounds, flags, irr_bits, irr, irr_cnt, cls, cls_tab, pass_bits, defer, defer_n, chains, best_h, cand, ncand, cex, cH, decided, stream,
        scratch, inl, tiles, tbox, perm, surv, nsurv, strip, err;
    long long stream_len = 0;
};
}  // namespace mim

struct mim_ctx {
    int device = 0;
    hipStream_t own = nullptr, stream = nullptr;
    std::mutex mu;
    std::string err;
    Arena arena;
    std::vector<SetRec> sets;
    // batch workspace
    DevBuf probs, works, parts, good_q, good_t, pts, n_good, results, masks, knn_idx, knn_dist, inl_tab, inl_out, knn_ctr, ham_works, flt_works;
    RansacWs rws;
    std::vector<ProbDev> h_probs;
    int n_ham_works = 0;  // Hamming work items of the current batch (its binary problems)
    int n_flt_works = 0;  // generic-float work items of the current batch
    // cross-check batches (mim_batch_run_filter): the one-pass Hamming kernel's work items
    // and column minima, and the per-problem table of where the reverse nearest rows are
    DevBuf ham_cross_works, colmin, cross_tab;
    int n_ham_cross_works = 0;
    long long n_colmin = 0;  // entries of colmin over the batch's fused binary problems
    // top-k entries (mim_knn_batch_dev): partial lists, work items and the merge's problem table
    DevBuf topk_parts, topk_ham_works, topk_flt_works, topk_probs;
    int topk_splits = 0;  // the most train splits of a problem of the last such call
    // train collections (mim_knn_collection_dev): one group's partial lists, the work items of its
    // three distance kernels, the i8 kernel's pair records and the merge's tables
    DevBuf coll_parts, coll_ham_works, coll_flt_works, coll_i8_probs, coll_i8_works, coll_tab, coll_queries;
    int coll_groups = 0;     // image groups of the last such call
    int coll_i8_splits = 0;  // the most train splits the i8 schedule gave a pair of it
    // radius matching (mim_radius_count / mim_radius_fill_dev): the call's arrays, the work items
    // of its three distance kernels, and what the last count call left for the fills that follow it
    DevBuf rad_counts, rad_cursor, rad_offsets, rad_meta, rad_keys, rad_scratch, rad_ham_works, rad_flt_works, rad_i8_works,
        rad_probs;
    struct RadLast {
        bool valid = false;
        std::vector<mim_problem> problems;
        float r = 0.f;
        long long gen = -1;              // sets generation at the count
        long long n_queries = 0, total = 0, longest = 0;
        int n_ham = 0, n_flt = 0, n_i8_works = 0, n_i8_blocks = 0;
        bool filled = false;             // a fill has used the cursors since the scan cleared them
    } rad;
    int knn_cross = 0;       // how the last batch found the reverse neighbours: 0 not, 1 second sweep, 2 fused
    int last_filter = 0;     // the last mim_batch_run_filter's filter, for its re-run
    int n_cu = 0;         // compute units of the device (first batch)
    int n_works = 0;  // distance segments of the current batch (works, then the per-block segment starts)
    std::vector<long long> h_good_off;
    PinnedStage stage;
    // sets created since the last batch: their prep runs as one launch at the next build_tables
    std::vector<PrepJob> pend;
    std::vector<int> pend_set;
    // per prep flush: the lowest set id it covered and the arena after its flags block
    std::vector<std::pair<int, Arena::Mark>> flushes;
    PinnedStage prep_stage;
    DevBuf prep_jobs;
    int last_n = 0;
    // the last mim_batch_run, kept so that mim_batch_results can re-run it on a longer RNG stream
    // (possible while its sets are intact: sets_gen unchanged since the batch)
    std::vector<mim_problem> last_problems;
    mim_params last_params{};
    long long sets_gen = 0, last_gen = -1;
    // the last batch is mim_find_homography's one record (no set table: no inlier points to gather)
    bool last_fh = false;
    // MIM_CAND_CAP: candidate-list capacity override (test knob for the replay's overflow rescan)
    int cand_cap = 0;
    // MIM_ATTEMPT_REP_CAP: the attempt kernel's redraw-list capacity (test knob for its in-place path)
    int rep_cap = 0;
    // MIM_STREAM_DRAWS: initial RNG stream length (test knob for the grow-and-re-run path)
    long long stream_draws = 0;
    // MIM_RANSAC_EXACT=1: evaluate every hypothesis exactly (reference mode for cross-checks)
    int exact_all = 0;
    int knn_grid = 0;      // resident distance-kernel blocks on the device (first batch)
    int n_knn_blocks = 0;  // distance-kernel blocks of the current batch (<= knn_grid)
    bool knn_dyn = false;  // current batch's distance work as 8 per-XCD lists pulled dynamically
    bool knn_whole = false;  // and every i8 problem as whole sweeps of one split (no tail pieces)
    int knn_mode = -1;       // the last batch's distance kernel: 0 exact, 1 ratio mode, 2 verdict mode
    hipStream_t cur = nullptr;  // stream the enqueue helpers launch on
    // sampler stream (RansacBufs::s2): the next chunk's getSubset replay beside this chunk's
    // selection kernels (MIM_SAMPLER_STREAM=0: one stream)
    hipStream_t samp = nullptr;
    hipEvent_t ev_samp_fork = nullptr, ev_samp[2] = {nullptr, nullptr};
    int samp_on = -1;
    // timing: events per stream, durations summed per kernel name over the streams
    bool timing = false;
    struct Ev {
        std::string name;
        hipStream_t s;
        hipEvent_t e;
        int seq;  // batch the event belongs to: spans are taken within one batch only
    };
    int ev_seq = 0;
    std::vector<Ev> evs;
    std::vector<hipEvent_t> ev_pool;  // recycled events (creating one per mark costs host time)
    std::map<std::string, double> last_ms;
    mim::SiftWs* sift = nullptr;
    std::vector<mim::SiftWs*> sift_last;  // the workspaces of the last SIFT call's images (mim_sift_debug_pyramid)
    std::vector<mim::SiftWs*> sift_scales;  // mim_sift_detect_compute_scales: one per scale + the scene  // SIFT pyramid / candidate / descriptor workspace (first use)
};

static mim_status fail(mim_ctx* c, mim_status code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    return code;
}

#define HIPCHK(c, expr)                                                                          \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            return fail((c), e_ == hipErrorOutOfMemory ? MIM_ENOMEM : MIM_EDEVICE, "%s: %s (%s:%d)", \
                        #expr, hipGetErrorString(e_), __FILE__, __LINE__);                       \
    } while (0)

// no RANSAC records: the previous batch's are invalidated (mim.h)
static void invalidate_batch(mim_ctx* c) {
    c->last_n = 0;
    c->last_gen = -1;
    c->last_fh = false;
}

// The row arguments every host-buffer entry takes; outputs_ok: the entry's own test of its output pointers.
static mim_status check_host_pair(mim_ctx* c, const char* entry, const void* q, int32_t nq, const void* t, int32_t nt,
                                  bool outputs_ok) {
    if (nq < 0 || nt < 0 || (nq > 0 && !q) || (nt > 0 && !t) || !outputs_ok)
        return fail(c, MIM_EINVAL, "%s: bad arguments", entry);
    return MIM_OK;
}

extern "C" {

const char* mim_version(void) { return "mim 0.1.0 (gfx950)"; }

void mim_default_params(mim_params* p) {
    p->ratio = 0.9f;          // TestsDetector.cpp:21
    p->min_good = 4;          // :22, :74
    p->min_inliers = 4;       // :22, :81
    p->ransac_thresh = 5.0;   // :23
    p->max_iters = 2000;      // findHomography default
    p->confidence = 0.995;    // findHomography default
    p->det_lo = (double)0.1f; // :24 (constexpr float)
    p->det_hi = (double)10.0f;  // :25
}

mim_status mim_ctx_create(int device, mim_ctx** out) {
    if (!out) return MIM_EINVAL;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return MIM_EDEVICE;
    if (device < 0 || device >= ndev) return MIM_EINVAL;
    if (hipSetDevice(device) != hipSuccess) return MIM_EDEVICE;
    mim_ctx* c = new mim_ctx();
    c->device = device;
    if (hipStreamCreateWithFlags(&c->own, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return MIM_EDEVICE;
    }
    c->stream = c->own;
    c->cur = c->own;
    const char* ex = getenv("MIM_RANSAC_EXACT");
    c->exact_all = (ex && ex[0] == '1') ? 1 : 0;
    const char* cc = getenv("MIM_CAND_CAP");
    c->cand_cap = cc ? std::max(1, atoi(cc)) : 0;
    const char* rc = getenv("MIM_ATTEMPT_REP_CAP");
    c->rep_cap = rc ? std::max(1, atoi(rc)) : 0;
    const char* sd = getenv("MIM_STREAM_DRAWS");
    c->stream_draws = sd ? std::max(4096LL, atoll(sd)) : 0;
    *out = c;
    return MIM_OK;
}

void mim_ctx_destroy(mim_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    for (auto& e : c->evs) (void)hipEventDestroy(e.e);
    for (hipEvent_t e : c->ev_pool) (void)hipEventDestroy(e);
    if (c->samp) (void)hipStreamSynchronize(c->samp);
    if (c->ev_samp_fork) (void)hipEventDestroy(c->ev_samp_fork);
    for (auto e : c->ev_samp)
        if (e) (void)hipEventDestroy(e);
    if (c->samp) (void)hipStreamDestroy(c->samp);
    mim::sift_ws_destroy(c->sift);
    for (mim::SiftWs* w : c->sift_scales) mim::sift_ws_destroy(w);
    c->stage.destroy();
    c->prep_stage.destroy();
    c->arena.release();
    for (DevBuf* b : {&c->probs, &c->works, &c->parts, &c->good_q, &c->good_t, &c->pts, &c->n_good,
                      &c->results, &c->masks, &c->knn_idx, &c->knn_dist, &c->inl_tab, &c->inl_out, &c->knn_ctr, &c->ham_works, &c->flt_works, &c->ham_cross_works, &c->colmin, &c->cross_tab, &c->topk_parts, &c->topk_ham_works, &c->topk_flt_works, &c->topk_probs, &c->coll_parts, &c->coll_ham_works, &c->coll_flt_works, &c->coll_i8_probs, &c->coll_i8_works, &c->coll_tab, &c->coll_queries, &c->rad_counts, &c->rad_cursor, &c->rad_offsets, &c->rad_meta, &c->rad_keys, &c->rad_scratch, &c->rad_ham_works, &c->rad_flt_works, &c->rad_i8_works, &c->rad_probs, &c->rws.state, &c->rws.samples,
                      &c->rws.hyp, &c->rws.counts, &c->rws.bounds, &c->rws.flags, &c->rws.irr_bits, &c->rws.irr, &c->rws.irr_cnt, &c->rws.cls, &c->rws.cls_tab, &c->rws.pass_bits, &c->rws.defer, &c->rws.defer_n, &c->rws.chains, &c->rws.best_h, &c->rws.cand, &c->rws.ncand, &c->rws.cex, &c->rws.cH, &c->rws.decided, &c->rws.stream, &c->rws.scratch, &c->rws.inl, &c->rws.tiles, &c->rws.tbox, &c->rws.perm, &c->rws.surv, &c->rws.nsurv, &c->rws.strip, &c->rws.err, &c->prep_jobs})
        b->release();
    if (c->own) (void)hipStreamDestroy(c->own);
    delete c;
}

const char* mim_last_error(const mim_ctx* c) { return c ? c->err.c_str() : "null ctx"; }

mim_status mim_ctx_set_stream(mim_ctx* c, void* stream) {
    if (!c) return MIM_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    c->stream = stream ? (hipStream_t)stream : c->own;
    return MIM_OK;
}

mim_status mim_ctx_set_sampler_stream(mim_ctx* c, int32_t on) {
    if (!c) return MIM_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    c->samp_on = on != 0;  // the stream itself is created on the first batch that uses it
    return MIM_OK;
}

void* mim_ctx_get_stream(const mim_ctx* c) { return c ? (void*)c->stream : nullptr; }

mim_status mim_synchronize(mim_ctx* c) {
    if (!c) return MIM_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MIM_OK;
}

mim_status mim_set_timing(mim_ctx* c, int32_t enable) {
    if (!c) return MIM_EINVAL;
    c->timing = enable != 0;
    return MIM_OK;
}

double mim_last_kernel_ms(mim_ctx* c, const char* name) {
    if (!c || !name) return -1;
    if (!strcmp(name, "knn_cross")) return c->knn_cross;  // nor this: how the last batch found the reverse neighbours
    if (!strcmp(name, "knn_topk_splits")) return c->topk_splits;  // nor this: the last top-k call's most train splits
    if (!strcmp(name, "knn_coll_groups")) return c->coll_groups;  // nor these: the last collection call's image groups
    if (!strcmp(name, "knn_coll_i8_splits")) return c->coll_i8_splits;  // and the most i8 train splits of a pair of it
    if (!strcmp(name, "radius_sort_cap")) return kRadSortCap;  // nor this: the longest list the radius sort keeps in LDS
    if (!strcmp(name, "knn_mode")) return c->knn_mode;  // not a time: the form the last batch's distance kernel ran in
    auto it = c->last_ms.find(name);
    return it == c->last_ms.end() ? -1 : it->second;
}

// sync: wait for the copies of host rows before returning (false: the caller waits once for several)
static mim_status set_create_locked(mim_ctx* c, const float* desc, const float* kp, int32_t n, int32_t dim,
                                    int32_t on_device, int32_t* set_id, bool sync = true) {
    if (!set_id || n < 0 || (n > 0 && (!desc || !kp))) return fail(c, MIM_EINVAL, "set_create: bad arguments");
    if (dim != kDim) return fail(c, MIM_EINVAL, "set_create: dim must be %d (got %d)", kDim, dim);
    HIPCHK(c, hipSetDevice(c->device));
    SetRec r{};
    r.mark = c->arena.pos();
    r.d.n = n;
    r.d.n_tiles = (n + 63) / 64;
    const size_t tiles = (size_t)std::max(r.d.n_tiles, 1);
    void *frag, *norm;
    HIPCHK(c, c->arena.alloc(tiles * kTileBytes, &frag));
    HIPCHK(c, c->arena.alloc(tiles * kNormWords * sizeof(int), &norm));
    const float* f32 = desc;
    const float* kpd = kp;
    if (!on_device && n > 0) {
        void *df, *dk;
        HIPCHK(c, c->arena.alloc((size_t)n * kDim * sizeof(float), &df));
        HIPCHK(c, c->arena.alloc((size_t)n * 2 * sizeof(float), &dk));
        HIPCHK(c, hipMemcpyAsync(df, desc, (size_t)n * kDim * sizeof(float), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(dk, kp, (size_t)n * 2 * sizeof(float), hipMemcpyHostToDevice, c->stream));
        f32 = (const float*)df;
        kpd = (const float*)dk;
    }
    r.d.frag = (const int8_t*)frag;
    r.d.norm = (const int*)norm;
    r.d.f32 = f32;
    r.d.kp = (const float2*)kpd;
    r.d.flags = nullptr;  // assigned when the prep is flushed
    if (!on_device && sync) HIPCHK(c, hipStreamSynchronize(c->stream));  // host buffers may go away
    *set_id = (int32_t)c->sets.size();
    c->pend.push_back(PrepJob{f32, (int8_t*)frag, (int*)norm, nullptr, n, 0});
    c->pend_set.push_back(*set_id);
    c->sets.push_back(r);
    return MIM_OK;
}

// Preps of the sets created since the last flush: one flags block, one memset, one launch.
static mim_status flush_preps(mim_ctx* c) {
    const int nj = (int)c->pend.size();
    if (nj == 0) return MIM_OK;
    void* flags;
    HIPCHK(c, c->arena.alloc(sizeof(int) * 4 * (size_t)nj, &flags));
    HIPCHK(c, hipMemsetAsync(flags, 0, sizeof(int) * 4 * (size_t)nj, c->stream));
    int tiles = 0;
    for (int j = 0; j < nj; ++j) {
        PrepJob& J = c->pend[j];
        J.flags = static_cast<int*>(flags) + 4 * j;
        J.tile0 = tiles;
        tiles += (J.n + 63) / 64;
        c->sets[c->pend_set[j]].d.flags = J.flags;
    }
    const size_t bytes = sizeof(PrepJob) * nj;
    HIPCHK(c, c->prep_jobs.ensure(bytes));
    StageWriter up(c->prep_stage, bytes, c->stream);
    up.put(c->prep_jobs, c->pend);
    HIPCHK(c, up.done());
    launch_prep_batch(c->prep_jobs.as<PrepJob>(), nj, tiles, c->stream);
    HIPCHK(c, hipGetLastError());
    c->flushes.push_back({*std::min_element(c->pend_set.begin(), c->pend_set.end()), c->arena.pos()});
    c->pend.clear();
    c->pend_set.clear();
    return MIM_OK;
}

mim_status mim_set_create(mim_ctx* c, const float* desc, const float* kp, int32_t n, int32_t dim,
                          int32_t on_device, int32_t* set_id) {
    if (!c) return MIM_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    return set_create_locked(c, desc, kp, n, dim, on_device, set_id);
}

// The sets that keep a copy of the caller's rows and need no prep job (binary, generic float): n rows of
// row_bytes at `step` copied to a stride of stored_bytes, zero filled, with zero rows up to the next multiple
// of row_pad (the kernels stage whole tiles).  r says the kind; `who` names the entry in the messages.
static mim_status set_create_rows_locked(mim_ctx* c, const char* who, SetRec r, const void* desc, int64_t step,
                                         size_t row_bytes, size_t stored_bytes, int row_pad, const float* kp, int32_t n,
                                         int32_t on_device, int32_t* set_id) {
    HIPCHK(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)std::max((n + row_pad - 1) / row_pad, 1) * row_pad * stored_bytes;
    r.mark = c->arena.pos();
    r.d.n = n;
    r.d.n_tiles = (n + 63) / 64;
    void *dd = nullptr, *dk = nullptr;
    auto undo = [&](mim_status st) {
        c->arena.seek(r.mark);
        return st;
    };
    if (c->arena.alloc(bytes, &dd) != hipSuccess ||
        c->arena.alloc((size_t)std::max(n, 1) * sizeof(float2), &dk) != hipSuccess)
        return undo(fail(c, MIM_ENOMEM, "%s: device allocation of %zu bytes failed", who, bytes));
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    hipError_t e = hipMemsetAsync(dd, 0, bytes, c->stream);
    if (e == hipSuccess && n > 0)
        e = hipMemcpy2DAsync(dd, stored_bytes, desc, (size_t)step, row_bytes, (size_t)n, kind, c->stream);
    if (e == hipSuccess && n > 0) e = hipMemcpyAsync(dk, kp, (size_t)n * sizeof(float2), kind, c->stream);
    if (e == hipSuccess && !on_device) e = hipStreamSynchronize(c->stream);  // host buffers may go away
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(c->stream);
        return undo(fail(c, MIM_EDEVICE, "%s: copy failed: %s", who, hipGetErrorString(e)));
    }
    if (r.is_bin()) r.d.frag = (const int8_t*)dd;
    else r.d.f32 = (const float*)dd;
    r.d.kp = (const float2*)dk;
    *set_id = (int32_t)c->sets.size();
    c->sets.push_back(r);
    return MIM_OK;
}

// A binary set: rows zero-padded to 16, 32 or 64 bytes, which the Hamming kernel reads as they are.
static mim_status set_create_bin_locked(mim_ctx* c, const uint8_t* desc, int64_t step, const float* kp, int32_t n,
                                        int32_t width, int32_t on_device, int32_t* set_id) {
    if (!set_id || n < 0 || (n > 0 && (!desc || !kp))) return fail(c, MIM_EINVAL, "set_create_bin: bad arguments");
    if (width < 1 || width > 64) return fail(c, MIM_EINVAL, "set_create_bin: width must be 1..64 bytes (got %d)", width);
    if (step < width)
        return fail(c, MIM_EINVAL, "set_create_bin: step %lld < width %d", (long long)step, width);
    SetRec r{};
    r.bin_pad = width <= 16 ? 16 : width <= 32 ? 32 : 64;
    r.bin_width = width;
    return set_create_rows_locked(c, "set_create_bin", r, desc, step, (size_t)width, (size_t)r.bin_pad, kHamTileRows,
                                  kp, n, on_device, set_id);
}

mim_status mim_set_create_bin(mim_ctx* c, const uint8_t* desc, int64_t step, const float* kp, int32_t n, int32_t width,
                              int32_t on_device, int32_t* set_id) {
    if (!c) return MIM_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    return set_create_bin_locked(c, desc, step, kp, n, width, on_device, set_id);
}

// A generic float set: rows at a stride of dim rounded up to 4 floats.  No flags: the host knows the kind,
// so such a set never takes the i8 path, and the float kernel never inserts a row past n.
static mim_status set_create_f32_locked(mim_ctx* c, const float* desc, int64_t step, const float* kp, int32_t n,
                                        int32_t dim, int32_t on_device, int32_t* set_id) {
    if (!set_id || n < 0 || (n > 0 && (!desc || !kp))) return fail(c, MIM_EINVAL, "set_create_f32: bad arguments");
    if (dim < 1 || dim > kFltMaxDim)
        return fail(c, MIM_EINVAL, "set_create_f32: dim must be 1..%d (got %d)", kFltMaxDim, dim);
    if (step < (int64_t)4 * dim || step % 4 != 0)
        return fail(c, MIM_EINVAL, "set_create_f32: step %lld must be a multiple of 4 and >= 4 * dim = %d",
                    (long long)step, 4 * dim);
    SetRec r{};
    r.fdim = dim;
    r.fpad = (dim + 3) & ~3;
    return set_create_rows_locked(c, "set_create_f32", r, desc, step, (size_t)dim * sizeof(float),
                                  (size_t)r.fpad * sizeof(float), kFltRowPad, kp, n, on_device, set_id);
}

mim_status mim_set_create_f32(mim_ctx* c, const float* desc, int64_t step, const float* kp, int32_t n, int32_t dim,
                              int32_t on_device, int32_t* set_id) {
    if (!c) return MIM_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    return set_create_f32_locked(c, desc, step, kp, n, dim, on_device, set_id);
}

static void sets_truncate_locked(mim_ctx* c, int n_keep);

mim_status mim_sets_create(mim_ctx* c, int32_t count, const float* const* desc, const float* const* kp,
                           const int32_t* rows, int32_t dim, int32_t on_device, int32_t* first_id) {
    if (!c) return MIM_EINVAL;
    if (count < 0 || !first_id || (count > 0 && (!desc || !kp || !rows)))
        return fail(c, MIM_EINVAL, "sets_create: bad arguments");
    std::lock_guard<std::mutex> lk(c->mu);
    const int n0 = (int)c->sets.size();
    const Arena::Mark m0 = c->arena.pos();
    // all or nothing: the sets of this call go, and so does the storage a set that failed part-way
    // took (it is not in `sets` yet, so only the arena mark of the call's start covers it)
    auto undo = [&](mim_status st) {
        if (!on_device) (void)hipStreamSynchronize(c->stream);  // copies already enqueued read the host rows
        if ((int)c->sets.size() > n0) sets_truncate_locked(c, n0);
        c->arena.seek(m0);
        return st;
    };
    for (int i = 0; i < count; ++i) {
        int32_t id = -1;
        const mim_status st = set_create_locked(c, desc[i], kp[i], rows[i], dim, on_device, &id, false);
        if (st != MIM_OK) return undo(st);
    }
    // host rows: every copy enqueued, one wait for all of them (the host buffers may go away after)
    if (!on_device && count > 0) {
        const hipError_t e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) return undo(fail(c, MIM_EDEVICE, "sets_create: hipStreamSynchronize: %s", hipGetErrorString(e)));
    }
    *first_id = n0;
    return MIM_OK;
}

mim_status mim_sets_clear(mim_ctx* c) {
    if (!c) return MIM_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    // no host wait: every write into the arena (prep kernels, copies of host rows) is ordered on the
    // ctx stream after the previous batch, whose groups join back into that stream
    c->sets.clear();
    c->pend.clear();
    c->pend_set.clear();
    c->flushes.clear();
    c->arena.rewind();
    ++c->sets_gen;
    return MIM_OK;
}

// Drops the sets with ids >= n_keep (0 <= n_keep <= sets.size()) and rewinds the arena to `mark`, the arena
// before the first dropped set's storage; n_keep == sets.size() drops nothing and only rewinds (what a failed
// set creation left behind).  The generation stays: callers that change what the user's ids mean bump it.
static void drop_sets_from(mim_ctx* c, int n_keep, Arena::Mark mark) {
    // the dropped sets' pending preps go; their storage (and prep flags blocks that cover only dropped
    // sets) is reused by later sets, ordered on the ctx stream after the work already enqueued, as
    // for mim_sets_clear
    size_t m = 0;
    for (size_t j = 0; j < c->pend.size(); ++j)
        if (c->pend_set[j] < n_keep) {
            c->pend[m] = c->pend[j];
            c->pend_set[m++] = c->pend_set[j];
        }
    c->pend.resize(m);
    c->pend_set.resize(m);
    for (const auto& f : c->flushes)
        if (f.first < n_keep && mark < f.second) mark = f.second;  // a kept set's flags lie beyond
    c->flushes.erase(std::remove_if(c->flushes.begin(), c->flushes.end(),
                                    [n_keep](const std::pair<int, Arena::Mark>& f) { return f.first >= n_keep; }),
                     c->flushes.end());
    c->arena.seek(mark);
    c->sets.resize(n_keep);
}

// mim_sets_truncate (n_keep < sets.size(), checked by the callers); with the lock held
static void sets_truncate_locked(mim_ctx* c, int n_keep) {
    drop_sets_from(c, n_keep, c->sets[n_keep].mark);
    ++c->sets_gen;
}

mim_status mim_sets_truncate(mim_ctx* c, int32_t n_keep) {
    if (!c) return MIM_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (n_keep < 0 || n_keep > (int)c->sets.size())
        return fail(c, MIM_EINVAL, "sets_truncate: %d sets registered, %d to keep", (int)c->sets.size(), n_keep);
    if (n_keep == (int)c->sets.size()) return MIM_OK;
    HIPCHK(c, hipSetDevice(c->device));
    sets_truncate_locked(c, n_keep);
    return MIM_OK;
}

mim_status mim_sets_info(mim_ctx* c, int32_t* n_sets, int64_t* generation) {
    if (!c) return MIM_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (n_sets) *n_sets = (int32_t)c->sets.size();
    if (generation) *generation = (int64_t)c->sets_gen;
    return MIM_OK;
}

mim_status mim_set_rows(mim_ctx* c, int32_t set_id, int32_t cap, float* desc, float* kp_xy, int32_t* n_rows) {
    if (!c) return MIM_EINVAL;
    if (!n_rows || cap < 0) return fail(c, MIM_EINVAL, "set_rows: bad arguments");
    std::lock_guard<std::mutex> lk(c->mu);
    if (set_id < 0 || set_id >= (int)c->sets.size())
        return fail(c, MIM_EINVAL, "set_rows: set %d not registered (%d sets)", set_id, (int)c->sets.size());
    if (c->sets[set_id].is_bin())
        return fail(c, MIM_EINVAL, "set_rows: set %d holds binary descriptors, not float rows", set_id);
    if (c->sets[set_id].is_f32())
        return fail(c, MIM_EINVAL, "set_rows: set %d holds generic float rows of dim %d, not 128-column rows", set_id,
                    c->sets[set_id].fdim);
    HIPCHK(c, hipSetDevice(c->device));
    const SetDev& d = c->sets[set_id].d;
    *n_rows = d.n;
    const int m = std::min(d.n, cap);
    if (m > 0 && desc && d.f32)
        HIPCHK(c, hipMemcpyAsync(desc, d.f32, sizeof(float) * kDim * m, hipMemcpyDeviceToHost, c->stream));
    if (m > 0 && kp_xy && d.kp)
        HIPCHK(c, hipMemcpyAsync(kp_xy, d.kp, sizeof(float2) * m, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MIM_OK;
}

}  // extern "C"

// the distance schedule's knobs (knn_schedule.h), read per batch (tests switch them)
static KnnSchedKnobs knn_knobs() {
    KnnSchedKnobs k;
    if (const char* e = getenv("MIM_KNN_SUB")) k.sub_target = atoi(e);
    if (const char* e = getenv("MIM_KNN_DYN")) k.dyn = atoi(e) != 0;
    if (const char* e = getenv("MIM_KNN_TAIL")) k.tail = atoi(e) != 0;
    return k;
}

// resident distance-kernel blocks: CUs x blocks per CU (occupancy query), once per ctx
static mim_status device_limits(mim_ctx* c) {
    if (c->knn_grid == 0) {
        hipDeviceProp_t prop;
        HIPCHK(c, hipGetDeviceProperties(&prop, c->device));
        c->knn_grid = std::max(1, prop.multiProcessorCount * std::max(1, knn_blocks_per_cu()));
        c->n_cu = std::max(1, prop.multiProcessorCount);
    }
    return MIM_OK;
}

// The pairing rules of a problem's two sets (mim_batch_run and every entry that takes mim_problem records):
// both of one kind, one width or dim, a train set below 2^18 rows; cross: the query set is a train set too.
static mim_status check_problem_sets(mim_ctx* c, int i, int qs, int ts, bool cross) {
    if (qs < 0 || qs >= (int)c->sets.size() || ts < 0 || ts >= (int)c->sets.size())
        return fail(c, MIM_EINVAL, "problem %d: bad set id (%d, %d)", i, qs, ts);
    if (c->sets[ts].d.n >= (1 << 18))  // BFMatcher::knnMatchImpl: train rows < 1 << 18 (IMGIDX_SHIFT)
        return fail(c, MIM_EINVAL, "problem %d: train set of %d rows exceeds OpenCV's 2^18 limit", i,
                    c->sets[ts].d.n);
    const SetRec &Q = c->sets[qs], &T = c->sets[ts];
    if (Q.is_bin() != T.is_bin())
        return fail(c, MIM_EINVAL, "problem %d: set %d holds %s descriptors and set %d %s ones", i, qs,
                    Q.is_bin() ? "binary" : "float", ts, T.is_bin() ? "binary" : "float");
    if (Q.bin_width != T.bin_width)
        return fail(c, MIM_EINVAL, "problem %d: binary sets of different widths (%d and %d bytes)", i, Q.bin_width,
                    T.bin_width);
    if (Q.is_f32() != T.is_f32())
        return fail(c, MIM_EINVAL, "problem %d: set %d holds %s rows and set %d %s ones", i, qs,
                    Q.is_f32() ? "generic float (mim_set_create_f32)" : "128-D float (mim_set_create)", ts,
                    T.is_f32() ? "generic float (mim_set_create_f32)" : "128-D float (mim_set_create)");
    if (Q.fdim != T.fdim)
        return fail(c, MIM_EINVAL, "problem %d: generic float sets of different dims (%d and %d)", i, Q.fdim, T.fdim);
    if (cross && Q.d.n >= (1 << 18))  // the query set is the reverse direction's train set
        return fail(c, MIM_EINVAL, "problem %d: query set of %d rows exceeds OpenCV's 2^18 limit under a cross-check "
                                   "filter", i, Q.d.n);
    return MIM_OK;
}

// A call's problem records checked and turned into the schedule's input.  sift_i8: 128-D sets enter as i8
// problems (the batch); else as float problems at dim 128 (top-k, radius).  qoff: the problems' first rows in
// the concatenated queries (n + 1 entries).
struct ProblemList {
    std::vector<KnnSchedProblem> in;
    std::vector<long long> qoff;
    int max_nq = 0;
};
static mim_status problem_list(mim_ctx* c, const mim_problem* problems, int n, bool cross, bool sift_i8,
                               ProblemList& L) {
    L.in.resize(n);
    L.qoff.assign(n + 1, 0);
    for (int i = 0; i < n; ++i) {
        const int qs = problems[i].query_set, ts = problems[i].train_set;
        const mim_status s = check_problem_sets(c, i, qs, ts, cross);
        if (s != MIM_OK) return s;
        const SetRec &Q = c->sets[qs], &T = c->sets[ts];
        L.in[i] = KnnSchedProblem{Q.d.n, T.d.n, T.d.n_tiles, Q.is_bin()};
        L.in[i].fdim = Q.is_sift() && !sift_i8 ? kDim : Q.fdim;
        L.qoff[i + 1] = L.qoff[i] + Q.d.n;
        L.max_nq = std::max(L.max_nq, Q.d.n);
    }
    return MIM_OK;
}

// The sweep's part of a work item (HamSweepWork, FltSweepWork): a piece of knn_hamming_plan / knn_float_plan with
// its problem's rows.  flags: a 128-D problem's pieces carry the sets' integrality flags (an i8 kernel runs too).
static HamSweepWork ham_sweep_work(const mim_ctx* c, const mim_problem& pr, const HamPiece& hp) {
    const SetRec &Q = c->sets[pr.query_set], &T = c->sets[pr.train_set];
    return HamSweepWork{reinterpret_cast<const uint32_t*>(Q.d.frag), reinterpret_cast<const uint32_t*>(T.d.frag), Q.d.n,
                        hp.q0, hp.r0, hp.r1, Q.bin_pad / 4};
}
static FltSweepWork flt_sweep_work(const mim_ctx* c, const mim_problem& pr, const FltPiece& fp, bool flags) {
    const SetRec &Q = c->sets[pr.query_set], &T = c->sets[pr.train_set];
    const bool fl = flags && Q.is_sift();
    return FltSweepWork{Q.d.f32, T.d.f32, fl ? Q.d.flags : nullptr, fl ? T.d.flags : nullptr, Q.d.n, fp.q0, fp.r0, fp.r1,
                        Q.flt_dim(), Q.flt_stride(), T.d.n, (((uintptr_t)Q.d.f32 | (uintptr_t)T.d.f32) & 15) == 0 ? 1 : 0};
}
// A schedule's pieces as the work items of a top-k or radius kernel: the sweep's part and dest(problem, split)
template <class Work, class Dest>
static std::vector<Work> ham_works(const mim_ctx* c, const mim_problem* problems, const KnnSchedule& S, Dest dest) {
    std::vector<Work> v;
    v.reserve(S.ham.size());
    for (const HamPiece& hp : S.ham) v.push_back(Work{ham_sweep_work(c, problems[hp.problem], hp), dest(hp.problem, hp.split)});
    return v;
}
template <class Work, class Dest>
static std::vector<Work> flt_works(const mim_ctx* c, const mim_problem* problems, const KnnSchedule& S, bool flags, Dest dest) {
    std::vector<Work> v;
    v.reserve(S.flt.size());
    for (const FltPiece& fp : S.flt)
        v.push_back(Work{flt_sweep_work(c, problems[fp.problem], fp, flags), dest(fp.problem, fp.split)});
    return v;
}

// ---------------------------------------------------------------------------------------------
// Problem table + distance work list (knn_schedule.h).  Work items of one problem are placed at
// block indices with equal (index % 8) so they share one XCD's L2 under round-robin dispatch
// (speed only).
// ---------------------------------------------------------------------------------------------
// filter != 0 (cross-check): the n problems are followed by their shadows (knn_cross_problems), which
// take part in the distance stage only; ProbDev i < n is still problem i.
static mim_status build_tables(mim_ctx* c, const mim_problem* user_problems, int n_user, int max_iters, int filter = 0) {
    const mim_problem* problems = user_problems;
    int n = n_user;
    mim_status fs = flush_preps(c);  // the sets' device tiles and flags, before ProbDev copies them
    if (fs != MIM_OK) return fs;
    fs = device_limits(c);
    if (fs != MIM_OK) return fs;
    ProblemList L;
    fs = problem_list(c, problems, n, filter != 0, true, L);
    if (fs != MIM_OK) return fs;
    std::vector<KnnSchedProblem>& in = L.in;
    // cross-check: the shadows join the problem list (binary problems under the fused kernel have none)
    std::vector<int> shadow_of;
    std::vector<mim_problem> ext;
    c->knn_cross = 0;
    if (filter != 0) {
        const char* e = getenv("MIM_CROSS_FUSED");  // read per launch; 0: binary problems take shadow sweeps too
        const bool fused = !(e && e[0] == '0');
        in = knn_cross_problems(in, fused, shadow_of);
        ext.assign(user_problems, user_problems + n_user);
        ext.resize(in.size());
        bool any_fused = false;
        for (int i = 0; i < n_user; ++i) {
            if (shadow_of[i] >= 0) ext[shadow_of[i]] = mim_problem{user_problems[i].train_set, user_problems[i].query_set};
            else any_fused = true;
        }
        problems = ext.data();
        n = (int)in.size();
        c->knn_cross = any_fused ? 2 : 1;
    }
    const KnnSchedule S = knn_schedule(in, c->knn_grid, c->n_cu, max_iters, knn_knobs());
    c->h_probs.assign(n, ProbDev{});
    for (int i = 0; i < n; ++i) {
        ProbDev& P = c->h_probs[i];
        const KnnSchedSlot& s = S.slots[i];
        P.q = c->sets[problems[i].query_set].d;
        P.t = c->sets[problems[i].train_set].d;
        P.nsplit = s.nsplit;
        P.q_pad = s.q_pad;
        P.part_off = s.part_off;
        P.good_off = s.good_off;
        P.it_off = s.it_off;
    }
    const std::vector<KnnWork>& works = S.works;
    const std::vector<int>& seg = S.seg;
    const long long part = S.part, good = S.good;
    HIPCHK(c, c->probs.ensure(sizeof(ProbDev) * std::max(n, 1)));
    HIPCHK(c, c->works.ensure(sizeof(KnnWork) * std::max<size_t>(works.size(), 1) + sizeof(int) * seg.size()));
    HIPCHK(c, c->parts.ensure(sizeof(Top2) * std::max<long long>(part, 1)));
    // cross-check: a fused binary problem's column minima colmin[nt], the others' shadows
    std::vector<CrossDev> cross;
    std::vector<long long> col_off;
    long long n_col = 0;
    if (filter != 0) {
        col_off.assign(n_user, -1);
        for (int i = 0; i < n_user; ++i)
            if (shadow_of[i] < 0) {
                col_off[i] = n_col;
                n_col += std::max(in[i].nt, 1);
            }
        HIPCHK(c, c->colmin.ensure(sizeof(uint32_t) * std::max<long long>(n_col, 1)));
        HIPCHK(c, c->cross_tab.ensure(sizeof(CrossDev) * std::max(n_user, 1)));
        cross.resize(n_user);
        for (int i = 0; i < n_user; ++i)
            cross[i] = CrossDev{shadow_of[i] < 0 ? c->colmin.as<uint32_t>() + col_off[i] : nullptr, shadow_of[i], 0};
    }
    c->n_colmin = n_col;
    // the Hamming pieces with their pointers (parts is sized above)
    std::vector<HamWork> ham;
    std::vector<HamCrossWork> hamx;
    ham.reserve(S.ham.size());
    for (const HamPiece& hp : S.ham) {
        const ProbDev& P = c->h_probs[hp.problem];
        const HamSweepWork f = ham_sweep_work(c, problems[hp.problem], hp);
        const HamWork hw{f.q, f.t, c->parts.as<Top2>() + P.part_off + (long long)hp.split * P.q_pad, f.nq, f.q0, f.r0,
                         f.r1, f.wdw, 0};
        if (filter != 0 && hp.problem < n_user && shadow_of[hp.problem] < 0)
            hamx.push_back(HamCrossWork{hw, c->colmin.as<uint32_t>() + col_off[hp.problem]});
        else
            ham.push_back(hw);
    }
    if (!ham.empty()) HIPCHK(c, c->ham_works.ensure(sizeof(HamWork) * ham.size()));
    if (!hamx.empty()) HIPCHK(c, c->ham_cross_works.ensure(sizeof(HamCrossWork) * hamx.size()));
    // and the generic-float pieces
    std::vector<FltWork> flt;
    flt.reserve(S.flt.size());
    for (const FltPiece& fp : S.flt) {
        const ProbDev& P = c->h_probs[fp.problem];
        const FltSweepWork f = flt_sweep_work(c, problems[fp.problem], fp, false);
        flt.push_back(FltWork{f.q, f.t, c->parts.as<Top2>() + P.part_off + (long long)fp.split * P.q_pad, f.nq, f.q0,
                              f.r0, f.r1, f.dim, f.dp});
    }
    if (!flt.empty()) HIPCHK(c, c->flt_works.ensure(sizeof(FltWork) * flt.size()));
    HIPCHK(c, c->good_q.ensure(sizeof(int32_t) * good));
    HIPCHK(c, c->good_t.ensure(sizeof(int32_t) * good));
    HIPCHK(c, c->pts.ensure(sizeof(float4) * good));
    HIPCHK(c, c->n_good.ensure(sizeof(int) * std::max(n, 1)));
    HIPCHK(c, c->masks.ensure(good));
    // the device tables are rewritten in stream order (after the previous batch's kernels)
    StageWriter up(c->stage, vec_bytes(c->h_probs) + vec_bytes(works) + vec_bytes(seg) + vec_bytes(ham) + vec_bytes(flt) +
                                  vec_bytes(hamx) + vec_bytes(cross),
                   c->stream);
    up.put(c->probs, c->h_probs);
    up.put(c->works.p, works.data(), vec_bytes(works), seg.data(), vec_bytes(seg));
    up.put(c->ham_works, ham);
    up.put(c->flt_works, flt);
    up.put(c->ham_cross_works, hamx);
    up.put(c->cross_tab, cross);
    HIPCHK(c, up.done());
    c->n_ham_works = (int)ham.size();
    c->n_ham_cross_works = (int)hamx.size();
    c->n_flt_works = (int)flt.size();
    c->h_good_off.resize(n_user);
    for (int i = 0; i < n_user; ++i) c->h_good_off[i] = c->h_probs[i].good_off;
    c->last_n = n_user;
    c->n_works = (int)works.size();
    c->n_knn_blocks = S.n_blocks;
    c->knn_dyn = S.dyn;
    c->knn_whole = S.dyn;
    for (int i = 0; i < n; ++i)
        if (knn_is_i8(in[i]) && S.slots[i].nsplit != 1) c->knn_whole = false;
    if (S.dyn) HIPCHK(c, c->knn_ctr.ensure(8 * sizeof(int)));
    return MIM_OK;
}

// Kernel timing: an event after every launch on the stream it ran on; a kernel's time is the gap to
// the previous event of the same stream (with pipelined groups these are the kernels' own spans,
// overlap with other groups included).
static void ev_mark(mim_ctx* c, const char* name) {
    if (!c->timing) return;
    hipEvent_t e;
    if (!c->ev_pool.empty()) {
        e = c->ev_pool.back();
        c->ev_pool.pop_back();
    } else if (hipEventCreate(&e) != hipSuccess) {
        return;
    }
    (void)hipEventRecord(e, c->cur);
    if (!strcmp(name, "begin")) ++c->ev_seq;
    c->evs.push_back({name, c->cur, e, c->ev_seq});
}

static void ev_collect(mim_ctx* c) {
    if (c->evs.empty()) return;
    for (auto& e : c->evs) (void)hipEventSynchronize(e.e);
    c->last_ms.clear();
    // kernel time summed over every batch since the last collection
    std::map<hipStream_t, const mim_ctx::Ev*> prev;
    for (auto& e : c->evs) {
        auto it = prev.find(e.s);
        if (it != prev.end() && it->second->seq == e.seq) {
            float ms = 0;
            (void)hipEventElapsedTime(&ms, it->second->e, e.e);
            c->last_ms[e.name] += ms;
        }
        prev[e.s] = &e;
    }
    for (auto& e : c->evs) c->ev_pool.push_back(e.e);
    c->evs.clear();
}

// kappa of the distance kernel's ratio mode (knn.hip): ratio^2 (1 + 2^-18) covers the three float
// roundings of sqrtf(d1) < ratio * sqrtf(d2), a further 2^-20 and the round-up the kernel's own float
// product.  0 = exact top-2: ratios whose kappa is not below 1, and MIM_KNN_RATIO=0 (read per launch).
static float knn_ratio_kappa(float ratio) {
    const char* e = getenv("MIM_KNN_RATIO");
    if (e && e[0] == '0') return 0.f;
    if (!(ratio > 0.f && ratio < 1.f)) return 0.f;
    const double k = (double)ratio * (double)ratio * (1.0 + 1.0 / 262144.0) * (1.0 + 1.0 / 1048576.0);
    const float kf = nextafterf((float)k, 2.f);
    return kf < 1.f ? kf : 0.f;
}

// The ratio mode's verdict form (knn.hip, knn2_i8_kernel<2>): a failing query's record carries no valid
// nearest index, which is sound only where the piece's own verdict is final, so it runs for whole sweeps
// of one split alone (KnnSchedule::dyn without tail pieces).  MIM_KNN_FLIP=0 (read per launch) keeps the
// ratio mode.  Returns the ratio for the kernel's own test, 0 = off.
static float knn_flip_ratio(const mim_ctx* c, float ratio, float kappa) {
    const char* e = getenv("MIM_KNN_FLIP");
    if (e && e[0] == '0') return 0.f;
    return kappa > 0.f && kappa < 1.f && c->knn_whole ? ratio : 0.f;
}

static void knn_launch(mim_ctx* c, float kappa = 0.f, float flip_ratio = 0.f) {
    const KnnWork* w = c->works.as<KnnWork>();
    launch_knn(c->probs.as<ProbDev>(), w, c->n_works, reinterpret_cast<const int*>(w + c->n_works), c->n_knn_blocks,
               c->parts.as<Top2>(), c->knn_dyn ? c->knn_ctr.as<int>() : nullptr, kappa, flip_ratio, c->cur);
    launch_knn_hamming(c->ham_works.as<HamWork>(), c->n_ham_works, c->cur);
    launch_knn_hamming_cross(c->ham_cross_works.as<HamCrossWork>(), c->n_ham_cross_works, c->colmin.as<uint32_t>(),
                             c->n_colmin, c->cur);
    launch_knn_float(c->flt_works.as<FltWork>(), c->n_flt_works, c->cur);
}

// distance + ratio kernels of the batch's problems
// filter != 0: the cross-check compaction instead of the ratio kernel, behind the exact distance kernel
// (the reverse top-1 and the mutuality test need exact nearest indices, which the ratio and verdict modes
// do not keep); match_idx / match_dist: mim_match_cross_sets' per-query rows
static mim_status knn_ratio_locked(mim_ctx* c, int n, float ratio, bool emit_knn, int filter = 0,
                                   int32_t* match_idx = nullptr, float* match_dist = nullptr) {
    c->cur = c->stream;
    ev_mark(c, "begin");
    // the ratio test is the only reader of the top-2 unless the knnMatch rows are emitted
    const float kappa = emit_knn || filter != 0 ? 0.f : knn_ratio_kappa(ratio);
    const float flip_ratio = knn_flip_ratio(c, ratio, kappa);
    c->knn_mode = flip_ratio > 0.f ? 2 : kappa > 0.f ? 1 : 0;
    knn_launch(c, kappa, flip_ratio);
    HIPCHK(c, hipGetLastError());
    ev_mark(c, "knn");
    if (filter != 0)
        launch_cross(c->probs.as<ProbDev>(), c->cross_tab.as<CrossDev>(), n, c->parts.as<Top2>(), ratio, filter,
                     c->good_q.as<int32_t>(), c->good_t.as<int32_t>(), c->pts.as<float4>(), c->n_good.as<int>(),
                     match_idx, match_dist, c->cur);
    else
        launch_ratio(c->probs.as<ProbDev>(), n, c->parts.as<Top2>(), ratio, c->good_q.as<int32_t>(), c->good_t.as<int32_t>(),
                     c->pts.as<float4>(), c->n_good.as<int>(), emit_knn ? c->knn_idx.as<int32_t>() : nullptr,
                     emit_knn ? c->knn_dist.as<float>() : nullptr, c->cur);
    HIPCHK(c, hipGetLastError());
    ev_mark(c, "ratio");
    return MIM_OK;
}

// The scope of a host-buffer entry's private sets (mim_knn2_*, mim_knn_*, mim_radius_* on host rows): make_q and
// make_t append the query and the train set after the user's sets, body runs on the pair, and then, whatever
// any of them returned, the private sets go with their pending preps and their storage (drop_sets_from), and
// the batch and radius records that named them are invalidated.  The user's ids and the generation stay.
template <class MakeQ, class MakeT, class Body>
static mim_status with_private_sets(mim_ctx* c, MakeQ make_q, MakeT make_t, Body body) {
    const int base = (int)c->sets.size();
    const Arena::Mark mark = c->arena.pos();
    int32_t sq = -1, st = -1;
    mim_status s = make_q(&sq);
    if (s == MIM_OK) s = make_t(&st);
    if (s == MIM_OK) s = body(mim_problem{sq, st});
    ev_collect(c);
    drop_sets_from(c, base, mark);
    invalidate_batch(c);
    c->rad.valid = false;
    return s;
}

// body of the k = 2 host-buffer entries: the batch's distance stage on the one problem, its knnMatch rows back
static mim_status knn2_host_body(mim_ctx* c, const mim_problem& pr, int nq, int32_t* idx, float* dist) {
    mim_status s = build_tables(c, &pr, 1, 1);
    if (s != MIM_OK) return s;
    HIPCHK(c, c->knn_idx.ensure(sizeof(int32_t) * 2 * nq));
    HIPCHK(c, c->knn_dist.ensure(sizeof(float) * 2 * nq));
    s = knn_ratio_locked(c, 1, 0.9f, true);
    if (s != MIM_OK) return s;
    HIPCHK(c, hipMemcpyAsync(idx, c->knn_idx.p, sizeof(int32_t) * 2 * nq, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(dist, c->knn_dist.p, sizeof(float) * 2 * nq, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MIM_OK;
}

extern "C" {

mim_status mim_knn2_l2(mim_ctx* c, const float* q, int32_t nq, const float* t, int32_t nt, int32_t dim,
                       int32_t* idx, float* dist) {
    if (!c) return MIM_EINVAL;
    if (check_host_pair(c, "knn2_l2", q, nq, t, nt, nq <= 0 || (idx && dist)) != MIM_OK) return MIM_EINVAL;
    if (dim != kDim) return fail(c, MIM_EINVAL, "knn2_l2: dim must be %d", kDim);
    if (nq == 0) return MIM_OK;  // knnMatch on an empty query returns no rows
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<float> kp0((size_t)std::max(nq, nt) * 2, 0.f);
    return with_private_sets(
        c, [&](int32_t* id) { return set_create_locked(c, q, kp0.data(), nq, dim, 0, id); },
        [&](int32_t* id) { return set_create_locked(c, t ? t : kp0.data(), kp0.data(), nt, dim, 0, id); },
        [&](const mim_problem& pr) { return knn2_host_body(c, pr, nq, idx, dist); });
}

mim_status mim_knn2_hamming(mim_ctx* c, const uint8_t* q, int32_t nq, const uint8_t* t, int32_t nt, int32_t width,
                            int32_t* idx, float* dist) {
    if (!c) return MIM_EINVAL;
    if (check_host_pair(c, "knn2_hamming", q, nq, t, nt, nq <= 0 || (idx && dist)) != MIM_OK) return MIM_EINVAL;
    if (width < 1 || width > 64) return fail(c, MIM_EINVAL, "knn2_hamming: width must be 1..64 bytes (got %d)", width);
    if (nq == 0) return MIM_OK;  // knnMatch on an empty query returns no rows
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<float> kp0((size_t)std::max(nq, nt) * 2, 0.f);
    return with_private_sets(
        c, [&](int32_t* id) { return set_create_bin_locked(c, q, width, kp0.data(), nq, width, 0, id); },
        [&](int32_t* id) { return set_create_bin_locked(c, t, width, kp0.data(), nt, width, 0, id); },
        [&](const mim_problem& pr) { return knn2_host_body(c, pr, nq, idx, dist); });
}

mim_status mim_knn2_l2_f32(mim_ctx* c, const float* q, int32_t nq, const float* t, int32_t nt, int32_t dim,
                           int32_t* idx, float* dist) {
    if (!c) return MIM_EINVAL;
    if (check_host_pair(c, "knn2_l2_f32", q, nq, t, nt, nq <= 0 || (idx && dist)) != MIM_OK) return MIM_EINVAL;
    if (dim < 1 || dim > kFltMaxDim)
        return fail(c, MIM_EINVAL, "knn2_l2_f32: dim must be 1..%d (got %d)", kFltMaxDim, dim);
    if (nq == 0) return MIM_OK;  // knnMatch on an empty query returns no rows
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<float> kp0((size_t)std::max(nq, nt) * 2, 0.f);
    return with_private_sets(
        c, [&](int32_t* id) { return set_create_f32_locked(c, q, (int64_t)4 * dim, kp0.data(), nq, dim, 0, id); },
        [&](int32_t* id) { return set_create_f32_locked(c, t, (int64_t)4 * dim, kp0.data(), nt, dim, 0, id); },
        [&](const mim_problem& pr) { return knn2_host_body(c, pr, nq, idx, dist); });
}

mim_status mim_ratio_filter(mim_ctx* c, const int32_t* idx, const float* dist, int32_t nq, float ratio,
                            int32_t* q_out, int32_t* t_out, int32_t* n_good) {
    if (!c) return MIM_EINVAL;
    if (nq < 0 || !n_good || (nq > 0 && (!idx || !dist))) return fail(c, MIM_EINVAL, "ratio_filter: bad arguments");
    *n_good = 0;
    if (nq == 0) return MIM_OK;
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // knnMatch rows -> one train split of Top2 partials, then the device ratio/compaction kernel
    int max_t = 0;
    std::vector<Top2> parts(nq);
    for (int i = 0; i < nq; ++i) {
        const int a = idx[2 * i], b = idx[2 * i + 1];
        parts[i] = Top2{a < 0 ? FLT_MAX : dist[2 * i], a < 0 ? INT_MAX : a, b < 0 ? FLT_MAX : dist[2 * i + 1],
                        b < 0 ? INT_MAX : b};
        max_t = std::max(max_t, std::max(a, b));
    }
    const int q_pad = (nq + kKnnBlockQ - 1) / kKnnBlockQ * kKnnBlockQ;
    const size_t nkp = (size_t)std::max(nq, max_t + 1);
    HIPCHK(c, c->parts.ensure(sizeof(Top2) * q_pad));
    HIPCHK(c, c->rws.scratch.ensure(sizeof(float2) * nkp));
    HIPCHK(c, c->good_q.ensure(sizeof(int32_t) * nq));
    HIPCHK(c, c->good_t.ensure(sizeof(int32_t) * nq));
    HIPCHK(c, c->pts.ensure(sizeof(float4) * nq));
    HIPCHK(c, c->n_good.ensure(sizeof(int)));
    HIPCHK(c, c->probs.ensure(sizeof(ProbDev)));
    HIPCHK(c, hipMemsetAsync(c->rws.scratch.p, 0, sizeof(float2) * nkp, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->parts.p, parts.data(), sizeof(Top2) * nq, hipMemcpyHostToDevice, c->stream));
    ProbDev P{};
    P.q.n = nq;
    P.q.kp = c->rws.scratch.as<float2>();
    P.t.kp = c->rws.scratch.as<float2>();
    P.nsplit = 1;
    P.q_pad = q_pad;
    HIPCHK(c, hipMemcpyAsync(c->probs.p, &P, sizeof P, hipMemcpyHostToDevice, c->stream));
    launch_ratio(c->probs.as<ProbDev>(), 1, c->parts.as<Top2>(), ratio, c->good_q.as<int32_t>(),
                 c->good_t.as<int32_t>(), c->pts.as<float4>(), c->n_good.as<int>(), nullptr, nullptr, c->stream);
    HIPCHK(c, hipGetLastError());
    int ng = 0;
    HIPCHK(c, hipMemcpyAsync(&ng, c->n_good.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (ng > 0) {
        if (q_out) HIPCHK(c, hipMemcpy(q_out, c->good_q.p, sizeof(int32_t) * ng, hipMemcpyDeviceToHost));
        if (t_out) HIPCHK(c, hipMemcpy(t_out, c->good_t.p, sizeof(int32_t) * ng, hipMemcpyDeviceToHost));
    }
    *n_good = ng;
    invalidate_batch(c);
    return MIM_OK;
}

mim_status mim_knn2_sets_dev(mim_ctx* c, int32_t query_set, int32_t train_set, int32_t* idx_dev,
                             float* dist_dev) {
    if (!c || !idx_dev || !dist_dev) return MIM_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    mim_problem pr{query_set, train_set};
    mim_status s = build_tables(c, &pr, 1, 1);
    if (s != MIM_OK) return s;
    c->cur = c->stream;
    ev_mark(c, "begin");
    knn_launch(c);
    HIPCHK(c, hipGetLastError());
    ev_mark(c, "knn");
    launch_knn_emit(c->probs.as<ProbDev>(), c->h_probs[0].q.n, c->parts.as<Top2>(), idx_dev, dist_dev, c->stream);
    HIPCHK(c, hipGetLastError());
    ev_mark(c, "ratio");
    invalidate_batch(c);
    return MIM_OK;
}

// Top-k: the work lists of knn_hamming_plan / knn_float_plan over the call's problems, the
// distance kernels of knn_topk.hip into the top-k partials, then the merge into the caller's rows.  128-D
// sets go through the float kernel on their f32 rows (no prep is needed or flushed).  With the lock held.
static mim_status knn_topk_locked(mim_ctx* c, const mim_problem* problems, int n, int k, int32_t* idx_dev,
                                  float* dist_dev) {
    invalidate_batch(c);
    if (k < 1 || k > MIM_KNN_MAX_K) return fail(c, MIM_EINVAL, "knn: k must be 1..%d (got %d)", MIM_KNN_MAX_K, k);
    if (n < 0 || (n > 0 && !problems)) return fail(c, MIM_EINVAL, "knn: bad arguments");
    if (n == 0) return MIM_OK;
    mim_status s = device_limits(c);
    if (s != MIM_OK) return s;
    ProblemList L;
    s = problem_list(c, problems, n, false, false, L);  // 128-D sets: the float work list at dim 128
    if (s != MIM_OK) return s;
    const std::vector<KnnSchedProblem>& in = L.in;
    if (L.qoff[n] > 0 && (!idx_dev || !dist_dev)) return fail(c, MIM_EINVAL, "knn: null output");
    KnnSchedule S;
    S.slots.assign(n, KnnSchedSlot{});
    knn_hamming_plan(in, c->n_cu, S);
    knn_float_plan(in, c->n_cu, S);
    const KnnTopkLayout Lo = knn_topk_offsets(in, S.slots, k);
    c->topk_splits = 0;
    for (const KnnSchedSlot& sl : S.slots) c->topk_splits = std::max(c->topk_splits, sl.nsplit);
    HIPCHK(c, c->topk_parts.ensure(sizeof(TopkEnt) * std::max<long long>(Lo.part, 1)));
    HIPCHK(c, c->topk_probs.ensure(sizeof(TopkProb) * n));
    TopkEnt* parts = c->topk_parts.as<TopkEnt>();
    std::vector<TopkProb> probs(n);
    for (int i = 0; i < n; ++i)
        probs[i] = TopkProb{parts + Lo.part_off[i], idx_dev + Lo.out_off[i], dist_dev + Lo.out_off[i], in[i].nq,
                            S.slots[i].nsplit, S.slots[i].q_pad, 0};
    const auto out = [&](int p, int split) { return parts + Lo.part_off[p] + (long long)split * S.slots[p].q_pad * k; };
    const std::vector<TopkHamWork> ham = ham_works<TopkHamWork>(c, problems, S, out);
    const std::vector<TopkFltWork> flt = flt_works<TopkFltWork>(c, problems, S, false, out);
    if (!ham.empty()) HIPCHK(c, c->topk_ham_works.ensure(sizeof(TopkHamWork) * ham.size()));
    if (!flt.empty()) HIPCHK(c, c->topk_flt_works.ensure(sizeof(TopkFltWork) * flt.size()));
    // the device tables are rewritten in stream order (after the previous call's kernels)
    StageWriter up(c->stage, vec_bytes(probs) + vec_bytes(ham) + vec_bytes(flt), c->stream);
    up.put(c->topk_probs, probs);
    up.put(c->topk_ham_works, ham);
    up.put(c->topk_flt_works, flt);
    HIPCHK(c, up.done());
    c->cur = c->stream;
    ev_mark(c, "begin");
    launch_knn_topk_hamming(c->topk_ham_works.as<TopkHamWork>(), (int)ham.size(), k, c->cur);
    launch_knn_topk_float(c->topk_flt_works.as<TopkFltWork>(), (int)flt.size(), k, c->cur);
    HIPCHK(c, hipGetLastError());
    ev_mark(c, "knn");
    launch_knn_topk_merge(c->topk_probs.as<TopkProb>(), n, L.max_nq, k, c->cur);
    HIPCHK(c, hipGetLastError());
    ev_mark(c, "ratio");
    return MIM_OK;
}

mim_status mim_knn_batch_dev(mim_ctx* c, const mim_problem* problems, int32_t n, int32_t k, int32_t* idx_dev,
                             float* dist_dev) {
    if (!c) return MIM_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    return knn_topk_locked(c, problems, n, k, idx_dev, dist_dev);
}

mim_status mim_knn_sets_dev(mim_ctx* c, int32_t query_set, int32_t train_set, int32_t k, int32_t* idx_dev,
                            float* dist_dev) {
    if (!c) return MIM_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    const mim_problem pr{query_set, train_set};
    return knn_topk_locked(c, &pr, 1, k, idx_dev, dist_dev);
}

// body of the top-k host-buffer entries (no prep is flushed on this path)
static mim_status knn_topk_host_body(mim_ctx* c, const mim_problem& pr, int nq, int k, int32_t* idx, float* dist) {
    HIPCHK(c, c->knn_idx.ensure(sizeof(int32_t) * k * nq));
    HIPCHK(c, c->knn_dist.ensure(sizeof(float) * k * nq));
    const mim_status s = knn_topk_locked(c, &pr, 1, k, c->knn_idx.as<int32_t>(), c->knn_dist.as<float>());
    if (s != MIM_OK) return s;
    HIPCHK(c, hipMemcpyAsync(idx, c->knn_idx.p, sizeof(int32_t) * k * nq, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(dist, c->knn_dist.p, sizeof(float) * k * nq, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MIM_OK;
}

mim_status mim_knn_l2(mim_ctx* c, const float* q, int32_t nq, const float* t, int32_t nt, int32_t dim, int32_t k,
                      int32_t* idx, float* dist) {
    if (!c) return MIM_EINVAL;
    if (check_host_pair(c, "knn_l2", q, nq, t, nt, nq <= 0 || (idx && dist)) != MIM_OK) return MIM_EINVAL;
    if (dim < 1 || dim > kFltMaxDim) return fail(c, MIM_EINVAL, "knn_l2: dim must be 1..%d (got %d)", kFltMaxDim, dim);
    if (k < 1 || k > MIM_KNN_MAX_K) return fail(c, MIM_EINVAL, "knn_l2: k must be 1..%d (got %d)", MIM_KNN_MAX_K, k);
    if (nq == 0) return MIM_OK;  // knnMatch on an empty query returns no rows
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<float> kp0((size_t)std::max(nq, nt) * 2, 0.f);
    return with_private_sets(
        c, [&](int32_t* id) { return set_create_f32_locked(c, q, (int64_t)4 * dim, kp0.data(), nq, dim, 0, id); },
        [&](int32_t* id) { return set_create_f32_locked(c, t, (int64_t)4 * dim, kp0.data(), nt, dim, 0, id); },
        [&](const mim_problem& pr) { return knn_topk_host_body(c, pr, nq, k, idx, dist); });
}

mim_status mim_knn_hamming(mim_ctx* c, const uint8_t* q, int32_t nq, const uint8_t* t, int32_t nt, int32_t width,
                           int32_t k, int32_t* idx, float* dist) {
    if (!c) return MIM_EINVAL;
    if (check_host_pair(c, "knn_hamming", q, nq, t, nt, nq <= 0 || (idx && dist)) != MIM_OK) return MIM_EINVAL;
    if (width < 1 || width > 64) return fail(c, MIM_EINVAL, "knn_hamming: width must be 1..64 bytes (got %d)", width);
    if (k < 1 || k > MIM_KNN_MAX_K)
        return fail(c, MIM_EINVAL, "knn_hamming: k must be 1..%d (got %d)", MIM_KNN_MAX_K, k);
    if (nq == 0) return MIM_OK;  // knnMatch on an empty query returns no rows
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<float> kp0((size_t)std::max(nq, nt) * 2, 0.f);
    return with_private_sets(
        c, [&](int32_t* id) { return set_create_bin_locked(c, q, width, kp0.data(), nq, width, 0, id); },
        [&](int32_t* id) { return set_create_bin_locked(c, t, width, kp0.data(), nt, width, 0, id); },
        [&](const mim_problem& pr) { return knn_topk_host_body(c, pr, nq, k, idx, dist); });
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// Train collections: every query set against the same images, one list per query row.
// ---------------------------------------------------------------------------------------------
// the byte budget of one image group's partial lists; MIM_COLL_PART_BYTES, read per call (tests force one
// image per group)
static long long coll_part_budget() {
    long long b = 256LL << 20;
    if (const char* e = getenv("MIM_COLL_PART_BYTES")) b = atoll(e);
    return std::max<long long>(b, 1);
}

// One image group's plans, made on the host before anything of the call is enqueued.
struct CollGroup {
    int g0 = 0, n_images = 0;       // images [g0, g0 + n_images) of the collection
    std::vector<mim_problem> pairs;  // [query set][image of the group]
    KnnSchedule S, S8;               // Hamming / float pieces; the i8 units (128-D sets)
    KnnCollLayout Lo;
    size_t up_bytes() const {
        return sizeof(TopkHamWork) * S.ham.size() + sizeof(TopkFltWork) * S.flt.size() + vec_bytes(S8.works) +
               vec_bytes(S8.seg) + (sizeof(CollPart) + sizeof(CollI8Prob)) * pairs.size();
    }
};

// With the lock held.  The problems of a group are its (query set, image) pairs; the work lists are those of
// knn_hamming_plan / knn_float_plan (128-D sets at dim 128) and, for the 128-D sets again, the i8 units of
// knn_schedule_static: a 128-D pair is in both lists, and the sets' integrality flags decide on the device
// which kernel's blocks do its pairs (as radius_count_locked).
static mim_status knn_collection_locked(mim_ctx* c, const int32_t* query_sets, int n_queries, const int32_t* train_sets,
                                        int n_images, int k, int32_t* idx_dev, int32_t* img_dev, float* dist_dev) {
    invalidate_batch(c);
    c->rad.valid = false;
    if (k < 1 || k > MIM_KNN_MAX_K)
        return fail(c, MIM_EINVAL, "knn_collection: k must be 1..%d (got %d)", MIM_KNN_MAX_K, k);
    if (n_images < 1 || n_images > kCollMaxImages)
        return fail(c, MIM_EINVAL, "knn_collection: n_images must be 1..%d (got %d)", kCollMaxImages, n_images);
    if (n_queries < 0 || (n_queries > 0 && !query_sets) || !train_sets)
        return fail(c, MIM_EINVAL, "knn_collection: bad arguments");
    if (n_queries == 0) return MIM_OK;
    mim_status s = flush_preps(c);  // the 128-D sets' fragment tiles, norm blocks and flags
    if (s != MIM_OK) return s;
    s = device_limits(c);
    if (s != MIM_OK) return s;
    // every pair under the pairing rules, query set major
    std::vector<mim_problem> pairs((size_t)n_queries * n_images);
    for (int qi = 0; qi < n_queries; ++qi)
        for (int j = 0; j < n_images; ++j) pairs[(size_t)qi * n_images + j] = mim_problem{query_sets[qi], train_sets[j]};
    ProblemList L;
    s = problem_list(c, pairs.data(), (int)pairs.size(), false, false, L);
    if (s != MIM_OK) return s;
    std::vector<int> nq(n_queries), nt(n_images);
    long long rows = 0;
    for (int qi = 0; qi < n_queries; ++qi) rows += nq[qi] = c->sets[query_sets[qi]].d.n;
    for (int j = 0; j < n_images; ++j) nt[j] = c->sets[train_sets[j]].d.n;
    if (rows > 0 && (!idx_dev || !img_dev || !dist_dev)) return fail(c, MIM_EINVAL, "knn_collection: null output");
    if (rows == 0) return MIM_OK;
    const SetRec& Q0 = c->sets[query_sets[0]];
    const bool sift = Q0.is_sift();
    const std::vector<int> start = knn_coll_groups(nq, nt, Q0.is_bin(), sift, k, coll_part_budget());
    const int n_groups = (int)start.size() - 1;

    std::vector<CollGroup> groups(n_groups);
    size_t max_ham = 0, max_flt = 0, max_pairs = 0, max_w8 = 0, max_up = 0;
    long long max_part = 1;
    int i8_splits = 0;
    for (int g = 0; g < n_groups; ++g) {
        CollGroup& G = groups[g];
        G.g0 = start[g];
        G.n_images = start[g + 1] - start[g];
        const int gn = G.n_images, n = n_queries * gn;
        G.pairs.resize((size_t)n);
        std::vector<KnnSchedProblem> in((size_t)n);
        for (int qi = 0; qi < n_queries; ++qi)
            for (int j = 0; j < gn; ++j) {
                G.pairs[(size_t)qi * gn + j] = pairs[(size_t)qi * n_images + G.g0 + j];
                in[(size_t)qi * gn + j] = L.in[(size_t)qi * n_images + G.g0 + j];
            }
        G.S.slots.assign(n, KnnSchedSlot{});
        knn_hamming_plan(in, c->n_cu, G.S);
        knn_float_plan(in, c->n_cu, G.S);
        if (sift) {
            for (KnnSchedProblem& p : in) p.fdim = 0;  // the i8 schedule's view of the same pairs
            G.S8.slots.assign(n, KnnSchedSlot{});
            knn_schedule_static(in, c->knn_grid, -1, G.S8);
            for (const KnnSchedSlot& sl : G.S8.slots) i8_splits = std::max(i8_splits, sl.nsplit);
        }
        G.Lo = knn_coll_offsets(nq, gn, G.S.slots, sift ? &G.S8.slots : nullptr, k);
        max_ham = std::max(max_ham, G.S.ham.size());
        max_flt = std::max(max_flt, G.S.flt.size());
        max_pairs = std::max(max_pairs, G.pairs.size());
        max_w8 = std::max(max_w8, vec_bytes(G.S8.works) + vec_bytes(G.S8.seg));
        max_part = std::max(max_part, G.Lo.part);
        max_up = std::max(max_up, G.up_bytes());
    }
    // every buffer at its largest before the first launch: none is reallocated under a group's kernels
    HIPCHK(c, c->coll_parts.ensure(sizeof(TopkEnt) * max_part));
    HIPCHK(c, c->coll_queries.ensure(sizeof(CollQuery) * n_queries));
    HIPCHK(c, c->coll_tab.ensure(sizeof(CollPart) * max_pairs));
    if (max_ham) HIPCHK(c, c->coll_ham_works.ensure(sizeof(TopkHamWork) * max_ham));
    if (max_flt) HIPCHK(c, c->coll_flt_works.ensure(sizeof(TopkFltWork) * max_flt));
    if (sift) HIPCHK(c, c->coll_i8_probs.ensure(sizeof(CollI8Prob) * max_pairs));
    if (max_w8) HIPCHK(c, c->coll_i8_works.ensure(max_w8));
    c->coll_groups = n_groups;
    c->coll_i8_splits = i8_splits;
    TopkEnt* const parts = c->coll_parts.as<TopkEnt>();
    std::vector<CollQuery> queries(n_queries);
    for (int qi = 0; qi < n_queries; ++qi) queries[qi] = CollQuery{groups[0].Lo.out_off[qi], nq[qi], 0};
    c->cur = c->stream;
    ev_mark(c, "begin");
    for (int g = 0; g < n_groups; ++g) {
        const CollGroup& G = groups[g];
        const KnnCollLayout& Lo = G.Lo;
        const int n = (int)G.pairs.size();
        const auto out = [&](int p, int split) { return parts + Lo.part_off[p] + (long long)split * G.S.slots[p].q_pad * k; };
        const std::vector<TopkHamWork> ham = ham_works<TopkHamWork>(c, G.pairs.data(), G.S, out);
        const std::vector<TopkFltWork> flt = flt_works<TopkFltWork>(c, G.pairs.data(), G.S, true, out);
        std::vector<CollPart> tab(n);
        std::vector<CollI8Prob> probs8(sift ? n : 0);
        for (int i = 0; i < n; ++i) {
            const SetRec &Q = c->sets[G.pairs[i].query_set], &T = c->sets[G.pairs[i].train_set];
            tab[i] = CollPart{nullptr, parts + Lo.part_off[i], nullptr, nullptr, 0, 0, G.S.slots[i].nsplit,
                              G.S.slots[i].q_pad, G.g0 + i % G.n_images, 0};
            if (sift) {
                tab[i].a = parts + Lo.part8_off[i];
                tab[i].qflags = Q.d.flags;
                tab[i].tflags = T.d.flags;
                tab[i].na = 2 * G.S8.slots[i].nsplit;
                tab[i].qa_pad = G.S8.slots[i].q_pad;
                probs8[i] = CollI8Prob{Q.d, T.d, parts + Lo.part8_off[i], G.S8.slots[i].q_pad, 0};
            }
        }
        // the device tables are rewritten in stream order (after the previous group's kernels)
        StageWriter up(c->stage, max_up + vec_bytes(queries), c->stream);
        if (g == 0) up.put(c->coll_queries, queries);
        up.put(c->coll_tab, tab);
        up.put(c->coll_ham_works, ham);
        up.put(c->coll_flt_works, flt);
        up.put(c->coll_i8_probs, probs8);
        const size_t wb = vec_bytes(G.S8.works);
        if (wb) up.put(c->coll_i8_works.p, G.S8.works.data(), wb, G.S8.seg.data(), vec_bytes(G.S8.seg));
        HIPCHK(c, up.done());
        ev_mark(c, "coll_upload");  // the table copies, outside the kernels' spans as in the other entries
        launch_knn_topk_hamming(c->coll_ham_works.as<TopkHamWork>(), (int)ham.size(), k, c->cur);
        launch_knn_topk_float(c->coll_flt_works.as<TopkFltWork>(), (int)flt.size(), k, c->cur);
        if (wb) {
            const KnnWork* w = c->coll_i8_works.as<KnnWork>();
            launch_knn_topk_i8(c->coll_i8_probs.as<CollI8Prob>(), w, reinterpret_cast<const int*>(w + G.S8.works.size()),
                               G.S8.n_blocks, k, c->cur);
        }
        HIPCHK(c, hipGetLastError());
        ev_mark(c, "knn");
        launch_knn_coll_merge(c->coll_queries.as<CollQuery>(), n_queries, c->coll_tab.as<CollPart>(), G.n_images, L.max_nq, k,
                              g > 0, idx_dev, img_dev, dist_dev, c->cur);
        HIPCHK(c, hipGetLastError());
        ev_mark(c, "ratio");
    }
    return MIM_OK;
}

extern "C" {

mim_status mim_knn_collection_dev(mim_ctx* c, const int32_t* query_sets, int32_t n_queries, const int32_t* train_sets,
                                  int32_t n_images, int32_t k, int32_t* idx_dev, int32_t* img_dev, float* dist_dev) {
    if (!c) return MIM_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    return knn_collection_locked(c, query_sets, n_queries, train_sets, n_images, k, idx_dev, img_dev, dist_dev);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// Radius matching: count + scan, then fill + sort + emit of the last count.
// ---------------------------------------------------------------------------------------------
static RadArgs radius_args(mim_ctx* c) {
    RadArgs a{};
    a.counts = c->rad_counts.as<int>();
    a.cursor = c->rad_cursor.as<int>();
    a.offsets = c->rad_offsets.as<long long>();
    a.keys = c->rad_keys.as<unsigned long long>();
    a.flt_t = radius_flt_threshold(c->rad.r);
    a.ham_t = radius_ham_threshold(c->rad.r);
    a.int_t2 = radius_int_threshold(c->rad.r);
    return a;
}

// one pass of the three distance kernels over the work items the last count left on the device
static void radius_launch(mim_ctx* c, const RadArgs& a, bool fill) {
    const KnnWork* w = c->rad_i8_works.as<KnnWork>();
    launch_radius_hamming(c->rad_ham_works.as<RadHamWork>(), c->rad.n_ham, a, fill, c->cur);
    launch_radius_float(c->rad_flt_works.as<RadFltWork>(), c->rad.n_flt, a, fill, c->cur);
    if (c->rad.n_i8_works > 0)
        launch_radius_i8(c->rad_probs.as<RadI8Prob>(), w, reinterpret_cast<const int*>(w + c->rad.n_i8_works),
                         c->rad.n_i8_blocks, a, fill, c->cur);
}

// With the lock held.  The work lists are those of knn_hamming_plan / knn_float_plan (128-D sets at dim 128, as
// the top-k entries) and, for the 128-D sets again, the i8 units of knn_schedule_static: a 128-D problem is in
// both lists, and the sets' integrality flags decide on the device which kernel's blocks do its pairs.
static mim_status radius_count_locked(mim_ctx* c, const mim_problem* problems, int n, float r, int64_t* offsets_dev,
                                      int64_t* total) {
    invalidate_batch(c);
    c->rad.valid = false;
    if (!total || n < 0 || (n > 0 && !problems)) return fail(c, MIM_EINVAL, "radius: bad arguments");
    *total = 0;
    if (!radius_arg_ok(r))
        return fail(c, MIM_EINVAL, "radius: max_distance must be above FLT_EPSILON (got %g)", (double)r);
    mim_status s = flush_preps(c);  // the 128-D sets' fragment tiles, norm blocks and flags
    if (s != MIM_OK) return s;
    s = device_limits(c);
    if (s != MIM_OK) return s;
    ProblemList L;
    s = problem_list(c, problems, n, false, false, L);
    if (s != MIM_OK) return s;
    const std::vector<KnnSchedProblem>& in = L.in;
    const std::vector<long long>& qoff = L.qoff;
    std::vector<KnnSchedProblem> in8 = in;  // the i8 schedule's view: the 128-D problems, every other out of it
    for (int i = 0; i < n; ++i) {
        in8[i].bin = !c->sets[problems[i].query_set].is_sift();
        in8[i].fdim = 0;
    }
    const long long nqs = qoff[n];
    KnnSchedule S, S8;
    S.slots.assign(n, KnnSchedSlot{});
    S8.slots.assign(n, KnnSchedSlot{});
    knn_hamming_plan(in, c->n_cu, S);
    knn_float_plan(in, c->n_cu, S);
    knn_schedule_static(in8, c->knn_grid, -1, S8);
    const auto first = [&](int p, int) { return qoff[p]; };
    const std::vector<RadHamWork> ham = ham_works<RadHamWork>(c, problems, S, first);
    const std::vector<RadFltWork> flt = flt_works<RadFltWork>(c, problems, S, true, first);
    std::vector<RadI8Prob> probs(n);
    for (int i = 0; i < n; ++i)
        probs[i] = RadI8Prob{c->sets[problems[i].query_set].d, c->sets[problems[i].train_set].d, qoff[i]};
    const size_t wb = vec_bytes(S8.works), sb = vec_bytes(S8.seg);
    HIPCHK(c, c->rad_counts.ensure(sizeof(int) * (nqs + 1)));
    HIPCHK(c, c->rad_cursor.ensure(sizeof(int) * (nqs + 1)));
    HIPCHK(c, c->rad_offsets.ensure(sizeof(long long) * (nqs + 1)));
    HIPCHK(c, c->rad_meta.ensure(sizeof(long long) * (2 + 2 * (size_t)radius_scan_blocks(nqs))));
    HIPCHK(c, c->rad_probs.ensure(sizeof(RadI8Prob) * std::max(n, 1)));
    if (!ham.empty()) HIPCHK(c, c->rad_ham_works.ensure(sizeof(RadHamWork) * ham.size()));
    if (!flt.empty()) HIPCHK(c, c->rad_flt_works.ensure(sizeof(RadFltWork) * flt.size()));
    if (wb) HIPCHK(c, c->rad_i8_works.ensure(wb + sb));
    // the device tables are rewritten in stream order (after the previous call's kernels)
    StageWriter up(c->stage, vec_bytes(probs) + vec_bytes(ham) + vec_bytes(flt) + wb + sb, c->stream);
    up.put(c->rad_probs, probs);
    up.put(c->rad_ham_works, ham);
    up.put(c->rad_flt_works, flt);
    if (wb) up.put(c->rad_i8_works.p, S8.works.data(), wb, S8.seg.data(), sb);
    HIPCHK(c, up.done());
    HIPCHK(c, hipMemsetAsync(c->rad_counts.p, 0, sizeof(int) * (nqs + 1), c->stream));
    c->rad.problems.assign(problems, problems + n);
    c->rad.r = r;
    c->rad.gen = c->sets_gen;
    c->rad.n_queries = nqs;
    c->rad.n_ham = (int)ham.size();
    c->rad.n_flt = (int)flt.size();
    c->rad.n_i8_works = (int)S8.works.size();
    c->rad.n_i8_blocks = S8.works.empty() ? 0 : S8.n_blocks;
    c->cur = c->stream;
    ev_mark(c, "begin");
    radius_launch(c, radius_args(c), false);
    HIPCHK(c, hipGetLastError());
    ev_mark(c, "radius_count");
    launch_radius_scan(c->rad_counts.as<int>(), c->rad_cursor.as<int>(), c->rad_offsets.as<long long>(),
                       reinterpret_cast<long long*>(offsets_dev), nqs, c->rad_meta.as<long long>(), c->cur);
    HIPCHK(c, hipGetLastError());
    ev_mark(c, "radius_scan");
    long long meta[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(meta, c->rad_meta.p, sizeof meta, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // the one scalar the caller sizes its buffers by
    ev_collect(c);
    c->rad.total = meta[0];
    c->rad.longest = meta[1];
    c->rad.filled = false;
    c->rad.valid = true;
    *total = meta[0];
    return MIM_OK;
}

static mim_status radius_fill_locked(mim_ctx* c, int32_t* idx_dev, float* dist_dev, int64_t cap) {
    invalidate_batch(c);
    if (!c->rad.valid) return fail(c, MIM_EINVAL, "radius_fill: no mim_radius_count call to fill");
    if (c->rad.gen != c->sets_gen)
        return fail(c, MIM_EINVAL, "radius_fill: sets were cleared or truncated since the mim_radius_count call");
    if (cap < c->rad.total)
        return fail(c, MIM_ERANGE, "radius_fill: %lld matches, room for %lld", c->rad.total, (long long)cap);
    if (c->rad.total == 0) return MIM_OK;
    if (!idx_dev || !dist_dev) return fail(c, MIM_EINVAL, "radius_fill: null output");
    if (c->rad_keys.ensure(sizeof(unsigned long long) * c->rad.total) != hipSuccess)
        return fail(c, MIM_ENOMEM, "radius_fill: key buffer of %lld entries", c->rad.total);
    if (c->rad.longest > kRadSortCap && c->rad_scratch.ensure(sizeof(unsigned long long) * c->rad.total) != hipSuccess)
        return fail(c, MIM_ENOMEM, "radius_fill: merge buffer of %lld entries", c->rad.total);
    c->cur = c->stream;
    if (c->rad.filled) HIPCHK(c, hipMemsetAsync(c->rad_cursor.p, 0, sizeof(int) * c->rad.n_queries, c->stream));
    c->rad.filled = true;
    ev_mark(c, "begin");
    radius_launch(c, radius_args(c), true);
    HIPCHK(c, hipGetLastError());
    ev_mark(c, "radius_fill");
    launch_radius_sort(c->rad_offsets.as<long long>(), c->rad.n_queries, c->rad_keys.as<unsigned long long>(),
                       c->rad_scratch.as<unsigned long long>(), idx_dev, dist_dev, c->cur);
    HIPCHK(c, hipGetLastError());
    ev_mark(c, "radius_sort");
    return MIM_OK;
}

// body of the radius host-buffer entries: the count and its offsets, then (idx != null) the fill.  The 128-D
// form flushes its sets' prep, whose flags block comes from the arena after their storage.
static mim_status radius_host_body(mim_ctx* c, const mim_problem& pr, int nq, float r, int64_t* offsets, int32_t* idx,
                                   float* dist, int64_t cap) {
    int64_t total = 0;
    mim_status s = radius_count_locked(c, &pr, 1, r, nullptr, &total);
    if (s != MIM_OK) return s;
    HIPCHK(c, hipMemcpyAsync(offsets, c->rad_offsets.p, sizeof(int64_t) * (nq + 1), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (!idx) return MIM_OK;  // offsets only
    if (total > cap) return fail(c, MIM_ERANGE, "radius: %lld matches, room for %lld", (long long)total, (long long)cap);
    if (total == 0) return MIM_OK;
    HIPCHK(c, c->knn_idx.ensure(sizeof(int32_t) * total));
    HIPCHK(c, c->knn_dist.ensure(sizeof(float) * total));
    s = radius_fill_locked(c, c->knn_idx.as<int32_t>(), c->knn_dist.as<float>(), total);
    if (s != MIM_OK) return s;
    HIPCHK(c, hipMemcpyAsync(idx, c->knn_idx.p, sizeof(int32_t) * total, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(dist, c->knn_dist.p, sizeof(float) * total, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MIM_OK;
}

extern "C" {

mim_status mim_radius_count(mim_ctx* c, const mim_problem* problems, int32_t n, float max_distance,
                            int64_t* offsets_dev, int64_t* total) {
    if (!c) return MIM_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    return radius_count_locked(c, problems, n, max_distance, offsets_dev, total);
}

mim_status mim_radius_fill_dev(mim_ctx* c, int32_t* idx_dev, float* dist_dev, int64_t cap) {
    if (!c) return MIM_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    return radius_fill_locked(c, idx_dev, dist_dev, cap);
}

mim_status mim_radius_l2(mim_ctx* c, const float* q, int32_t nq, const float* t, int32_t nt, int32_t dim,
                         float max_distance, int64_t* offsets, int32_t* idx, float* dist, int64_t cap) {
    if (!c) return MIM_EINVAL;
    if (check_host_pair(c, "radius_l2", q, nq, t, nt, offsets && (!idx || dist) && cap >= 0) != MIM_OK)
        return MIM_EINVAL;
    if (dim < 1 || dim > kFltMaxDim) return fail(c, MIM_EINVAL, "radius_l2: dim must be 1..%d (got %d)", kFltMaxDim, dim);
    if (!radius_arg_ok(max_distance))
        return fail(c, MIM_EINVAL, "radius_l2: max_distance must be above FLT_EPSILON (got %g)", (double)max_distance);
    offsets[0] = 0;
    if (nq == 0) return MIM_OK;  // radiusMatch on an empty query returns no rows
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<float> kp0((size_t)std::max(std::max(nq, nt), 1) * 2, 0.f);
    auto make = [&](const float* rows, int n, int32_t* id) {
        // dim 128: the 128-D path, so that integer rows take the MFMA kernel (the same bits either way)
        if (dim == kDim) return set_create_locked(c, rows ? rows : kp0.data(), kp0.data(), n, dim, 0, id);
        return set_create_f32_locked(c, rows, (int64_t)4 * dim, kp0.data(), n, dim, 0, id);
    };
    return with_private_sets(
        c, [&](int32_t* id) { return make(q, nq, id); }, [&](int32_t* id) { return make(t, nt, id); },
        [&](const mim_problem& pr) { return radius_host_body(c, pr, nq, max_distance, offsets, idx, dist, cap); });
}

mim_status mim_radius_hamming(mim_ctx* c, const uint8_t* q, int32_t nq, const uint8_t* t, int32_t nt, int32_t width,
                              float max_distance, int64_t* offsets, int32_t* idx, float* dist, int64_t cap) {
    if (!c) return MIM_EINVAL;
    if (check_host_pair(c, "radius_hamming", q, nq, t, nt, offsets && (!idx || dist) && cap >= 0) != MIM_OK)
        return MIM_EINVAL;
    if (width < 1 || width > 64) return fail(c, MIM_EINVAL, "radius_hamming: width must be 1..64 bytes (got %d)", width);
    if (!radius_arg_ok(max_distance))
        return fail(c, MIM_EINVAL, "radius_hamming: max_distance must be above FLT_EPSILON (got %g)", (double)max_distance);
    offsets[0] = 0;
    if (nq == 0) return MIM_OK;  // radiusMatch on an empty query returns no rows
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<float> kp0((size_t)std::max(std::max(nq, nt), 1) * 2, 0.f);
    return with_private_sets(
        c, [&](int32_t* id) { return set_create_bin_locked(c, q, width, kp0.data(), nq, width, 0, id); },
        [&](int32_t* id) { return set_create_bin_locked(c, t, width, kp0.data(), nt, width, 0, id); },
        [&](const mim_problem& pr) { return radius_host_body(c, pr, nq, max_distance, offsets, idx, dist, cap); });
}

void mim_default_box_params(mim_box_params* p) {
    const mim::BoxParams d;
    p->cluster_distance = d.cluster_distance;
    p->min_points_per_cluster = d.min_points_per_cluster;
    p->box_merge_distance = d.box_merge_distance;
    p->min_box_area = d.min_box_area;
    p->dynamic_margin = d.dynamic_margin;
}

mim_status mim_detect_boxes(const float* pts_xy, int32_t n, const mim_box_params* bp, mim_rect* boxes, int32_t cap,
                            int32_t* n_boxes) {
    if (n < 0 || (n > 0 && !pts_xy) || !n_boxes || cap < 0 || (cap > 0 && !boxes)) return MIM_EINVAL;
    mim::BoxParams p;
    if (bp) {
        p.cluster_distance = bp->cluster_distance;
        p.min_points_per_cluster = bp->min_points_per_cluster;
        p.box_merge_distance = bp->box_merge_distance;
        p.min_box_area = bp->min_box_area;
        p.dynamic_margin = bp->dynamic_margin;
    }
    try {
        std::vector<mim::Point2f> pts(n);
        for (int32_t i = 0; i < n; ++i) pts[i] = {pts_xy[2 * i], pts_xy[2 * i + 1]};
        mim::Detections dets;
        mim::boxes_for_model(pts, "", dets, p);
        *n_boxes = (int32_t)dets.size();
        for (int32_t i = 0; i < std::min(cap, *n_boxes); ++i)
            boxes[i] = mim_rect{dets[i].first.x, dets[i].first.y, dets[i].first.width, dets[i].first.height};
    } catch (const std::bad_alloc&) {
        return MIM_ENOMEM;
    }
    return MIM_OK;
}

mim_status mim_sift_detect_compute(mim_ctx* c, const uint8_t* gray, int32_t rows, int32_t cols, int64_t step,
                                   const uint8_t* mask, int64_t mask_step, int32_t max_kp, mim_keypoint* kps,
                                   float* desc, int32_t* n_kp) {
    if (!c) return MIM_EINVAL;
    if (!gray || !n_kp || rows <= 0 || cols <= 0 || step < cols || max_kp < 0 || (max_kp > 0 && (!kps || !desc)) ||
        (mask && mask_step < cols))
        return fail(c, MIM_EINVAL, "sift_detect_compute: bad arguments");
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->sift) c->sift = mim::sift_ws_create();
    int n = 0;
    c->sift_last.clear();
    const int r = mim::sift_detect_compute(c->sift, c->stream, gray, rows, cols, step, mask, mask_step, max_kp, kps,
                                           desc, &n, c->err);
    if (r == 0) c->sift_last.assign(1, c->sift);
    *n_kp = n;
    if (r == -1) return MIM_EDEVICE;
    if (r == -2) return MIM_ERANGE;
    if (r == -4) return MIM_ELIMIT;
    return MIM_OK;
}

mim_status mim_sift_detect_compute_scales(mim_ctx* c, const uint8_t* gray, int32_t rows, int32_t cols, int64_t step,
                                          int32_t n_scales, const float* scales, int32_t max_kp, mim_keypoint* kps,
                                          float* desc, int32_t* n_kp) {
    if (!c) return MIM_EINVAL;
    if (!gray || !n_kp || !scales || n_scales <= 0 || n_scales > 64 || rows <= 0 || cols <= 0 || step < cols ||
        max_kp < 0 || (max_kp > 0 && (!kps || !desc)))
        return fail(c, MIM_EINVAL, "sift_detect_compute_scales: bad arguments");
    for (int i = 0; i < n_scales; ++i)
        if (!(scales[i] > 0)) return fail(c, MIM_EINVAL, "sift_detect_compute_scales: scale %d is not > 0", i);
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<int> n(n_scales, 0);
    c->sift_last.clear();
    const int r = mim::sift_detect_compute_scales(c->sift_scales, c->stream, gray, rows, cols, step, n_scales, scales,
                                                  max_kp, kps, desc, n.data(), c->err);
    if (r == 0 || r == -2) c->sift_last.assign(c->sift_scales.begin(), c->sift_scales.begin() + n_scales);
    for (int i = 0; i < n_scales; ++i) n_kp[i] = n[i];
    if (r == -1) return MIM_EDEVICE;
    if (r == -2) return MIM_ERANGE;
    if (r == -3) return MIM_EINVAL;
    if (r == -4) return MIM_ELIMIT;
    return MIM_OK;
}

mim_status mim_sift_debug_pyramid(mim_ctx* c, int32_t image_index, int32_t* n_oct, int32_t* orows, int32_t* ocols,
                                  float* planes, int64_t cap, int64_t* need, int32_t* counters) {
    if (!c) return MIM_EINVAL;
    if (!n_oct || !orows || !ocols || !need || !counters || cap < 0)
        return fail(c, MIM_EINVAL, "sift_debug_pyramid: bad arguments");
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->sift_last.empty()) return fail(c, MIM_EINVAL, "sift_debug_pyramid: no SIFT call completed on this ctx");
    if (image_index < 0 || image_index >= (int32_t)c->sift_last.size())
        return fail(c, MIM_EINVAL, "sift_debug_pyramid: image %d, the last SIFT call had %d", image_index,
                    (int)c->sift_last.size());
    HIPCHK(c, hipSetDevice(c->device));
    long long nd = 0;
    const int r = mim::sift_debug_pyramid(c->sift_last[image_index], c->stream, n_oct, orows, ocols, planes, cap, &nd,
                                          counters, c->err);
    *need = nd;
    if (r == -1) return MIM_EDEVICE;
    if (r == -3) return MIM_EINVAL;
    return MIM_OK;
}

// mim_sift_scales_sets' registration of the scales as sets (lock held); total = keypoints of all scales
static mim_status scales_sets_register(mim_ctx* c, const mim::SiftDevOut* out, int n_scales, int32_t* set_ids,
                                       int32_t* n_kp, long long& total) {
    std::vector<float*> ddesc(n_scales, nullptr);
    std::vector<float2*> dkp(n_scales, nullptr);
    for (int i = 0; i < n_scales; ++i) {
        const int n = out[i].n;
        n_kp[i] = n;
        total += n;
        SetRec rec{};
        rec.mark = c->arena.pos();
        rec.d.n = n;
        rec.d.n_tiles = (n + 63) / 64;
        const size_t tiles = (size_t)std::max(rec.d.n_tiles, 1);
        void *frag, *norm, *df = nullptr, *dk = nullptr;
        HIPCHK(c, c->arena.alloc(tiles * kTileBytes, &frag));
        HIPCHK(c, c->arena.alloc(tiles * kNormWords * sizeof(int), &norm));
        if (n > 0) {
            HIPCHK(c, c->arena.alloc((size_t)n * kDim * sizeof(float), &df));
            HIPCHK(c, c->arena.alloc((size_t)n * 2 * sizeof(float), &dk));
        }
        ddesc[i] = (float*)df;
        dkp[i] = (float2*)dk;
        rec.d.frag = (const int8_t*)frag;
        rec.d.norm = (const int*)norm;
        rec.d.f32 = (const float*)df;
        rec.d.kp = (const float2*)dk;
        rec.d.flags = nullptr;
        set_ids[i] = (int32_t)c->sets.size();
        c->pend.push_back(PrepJob{(const float*)df, (int8_t*)frag, (int*)norm, nullptr, n, 0});
        c->pend_set.push_back(set_ids[i]);
        c->sets.push_back(rec);
    }
    // every scale's rows and KeyPoint::pt (the first two floats of each mim_keypoint) in one launch
    if (mim::sift_copy_sets(out, n_scales, ddesc.data(), dkp.data(), c->stream) != 0)
        return fail(c, MIM_EDEVICE, "sift_scales_sets: set copy launch failed");
    return MIM_OK;
}

// mim_sift_scales_sets and mim_sift_scales_sets_image: the scene (channels 1 or 3, checked by the
// callers) resized and described at every scale on the device, the scales registered as sets
static mim_status sift_scales_sets_impl(mim_ctx* c, const uint8_t* img, int32_t rows, int32_t cols, int64_t step,
                                        int32_t channels, int32_t n_scales, const float* scales, int32_t* set_ids,
                                        int32_t* n_kp, int32_t max_kp, mim_keypoint* kps) {
    if (!img || !set_ids || !n_kp || !scales || n_scales <= 0 || n_scales > 8 || rows <= 0 || cols <= 0 ||
        step < (int64_t)cols * channels || max_kp < 0 || (max_kp > 0 && !kps))
        return fail(c, MIM_EINVAL, "sift_scales_sets: bad arguments");
    for (int i = 0; i < n_scales; ++i)
        if (!(scales[i] > 0)) return fail(c, MIM_EINVAL, "sift_scales_sets: scale %d is not > 0", i);
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<mim::SiftDevOut> out(n_scales);
    c->sift_last.clear();
    const int r = mim::sift_scales_device(c->sift_scales, c->stream, img, rows, cols, step, channels, n_scales, scales,
                                          out.data(), c->err);
    if (r == 0) c->sift_last.assign(c->sift_scales.begin(), c->sift_scales.begin() + n_scales);
    if (r == -1) return MIM_EDEVICE;
    if (r == -3) return MIM_EINVAL;
    if (r == -4) return MIM_ELIMIT;
    if (r != 0) return MIM_ERANGE;
    // each scale's rows and keypoint positions copied on the device into the set arena (the SIFT
    // workspaces are overwritten by the next SIFT call), the set registered as by mim_set_create; a
    // failure part-way (arena allocation, copy) drops the scales registered so far, so the ctx is left
    // as before the call
    const int n0 = (int)c->sets.size();
    const Arena::Mark mark0 = c->arena.pos();
    long long total = 0;
    const mim_status rs = scales_sets_register(c, out.data(), n_scales, set_ids, n_kp, total);
    if (rs != MIM_OK) {
        if ((int)c->sets.size() > n0)
            sets_truncate_locked(c, n0);
        else
            c->arena.seek(mark0);
        return rs;
    }
    if (kps && max_kp > 0) {  // the keypoints on the host too, concatenated in scale order
        long long used = 0;
        for (int i = 0; i < n_scales && used < max_kp; ++i) {
            const long long m = std::min<long long>(out[i].n, max_kp - used);
            if (m > 0)
                HIPCHK(c, hipMemcpyAsync(kps + used, out[i].kp, sizeof(mim_keypoint) * m, hipMemcpyDeviceToHost, c->stream));
            used += m;
        }
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    if (kps && total > max_kp) return fail(c, MIM_ERANGE, "sift_scales_sets: %lld keypoints, buffer holds %d", total, max_kp);
    return MIM_OK;
}

mim_status mim_sift_scales_sets(mim_ctx* c, const uint8_t* gray, int32_t rows, int32_t cols, int64_t step,
                                int32_t n_scales, const float* scales, int32_t* set_ids, int32_t* n_kp, int32_t max_kp,
                                mim_keypoint* kps) {
    if (!c) return MIM_EINVAL;
    return sift_scales_sets_impl(c, gray, rows, cols, step, 1, n_scales, scales, set_ids, n_kp, max_kp, kps);
}

mim_status mim_sift_scales_sets_image(mim_ctx* c, const mim_image* scene, int32_t n_scales, const float* scales,
                                      int32_t* set_ids, int32_t* n_kp, int32_t max_kp, mim_keypoint* kps) {
    if (!c) return MIM_EINVAL;
    if (!scene) return fail(c, MIM_EINVAL, "sift_scales_sets_image: null image");
    if (scene->channels != 1 && scene->channels != 3)
        return fail(c, MIM_EINVAL, "sift_scales_sets_image: %d channels (1: CV_8UC1, 3: CV_8UC3 BGR)", scene->channels);
    if (scene->cols > 0 && scene->step < (int64_t)scene->cols * scene->channels)
        return fail(c, MIM_EINVAL, "sift_scales_sets_image: step %lld < cols * channels = %lld", (long long)scene->step,
                    (long long)scene->cols * scene->channels);
    return sift_scales_sets_impl(c, scene->data, scene->rows, scene->cols, scene->step, scene->channels, n_scales,
                                 scales, set_ids, n_kp, max_kp, kps);
}

mim_status mim_cvt_bgr2gray_u8(mim_ctx* c, const uint8_t* bgr, int32_t rows, int32_t cols, int64_t step,
                               uint8_t* gray_out) {
    if (!c) return MIM_EINVAL;
    if (!bgr || !gray_out || rows <= 0 || cols <= 0)
        return fail(c, MIM_EINVAL, "cvt_bgr2gray_u8: bad arguments");
    if (step < (int64_t)cols * 3)
        return fail(c, MIM_EINVAL, "cvt_bgr2gray_u8: step %lld < 3 * cols = %lld", (long long)step, (long long)cols * 3);
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->sift) c->sift = mim::sift_ws_create();
    const int r = mim::sift_bgr2gray_u8(c->sift, c->stream, bgr, rows, cols, step, gray_out, c->err);
    if (r == -3) return MIM_EINVAL;
    if (r == -4) return MIM_ELIMIT;
    if (r != 0) return MIM_EDEVICE;
    return MIM_OK;
}

mim_status mim_resize_linear_u8(mim_ctx* c, const uint8_t* src, int32_t rows, int32_t cols, int64_t step,
                                uint8_t* dst, int32_t drows, int32_t dcols, double fx, double fy) {
    if (!c) return MIM_EINVAL;
    if (!src || !dst || rows <= 0 || cols <= 0 || step < cols || drows <= 0 || dcols <= 0 || fx < 0 || fy < 0 ||
        (fx > 0) != (fy > 0))
        return fail(c, MIM_EINVAL, "resize_linear_u8: bad arguments");
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->sift) c->sift = mim::sift_ws_create();
    if (mim::sift_resize_u8(c->sift, c->stream, src, rows, cols, step, dst, drows, dcols, fx, fy, c->err) != 0)
        return MIM_EDEVICE;
    return MIM_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// RANSAC: RNG stream, workspace, batch entry points
// ---------------------------------------------------------------------------------------------
static void mark_cb(void* vc, const char* name, hipStream_t st) {
    mim_ctx* c = (mim_ctx*)vc;
    const hipStream_t keep = c->cur;
    c->cur = st;
    ev_mark(c, name);
    c->cur = keep;
}

// cv::RNG((uint64)-1).next() stream (core/include/opencv2/core/operations.hpp).  Every
// findHomography call re-seeds, so one stream serves all problems of a ctx.  Generated on the
// device: the MWC state s' = (u32)s * a + (s >> 32) (a = 4164903690) is, from the second state on,
// the Lehmer sequence s_{n+1} = a * s_n mod (a * 2^32 - 1), so each 4096-draw segment starts from
// a * ... jump-ahead computed here in 128-bit arithmetic and the device expands the segments.
constexpr long long kStreamMin = 1LL << 23, kStreamCap = 1LL << 30;  // draws (the cap: 4 GiB)
constexpr int kStreamSeg = 4096;

static inline unsigned long long mwc_next(unsigned long long s) {
    return (unsigned long long)(uint32_t)s * 4164903690ULL + (s >> 32);
}
static inline unsigned long long mulmod(unsigned long long x, unsigned long long y, unsigned long long m) {
    return (unsigned long long)(((unsigned __int128)x * y) % m);
}

static mim_status ensure_stream(mim_ctx* c, long long need) {
    if (c->rws.stream_len >= need) return MIM_OK;
    long long len = std::max(need, kStreamMin);
    if (c->stream_draws && c->rws.stream_len == 0) len = c->stream_draws;  // test knob: first stream only
    if (len > kStreamCap) return fail(c, MIM_ERANGE, "RNG stream of %lld draws exceeds the 2^30 cap", len);
    len = (len + kStreamSeg - 1) / kStreamSeg * kStreamSeg;
    const int n_seg = (int)(len / kStreamSeg);
    const unsigned long long a = 4164903690ULL, m = a * 4294967296ULL - 1;
    std::vector<unsigned long long> seg((size_t)n_seg);
    const unsigned long long s0 = mwc_next(~0ULL), s1 = mwc_next(s0);
    // a^(kStreamSeg) and a^(kStreamSeg - 1) mod m
    unsigned long long J = 1, Jm1 = 1;
    for (int k = 0; k < kStreamSeg; ++k) {
        Jm1 = J;
        J = mulmod(J, a, m);
    }
    seg[0] = s0;
    if (n_seg > 1) seg[1] = mulmod(Jm1, s1, m);  // s_{4096} = a^4095 s_1
    for (int i = 2; i < n_seg; ++i) seg[(size_t)i] = mulmod(seg[(size_t)i - 1], J, m);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // 64 zero draws of padding: the draw prefetches of resolve_at may read up to 7 past the end
    HIPCHK(c, c->rws.stream.ensure(sizeof(uint32_t) * (len + 64)));
    DevBuf segs;
    HIPCHK(c, segs.ensure(sizeof(unsigned long long) * n_seg));
    HIPCHK(c, hipMemcpy(segs.p, seg.data(), sizeof(unsigned long long) * n_seg, hipMemcpyHostToDevice));
    launch_rng_stream(segs.as<unsigned long long>(), c->rws.stream.as<uint32_t>(), len, kStreamSeg, n_seg,
                      c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemsetAsync((uint32_t*)c->rws.stream.p + len, 0, sizeof(uint32_t) * 64, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    segs.release();
    c->rws.stream_len = len;
    return MIM_OK;
}

// Longer stream after a batch ran out (status MIM_STREAM_SHORT): x8, up to the cap.
static mim_status grow_stream(mim_ctx* c) {
    if (c->rws.stream_len >= kStreamCap)
        return fail(c, MIM_ERANGE, "RANSAC consumed the whole RNG stream (%lld draws, the cap)", c->rws.stream_len);
    return ensure_stream(c, std::min(kStreamCap, c->rws.stream_len * 8));
}

// Buffers and parameters of one RANSAC batch over n problems (allocation only: call before any
// launch of the batch, a reallocation synchronises the device).
static mim_status ransac_prepare(mim_ctx* c, int n, const mim_params* prm, RansacBufs& b, RansacParams& rp,
                                 long long& flag_per) {
    const int max_iters = std::max(prm->max_iters, 1);
    mim_status s = ensure_stream(c, (long long)max_iters * 64 + 40000 * 4);
    if (s != MIM_OK) return s;
    long long it_total = 0, good_total = 0;
    int q_max = 0;  // the largest query set bounds every problem's good-match count
    for (int i = 0; i < n; ++i) {
        q_max = std::max(q_max, c->h_probs[i].q.n);
        it_total = std::max(it_total, c->h_probs[i].it_off + max_iters);
        good_total = std::max(good_total, c->h_probs[i].good_off + std::max(c->h_probs[i].q.n, 1));
    }
    HIPCHK(c, c->rws.state.ensure(sizeof(RansacState) * std::max(n, 1)));
    HIPCHK(c, c->rws.samples.ensure(sizeof(int4) * it_total));
    HIPCHK(c, c->rws.hyp.ensure(sizeof(float) * 8 * it_total));
    HIPCHK(c, c->rws.counts.ensure(sizeof(int) * it_total));
    HIPCHK(c, c->rws.bounds.ensure(sizeof(int2) * it_total));
    // attempt-outcome windows: largest chunk x 28 draws per problem, 64-byte granular per problem
    const long long chunk_max = std::min<long long>(max_iters, 1 << 18);
    flag_per = (chunk_max * 28 + 4096 + 63) & ~63LL;
    const long long flag_cap = (long long)std::max(n, 1) * flag_per;
    HIPCHK(c, c->rws.flags.ensure((size_t)flag_cap));
    HIPCHK(c, c->rws.irr_bits.ensure((size_t)flag_cap / 8));
    const int irr_blocks = (int)((flag_per + kIrrBlock - 1) / kIrrBlock);
    HIPCHK(c, c->rws.irr.ensure(sizeof(int) * (size_t)std::max(n, 1) * irr_blocks * kIrrCap));
    HIPCHK(c, c->rws.irr_cnt.ensure(sizeof(int) * (size_t)std::max(n, 1) * irr_blocks));
    // sampler classes: one record per problem, one table slot per possible good-match count
    HIPCHK(c, c->rws.cls.ensure(sizeof(SamplerClass) * (size_t)std::max(n, 1)));
    HIPCHK(c, c->rws.cls_tab.ensure(sizeof(SamplerClassSlot) * ((size_t)q_max + 1)));
    HIPCHK(c, c->rws.pass_bits.ensure((size_t)flag_cap / 8));
    // deferred-attempt lists of the check rounds: a chain holds at most ~window / 4 attempts
    const int def_rounds = (int)((flag_per / 4 + 2 * kRansacDefRoundAttempts) / kRansacDefRoundAttempts);
    HIPCHK(c, c->rws.defer.ensure(sizeof(int2) * kRansacDefSlots * (size_t)std::max(n, 1) * def_rounds));
    HIPCHK(c, c->rws.defer_n.ensure(sizeof(int) * (size_t)std::max(n, 1) * def_rounds));
    HIPCHK(c, c->rws.chains.ensure(ransac_chain_bytes() * (size_t)std::max(n, 1)));
    HIPCHK(c, c->rws.best_h.ensure(sizeof(double) * 9 * std::max(n, 1)));
    // two candidate lists per problem: chunk 1's (kept when its exact pass is deferred) and chunk 2's
    const size_t cap = (size_t)std::max(n, 1) * 2 * kCandPerProblem;
    HIPCHK(c, c->rws.cand.ensure(sizeof(int) * cap));
    HIPCHK(c, c->rws.ncand.ensure(sizeof(int) * 2 * std::max(n, 1)));
    HIPCHK(c, c->rws.cex.ensure(sizeof(int) * cap));
    HIPCHK(c, c->rws.cH.ensure(sizeof(double) * 9 * cap));
    HIPCHK(c, c->rws.decided.ensure(sizeof(int) * cap));
    HIPCHK(c, c->rws.inl.ensure(sizeof(float4) * good_total));
    HIPCHK(c, c->rws.tiles.ensure(sizeof(uint4) * 128 * ((good_total + 31) / 32)));
    HIPCHK(c, c->rws.tbox.ensure(sizeof(float4) * ((good_total + 31) / 32)));
    HIPCHK(c, c->rws.perm.ensure(sizeof(int) * 2 * good_total));
    // the survivor list of the capped bound holds a whole chunk per problem
    HIPCHK(c, c->rws.surv.ensure(sizeof(int) * it_total));
    HIPCHK(c, c->rws.nsurv.ensure(sizeof(int) * std::max(n, 1)));
    HIPCHK(c, c->rws.strip.ensure(sizeof(int4) * std::max(n, 1)));
    HIPCHK(c, c->rws.err.ensure(sizeof(int) * 4));
    HIPCHK(c, c->results.ensure(sizeof(mim_result) * std::max(n, 1)));
    HIPCHK(c, c->masks.ensure(good_total));
    HIPCHK(c, hipMemsetAsync(c->rws.err.p, 0, sizeof(int) * 4, c->stream));
    b = RansacBufs{};
    b.state = c->rws.state.as<RansacState>();
    b.samples = c->rws.samples.as<int4>();
    b.hyp = c->rws.hyp.as<float>();
    b.counts = c->rws.counts.as<int>();
    b.bounds = c->rws.bounds.as<int2>();
    b.flags = c->rws.flags.as<uint8_t>();
    b.irr_bits = c->rws.irr_bits.as<uint8_t>();
    b.best_h = c->rws.best_h.as<double>();
    b.cand = c->rws.cand.as<int>();
    b.ncand = c->rws.ncand.as<int>();
    b.cex = c->rws.cex.as<int>();
    b.cH = c->rws.cH.as<double>();
    b.decided = c->rws.decided.as<int>();
    b.flag_cap = flag_cap;
    b.irr = c->rws.irr.as<int>();
    b.irr_cnt = c->rws.irr_cnt.as<int>();
    b.pass_bits = c->rws.pass_bits.as<uint32_t>();
    b.defer = c->rws.defer.as<int2>();
    b.defer_n = c->rws.defer_n.as<int>();
    // MIM_CHECK_DEFER=0: every deferred attempt decided inside the check kernel (test knob)
    const char* cde = getenv("MIM_CHECK_DEFER");
    b.def_rounds = (cde && cde[0] == '0') ? 0 : def_rounds;
    b.irr_blocks = irr_blocks;
    b.cls = c->rws.cls.as<SamplerClass>();
    b.cls_tab = c->rws.cls_tab.as<SamplerClassSlot>();
    b.cls_tab_n = q_max + 1;
    b.chains = c->rws.chains.p;
    b.stream = c->rws.stream.as<uint32_t>();
    b.stream_len = c->rws.stream_len;
    b.inl = c->rws.inl.as<float4>();
    b.tiles = c->rws.tiles.as<uint4>();
    b.tbox = c->rws.tbox.as<float4>();
    b.perm = c->rws.perm.as<int>();
    b.surv = c->rws.surv.as<int>();
    b.nsurv = c->rws.nsurv.as<int>();
    b.strip = c->rws.strip.as<int4>();
    b.err = c->rws.err.as<int>();
    if (c->samp_on < 0) {
        const char* e = getenv("MIM_SAMPLER_STREAM");
        c->samp_on = (e && e[0] == '0') ? 0 : 1;
    }
    if (c->samp_on && !c->samp) {
        HIPCHK(c, hipStreamCreateWithFlags(&c->samp, hipStreamNonBlocking));
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_samp_fork, hipEventDisableTiming));
        for (auto& e : c->ev_samp) HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    b.s2 = c->samp_on ? c->samp : nullptr;
    b.ev_fork = c->ev_samp_fork;
    b.ev_samp[0] = c->ev_samp[0];
    b.ev_samp[1] = c->ev_samp[1];
    rp = RansacParams{};
    rp.thresh = prm->ransac_thresh > 0 ? prm->ransac_thresh : 3.0;  // findHomography: thresh <= 0 -> 3
    rp.conf = prm->confidence;
    rp.max_iters = max_iters;
    rp.ratio = prm->ratio;
    rp.min_good = prm->min_good;
    rp.min_inliers = prm->min_inliers;
    rp.det_lo = prm->det_lo;
    rp.det_hi = prm->det_hi;
    rp.cand_cap = c->cand_cap;
    rp.rep_cap = c->rep_cap;
    return MIM_OK;
}

// RANSAC kernels for problems [p0, p0 + np) on c->cur: per-problem buffers are offset to the range
// (problem-indexed ones by p0, the iteration/point-indexed ones use the global it_off/good_off).
static mim_status ransac_enqueue_range(mim_ctx* c, int p0, int np, const RansacBufs& b, const RansacParams& rp,
                                       long long flag_per, int raw) {
    RansacBufs g = b;
    g.state += p0;
    g.flags += (long long)p0 * flag_per;
    g.irr_bits += (long long)p0 * flag_per / 8;
    g.flag_cap = (long long)np * flag_per;
    g.irr += (long long)p0 * b.irr_blocks * kIrrCap;
    g.irr_cnt += (long long)p0 * b.irr_blocks;
    g.cls += p0;
    g.pass_bits += (long long)p0 * flag_per / 32;
    g.defer += (long long)p0 * b.def_rounds * kRansacDefSlots;
    g.defer_n += (long long)p0 * b.def_rounds;
    g.chains = static_cast<char*>(b.chains) + (size_t)p0 * ransac_chain_bytes();
    g.best_h += 9LL * p0;
    g.cand += (long long)p0 * 2 * kCandPerProblem;
    g.ncand += 2 * p0;
    g.cex += (long long)p0 * 2 * kCandPerProblem;
    g.cH += 9LL * p0 * 2 * kCandPerProblem;
    g.decided += (long long)p0 * 2 * kCandPerProblem;
    g.nsurv += p0;
    g.strip += p0;
    ransac_enqueue(rp, np, c->probs.as<ProbDev>() + p0, c->pts.as<float4>(), c->n_good.as<int>() + p0, g,
                   c->masks.as<uint8_t>(), c->results.as<mim_result>() + p0, raw, c->cur, mark_cb, c, c->exact_all);
    HIPCHK(c, hipGetLastError());
    return MIM_OK;
}

static mim_status ransac_locked(mim_ctx* c, int n, const mim_params* prm, int raw) {
    RansacBufs b;
    RansacParams rp;
    long long flag_per = 0;
    mim_status s = ransac_prepare(c, n, prm, b, rp, flag_per);
    if (s != MIM_OK) return s;
    c->cur = c->stream;
    return ransac_enqueue_range(c, 0, n, b, rp, flag_per, raw);
}

static mim_status check_params(mim_ctx* c, const mim_params* p) {
    if (!p) return fail(c, MIM_EINVAL, "null params");
    if (!(p->confidence > 0 && p->confidence < 1)) return fail(c, MIM_EINVAL, "confidence must be in (0,1)");
    if (p->max_iters > 10000000) return fail(c, MIM_EINVAL, "max_iters too large");
    return MIM_OK;
}

extern "C" {

}  // extern "C"

static mim_status batch_run_locked(mim_ctx* c, const mim_problem* problems, int32_t n, const mim_params* params,
                                   int filter) {
    HIPCHK(c, hipSetDevice(c->device));
    c->last_problems.assign(problems, problems + n);
    c->last_params = *params;
    c->last_filter = filter;
    c->last_gen = c->sets_gen;
    c->last_fh = false;
    if (n == 0) { c->last_n = 0; return MIM_OK; }
    mim_status s = build_tables(c, problems, n, std::max(params->max_iters, 1), filter);
    if (s != MIM_OK) return s;
    RansacBufs b;
    RansacParams rp;
    long long flag_per = 0;
    s = ransac_prepare(c, n, params, b, rp, flag_per);
    if (s != MIM_OK) return s;
    s = knn_ratio_locked(c, n, params->ratio, false, filter);
    if (s != MIM_OK) return s;
    return ransac_enqueue_range(c, 0, n, b, rp, flag_per, 0);
}

// Waits for the last batch; if a problem ran out of RNG draws (status MIM_STREAM_SHORT: OpenCV's
// loop consumed more than the stream holds), grows the stream and re-runs the batch, which is
// possible while its sets are intact.  `res` receives the final records.
static mim_status finish_batch_locked(mim_ctx* c, std::vector<mim_result>& res) {
    for (;;) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        ev_collect(c);
        res.resize((size_t)c->last_n);
        if (c->last_n > 0)
            HIPCHK(c, hipMemcpy(res.data(), c->results.p, sizeof(mim_result) * c->last_n, hipMemcpyDeviceToHost));
        bool short_ = false;
        for (const mim_result& r : res) short_ |= r.status == MIM_STREAM_SHORT;
        if (!short_) return MIM_OK;
        if (c->last_gen != c->sets_gen || c->last_problems.size() != res.size())
            return fail(c, MIM_ERANGE, "a problem ran out of RNG draws (%lld) and its sets were cleared: re-run the "
                                       "batch", c->rws.stream_len);
        mim_status s = grow_stream(c);
        if (s != MIM_OK) return s;
        const std::vector<mim_problem> probs = c->last_problems;
        const mim_params prm = c->last_params;
        s = batch_run_locked(c, probs.data(), (int32_t)probs.size(), &prm, c->last_filter);
        if (s != MIM_OK) return s;
    }
}

extern "C" {

mim_status mim_batch_run(mim_ctx* c, const mim_problem* problems, int32_t n, const mim_params* params) {
    if (!c) return MIM_EINVAL;
    if (n < 0 || (n > 0 && !problems)) return fail(c, MIM_EINVAL, "batch_run: bad arguments");
    mim_status s = check_params(c, params);
    if (s != MIM_OK) return s;
    std::lock_guard<std::mutex> lk(c->mu);
    return batch_run_locked(c, problems, n, params, MIM_FILTER_RATIO);
}

mim_status mim_batch_run_filter(mim_ctx* c, const mim_problem* problems, int32_t n, const mim_params* params,
                                int32_t filter) {
    if (!c) return MIM_EINVAL;
    if (n < 0 || (n > 0 && !problems)) return fail(c, MIM_EINVAL, "batch_run_filter: bad arguments");
    if (filter < MIM_FILTER_RATIO || filter > MIM_FILTER_RATIO_CROSS)
        return fail(c, MIM_EINVAL, "batch_run_filter: filter must be 0 (ratio), 1 (cross) or 2 (ratio and cross), got %d",
                    filter);
    mim_status s = check_params(c, params);
    if (s != MIM_OK) return s;
    std::lock_guard<std::mutex> lk(c->mu);
    return batch_run_locked(c, problems, n, params, filter);
}

mim_status mim_match_cross_sets(mim_ctx* c, int32_t query_set, int32_t train_set, int32_t* idx, float* dist) {
    if (!c) return MIM_EINVAL;
    if (!idx || !dist) return fail(c, MIM_EINVAL, "match_cross_sets: null output");
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    mim_problem pr{query_set, train_set};
    mim_status s = build_tables(c, &pr, 1, 1, MIM_FILTER_CROSS);
    invalidate_batch(c);
    if (s != MIM_OK) return s;
    const int nq = c->h_probs[0].q.n;
    HIPCHK(c, c->knn_idx.ensure(sizeof(int32_t) * std::max(nq, 1)));
    HIPCHK(c, c->knn_dist.ensure(sizeof(float) * std::max(nq, 1)));
    s = knn_ratio_locked(c, 1, 0.f, false, MIM_FILTER_CROSS, c->knn_idx.as<int32_t>(), c->knn_dist.as<float>());
    if (s != MIM_OK) return s;
    if (nq > 0) {
        HIPCHK(c, hipMemcpyAsync(idx, c->knn_idx.p, sizeof(int32_t) * nq, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(dist, c->knn_dist.p, sizeof(float) * nq, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    ev_collect(c);
    return MIM_OK;
}

mim_status mim_batch_results(mim_ctx* c, mim_result* out) {
    if (!c) return MIM_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<mim_result> res;
    mim_status s = finish_batch_locked(c, res);
    if (s != MIM_OK) return s;
    if (out && !res.empty()) memcpy(out, res.data(), sizeof(mim_result) * res.size());
    return MIM_OK;
}

const mim_result* mim_batch_results_dev(mim_ctx* c) { return c ? c->results.as<mim_result>() : nullptr; }

mim_status mim_batch_results_copy(mim_ctx* c, void* dst, int32_t dst_on_device) {
    if (!c || !dst) return MIM_EINVAL;
    if (!dst_on_device) return mim_batch_results(c, (mim_result*)dst);
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    if (c->last_n > 0)
        HIPCHK(c, hipMemcpyAsync(dst, c->results.p, sizeof(mim_result) * c->last_n, hipMemcpyDeviceToDevice, c->stream));
    return MIM_OK;
}

mim_status mim_batch_problem_detail(mim_ctx* c, int32_t i, int32_t* q_idx, int32_t* t_idx, uint8_t* mask) {
    if (!c) return MIM_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (i < 0 || i >= c->last_n) return fail(c, MIM_EINVAL, "problem %d out of range", i);
    HIPCHK(c, hipSetDevice(c->device));
    // the final records first: a batch cut short by the RNG stream is re-run here, as in
    // mim_batch_results, so the mask is never that of an unfinished RANSAC
    std::vector<mim_result> res;
    mim_status fs = finish_batch_locked(c, res);
    if (fs != MIM_OK) return fs;
    int ng = 0;
    HIPCHK(c, hipMemcpy(&ng, c->n_good.as<int>() + i, sizeof(int), hipMemcpyDeviceToHost));
    const long long o = c->h_good_off[i];
    if (ng > 0) {
        if (q_idx) HIPCHK(c, hipMemcpy(q_idx, c->good_q.as<int32_t>() + o, sizeof(int32_t) * ng, hipMemcpyDeviceToHost));
        if (t_idx) HIPCHK(c, hipMemcpy(t_idx, c->good_t.as<int32_t>() + o, sizeof(int32_t) * ng, hipMemcpyDeviceToHost));
        if (mask) HIPCHK(c, hipMemcpy(mask, c->masks.as<uint8_t>() + o, ng, hipMemcpyDeviceToHost));
    }
    return MIM_OK;
}

mim_status mim_batch_inlier_points(mim_ctx* c, const float* scales, float* out_xy, int64_t cap, int64_t* offsets) {
    if (!c) return MIM_EINVAL;
    if (!offsets || cap < 0) return fail(c, MIM_EINVAL, "batch_inlier_points: bad arguments");
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<mim_result> res;
    mim_status fs = finish_batch_locked(c, res);  // waits; re-runs a batch cut short by the RNG stream
    if (fs != MIM_OK) return fs;
    const int n = c->last_n;
    // the gather reads the scene keypoints through the batch's set table: sets cleared or truncated
    // since mim_batch_run have had their storage rewound and possibly reused by newer sets
    if (n > 0 && c->last_fh)
        return fail(c, MIM_EINVAL, "batch_inlier_points: the last call was mim_find_homography, whose record has "
                                   "no scene set to gather from (read its mask instead)");
    if (n > 0 && c->last_gen != c->sets_gen)
        return fail(c, MIM_EINVAL, "batch_inlier_points: the batch's sets were cleared or truncated since "
                                   "mim_batch_run");
    offsets[0] = 0;
    for (int i = 0; i < n; ++i)  // TestsDetector.cpp:79-84: only accepted problems contribute
        offsets[i + 1] = offsets[i] + (res[i].status == MIM_ACCEPTED ? res[i].n_inl : 0);
    const long long total = n ? offsets[n] : 0;
    if (!out_xy || total == 0) return MIM_OK;
    if (total > cap) return fail(c, MIM_ERANGE, "batch_inlier_points: %lld points, buffer holds %lld", total, (long long)cap);
    // table: offsets (n + 1) then the scales (n), one copy; the gather; one copy of the points back
    const size_t tb = sizeof(long long) * (n + 1) + (scales ? sizeof(float) * n : 0);
    HIPCHK(c, c->inl_tab.ensure(tb));
    HIPCHK(c, c->inl_out.ensure(sizeof(float2) * total));
    StageWriter up(c->stage, tb, c->stream);
    up.put(c->inl_tab.p, offsets, sizeof(long long) * (n + 1), scales, scales ? sizeof(float) * n : 0);
    HIPCHK(c, up.done());
    const long long* offs = c->inl_tab.as<long long>();
    launch_inlier_gather(c->probs.as<ProbDev>(), n, c->results.as<mim_result>(), c->good_t.as<int32_t>(),
                         c->masks.as<uint8_t>(), offs,
                         scales ? reinterpret_cast<const float*>(offs + n + 1) : nullptr, c->inl_out.as<float2>(),
                         c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out_xy, c->inl_out.p, sizeof(float2) * total, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MIM_OK;
}

mim_status mim_find_homography(mim_ctx* c, const float* src, const float* dst, int32_t n, double thresh,
                               int32_t max_iters, double conf, double H[9], uint8_t* mask) {
    if (!c) return MIM_EINVAL;
    if (!src || !dst || !H || !mask) return fail(c, MIM_EINVAL, "find_homography: null pointer");
    if (n < 4)  // CV_Error(StsVecLengthErr) in cv::findHomography
        return fail(c, MIM_EINVAL, "The input arrays should have at least 4 corresponding point sets");
    mim_params prm;
    mim_default_params(&prm);
    prm.ransac_thresh = thresh;
    prm.max_iters = max_iters;
    prm.confidence = conf;
    prm.min_good = 4;
    prm.min_inliers = 0;
    mim_status s = check_params(c, &prm);
    if (s != MIM_OK) return s;
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::vector<float4> pts(n);
    for (int i = 0; i < n; ++i) pts[i] = make_float4(src[2 * i], src[2 * i + 1], dst[2 * i], dst[2 * i + 1]);
    HIPCHK(c, c->pts.ensure(sizeof(float4) * n));
    HIPCHK(c, c->n_good.ensure(sizeof(int)));
    HIPCHK(c, c->probs.ensure(sizeof(ProbDev)));
    HIPCHK(c, hipMemcpy(c->pts.p, pts.data(), sizeof(float4) * n, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->n_good.p, &n, sizeof(int), hipMemcpyHostToDevice));
    ProbDev P{};
    P.q.n = n;
    P.good_off = 0;
    P.it_off = 0;
    HIPCHK(c, hipMemcpy(c->probs.p, &P, sizeof P, hipMemcpyHostToDevice));
    c->h_probs.assign(1, P);
    c->h_good_off.assign(1, 0);
    c->last_n = 1;  // mim_batch_results returns this call's record (mim.h)
    c->last_gen = -1;
    c->last_fh = true;
    c->last_problems.clear();
    mim_result r;
    for (;;) {  // a run out of RNG draws is re-run on a longer stream
        c->cur = c->stream;
        ev_mark(c, "begin");
        s = ransac_locked(c, 1, &prm, 1);
        if (s != MIM_OK) return s;
        HIPCHK(c, hipStreamSynchronize(c->stream));
        ev_collect(c);
        HIPCHK(c, hipMemcpy(&r, c->results.p, sizeof r, hipMemcpyDeviceToHost));
        if (r.status != MIM_STREAM_SHORT) break;
        s = grow_stream(c);
        if (s != MIM_OK) return s;
    }
    HIPCHK(c, hipMemcpy(mask, c->masks.p, n, hipMemcpyDeviceToHost));
    if (r.status == MIM_EMPTY_H) {
        for (int i = 0; i < 9; ++i) H[i] = 0;
        memset(mask, 0, n);
        return MIM_ENOMODEL;
    }
    for (int i = 0; i < 9; ++i) H[i] = r.H[i];
    return MIM_OK;
}

}  // extern "C"
