// mim_internal.h — device-side data layout shared by the HIP kernels and the host launcher.
// See DESIGN.md "Data layout in HBM".  gfx950 only (wave64, i8 MFMA 32x32x32, f16/fp64 RANSAC).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "knn_schedule.h"  // KnnWork, kKnnBlockQ and what it is derived from, the Hamming block constants
#include "knn_topk_merge.h"  // TopkEnt

namespace mim {

constexpr int kDim = 128;          // SIFT descriptor length (TestsDetector.cpp:60 operands)
constexpr int kTileRows = 64;      // descriptor rows per staged tile
constexpr int kTileBytes = kTileRows * kDim;  // 8 KiB of i8 per tile
constexpr int kNormWords = 4 * kTileRows;      // norm block per tile (knn.hip prep_tile)
constexpr int kWave = 64;
#ifndef MIM_KNN_STAGE
#define MIM_KNN_STAGE 4
#endif
constexpr int kKnnStage = MIM_KNN_STAGE;       // 64-row train tiles per LDS stage (per barrier)

// One descriptor set = one ObjectModel view (objectModel.hpp:11-16) or one scaled scene
// (TestsDetector.cpp:104-106), resident in HBM.
struct SetDev {
    const int8_t* frag;    // 127 - d as i8, "fragment-major" tiles: [tile][u 0..1][kstep 0..3][lane 0..63][16]
    const int* norm;       // per tile kNormWords: floor(n2/2), n2 & 1, c, early-phase key addends (knn.hip prep_tile)
    const float* f32;      // row-major n x 128 fp32 (the caller's CV_32F rows)
    const float2* kp;      // KeyPoint::pt per row
    int n;
    int n_tiles;           // ceil(n / 64)
    int* flags;            // bit0: a value is not an integer in [0,255]
};

// Deferred prep of one set (i8 fragments, norms, integrality flag), batched per match call.
struct PrepJob {
    const float* src;
    int8_t* frag;
    int* norm;
    int* flags;
    int n;
    int tile0;  // first block of this set in the batched launch
};

struct Top2 {  // partial top-2 of one query over one train split; key = distance (float)
    float k1; int i1; float k2; int i2;
};

// Per-problem device record (knn + ratio + RANSAC).  Built by the host launcher.
struct ProbDev {
    SetDev q, t;
    int nsplit;          // train splits for the distance kernel
    int q_pad;           // nq rounded up to kKnnBlockQ
    long long part_off;  // into Top2 partials: [split][q_pad]
    long long good_off;  // into good arrays (capacity nq)
    long long it_off;    // into per-iteration arrays (capacity max_iters)
};

// Binary descriptor sets (hamming.hip, DESIGN.md "Binary descriptors").  Such a set's SetDev has
// frag = its rows zero-padded to 16, 32 or 64 bytes (zero rows up to the next multiple of kHamTileRows
// past the last row), kp and n; norm, f32 and flags are null.  The padded width is host knowledge
// (api.cpp SetRec), carried to the device in each work item.  kHamBlockQ, kHamTileRows: knn_schedule.h.

// Work item of the Hamming kernel: kHamBlockQ queries from q0 x train rows [r0, r1) of one problem,
// written to one train split.  r0 is a multiple of kHamTileRows.
struct HamWork {
    const uint32_t* q;   // padded query rows of the problem
    const uint32_t* t;   // padded train rows
    Top2* out;           // the split's partials: parts + part_off + split * q_pad
    int nq;
    int q0;
    int r0, r1;
    int wdw;             // dwords per padded row: 4, 8 or 16
    int pad_;
};

// Work item of the one-pass Hamming cross kernel (knn2_hamming_cross_kernel): the same piece, and the
// problem's column minima colmin[nt], packed keys distance << 18 | query row, 0xFFFFFFFF before any.
struct HamCrossWork {
    HamWork w;
    uint32_t* colmin;
};

// Cross-check table of one problem (cross_compact_kernel): where the reverse nearest
// row of a train row is found.
struct CrossDev {
    const uint32_t* colmin;  // fused Hamming kernel's column minima [nt]; null: the shadow's partials
    int shadow;              // the shadow's ProbDev (the two sets swapped), -1 with colmin
    int pad_;
};

// Generic float sets (knn_float.hip, DESIGN.md "Float descriptors of any dimension").  Such a set's
// SetDev has f32 = its rows at a stride of `dp` floats (dim rounded up to a multiple of 4, zero filled;
// zero rows up to the next multiple of kFltRowPad past the last row), kp and n; frag, norm and flags are
// null.  dim is host knowledge (api.cpp SetRec), carried to the device in each work item.

// Work item of the generic-float kernel: kFltBlockQ queries from q0 x train rows [r0, r1) of one
// problem, written to one train split.  r0 is a multiple of kFltRowPad.
struct FltWork {
    const float* q;      // padded query rows of the problem
    const float* t;      // padded train rows
    Top2* out;           // the split's partials: parts + part_off + split * q_pad
    int nq;
    int q0;
    int r0, r1;
    int dim;             // floats per row as the caller gave them (1..kFltMaxDim)
    int dp;              // floats per stored row: dim rounded up to a multiple of 4
};

// The shared sweeps (sweep_hamming.h, sweep_float.h): one piece of knn_hamming_plan /
// knn_float_plan, without where its results go.  The top-k and radius work items are this plus that.

// kHamBlockQ queries from q0 x train rows [r0, r1) of one problem; r0 is a multiple of kHamTileRows.
struct HamSweepWork {
    const uint32_t* q;   // padded query rows of the problem
    const uint32_t* t;   // padded train rows
    int nq;
    int q0;
    int r0, r1;
    int wdw;             // dwords per padded row: 4, 8 or 16
};

// kFltBlockQ queries from q0 x train rows [r0, r1) of one problem, for generic float sets and for the f32 rows
// of 128-D sets (dim = dp = 128), whose storage ends at row nt and whose pointers the caller may have borrowed us.
struct FltSweepWork {
    const float* q;
    const float* t;
    // the 128-D sets' integrality flags (SetDev::flags) where an i8 MFMA kernel runs beside the float one: a
    // block returns at once when both say integer-valued, the i8 kernel owns those pairs.  Null otherwise.
    const int* qflags;
    const int* tflags;
    int nq;
    int q0;
    int r0, r1;
    int dim;             // floats per row as the caller gave them (1..kFltMaxDim)
    int dp;              // floats per stored row
    int nt;              // train rows: no row from nt on is read
    int vec;             // both row pointers are 16-byte aligned (dp is a multiple of 4): float4 loads
};

// Top-k entries (knn_topk.hip): mim_knn_batch_dev and what is built on it.  A piece writes its
// queries' sorted lists of k entries to the split's share of the top-k partials, [q_pad][k] TopkEnt.
struct TopkHamWork {
    HamSweepWork s;
    TopkEnt* out;        // the split's lists: the problem's partials + split * q_pad * k
};
struct TopkFltWork {
    FltSweepWork s;
    TopkEnt* out;
};

// One problem of the top-k merge and emit kernel.
struct TopkProb {
    const TopkEnt* parts;  // [nsplit][q_pad][k]
    int32_t* idx;          // the problem's output rows [nq][k]
    float* dist;
    int nq;
    int nsplit;
    int q_pad;
    int pad_;
};

// RANSAC state per problem (RANSACPointSetRegistrator::run locals, ptsetreg.cpp).
struct RansacState {
    long long stream_pos;  // RNG draws consumed so far (all calls see RNG((uint64)-1))
    int produced;          // samples produced (iterations whose getSubset succeeded)
    int fail_iter;         // iteration whose getSubset failed after 10000 attempts (-1: none)
    int fail_run;          // consecutive failed subset attempts carried across sampler rounds
    int niters;            // current iteration bound (RANSACUpdateNumIters)
    int max_good;          // maxGoodCount
    int best_iter;         // iteration of bestModel
    int next_iter;         // first iteration not yet replayed by the select kernel
    int done;              // loop finished (iter >= niters or getSubset failure)
    int n;                 // point count (= n_good)
    int active;            // problem takes the RANSAC path (n_good > 4)
    int lo_max;            // max lower-bound count seen (filtered path: lower bound of maxGoodCount)
    unsigned long long modM;  // Lemire fast-modulo constant for % n (RNG::uniform(0, n))
    float sa, sb;          // power-of-two scales of the source / destination coordinates (MFMA bound)
    float smax;            // max over points of |x|+|y|+|u|+|v| (MFMA bound margin)
    int defer;             // chunk 1's exact pass deferred to chunk 2's (no early stop possible in chunk 1)
};

struct RansacParams {
    double thresh;   // reprojection threshold (5.0)
    double conf;     // 0.995
    int max_iters;   // 2000 (reference) / 50000 (BASELINE C3/C4)
    float ratio;
    int min_good, min_inliers;
    double det_lo, det_hi;
    int cand_cap;    // candidate-list capacity per problem and chunk (0: kCandPerProblem)
    int rep_cap;     // attempt kernel's list of repeated-index positions per block (0: kAttemptRepCap)
};

}  // namespace mim

namespace mim {
constexpr int kCandPerProblem = 1024;  // listed exact-evaluation candidates per problem and chunk
constexpr int kIrrBlock = 16384;       // attempt positions per irregular-list block
constexpr int kRansacDefSlots = 16;             // deferred attempts listed per check round (ransac.hip)
#ifndef MIM_CHECK_PER
#define MIM_CHECK_PER 4  // chain attempts per thread and check round (ransac.hip kCheckPer)
#endif
constexpr int kRansacDefRoundAttempts = 256 * MIM_CHECK_PER;  // chain attempts per check round (kCheckBlock x kCheckPer)
constexpr int kIrrCap = 4096;          // listed irregular attempts per block (25 %: n >= ~25 points fit)

// Sampler class of one problem and chunk (ransac_class_kernel).  The attempt tables (flags, irr_bits,
// irr, irr_cnt) are a function of (RNG stream, n, absolute stream position) only, so the windowed
// problems of a call with equal n and nearby stream positions form a class whose leader (smallest
// stream_pos) builds the tables once, in its own slices, at positions relative to the class base.
struct SamplerClass {
    long long base;  // stream position of the leader's flags[0]: the leader's stream_pos rounded down to 64
    int leader;      // problem whose slices hold the class's tables (-1: no window this chunk)
    int cwlen;       // positions the leader's tables cover (a multiple of 64, <= wcap)
    int delta;       // stream_pos - base
    int wlen;        // own window length (a multiple of 64): delta + wlen <= cwlen
    int pad_[2];
};
// Slot n of the class table: key = (smallest stream_pos << 32 | that problem) over the windowed
// problems with n points, end = largest delta + window length over the class's members.
struct SamplerClassSlot {
    unsigned long long key;
    int end;
    int pad_;
};

// Device buffers of one RANSAC batch (owned by the ctx in api.cpp).
struct RansacBufs {
    RansacState* state;       // [n_probs]
    int4* samples;            // [it_off + iter]  4 point indices of the minimal sample
    float* hyp;               // [(it_off + iter) * 8]  (float)H[0..7] of the minimal-sample model
    int* counts;              // [it_off + iter]  inlier count, -1 when runKernel returned 0
    int2* bounds;             // [it_off + iter]  (lower, upper) bound of the count (filtered path)
    double* best_h;           // [problem][9] bestModel of the filtered select (double H of the best sample)
    int* cand;                // [problem][list 0..1][kCandPerProblem] candidate iterations (list = chunk)
    int* ncand;               // [problem][list] candidates listed (may exceed the capacity)
    int* cex;                 // [problem][list][kCandPerProblem] their exact inlier counts
    double* cH;               // [problem][list][kCandPerProblem][9] their exact models
    int* decided;             // [problem][list][kCandPerProblem] 1: the prescreen decided the listed candidate
    uint8_t* flags;           // [problem][window] getSubset attempt outcomes from the class base on (written and
                              // valid only where irr_bits is set: the repeated-index and serial attempts);
                              // flags, irr_bits, irr and irr_cnt: only the slices of class leaders are written
    uint8_t* irr_bits;        // [problem][window / 8] bit per attempt position: irregular (its flag byte is
                              // written); a clear bit means kPassUnknown (4 draws, checkSubset not evaluated)
    long long flag_cap;       // bytes of `flags`
    int* irr;                 // [problem][block][kIrrCap] positions of irregular attempts (chain sampler)
    int* irr_cnt;             // [problem][block] their count (-1: more than kIrrCap)
    uint32_t* pass_bits;      // [problem][window / 32] bit per chain attempt: checkSubset passes
    void* chains;             // [problem] ChainSegs (ransac.hip): the walked chain of the chunk
    int2* defer;              // [problem][check round][kDefSlots] deferred attempts (attempt index, position)
    int* defer_n;             // [problem][check round] how many are listed
    int def_rounds;           // check rounds per problem with a list (0: every deferred attempt in place)
    int irr_blocks;           // list blocks per problem
    SamplerClass* cls;        // [problem] sampler class of the current chunk
    SamplerClassSlot* cls_tab;  // [cls_tab_n] class table indexed by the point count (one enqueue at a time)
    int cls_tab_n;            // its slots: the largest query set + 1
    const uint32_t* stream;  // raw cv::RNG((uint64)-1).next() stream shared by every problem
    long long stream_len;
    float4* inl;              // [good_off + k] compressed inliers for the refit (scratch)
    uint4* tiles;             // [good_off / 32 + tile][2][64] f16 MFMA operand tiles of the points
    float4* tbox;             // [good_off / 32 + tile] (cx, cy, rx, ry): box of the tile's source points (scaled)
    int* perm;                // [2 * good_off ..][2][n] scratch of the tiles' order (arrival order, row -> point)
    int* surv;                // [it_off + k] iterations of the chunk whose capped upper bound beats the bar
    int* nsurv;               // [problem] how many are listed
    int4* strip;              // [problem] strip pre-stage: (bar B, strip records stand, iterations above the bar,
                              // largest pilot count), ransac_strip_pilot_kernel
    int* err;                 // device error word (bit0: RNG stream exhausted)
    // Sampler stream: the getSubset replay of chunk c+1 runs on s2 concurrently with the bound /
    // candidate / exact / replay kernels of chunk c (null: everything on the caller's stream)
    hipStream_t s2;
    hipEvent_t ev_fork;
    hipEvent_t ev_samp[2];
};
}  // namespace mim

// SIFT detectAndCompute + 8-bit linear resize (sift.hip), driven by mim_sift_detect_compute /
// mim_resize_linear_u8 (api.cpp).  Return 0, -1 on a HIP error, -2 when the caller's keypoint buffer is
// too small (the counts are set), -3 on a bad argument, -4 when an internal hard limit is exceeded
// (image size, candidates, keypoints, Gaussian kernel size); `err` gets the text.
#include <string>
#include <vector>
#include "../../include/mim.h"
namespace mim {
struct SiftWs;
SiftWs* sift_ws_create();
void sift_ws_destroy(SiftWs* w);
int sift_detect_compute(SiftWs* w, hipStream_t st, const uint8_t* img, int rows, int cols, long long step,
                        const uint8_t* mask, long long mstep, int max_kp, mim_keypoint* kps, float* desc, int* n_out,
                        std::string& err);
int sift_detect_compute_scales(std::vector<SiftWs*>& ws, hipStream_t st, const uint8_t* img, int rows, int cols,
                               long long step, int n_scales, const float* scales, int max_kp, mim_keypoint* kps,
                               float* desc, int* n_out, std::string& err);
int sift_resize_u8(SiftWs* w, hipStream_t st, const uint8_t* src, int rows, int cols, long long step, uint8_t* dst,
                   int drows, int dcols, double fx, double fy, std::string& err);
// the keypoints / descriptors of one image left on the device by sift_scales_device
struct SiftDevOut {
    const mim_keypoint* kp;
    const float* desc;
    int n;
};
// img: `channels` 1 (CV_8UC1) or 3 (CV_8UC3 in B, G, R order: converted to gray on the device first)
int sift_scales_device(std::vector<SiftWs*>& ws, hipStream_t st, const uint8_t* img, int rows, int cols,
                       long long step, int channels, int n_scales, const float* scales, SiftDevOut* out,
                       std::string& err);
// cvtColor(BGR2GRAY) of a CV_8UC3 image (row step `step` bytes) into the dense rows x cols plane `gray`
int sift_bgr2gray_u8(SiftWs* w, hipStream_t st, const uint8_t* bgr, int rows, int cols, long long step, uint8_t* gray,
                     std::string& err);
// out[j]'s n rows and keypoint positions into ddesc[j] / dkp[j], j < n <= 8, one launch (0, -1 HIP error)
int sift_copy_sets(const SiftDevOut* out, int n, float* const* ddesc, float2* const* dkp, hipStream_t st);
// test support: the pyramid and counters the last SIFT call left in w (mim_sift_debug_pyramid)
int sift_debug_pyramid(SiftWs* w, hipStream_t st, int* n_oct, int* orows, int* ocols, float* planes, long long cap,
                       long long* need, int* counters, std::string& err);
}  // namespace mim
