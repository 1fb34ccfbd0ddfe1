// fv_internal.h — what the translation units of libflashvit.so share: the context behind the opaque fv_ctx of
// include/flashvit.h, device buffers, the error macro and the few functions that cross a seam.
//   fv_context.hip  fv_create / fv_destroy / options / statistics, workspace, batch admission, decode epilogue, model upload, emission staging
//   fv_model.cpp    the host-only model builders of fv_set_model / fv_set_model_sparse (value checks, logs, table encodings)
//   fv_full.hip     full-state kernels and their decode drivers (FLASH, vanilla, checkpoint)
//   fv_beam.hip     FLASH-BS kernels and their decode driver
//   fv_comm.hip     multi-GPU: partition, RCCL all-gather, merge, the single-process multi-device context
//   fv_stream.hip   fv_stream_* / fv_streams_*: the online decode — the ancestor kernels, the buffers of a stream and of a set
//                   of streams, and their entry points
//   fv_sumprod.hip  fv_loglik / fv_loglik_batch / fv_posteriors: the sum-product kernels and their driver; fv_expected_counts
#pragma once

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "flashvit.h"
#include "fv_layout.h"
#include "fv_schedule.h"

using clk = std::chrono::steady_clock;
inline double ms_since(clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); }

// device memory that frees itself (on the device that is current: fv_destroy sets it before it deletes the context)
template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    hipError_t ensure(size_t want)
    {
        if (want <= n) return hipSuccess;
        if (p) { (void)hipFree(p); p = nullptr; n = 0; }
        hipError_t e = hipMalloc(&p, want * sizeof(T));
        if (e == hipSuccess) n = want;
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
    size_t bytes() const { return n * sizeof(T); }
};

namespace fvb { struct HNode { float v; int s; }; }         // heap node / select candidate: {value, state}

// The bits of FV_OPT_DEBUG the host code tests (fv_ctx::opt_debug), named after what include/flashvit.h says each does.
// (Bits 0, 4, 5, 11, 12 are FV_DEBUG_TIMING_ONLY: the kernels of the timing build read them from their arguments.)
enum : int {
    FV_DBG_NO_REVERSE = 1 << 1,             // full-state: no reverse sweep
    FV_DBG_ALT_LOADS = 1 << 2,              // alternate load schedule
    FV_DBG_FULL_LAST_STEP = 1 << 3,         // full last step instead of one column
    FV_DBG_GRAPH = 1 << 6,                  // hipGraph replay of a generation
    FV_DBG_OWN_CUTS = 1 << 7,               // FLASH-BS: the cut predictor uses the pass's own cuts only
    FV_DBG_BEAM_F64 = 1 << 8,               // float64 step kernel always
    FV_DBG_BEAM_Q16 = 1 << 9,               // 16-bit step kernel always
    FV_DBG_NO_CAND_LISTS = 1 << 10,         // no candidate lists
    FV_DBG_U16_W16 = 1 << 13,               // full-state: packed kernel in 16-wave workgroups
    FV_DBG_U16_BATCHED = 1 << 14,           // packed kernel for every batched launch
    FV_DBG_SELECT_WHOLE_GROUP = 1 << 15,    // FLASH-BS: whole-workgroup select for short lists too
    FV_DBG_BEAM_ONE_STREAM = 1 << 16,       // pass groups on one stream whatever the size
    FV_DBG_BEAM_GROUPS = 1 << 17,           // pass groups on four streams whatever the size
    FV_DBG_FULL_ONE_STREAM = 1 << 18,       // full-state: right-hand generations on one stream
    FV_DBG_ALL_LAYOUTS = 1 << 19,           // FLASH-BS: every heap layout rebuilt, every tie re-decided
    FV_DBG_EAGER_REPLAY = 1 << 20,          // every duplicate step replays its heap at once
    FV_DBG_SLABS = 1 << 21,                 // full-state: three slabs of source rows at any size
    FV_DBG_SELECT_IN_MEMORY = 1 << 22,      // FLASH-BS: every selection in the memory-resident form
    FV_DBG_DECIDE_IN_FULL = 1 << 23,        // runs of undecided steps always decided in full
    FV_DBG_SELECT4_DIRTY = 1 << 24,         // four-wave select also on steps that may have to be resolved
    FV_DBG_BEAM_WIDE = 1 << 25,             // 16-wave step-kernel workgroups whatever the launch size
    FV_DBG_BEAM_NARROW = 1 << 26,           // 8-wave workgroups of the 16-bit step kernel whatever the launch size
    FV_DBG_BATCH_GEN0_SERIAL = 1 << 28,     // fv_decode_full_batch: generation 0 in single-stream launches
    FV_DBG_BEAM_BATCH_GEN0_OTHER = 1 << 29, // fv_decode_beam_batch: generation 0 in the launch form that is not the default
};

struct fv_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    // FLASH-BS: the passes of a generation are dealt to up to 1 + BEAM_AUX streams, so that the selects / exact replays
    // of one group (a CU each) run under the step kernels of the others
    static constexpr int BEAM_AUX = 3;
    hipStream_t aux[BEAM_AUX] = { nullptr, nullptr, nullptr };
    hipEvent_t ev_fork = nullptr, ev_join[BEAM_AUX] = { nullptr, nullptr, nullptr };
    bool fork_active = false;     // a forked generation of the current decode has been queued
    int num_cus = 256;       // multiProcessorCount of the device (MI355X: 256)
    hipEvent_t ev_start = nullptr, ev_stop = nullptr, ev_top = nullptr, ev_s0 = nullptr, ev_s1 = nullptr;
    std::string detail;

    // model
    int K = 0, M = 0, nrows = 0;
    bool full_ok = false;    // every full-state kernel can take this K (one float32 score row fits LDS: K <= ~40100)
    bool u16_ok = false;     // the packed 16-bit kernel can (one row of 16-bit score codes fits LDS: K <= 65536; beyond: float64 slabs)
    bool logs_nonpositive = false;
    DevBuf<float> LA32, LB32T;
    DevBuf<unsigned short> LA16, LAQ16;
    DevBuf<uint4> SPdata;    // sparse CSC-Q16 table (fv_kernels.hip.inc, trellis_step_sparse)
    DevBuf<int> SPoff, SPnwb;
    double density = 1.0;    // finite fraction of log A
    float window16 = 0.0f;   // 2 * max |half(L) - L| over the finite table entries
    float windowq = 0.0f, qscale = -1.0f;   // same for the fixed-point table; value = code * qscale
    bool laq16_ready = false; // LAQ16 holds this model's codes and windowq / qscale belong to it (host-built in fv_set_model, or
                              // built on the device by the first full-state decode of a model beyond the float32 kernels' limit)
    DevBuf<double> LA64, LB64T, LPi64;
    // a model set by fv_set_model_sparse (csr): no dense table at all.  Per destination column the stored finite entries in
    // ascending source state (fv_kernels.hip.inc, trellis_step_csr), and the caller's rows for init_rows
    bool csr = false;
    DevBuf<uint4> CSk;           // source states: a lane load holds 4 consecutive entries of one column
    DevBuf<uint2> CSq;           // their Q16 codes (4 x 16 bit), same vector index
    DevBuf<double> CS64;         // their float64 logs: entry q of vector v at 4 * v + q
    DevBuf<long long> CSoff;     // [ntiles] first vector of each 16-column tile
    DevBuf<int> CSnwb;           // [ntiles] wave-blocks (64 vectors) of each tile
    DevBuf<long long> CRptr;     // [K + 1] rows by source state: log A[Ans[L-1]][*] of init_rows
    DevBuf<int> CRcol;
    DevBuf<double> CRlog;
    // per-time emission scores staged by fv_set_emissions: row t holds the K log scores of time t, in the
    // two precisions of LB32T / LB64T, so that "symbol of time t = t" makes every kernel read them as it reads log B
    DevBuf<float> E32;
    DevBuf<double> E64;
    DevBuf<unsigned long long> d_emflags;    // [0] FV_EMIS_BAD / FV_EMIS_POSITIVE bits, [1] lowest t * K + i of a refused value
    long long emis_rows = 0;     // staged rows (0: none)
    bool emis_positive = false;  // a staged score is above 0
    // fv_set_emission_map: the K states share emis_P score classes through EMap[K] (emis_P == 0: no map, rows of K scores);
    // it belongs to the model, as log B does
    DevBuf<int> EMap;
    int emis_P = 0;
    std::vector<int> h_iota;     // 0, 1, 2, ...: the observation sequence of a decode given ob == NULL
    // What the decode in flight reads its emission term from (fvi::emission_view sets it first thing in every decode):
    // log B of the model by symbol, or the staged rows by time.
    struct EmisView {
        const float *lb32 = nullptr;
        const double *lb64 = nullptr;
        int nsym = 0;                    // rows of lb32 / lb64: the bound of an observation
        bool logs_nonpositive = false;   // every log of the model and of these rows is <= 0 (the filter kernels' condition)
    } view;

    // workspace
    DevBuf<int> d_ob, d_ans, d_bp, d_gather;
    DevBuf<float> d_rows, d_score, d_ckpt;            // d_ckpt: kept score rows of fv_decode_checkpoint
    DevBuf<unsigned long long> d_counters;
    // FV_OPT_ROW_CODES (fv_full.hip, launch_step_kernel): beside every score row of d_rows its 16-bit codes [nrows] and
    // its tile maxima [nrows / 16], allocated only for decodes that take the route (row_codes != 0).  row_coded[r]: row r
    // of d_rows (in units of nrows floats) was last written by a kernel that left its codes — the host knows, launch by launch.
    DevBuf<unsigned short> d_rcodes;
    DevBuf<float> d_rtmax;
    std::vector<unsigned char> row_coded;
    int row_codes = 0;       // the decode in flight: bit 0 single-task launches take the route, bit 1 batched launches
    // FV_OPT_FLAT_GENERATIONS (fv_full.hip, run_flat_full): snapshot S of the whole-sequence chain, the private arg rows of
    // the generations >= 2, the chain of every right-hand pass and the pass table the back-track and the resolver read
    DevBuf<int> d_snap, d_flat_bp, d_chain;
    DevBuf<fvk::FlatDesc> d_flat;
    fv::FlatPlan flat_plan;                   // the plan d_flat holds, kept across decodes of one (T, n_split, cap, streams)
    int flat_key[4] = { 0, 0, 0, 0 };
    const void *flat_uploaded = nullptr;      // d_flat.p at the upload (a grown buffer is filled again)
    int flat_poison = -1;                     // fv_test_flat_poison
    // decode epilogue: path (or the gathered paths), score and counters are packed into one device block and come back
    // in ONE copy into pinned host memory (three small pageable copies cost ~15 us each)
    DevBuf<int> d_pack;
    int *h_pin = nullptr;
    size_t h_pin_n = 0;          // ints
    // beam workspace
    DevBuf<float> d_hval, d_scores, d_slot_val;      // [T][B] members, [T][K] scores, [T][B] exact layout
    DevBuf<int> d_hstate, d_slot_state, d_flags;
    DevBuf<double> LA64R;                            // row-gather copy of the float64 table (built on first beam decode)
    DevBuf<unsigned short> LAQ16R;                   // row-major fixed-point table of beam_step_q16 (built on the first beam decode, with d_qaux's parameters)
    bool rowq_ready = false, beam_q16_ready = false; // LAQ16R holds this model's codes / d_qaux holds its parameters
    DevBuf<unsigned long long> d_qaux;               // [0] lmax bits, [1] dmax bits, then {qscale, window} as floats (q16_params)
    DevBuf<int2> d_tie_list;
    DevBuf<float> d_cut;         // [T][CUT_W] theta, duplicate flag, predicted lower bound of the next cut (topb_select)
    DevBuf<fvb::HNode> d_cand;   // [T][cand_cap] candidate lists of the selects (beam_step epilogue)
    DevBuf<int> d_cand_count;    // [T]
    float opt_sel_margin = 0.3f; // FV_OPT_SEL_MARGIN (in 1/1000): starting margin of the predicted cut bound in beam spreads
    DevBuf<int> d_dupwin;        // [T]
    DevBuf<int> d_doubt, d_doubt_count;   // [T][DOUBT_CAP] columns of step j won by an undecided cut duplicate of step j - 1, [T] their number
    DevBuf<int> d_needfull;      // [sequences of the call] a pass's back-track met a tied cell: rebuild the layouts of its sequence's
                                 // passes of the generation (beam_end_backtrack); one flag for fv_decode_beam
    DevBuf<int> d_seqof;         // fv_decode_beam_batch: [total T] sequence of every absolute time (heap_build_all, tie_fixup)
    std::vector<int> h_seqof;
    DevBuf<int> d_passL;         // first position of every pass of the generation in flight (beam decodes)
    std::vector<int> h_passL;
    DevBuf<unsigned int> d_tie_count;
    // FV_OPT_SPARSE_BEAM (beam_scatter_csr / beam_finish_csr): per (observation, state) the packed column maximum and the tie
    // word, all zero outside a step launch; allocated only by beam decodes of a sparse-set model
    DevBuf<unsigned long long> d_csr_acc;
    DevBuf<unsigned int> d_csr_tie;
    long long csr_nnz = 0;       // stored entries of the model set by fv_set_model_sparse

    // options
    int opt_sparse_beam = 0; // FV_OPT_SPARSE_BEAM: the beam calls run on a model set by fv_set_model_sparse
    int opt_kernel = FV_KERNEL_AUTO;
    int opt_max_batch = fvk::MAX_BATCH;
    int opt_profile = 0;
    int opt_flat = 1;        // FV_OPT_FLAT_GENERATIONS: 0 off, 1 auto, 2 on
    int opt_row_codes = 1;   // FV_OPT_ROW_CODES: 0 off, 1 auto, 2 on; 3 / 4 (measurements): single-task / batched launches only
    int vanilla = 0;         // set for the duration of fv_decode_vanilla
    int opt_csr_mem = 0;     // FV_OPT_DEBUG bit 31: trellis_step_csr / trellis_step_csr_f64 read their score rows from memory at any K
    int opt_debug = 0;       // FV_OPT_DEBUG: the FV_DBG_* bits below; include/flashvit.h says what each does
    std::vector<hipEvent_t> prof_events;
    std::vector<int> h_ob;
    std::vector<hipGraphExec_t> graphs;     // experiment (FV_OPT_DEBUG bit 6): destroyed after the decode's sync
    // test hooks (include/flashvit_testing.h): while test_record is set, the launch helpers OR the FV_TV_* bit of every
    // step-kernel instantiation they launch into test_variants (a host branch; nothing else runs on a decode)
    bool test_record = false;
    unsigned long long test_variants = 0;
    unsigned long long test_selects = 0;     // the same for the select kernels: FV_TS_* bits

    // comm
    ncclComm_t comm = nullptr;
    int rank = 0, nranks = 1;
    // single-process multi-device context (fv_create_multi): every member points to the group; member 0 is the handle
    // the caller holds and the one that owns the group
    struct fv_group *group = nullptr;
    int group_rank = 0;

    // fv_stream_* (fv_stream.hip): the open stream and its device buffers, which are its own — allocated at open and on
    // growth, freed at close or abort, in no workspace request and not in each_buffer — and the statistics of the open or
    // the last stream
    struct fv_stream *strm = nullptr;
    fv_stream_stats strm_stats{};
    bool strm_any = false;
    // fv_streams_*: the open set of streams (the same rules: its buffers are its own), the statistics of the open or the last set
    struct fv_streams *set = nullptr;
    fv_streams_stats set_stats{};
    bool set_any = false;
    // fv_set_max_lag: the bound streams and sets opened from now on force commits at (0: none; kept across fv_set_model*),
    // and fv_last_lag_stats' record of the last stream closed or aborted and of the slots of the last set ended
    long long max_lag = 0;
    fv_lag_stats strm_lag{};
    std::vector<fv_lag_stats> set_lag;

    // fv_loglik / fv_posteriors (fv_sumprod.hip).  SPA / SPAT: A and its transpose as float32, tile-major as
    // LA32 with pads of 0, built on the device from LA64 by the first call that needs each; they belong to the model.
    // sp_rows: the score rows of the forward pass (two per sequence, or all T of fv_posteriors), sp_beta: the backward
    // pass's, sp_res: [refine counters | one loglik per sequence], sp_gamma / sp_path: results staged for the host
    DevBuf<float> SPA, SPAT;
    bool spa_ready = false, spat_ready = false;
    DevBuf<double> sp_rows, sp_beta;
    DevBuf<unsigned long long> sp_res;
    DevBuf<float> sp_gamma;
    DevBuf<int> sp_path;
    fv_sumprod_stats sp_stats{};
    bool sp_any = false;
    // fv_set_sparse_sumprod: the same calls on a model set by fv_set_model_sparse (kept across
    // fv_set_model*).  CSlin / CRlin: the stored values as float32 at the index of CS64 / CRlog (pads 0), built on the
    // device from those logs by the first call that needs each; they belong to the model.  sp_scaled / sp_scale_m: the
    // memory form's scaled rows of one step launch, and [their maxima | the partial maxima of sumprod_rowmax].
    // sp_forms: the FV_SPF_* bits of the step kernels the last call launched (fv_test_sumprod_forms)
    int opt_sparse_sumprod = 0;
    long long csr_vectors = 0;   // vectors of the CSC-32 table (CSk holds one element more when there is none)
    DevBuf<float> CSlin, CRlin;
    bool cslin_ready = false, crlin_ready = false;
    DevBuf<double> sp_scaled, sp_scale_m;
    unsigned long long sp_forms = 0;
    // fv_expected_counts (fv_sumprod.hip).  ct_p / ct_q: the scaled rows P and Q of the sequence in flight
    // ((T - 1) x K each), ct_wide: its wide-time flags, ct_ob: the call's observations; the call's float64 accumulators
    // ct_trans (K x K, unless trans_out is a device block), ct_emit (K x M) and ct_vec [init | occ]; ct_emit_seq: the
    // emission sums of the sequence in flight
    DevBuf<double> ct_p, ct_q, ct_trans, ct_emit, ct_emit_seq, ct_vec;
    DevBuf<int> ct_ob, ct_wide;
    fv_counts_stats ct_stats{};
    bool ct_any = false;

    fv_stats stats{};
    // statistics of a decode about to start: everything cleared but what the model and the staged emissions own
    void start_stats(int kernel, int generations, long long table_bytes_per_step, double density_reported)
    {
        const double model_ms = stats.set_model_ms, emis_ms = stats.set_emissions_ms;
        const long long rows = stats.emission_rows;
        stats = fv_stats{};
        stats.set_model_ms = model_ms; stats.set_emissions_ms = emis_ms; stats.emission_rows = rows;
        stats.kernel = kernel; stats.generations = generations;
        stats.table_bytes_per_step = table_bytes_per_step; stats.density = density_reported;
        stats.flat_first_miss = -1;
    }
    // ... and of one whose launches are all queued: cells evaluated per task step and per column step, 4 B each
    void close_stats(long long cells_per_task_step, long long cells_per_column_step)
    {
        stats.cells = stats.task_steps * cells_per_task_step + stats.column_steps * cells_per_column_step;
        stats.alg_bytes = 4 * stats.cells;
    }

    // every device buffer of the context: the one list (device_bytes adds them up; each frees itself with the context)
    template <class F>
    void each_buffer(F &&f) const
    {
        f(LA32); f(LB32T); f(LA16); f(LAQ16); f(SPdata); f(SPoff); f(SPnwb); f(LA64); f(LB64T); f(LPi64);
        f(CSk); f(CSq); f(CS64); f(CSoff); f(CSnwb); f(CRptr); f(CRcol); f(CRlog);
        f(E32); f(E64); f(d_emflags); f(EMap);
        f(d_ob); f(d_ans); f(d_bp); f(d_gather); f(d_rows); f(d_rcodes); f(d_rtmax); f(d_score); f(d_ckpt); f(d_counters); f(d_pack);
        f(d_snap); f(d_flat_bp); f(d_chain); f(d_flat);
        f(d_hval); f(d_scores); f(d_slot_val); f(d_hstate); f(d_slot_state); f(d_flags); f(LA64R); f(LAQ16R); f(d_qaux);
        f(d_tie_list); f(d_cut); f(d_cand); f(d_cand_count); f(d_dupwin); f(d_doubt); f(d_doubt_count); f(d_needfull);
        f(d_seqof); f(d_passL); f(d_tie_count); f(d_csr_acc); f(d_csr_tie);
        f(SPA); f(SPAT); f(sp_rows); f(sp_beta); f(sp_res); f(sp_gamma); f(sp_path);
        f(CSlin); f(CRlin); f(sp_scaled); f(sp_scale_m);
        f(ct_p); f(ct_q); f(ct_trans); f(ct_emit); f(ct_emit_seq); f(ct_vec); f(ct_ob); f(ct_wide);
    }
};

// A test hook's scope (include/flashvit_testing.h): the launch helpers record what they launch into the cleared
// test_variants / test_selects until it ends.  on = false: an ordinary decode going through code a hook shares.
struct FvTestRecording {
    fv_ctx *c;
    explicit FvTestRecording(fv_ctx *ctx, bool on = true) : c(ctx) { if (on) { c->test_record = true; c->test_variants = c->test_selects = 0; } }
    ~FvTestRecording() { c->test_record = false; }
    FvTestRecording(const FvTestRecording &) = delete;
    FvTestRecording &operator=(const FvTestRecording &) = delete;
};

#define FV_HIP(call)                                                                          \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess) {                                                               \
            ctx->detail = std::string(#call) + ": " + hipGetErrorString(e_);                  \
            return e_ == hipErrorOutOfMemory ? FV_ERR_NOMEM : FV_ERR_DEVICE;                  \
        }                                                                                     \
    } while (0)

// every entry point that runs on the context's buffers or changes what a stream was opened on refuses while one is open,
// or a set of them
#define FV_NO_STREAM(c)                                                                                        \
    do {                                                                                                      \
        if ((c)->strm) {                                                                                      \
            (c)->detail = "a stream is open on this context: fv_stream_close or fv_stream_abort first";       \
            return FV_ERR_STATE;                                                                              \
        }                                                                                                     \
        if ((c)->set) {                                                                                       \
            (c)->detail = "a set of streams is open on this context: fv_streams_end first";                   \
            return FV_ERR_STATE;                                                                              \
        }                                                                                                     \
    } while (0)

constexpr int FV_NCOUNTERS = fvk::NCOUNTERS;   // device statistics words (fv_layout.h names them)

inline int round_up(int x, int m) { return (x + m - 1) / m * m; }
inline int fv_ldq(int K) { return round_up(K, 128); }         // pitch of the row-major 16-bit table

namespace fvi {

// what fv_set_model computes on the host, once per model
struct HostTables {
    int K = 0, M = 0, nrows = 0, ntiles = 0;
    size_t tab = 0;                      // entries of one tile-major table
    bool full_ok = false, u16_ok = false, any_big = false;
    std::vector<double> h64, b64, pi64;
    std::vector<float> h32, b32;
    std::vector<unsigned short> h16, hq;
    std::vector<uint4> sp;               // sparse CSC-Q16 table
    std::vector<int> sp_off, sp_nwb;
    float window16 = 0.0f, windowq = 0.0f, qscale = -1.0f;
    double density = 1.0;
};
// what fv_set_model_sparse computes on the host: everything is O(nnz + K * M)
struct HostCsr {
    HostTables e;                        // K, M, nrows, ntiles, log B / log Pi, windowq, qscale, density, any_big
    std::vector<uint4> ck;               // CSC-32 table (fv_kernels.hip.inc, trellis_step_csr)
    std::vector<uint2> cq;
    std::vector<double> c64, rlog;       // rlog: the log of every stored entry, in the caller's order
    std::vector<long long> off;
    std::vector<int> nwb;
};
// fv_model.cpp: the two builders, host code only.  A refusal (FV_ERR_ARG) leaves its sentence in `detail`.
int build_host_tables(const float *A, const float *B, const float *Pi, int K, int M, HostTables &h, std::string &detail);
int build_host_csr(const long long *row_ptr, const int *col, const float *val, const float *B, const float *Pi, int K, int M,
                   HostCsr &h, std::string &detail);

size_t device_bytes(const fv_ctx *c);
// A workspace request: buffers and the elements each is wanted to hold.  A batch decode names itself (`what`) and its
// dominant term: its request is then refused with those, before anything is allocated, if the device has not the room.
struct Wants {
    struct Want { void *buf; size_t n, have, elem; hipError_t (*ensure)(void *, size_t); };
    std::vector<Want> list;
    std::string what, dominant;
    template <typename T>
    void add(DevBuf<T> &b, size_t n)
    {
        list.push_back({ &b, n, b.n, sizeof(T), [](void *p, size_t m) { return static_cast<DevBuf<T> *>(p)->ensure(m); } });
    }
};
// grows every buffer of the request; check: the growth is first added up in 64 bits and compared with the free device
// memory plus what growing releases (FV_ERR_NOMEM with bytes needed, the dominant term and bytes free)
int grant(fv_ctx *ctx, const Wants &w, bool check);
// the workspace every decode needs, for T observations, rows_needed passes in flight and nscores scores, added to what
// the caller wants (the beam buffers).  nscores > 1: a batch decode, whose request is checked before it is granted.
int ensure_workspace(fv_ctx *ctx, int T, size_t rows_needed, int nscores = 1, Wants w = {});
// the extra workspace of a flat decode (score rows of `passes` passes, arg_rows private arg rows, the snapshot, the chains and
// the pass table), checked against the free device memory before anything grows: FV_ERR_NOMEM leaves every buffer as it was
int ensure_flat_workspace(fv_ctx *ctx, int T, size_t passes, long long arg_rows, int chain_len);
// Admission of fv_decode_full_batch / fv_decode_beam_batch (`who`, for the detail text), in the steps the entry points
// take in this order: arguments, offsets -> lengths, emission view and model; the symbols' range; the forest plan.
int batch_lengths(fv_ctx *ctx, const char *who, const int *&ob, const long long *offsets, int nseq, int n_split, int mode,
                  const int *path_out, std::vector<int> &lengths);
int batch_symbols(fv_ctx *ctx, const char *who, const int *ob, const long long *offsets, int nseq);
int batch_plan(fv_ctx *ctx, const char *who, const std::vector<int> &lengths, int n_split, int mode, fv::Plan &plan);
// the passes of a plan this rank runs (all of them on a context without a partition), generation by generation;
// most: the size of the largest generation
std::vector<std::vector<fv::Pass>> deal_passes(const fv_ctx *ctx, const fv::Plan &plan, size_t *most = nullptr);
// Decode epilogue of nseq sequences laid end to end (a single decode: nseq = 1, and its one extra branch, the
// multi-rank all-gather + merge): paths / scores / counters to the host in one copy, one sync, statistics.  A sequence
// whose path holds -1 reports FV_ERR_NO_PRED (beam: FV_WARN_BEAM_MISS) in status_out; the return value is the most
// negative status, else the largest.
int finish_decode(fv_ctx *ctx, const fv::Plan &plan, const long long *offsets, int nseq, int *path_out, float *score_out,
                  int *status_out, clk::time_point t0, size_t nprof, bool beam);
int drained(fv_ctx *ctx, int rc);
// decode prologue, before any admission check: chooses what the decode reads its emission term from.  ob != NULL: the
// model's log B.  ob == NULL: the T rows fv_set_emissions staged (FV_ERR_ARG if there are fewer), and ob is pointed at
// 0 .. T-1, which the rest of the decode handles as any observation sequence.
int emission_view(fv_ctx *ctx, const int *&ob, long long T);
// fvk::stage_emissions lives with the full-state kernels (fv_full.hip); stage_block launches it through here
enum { FV_EMIS_BAD = 1, FV_EMIS_POSITIVE = 2 };
// (through the context's emission map while one is set: the tied form)  E32 / E64: the two tables the rows go to, flags: the
// two words the value rules report into (fv_set_emissions: the context's; a stream: its own chunk tables)
int launch_stage_emissions(fv_ctx *ctx, const void *src, int dtype, long long ld, int T, float *E32, double *E64, unsigned long long *flags);
// Staging a block of emission scores: the one path of fv_set_emissions, a stream's score-row push and
// fv_test_stage_emissions_ms.  n rows of K scores (P while an emission map is set) at row pitch ld, in elements of dtype.
struct EmisBlock { const void *scores; int dtype; int n; long long ld; };
constexpr size_t emis_elem_size[4] = { 4, 8, 2, 2 };      // by FV_EMIS_LOG_F32, _F64, _F16, _BF16
inline size_t emis_width(const fv_ctx *ctx) { return ctx->emis_P ? (size_t)ctx->emis_P : (size_t)ctx->K; }    // scores of a row
// the argument rule (each caller words its own refusal)
inline bool emis_block_ok(const fv_ctx *ctx, const EmisBlock &b)
{
    return b.scores && b.n >= 1 && b.ld >= (long long)emis_width(ctx) && b.ld <= (1ll << 59) / b.n && b.dtype >= FV_EMIS_LOG_F32 &&
           b.dtype <= FV_EMIS_LOG_BF16;
}
// bytes of the raw copy of a block the kernel cannot read where it lies (the last row ends at its last score)
inline size_t emis_raw_bytes(const fv_ctx *ctx, const EmisBlock &b) { return ((size_t)(b.n - 1) * (size_t)b.ld + emis_width(ctx)) * emis_elem_size[b.dtype]; }
// where a caller's block lies; a pointer the runtime does not know (plain malloc) makes the query fail: host memory
struct PointerPlace { bool on_device; int device; };
PointerPlace pointer_place(const void *p);
// raw != NULL: the block is copied there first (emis_raw_bytes of the caller's, kept until the stream has drained); then
// reset_flags(), the caller's way of resetting the two words it owns; then the staging launch into E32 / E64, the value rules
// reporting into flags[2].  All on ctx->stream, no sync: reading the words back is the caller's.
template <class Reset>
int stage_block(fv_ctx *ctx, const EmisBlock &b, unsigned char *raw, float *E32, double *E64, unsigned long long *flags, Reset &&reset_flags)
{
    if (raw) FV_HIP(hipMemcpyAsync(raw, b.scores, emis_raw_bytes(ctx, b), hipMemcpyDefault, ctx->stream));
    if (int rc = reset_flags()) return rc;
    return launch_stage_emissions(ctx, raw ? raw : b.scores, b.dtype, b.ld, b.n, E32, E64, flags);
}
// refuses the score at staged index `where` (row * K + state, rows counted from time t_base) in who's name: FV_ERR_ARG
int emis_refusal(fv_ctx *ctx, const char *who, unsigned long long where, long long t_base);
// decode prologue: observation sequence to the device (through the pinned block), counters and answers cleared
int begin_decode(fv_ctx *ctx, const int *ob, int T);
// big-LDS attributes of the kernels each translation unit owns
int full_setup(fv_ctx *ctx);
int beam_setup(fv_ctx *ctx);
int sumprod_setup(fv_ctx *ctx);
// fvk::init_rows lives with the full-state kernels; the beam driver starts its passes from the same rows
int launch_init_rows(fv_ctx *ctx, const fvk::PassChunk &ch, float *rows);
// What a stream (fv_stream.hip) takes from the full-state path, whose kernels live in fv_full.hip.
// stream_admit: the kernel fv_decode_full would run this model on under the options in force, refused as there.
int stream_admit(fv_ctx *ctx, int &kernel);
// time 0 from Pi: the init row, with the emission term lb64[sym[0] * K + i] (sym on the device)
int stream_init_row(fv_ctx *ctx, const double *lb64, const int *sym, float *row);
// one single-task step launch, the form the whole-sequence pass of a one-shot decode takes
int stream_step(fv_ctx *ctx, int kernel, const float *t1_in, float *t1_out, const float *tmp_row, const double *tmp64_row,
                int *bp_out, int reverse);
// A set's lock-step (fv_streams_*): one step launch of nb <= stream_batch_cap tasks, each on rows and emission rows of its
// own slot — the form a batch decode's step launches take (fv_decode_full_batch), bit for bit the single-task launches.
// stream_batch_cap: tasks per launch the generation policy allows this kernel under the FV_OPT_MAX_BATCH in force.
struct StreamTask { const float *t1_in; float *t1_out; const float *tmp_row; const double *tmp64_row; int *bp_out; };
int stream_step_batch(fv_ctx *ctx, int kernel, const StreamTask *tasks, int nb, int reverse);
int stream_batch_cap(const fv_ctx *ctx, int kernel);
// the end pick on `row` into *end / *score, and the back-track of local times 0 .. R from path[R] through the arg rows
// (row j of `bp`: local time j; row 0 is never read) into path[0 .. R-1]
int stream_end_pick(fv_ctx *ctx, const float *row, int *end, float *score);
int stream_backtrack(fv_ctx *ctx, const int *bp, int R, int *path, unsigned long long *restarts);
// what a filter kernel answers to input beyond [0,1] / above 0 (the one-shot decodes' admission and a stream's score push)
constexpr const char *FILTER_RANGE_DETAIL = "the filter+refine kernels need every model entry in [0,1] (and every staged emission score <= 0)";
constexpr const char *CSR_FILTER_RANGE_DETAIL =
    "fv_set_model_sparse: the walk over the stored entries is a filter kernel and needs every model entry in [0,1] "
    "(and every staged emission score <= 0); FV_KERNEL_CSR_F64 decodes such input";
inline const char *filter_range_detail(const fv_ctx *ctx) { return ctx->csr ? CSR_FILTER_RANGE_DETAIL : FILTER_RANGE_DETAIL; }
// frees an open stream's buffers, and an open set's (fv_destroy, close, abort, fv_streams_end)
void stream_drop(fv_ctx *ctx);
// fv_comm.hip
// Multi-device context: one host thread per member runs the same decode on its own device (whole-sequence pass + the
// segments the member owns), the members meet in ONE gather of their answer arrays.
struct fv_group_barrier {
    std::mutex mu;
    std::condition_variable cv;
    int n = 1, waiting = 0;
    unsigned generation = 0;
    bool failed = false;
    bool arrive_and_wait();              // false: a member failed, nobody waits any longer
    void fail();
    void reset(int members);
};
inline int group_size(const fv_ctx *ctx);
inline fv_ctx *group_member(fv_ctx *ctx, int r);
// runs fn(member, path, score) for every member (member 0 on the calling thread), returns the worst return code and
// member 0's merged path / score
int group_run(fv_ctx *ctx, int T, int *path_out, float *score_out, const std::function<int(fv_ctx *, int *, float *)> &fn);
int gather_answers(fv_ctx *ctx, int T);      // ncclAllGather of d_ans (T int32 per rank) into d_gather, on ctx->stream
void merge_gathered(const fv::Plan &plan, const std::vector<int> &gathered, int T, int nranks, int *path);

}  // namespace fvi

struct fv_group {
    std::vector<fv_ctx *> members;       // members[0]: the context the caller holds
    bool rccl = false;                   // distinct devices: the members carry the communicators of one ncclCommInitAll;
                                         // else (a device listed more than once) the gather is device-to-device copies
    fvi::fv_group_barrier barrier;
    std::vector<hipEvent_t> ans_ready;   // per member: its answer array is final (copy gather)
};

namespace fvi {
inline int group_size(const fv_ctx *ctx) { return ctx->group ? (int)ctx->group->members.size() : 1; }
inline fv_ctx *group_member(fv_ctx *ctx, int r) { return ctx->group ? ctx->group->members[(size_t)r] : ctx; }
}  // namespace fvi
