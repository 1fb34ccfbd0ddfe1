// fv_beam.hip — the FLASH-BS (dynamic beam) path of libflashvit.so: fv_decode_beam and its generation driver.
#include "fv_internal.h"
#include "fv_device_common.h"
#include "fv_beam_kernels.hip.inc"
#include "flashvit_testing.h"

namespace {
int decode_beam_impl(fv_ctx *ctx, const int *ob, int T, int n_split, int beam_width, int mode, int *path_out, float *score_out);
int decode_beam_batch_impl(fv_ctx *ctx, const int *ob, const long long *offsets, int nseq, int n_split, int beam_width, int mode,
                           int *path_out, float *score_out, int *status_out);

// row pitch of the row-major float64 table the beam kernels gather from
inline int beam_ld(int K) { return (K + fvb::BEAM_COLS - 1) / fvb::BEAM_COLS * fvb::BEAM_COLS; }
inline int beam_ldq(int K) { static_assert(fvb::BEAMQ_COLS == 128, "fv_ldq"); return fv_ldq(K); }   // ... of the 16-bit one

// Streams generation g (np passes) of a decode of nseq sequences is dealt to: pass i of the length-sorted list goes to
// group i % n.  FV_OPT_DEBUG bits 16 / 17 force one stream / the groups.
// A generation of one sequence's passes: only for big steps (cfg5: 64 M cells per pass and step) — once the auxiliary
// queues have carried work, every dispatch on the main stream takes ~2 us longer (measured, also with the main stream at
// high priority) — 1 ms over the whole-sequence pass of cfg4, more than the overlap returns there.
// Generation 0 of fv_decode_beam_batch: np whole-sequence passes in lock-step.  A select launch lasts as long as its slowest
// workgroup, and a workgroup that meets a reach event replays heaps for tens of microseconds: on one stream every pass
// of the lock-step waits behind it, dealt to the stream groups only the passes of its group do — at the price of that
// dispatch overhead.  DESIGN.md 5.4b has both forms' numbers; FV_OPT_DEBUG bit 29 selects the form that is not the default.
constexpr bool BATCH_GEN0_DEALT = true;
int gen_groups(const fv_ctx *ctx, size_t g, int np, int beam, int nseq)
{
    if ((ctx->opt_debug & FV_DBG_BEAM_ONE_STREAM) || np < 2) return 1;
    const bool dealt = (g == 0 && nseq > 1) ? BATCH_GEN0_DEALT != !!(ctx->opt_debug & FV_DBG_BEAM_BATCH_GEN0_OTHER)
                                            : (double)beam * ctx->K >= 16e6;
    return (dealt || (ctx->opt_debug & FV_DBG_BEAM_GROUPS)) ? std::min(1 + fv_ctx::BEAM_AUX, np) : 1;
}

// The arguments every job of a step launch shares; the caller sets n and fills p[0 .. n) with beam_step_job.
fvb::BeamStepArgs beam_step_args(const fv_ctx *ctx, int beam, int cand_cap)
{
    const int K = ctx->K;
    fvb::BeamStepArgs a;
    a.LA64R = ctx->LA64R.p; a.tie_count = ctx->d_tie_count.p; a.tie_list = ctx->d_tie_list.p;
    a.tie_cap = (unsigned int)ctx->d_tie_list.n;
    a.counters = ctx->d_counters.p;
    a.K = K; a.ld = beam_ld(K); a.ldq = beam_ldq(K); a.beam = beam;
    a.LAQ16R = ctx->LAQ16R.p; a.qpar = ctx->beam_q16_ready ? reinterpret_cast<const float *>(ctx->d_qaux.p + 2) : nullptr;
    a.cand = ctx->d_cand.p; a.cand_count = ctx->d_cand_count.p; a.cand_cap = cand_cap;
    a.n = 0;
    return a;
}
// One job: from the members and the cut at index `in` of the per-step buffers, consuming symbol sym, the records of step
// j at index j (a decode: in = j - 1; fv_test_beam_step: in = j, the caller's slot sets).
fvb::BeamSlot beam_step_job(const fv_ctx *ctx, int beam, int j, int in, int sym)
{
    const size_t K = (size_t)ctx->K, BP = (size_t)fvb::beam_pitch(beam);
    fvb::BeamSlot p;
    p.sval = ctx->d_hval.p + in * BP;
    p.sstate = ctx->d_hstate.p + in * BP;
    p.doubt = ctx->d_doubt.p + (size_t)j * fvb::DOUBT_CAP;
    p.doubt_count = ctx->d_doubt_count.p + j;
    p.scores = ctx->d_scores.p + j * K;
    p.bp_row = ctx->d_bp.p + j * K;
    p.tmp_row = ctx->view.lb32 + sym * K;
    p.j = j;
    p.cut = ctx->d_cut.p + (size_t)in * fvb::CUT_W;
    p.dupwin = ctx->d_dupwin.p + j;
    return p;
}

// The step kernel of one beam launch: the one rule beam_forward and fv_test_beam_step share.
int launch_beam_step(fv_ctx *ctx, const fvb::BeamStepArgs &a, hipStream_t st)
{
    const int K = ctx->K, beam = a.beam;
    auto record = [&](unsigned long long bit) { if (ctx->test_record) ctx->test_variants |= bit; };
    if (ctx->csr) {
        // A model set by fv_set_model_sparse (the entry points let it through under FV_OPT_SPARSE_BEAM only): no row to
        // gather — the list's entries scatter their CSR rows into the accumulators, then one K-wide finish.
        record(FV_TV_BEAM_CSR);
        fvb::BeamCsrArgs ca;
        ca.a = a;
        ca.m.ptr = ctx->CRptr.p; ca.m.col = ctx->CRcol.p; ca.m.log = ctx->CRlog.p;
        ca.acc = ctx->d_csr_acc.p; ca.tieval = ctx->d_csr_tie.p;
        const int groups = (fvb::beam_pitch(beam) + fvb::CSR_SCATTER_WAVES - 1) / fvb::CSR_SCATTER_WAVES;
        hipLaunchKernelGGL(fvb::beam_scatter_csr, dim3(groups, a.n), dim3(fvb::CSR_SCATTER_WAVES * 64), 0, st, ca);
        hipLaunchKernelGGL(fvb::beam_finish_csr, dim3((K + fvb::CSR_FINISH_BLOCK - 1) / fvb::CSR_FINISH_BLOCK, a.n),
                           dim3(fvb::CSR_FINISH_BLOCK), 0, st, ca);
        FV_HIP(hipGetLastError());
        return 0;
    }
    // The 16-bit filter kernel moves a quarter of the bytes but has two more dependent phases (window,
    // float64 refine): measured at K = 16384, B = 256 it takes 13.7 us + 2.6 us per extra pass of the
    // launch against 10.6 + 5.0 for the float64 kernel, so it is used from ~80 MB of float64 rows per
    // launch on (cfg5: 537 MB per pass).  FV_OPT_DEBUG bit 8: never, bit 9: always.
    // (emission scores above 0, fv_set_emissions: the float64 kernel, as for a model with an entry above 1)
    const bool use_q16 = ctx->beam_q16_ready && ctx->view.logs_nonpositive && !(ctx->opt_debug & FV_DBG_BEAM_F64) &&
                         ((ctx->opt_debug & FV_DBG_BEAM_Q16) || (double)a.n * beam * K * 8.0 >= 80e6);
    // 8-wave workgroups once the launch has more 16-wave workgroups than fit the chip together (two per CU);
    // FV_OPT_DEBUG bit 25: never, bit 26: always
    const int panels = beam_ldq(K) / fvb::BEAMQ_COLS;
    const bool narrow = !(ctx->opt_debug & FV_DBG_BEAM_WIDE) &&
                        ((ctx->opt_debug & FV_DBG_BEAM_NARROW) || (long long)panels * a.n > 2LL * ctx->num_cus);
    // (4-wave workgroups for launches beyond four 8-wave workgroups per CU: cfg4 right-hand 3.51 -> 3.56 ms, cfg5 95.8 -> 97.1)
    if (use_q16 && narrow) {
        record(FV_TV_BEAM_Q16_W8);
        hipLaunchKernelGGL(fvb::beam_step_q16<8>, dim3(panels, a.n), dim3(8 * 64), fvb::beam_step_q16_lds(beam, 8), st, a);
    } else if (use_q16) {
        record(FV_TV_BEAM_Q16_W16);
        hipLaunchKernelGGL(fvb::beam_step_q16<16>, dim3(panels, a.n), dim3(fvb::BEAM_BLOCK),
                           fvb::beam_step_q16_lds(beam), st, a);
    // (small beams: four waves per workgroup — K = 3965, B = 32: 4.55 -> 4.23 ms; eight waves at B = 256: 6.43 -> 6.50, not kept)
    } else if (beam <= 64 && !(ctx->opt_debug & FV_DBG_BEAM_WIDE)) {
        record(FV_TV_BEAM_W4);
        hipLaunchKernelGGL(fvb::beam_step<4>, dim3(beam_ld(K) / fvb::BEAM_COLS, a.n), dim3(4 * 64), fvb::beam_step_lds(beam, 4), st, a);
    } else {
        record(FV_TV_BEAM_W16);
        hipLaunchKernelGGL(fvb::beam_step<16>, dim3(beam_ld(K) / fvb::BEAM_COLS, a.n), dim3(fvb::BEAM_BLOCK), fvb::beam_step_lds(beam),
                           st, a);
    }
    FV_HIP(hipGetLastError());
    return 0;
}

// Capacity of a step's candidate list under the current options (0: no lists).  FV_OPT_DEBUG bit 10: never a list.
inline int beam_cand_cap(const fv_ctx *ctx, int K, int beam) { return (ctx->opt_debug & FV_DBG_NO_CAND_LISTS) ? 0 : fvb::cand_cap_for(K, beam); }

// FV_TS_* bit of a select-kernel instantiation (test hooks only)
unsigned long long select_variant(fvb::SelKernel k)
{
    const struct { fvb::SelKernel k; unsigned long long bit; } tab[] = {
        { fvb::topb_select<4, true>, FV_TS_SEL4_LISTED }, { fvb::topb_select<4, false>, FV_TS_SEL4_DERIVED },
        { fvb::topb_select<16, true>, FV_TS_SEL16_LISTED }, { fvb::topb_select<16, false>, FV_TS_SEL16_DERIVED },
        { fvb::topb_select<fvb::SEL_MAX_ROUNDS, true>, FV_TS_SEL64_LISTED }, { fvb::topb_select<fvb::SEL_MAX_ROUNDS, false>, FV_TS_SEL64_DERIVED },
        { fvb::topb_select_cand<8, true>, FV_TS_CAND8_LISTED }, { fvb::topb_select_cand<8, false>, FV_TS_CAND8_DERIVED },
        { fvb::topb_select_cand<16, true>, FV_TS_CAND16_LISTED }, { fvb::topb_select_cand<16, false>, FV_TS_CAND16_DERIVED },
        // (the CSR instantiations differ in the resolve code only: same bits)
        { fvb::topb_select<4, true, true>, FV_TS_SEL4_LISTED }, { fvb::topb_select<4, false, true>, FV_TS_SEL4_DERIVED },
        { fvb::topb_select<16, true, true>, FV_TS_SEL16_LISTED }, { fvb::topb_select<16, false, true>, FV_TS_SEL16_DERIVED },
        { fvb::topb_select<fvb::SEL_MAX_ROUNDS, true, true>, FV_TS_SEL64_LISTED }, { fvb::topb_select<fvb::SEL_MAX_ROUNDS, false, true>, FV_TS_SEL64_DERIVED },
        { fvb::topb_select_cand<8, true, true>, FV_TS_CAND8_LISTED }, { fvb::topb_select_cand<8, false, true>, FV_TS_CAND8_DERIVED },
        { fvb::topb_select_cand<16, true, true>, FV_TS_CAND16_LISTED }, { fvb::topb_select_cand<16, false, true>, FV_TS_CAND16_DERIVED } };
    for (const auto &e : tab) if (e.k == k) return e.bit;
    return 0;
}

// The select of one lock-step — the members of the heaps of `count` passes at lock-step s, one launch: the one rule
// beam_forward and fv_test_beam_select share.  K: states per score row; T: entries of the per-step buffers (which are
// the context's, indexed by absolute time); rcx.b.passL is ignored: passL[q] (device) and first_of(q) (host) both give the
// first position of pass q of the launch.
template <class FirstOf>
int launch_beam_select(fv_ctx *ctx, int K, int beam, int T, const fvb::ResolveCtx &rcx, const int *passL, int count, int s,
                       FirstOf &&first_of, hipStream_t st)
{
    const int cand_cap = beam_cand_cap(ctx, K, beam), BP = fvb::beam_pitch(beam);
    fvb::SelArgs a;
    a.counters = ctx->d_counters.p; a.K = K; a.beam = beam; a.s = s;
    a.no_wave = (ctx->opt_debug & FV_DBG_SELECT_WHOLE_GROUP) ? 1 : 0;
    a.eager = (ctx->opt_debug & FV_DBG_EAGER_REPLAY) ? 1 : 0;
    a.quad_dirty = (ctx->opt_debug & FV_DBG_SELECT4_DIRTY) ? 1 : 0;
    a.sb_rounds = (ctx->opt_debug & FV_DBG_SELECT_IN_MEMORY) ? 2 : fvb::SEL_MAX_ROUNDS;
    a.T = T; a.own_pred = (ctx->opt_debug & FV_DBG_OWN_CUTS) ? 1 : 0;
    a.margin = ctx->opt_sel_margin; a.cand_cap = cand_cap;
    a.cand = ctx->d_cand.p; a.cand_count = ctx->d_cand_count.p; a.rc = rcx;
    a.rc.b.passL = passL;
    const bool listed = count <= fvb::BEAM_CHUNK;
    for (int q = 0; listed && q < count; ++q) {
        const int L = first_of(q), j = L + s;
        a.p[q] = fvb::SelJob{ ctx->d_scores.p + (size_t)j * K, ctx->d_hval.p + (size_t)j * BP, ctx->d_hstate.p + (size_t)j * BP,
                              ctx->d_cut.p + (size_t)j * fvb::CUT_W, s >= 1 ? ctx->d_cut.p + (size_t)(j - 1) * fvb::CUT_W : nullptr,
                              (cand_cap && s >= 1) ? ctx->d_cand.p + (size_t)j * cand_cap : nullptr, ctx->d_cand_count.p + j,
                              j, L };
    }
    // steps >= 2 of a pass have a candidate list (the predictor needs two cut values)
    // K > 65536 (FV_OPT_DEBUG bit 22: any K): beyond the 64 rounds the register kernels hold, every selection runs in the
    // lean kernel — on the candidate list where there is one, otherwise over the K scores in memory
    const bool many = K > fvb::SEL_MAX_ROUNDS * fvb::SEL_BLOCK || (ctx->opt_debug & FV_DBG_SELECT_IN_MEMORY);
    const bool csr = rcx.csr.ptr != nullptr;        // a sparse-set model's decode: the instantiations that resolve on its rows
    fvb::SelKernel lean = (s >= 2 || many) ? fvb::sel_cand_kernel_for(K, cand_cap, listed, many, csr) : nullptr;
    const fvb::SelKernel kernel = lean ? lean : fvb::sel_kernel_for(K, listed, csr);
    if (ctx->test_record) ctx->test_selects |= select_variant(kernel);
    hipLaunchKernelGGL(kernel, dim3(count), dim3(fvb::SEL_BLOCK), fvb::sel_lds(beam), st, a);
    FV_HIP(hipGetLastError());
    return 0;
}

// What the resolve code works on, over K states per score row and the passes whose first positions passL (device) lists.
// model = false (fv_test_beam_select, which takes K as an argument and needs no model): what only the resolve code reads
// stays null — no row of the hook is a dirty step.
fvb::ResolveCtx resolve_ctx(const fv_ctx *ctx, int K, int beam, const int *passL, bool model)
{
    fvb::ResolveCtx r;
    r.counters = ctx->d_counters.p; r.K = K; r.beam = beam; r.ld = beam_ld(K);
    r.no_cut = (model && (ctx->opt_debug & FV_DBG_DECIDE_IN_FULL)) ? 1 : 0;
    r.LA64R = model ? ctx->LA64R.p : nullptr; r.LB32T = model ? ctx->view.lb32 : nullptr; r.ob = model ? ctx->d_ob.p : nullptr;
    r.bp = model ? ctx->d_bp.p : nullptr; r.doubt = model ? ctx->d_doubt.p : nullptr; r.doubt_count = ctx->d_doubt_count.p;
    r.b.scores_all = ctx->d_scores.p; r.b.hval = ctx->d_hval.p; r.b.hstate = ctx->d_hstate.p;
    r.b.cut = ctx->d_cut.p; r.b.passL = passL;
    if (model && ctx->csr) { r.csr.ptr = ctx->CRptr.p; r.csr.col = ctx->CRcol.p; r.csr.log = ctx->CRlog.p; }
    return r;
}

// The arguments of a heap_build_all launch but its ranges: the caller appends them to p[0 .. n).
fvb::HeapAllArgs heap_all_args(const fv_ctx *ctx, int K, int beam, const int *gate, const int *seq_of)
{
    fvb::HeapAllArgs h;
    h.scores_all = ctx->d_scores.p; h.slot_val = ctx->d_slot_val.p; h.slot_state = ctx->d_slot_state.p;
    h.err_counter = ctx->d_counters.p + fvk::CNT_HANDSHAKE_TIMEOUT; h.gate = gate; h.seq_of = seq_of;
    h.K = K; h.beam = beam; h.n = 0;
    return h;
}

// One generation of beam passes in flight (same shape as run_generation_full): what its forward part and its pass ends
// work on.  Buffers are indexed by absolute time j (passes of one generation cover disjoint time ranges): scores_all[j] =
// the K scores after consuming ob[j] (j = L: the init row), set_*[j] = the members of the heap built from them
// (order-free), slot_*[j] = its exact array layout (rebuilt after the lock-step loop).
struct BeamGen {
    const std::vector<fv::Pass> &passes;    // group by group (run_beam_generations), longest first inside a group;
                                            // rcx.b.passL: their first positions on the device, in the same order
    int beam, T, ng;                        // T: length of the time axis (a batch: all sequences end to end); ng: stream groups
    int nseq; const int *seq_of;            // the tie gates are per sequence (seq_of: fv_decode_beam_batch's time -> sequence map on the device)
    fvb::ResolveCtx rcx;
    std::vector<fvb::BeamEnd> ends;         // the passes as the pass-end kernels take them, sliced per launch
};

// Forward part of a generation: init rows, then every stream group's passes in lock-step (step, select).
int beam_forward(fv_ctx *ctx, const BeamGen &gen)
{
    const std::vector<fv::Pass> &passes = gen.passes;
    const int K = ctx->K, np = (int)passes.size(), beam = gen.beam, ng = gen.ng;
    FV_HIP(hipMemsetAsync(ctx->d_tie_count.p, 0, sizeof(unsigned int), ctx->stream));
    FV_HIP(hipMemsetAsync(ctx->d_doubt_count.p, 0, (size_t)gen.T * sizeof(int), ctx->stream));      // doubtful-column lists of this generation
    // members of the heaps of passes [first, first + count) at lock-step s: one launch
    auto select = [&](int first, int count, int s, hipStream_t st) -> int {
        return launch_beam_select(ctx, K, beam, gen.T, gen.rcx, gen.rcx.b.passL + first, count, s,
                                  [&](int q) { return passes[first + q].L; }, st);
    };
    // init scores (the same rows the full variant starts from, FLASH_BS:407-427)
    int rc0 = 0;
    for (int base = 0; base < np; base += fvk::PASS_CHUNK) {
        fvk::PassChunk ch;
        ch.n = std::min(fvk::PASS_CHUNK, np - base);
        for (int q = 0; q < ch.n; ++q) {
            const fv::Pass &p = passes[base + q];
            ch.p[q] = fvk::PassDesc{ p.L, p.R, p.from_pi ? 1 : 0, p.whole ? 1 : 0, (long long)p.L * K };
        }
        if ((rc0 = fvi::launch_init_rows(ctx, ch, ctx->d_scores.p))) return rc0;
    }
    // Every group runs its passes in lock-step on its own stream: first heaps' members, then step + select per position.
    // A select launch lasts as long as its slowest exact replay and keeps one CU per pass busy; the step kernels of
    // the other groups fill the rest of the chip meanwhile.
    if (ng > 1) FV_HIP(hipEventRecord(ctx->ev_fork, ctx->stream));
    int rc = 0;
    fvb::BeamStepArgs a = beam_step_args(ctx, beam, beam_cand_cap(ctx, K, beam));
    for (int g = 0, first = 0; g < ng; ++g) {
        const int gn = (np - g + ng - 1) / ng;                 // passes g, g + ng, ... of the sorted list
        hipStream_t st = g == 0 ? ctx->stream : ctx->aux[g - 1];
        if (g > 0) FV_HIP(hipStreamWaitEvent(st, ctx->ev_fork, 0));
        if ((rc = select(first, gn, 0, st))) return rc;
        const int maxlen = passes[first].R - passes[first].L;
        int active = gn;
        for (int s = 1; s <= maxlen; ++s) {
            while (active > 0 && passes[first + active - 1].R - passes[first + active - 1].L < s) --active;
            for (int base = 0; base < active; base += fvb::BEAM_CHUNK) {
                a.n = std::min(fvb::BEAM_CHUNK, active - base);
                for (int q = 0; q < a.n; ++q) {
                    const int j = passes[first + base + q].L + s;
                    a.p[q] = beam_step_job(ctx, beam, j, j - 1, ctx->h_ob[j]);
                }
                if ((rc = launch_beam_step(ctx, a, st))) return rc;
                ctx->stats.step_launches += 1;
                ctx->stats.task_steps += a.n;
            }
            if ((rc = select(first, active, s, st))) return rc;
        }
        if (g > 0) {
            FV_HIP(hipEventRecord(ctx->ev_join[g - 1], st));
            FV_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_join[g - 1], 0));
        }
        first += gn;
    }
    return 0;
}

// Pass ends of a generation.  First attempt on the provisional back-pointers (beam_end_backtrack); only the
// whole-sequence pass needs a layout for that — its last heap's.  The exact layouts of every step's heap and the tie
// fix-up are queued behind it but run only if the walk met a tied cell (FV_OPT_DEBUG bit 19: always).
int beam_pass_ends(fv_ctx *ctx, const BeamGen &gen)
{
    const int K = ctx->K, np = (int)gen.ends.size(), beam = gen.beam;
    int *const needfull = ctx->d_needfull.p;
    FV_HIP(hipMemsetAsync(needfull, 0, (size_t)gen.nseq * sizeof(int), ctx->stream));
    auto layouts = [&](bool last_only, const int *gate) -> int {
        for (int base = 0; base < np; base += fvb::HEAP_CHUNK) {
            fvb::HeapAllArgs h = heap_all_args(ctx, K, beam, gate, gen.seq_of);
            int longest = 0;
            for (int q = 0; q < std::min(fvb::HEAP_CHUNK, np - base); ++q) {
                const fvb::BeamEnd &p = gen.ends[(size_t)(base + q)];
                if (last_only && !p.whole) continue;
                h.p[h.n++] = fvb::HeapRange{ last_only ? p.R : p.L, p.R };
                longest = std::max(longest, last_only ? 1 : p.R - p.L + 1);
            }
            if (h.n == 0) continue;
            hipLaunchKernelGGL(fvb::heap_build_all, dim3(longest, h.n), dim3(128), fvb::heap_lds(beam), ctx->stream, h);
            FV_HIP(hipGetLastError());
        }
        return 0;
    };
    auto ends = [&](int lazy_walk) -> int {
        for (int base = 0; base < np; base += fvb::BEAM_CHUNK) {
            fvb::BeamEndArgs e;
            e.K = K; e.beam = beam; e.n = std::min(fvb::BEAM_CHUNK, np - base);
            e.lazy = lazy_walk; e.flag = needfull; e.restarts = ctx->d_counters.p + fvk::BT_COUNTER;
            std::copy_n(gen.ends.data() + base, e.n, e.p);
            hipLaunchKernelGGL(fvb::beam_end_backtrack, dim3(e.n), dim3(64), 0, ctx->stream, e, ctx->d_slot_val.p,
                               ctx->d_slot_state.p, ctx->d_hstate.p, ctx->d_cut.p, ctx->d_bp.p, ctx->d_ans.p, ctx->d_score.p);
            FV_HIP(hipGetLastError());
        }
        return 0;
    };
    // Undecided duplicate steps (lazy replays, fv_beam_kernels.hip.inc): mode 0 decides what the pass ends themselves read,
    // mode 1 — behind the same gate as the layouts — everything, because heap_build_all replays every step's exact scores.
    auto resolve = [&](int mode, const int *gate) -> int {
        for (int base = 0; base < np; base += fvb::BEAM_CHUNK) {
            fvb::ResolveArgs r;
            r.rc = gen.rcx; r.mode = mode; r.gate = gate; r.ans = ctx->d_ans.p;
            r.n = std::min(fvb::BEAM_CHUNK, np - base);
            std::copy_n(gen.ends.data() + base, r.n, r.p);
            hipLaunchKernelGGL(ctx->csr ? fvb::beam_resolve<true> : fvb::beam_resolve<false>, dim3(r.n), dim3(fvb::RESOLVE_BLOCK),
                               fvb::heap_lds(beam), ctx->stream, r);
            FV_HIP(hipGetLastError());
        }
        return 0;
    };
    int rc = 0;
    if ((rc = resolve(0, nullptr))) return rc;
    if (!(ctx->opt_debug & FV_DBG_ALL_LAYOUTS)) {
        if ((rc = layouts(true, nullptr))) return rc;
        if ((rc = ends(1))) return rc;
    } else {
        FV_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(needfull), 1, (size_t)gen.nseq, ctx->stream));    // every flag up
    }
    if ((rc = resolve(1, needfull))) return rc;
    if ((rc = layouts(false, needfull))) return rc;
    {
        fvb::FixArgs f;
        f.LA64R = ctx->LA64R.p; f.LB32T = ctx->view.lb32; f.ob = ctx->d_ob.p;
        f.tie_count = ctx->d_tie_count.p; f.tie_list = ctx->d_tie_list.p; f.tie_cap = (unsigned int)ctx->d_tie_list.n;
        f.slot_val = ctx->d_slot_val.p; f.slot_state = ctx->d_slot_state.p; f.bp = ctx->d_bp.p;
        f.K = K; f.ld = beam_ld(K); f.beam = beam; f.total = ctx->d_counters.p + fvk::CNT_BEAM_TIES; f.gate = needfull;
        f.seq_of = gen.seq_of; f.csr = gen.rcx.csr;
        hipLaunchKernelGGL(ctx->csr ? fvb::tie_fixup<true> : fvb::tie_fixup<false>, dim3(512), dim3(256), 0, ctx->stream, f);
        FV_HIP(hipGetLastError());
    }
    return ends(0);
}

}  // namespace

extern "C" int fv_decode_beam(fv_ctx *ctx, const int *ob, int T, int n_split, int beam_width, int mode,
                              int *path_out, float *score_out)
{
    if (!ctx) return FV_ERR_ARG;
    FV_NO_STREAM(ctx);
    if (ctx->csr && !ctx->opt_sparse_beam) { ctx->detail = "fv_decode_beam: not available on a model set by fv_set_model_sparse (the beam kernels gather dense rows)"; return FV_ERR_UNSUPPORTED; }
    if (ctx->group && ctx->group_rank == 0) {
        if (!path_out || T < 2) return FV_ERR_ARG;
        return fvi::group_run(ctx, T, path_out, score_out, [&](fv_ctx *m, int *path, float *score) {
            return fvi::drained(m, decode_beam_impl(m, ob, T, n_split, beam_width, mode, path, score));
        });
    }
    return fvi::drained(ctx, decode_beam_impl(ctx, ob, T, n_split, beam_width, mode, path_out, score_out));
}

namespace {
// Beam widths the beam path takes over K states: the admission fv_decode_beam and the test hooks share.
int beam_admit_k(int K, int beam)
{
    // beam > K reads uninitialised heap slots in the reference
    if (beam < 2 || beam > K) return FV_ERR_ARG;
    if (fvb::beam_step_lds(beam) > fvk::BEAM_LDS_LIMIT || fvb::beam_step_q16_lds(beam) > fvk::BEAM_LDS_LIMIT ||
        fvb::heap_lds(beam) > fvk::BEAM_LDS_LIMIT) return FV_ERR_UNSUPPORTED;
    return 0;
}
int beam_admit(fv_ctx *ctx, int beam) { return beam_admit_k(ctx->K, beam); }

// The row-major tables of the beam step kernels (float64 LA64R, 16-bit LAQ16R and its parameters qpar), built on the
// device by the first beam decode or test-hook call of a model.
int beam_tables(fv_ctx *ctx)
{
    if (ctx->csr) return 0;          // FV_OPT_SPARSE_BEAM: the kernels read the rows fv_set_model_sparse uploaded; nothing to build
    if (!ctx->LA64R.p) {
        const int ld = beam_ld(ctx->K);
        FV_HIP(ctx->LA64R.ensure((size_t)ctx->K * ld));
        hipLaunchKernelGGL(fvb::relayout_rows, dim3(2048), dim3(256), 0, ctx->stream, ctx->LA64.p, ctx->LA64R.p, ctx->K, ctx->nrows, ld);
        FV_HIP(hipGetLastError());
    }
    if (!ctx->beam_q16_ready && ctx->logs_nonpositive) {
        // filter table of beam_step_q16, quantised on the device from LA64R
        const int ld = beam_ld(ctx->K), ldq = beam_ldq(ctx->K);
        FV_HIP(ctx->LAQ16R.ensure((size_t)ctx->K * ldq));
        FV_HIP(ctx->d_qaux.ensure(3));
        FV_HIP(hipMemsetAsync(ctx->d_qaux.p, 0, 3 * sizeof(unsigned long long), ctx->stream));
        hipLaunchKernelGGL(fvk::q16_range, dim3(2048), dim3(256), 0, ctx->stream, ctx->LA64R.p, (size_t)ctx->K * ld, ctx->d_qaux.p);
        hipLaunchKernelGGL(fvb::q16_rows, dim3(2048), dim3(256), 0, ctx->stream, ctx->LA64R.p, ctx->LAQ16R.p, ctx->K, ld, ldq,
                           ctx->d_qaux.p, ctx->d_qaux.p + 1);
        hipLaunchKernelGGL(fvb::q16_params, dim3(1), dim3(1), 0, ctx->stream, ctx->d_qaux.p, ctx->d_qaux.p + 1,
                           reinterpret_cast<float *>(ctx->d_qaux.p + 2));
        FV_HIP(hipGetLastError());
        ctx->beam_q16_ready = true; ctx->rowq_ready = true;
    }
    return 0;
}

// The workspace of a beam decode over T observations (a batch: all sequences end to end): the per-step buffers, indexed
// by absolute time, on top of what every decode needs.  nseq > 0 (fv_decode_beam_batch): the whole request is first added
// up in 64 bits and compared with the free device memory plus what growing a buffer releases, before anything is allocated.
int beam_workspace(fv_ctx *ctx, int T, int beam, int nseq)
{
    const size_t K = (size_t)ctx->K, BP = (size_t)fvb::beam_pitch(beam), cap = (size_t)fvb::cand_cap_for(ctx->K, beam), t = (size_t)T;
    fvi::Wants w;
    w.add(ctx->d_scores, t * K); w.add(ctx->d_hval, t * BP); w.add(ctx->d_hstate, t * BP);
    w.add(ctx->d_doubt, t * fvb::DOUBT_CAP); w.add(ctx->d_doubt_count, t);
    w.add(ctx->d_slot_val, t * beam); w.add(ctx->d_slot_state, t * beam);
    w.add(ctx->d_tie_list, t * K); w.add(ctx->d_tie_count, (size_t)4);
    w.add(ctx->d_cut, t * fvb::CUT_W); w.add(ctx->d_cand_count, t);
    if (cap) w.add(ctx->d_cand, t * cap);
    w.add(ctx->d_dupwin, t); w.add(ctx->d_needfull, (size_t)std::max(4, nseq));
    // a sparse-set model (FV_OPT_SPARSE_BEAM): the scatter accumulators, 12 bytes per (observation, state)
    if (ctx->csr) { w.add(ctx->d_csr_acc, t * K); w.add(ctx->d_csr_tie, t * K); }
    if (nseq > 0) {
        w.add(ctx->d_seqof, t);
        w.what = "beam batch workspace";
        w.dominant = ctx->csr ? "score rows, back-pointers, tie list and scatter accumulators: " + std::to_string(28ull * t * K)
                              : "score rows, back-pointers and tie list: " + std::to_string(16ull * t * K);
    }
    if (int rc = fvi::ensure_workspace(ctx, T, 1, nseq > 0 ? std::max(nseq, 2) : 1, std::move(w))) return rc;
    if (ctx->csr) {                  // once per decode: beam_finish_csr clears every cell it reads
        FV_HIP(hipMemsetAsync(ctx->d_csr_acc.p, 0, t * K * sizeof(unsigned long long), ctx->stream));
        FV_HIP(hipMemsetAsync(ctx->d_csr_tie.p, 0, t * K * sizeof(unsigned int), ctx->stream));
    }
    FV_HIP(hipMemsetAsync(ctx->d_cut.p, 0xFF, t * fvb::CUT_W * sizeof(float), ctx->stream));      // NaN: no earlier pass has left a cut here
    FV_HIP(hipMemsetAsync(ctx->d_cand_count.p, 0, t * sizeof(int), ctx->stream));
    FV_HIP(hipMemsetAsync(ctx->d_dupwin.p, 0, t * sizeof(int), ctx->stream));
    return 0;
}

// The generations of a beam decode, after begin_decode: pass lists to the device, then generation by generation.
int run_beam_generations(fv_ctx *ctx, std::vector<std::vector<fv::Pass>> &gens, int beam_width, int T, int nseq, const int *seq_of)
{
    int rc = 0;
    // The passes of a generation run in lock-step, longest first (the active ones are a prefix); the kernels find a
    // pass's rows from its first position, so the whole plan's pass lists go to the device once, before the clock starts.
    std::vector<size_t> pass_off(gens.size(), 0);
    std::vector<int> groups(gens.size(), 1);         // stream groups of every generation
    ctx->h_passL.clear();
    for (size_t g = 0; g < gens.size(); ++g) {
        std::stable_sort(gens[g].begin(), gens[g].end(),
                         [](const fv::Pass &a, const fv::Pass &b) { return a.R - a.L > b.R - b.L; });
        {   // group-major: the passes of stream group q (i % ng == q), longest first, then those of group q + 1
            const int np = (int)gens[g].size(), ng = groups[g] = gen_groups(ctx, g, np, beam_width, nseq);
            std::vector<fv::Pass> byg;
            byg.reserve(gens[g].size());
            for (int q = 0; q < ng; ++q)
                for (int i = q; i < np; i += ng) byg.push_back(gens[g][i]);
            gens[g].swap(byg);
        }
        pass_off[g] = ctx->h_passL.size();
        for (const fv::Pass &p : gens[g]) ctx->h_passL.push_back(p.L);
    }
    FV_HIP(ctx->d_passL.ensure(std::max<size_t>(1, ctx->h_passL.size())));
    if (!ctx->h_passL.empty())
        FV_HIP(hipMemcpyAsync(ctx->d_passL.p, ctx->h_passL.data(), ctx->h_passL.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    FV_HIP(hipEventRecord(ctx->ev_start, ctx->stream));
    FV_HIP(hipEventRecord(ctx->ev_s0, ctx->stream));
    for (size_t g = 0; g < gens.size(); ++g) {
        ctx->stats.passes += (int)gens[g].size();
        // Work queued on the auxiliary streams slows every dispatch of the main one while it waits there for its fork
        // event (the command processor keeps re-examining the blocked queues: +2 us per launch, 1 ms over the
        // whole-sequence pass of cfg4).  The host therefore does not run ahead of a serial generation into a forked one.
        if (g > 0 && groups[g] > 1 && groups[g - 1] == 1) FV_HIP(hipStreamSynchronize(ctx->stream));
        if (!gens[g].empty()) {
            BeamGen gen{ gens[g], beam_width, T, groups[g], nseq, seq_of,
                         resolve_ctx(ctx, ctx->K, beam_width, ctx->d_passL.p + pass_off[g], true), {} };
            for (const fv::Pass &p : gens[g]) gen.ends.push_back(fvb::BeamEnd{ p.L, p.R, p.whole ? 1 : 0, p.seq });
            if ((rc = beam_forward(ctx, gen)) || (rc = beam_pass_ends(ctx, gen))) return rc;
        }
        if (g == 0) { FV_HIP(hipEventRecord(ctx->ev_top, ctx->stream)); FV_HIP(hipEventRecord(ctx->ev_s1, ctx->stream)); }
    }
    return 0;
}

// statistics of a beam decode about to start (the float64 rows of the beam's members per step; no density is reported)
void start_beam_stats(fv_ctx *ctx, const fv::Plan &plan, int beam_width)
{
    // (a sparse-set model: the float64 logs of the stored entries; an ESTIMATE — 12 bytes per entry of beam_width average rows)
    if (ctx->csr) ctx->start_stats(FV_KERNEL_CSR_F64, plan.generations(), 12LL * beam_width * ctx->csr_nnz / ctx->K, 0.0);
    else ctx->start_stats(FV_KERNEL_F64_STREAM, plan.generations(), (long long)beam_width * ctx->K * 8, 0.0);
}

// What fv_decode_beam, fv_decode_beam_batch and fv_test_beam_forward do once admitted and planned: workspace, tables,
// statistics, prologue, generations, epilogue.  offsets: the sequences laid end to end — nseq + 1 entries of a batch
// (whose request is checked against the free memory first, whose tie gates are per sequence), { 0, T } and nseq = 0 of a
// single sequence.  after_begin (may be empty): what the caller uploads between the prologue and the generations.
// record: a test hook's call, see FvTestRecording.
int run_beam_decode(fv_ctx *ctx, const int *ob, const fv::Plan &plan, std::vector<std::vector<fv::Pass>> &gens,
                    const long long *offsets, int nseq, int beam_width, int *path_out, float *score_out, int *status_out,
                    clk::time_point t0, const std::function<int()> &after_begin, bool record)
{
    const int T = (int)offsets[std::max(nseq, 1)];
    int rc = 0;
    FV_HIP(hipSetDevice(ctx->device));
    if ((rc = beam_workspace(ctx, T, beam_width, nseq))) return rc;
    if ((rc = beam_tables(ctx))) return rc;
    start_beam_stats(ctx, plan, beam_width);

    if ((rc = fvi::begin_decode(ctx, ob, T))) return rc;
    if (after_begin && (rc = after_begin())) return rc;
    FvTestRecording recording(ctx, record);
    if ((rc = run_beam_generations(ctx, gens, beam_width, T, std::max(nseq, 1), nseq ? ctx->d_seqof.p : nullptr))) return rc;
    ctx->close_stats((long long)ctx->K * beam_width, 0);
    return fvi::finish_decode(ctx, plan, offsets, std::max(nseq, 1), path_out, score_out, status_out, t0, 0, true);
}

int decode_beam_impl(fv_ctx *ctx, const int *ob, int T, int n_split, int beam_width, int mode, int *path_out, float *score_out)
{
    if (!ctx || !path_out || T < 2 || n_split < 1) return FV_ERR_ARG;
    int rc = fvi::emission_view(ctx, ob, T);
    if (rc) return rc;
    if (ctx->K == 0) return FV_ERR_STATE;
    if ((rc = beam_admit(ctx, beam_width))) return rc;
    for (int j = 0; j < T; ++j) if (ob[j] < 0 || ob[j] >= ctx->view.nsym) return FV_ERR_ARG;
    auto t0 = clk::now();
    fv::Plan plan;
    if ((rc = fv::build_plan(T, n_split, mode, ctx->nranks, plan))) return rc;
    std::vector<std::vector<fv::Pass>> gens = fvi::deal_passes(ctx, plan);
    const long long whole[2] = { 0, T };
    return run_beam_decode(ctx, ob, plan, gens, whole, 0, beam_width, path_out, score_out, nullptr, t0, nullptr, false);
}

// fv_decode_beam_batch: the forest plan (fv::build_forest, as fv_decode_full_batch) run by the beam generation driver.
// Every beam buffer is indexed by absolute time, so the passes of different sequences share the lock-step launches as
// the passes of one sequence's right-hand generations do; what is per sequence is the end pick's score and the tie gate.
int decode_beam_batch_impl(fv_ctx *ctx, const int *ob, const long long *offsets, int nseq, int n_split, int beam_width, int mode,
                           int *path_out, float *score_out, int *status_out)
{
    const char *who = "fv_decode_beam_batch";
    std::vector<int> lengths;
    int rc = fvi::batch_lengths(ctx, who, ob, offsets, nseq, n_split, mode, path_out, lengths);
    if (rc || (rc = beam_admit(ctx, beam_width)) || (rc = fvi::batch_symbols(ctx, who, ob, offsets, nseq))) return rc;
    auto t0 = clk::now();
    const int sumT = (int)offsets[nseq];
    fv::Plan plan;
    if ((rc = fvi::batch_plan(ctx, who, lengths, n_split, mode, plan))) return rc;
    std::vector<std::vector<fv::Pass>> gens = fvi::deal_passes(ctx, plan);
    // time -> sequence: how heap_build_all and tie_fixup find the gate of a step (4 bytes per observation)
    auto upload_seq_of = [&]() -> int {
        ctx->h_seqof.resize((size_t)sumT);
        for (int s = 0; s < nseq; ++s) std::fill(ctx->h_seqof.begin() + offsets[s], ctx->h_seqof.begin() + offsets[s + 1], s);
        FV_HIP(hipMemcpyAsync(ctx->d_seqof.p, ctx->h_seqof.data(), (size_t)sumT * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
        return 0;
    };
    return run_beam_decode(ctx, ob, plan, gens, offsets, nseq, beam_width, path_out, score_out, status_out, t0, upload_seq_of, false);
}
}  // namespace

extern "C" int fv_decode_beam_batch(fv_ctx *ctx, const int *ob, const long long *offsets, int nseq, int n_split, int beam_width,
                                    int mode, int *path_out, float *score_out, int *status_out)
{
    if (!ctx) return FV_ERR_ARG;
    FV_NO_STREAM(ctx);
    if (ctx->csr && !ctx->opt_sparse_beam) { ctx->detail = "fv_decode_beam_batch: not available on a model set by fv_set_model_sparse (the beam kernels gather dense rows)"; return FV_ERR_UNSUPPORTED; }
    if (ctx->group || ctx->comm || ctx->nranks > 1) {
        ctx->detail = "fv_decode_beam_batch: one device, no communicator and no partition (sequences are not dealt to ranks)";
        return FV_ERR_UNSUPPORTED;
    }
    return fvi::drained(ctx, decode_beam_batch_impl(ctx, ob, offsets, nseq, n_split, beam_width, mode, path_out, score_out, status_out));
}

namespace {
// fv_test_beam_step (include/flashvit_testing.h): one launch of the beam step kernel over caller-given slot sets.  Set q
// plays step j = q: its slots, cut record, scores, back-pointers, doubt and candidate lists sit at index q of the
// decode's own per-step buffers.
int test_beam_step_impl(fv_ctx *ctx, int beam, const fv_test_beam_set *sets, int nsets, const int *sym, int speculative,
                        float theta, float next_bound, int cand_cap, float *scores_out, int *bp_out, int *ties_out,
                        int *tie_count_out, int *doubt_out, int *doubt_counts, fv_test_cand *cand_out, int *cand_counts,
                        unsigned long long *variants_out)
{
    if (!sets || !sym || nsets < 1 || nsets > fvb::BEAM_CHUNK || !scores_out || !bp_out || !ties_out || !tie_count_out ||
        !doubt_out || !doubt_counts || cand_cap < 0 || (cand_cap > 0 && (!cand_out || !cand_counts))) return FV_ERR_ARG;
    if (ctx->K == 0) return FV_ERR_STATE;
    int rc = beam_admit(ctx, beam);
    if (rc) return rc;
    {   // model symbols only: the launch rule reads the view of the model's log B
        const int *model_ob = sym;
        if ((rc = fvi::emission_view(ctx, model_ob, nsets))) return rc;
    }
    const int K = ctx->K, BP = fvb::beam_pitch(beam);
    // the kernels stage beam_pitch(beam) entries of every set, whatever its length: the rest is padding
    std::vector<float> hv((size_t)nsets * BP, -HUGE_VALF), cut((size_t)nsets * fvb::CUT_W, 0.0f);
    std::vector<int> hs((size_t)nsets * BP, 0);
    for (int q = 0; q < nsets; ++q) {
        const fv_test_beam_set &st = sets[q];
        if (!st.val || !st.state || st.n < beam || st.n > BP || sym[q] < 0 || sym[q] >= ctx->M) return FV_ERR_ARG;
        for (int e = 0; e < st.n; ++e) {
            if (st.state[e] < 0 || st.state[e] >= K) return FV_ERR_ARG;
            hv[(size_t)q * BP + e] = st.val[e];
            hs[(size_t)q * BP + e] = st.state[e];
        }
        float *c = cut.data() + (size_t)q * fvb::CUT_W;
        c[fvb::CUT_THETA] = theta;
        c[fvb::CUT_STATE] = speculative ? 1.0f : 0.0f;
        c[fvb::CUT_NEXT] = next_bound;
        c[fvb::CUT_N] = (float)st.n;
    }
    FV_HIP(hipSetDevice(ctx->device));
    if ((rc = beam_tables(ctx))) return rc;
    const size_t n = (size_t)nsets;
    fvi::Wants w;
    w.add(ctx->d_hval, n * BP); w.add(ctx->d_hstate, n * BP); w.add(ctx->d_cut, n * fvb::CUT_W);
    w.add(ctx->d_scores, n * K); w.add(ctx->d_bp, n * K); w.add(ctx->d_dupwin, n);
    w.add(ctx->d_doubt, n * fvb::DOUBT_CAP); w.add(ctx->d_doubt_count, n);
    w.add(ctx->d_tie_list, n * K); w.add(ctx->d_tie_count, (size_t)4);
    w.add(ctx->d_counters, (size_t)FV_NCOUNTERS); w.add(ctx->d_cand_count, n);
    if (cand_cap) w.add(ctx->d_cand, n * cand_cap);
    if (ctx->csr) { w.add(ctx->d_csr_acc, n * K); w.add(ctx->d_csr_tie, n * K); }
    if ((rc = fvi::grant(ctx, w, false))) return rc;
    if (ctx->csr) {
        FV_HIP(hipMemsetAsync(ctx->d_csr_acc.p, 0, (size_t)nsets * K * sizeof(unsigned long long), ctx->stream));
        FV_HIP(hipMemsetAsync(ctx->d_csr_tie.p, 0, (size_t)nsets * K * sizeof(unsigned int), ctx->stream));
    }
    FV_HIP(hipMemcpyAsync(ctx->d_hval.p, hv.data(), hv.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    FV_HIP(hipMemcpyAsync(ctx->d_hstate.p, hs.data(), hs.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    FV_HIP(hipMemcpyAsync(ctx->d_cut.p, cut.data(), cut.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    FV_HIP(hipMemsetAsync(ctx->d_dupwin.p, 0, (size_t)nsets * sizeof(int), ctx->stream));
    FV_HIP(hipMemsetAsync(ctx->d_doubt_count.p, 0, (size_t)nsets * sizeof(int), ctx->stream));
    FV_HIP(hipMemsetAsync(ctx->d_cand_count.p, 0, (size_t)nsets * sizeof(int), ctx->stream));
    FV_HIP(hipMemsetAsync(ctx->d_tie_count.p, 0, sizeof(unsigned int), ctx->stream));
    FV_HIP(hipMemsetAsync(ctx->d_counters.p, 0, FV_NCOUNTERS * sizeof(unsigned long long), ctx->stream));
    fvb::BeamStepArgs a = beam_step_args(ctx, beam, cand_cap);
    a.n = nsets;
    for (int q = 0; q < nsets; ++q) a.p[q] = beam_step_job(ctx, beam, q, q, sym[q]);      // (the view is the model's log B)
    FvTestRecording recording(ctx);
    if ((rc = launch_beam_step(ctx, a, ctx->stream))) return rc;
    unsigned int nties = 0;
    FV_HIP(hipMemcpyAsync(scores_out, ctx->d_scores.p, (size_t)nsets * K * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    FV_HIP(hipMemcpyAsync(bp_out, ctx->d_bp.p, (size_t)nsets * K * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    FV_HIP(hipMemcpyAsync(&nties, ctx->d_tie_count.p, sizeof nties, hipMemcpyDeviceToHost, ctx->stream));
    FV_HIP(hipMemcpyAsync(ties_out, ctx->d_tie_list.p, (size_t)nsets * K * sizeof(int2), hipMemcpyDeviceToHost, ctx->stream));
    FV_HIP(hipMemcpyAsync(doubt_out, ctx->d_doubt.p, (size_t)nsets * fvb::DOUBT_CAP * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    FV_HIP(hipMemcpyAsync(doubt_counts, ctx->d_doubt_count.p, (size_t)nsets * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    if (cand_cap) {
        static_assert(sizeof(fv_test_cand) == sizeof(fvb::HNode), "fv_test_cand mirrors HNode");
        FV_HIP(hipMemcpyAsync(cand_out, ctx->d_cand.p, (size_t)nsets * cand_cap * sizeof(fvb::HNode), hipMemcpyDeviceToHost, ctx->stream));
        FV_HIP(hipMemcpyAsync(cand_counts, ctx->d_cand_count.p, (size_t)nsets * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    }
    FV_HIP(hipStreamSynchronize(ctx->stream));
    *tie_count_out = (int)std::min<unsigned int>(nties, (unsigned int)(nsets * K));
    if (variants_out) *variants_out = ctx->test_variants;
    return FV_OK;
}
}  // namespace

extern "C" int fv_test_beam_step(fv_ctx *ctx, int beam, const fv_test_beam_set *sets, int nsets, const int *sym, int speculative,
                                 float theta, float next_bound, int cand_cap, float *scores_out, int *bp_out, int *ties_out,
                                 int *tie_count_out, int *doubt_out, int *doubt_counts, fv_test_cand *cand_out, int *cand_counts,
                                 unsigned long long *variants_out)
{
    if (!ctx) return FV_ERR_ARG;
    FV_NO_STREAM(ctx);
    if (fvi::group_size(ctx) > 1) { ctx->detail = "fv_test_beam_step: one device per context"; return FV_ERR_ARG; }
    if (ctx->csr && !ctx->opt_sparse_beam) { ctx->detail = "fv_test_beam_step: not available on a model set by fv_set_model_sparse"; return FV_ERR_UNSUPPORTED; }
    return fvi::drained(ctx, test_beam_step_impl(ctx, beam, sets, nsets, sym, speculative, theta, next_bound, cand_cap, scores_out,
                                                 bp_out, ties_out, tie_count_out, doubt_out, doubt_counts, cand_out, cand_counts,
                                                 variants_out));
}

namespace {
// fv_test_beam_select (include/flashvit_testing.h): one select launch over caller-given score rows.  Row q plays time
// j = 3 q + 2 of a pass that began at j - s: its own records, the previous cut (j - 1) and the slot the seeded predictor
// reads (j + 1) are no other row's.
int test_beam_select_impl(fv_ctx *ctx, int K, int beam, int s, const fv_test_select_set *sets, int nsets, float prev_theta,
                          float prev_margin, const float *seed, int want_layout, int *cand_cap_out, float *cut_out,
                          float *member_val_out, int *member_state_out, unsigned long long *counters_out, float *slot_val_out,
                          int *slot_state_out, unsigned long long *selects_out)
{
    constexpr int MAX_SETS = 64;
    static_assert(MAX_SETS <= fvb::HEAP_CHUNK, "one heap_build_all launch");
    if (!cand_cap_out || s < 0 || s > 2 || nsets < 0 || nsets > MAX_SETS) return FV_ERR_ARG;
    int rc = beam_admit_k(K, beam);
    if (rc) return rc;
    const int cap = beam_cand_cap(ctx, K, beam), BP = fvb::beam_pitch(beam), Tn = 3 * nsets + 3;
    *cand_cap_out = cap;
    if (nsets == 0) return FV_OK;
    if (!sets || !cut_out || !member_val_out || !member_state_out || !counters_out ||
        (want_layout && (!slot_val_out || !slot_state_out))) return FV_ERR_ARG;
    for (int q = 0; q < nsets; ++q) {
        const fv_test_select_set &st = sets[q];
        if (!st.scores) return FV_ERR_ARG;
        if (!st.cand) continue;
        if (cap == 0 || s == 0 || st.cand_count < 0) { ctx->detail = "fv_test_beam_select: a decode has no candidate list here"; return FV_ERR_ARG; }
        for (int e = 0; e < std::min(st.cand_count, cap); ++e)
            if (st.cand[e].state < 0 || st.cand[e].state >= K) return FV_ERR_ARG;
    }
    FV_HIP(hipSetDevice(ctx->device));
    auto slot = [](int q) { return (size_t)(3 * q + 2); };
    const size_t n = (size_t)Tn;
    fvi::Wants w;
    w.add(ctx->d_scores, n * K); w.add(ctx->d_hval, n * BP); w.add(ctx->d_hstate, n * BP); w.add(ctx->d_cut, n * fvb::CUT_W);
    w.add(ctx->d_doubt_count, n); w.add(ctx->d_cand_count, n);
    if (cap) w.add(ctx->d_cand, n * cap);
    w.add(ctx->d_counters, (size_t)FV_NCOUNTERS); w.add(ctx->d_passL, (size_t)nsets);
    if (want_layout) { w.add(ctx->d_slot_val, n * beam); w.add(ctx->d_slot_state, n * beam); }
    if ((rc = fvi::grant(ctx, w, false))) return rc;
    std::vector<float> cut((size_t)Tn * fvb::CUT_W, std::nanf(""));
    std::vector<int> counts((size_t)Tn, 0), first((size_t)nsets);
    static_assert(sizeof(fv_test_cand) == sizeof(fvb::HNode), "fv_test_cand mirrors HNode");
    for (int q = 0; q < nsets; ++q) {
        const size_t j = slot(q);
        first[(size_t)q] = (int)j - s;
        if (seed) { cut[j * fvb::CUT_W + fvb::CUT_THETA] = seed[0]; cut[(j + 1) * fvb::CUT_W + fvb::CUT_THETA] = seed[1]; }
        if (s >= 1) {
            float *c = cut.data() + (j - 1) * fvb::CUT_W;
            std::fill(c, c + fvb::CUT_W, 0.0f);
            c[fvb::CUT_THETA] = prev_theta; c[fvb::CUT_STATE] = 0.0f; c[fvb::CUT_NEXT] = HUGE_VALF;
            c[fvb::CUT_N] = (float)beam; c[fvb::CUT_MARGIN] = prev_margin;
        }
        FV_HIP(hipMemcpyAsync(ctx->d_scores.p + j * K, sets[q].scores, (size_t)K * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
        if (sets[q].cand) {
            counts[j] = sets[q].cand_count;
            FV_HIP(hipMemcpyAsync(ctx->d_cand.p + j * cap, sets[q].cand, (size_t)std::min(sets[q].cand_count, cap) * sizeof(fvb::HNode),
                                  hipMemcpyHostToDevice, ctx->stream));
        }
    }
    FV_HIP(hipMemcpyAsync(ctx->d_cut.p, cut.data(), cut.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    FV_HIP(hipMemcpyAsync(ctx->d_cand_count.p, counts.data(), counts.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    FV_HIP(hipMemcpyAsync(ctx->d_passL.p, first.data(), first.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    FV_HIP(hipMemsetAsync(ctx->d_hval.p, 0xFF, (size_t)Tn * BP * sizeof(float), ctx->stream));       // NaN / -1: not written
    FV_HIP(hipMemsetAsync(ctx->d_hstate.p, 0xFF, (size_t)Tn * BP * sizeof(int), ctx->stream));
    FV_HIP(hipMemsetAsync(ctx->d_doubt_count.p, 0, (size_t)Tn * sizeof(int), ctx->stream));
    FV_HIP(hipMemsetAsync(ctx->d_counters.p, 0, FV_NCOUNTERS * sizeof(unsigned long long), ctx->stream));
    const fvb::ResolveCtx rcx = resolve_ctx(ctx, K, beam, ctx->d_passL.p, false);
    FvTestRecording recording(ctx);
    if ((rc = launch_beam_select(ctx, K, beam, Tn, rcx, ctx->d_passL.p, nsets, s, [&](int q) { return first[(size_t)q]; }, ctx->stream)))
        return rc;
    if (want_layout) {
        fvb::HeapAllArgs h = heap_all_args(ctx, K, beam, nullptr, nullptr);
        h.n = nsets;
        for (int q = 0; q < nsets; ++q) h.p[q] = fvb::HeapRange{ (int)slot(q), (int)slot(q) };
        ctx->test_selects |= FV_TS_HEAP_BUILD_ALL;
        hipLaunchKernelGGL(fvb::heap_build_all, dim3(1, nsets), dim3(128), fvb::heap_lds(beam), ctx->stream, h);
        FV_HIP(hipGetLastError());
    }
    unsigned long long cnt[FV_NCOUNTERS];
    FV_HIP(hipMemcpyAsync(cut.data(), ctx->d_cut.p, cut.size() * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    FV_HIP(hipMemcpyAsync(cnt, ctx->d_counters.p, sizeof cnt, hipMemcpyDeviceToHost, ctx->stream));
    for (int q = 0; q < nsets; ++q) {
        const size_t j = slot(q);
        FV_HIP(hipMemcpyAsync(member_val_out + (size_t)q * BP, ctx->d_hval.p + j * BP, (size_t)BP * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        FV_HIP(hipMemcpyAsync(member_state_out + (size_t)q * BP, ctx->d_hstate.p + j * BP, (size_t)BP * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        if (want_layout) {
            FV_HIP(hipMemcpyAsync(slot_val_out + (size_t)q * beam, ctx->d_slot_val.p + j * beam, (size_t)beam * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
            FV_HIP(hipMemcpyAsync(slot_state_out + (size_t)q * beam, ctx->d_slot_state.p + j * beam, (size_t)beam * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        }
    }
    FV_HIP(hipStreamSynchronize(ctx->stream));
    for (int q = 0; q < nsets; ++q)
        std::copy(cut.begin() + slot(q) * fvb::CUT_W, cut.begin() + (slot(q) + 1) * fvb::CUT_W, cut_out + (size_t)q * fvb::CUT_W);
    const int which[8] = { fvk::CNT_BEAM_EXACT_SETS, fvk::CNT_HANDSHAKE_TIMEOUT, fvk::CNT_BEAM_CAND_SELECTS, fvk::CNT_BEAM_SPEC_STEPS,
                           fvk::CNT_BEAM_REACH_EVENTS, fvk::CNT_BEAM_LIST_SHORT, fvk::CNT_BEAM_LIST_LONG, fvk::CNT_BEAM_LIST_ENTRIES };
    for (int i = 0; i < 8; ++i) counters_out[i] = cnt[which[i]];
    if (selects_out) *selects_out = ctx->test_selects;
    return FV_OK;
}
}  // namespace

extern "C" int fv_test_beam_select(fv_ctx *ctx, int K, int beam, int s, const fv_test_select_set *sets, int nsets, float prev_theta,
                                   float prev_margin, const float *seed, int want_layout, int *cand_cap_out, float *cut_out,
                                   float *member_val_out, int *member_state_out, unsigned long long *counters_out,
                                   float *slot_val_out, int *slot_state_out, unsigned long long *selects_out)
{
    if (!ctx) return FV_ERR_ARG;
    FV_NO_STREAM(ctx);
    if (fvi::group_size(ctx) > 1) { ctx->detail = "fv_test_beam_select: one device per context"; return FV_ERR_ARG; }
    return fvi::drained(ctx, test_beam_select_impl(ctx, K, beam, s, sets, nsets, prev_theta, prev_margin, seed, want_layout, cand_cap_out,
                                                   cut_out, member_val_out, member_state_out, counters_out, slot_val_out,
                                                   slot_state_out, selects_out));
}

namespace {
// fv_test_beam_forward (include/flashvit_testing.h): the caller's passes as one generation of run_beam_generations — the
// decode's own prologue, driver and epilogue — then the per-step buffers of the passes' ranges copied out.
int test_beam_forward_impl(fv_ctx *ctx, const int *ob, int T, int beam, const fv_test_beam_pass *tp, int np,
                           const fv_test_beam_tables *out)
{
    static_assert(FV_TEST_TIE_TAG == fvb::TIE_TAG, "bp is copied out raw");
    constexpr int MAX_PASSES = 64;
    if (!tp || !out || T < 2 || np < 1 || np > MAX_PASSES) return FV_ERR_ARG;
    int rc = fvi::emission_view(ctx, ob, T);
    if (rc) return rc;
    if (ctx->K == 0) return FV_ERR_STATE;
    if ((rc = beam_admit(ctx, beam))) return rc;
    for (int j = 0; j < T; ++j) if (ob[j] < 0 || ob[j] >= ctx->view.nsym) return FV_ERR_ARG;
    const int K = ctx->K;
    const bool whole = np == 1 && tp[0].L == 0 && tp[0].R == T - 1 && tp[0].init_state < 0 && tp[0].end_state < 0;
    std::vector<std::vector<fv::Pass>> gens(1);
    std::vector<int> byL((size_t)np), ans((size_t)T, 0);
    for (int q = 0; q < np; ++q) {
        const fv_test_beam_pass &p = tp[q];
        if (p.L < 0 || p.R <= p.L || p.R >= T) { ctx->detail = "fv_test_beam_forward: a pass needs 0 <= L < R < T"; return FV_ERR_ARG; }
        if (p.init_state < -1 || p.init_state >= K || p.end_state < -1 || p.end_state >= K || (p.L == 0 && p.init_state >= 0)) {
            ctx->detail = "fv_test_beam_forward: states in [-1, K), init_state < 0 at L = 0";
            return FV_ERR_ARG;
        }
        gens[0].push_back(fv::Pass{ p.L, p.R, p.L == 0, whole, 0, -1, 0 });
        byL[(size_t)q] = q;
    }
    std::sort(byL.begin(), byL.end(), [&](int a, int b) { return tp[a].L < tp[b].L; });
    for (int q = 1; q < np; ++q) {
        const fv_test_beam_pass &l = tp[byL[(size_t)q - 1]], &r = tp[byL[(size_t)q]];
        if (r.L <= l.R) { ctx->detail = "fv_test_beam_forward: passes overlap"; return FV_ERR_ARG; }
        if (r.L == l.R + 1 && r.init_state != l.end_state) {
            ctx->detail = "fv_test_beam_forward: touching passes disagree on the answer entry they share";
            return FV_ERR_ARG;
        }
    }
    auto t0 = clk::now();
    fv::Plan plan;                   // one generation; no segments: the epilogue gathers nothing
    plan.gen_begin = { 0, np };
    // what the init rows (ans[L-1]) and the pass ends (ans[R]) read; `ans` lives until the epilogue has synchronised
    auto upload_ans = [&]() -> int {
        if (whole) return 0;
        for (int q = 0; q < np; ++q) {
            ans[(size_t)tp[q].R] = tp[q].end_state;
            if (tp[q].L > 0) ans[(size_t)tp[q].L - 1] = tp[q].init_state;
        }
        FV_HIP(hipMemcpyAsync(ctx->d_ans.p, ans.data(), (size_t)T * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
        return 0;
    };
    std::vector<int> path((size_t)T);
    float score = 0.0f;
    const long long seq[2] = { 0, T };
    if ((rc = run_beam_decode(ctx, ob, plan, gens, seq, 0, beam, path.data(), &score, nullptr, t0, upload_ans, true)) < 0) return rc;
    // the generation has finished (finish_decode synchronised): plain copies of the passes' rows
    const size_t BP = (size_t)fvb::beam_pitch(beam), B = (size_t)beam, Ks = (size_t)K;
    auto rows = [&](auto *dst, const auto *src, size_t first, size_t n, size_t width) -> hipError_t {
        if (!dst || n == 0) return hipSuccess;
        return hipMemcpy(dst + first * width, src + first * width, n * width * sizeof(*dst), hipMemcpyDeviceToHost);
    };
    for (int q = 0; q < np; ++q) {
        const size_t L = (size_t)tp[q].L, n = (size_t)(tp[q].R - tp[q].L + 1);
        FV_HIP(rows(out->scores, ctx->d_scores.p, L, n, Ks));
        FV_HIP(rows(out->bp, ctx->d_bp.p, L + 1, n - 1, Ks));
        FV_HIP(rows(out->cut, ctx->d_cut.p, L, n, (size_t)fvb::CUT_W));
        FV_HIP(rows(out->member_val, ctx->d_hval.p, L, n, BP));
        FV_HIP(rows(out->member_state, ctx->d_hstate.p, L, n, BP));
        FV_HIP(rows(out->doubt, ctx->d_doubt.p, L, n, (size_t)fvb::DOUBT_CAP));
        FV_HIP(rows(out->doubt_count, ctx->d_doubt_count.p, L, n, (size_t)1));
        FV_HIP(rows(out->slot_val, ctx->d_slot_val.p, L, n, B));
        FV_HIP(rows(out->slot_state, ctx->d_slot_state.p, L, n, B));
        if (out->path) std::copy(path.begin() + tp[q].L, path.begin() + tp[q].R + 1, out->path + tp[q].L);
    }
    if (out->gate) FV_HIP(hipMemcpy(out->gate, ctx->d_needfull.p, sizeof(int), hipMemcpyDeviceToHost));
    if (out->score && whole) *out->score = score;
    if (out->variants) *out->variants = ctx->test_variants;
    if (out->selects) *out->selects = ctx->test_selects;
    return rc;
}
}  // namespace

extern "C" int fv_test_beam_forward(fv_ctx *ctx, const int *ob, int T, int beam, const fv_test_beam_pass *passes, int npasses,
                                    const fv_test_beam_tables *out)
{
    if (!ctx) return FV_ERR_ARG;
    FV_NO_STREAM(ctx);
    if (fvi::group_size(ctx) > 1 || ctx->comm || ctx->nranks > 1) {
        ctx->detail = "fv_test_beam_forward: one device, no communicator and no partition";
        return FV_ERR_ARG;
    }
    if (ctx->csr && !ctx->opt_sparse_beam) { ctx->detail = "fv_test_beam_forward: not available on a model set by fv_set_model_sparse"; return FV_ERR_UNSUPPORTED; }
    return fvi::drained(ctx, test_beam_forward_impl(ctx, ob, T, beam, passes, npasses, out));
}

#ifdef FV_REPLAY_PROF
// Experiment builds only: read and reset the replay profile (fv_beam_kernels.hip.inc, replay_prof).
extern "C" int fv_debug_replay_prof(unsigned long long *out8)
{
    unsigned long long z[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(fvb::replay_prof), sizeof z) != hipSuccess) return FV_ERR_DEVICE;
    if (hipMemcpyToSymbol(HIP_SYMBOL(fvb::replay_prof), z, sizeof z) != hipSuccess) return FV_ERR_DEVICE;
    return FV_OK;
}
extern "C" int fv_debug_reach_prof(unsigned long long *out8)
{
    unsigned long long z[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(fvb::reach_prof), sizeof z) != hipSuccess) return FV_ERR_DEVICE;
    if (hipMemcpyToSymbol(HIP_SYMBOL(fvb::reach_prof), z, sizeof z) != hipSuccess) return FV_ERR_DEVICE;
    return FV_OK;
}
#endif

namespace fvi {
int beam_setup(fv_ctx *ctx) { return fvb::allow_big_lds(ctx->detail); }
}  // namespace fvi
