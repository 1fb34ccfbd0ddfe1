// fv_full.hip — the full-state path of libflashvit.so: step-kernel launchers, the lock-step generation driver and
// the decode entry points fv_decode_full / fv_decode_vanilla / fv_decode_checkpoint.
//
// Everything a decode needs is enqueued on one HIP stream without a single host
// round trip: the task tree depends only on (T, n_split), and every state index a
// later pass consumes (Ans[L-1], Ans[R]) stays in device memory.  One sync at the end.
#include "fv_internal.h"
#include "fv_kernels.hip.inc"
#include "flashvit_testing.h"

namespace {

int pick_kernel(const fv_ctx *ctx)
{
    if (ctx->opt_kernel == FV_KERNEL_F64_STREAM) return FV_KERNEL_F64_STREAM;
    // the filter kernels' error bracket needs every log <= 0 (no cancellation between score and log A)
    if (!ctx->view.logs_nonpositive) return FV_KERNEL_F64_STREAM;
    // Measured at K=3965 (us per step of the whole-sequence pass): q16 9.5, f32 11.1, f16 12.8, f64 20.7.
    // binary16's 2^-11 relative spacing makes its window ~0.008 wide (~430 extra candidates and ~7 lane
    // rescans per step); 16-bit fixed point has a window of ~3e-4 (~21 and 0.4) at the same 2 B/cell.
    if (ctx->opt_kernel == FV_KERNEL_F16_REFINE || ctx->opt_kernel == FV_KERNEL_F32_REFINE ||
        ctx->opt_kernel == FV_KERNEL_Q16_REFINE || ctx->opt_kernel == FV_KERNEL_U16_REFINE)
        return ctx->opt_kernel;
    if (ctx->opt_kernel == FV_KERNEL_SPARSE_Q16) return ctx->SPdata.p ? FV_KERNEL_SPARSE_Q16 : FV_KERNEL_U16_REFINE;
    // AUTO: the sparse walk visits only finite entries; it wins clearly below ~1/3 density
    return (ctx->SPdata.p && ctx->density <= 0.35) ? FV_KERNEL_SPARSE_Q16 : FV_KERNEL_U16_REFINE;
}

// Kernel variants: chunks of U 16-byte loads per lane, double-buffered in registers.
// "Upfront" (one register buffer holding the wave's whole share of the tile, requested before the
// score row is staged) measured SLOWER for the f32 table at K=3965 (16.3 vs 12.9 us/step): with every
// workgroup's whole tile in flight the L2 lines kept from the previous (opposite-direction) sweep are
// evicted before they are re-read.  Kept behind FV_OPT_DEBUG bit 2 for experiments.
constexpr int U_UP = 16, U_DB32 = 4, U_DB64 = 2, U_DB16 = 2;

// FV_TV_* bit of each step-kernel instantiation (include/flashvit_testing.h), recorded by the launch helpers during a
// test-hook call only.  U follows from the table type and DB.
constexpr int nb_slot(int NB) { return NB == 1 ? 0 : NB == 2 ? 1 : NB == 4 ? 2 : 3; }
template <typename TA> constexpr int tab_slot()
{
    return std::is_same<TA, double>::value ? 0 : std::is_same<TA, float>::value ? 1 : std::is_same<TA, fvk::half_t>::value ? 2 : 3;
}
template <typename TA, int NB, bool DB> constexpr unsigned long long step_variant()
{
    // per table type: the double-buffered forms (NB = 1, 2, 4, 8), then (all but float64) the whole-tile forms (NB = 1, 2)
    return 1ull << ((tab_slot<TA>() == 0 ? 0 : 4 + (tab_slot<TA>() - 1) * 6) + (DB ? 0 : 4) + nb_slot(NB));
}
template <typename TA> constexpr unsigned long long slab_variant() { return 1ull << (22 + tab_slot<TA>()); }
template <int NB, bool DB, int NWV> constexpr unsigned long long u16_variant()
{
    return 1ull << (26 + (NWV == 16 ? 0 : 8) + (DB ? 4 : 0) + nb_slot(NB));
}
template <int NB> constexpr unsigned long long sparse_variant() { return 1ull << (42 + nb_slot(NB)); }
template <int NB, bool MEM> constexpr unsigned long long csr_variant() { return 1ull << (FV_TV_CSR_SHIFT + (MEM ? 4 : 0) + nb_slot(NB)); }
// (the float64 walk: one bit per NB and one, set in addition, for the launches that read their score rows from memory)
template <int NB, bool MEM> constexpr unsigned long long csr_f64_variant() { return (1ull << (FV_TV_CSR64_SHIFT + nb_slot(NB))) | (MEM ? 1ull << (FV_TV_CSR64_SHIFT + 4) : 0ull); }
static_assert(step_variant<double, 8, true>() == FV_TV_F64_NB8 && step_variant<float, 2, false>() == FV_TV_F32_UP_NB2 &&
              step_variant<fvk::half_t, 1, true>() == FV_TV_F16_NB1 && step_variant<fvk::q16_t, 2, false>() == FV_TV_Q16_UP_NB2 &&
              slab_variant<fvk::q16_t>() == FV_TV_SLAB_Q16 && u16_variant<1, false, 16>() == FV_TV_U16_W16_UP_NB1 &&
              u16_variant<8, true, 8>() == FV_TV_U16_W8_NB8 && sparse_variant<8>() == FV_TV_SPARSE_NB8 &&
              csr_variant<1, false>() == FV_TV_CSR_LDS_NB1 && csr_variant<8, true>() == FV_TV_CSR_MEM_NB8 &&
              csr_f64_variant<1, false>() == FV_TV_CSR64_NB1 && csr_f64_variant<8, true>() == (FV_TV_CSR64_NB8 | FV_TV_CSR64_MEM),
              "FV_TV_* bits of include/flashvit_testing.h");

// One step launch as its caller describes it.  Everything else a launch reads is the context's model and options, which
// hold for the whole decode.
struct StepLaunch {
    int kernel;             // the FV_KERNEL_* the decode runs on (admit_full)
    hipStream_t stream;     // the queue the launch goes to
    bool forked;            // one of a generation's launches dealt to several streams: co-resident workgroups wanted (the
                            // packed 16-bit kernel in its double-buffered form, and for the batched launches as well)
    int reverse;            // sweep direction (StepArgs::reverse): alternates from step to step
};
// FV_OPT_ROW_CODES: what launch_step_kernel found for a launch's rows — StepArgs::codes and one CodeSlot per task
struct LaunchCodes { int codes; const fvk::CodeSlot *slots; };

// The task counts the step kernels are instantiated for.  with_nb calls f(std::integral_constant<int, NB>) for the
// smallest of them that holds nb tasks: the one place a run-time task count becomes a template argument.
template <int... NB> struct NbList {};
constexpr NbList<1, 2, 4, 8> STEP_NB{};
template <typename F, int... NB>
int with_nb(NbList<NB...>, int nb, F &&f)
{
    constexpr int all[] = { NB... }, last = all[sizeof...(NB) - 1];
    static_assert(last == fvk::MAX_BATCH, "the largest instantiation holds MAX_BATCH tasks");
    int rc = 0;
    (void)((nb <= NB || NB == last ? (rc = f(std::integral_constant<int, NB>{}), true) : false) || ...);
    return rc;
}

// what every argument struct has: the model's geometry and the task slots, the unused ones padded with slot 0
template <typename Args>
void fill_common(const fv_ctx *ctx, const fvk::TaskSlot *slots, int nb, Args &a)
{
    a.K = ctx->K;
    a.nrows = ctx->nrows;
    a.ntiles = (ctx->K + fvk::TILE_W - 1) / fvk::TILE_W;
    a.tiles_per_xcd = (a.ntiles + 7) / 8;
    a.nb = nb;
    constexpr int NB = (int)(sizeof(a.t) / sizeof(a.t[0]));
    for (int t = 0; t < NB; ++t) a.t[t] = slots[t < nb ? t : 0];
}

template <typename TA, int NB, int U, bool DB>
int launch_variant(fv_ctx *ctx, const StepLaunch &ln, const fvk::StepArgs<NB> &a, size_t lds)
{
    if (ctx->test_record) ctx->test_variants |= step_variant<TA, NB, DB>();
    hipLaunchKernelGGL((fvk::trellis_step<TA, NB, U, DB>), dim3(a.tiles_per_xcd * 8), dim3(fvk::BLOCK), lds, ln.stream, a);
    FV_HIP(hipGetLastError());
    return 0;
}

// source rows per launch of trellis_step: all of them if NB score rows fit LDS next to the reduction scratch
template <int NB>
int slab_rows(const fv_ctx *ctx)
{
    int slab = ctx->nrows;
    if (ctx->opt_debug & FV_DBG_SLABS) slab = std::max(64, (ctx->nrows / 3 + 63) / 64 * 64);
    while (slab > 64 && fvk::step_lds_bytes<NB>(slab) > (size_t)fvk::LDS_LIMIT) slab = (slab / 2 + 63) / 64 * 64;
    return slab;
}

// the fields of StepArgs both of its kernels read (trellis_step, trellis_step_u16); LA and window are the caller's
template <int NB>
void fill_step_args(const fv_ctx *ctx, const StepLaunch &ln, const fvk::TaskSlot *slots, int nb, fvk::StepArgs<NB> &a)
{
    fill_common(ctx, slots, nb, a);
    a.qscale = ctx->qscale;
    a.LA64 = ctx->LA64.p;
    a.counters = ctx->d_counters.p;
    a.reverse = (ctx->opt_debug & FV_DBG_NO_REVERSE) ? 0 : ln.reverse;
    a.debug = ctx->opt_debug;
    a.row_lo = 0; a.srows = ctx->nrows; a.merge = 0;
}

template <typename TA, int NB>
int launch_step_nb(fv_ctx *ctx, const StepLaunch &ln, const fvk::TaskSlot *slots, int nb)
{
    fvk::StepArgs<NB> a;
    fill_step_args(ctx, ln, slots, nb, a);
    if constexpr (std::is_same<TA, double>::value) { a.LA = ctx->LA64.p; a.window = 0.0f; }
    else if constexpr (std::is_same<TA, float>::value) { a.LA = ctx->LA32.p; a.window = 0.0f; }
    else if constexpr (std::is_same<TA, fvk::q16_t>::value) { a.LA = ctx->LAQ16.p; a.window = ctx->windowq; }
    else { a.LA = ctx->LA16.p; a.window = ctx->window16; }
    a.vanilla = ctx->vanilla;
    a.codes = 0;
    for (int t = 0; t < NB; ++t) a.c[t] = fvk::CodeSlot{ nullptr, nullptr, nullptr, nullptr };
    const size_t lds = fvk::step_lds_bytes<NB>(ctx->nrows);
    constexpr int RBR = 4 * fvk::Tab<TA>::R;
    const int nj_max = (ctx->nrows / RBR + fvk::NWAVES - 1) / fvk::NWAVES;
    // One launch when the score rows fit LDS; otherwise (K > ~40100 at NB = 1: the route of every model the packed 16-bit
    // kernel cannot take — K > 65536, or entries above 1) one launch per slab of source rows, ascending, each merging
    // into what the slabs below it left in t1_out / bp_out.  FV_OPT_DEBUG bit 21 forces three slabs (tests).
    const int slab = slab_rows<NB>(ctx);
    if (slab < ctx->nrows) {
        constexpr int U = std::is_same<TA, double>::value ? U_DB64 : std::is_same<TA, float>::value ? U_DB32 : U_DB16;
        a.reverse = 0;
        if (ctx->test_record) ctx->test_variants |= slab_variant<TA>();
        for (int lo = 0; lo < ctx->nrows; lo += slab) {
            a.row_lo = lo; a.srows = std::min(slab, ctx->nrows - lo); a.merge = lo > 0 ? 1 : 0;
            const int rc = launch_variant<TA, NB, U, true>(ctx, ln, a, fvk::step_lds_bytes<NB>(a.srows));
            if (rc) return rc;
        }
        return 0;
    }
    if constexpr (std::is_same<TA, double>::value) {
        return launch_variant<TA, NB, U_DB64, true>(ctx, ln, a, lds);
    } else if constexpr (std::is_same<TA, float>::value) {
        if constexpr (NB <= 2) {
            if (nj_max <= U_UP && (ctx->opt_debug & FV_DBG_ALT_LOADS)) return launch_variant<TA, NB, U_UP, false>(ctx, ln, a, lds);
        }
        return launch_variant<TA, NB, U_DB32, true>(ctx, ln, a, lds);
    } else {
        // 16-bit tables: an XCD's slab (3.9 MB at K=3965) nearly fits its L2, so requesting the whole
        // tile before staging the score row wins (9.5 vs 9.8 us/step); FV_OPT_DEBUG bit 2 turns it off.
        // That variant holds the tile in 86 VGPRs: one workgroup per CU.  With more tiles than CUs the
        // double-buffered one (46 VGPRs, two workgroups per CU) keeps the grid in one round
        // (K=5632: 18.3 vs 25.3 us/step, K=8192: 25.8 vs 39.8).
        if constexpr (NB <= 2) {
            if (nj_max <= U_UP && a.ntiles <= ctx->num_cus && !(ctx->opt_debug & FV_DBG_ALT_LOADS)) return launch_variant<TA, NB, U_UP, false>(ctx, ln, a, lds);
        }
        // (8-wave workgroups for the batched launches, as the packed 16-bit kernel uses, were measured: 2.14 vs 2.10 ms of
        // right-hand passes at cfg2, 65.6 vs 62.7 ms at cfg3 — the f32 sweep needs its four waves per SIMD)
        return launch_variant<TA, NB, U_DB16, true>(ctx, ln, a, lds);
    }
}

template <typename TA>
int launch_step(fv_ctx *ctx, const StepLaunch &ln, const fvk::TaskSlot *slots, int nb)
{
    return with_nb(STEP_NB, nb, [&](auto NB) { return launch_step_nb<TA, NB()>(ctx, ln, slots, nb); });
}

template <int NB>
int launch_sparse_nb(fv_ctx *ctx, const StepLaunch &ln, const fvk::TaskSlot *slots, int nb)
{
    fvk::SparseArgs<NB> a;
    fill_common(ctx, slots, nb, a);
    a.data = ctx->SPdata.p; a.tile_off = ctx->SPoff.p; a.tile_nwb = ctx->SPnwb.p;
    a.LA64 = ctx->LA64.p; a.counters = ctx->d_counters.p;
    a.debug = ctx->opt_debug;
    a.window = ctx->windowq; a.qscale = ctx->qscale;
    if (ctx->test_record) ctx->test_variants |= sparse_variant<NB>();
    hipLaunchKernelGGL((fvk::trellis_step_sparse<NB>), dim3(a.tiles_per_xcd * 8), dim3(fvk::SP_BLOCK),
                       fvk::sparse_lds_bytes<NB>(ctx->nrows), ln.stream, a);
    FV_HIP(hipGetLastError());
    return 0;
}

// The two walks over a CSR-set model keep their score rows in LDS while NB of them fit (lds_form_bytes), else — or under
// FV_OPT_DEBUG bit 31 — read them from memory: go(std::true_type) launches the memory form, go(std::false_type) the LDS form.
template <typename Go>
void launch_csr_form(const fv_ctx *ctx, size_t lds_form_bytes, Go &&go)
{
    if (ctx->opt_csr_mem || lds_form_bytes > (size_t)fvk::LDS_LIMIT) go(std::true_type{});
    else go(std::false_type{});
}

// trellis_step_csr (FV_KERNEL_SPARSE_CSR): the filter walk
template <int NB>
int launch_csr_nb(fv_ctx *ctx, const StepLaunch &ln, const fvk::TaskSlot *slots, int nb)
{
    fvk::CsrArgs<NB> a;
    fill_common(ctx, slots, nb, a);
    a.ck = ctx->CSk.p; a.cq = ctx->CSq.p; a.c64 = ctx->CS64.p; a.tile_off = ctx->CSoff.p; a.tile_nwb = ctx->CSnwb.p;
    a.counters = ctx->d_counters.p;
    a.debug = ctx->opt_debug;
    a.window = ctx->windowq; a.qscale = ctx->qscale;
    launch_csr_form(ctx, fvk::csr_lds_bytes<NB>(ctx->nrows, false), [&](auto MEM) {
        if (ctx->test_record) ctx->test_variants |= csr_variant<NB, MEM()>();
        hipLaunchKernelGGL((fvk::trellis_step_csr<NB, MEM()>), dim3(a.tiles_per_xcd * 8), dim3(fvk::SP_BLOCK),
                           fvk::csr_lds_bytes<NB>(ctx->nrows, MEM()), ln.stream, a);
    });
    FV_HIP(hipGetLastError());
    return 0;
}

// trellis_step_csr_f64 (FV_KERNEL_CSR_F64): the float64 walk
template <int NB>
int launch_csr_f64_nb(fv_ctx *ctx, const StepLaunch &ln, const fvk::TaskSlot *slots, int nb)
{
    fvk::CsrF64Args<NB> a;
    fill_common(ctx, slots, nb, a);
    a.ck = ctx->CSk.p; a.c64 = ctx->CS64.p; a.tile_off = ctx->CSoff.p; a.tile_nwb = ctx->CSnwb.p;
    a.vanilla = ctx->vanilla;
    launch_csr_form(ctx, fvk::csr_f64_lds_bytes<NB>(ctx->nrows, false), [&](auto MEM) {
        if (ctx->test_record) ctx->test_variants |= csr_f64_variant<NB, MEM()>();
        hipLaunchKernelGGL((fvk::trellis_step_csr_f64<NB, MEM()>), dim3(a.tiles_per_xcd * 8), dim3(fvk::SP_BLOCK),
                           fvk::csr_f64_lds_bytes<NB>(ctx->nrows, MEM()), ln.stream, a);
    });
    FV_HIP(hipGetLastError());
    return 0;
}

// which task counts of trellis_step_u16 have a second instantiation without the FV_OPT_ROW_CODES code (CODES = false)
template <int NB> constexpr bool U16_CODE_FREE = NB == 1;

template <int NB, int U, bool DB, int NWV>
int launch_u16_variant(fv_ctx *ctx, const StepLaunch &ln, const fvk::StepArgs<NB> &a)
{
    const size_t lds = fvk::u16_lds_bytes<NB, NWV>(ctx->nrows);
    fvk::StepArgs<NB> b = a;
    if (!fvk::u16_takes_codes<NB, DB, NWV>()) b.codes &= ~1;
    if (ctx->test_record) ctx->test_variants |= u16_variant<NB, DB, NWV>() | ((b.codes & 1) ? FV_TV_ROW_CODES : 0ull);
    // a single-task launch that neither reads nor writes codes (under auto: every one) runs the form without the route's code;
    // the batched forms have no such twin (U16_CODE_FREE: there the last argument is `true` again, the same instantiation)
    if (U16_CODE_FREE<NB> && a.codes == 0)
        hipLaunchKernelGGL((fvk::trellis_step_u16<NB, U, DB, NWV, !U16_CODE_FREE<NB>>), dim3(a.tiles_per_xcd * 8), dim3(NWV * 64), lds, ln.stream, b);
    else
        hipLaunchKernelGGL((fvk::trellis_step_u16<NB, U, DB, NWV>), dim3(a.tiles_per_xcd * 8), dim3(NWV * 64), lds, ln.stream, b);
    FV_HIP(hipGetLastError());
    return 0;
}

template <int NB>
int launch_u16_nb(fv_ctx *ctx, const StepLaunch &ln, const LaunchCodes &lc, const fvk::TaskSlot *slots, int nb)
{
    fvk::StepArgs<NB> a;
    fill_step_args(ctx, ln, slots, nb, a);
    a.LA = ctx->LAQ16.p; a.window = ctx->windowq; a.vanilla = 0;
    a.codes = lc.codes;
    for (int t = 0; t < NB; ++t) a.c[t] = lc.slots[t < nb ? t : 0];
    const int nq = ctx->nrows / 32;
    // 8 waves per workgroup (FV_OPT_DEBUG bit 13: 16): everything outside the sweep — quantisation, reductions, refine —
    // is executed by every wave, so fewer, longer waves spend fewer issue slots on it
    if (ctx->opt_debug & FV_DBG_U16_W16) {
        if (a.ntiles <= ctx->num_cus && (nq + 15) / 16 <= 8 && !(ctx->opt_debug & FV_DBG_ALT_LOADS)) return launch_u16_variant<NB, 8, false, 16>(ctx, ln, a);
        return launch_u16_variant<NB, U_DB16, true, 16>(ctx, ln, a);
    }
    // (forked batches: the double-buffered form, 81 VGPRs at NB = 4 — three 8-wave workgroups of three streams share a CU;
    // the whole-tile form's 137 would leave room for one)
    if (a.ntiles <= ctx->num_cus && (nq + 7) / 8 <= 16 && !(ctx->opt_debug & FV_DBG_ALT_LOADS) && !ln.forked) return launch_u16_variant<NB, 16, false, 8>(ctx, ln, a);
    return launch_u16_variant<NB, U_DB16, true, 8>(ctx, ln, a);
}

// FV_OPT_ROW_CODES — the packed 16-bit kernel leaves, beside every score row it writes, the row's 16-bit codes and tile
// maxima, and a launch all of whose incoming rows have them copies them instead of quantising the floats again
// (fv_kernels.hip.inc, trellis_step_u16).  The host knows which kernel wrote each row: every step launch comes through
// launch_step_kernel, which finds the slots' rows in d_rows, hands the packed kernel their code rows and records what the
// launch leaves.  Rows outside d_rows (checkpoints), rows the other kernels wrote and rows past the code buffers have none.
// auto (profiles/row_codes_ab.json): the batched launches only, from the smallest K at which their part
// of a decode was measured to gain (K = 2048: 0.78 -> 0.73 ms; nothing at 512 and 1024) — small contexts keep their device
// bytes.  The single-task launches of the whole-sequence pass lose on the route (8.4 -> 8.9 us per step at K = 3965: writing
// the codes in the launch's tail costs more than the shorter prologue saves), so under auto they neither read nor write codes.
constexpr int ROW_CODES_AUTO_MIN_K = 2048;
constexpr int ROW_CODES_AUTO_FAMILIES = 2;       // bit 0 single-task launches, bit 1 batched launches

int coded_row_index(const fv_ctx *ctx, const float *row)
{
    if (!row || row < ctx->d_rows.p || row >= ctx->d_rows.p + ctx->d_rows.n) return -1;
    const size_t off = (size_t)(row - ctx->d_rows.p);
    if (off % (size_t)ctx->nrows) return -1;
    const size_t r = off / (size_t)ctx->nrows;
    return r < ctx->row_coded.size() ? (int)r : -1;
}

// the code rows for `pairs` passes' score rows (two each); no room for them: the decode runs without the route
int ensure_row_codes(fv_ctx *ctx, size_t pairs)
{
    if (!ctx->row_codes) { ctx->row_coded.clear(); return 0; }
    const size_t rows = pairs * 2, want = rows * (size_t)ctx->nrows;
    if (want > ctx->d_rcodes.n || want / fvk::TILE_W > ctx->d_rtmax.n) {
        if (ctx->d_rcodes.ensure(want) != hipSuccess || ctx->d_rtmax.ensure(want / fvk::TILE_W) != hipSuccess) {
            (void)hipGetLastError();
            ctx->d_rcodes.release(); ctx->d_rtmax.release();
            ctx->row_codes = 0; ctx->row_coded.clear();
            return 0;
        }
        // (pad tiles past the last real one are never written: 0xff is code 65535 and a NaN tile maximum, which score_code
        // turns into 65535 as well)
        FV_HIP(hipMemsetAsync(ctx->d_rcodes.p, 0xff, ctx->d_rcodes.bytes(), ctx->stream));
        FV_HIP(hipMemsetAsync(ctx->d_rtmax.p, 0xff, ctx->d_rtmax.bytes(), ctx->stream));
    }
    ctx->row_coded.assign(ctx->d_rcodes.n / (size_t)ctx->nrows, 0);
    return 0;
}

// init_rows' share: the code rows it writes beside the first row of `n` passes from pass `base` on (NULL: none)
bool init_rows_coded(fv_ctx *ctx, int base, int n)
{
    if (!ctx->row_codes || ctx->csr || (size_t)(base + n) * 2 > ctx->row_coded.size()) return false;
    for (int q = 0; q < n; ++q) ctx->row_coded[(size_t)(base + q) * 2] = 1;
    return true;
}

// One step launch of `nb` tasks, as `ln` describes it.  (Bare: a decode's launches go through queue_step, which counts them.)
int launch_step_kernel(fv_ctx *ctx, const StepLaunch &ln, const fvk::TaskSlot *slots, int nb)
{
    fvk::CodeSlot cs[fvk::MAX_BATCH];
    // Both filters of FV_KERNEL_U16_REFINE read the same 16-bit table and give the same bits, so the choice is per launch: the
    // packed 16-bit filter for single-task launches (the whole-sequence pass: 9.1 vs 9.3 us per step at K=3965/T=256,
    // 10.4 vs 14.2 at T=4096 where its window is the narrower one), for models whose float32 rows do not fit LDS and for
    // forked batches; the f32 filter for the other batched launches, where the 16-bit kernel's per-task prologue (row
    // maximum, quantisation) costs what its cheaper sweep saves.  FV_OPT_DEBUG bit 14: packed 16-bit for every launch.
    const bool packed = ln.kernel == FV_KERNEL_U16_REFINE && (nb <= 1 || !ctx->full_ok || (ctx->opt_debug & FV_DBG_U16_BATCHED) || ln.forked);
    bool all_in = packed && ctx->row_codes != 0, all_out = all_in;
    int rout[fvk::MAX_BATCH];
    for (int q = 0; q < nb; ++q) {
        const int rin = coded_row_index(ctx, slots[q].t1_in);
        rout[q] = coded_row_index(ctx, slots[q].t1_out);
        const size_t ntp = (size_t)ctx->nrows / fvk::TILE_W;
        cs[q].c_in = rin >= 0 ? ctx->d_rcodes.p + (size_t)rin * ctx->nrows : nullptr;
        cs[q].tmax_in = rin >= 0 ? ctx->d_rtmax.p + (size_t)rin * ntp : nullptr;
        cs[q].c_out = rout[q] >= 0 ? ctx->d_rcodes.p + (size_t)rout[q] * ctx->nrows : nullptr;
        cs[q].tmax_out = rout[q] >= 0 ? ctx->d_rtmax.p + (size_t)rout[q] * ntp : nullptr;
        all_in = all_in && rin >= 0 && ctx->row_coded[(size_t)rin];
        all_out = all_out && rout[q] >= 0;
    }
    // a batch only ever shrinks: the rows of a single-task launch are read by single-task launches, so it writes codes only if
    // those take the route; a batched launch writes them for whichever family reads its rows next
    const int family = nb <= 1 ? 1 : 2;
    const bool produce = all_out && (nb > 1 || (ctx->row_codes & 1));
    const LaunchCodes lc{ ((all_in && (ctx->row_codes & family)) ? 1 : 0) | (produce ? 2 : 0), cs };
    for (int q = 0; q < nb; ++q)
        if (rout[q] >= 0) ctx->row_coded[(size_t)rout[q]] = produce ? 1 : 0;
    switch (ln.kernel) {
    case FV_KERNEL_U16_REFINE:
        if (packed) return with_nb(STEP_NB, nb, [&](auto NB) { return launch_u16_nb<NB()>(ctx, ln, lc, slots, nb); });
        return launch_step<fvk::q16_t>(ctx, ln, slots, nb);
    case FV_KERNEL_SPARSE_Q16: return with_nb(STEP_NB, nb, [&](auto NB) { return launch_sparse_nb<NB()>(ctx, ln, slots, nb); });
    case FV_KERNEL_SPARSE_CSR: return with_nb(STEP_NB, nb, [&](auto NB) { return launch_csr_nb<NB()>(ctx, ln, slots, nb); });
    case FV_KERNEL_CSR_F64: return with_nb(STEP_NB, nb, [&](auto NB) { return launch_csr_f64_nb<NB()>(ctx, ln, slots, nb); });
    case FV_KERNEL_F64_STREAM: return launch_step<double>(ctx, ln, slots, nb);
    case FV_KERNEL_F32_REFINE: return launch_step<float>(ctx, ln, slots, nb);
    case FV_KERNEL_Q16_REFINE: return launch_step<fvk::q16_t>(ctx, ln, slots, nb);
    default: return launch_step<fvk::half_t>(ctx, ln, slots, nb);
    }
}

// a decode's step launch: queued and counted (fv_last_stats).  A stream's steps are not a decode's: fvi::stream_step
// calls launch_step_kernel itself.
int queue_step(fv_ctx *ctx, const StepLaunch &ln, const fvk::TaskSlot *slots, int nb)
{
    if (int rc = launch_step_kernel(ctx, ln, slots, nb)) return rc;
    ctx->stats.step_launches += 1;
    ctx->stats.task_steps += nb;
    return 0;
}

template <typename K>
int set_big_lds(fv_ctx *ctx, K kernel)
{
    FV_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, fvk::LDS_LIMIT));
    return 0;
}

template <typename TA, int NB>
int allow_big_lds(fv_ctx *ctx)
{
    int rc = 0;
    if constexpr (std::is_same<TA, double>::value) {
        rc = set_big_lds(ctx, &fvk::trellis_step<TA, NB, U_DB64, true>);
    } else {
        constexpr int U = std::is_same<TA, float>::value ? U_DB32 : U_DB16;
        rc = set_big_lds(ctx, &fvk::trellis_step<TA, NB, U, true>);
        if constexpr (NB <= 2) { if (!rc) rc = set_big_lds(ctx, &fvk::trellis_step<TA, NB, U_UP, false>); }
    }
    return rc;
}

// largest batch whose score rows fit LDS next to the reduction scratch
// (u16_only: models beyond the float32 kernels' limit — rows of 16-bit codes)
int max_batch_for(int nrows, bool u16_only)
{
    int nb = fvk::MAX_BATCH;
    for (; nb > 1; nb >>= 1) {
        const int fits = with_nb(STEP_NB, nb, [&](auto NB) {
            return (u16_only ? fvk::u16_lds_bytes<NB(), 8>(nrows) : fvk::step_lds_bytes<NB()>(nrows)) <= (size_t)fvk::LDS_LIMIT ? 1 : 0;
        });
        if (fits) break;
    }
    return nb;
}

// The generation policy: how many tasks a step launch of a generation takes (cap) and how many streams its batches are
// dealt to (nstreams; 1: not forked) — for the generation driver, the flat form's admission and the checkpoint decode.
//
// The batches of a lock-step are independent, and a step launch is latency-bound at both ends (staging the score
// rows; reductions and refine): the right-hand generations of the packed 16-bit kernel therefore run as batches of
// FORK_CAP tasks dealt to FORK_STREAMS streams, small enough (36 KB of LDS, 81 VGPRs, 8 waves) for three workgroups
// of different launches to share a CU — one launch's head and tail run under the sweeps of the others.  cfg2
// right-hand passes 2.10 -> 1.85 ms, cfg3 62.7 -> 44.7 ms; the f32 filter in two co-resident 8-wave workgroups gave
// 1.96 / 53.0, batches of two tasks and four streams were slower, batches of three tasks too (2.16 / 54.9 ms).  The
// sparse walk gains the same way (cfg3 right-hand 33.4 -> 23.1 ms; at cfg2's 31-step passes nothing, so short
// generations stay on one stream and the host keeps running ahead).  FV_OPT_DEBUG bit 18: off.
// (Round 3, measured and not kept: the co-resident batches in ONE launch, gridDim.y = three batches of four, instead
// of three launches on three streams — no fork / join, a third of the host launches — cfg2 right-hand 1.64 -> 1.79 ms,
// cfg3 43.8 -> 51.1 ms: workgroups of one launch run in phase, all in their prologue or all in their sweep; what the
// streams provide is the stagger.)
constexpr int FORK_STREAMS = 3, FORK_CAP = 4;
struct GenShape { int cap, nstreams; };
// maxlen: steps of the longest pass; nfork: the passes that would be dealt (a generation's passes; the flat form's passes
// of more than one step); may_fork: nothing about the caller forbids a fork.
// all_streams — the one point where the callers differ: a generation of 5 to 8 passes makes two batches of FORK_CAP, and the
// generation driver (false) opens a stream per batch, two; the flat form (true) takes FORK_STREAMS whenever it forks,
// which its plan (build_flat) and the plan's key are made for.  Whether two would serve it as well has not been measured.
GenShape generation_shape(const fv_ctx *ctx, int kernel, int maxlen, int nfork, bool may_fork, bool all_streams)
{
    // (the float64 kernel beyond one LDS row sweeps slabs of source rows: four tasks per launch keep a slab at ~10000 rows)
    const bool slabbed = (kernel == FV_KERNEL_F64_STREAM || kernel == FV_KERNEL_Q16_REFINE) && !ctx->full_ok;
    const bool walk = kernel == FV_KERNEL_SPARSE_Q16 || kernel == FV_KERNEL_SPARSE_CSR || kernel == FV_KERNEL_CSR_F64;
    GenShape g{ std::max(1, std::min(ctx->opt_max_batch, slabbed ? 4 : max_batch_for(ctx->nrows, !ctx->full_ok))), 1 };
    if (kernel == FV_KERNEL_SPARSE_CSR || kernel == FV_KERNEL_CSR_F64) g.cap = ctx->opt_max_batch;     // (rows that do not fit LDS are read from memory)
    if (may_fork && !(ctx->opt_debug & FV_DBG_FULL_ONE_STREAM) && nfork > FORK_CAP && ((kernel == FV_KERNEL_U16_REFINE && ctx->u16_ok) || (walk && maxlen >= 64))) {
        g.cap = std::min(g.cap, FORK_CAP);
        g.nstreams = all_streams ? FORK_STREAMS : std::min(FORK_STREAMS, (nfork + FORK_CAP - 1) / FORK_CAP);
    }
    return g;
}

inline hipStream_t stream_of(const fv_ctx *ctx, int sid) { return sid ? ctx->aux[sid - 1] : ctx->stream; }

// Fork: streams 1 .. n - 1 wait for what the main stream holds so far.
int fork_streams(fv_ctx *ctx, int n)
{
    // no packets may wait on the other queues while a serial generation runs (decode_beam_impl has the measurement)
    // (polled: a blocking hipStreamSynchronize wakes the host ~30 us after the stream has drained, and the chip idles
    // until the first forked launch arrives)
    if (!ctx->fork_active) {
        hipError_t qe;
        while ((qe = hipStreamQuery(ctx->stream)) == hipErrorNotReady) std::this_thread::yield();
        FV_HIP(qe);
    }
    ctx->fork_active = true;
    FV_HIP(hipEventRecord(ctx->ev_fork, ctx->stream));
    for (int q = 1; q < n; ++q) FV_HIP(hipStreamWaitEvent(stream_of(ctx, q), ctx->ev_fork, 0));
    return 0;
}

// ... and the join: the main stream waits for each of them
int join_streams(fv_ctx *ctx, int n)
{
    for (int q = 1; q < n; ++q) {
        FV_HIP(hipEventRecord(ctx->ev_join[q - 1], stream_of(ctx, q)));
        FV_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_join[q - 1], 0));
    }
    return 0;
}

// init_rows / init_rows_csr over one chunk of passes, on the main stream: the first score row of each pass into
// rows + PassDesc::row_off, from Pi or from the state `ans` holds at L - 1, with the emission term lb64[sym[L] * K + i]
// (sym on the device).  coded: the rows' 16-bit codes and tile maxima beside them (init_rows_coded).
int launch_init(fv_ctx *ctx, const fvk::PassChunk &ch, const int *ans, float *rows, const double *lb64, const int *sym, bool coded)
{
    const int K = ctx->K;
    if (ctx->csr)
        hipLaunchKernelGGL(fvk::init_rows_csr, dim3((K + 255) / 256, ch.n), dim3(256), 0, ctx->stream, ch, ctx->CRptr.p,
                           ctx->CRcol.p, ctx->CRlog.p, lb64, ctx->LPi64.p, sym, ans, rows, K);
    else
        hipLaunchKernelGGL(fvk::init_rows, dim3((K + 255) / 256, ch.n), dim3(256), 0, ctx->stream, ch, ctx->LA64.p, ctx->nrows,
                           lb64, ctx->LPi64.p, sym, ans, rows, K, coded ? ctx->d_rcodes.p : nullptr,
                           coded ? ctx->d_rtmax.p : nullptr, -1.0f / ctx->qscale);
    FV_HIP(hipGetLastError());
    return 0;
}

// the slot of one task step: the rows it reads and writes, the emission rows of the symbol at time j, the arg row it leaves
fvk::TaskSlot task_slot(const fv_ctx *ctx, const float *in, float *out, int j, int *arg_row)
{
    fvk::TaskSlot sl;
    sl.t1_in = in; sl.t1_out = out; sl.bp_out = arg_row;
    sl.tmp_row = ctx->view.lb32 + (size_t)ctx->h_ob[j] * ctx->K;
    sl.tmp64_row = ctx->view.lb64 + (size_t)ctx->h_ob[j] * ctx->K;
    return sl;
}

// Single-column last steps of passes that finish (fvk::last_column: the one column the back-track reads), collected and
// flushed COL_CHUNK jobs per launch to one stream; `ans` holds the passes' end states (d_ans, or the flat form's snapshot).
struct ColumnQueue {
    fv_ctx *ctx;
    hipStream_t stream;
    fvk::ColArgs c;
    ColumnQueue(fv_ctx *ctx_, hipStream_t st, const int *ans) : ctx(ctx_), stream(st)
    {
        c.LA64 = ctx->LA64.p; c.ans = ans; c.K = ctx->K; c.nrows = ctx->nrows; c.n = 0;
    }
    // the pass that ends at time R: its last row but one, the arg row its column goes to
    int add(const float *row, int R, int *arg_row)
    {
        c.p[c.n++] = fvk::ColJob{ row, ctx->view.lb32 + (size_t)ctx->h_ob[R] * ctx->K, arg_row, R };
        return c.n == fvk::COL_CHUNK ? flush() : 0;
    }
    int flush()
    {
        if (c.n == 0) return 0;
        if (ctx->csr) {
            fvk::CsrColArgs cc;
            cc.ck = ctx->CSk.p; cc.c64 = ctx->CS64.p; cc.tile_off = ctx->CSoff.p; cc.tile_nwb = ctx->CSnwb.p;
            cc.ans = c.ans; cc.K = c.K; cc.n = c.n;
            std::copy(c.p, c.p + c.n, cc.p);
            hipLaunchKernelGGL(fvk::last_column_csr, dim3(c.n), dim3(256), 0, stream, cc);
        } else
            hipLaunchKernelGGL(fvk::last_column, dim3(c.n), dim3(256), 0, stream, c);
        FV_HIP(hipGetLastError());
        ctx->stats.column_steps += c.n;
        c.n = 0;
        return 0;
    }
};

// the end pick of a single whole-sequence pass on its last row, into *end / *score ...
int end_pick(fv_ctx *ctx, const float *row, int *end, float *score)
{
    hipLaunchKernelGGL(fvk::final_argmax, dim3(1), dim3(1024), 0, ctx->stream, row, ctx->K, end, score);
    FV_HIP(hipGetLastError());
    return 0;
}

// ... and its back-track from path[R] through the arg rows (row j of `bp`: time j) into path[0 .. R - 1]
int backtrack_whole(fv_ctx *ctx, const int *bp, int R, int *path, unsigned long long *restarts)
{
    fvk::PassChunk ch;
    ch.n = 1;
    ch.p[0] = fvk::PassDesc{ 0, R, 1, 1, 0 };
    hipLaunchKernelGGL(fvk::backtrack, dim3(1), dim3(64), 0, ctx->stream, ch, bp, ctx->K, path, restarts);
    FV_HIP(hipGetLastError());
    return 0;
}

int prof_event(fv_ctx *ctx, size_t idx, hipEvent_t *out)
{
    while (ctx->prof_events.size() <= idx) {
        hipEvent_t e;
        FV_HIP(hipEventCreate(&e));
        ctx->prof_events.push_back(e);
    }
    *out = ctx->prof_events[idx];
    return 0;
}

// Runs every pass of one generation in lock-step: at lock-step s each still-active pass advances
// from time L+s-1 to L+s.  Passes are sorted longest first so the active set is a prefix.
// batch: 0 a single-sequence decode; else a generation of fv_decode_full_batch (passes of several sequences on one
// concatenated time axis; the whole-sequence passes write their scores to d_score[seq]) — BATCH_FORK: its generation 0
// takes the three-stream form of the right-hand generations, BATCH_SERIAL: it stays on one stream.
enum { BATCH_NONE = 0, BATCH_SERIAL = 1, BATCH_FORK = 2 };
int run_generation_full(fv_ctx *ctx, std::vector<fv::Pass> &passes, int kernel, size_t &nprof, int batch = BATCH_NONE)
{
    const int K = ctx->K;
    const int np = (int)passes.size();
    if (np == 0) return 0;
    std::stable_sort(passes.begin(), passes.end(),
                     [](const fv::Pass &a, const fv::Pass &b) { return a.R - a.L > b.R - b.L; });
    // init rows
    for (int base = 0; base < np; base += fvk::PASS_CHUNK) {
        fvk::PassChunk ch;
        ch.n = std::min(fvk::PASS_CHUNK, np - base);
        for (int q = 0; q < ch.n; ++q) {
            const fv::Pass &p = passes[base + q];
            ch.p[q] = fvk::PassDesc{ p.L, p.R, p.from_pi ? 1 : 0, p.whole ? 1 : 0, (long long)(base + q) * 2 * ctx->nrows };
        }
        if (int rc = launch_init(ctx, ch, ctx->d_ans.p, ctx->d_rows.p, ctx->view.lb64, ctx->d_ob.p, init_rows_coded(ctx, base, ch.n))) return rc;
    }
    const int maxlen = passes[0].R - passes[0].L;
    const bool whole_gen = passes[0].whole;       // generation 0: bracket its step launches for the stats
    // (a generation 0 forks only as a batch's; nothing that brackets or captures single launches forks)
    const bool may_fork = (!whole_gen || batch == BATCH_FORK) && !ctx->opt_profile && !(ctx->opt_debug & FV_DBG_GRAPH);
    const GenShape shape = generation_shape(ctx, kernel, maxlen, np, may_fork, false);
    const int cap = shape.cap, nstreams = shape.nstreams;
    const bool two = nstreams > 1;
    if (two) { if (int rc = fork_streams(ctx, nstreams)) return rc; }
    const bool col_last = !(ctx->opt_debug & FV_DBG_FULL_LAST_STEP);  // FV_OPT_DEBUG bit 3: run every last step as a full step
    // FV_OPT_DEBUG bit 6 (experiment): capture this generation's step launches into a hipGraph and replay it
    const bool use_graph = (ctx->opt_debug & FV_DBG_GRAPH) && !ctx->opt_profile;
    if (use_graph) FV_HIP(hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal));
    if (whole_gen && !use_graph) FV_HIP(hipEventRecord(ctx->ev_s0, ctx->stream));
    // passes are sorted longest first: at lock-step s the passes with len >= s are a prefix; those with
    // len == s are finishing and (unless they are the whole-sequence pass) only need one column
    int active = np;
    for (int s = 1; s <= maxlen; ++s) {
        while (active > 0 && passes[active - 1].R - passes[active - 1].L < s) --active;
        int full = active;                           // passes [0, full) take a full step
        if (col_last) while (full > 0 && passes[full - 1].R - passes[full - 1].L == s && !passes[full - 1].whole) --full;
        auto row = [&](int q, int parity) { return ctx->d_rows.p + (size_t)q * 2 * ctx->nrows + (size_t)parity * ctx->nrows; };
        for (int base = 0; base < full; base += cap) {
            const int nb = std::min(cap, full - base);
            fvk::TaskSlot slots[fvk::MAX_BATCH];
            for (int q = 0; q < nb; ++q) {
                const int j = passes[base + q].L + s;
                slots[q] = task_slot(ctx, row(base + q, (s - 1) & 1), row(base + q, s & 1), j, ctx->d_bp.p + (size_t)j * K);
            }
            hipEvent_t e0 = nullptr, e1 = nullptr;
            if (ctx->opt_profile) {
                int rc = prof_event(ctx, nprof, &e0); if (rc) return rc;
                rc = prof_event(ctx, nprof + 1, &e1); if (rc) return rc;
                nprof += 2;
                FV_HIP(hipEventRecord(e0, ctx->stream));
            }
            const int sid = two ? (base / cap) % nstreams : 0;           // batch b keeps its stream for the whole generation
            if (int rc = queue_step(ctx, StepLaunch{ kernel, stream_of(ctx, sid), two, s & 1 }, slots, nb)) return rc;
            if (ctx->opt_profile) FV_HIP(hipEventRecord(e1, ctx->stream));
        }
        // Single-column last steps of the passes that finish at this lock-step.  A pass's row was written by the stream its
        // batch keeps for the whole generation (or, at lock-step 1, by init_rows on the main stream), so its last step goes
        // to that very stream: no cross-stream join in the middle of a generation (a join cost ~10 us of host time, and
        // the dependency between queues left the chip idle for 15-50 us at each of the 24 of a cfg2 decode).
        for (int sid = 0; sid < nstreams && full < active; ++sid) {
            ColumnQueue cols(ctx, stream_of(ctx, sid), ctx->d_ans.p);
            for (int q = full; q < active; ++q) {
                const int owner = (two && s > 1) ? (q / cap) % nstreams : 0;
                if (owner != sid) continue;
                if (int rc = cols.add(row(q, (s - 1) & 1), passes[q].R, ctx->d_bp.p + (size_t)passes[q].R * K)) return rc;
            }
            if (int rc = cols.flush()) return rc;
        }
    }
    if (use_graph) {
        hipGraph_t g = nullptr;
        FV_HIP(hipStreamEndCapture(ctx->stream, &g));
        hipGraphExec_t ge = nullptr;
        FV_HIP(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
        if (whole_gen) FV_HIP(hipEventRecord(ctx->ev_s0, ctx->stream));
        FV_HIP(hipGraphLaunch(ge, ctx->stream));
        ctx->graphs.push_back(ge);
        (void)hipGraphDestroy(g);
    }
    if (whole_gen && !two) FV_HIP(hipEventRecord(ctx->ev_s1, ctx->stream));
    if (two) { if (int rc = join_streams(ctx, nstreams)) return rc; }
    if (whole_gen && two) FV_HIP(hipEventRecord(ctx->ev_s1, ctx->stream));      // (a batch's forked generation 0: after the join)
    // end states + chains
    if (batch) {
        // one launch for the end picks of all whole-sequence passes (one per sequence), a workgroup each
        fvk::ArgmaxArgs a;
        a.rows = ctx->d_rows.p; a.ans = ctx->d_ans.p; a.score = ctx->d_score.p; a.K = K; a.nrows = ctx->nrows; a.n = 0;
        auto flush = [&]() -> int {
            if (a.n == 0) return 0;
            hipLaunchKernelGGL(fvk::final_argmax_batch, dim3(a.n), dim3(1024), 0, ctx->stream, a);
            FV_HIP(hipGetLastError());
            a.n = 0;
            return 0;
        };
        for (int q = 0; q < np; ++q) {
            if (!passes[q].whole) continue;
            const int len = passes[q].R - passes[q].L;
            a.j[a.n++] = fvk::ArgmaxJob{ q * 2 + (len & 1), passes[q].R, passes[q].seq };
            if (a.n == fvk::ARGMAX_CHUNK) { int rc = flush(); if (rc) return rc; }
        }
        int rc = flush();
        if (rc) return rc;
    }
    for (int q = 0; q < np && !batch; ++q) {
        if (!passes[q].whole) continue;
        const int len = passes[q].R - passes[q].L;
        const float *last = ctx->d_rows.p + (size_t)q * 2 * ctx->nrows + (size_t)(len & 1) * ctx->nrows;
        if (int rc = end_pick(ctx, last, ctx->d_ans.p + passes[q].R, ctx->d_score.p)) return rc;
    }
    for (int base = 0; base < np; base += fvk::PASS_CHUNK) {
        fvk::PassChunk ch;
        ch.n = std::min(fvk::PASS_CHUNK, np - base);
        for (int q = 0; q < ch.n; ++q) {
            const fv::Pass &p = passes[base + q];
            ch.p[q] = fvk::PassDesc{ p.L, p.R, p.from_pi ? 1 : 0, p.whole ? 1 : 0, 0 };
        }
        hipLaunchKernelGGL(fvk::backtrack, dim3(ch.n), dim3(64), 0, ctx->stream, ch, ctx->d_bp.p, K, ctx->d_ans.p,
                           ctx->d_counters.p + fvk::BT_COUNTER);
        FV_HIP(hipGetLastError());
    }
    return 0;
}

// FV_OPT_FLAT_GENERATIONS — the right-hand passes of ALL generations as one independent set.
//
// run_generation_full orders the generations because generation g + 1 reads Ans[L-1] and Ans[R] from generation g's
// back-track.  Those two states are, in practice, the ones the whole-sequence chain already holds there, so after
// generation 0 every right-hand pass is started from a snapshot S of that chain: one init_rows, the step launches of all
// passes dealt to the streams by length (a pass is at most T / 4 steps long: 31 dependent lock-steps at cfg2 instead of
// 57), one back-track launch into per-pass chain slots, and a one-workgroup resolver that commits the chains generation
// by generation while S agrees with the committed answers.  A pass is a deterministic function of (L, R, start state,
// end state, observations): where the resolver commits, every bit is the generation-by-generation result; where it
// stops (counter FLAT_COUNTER), decode_full_impl runs the remaining generations the old way.
// Its launches take the winning form of a forked generation (generation_shape: batches of FORK_CAP on FORK_STREAMS streams).
// auto: from the smallest measured K at which the flat form wins, and up to the longest measured T at which it does — long
// sequences keep their launch slots full generation by generation, have nothing to gain, and the more passes a decode
// has the likelier one of them mis-speculates (cfg3, T = 4096: 2 of 4095, which costs the whole fall-back)
constexpr int FLAT_AUTO_MIN_K = 512, FLAT_AUTO_MAX_T = 1024;

int run_flat_full(fv_ctx *ctx, int kernel, int T)
{
    const fv::FlatPlan &fp = ctx->flat_plan;
    const int K = ctx->K, np = (int)fp.passes.size(), nstreams = fp.nstreams;
    const bool two = nstreams > 1;
    auto row = [&](int i, int parity) { return ctx->d_rows.p + (size_t)i * 2 * ctx->nrows + (size_t)parity * ctx->nrows; };
    auto arg_rows = [&](const fv::FlatPass &p) { return p.arg_row < 0 ? ctx->d_bp.p + (size_t)(p.L + 1) * K : ctx->d_flat_bp.p + (size_t)p.arg_row * K; };
    // pass table (kept on the device across decodes of one plan)
    if (ctx->flat_uploaded != ctx->d_flat.p) {
        std::vector<fvk::FlatDesc> table((size_t)np);
        for (int i = 0; i < np; ++i) table[(size_t)i] = fvk::FlatDesc{ fp.passes[i].L, fp.passes[i].R, fp.passes[i].generation, fp.passes[i].chain, fp.passes[i].arg_row };
        FV_HIP(hipMemcpyAsync(ctx->d_flat.p, table.data(), (size_t)np * sizeof(fvk::FlatDesc), hipMemcpyHostToDevice, ctx->stream));
        FV_HIP(hipStreamSynchronize(ctx->stream));       // (once per plan: `table` is gone after this scope)
        ctx->flat_uploaded = ctx->d_flat.p;
    }
    hipLaunchKernelGGL(fvk::flat_snapshot, dim3((T + 255) / 256), dim3(256), 0, ctx->stream, ctx->d_ans.p, ctx->d_snap.p, T, ctx->flat_poison, K);
    FV_HIP(hipGetLastError());
    // init rows of every pass, from S
    for (int base = 0; base < np; base += fvk::PASS_CHUNK) {
        fvk::PassChunk ch;
        ch.n = std::min(fvk::PASS_CHUNK, np - base);
        for (int q = 0; q < ch.n; ++q) ch.p[q] = fvk::PassDesc{ fp.passes[base + q].L, fp.passes[base + q].R, 0, 0, (long long)(base + q) * 2 * ctx->nrows };
        if (int rc = launch_init(ctx, ch, ctx->d_snap.p, ctx->d_rows.p, ctx->view.lb64, ctx->d_ob.p, init_rows_coded(ctx, base, ch.n))) return rc;
    }
    if (two) { if (int rc = fork_streams(ctx, nstreams)) return rc; }
    const bool col_last = !(ctx->opt_debug & FV_DBG_FULL_LAST_STEP);
    // single-column last steps of a set of passes, on one stream
    auto columns = [&](const std::vector<int> &which, hipStream_t st) -> int {
        ColumnQueue cols(ctx, st, ctx->d_snap.p);
        for (int i : which) {
            const fv::FlatPass &p = fp.passes[i];
            const int len = p.R - p.L;
            if (int rc = cols.add(row(i, (len - 1) & 1), p.R, arg_rows(p) + (size_t)(len - 1) * K)) return rc;
        }
        return cols.flush();
    };
    // Every stream walks its batches one after the other (a batch keeps its stream); the host deals its launches to the
    // streams in turn, so that each queue always holds work.
    struct Cursor { size_t b = 0; int s = 1; };
    Cursor cur[FORK_STREAMS];
    for (bool any = true; any;) {
        any = false;
        for (int sid = 0; sid < nstreams; ++sid) {
            Cursor &c = cur[sid];
            const std::vector<int> &mine = fp.stream_batches[(size_t)sid];
            if (c.b >= mine.size()) continue;
            any = true;
            const fv::FlatBatch &bt = fp.batches[(size_t)mine[c.b]];
            const int s = c.s;
            // passes are sorted longest first: those with more than s steps take a full step, those with exactly s finish
            // with their single column (FV_OPT_DEBUG bit 3: with a full step as well)
            int nb = 0;
            std::vector<int> done;
            fvk::TaskSlot slots[fvk::MAX_BATCH];
            for (int i : bt.pass) {
                const fv::FlatPass &p = fp.passes[i];
                const int len = p.R - p.L;
                if (len < s) continue;
                if (len == s && col_last) { done.push_back(i); continue; }
                slots[nb++] = task_slot(ctx, row(i, (s - 1) & 1), row(i, s & 1), p.L + s, arg_rows(p) + (size_t)(s - 1) * K);
            }
            if (nb) { if (int rc = queue_step(ctx, StepLaunch{ kernel, stream_of(ctx, sid), two, s & 1 }, slots, nb)) return rc; }
            if (!done.empty()) { if (int rc = columns(done, stream_of(ctx, sid))) return rc; }
            if (++c.s > bt.len) { ++c.b; c.s = 1; }
        }
    }
    // the one-step passes: column jobs only
    for (int sid = 0; sid < nstreams; ++sid) {
        std::vector<int> ones;
        for (int i = 0; i < np; ++i) if (fp.passes[i].batch < 0 && fp.passes[i].stream == sid) ones.push_back(i);
        if (ones.empty()) continue;
        if (col_last) { const int rc = columns(ones, stream_of(ctx, sid)); if (rc) return rc; continue; }
        const size_t cap = (size_t)std::max(1, ctx->flat_key[2]);
        for (size_t base = 0; base < ones.size(); base += cap) {      // FV_OPT_DEBUG bit 3: as full steps
            const int nb = (int)std::min(cap, ones.size() - base);
            fvk::TaskSlot slots[fvk::MAX_BATCH];
            for (int q = 0; q < nb; ++q) {
                const int i = ones[base + q];
                slots[q] = task_slot(ctx, row(i, 0), row(i, 1), fp.passes[i].R, arg_rows(fp.passes[i]));
            }
            if (int rc = queue_step(ctx, StepLaunch{ kernel, stream_of(ctx, sid), two, 1 }, slots, nb)) return rc;
        }
    }
    if (int rc = join_streams(ctx, nstreams)) return rc;
    // every chain in one launch, then the resolver
    hipLaunchKernelGGL(fvk::backtrack_flat, dim3(np), dim3(64), 0, ctx->stream, ctx->d_flat.p, ctx->d_bp.p, ctx->d_flat_bp.p, K,
                       ctx->d_snap.p, ctx->d_chain.p, ctx->d_counters.p + fvk::BT_COUNTER);
    FV_HIP(hipGetLastError());
    fvk::FlatGens gens;
    gens.ngen = (int)fp.gen_begin.size() - 1;
    for (int g = 0; g <= gens.ngen; ++g) gens.begin[g] = fp.gen_begin[(size_t)g];
    hipLaunchKernelGGL(fvk::flat_resolve, dim3(1), dim3(1024), 0, ctx->stream, ctx->d_flat.p, gens, ctx->d_snap.p, ctx->d_chain.p,
                       ctx->d_ans.p, ctx->d_counters.p + fvk::FLAT_COUNTER);
    FV_HIP(hipGetLastError());
    ctx->stats.passes += np;
    ctx->stats.flat_passes = np;
    return 0;
}

}  // namespace

namespace fvi {

// every full-state step kernel launched with its score rows in LDS may use the whole of it (LDS_LIMIT): per task count
// the four dense tables' forms (allow_big_lds), the three walks in their LDS form and the packed kernel's four forms
template <int NB>
int setup_nb(fv_ctx *ctx)
{
    int rc = 0;
    if ((rc = allow_big_lds<float, NB>(ctx)) || (rc = allow_big_lds<double, NB>(ctx)) || (rc = allow_big_lds<fvk::half_t, NB>(ctx)) ||
        (rc = allow_big_lds<fvk::q16_t, NB>(ctx)) || (rc = set_big_lds(ctx, &fvk::trellis_step_sparse<NB>)) ||
        (rc = set_big_lds(ctx, &fvk::trellis_step_csr<NB, false>)) || (rc = set_big_lds(ctx, &fvk::trellis_step_csr_f64<NB, false>)) ||
        (rc = set_big_lds(ctx, &fvk::trellis_step_u16<NB, 8, false, 16>)) || (rc = set_big_lds(ctx, &fvk::trellis_step_u16<NB, U_DB16, true, 16>)) ||
        (rc = set_big_lds(ctx, &fvk::trellis_step_u16<NB, 16, false, 8>)) || (rc = set_big_lds(ctx, &fvk::trellis_step_u16<NB, U_DB16, true, 8>)))
        return rc;
    // the forms without the FV_OPT_ROW_CODES code (launch_u16_variant)
    if constexpr (U16_CODE_FREE<NB>) {
        if ((rc = set_big_lds(ctx, &fvk::trellis_step_u16<NB, 8, false, 16, false>)) || (rc = set_big_lds(ctx, &fvk::trellis_step_u16<NB, U_DB16, true, 16, false>)) ||
            (rc = set_big_lds(ctx, &fvk::trellis_step_u16<NB, 16, false, 8, false>)) || (rc = set_big_lds(ctx, &fvk::trellis_step_u16<NB, U_DB16, true, 8, false>)))
            return rc;
    }
    return 0;
}

template <int... NB>
int setup_all(fv_ctx *ctx, NbList<NB...>)
{
    int rc = 0;
    (void)(((rc = setup_nb<NB>(ctx)) != 0) || ...);
    return rc;
}

int full_setup(fv_ctx *ctx) { return setup_all(ctx, STEP_NB); }

int launch_init_rows(fv_ctx *ctx, const fvk::PassChunk &ch, float *rows)
{
    // (ctx->csr here: a beam decode of a sparse-set model, FV_OPT_SPARSE_BEAM)
    return launch_init(ctx, ch, ctx->d_ans.p, rows, ctx->view.lb64, ctx->d_ob.p, false);
}

// Workgroups of EMIS_BLOCK states by rows, about 2048 in all (eight per CU); the kernel strides over the rest.
template <typename TIN>
static void launch_stage_as(fv_ctx *ctx, const void *src, long long ld, int T, const int *map, dim3 grid, float *E32, double *E64,
                            unsigned long long *flags)
{
    if (map)
        hipLaunchKernelGGL((fvk::stage_emissions<TIN, true>), grid, dim3(fvk::EMIS_BLOCK), 0, ctx->stream,
                           static_cast<const TIN *>(src), ld, T, ctx->K, map, E32, E64, flags);
    else
        hipLaunchKernelGGL((fvk::stage_emissions<TIN, false>), grid, dim3(fvk::EMIS_BLOCK), 0, ctx->stream,
                           static_cast<const TIN *>(src), ld, T, ctx->K, map, E32, E64, flags);
}

// while an emission map is set: the tied form, rows of P scores gathered through the K entries of the map
int launch_stage_emissions(fv_ctx *ctx, const void *src, int dtype, long long ld, int T, float *E32, double *E64, unsigned long long *flags)
{
    const int K = ctx->K;
    const int gx = std::min((K + fvk::EMIS_BLOCK - 1) / fvk::EMIS_BLOCK, 2048), gy = std::max(1, std::min(T, 2048 / gx));
    const int *map = ctx->emis_P > 0 ? ctx->EMap.p : nullptr;
    switch (dtype) {
    case FV_EMIS_LOG_F64: launch_stage_as<double>(ctx, src, ld, T, map, dim3(gx, gy), E32, E64, flags); break;
    case FV_EMIS_LOG_F32: launch_stage_as<float>(ctx, src, ld, T, map, dim3(gx, gy), E32, E64, flags); break;
    case FV_EMIS_LOG_F16: launch_stage_as<_Float16>(ctx, src, ld, T, map, dim3(gx, gy), E32, E64, flags); break;
    case FV_EMIS_LOG_BF16: launch_stage_as<fvk::bf16_bits>(ctx, src, ld, T, map, dim3(gx, gy), E32, E64, flags); break;
    default: ctx->detail = "fv_set_emissions: unknown dtype"; return FV_ERR_ARG;
    }
    FV_HIP(hipGetLastError());
    return 0;
}

// ---- what fv_stream.hip takes from this file (fv_internal.h)

int stream_init_row(fv_ctx *ctx, const double *lb64, const int *sym, float *row)
{
    fvk::PassChunk ch;
    ch.n = 1;
    ch.p[0] = fvk::PassDesc{ 0, 0, 1, 1, 0 };
    return launch_init(ctx, ch, sym, row, lb64, sym, false);      // (from Pi: no answer is read)
}

// (the stream's own rows and emission tables; the bare launch — a stream's steps are not counted as a decode's)
int stream_step(fv_ctx *ctx, int kernel, const float *t1_in, float *t1_out, const float *tmp_row, const double *tmp64_row,
                int *bp_out, int reverse)
{
    fvk::TaskSlot sl;
    sl.t1_in = t1_in; sl.t1_out = t1_out; sl.bp_out = bp_out; sl.tmp_row = tmp_row; sl.tmp64_row = tmp64_row;
    return launch_step_kernel(ctx, StepLaunch{ kernel, ctx->stream, false, reverse }, &sl, 1);
}

int stream_step_batch(fv_ctx *ctx, int kernel, const StreamTask *tasks, int nb, int reverse)
{
    fvk::TaskSlot slots[fvk::MAX_BATCH];
    if (nb < 1 || nb > fvk::MAX_BATCH) return FV_ERR_ARG;
    for (int q = 0; q < nb; ++q) {
        slots[q].t1_in = tasks[q].t1_in; slots[q].t1_out = tasks[q].t1_out; slots[q].bp_out = tasks[q].bp_out;
        slots[q].tmp_row = tasks[q].tmp_row; slots[q].tmp64_row = tasks[q].tmp64_row;
    }
    return launch_step_kernel(ctx, StepLaunch{ kernel, ctx->stream, false, reverse }, slots, nb);
}

// (one stream: nothing is forked)
int stream_batch_cap(const fv_ctx *ctx, int kernel) { return std::min(generation_shape(ctx, kernel, 0, 0, false, false).cap, fvk::MAX_BATCH); }

int stream_end_pick(fv_ctx *ctx, const float *row, int *end, float *score) { return end_pick(ctx, row, end, score); }

int stream_backtrack(fv_ctx *ctx, const int *bp, int R, int *path, unsigned long long *restarts)
{
    return backtrack_whole(ctx, bp, R, path, restarts);
}

}  // namespace fvi

namespace {
int decode_full_impl(fv_ctx *ctx, const int *ob, int T, int n_split, int mode, int *path_out, float *score_out);
int decode_checkpoint_impl(fv_ctx *ctx, const int *ob, int T, int step, int *path_out, float *score_out);
}  // namespace

extern "C" int fv_decode_full(fv_ctx *ctx, const int *ob, int T, int n_split, int mode, int *path_out, float *score_out)
{
    if (!ctx) return FV_ERR_ARG;
    FV_NO_STREAM(ctx);
    if (ctx->group && ctx->group_rank == 0 && !ctx->vanilla) {
        // multi-device context: every member decodes its share on its own device and host thread, one gather merges them
        if (!path_out || T < 2) return FV_ERR_ARG;
        return fvi::group_run(ctx, T, path_out, score_out, [&](fv_ctx *m, int *path, float *score) {
            return fvi::drained(m, decode_full_impl(m, ob, T, n_split, mode, path, score));
        });
    }
    return fvi::drained(ctx, decode_full_impl(ctx, ob, T, n_split, mode, path_out, score_out));
}

namespace {
int decode_full_batch_impl(fv_ctx *ctx, const int *ob, const long long *offsets, int nseq, int n_split, int mode, int *path_out,
                           float *score_out, int *status_out);
}  // namespace

extern "C" int fv_decode_full_batch(fv_ctx *ctx, const int *ob, const long long *offsets, int nseq, int n_split, int mode,
                                    int *path_out, float *score_out, int *status_out)
{
    if (!ctx) return FV_ERR_ARG;
    FV_NO_STREAM(ctx);
    if (ctx->group || ctx->comm || ctx->nranks > 1) {
        ctx->detail = "fv_decode_full_batch: one device, no communicator and no partition (sequences are not dealt to ranks)";
        return FV_ERR_UNSUPPORTED;
    }
    return fvi::drained(ctx, decode_full_batch_impl(ctx, ob, offsets, nseq, n_split, mode, path_out, score_out, status_out));
}

namespace {
// What fv_decode_full and fv_test_forward do before their passes run, through this one path: admission of the kernel
// choice for the model and of the sequence, the kernel choice itself, the 16-bit table of a model beyond the float32
// kernels' limit (built on the device on first use) and the workspace for `rows_needed` passes in flight.  (The LDS
// attributes of every step kernel, fvi::full_setup, are set once by fv_create.)
// admit_full: the admission and the choice, in the order the refusals have always come in (ob == NULL: no sequence to
// check — fvi::stream_admit, whose symbols arrive push by push).  prepare_full: that, then workspace and row codes.
int admit_full(fv_ctx *ctx, const int *ob, int T, int &kernel)
{
    // Beyond the float32 kernels' LDS limit (one score row of K floats) two routes remain:
    //   * the packed 16-bit kernel — a row of 16-bit score codes is half the bytes (K <= 65536); it needs every model entry
    //     in [0,1], and its table is built on the device on first use;
    //   * the float64 kernel in slabs of source rows (launch_step_nb): any K the float64 table fits the device for, any
    //     model; 8 B per cell instead of 2.
    if (ctx->csr) {
        // a model set by fv_set_model_sparse has no dense table: the walks over its stored entries are its kernels — the
        // filter walk, or under FV_KERNEL_CSR_F64 the float64 walk, which has no condition on the values
        const bool f64 = ctx->opt_kernel == FV_KERNEL_CSR_F64;
        if (!f64 && ctx->opt_kernel != FV_KERNEL_AUTO && ctx->opt_kernel != FV_KERNEL_SPARSE_Q16) {
            ctx->detail = "a model set by fv_set_model_sparse has no dense table: FV_KERNEL_AUTO or FV_KERNEL_SPARSE_Q16 (the filter walk), or FV_KERNEL_CSR_F64";
            return FV_ERR_UNSUPPORTED;
        }
        if (!f64 && !ctx->view.logs_nonpositive) {
            ctx->detail = fvi::filter_range_detail(ctx);
            return FV_ERR_UNSUPPORTED;
        }
        for (int j = 0; ob && j < T; ++j) if (ob[j] < 0 || ob[j] >= ctx->view.nsym) return FV_ERR_ARG;
        FV_HIP(hipSetDevice(ctx->device));
        kernel = f64 ? FV_KERNEL_CSR_F64 : FV_KERNEL_SPARSE_CSR;
        return 0;
    }
    if (ctx->opt_kernel == FV_KERNEL_CSR_F64) {
        ctx->detail = "FV_KERNEL_CSR_F64 walks the stored entries of a model set by fv_set_model_sparse: this model was set by fv_set_model";
        return FV_ERR_UNSUPPORTED;
    }
    const bool wide = !ctx->full_ok;
    const bool big = wide && ctx->u16_ok && ctx->view.logs_nonpositive && !ctx->vanilla &&
                     (ctx->opt_kernel == FV_KERNEL_AUTO || ctx->opt_kernel == FV_KERNEL_U16_REFINE);
    // ... and the same slabs for the f32 filter on the 16-bit table (2 B per cell; model entries in [0,1]): what AUTO takes
    // beyond K = 65536
    const bool wide_q16 = wide && !big && ctx->view.logs_nonpositive && !ctx->vanilla &&
                          (ctx->opt_kernel == FV_KERNEL_AUTO || ctx->opt_kernel == FV_KERNEL_Q16_REFINE);
    if (wide && !big && !wide_q16 && !(ctx->opt_kernel == FV_KERNEL_AUTO || ctx->opt_kernel == FV_KERNEL_F64_STREAM)) {
        ctx->detail = "full-state decode of K > ~40100: FV_KERNEL_AUTO, FV_KERNEL_U16_REFINE (K <= 65536), FV_KERNEL_Q16_REFINE (both: model entries in [0,1]) or FV_KERNEL_F64_STREAM";
        return FV_ERR_UNSUPPORTED;
    }
    for (int j = 0; ob && j < T; ++j) if (ob[j] < 0 || ob[j] >= ctx->view.nsym) return FV_ERR_ARG;
    if (ctx->opt_kernel >= FV_KERNEL_F32_REFINE && !ctx->view.logs_nonpositive) {
        ctx->detail = fvi::filter_range_detail(ctx);
        return FV_ERR_UNSUPPORTED;
    }
    FV_HIP(hipSetDevice(ctx->device));
    kernel = big ? FV_KERNEL_U16_REFINE : wide_q16 ? FV_KERNEL_Q16_REFINE : wide ? FV_KERNEL_F64_STREAM : pick_kernel(ctx);
    if ((big || wide_q16) && !ctx->laq16_ready) {      // (the flag, not the pointer: a build that failed half way leaves the buffer allocated)
        const int ntiles = (ctx->K + fvk::TILE_W - 1) / fvk::TILE_W;
        const size_t tab = (size_t)ntiles * ctx->nrows * fvk::TILE_W;
        FV_HIP(ctx->LAQ16.ensure(tab));
        FV_HIP(ctx->d_qaux.ensure(3));
        FV_HIP(hipMemsetAsync(ctx->d_qaux.p, 0, 2 * sizeof(unsigned long long), ctx->stream));
        hipLaunchKernelGGL(fvk::q16_range, dim3(2048), dim3(256), 0, ctx->stream, ctx->LA64.p, tab, ctx->d_qaux.p);
        hipLaunchKernelGGL(fvk::q16_tile_codes, dim3(4096), dim3(256), 0, ctx->stream, ctx->LA64.p, ctx->LAQ16.p, ctx->K, ctx->nrows,
                           ntiles, ctx->d_qaux.p, ctx->d_qaux.p + 1);
        FV_HIP(hipGetLastError());
        unsigned long long bits[2] = { 0, 0 };
        FV_HIP(hipMemcpyAsync(bits, ctx->d_qaux.p, sizeof bits, hipMemcpyDeviceToHost, ctx->stream));
        FV_HIP(hipStreamSynchronize(ctx->stream));
        double lmax, dqmax;
        std::memcpy(&lmax, &bits[0], 8); std::memcpy(&dqmax, &bits[1], 8);
        const float stepf = lmax > 0.0 ? (float)(lmax / 65534.0) : 1.0f;
        ctx->windowq = std::nextafter((float)(2.0 * dqmax), HUGE_VALF);
        ctx->qscale = -stepf;
        ctx->laq16_ready = true;
    }
    return 0;
}

int prepare_full(fv_ctx *ctx, const int *ob, int T, size_t rows_needed, int &kernel, int nscores = 1, bool auto_codes = false)
{
    ctx->row_codes = 0;
    ctx->row_coded.clear();
    if (int rc = admit_full(ctx, ob, T, kernel)) return rc;
    if (int rc = fvi::ensure_workspace(ctx, T, rows_needed, nscores)) return rc;
    if (ctx->csr) return 0;
    // FV_OPT_ROW_CODES: which launch families of the packed kernel take their score codes from the producer (auto_codes: the
    // caller is a decode auto was measured on — fv_decode_full of one sequence; the others take the route under 2 only)
    if (kernel == FV_KERNEL_U16_REFINE && !ctx->vanilla) {
        const int o = ctx->opt_row_codes;
        ctx->row_codes = o == 2 ? 3 : o == 3 ? 1 : o == 4 ? 2 : (o == 1 && auto_codes && ctx->K >= ROW_CODES_AUTO_MIN_K) ? ROW_CODES_AUTO_FAMILIES : 0;
    }
    return ensure_row_codes(ctx, rows_needed);
}

}  // namespace

// a stream's steps are single-task launches from rows of its own: the emission term is the model's log B until a
// score push refuses what the chosen kernel cannot take; row codes stay off
int fvi::stream_admit(fv_ctx *ctx, int &kernel)
{
    static const int none = 0;
    const int *symbols = &none;                   // (any non-NULL sequence: the view of a decode by symbols)
    if (int rc = fvi::emission_view(ctx, symbols, 0)) return rc;
    ctx->row_codes = 0;
    ctx->row_coded.clear();
    return admit_full(ctx, nullptr, 0, kernel);
}

namespace {
// statistics of a full-state decode about to start: the table bytes a step of `kernel` streams
void start_full_stats(fv_ctx *ctx, int kernel, int generations)
{
    long long table = (long long)((ctx->K + fvk::TILE_W - 1) / fvk::TILE_W) * ctx->nrows * fvk::TILE_W * (kernel == FV_KERNEL_F64_STREAM ? 8 : kernel == FV_KERNEL_F32_REFINE ? 4 : 2);
    if (kernel == FV_KERNEL_SPARSE_Q16) table = (long long)ctx->SPdata.bytes();
    if (kernel == FV_KERNEL_SPARSE_CSR) table = (long long)(ctx->CSk.bytes() + ctx->CSq.bytes());
    if (kernel == FV_KERNEL_CSR_F64) table = (long long)(ctx->CSk.bytes() + ctx->CS64.bytes());
    ctx->start_stats(kernel, generations, table, ctx->density);
}

int decode_full_impl(fv_ctx *ctx, const int *ob, int T, int n_split, int mode, int *path_out, float *score_out)
{
    if (!ctx || !path_out || T < 2 || n_split < 1) return FV_ERR_ARG;
    int rc = fvi::emission_view(ctx, ob, T);
    if (rc) return rc;
    if (ctx->K == 0) return FV_ERR_STATE;
    auto t0 = clk::now();
    fv::Plan plan;
    rc = fv::build_plan(T, n_split, mode, ctx->nranks, plan);
    if (rc) return rc;
    size_t most = 1;
    std::vector<std::vector<fv::Pass>> gens = fvi::deal_passes(ctx, plan, &most);
    int kernel = FV_KERNEL_AUTO;
    if ((rc = prepare_full(ctx, ob, T, most, kernel, 1, true))) return rc;
    start_full_stats(ctx, kernel, plan.generations());

    // the flat form of the right-hand generations: one device, one sequence, the reference's task tree, nothing that
    // brackets or captures single launches — and room for its workspace
    bool flat = ctx->opt_flat != 0 && mode == FV_MODE_REFERENCE && plan.generations() >= 2 && plan.generations() - 1 <= fvk::FLAT_MAX_GENS &&
                !ctx->group && !ctx->comm && ctx->nranks == 1 && !ctx->opt_profile && !ctx->vanilla && !(ctx->opt_debug & FV_DBG_GRAPH);
    if (flat) {
        // the shape of one forked generation holding every right-hand pass of more than one step (the others are column jobs)
        int maxlen = 0, nlong = 0;
        for (const fv::Pass &p : plan.passes)
            if (!p.whole) { maxlen = std::max(maxlen, p.R - p.L); nlong += p.R - p.L > 1 ? 1 : 0; }
        const GenShape shape = generation_shape(ctx, kernel, maxlen, nlong, true, true);
        const int cap = shape.cap, nstreams = shape.nstreams;
        // auto: the measured form only — the packed 16-bit kernel's three streams, more than one right-hand generation
        if (ctx->opt_flat == 1 && !(kernel == FV_KERNEL_U16_REFINE && nstreams > 1 && ctx->K >= FLAT_AUTO_MIN_K && T <= FLAT_AUTO_MAX_T && plan.generations() >= 3)) flat = false;
        if (flat) {
            const int key[4] = { T, n_split, cap, nstreams };
            if (std::memcmp(key, ctx->flat_key, sizeof key) != 0) {
                fv::build_flat(plan, cap, nstreams, ctx->flat_plan);
                std::memcpy(ctx->flat_key, key, sizeof key);
                ctx->flat_uploaded = nullptr;
            }
            const int wrc = fvi::ensure_flat_workspace(ctx, T, ctx->flat_plan.passes.size(), ctx->flat_plan.arg_rows, ctx->flat_plan.chain_len);
            if (wrc == FV_ERR_NOMEM) { flat = false; ctx->detail.clear(); }
            else if (wrc) return wrc;
            else if ((rc = ensure_row_codes(ctx, std::max(most, ctx->flat_plan.passes.size())))) return rc;
        }
    }

    if ((rc = fvi::begin_decode(ctx, ob, T))) return rc;
    FV_HIP(hipEventRecord(ctx->ev_start, ctx->stream));
    size_t nprof = 0;
    ctx->fork_active = false;
    for (size_t g = 0; g < gens.size() && !(flat && g == 1); ++g) {
        ctx->stats.passes += (int)gens[g].size();
        if ((rc = run_generation_full(ctx, gens[g], kernel, nprof))) return rc;
        if (g == 0) FV_HIP(hipEventRecord(ctx->ev_top, ctx->stream));
    }
    if (flat && (rc = run_flat_full(ctx, kernel, T))) return rc;
    ctx->close_stats((long long)ctx->K * ctx->K, ctx->K);
    const long long whole[2] = { 0, T };
    rc = fvi::finish_decode(ctx, plan, whole, 1, path_out, score_out, nullptr, t0, nprof, false);
    if (!flat || ctx->stats.flat_first_miss < 1 || rc == FV_ERR_DEVICE) return rc;
    // a generation the resolver could not commit: the answers are exact through the one before it, and the decode goes on
    // from there generation by generation (the one extra host round trip of the flat form)
    ctx->fork_active = false;
    for (size_t g = (size_t)ctx->stats.flat_first_miss; g < gens.size(); ++g) {
        ctx->stats.passes += (int)gens[g].size();
        if ((rc = run_generation_full(ctx, gens[g], kernel, nprof))) return rc;
    }
    ctx->close_stats((long long)ctx->K * ctx->K, ctx->K);
    return fvi::finish_decode(ctx, plan, whole, 1, path_out, score_out, nullptr, t0, nprof, false);
}

// fv_decode_full_batch: the forest plan (build_plan of every sequence on one concatenated time axis) run generation by
// generation — generation g of the batch is generation g of every sequence, so a lock-step's launches carry passes of
// different sequences.  Observations, answers and arg rows are indexed by absolute time, and a pass starts from Pi by
// its flag, not by L == 0: init rows, step kernels, last columns and back-tracks run on the shifted passes as they are.
int decode_full_batch_impl(fv_ctx *ctx, const int *ob, const long long *offsets, int nseq, int n_split, int mode, int *path_out,
                           float *score_out, int *status_out)
{
    const char *who = "fv_decode_full_batch";
    std::vector<int> lengths;
    int rc = fvi::batch_lengths(ctx, who, ob, offsets, nseq, n_split, mode, path_out, lengths);
    if (rc || (rc = fvi::batch_symbols(ctx, who, ob, offsets, nseq))) return rc;
    auto t0 = clk::now();
    const int sumT = (int)offsets[nseq];
    fv::Plan plan;
    if ((rc = fvi::batch_plan(ctx, who, lengths, n_split, mode, plan))) return rc;
    size_t most = 1;
    std::vector<std::vector<fv::Pass>> gens = fvi::deal_passes(ctx, plan, &most);
    int kernel = FV_KERNEL_AUTO;
    if ((rc = prepare_full(ctx, ob, sumT, most, kernel, std::max(nseq, 2)))) return rc;
    start_full_stats(ctx, kernel, plan.generations());

    if ((rc = fvi::begin_decode(ctx, ob, sumT))) return rc;
    FV_HIP(hipEventRecord(ctx->ev_start, ctx->stream));
    size_t nprof = 0;
    ctx->fork_active = false;
    // Generation 0 — nseq whole-sequence passes in lock-step — in the three-stream, four-task form of the right-hand
    // generations (DESIGN.md 5.2f has the measurement); FV_OPT_DEBUG bit 28: single-stream launches of up to
    // FV_OPT_MAX_BATCH tasks instead.
    const int gen0 = (ctx->opt_debug & FV_DBG_BATCH_GEN0_SERIAL) ? BATCH_SERIAL : BATCH_FORK;
    for (size_t g = 0; g < gens.size(); ++g) {
        ctx->stats.passes += (int)gens[g].size();
        if ((rc = run_generation_full(ctx, gens[g], kernel, nprof, gen0))) return rc;
        if (g == 0) FV_HIP(hipEventRecord(ctx->ev_top, ctx->stream));
    }
    ctx->close_stats((long long)ctx->K * ctx->K, ctx->K);
    return fvi::finish_decode(ctx, plan, offsets, nseq, path_out, score_out, status_out, t0, nprof, false);
}

// fv_test_forward (include/flashvit_testing.h): the caller's passes as one right-hand generation of run_generation_full
int test_forward_impl(fv_ctx *ctx, const int *ob, int T, const fv_test_pass *tp, int np, float *rows_out, int *bp_out,
                      unsigned long long *variants_out)
{
    if (!tp || np < 1 || !rows_out || !bp_out || T < 2) return FV_ERR_ARG;
    if (int rv = fvi::emission_view(ctx, ob, T)) return rv;
    if (ctx->K == 0) return FV_ERR_STATE;
    const int K = ctx->K;
    std::vector<fv::Pass> gen((size_t)np);
    std::vector<int> byL((size_t)np);
    for (int q = 0; q < np; ++q) {
        const fv_test_pass &p = tp[q];
        if (p.L < 0 || p.R <= p.L || p.R >= T) { ctx->detail = "fv_test_forward: a pass needs 0 <= L < R < T"; return FV_ERR_ARG; }
        if (p.L == 0 ? p.init_state >= 0 : (p.init_state < 0 || p.init_state >= K)) {
            ctx->detail = "fv_test_forward: init_state < 0 (Pi) at L = 0 only, a state in [0, K) at L > 0";
            return FV_ERR_ARG;
        }
        gen[(size_t)q] = fv::Pass{ p.L, p.R, p.L == 0, false, 0, -1 };       // never the whole-sequence pass
        byL[(size_t)q] = q;
    }
    std::sort(byL.begin(), byL.end(), [&](int a, int b) { return tp[a].L < tp[b].L; });
    for (int q = 1; q < np; ++q)
        if (tp[byL[q]].L <= tp[byL[q - 1]].R) { ctx->detail = "fv_test_forward: passes overlap"; return FV_ERR_ARG; }
    int kernel = FV_KERNEL_AUTO;
    int rc = prepare_full(ctx, ob, T, (size_t)np, kernel);
    if (rc) return rc;
    start_full_stats(ctx, kernel, 1);
    ctx->stats.passes = np;
    if ((rc = fvi::begin_decode(ctx, ob, T))) return rc;
    // Answer array: a valid state at every R (the generation's back-track starts there), then every pass's initial state
    // at L - 1 (written last: it may be the R of the pass before).  Staged through the head of the pinned block, which
    // begin_decode leaves free.
    int *ans = ctx->h_pin;
    std::fill(ans, ans + T, 0);
    for (int q = 0; q < np; ++q) if (tp[q].L > 0) ans[tp[q].L - 1] = tp[q].init_state;
    FV_HIP(hipMemcpyAsync(ctx->d_ans.p, ans, (size_t)T * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    struct Restore { fv_ctx *c; int debug; ~Restore() { c->opt_debug = debug; } } restore{ ctx, ctx->opt_debug };
    ctx->opt_debug |= FV_DBG_FULL_LAST_STEP;     // the whole last row, not the one column a decode reads
    FvTestRecording recording(ctx);
    ctx->fork_active = false;
    size_t nprof = 0;
    if ((rc = run_generation_full(ctx, gen, kernel, nprof))) return rc;      // (sorts `gen` longest first)
    for (int q = 0; q < np; ++q) {
        const fv::Pass &p = gen[(size_t)q];
        int c = 0;
        while (tp[c].L != p.L) ++c;
        const float *row = ctx->d_rows.p + (size_t)q * 2 * ctx->nrows + (size_t)((p.R - p.L) & 1) * ctx->nrows;
        FV_HIP(hipMemcpyAsync(rows_out + (size_t)c * K, row, (size_t)K * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        FV_HIP(hipMemcpyAsync(bp_out + (size_t)(p.L + 1) * K, ctx->d_bp.p + (size_t)(p.L + 1) * K,
                              (size_t)(p.R - p.L) * K * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    }
    FV_HIP(hipStreamSynchronize(ctx->stream));
    for (hipGraphExec_t ge : ctx->graphs) (void)hipGraphExecDestroy(ge);
    ctx->graphs.clear();
    if (variants_out) *variants_out = ctx->test_variants;
    return FV_OK;
}
}  // namespace

extern "C" int fv_test_forward(fv_ctx *ctx, const int *ob, int T, const fv_test_pass *passes, int npasses,
                               float *rows_out, int *bp_out, unsigned long long *variants_out)
{
    if (!ctx) return FV_ERR_ARG;
    FV_NO_STREAM(ctx);
    if (fvi::group_size(ctx) > 1) { ctx->detail = "fv_test_forward: one device per context"; return FV_ERR_ARG; }
    return fvi::drained(ctx, test_forward_impl(ctx, ob, T, passes, npasses, rows_out, bp_out, variants_out));
}

extern "C" int fv_decode_vanilla(fv_ctx *ctx, const int *ob, int T, int *path_out, float *score_out)
{
    if (!ctx) return FV_ERR_ARG;
    FV_NO_STREAM(ctx);
    // (a model set by fv_set_model_sparse: the float64 walk carries the baseline's rounding order, the filter walk cannot)
    if (ctx->csr && ctx->opt_kernel != FV_KERNEL_CSR_F64) { ctx->detail = "fv_decode_vanilla: not available on a model set by fv_set_model_sparse (its kernel reads the dense table) unless FV_KERNEL_CSR_F64 is selected"; return FV_ERR_UNSUPPORTED; }
    const int keep_kernel = ctx->opt_kernel;
    if (!ctx->csr) ctx->opt_kernel = FV_KERNEL_F64_STREAM;      // the baseline's expression has no filter form
    ctx->vanilla = 1;
    int rc = fv_decode_full(ctx, ob, T, 1, FV_MODE_SINGLE_PASS, path_out, score_out);
    ctx->vanilla = 0;
    ctx->opt_kernel = keep_kernel;
    return rc;
}

// checkpoint Viterbi.c:176-251 on the device.  First pass: T-1 steps of the baseline's recurrence with the
// score row of every step that is a multiple of `step` written straight into its checkpoint slot (the next
// step reads it from there; the arg rows of this pass are scratch).  Second pass: every segment
// [c, next checkpoint] restarts from its kept row and re-runs its steps, this time keeping the arg rows;
// the segments are independent, so they advance in lock-step and share table sweeps (up to 8 per launch)
// instead of running last-to-first as the CPU program does.  End state and back-track as in vanilla.
extern "C" int fv_decode_checkpoint(fv_ctx *ctx, const int *ob, int T, int step, int *path_out, float *score_out)
{
    if (!ctx) return FV_ERR_ARG;
    FV_NO_STREAM(ctx);
    if (ctx->csr) { ctx->detail = "fv_decode_checkpoint: not available on a model set by fv_set_model_sparse (its kernel reads the dense table)"; return FV_ERR_UNSUPPORTED; }
    return fvi::drained(ctx, decode_checkpoint_impl(ctx, ob, T, step, path_out, score_out));
}

namespace {
int decode_checkpoint_impl(fv_ctx *ctx, const int *ob, int T, int step, int *path_out, float *score_out)
{
    if (!ctx || !path_out || T < 2) return FV_ERR_ARG;
    if (int rv = fvi::emission_view(ctx, ob, T)) return rv;
    if (ctx->K == 0) return FV_ERR_STATE;
    for (int j = 0; j < T; ++j) if (ob[j] < 0 || ob[j] >= ctx->view.nsym) return FV_ERR_ARG;
    if (step <= 0) step = (int)std::floor(std::sqrt(1.0 * T));        // checkpoint Viterbi.c:179-180
    auto t0 = clk::now();
    FV_HIP(hipSetDevice(ctx->device));
    const int K = ctx->K, nrows = ctx->nrows;
    const int nck = (T + step - 1) / step;
    fv::Plan plan;
    int rc = fv::build_plan(T, 1, FV_MODE_SINGLE_PASS, 1, plan);
    if (rc) return rc;
    if ((rc = fvi::ensure_workspace(ctx, T, (size_t)nck + 1))) return rc;  // two rows per segment + two for the first pass
    if (ctx->d_ckpt.n < (size_t)nck * nrows) {
        FV_HIP(ctx->d_ckpt.ensure((size_t)nck * nrows));
        FV_HIP(hipMemsetAsync(ctx->d_ckpt.p, 0, (size_t)nck * nrows * sizeof(float), ctx->stream));   // row pads stay zero
    }
    start_full_stats(ctx, FV_KERNEL_F64_STREAM, 2);
    ctx->stats.passes = 1 + nck;
    if ((rc = fvi::begin_decode(ctx, ob, T))) return rc;
    FV_HIP(hipEventRecord(ctx->ev_start, ctx->stream));

    struct Restore { fv_ctx *c; ~Restore() { c->vanilla = 0; } } restore{ ctx };
    ctx->vanilla = 1;
    auto ckpt = [&](int c) { return ctx->d_ckpt.p + (size_t)c * nrows; };
    auto scratch = [&](int q, int parity) { return ctx->d_rows.p + ((size_t)q * 2 + parity) * nrows; };
    auto slot_for = [&](const float *in, float *out, int j) { return task_slot(ctx, in, out, j, ctx->d_bp.p + (size_t)j * K); };
    auto launch_at = [&](int parity) { return StepLaunch{ FV_KERNEL_F64_STREAM, ctx->stream, false, parity }; };
    {   // initT1 (:119) into checkpoint 0
        fvk::PassChunk ch;
        ch.n = 1;
        ch.p[0] = fvk::PassDesc{ 0, T - 1, 1, 1, 0 };
        if ((rc = launch_init(ctx, ch, ctx->d_ans.p, ctx->d_ckpt.p, ctx->view.lb64, ctx->d_ob.p, false))) return rc;
    }
    // first pass (:213-232)
    auto row_after = [&](int j) -> float * { return j % step == 0 ? ckpt(j / step) : scratch(nck, j & 1); };
    FV_HIP(hipEventRecord(ctx->ev_s0, ctx->stream));
    for (int j = 1; j < T; ++j) {
        fvk::TaskSlot sl = slot_for(row_after(j - 1), row_after(j), j);
        if ((rc = queue_step(ctx, launch_at(j & 1), &sl, 1))) return rc;
    }
    FV_HIP(hipEventRecord(ctx->ev_s1, ctx->stream));
    FV_HIP(hipEventRecord(ctx->ev_top, ctx->stream));
    // second pass (:236-248, subroutine :121-174): segment c = times c*step .. min((c+1)*step, T-1)
    std::vector<int> order(nck);
    for (int c = 0; c < nck; ++c) order[c] = c;
    auto seg_len = [&](int c) { return std::min((c + 1) * step, T - 1) - c * step; };
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return seg_len(a) > seg_len(b); });
    const int maxlen = seg_len(order[0]);
    const int cap = generation_shape(ctx, FV_KERNEL_F64_STREAM, maxlen, nck, false, false).cap;     // (one stream: no fork)
    int active = nck;
    for (int s = 1; s <= maxlen; ++s) {
        while (active > 0 && seg_len(order[active - 1]) < s) --active;
        for (int base = 0; base < active; base += cap) {
            const int nb = std::min(cap, active - base);
            fvk::TaskSlot slots[fvk::MAX_BATCH];
            for (int q = 0; q < nb; ++q) {
                const int c = order[base + q];
                slots[q] = slot_for(s == 1 ? ckpt(c) : scratch(c, (s - 1) & 1), scratch(c, s & 1), c * step + s);
            }
            if ((rc = queue_step(ctx, launch_at(s & 1), slots, nb))) return rc;
        }
    }
    // end state (:152-165) from the first pass's last row, then the back-track through the kept arg rows (:167-171)
    if ((rc = end_pick(ctx, row_after(T - 1), ctx->d_ans.p + (T - 1), ctx->d_score.p))) return rc;
    if ((rc = backtrack_whole(ctx, ctx->d_bp.p, T - 1, ctx->d_ans.p, ctx->d_counters.p + fvk::BT_COUNTER))) return rc;
    ctx->close_stats((long long)K * K, 0);
    const long long whole[2] = { 0, T };
    return fvi::finish_decode(ctx, plan, whole, 1, path_out, score_out, nullptr, t0, 0, false);
}
}  // namespace
