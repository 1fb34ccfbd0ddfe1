// fv_sumprod.hip — fv_loglik / fv_loglik_batch / fv_posteriors: the sum-product kernels and their driver.
// One driver runs forward passes of any number of sequences in lock-step (two float64 rows each); fv_posteriors keeps
// every row of one sequence, runs the backward pass on the transposed table and finishes with the gamma kernel.
// A model set by fv_set_model_sparse takes the same driver under fv_set_sparse_sumprod: the step launches
// are sumprod_step_csr / sumprod_back_csr over the stored transitions, everything else is shared.
// fv_expected_counts runs the two passes of fv_posteriors per sequence and the counting kernels of
// fv_counts_kernels.hip.inc behind them.
#include "fv_internal.h"
#include "flashvit_testing.h"
#include "fv_sumprod_kernels.hip.inc"
#include "fv_counts_kernels.hip.inc"

namespace {

using fvs::StepTask;

size_t step_lds_bytes(int nb, int nrows) { return fvs::step_lds_doubles(nb, nrows) * sizeof(double); }

// most tasks of one step launch: FV_OPT_MAX_BATCH, the instantiations there are, the float64 rows LDS holds (0: not even one)
int batch_cap(const fv_ctx *ctx)
{
    int cap = 0;
    for (int nb = 1; nb <= fvs::MAX_NB && nb <= std::max(1, ctx->opt_max_batch); nb *= 2)
        if (step_lds_bytes(nb, ctx->nrows) <= (size_t)fvk::LDS_LIMIT) cap = nb;
    return cap;
}

// How a call sweeps the transitions: the dense tables, or (csr) the stored entries with the scaled rows in LDS or (mem) in
// workspace rows.  cap: most tasks of one step launch.
struct Route { bool csr, mem; int cap; };

Route route_of(const fv_ctx *ctx)
{
    Route r{ ctx->csr, false, batch_cap(ctx) };
    if (r.csr && (ctx->opt_csr_mem || r.cap < 1)) {
        r.mem = true;
        r.cap = 1;
        while (r.cap * 2 <= fvs::MAX_NB && r.cap * 2 <= ctx->opt_max_batch) r.cap *= 2;
    }
    return r;
}

template <int NB> constexpr unsigned long long form_bit(int base) { return 1ull << (base + (NB == 1 ? 0 : NB == 2 ? 1 : 2)); }

template <int NB>
void launch_step_nb(fv_ctx *ctx, const StepTask *tasks, const float *tab)
{
    fvs::StepArgs<NB> a;
    for (int b = 0; b < NB; ++b) a.t[b] = tasks[b];
    const int ntiles = (ctx->K + fvk::TILE_W - 1) / fvk::TILE_W;
    ctx->sp_forms |= form_bit<NB>(FV_SPF_DENSE_SHIFT);
    hipLaunchKernelGGL(fvs::sumprod_step<NB>, dim3(ntiles), dim3(fvs::BLOCK), step_lds_bytes(NB, ctx->nrows), ctx->stream, a, tab,
                       ctx->K, ctx->nrows, ctx->sp_res.p);
}

// the memory form's scale launch for the NB tasks of the step launch that follows: row maxima, then p and m
int launch_scale(fv_ctx *ctx, const StepTask *tasks, int nb)
{
    fvs::StepArgs<fvs::MAX_NB> a{};
    for (int b = 0; b < nb; ++b) a.t[b] = tasks[b];
    double *m = ctx->sp_scale_m.p, *part = m + fvs::MAX_NB;
    const unsigned blocks = (unsigned)((ctx->K + fvs::SCALE_BLOCK * fvs::SCALE_PER_THREAD - 1) / (fvs::SCALE_BLOCK * fvs::SCALE_PER_THREAD));
    hipLaunchKernelGGL(fvs::sumprod_rowmax, dim3(fvs::SCALE_PARTS, nb), dim3(fvs::SCALE_BLOCK), 0, ctx->stream, a, ctx->K, part);
    hipLaunchKernelGGL(fvs::sumprod_scale, dim3(blocks, nb), dim3(fvs::SCALE_BLOCK), 0, ctx->stream, a, ctx->K, part, ctx->sp_scaled.p,
                       (size_t)ctx->K, m);
    FV_HIP(hipGetLastError());
    return 0;
}

template <int NB, bool MEM>
void launch_csr_nb(fv_ctx *ctx, const StepTask *tasks, bool backward)
{
    const fvs::ScaledRows rows = MEM ? fvs::ScaledRows{ ctx->sp_scaled.p, ctx->sp_scale_m.p } : fvs::ScaledRows{ nullptr, nullptr };
    if (!backward) {
        fvs::CsrStepArgs<NB> a;
        a.ck = ctx->CSk.p; a.clin = ctx->CSlin.p; a.c64 = ctx->CS64.p; a.tile_off = ctx->CSoff.p; a.tile_nwb = ctx->CSnwb.p;
        a.counters = ctx->sp_res.p;
        a.K = ctx->K; a.nrows = ctx->nrows; a.ntiles = (ctx->K + fvk::TILE_W - 1) / fvk::TILE_W; a.tiles_per_xcd = (a.ntiles + 7) / 8;
        a.s = rows;
        for (int b = 0; b < NB; ++b) a.t[b] = tasks[b];
        ctx->sp_forms |= form_bit<NB>(MEM ? FV_SPF_CSR_FWD_MEM_SHIFT : FV_SPF_CSR_FWD_LDS_SHIFT);
        hipLaunchKernelGGL((fvs::sumprod_step_csr<NB, MEM>), dim3(a.tiles_per_xcd * 8), dim3(fvs::CSR_BLOCK),
                           fvs::csr_step_lds_doubles(NB, ctx->nrows, MEM) * sizeof(double), ctx->stream, a);
    } else {
        fvs::CsrBackArgs<NB> a;
        a.rptr = ctx->CRptr.p; a.rcol = ctx->CRcol.p; a.rlin = ctx->CRlin.p; a.rlog = ctx->CRlog.p;
        a.counters = ctx->sp_res.p;
        a.K = ctx->K; a.nrows = ctx->nrows;
        a.s = rows;
        for (int b = 0; b < NB; ++b) a.t[b] = tasks[b];
        ctx->sp_forms |= form_bit<NB>(MEM ? FV_SPF_CSR_BACK_MEM_SHIFT : FV_SPF_CSR_BACK_LDS_SHIFT);
        hipLaunchKernelGGL((fvs::sumprod_back_csr<NB, MEM>), dim3((ctx->K + fvs::BACK_ROWS - 1) / fvs::BACK_ROWS), dim3(fvs::BLOCK),
                           fvs::csr_back_lds_doubles(NB, ctx->nrows, MEM) * sizeof(double), ctx->stream, a);
    }
}

template <int NB>
int launch_csr(fv_ctx *ctx, const StepTask *tasks, const Route &r, bool backward)
{
    if (r.mem) {
        if (int rc = launch_scale(ctx, tasks, NB)) return rc;
        launch_csr_nb<NB, true>(ctx, tasks, backward);
    } else {
        launch_csr_nb<NB, false>(ctx, tasks, backward);
    }
    return 0;
}

// n tasks in launches of the largest instantiation that fits the cap and what is left: every task's bits are those of
// a launch of its own.  backward: the transposed table, or the walk over the caller's rows.
int launch_steps(fv_ctx *ctx, const std::vector<StepTask> &tasks, const Route &r, bool backward, fv_sumprod_stats &st)
{
    const float *tab = backward ? ctx->SPAT.p : ctx->SPA.p;
    size_t at = 0;
    while (at < tasks.size()) {
        int nb = 1, rc = 0;
        while (nb * 2 <= r.cap && (size_t)nb * 2 <= tasks.size() - at) nb *= 2;
        if (r.csr) {
            rc = nb == 4 ? launch_csr<4>(ctx, &tasks[at], r, backward) : nb == 2 ? launch_csr<2>(ctx, &tasks[at], r, backward)
                                                                                 : launch_csr<1>(ctx, &tasks[at], r, backward);
            if (rc) return rc;
        }
        else if (nb == 4) launch_step_nb<4>(ctx, &tasks[at], tab);
        else if (nb == 2) launch_step_nb<2>(ctx, &tasks[at], tab);
        else launch_step_nb<1>(ctx, &tasks[at], tab);
        FV_HIP(hipGetLastError());
        at += (size_t)nb; st.step_launches += 1; st.task_steps += nb;
    }
    return 0;
}

// init rows (lpi != NULL: log Pi + the emission row; else zeros) and final log-sums, SMALL_NB tasks per launch
int launch_small(fv_ctx *ctx, const std::vector<StepTask> &tasks, bool final_sum)
{
    for (size_t at = 0; at < tasks.size(); at += fvs::SMALL_NB) {
        fvs::StepArgs<fvs::SMALL_NB> a{};
        const int n = (int)std::min<size_t>(fvs::SMALL_NB, tasks.size() - at);
        for (int b = 0; b < n; ++b) a.t[b] = tasks[at + (size_t)b];
        if (final_sum) hipLaunchKernelGGL(fvs::sumprod_final, dim3(n), dim3(fvs::BLOCK), 0, ctx->stream, a, ctx->K);
        else hipLaunchKernelGGL(fvs::sumprod_init, dim3((ctx->K + 255) / 256, n), dim3(256), 0, ctx->stream, a, ctx->K);
        FV_HIP(hipGetLastError());
    }
    return 0;
}

// what every entry point refuses alike, before any device work; then the emission view
int admission(fv_ctx *ctx, const char *who, const int *&ob, long long T)
{
    const std::string w = who;
    FV_NO_STREAM(ctx);
    if (ctx->group || ctx->comm || ctx->nranks > 1) {
        ctx->detail = w + ": one device, no communicator and no partition";
        return FV_ERR_UNSUPPORTED;
    }
    if (ctx->K == 0) { ctx->detail = w + ": no model"; return FV_ERR_STATE; }
    if (ctx->csr && !ctx->opt_sparse_sumprod) {
        ctx->detail = w + ": models set by fv_set_model_sparse are not supported (the backward pass needs the out-edge form "
                          "on the device); set the model with fv_set_model";
        return FV_ERR_UNSUPPORTED;
    }
    if (!ctx->csr && batch_cap(ctx) < 1) {
        ctx->detail = w + ": K = " + std::to_string(ctx->K) + " is beyond the float64 score row the step kernel stages in LDS (K <= 20192)";
        return FV_ERR_UNSUPPORTED;
    }
    return fvi::emission_view(ctx, ob, T);
}

// the linear tables, built on the device from LA64 on first use (the buffers are granted by the caller)
int build_table(fv_ctx *ctx, bool transpose)
{
    bool &ready = transpose ? ctx->spat_ready : ctx->spa_ready;
    if (ready) return 0;
    const int ntiles = (ctx->K + fvk::TILE_W - 1) / fvk::TILE_W;
    const size_t tab = (size_t)ntiles * ctx->nrows * fvk::TILE_W;
    hipLaunchKernelGGL(fvs::sumprod_build_table, dim3((unsigned)((tab + 255) / 256)), dim3(256), 0, ctx->stream, ctx->LA64.p,
                       transpose ? ctx->SPAT.p : ctx->SPA.p, ctx->K, ctx->nrows, ntiles, transpose ? 1 : 0);
    FV_HIP(hipGetLastError());
    ready = true;
    return 0;
}

// the linear values of a CSR-set model, built on the device from CS64 / CRlog on first use (the buffers are granted by the caller)
int build_lin(fv_ctx *ctx, bool rows)
{
    bool &ready = rows ? ctx->crlin_ready : ctx->cslin_ready;
    if (ready) return 0;
    const size_t n = rows ? (size_t)ctx->csr_nnz : 4 * (size_t)ctx->csr_vectors;
    if (n) {
        hipLaunchKernelGGL(fvs::sumprod_build_lin, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream,
                           rows ? ctx->CRlog.p : ctx->CS64.p, rows ? ctx->CRlin.p : ctx->CSlin.p, n);
        FV_HIP(hipGetLastError());
    }
    ready = true;
    return 0;
}

// what a call asks for beside its rows: the table(s) it sweeps and, in the memory form, the scaled rows of one step launch
void want_tables(fv_ctx *ctx, fvi::Wants &wants, const Route &r, bool backward)
{
    if (!r.csr) {
        const size_t tab = (size_t)((ctx->K + fvk::TILE_W - 1) / fvk::TILE_W) * ctx->nrows * fvk::TILE_W;
        wants.add(ctx->SPA, tab);
        if (backward) wants.add(ctx->SPAT, tab);
        return;
    }
    wants.add(ctx->CSlin, std::max<size_t>(4 * (size_t)ctx->csr_vectors, 1));
    if (backward) wants.add(ctx->CRlin, std::max<size_t>((size_t)ctx->csr_nnz, 1));
    if (r.mem) {
        wants.add(ctx->sp_scaled, (size_t)fvs::MAX_NB * ctx->K);
        wants.add(ctx->sp_scale_m, (size_t)fvs::MAX_NB * (1 + fvs::SCALE_PARTS));
    }
}

int build_tables(fv_ctx *ctx, const Route &r, bool backward)
{
    int rc = 0;
    if (r.csr) { if ((rc = build_lin(ctx, false)) || (backward && (rc = build_lin(ctx, true)))) return rc; }
    else if ((rc = build_table(ctx, false)) || (backward && (rc = build_table(ctx, true)))) return rc;
    return 0;
}

struct Call {
    clk::time_point t0 = clk::now();
    fv_sumprod_stats st{};
};

int begin_call(fv_ctx *ctx, Call &c, int passes, int cap, size_t nres)
{
    c.st.passes = passes; c.st.batch_cap = cap;
    c.st.table_bytes_per_step = ctx->csr ? 8ll * 4 * ctx->csr_vectors : 4ll * ((ctx->K + fvk::TILE_W - 1) / fvk::TILE_W) * ctx->nrows * fvk::TILE_W;
    ctx->sp_forms = 0;
    FV_HIP(hipMemsetAsync(ctx->sp_res.p, 0, nres * sizeof(unsigned long long), ctx->stream));
    FV_HIP(hipEventRecord(ctx->ev_start, ctx->stream));
    return 0;
}

// the result words to the host (one copy, the call's one wait), the statistics
int end_call(fv_ctx *ctx, Call &c, std::vector<unsigned long long> &res)
{
    FV_HIP(hipEventRecord(ctx->ev_stop, ctx->stream));
    FV_HIP(hipMemcpyAsync(res.data(), ctx->sp_res.p, res.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    FV_HIP(hipStreamSynchronize(ctx->stream));
    float ms = 0.f;
    FV_HIP(hipEventElapsedTime(&ms, ctx->ev_start, ctx->ev_stop));
    c.st.gpu_ms = ms;
    c.st.refine_columns = (long long)res[fvs::CNT_REFINE_COLUMNS];
    c.st.refine_finite = (long long)res[fvs::CNT_REFINE_FINITE];
    return 0;
}

void publish(fv_ctx *ctx, Call &c)
{
    c.st.call_ms = ms_since(c.t0);
    c.st.device_bytes = (long long)fvi::device_bytes(ctx);
    ctx->sp_stats = c.st; ctx->sp_any = true;
}

inline double as_double(unsigned long long w) { double d; std::memcpy(&d, &w, sizeof d); return d; }

int loglik_batch(fv_ctx *ctx, const char *who, const int *ob, const long long *offsets, int nseq, double *loglik_out, int *status_out)
{
    const std::string w = who;
    if (!offsets || !loglik_out || nseq < 1) { ctx->detail = w + ": offsets != NULL, loglik_out != NULL and nseq >= 1"; return FV_ERR_ARG; }
    if (offsets[0] != 0) { ctx->detail = w + ": offsets[0] must be 0"; return FV_ERR_ARG; }
    for (int s = 0; s < nseq; ++s) {
        const long long len = offsets[s + 1] - offsets[s];
        if (len < 0) { ctx->detail = w + ": offsets decrease at sequence " + std::to_string(s); return FV_ERR_ARG; }
        if (len < 1) { ctx->detail = w + ": sequence " + std::to_string(s) + " has no observation (T >= 1)"; return FV_ERR_ARG; }
        if (offsets[s + 1] > 0x7fffffffLL) { ctx->detail = w + ": more than 2^31 - 1 observations in all (at sequence " + std::to_string(s) + ")"; return FV_ERR_ARG; }
    }
    if (int rc = admission(ctx, who, ob, offsets[nseq])) return rc;
    if (int rc = fvi::batch_symbols(ctx, who, ob, offsets, nseq)) return rc;
    FV_HIP(hipSetDevice(ctx->device));

    const Route route = route_of(ctx);
    const int K = ctx->K, cap = route.cap;
    const size_t tab = (size_t)((K + fvk::TILE_W - 1) / fvk::TILE_W) * ctx->nrows * fvk::TILE_W, nres = fvs::NCOUNTERS + (size_t)nseq;
    fvi::Wants wants;
    wants.what = w + " workspace";
    wants.dominant = route.csr ? "linear values " + std::to_string(16ull * (unsigned long long)ctx->csr_vectors) : "linear table " + std::to_string(4ull * tab);
    want_tables(ctx, wants, route, false);
    wants.add(ctx->sp_rows, (size_t)nseq * 2 * K); wants.add(ctx->sp_res, nres);
    if (int rc = fvi::grant(ctx, wants, true)) return rc;

    Call c;
    int rc = 0;
    if ((rc = begin_call(ctx, c, 1, cap, nres)) || (rc = build_tables(ctx, route, false))) return rc;
    auto row = [&](int s, long long t) { return ctx->sp_rows.p + ((size_t)s * 2 + (size_t)(t & 1)) * K; };
    auto emis = [&](int s, long long t) { return ctx->view.lb64 + (size_t)ob[offsets[s] + t] * K; };
    std::vector<StepTask> tasks;
    long long longest = 0;
    for (int s = 0; s < nseq; ++s) {
        tasks.push_back({ ctx->LPi64.p, nullptr, emis(s, 0), row(s, 0) });
        longest = std::max(longest, offsets[s + 1] - offsets[s]);
    }
    if ((rc = launch_small(ctx, tasks, false))) return rc;
    for (long long t = 1; t < longest; ++t) {
        tasks.clear();
        for (int s = 0; s < nseq; ++s)
            if (offsets[s + 1] - offsets[s] > t) tasks.push_back({ row(s, t - 1), nullptr, emis(s, t), row(s, t) });
        if ((rc = launch_steps(ctx, tasks, route, false, c.st))) return rc;
    }
    tasks.clear();
    double *d_ll = reinterpret_cast<double *>(ctx->sp_res.p + fvs::NCOUNTERS);
    for (int s = 0; s < nseq; ++s) tasks.push_back({ row(s, offsets[s + 1] - offsets[s] - 1), nullptr, nullptr, d_ll + s });
    if ((rc = launch_small(ctx, tasks, true))) return rc;
    std::vector<unsigned long long> res(nres);
    if ((rc = end_call(ctx, c, res))) return rc;
    int worst = FV_OK;
    for (int s = 0; s < nseq; ++s) {
        loglik_out[s] = as_double(res[fvs::NCOUNTERS + (size_t)s]);
        const int st = loglik_out[s] > -HUGE_VAL ? FV_OK : FV_ERR_NO_PRED;
        if (status_out) status_out[s] = st;
        worst = std::min(worst, st);
    }
    publish(ctx, c);
    return worst;
}

// The two passes of one sequence, every launch single-task: the alpha rows, loglik into *d_ll, the beta rows.  emis(t): the
// emission row of time t.
template <class Emis>
int two_passes(fv_ctx *ctx, const Route &route, int T, Emis &&emis, double *alpha, double *beta, double *d_ll, fv_sumprod_stats &st)
{
    const int K = ctx->K;
    int rc = 0;
    std::vector<StepTask> one(1);
    one[0] = { ctx->LPi64.p, nullptr, emis(0), alpha };
    if ((rc = launch_small(ctx, one, false))) return rc;
    for (int t = 1; t < T; ++t) {
        one[0] = { alpha + (size_t)(t - 1) * K, nullptr, emis(t), alpha + (size_t)t * K };
        if ((rc = launch_steps(ctx, one, route, false, st))) return rc;
    }
    one[0] = { alpha + (size_t)(T - 1) * K, nullptr, nullptr, d_ll };
    if ((rc = launch_small(ctx, one, true))) return rc;
    one[0] = { nullptr, nullptr, nullptr, beta + (size_t)(T - 1) * K };
    if ((rc = launch_small(ctx, one, false))) return rc;
    for (int t = T - 2; t >= 0; --t) {
        one[0] = { beta + (size_t)(t + 1) * K, emis(t + 1), nullptr, beta + (size_t)t * K };
        if ((rc = launch_steps(ctx, one, route, true, st))) return rc;
    }
    return 0;
}

// fv_posteriors and fv_test_sumprod_rows: alpha_out / beta_out are the hook's
int posteriors(fv_ctx *ctx, const char *who, const int *ob, int T, float *gamma_out, long long ld, int *path_out, double *loglik_out,
               double *alpha_out, double *beta_out)
{
    const std::string w = who;
    if (T < 1) { ctx->detail = w + ": T >= 1"; return FV_ERR_ARG; }
    if (gamma_out && (ld < ctx->K || ld > (1ll << 59) / T)) { ctx->detail = w + ": ld >= K"; return FV_ERR_ARG; }
    if (int rc = admission(ctx, who, ob, T)) return rc;
    for (int t = 0; t < T; ++t)
        if (ob[t] < 0 || ob[t] >= ctx->view.nsym) {
            ctx->detail = w + ": a symbol outside [0, M) at position " + std::to_string(t);
            return FV_ERR_ARG;
        }
    FV_HIP(hipSetDevice(ctx->device));
    const Route route = route_of(ctx);
    const int K = ctx->K, cap = route.cap;
    bool gamma_on_device = false;
    if (gamma_out) {
        const fvi::PointerPlace at = fvi::pointer_place(gamma_out);
        gamma_on_device = at.on_device;
        if (at.on_device && at.device != ctx->device) { ctx->detail = w + ": gamma_out lies on another device than the context"; return FV_ERR_ARG; }
    }
    const size_t nres = fvs::NCOUNTERS + 1;
    const size_t cells = (size_t)T * K;
    fvi::Wants wants;
    wants.what = w + " workspace"; wants.dominant = "alpha and beta rows " + std::to_string(16ull * cells);
    want_tables(ctx, wants, route, true);
    wants.add(ctx->sp_rows, cells); wants.add(ctx->sp_beta, cells);
    wants.add(ctx->sp_res, nres); wants.add(ctx->sp_path, (size_t)T);
    if (gamma_out && !gamma_on_device) wants.add(ctx->sp_gamma, cells);
    if (int rc = fvi::grant(ctx, wants, true)) return rc;

    Call c;
    int rc = 0;
    if ((rc = begin_call(ctx, c, 2, cap, nres)) || (rc = build_tables(ctx, route, true))) return rc;
    double *alpha = ctx->sp_rows.p, *beta = ctx->sp_beta.p;
    auto emis = [&](int t) { return ctx->view.lb64 + (size_t)ob[t] * K; };
    double *d_ll = reinterpret_cast<double *>(ctx->sp_res.p + fvs::NCOUNTERS);
    if ((rc = two_passes(ctx, route, T, emis, alpha, beta, d_ll, c.st))) return rc;
    if (gamma_out || path_out) {
        float *g = !gamma_out ? nullptr : gamma_on_device ? gamma_out : ctx->sp_gamma.p;
        hipLaunchKernelGGL(fvs::sumprod_gamma, dim3(T), dim3(fvs::BLOCK), 0, ctx->stream, alpha, beta, d_ll, K, g,
                           gamma_on_device ? ld : (long long)K, path_out ? ctx->sp_path.p : nullptr);
        FV_HIP(hipGetLastError());
    }
    std::vector<unsigned long long> res(nres);
    if ((rc = end_call(ctx, c, res))) return rc;
    const double ll = as_double(res[fvs::NCOUNTERS]);
    if (loglik_out) *loglik_out = ll;
    const bool dead = !(ll > -HUGE_VAL);
    if (path_out) {
        if (dead) std::fill(path_out, path_out + T, -1);
        else FV_HIP(hipMemcpyAsync(path_out, ctx->sp_path.p, (size_t)T * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    }
    if (gamma_out && !gamma_on_device && !dead)
        FV_HIP(hipMemcpy2DAsync(gamma_out, (size_t)ld * sizeof(float), ctx->sp_gamma.p, (size_t)K * sizeof(float), (size_t)K * sizeof(float),
                                (size_t)T, hipMemcpyDeviceToHost, ctx->stream));
    if (alpha_out) FV_HIP(hipMemcpyAsync(alpha_out, alpha, cells * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (beta_out) FV_HIP(hipMemcpyAsync(beta_out, beta, cells * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    FV_HIP(hipStreamSynchronize(ctx->stream));
    publish(ctx, c);
    return dead ? FV_ERR_NO_PRED : FV_OK;
}

// fv_expected_counts.  Sequence by sequence on the one stream: posteriors()'s two passes, then the scale
// launch, the xi kernel and the gamma sums, each adding the sequence's finished values into the call's accumulators.  The
// host learns which sequences were dead from the logliks, after the call's one wait.
int expected_counts(fv_ctx *ctx, const int *ob, const long long *offsets, int nseq, double *trans_out, long long ld, double *emit_out,
                    double *init_out, double *occ_out, double *loglik_out, int *status_out)
{
    const std::string w = "fv_expected_counts";
    if (!offsets || nseq < 1) { ctx->detail = w + ": offsets != NULL and nseq >= 1"; return FV_ERR_ARG; }
    if (offsets[0] != 0) { ctx->detail = w + ": offsets[0] must be 0"; return FV_ERR_ARG; }
    long long longest = 0;
    for (int s = 0; s < nseq; ++s) {
        const long long len = offsets[s + 1] - offsets[s];
        if (len < 0) { ctx->detail = w + ": offsets decrease at sequence " + std::to_string(s); return FV_ERR_ARG; }
        if (len < 1) { ctx->detail = w + ": sequence " + std::to_string(s) + " has no observation (T >= 1)"; return FV_ERR_ARG; }
        if (offsets[s + 1] > 0x7fffffffLL) { ctx->detail = w + ": more than 2^31 - 1 observations in all (at sequence " + std::to_string(s) + ")"; return FV_ERR_ARG; }
        longest = std::max(longest, len);
    }
    if (!ob && emit_out) { ctx->detail = w + ": emit_out must be NULL with ob == NULL (staged emissions have no symbol alphabet)"; return FV_ERR_ARG; }
    FV_NO_STREAM(ctx);
    if (ctx->csr && !ctx->group && !ctx->comm && ctx->nranks <= 1) {
        ctx->detail = w + ": models set by fv_set_model_sparse are not supported, with or without fv_set_sparse_sumprod (the "
                          "counts over the stored transitions are a follow-up); set the model with fv_set_model";
        return FV_ERR_UNSUPPORTED;
    }
    const bool staged = !ob;
    if (int rc = admission(ctx, "fv_expected_counts", ob, offsets[nseq])) return rc;
    const int K = ctx->K, M = ctx->M;
    if (trans_out && (ld < K || ld > (1ll << 59) / K)) { ctx->detail = w + ": ld >= K"; return FV_ERR_ARG; }
    if (int rc = fvi::batch_symbols(ctx, "fv_expected_counts", ob, offsets, nseq)) return rc;
    FV_HIP(hipSetDevice(ctx->device));
    bool trans_on_device = false;
    if (trans_out) {
        const fvi::PointerPlace at = fvi::pointer_place(trans_out);
        trans_on_device = at.on_device;
        if (at.on_device && at.device != ctx->device) { ctx->detail = w + ": trans_out lies on another device than the context"; return FV_ERR_ARG; }
    }

    const Route route = route_of(ctx);
    const size_t total = (size_t)offsets[nseq], cells = (size_t)longest * K, pq = std::max<size_t>((size_t)(longest - 1) * K, 1);
    const size_t nres = fvs::NCOUNTERS + (size_t)nseq + 1, km = (size_t)K * std::max(M, 1);
    const bool want_emit = emit_out && !staged, want_vec = init_out || occ_out;
    fvi::Wants wants;
    wants.what = w + " workspace"; wants.dominant = "alpha, beta, P and Q rows " + std::to_string(16ull * cells + 16ull * (cells - K));
    want_tables(ctx, wants, route, true);
    wants.add(ctx->sp_rows, cells); wants.add(ctx->sp_beta, cells); wants.add(ctx->sp_res, nres);
    wants.add(ctx->ct_ob, total);
    if (trans_out) { wants.add(ctx->ct_p, pq); wants.add(ctx->ct_q, pq); wants.add(ctx->ct_wide, (size_t)longest); }
    if (trans_out && !trans_on_device) wants.add(ctx->ct_trans, (size_t)K * K);
    if (want_emit) { wants.add(ctx->ct_emit, km); wants.add(ctx->ct_emit_seq, km); }
    if (want_vec) wants.add(ctx->ct_vec, 2 * (size_t)K);
    if (int rc = fvi::grant(ctx, wants, true)) return rc;

    const clk::time_point t0 = clk::now();
    fv_counts_stats cs{};
    fv_sumprod_stats steps{};
    const unsigned long long forms = ctx->sp_forms;         // fv_test_sumprod_forms keeps reporting the sum-product calls
    int rc = 0;
    FV_HIP(hipMemsetAsync(ctx->sp_res.p, 0, nres * sizeof(unsigned long long), ctx->stream));
    FV_HIP(hipEventRecord(ctx->ev_start, ctx->stream));
    if ((rc = build_tables(ctx, route, true))) return rc;
    FV_HIP(hipMemcpyAsync(ctx->ct_ob.p, ob, total * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    double *acc = !trans_out ? nullptr : trans_on_device ? trans_out : ctx->ct_trans.p;
    const long long acc_ld = trans_on_device ? ld : (long long)K;
    if (acc) FV_HIP(hipMemset2DAsync(acc, (size_t)acc_ld * sizeof(double), 0, (size_t)K * sizeof(double), (size_t)K, ctx->stream));
    if (want_emit) FV_HIP(hipMemsetAsync(ctx->ct_emit.p, 0, km * sizeof(double), ctx->stream));
    if (want_vec) FV_HIP(hipMemsetAsync(ctx->ct_vec.p, 0, 2 * (size_t)K * sizeof(double), ctx->stream));
    double *alpha = ctx->sp_rows.p, *beta = ctx->sp_beta.p;
    double *d_ll = reinterpret_cast<double *>(ctx->sp_res.p + fvs::NCOUNTERS);
    unsigned long long *d_wide = ctx->sp_res.p + fvs::NCOUNTERS + (size_t)nseq;
    const unsigned tiles = (unsigned)((K + fvc::TILE - 1) / fvc::TILE);
    for (int s = 0; s < nseq && !rc; ++s) {
        const int T = (int)(offsets[s + 1] - offsets[s]);
        const int *sob = ob + offsets[s], *d_sob = ctx->ct_ob.p + offsets[s];
        auto emis = [&](int t) { return ctx->view.lb64 + (size_t)sob[t] * K; };
        if ((rc = two_passes(ctx, route, T, emis, alpha, beta, d_ll + s, steps))) break;
        if (acc && T >= 2) {
            hipLaunchKernelGGL(fvc::counts_scale, dim3(T - 1), dim3(fvc::SCALE_BLOCK), 0, ctx->stream, alpha, beta, ctx->view.lb64, d_sob,
                               d_ll + s, K, ctx->ct_p.p, ctx->ct_q.p, ctx->ct_wide.p, d_wide);
            hipLaunchKernelGGL(fvc::counts_xi, dim3(tiles, tiles), dim3(fvc::XI_BLOCK), 0, ctx->stream, ctx->ct_p.p, ctx->ct_q.p,
                               ctx->ct_wide.p, d_ll + s, T - 1, K, ctx->nrows, ctx->SPA.p, ctx->LA64.p, acc, acc_ld);
            cs.xi_launches += 1;
        }
        if (want_emit || want_vec) {
            if (want_emit) FV_HIP(hipMemsetAsync(ctx->ct_emit_seq.p, 0, km * sizeof(double), ctx->stream));
            hipLaunchKernelGGL(fvc::counts_gamma, dim3((K + fvc::GAMMA_BLOCK - 1) / fvc::GAMMA_BLOCK), dim3(fvc::GAMMA_BLOCK), 0, ctx->stream,
                               alpha, beta, d_ll + s, d_sob, T, K, M, init_out ? ctx->ct_vec.p : nullptr,
                               occ_out ? ctx->ct_vec.p + K : nullptr, want_emit ? ctx->ct_emit_seq.p : nullptr);
            if (want_emit)
                hipLaunchKernelGGL(fvc::counts_add, dim3((unsigned)((km + 255) / 256)), dim3(256), 0, ctx->stream, ctx->ct_emit.p,
                                   ctx->ct_emit_seq.p, d_ll + s, km);
        }
        FV_HIP(hipGetLastError());
    }
    ctx->sp_forms = forms;
    if (rc) return rc;
    FV_HIP(hipEventRecord(ctx->ev_stop, ctx->stream));
    std::vector<unsigned long long> res(nres);
    FV_HIP(hipMemcpyAsync(res.data(), ctx->sp_res.p, nres * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    if (trans_out && !trans_on_device)
        FV_HIP(hipMemcpy2DAsync(trans_out, (size_t)ld * sizeof(double), ctx->ct_trans.p, (size_t)K * sizeof(double), (size_t)K * sizeof(double),
                                (size_t)K, hipMemcpyDeviceToHost, ctx->stream));
    if (want_emit) FV_HIP(hipMemcpyAsync(emit_out, ctx->ct_emit.p, km * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (init_out) FV_HIP(hipMemcpyAsync(init_out, ctx->ct_vec.p, (size_t)K * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (occ_out) FV_HIP(hipMemcpyAsync(occ_out, ctx->ct_vec.p + K, (size_t)K * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    FV_HIP(hipStreamSynchronize(ctx->stream));
    float ms = 0.f;
    FV_HIP(hipEventElapsedTime(&ms, ctx->ev_start, ctx->ev_stop));
    int worst = FV_OK;
    for (int s = 0; s < nseq; ++s) {
        const double ll = as_double(res[fvs::NCOUNTERS + (size_t)s]);
        const int st = ll > -HUGE_VAL ? FV_OK : FV_ERR_NO_PRED;
        if (loglik_out) loglik_out[s] = ll;
        if (status_out) status_out[s] = st;
        worst = std::min(worst, st);
        if (st == FV_OK) cs.times += offsets[s + 1] - offsets[s]; else cs.dead_sequences += 1;
    }
    cs.gpu_ms = ms; cs.sequences = nseq;
    cs.step_launches = steps.step_launches; cs.task_steps = steps.task_steps;
    cs.wide_times = (long long)res[fvs::NCOUNTERS + (size_t)nseq];
    cs.call_ms = ms_since(t0);
    cs.device_bytes = (long long)fvi::device_bytes(ctx);
    ctx->ct_stats = cs; ctx->ct_any = true;
    return worst;
}

}  // namespace

int fvi::sumprod_setup(fv_ctx *ctx)
{
    const void *steps[] = { reinterpret_cast<const void *>(&fvs::sumprod_step<1>), reinterpret_cast<const void *>(&fvs::sumprod_step<2>),
                            reinterpret_cast<const void *>(&fvs::sumprod_step<4>),
                            reinterpret_cast<const void *>(&fvs::sumprod_step_csr<1, false>), reinterpret_cast<const void *>(&fvs::sumprod_step_csr<2, false>),
                            reinterpret_cast<const void *>(&fvs::sumprod_step_csr<4, false>),
                            reinterpret_cast<const void *>(&fvs::sumprod_back_csr<1, false>), reinterpret_cast<const void *>(&fvs::sumprod_back_csr<2, false>),
                            reinterpret_cast<const void *>(&fvs::sumprod_back_csr<4, false>) };
    for (const void *f : steps) FV_HIP(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, fvk::LDS_LIMIT));
    return 0;
}

extern "C" int fv_loglik(fv_ctx *ctx, const int *ob, int T, double *loglik_out)
{
    if (!ctx) return FV_ERR_ARG;
    if (T < 1 || !loglik_out) { ctx->detail = "fv_loglik: T >= 1 and loglik_out != NULL"; return FV_ERR_ARG; }
    const long long offsets[2] = { 0, T };
    return fvi::drained(ctx, loglik_batch(ctx, "fv_loglik", ob, offsets, 1, loglik_out, nullptr));
}

extern "C" int fv_loglik_batch(fv_ctx *ctx, const int *ob, const long long *offsets, int nseq, double *loglik_out, int *status_out)
{
    if (!ctx) return FV_ERR_ARG;
    return fvi::drained(ctx, loglik_batch(ctx, "fv_loglik_batch", ob, offsets, nseq, loglik_out, status_out));
}

extern "C" int fv_posteriors(fv_ctx *ctx, const int *ob, int T, float *gamma_out, long long ld, int *path_out, double *loglik_out)
{
    if (!ctx) return FV_ERR_ARG;
    return fvi::drained(ctx, posteriors(ctx, "fv_posteriors", ob, T, gamma_out, ld, path_out, loglik_out, nullptr, nullptr));
}

extern "C" int fv_test_sumprod_rows(fv_ctx *ctx, const int *ob, int T, double *alpha_out, double *beta_out)
{
    if (!ctx) return FV_ERR_ARG;
    return fvi::drained(ctx, posteriors(ctx, "fv_test_sumprod_rows", ob, T, nullptr, 0, nullptr, nullptr, alpha_out, beta_out));
}

extern "C" int fv_expected_counts(fv_ctx *ctx, const int *ob, const long long *offsets, int nseq, double *trans_out, long long ld,
                                  double *emit_out, double *init_out, double *occ_out, double *loglik_out, int *status_out)
{
    if (!ctx) return FV_ERR_ARG;
    return fvi::drained(ctx, expected_counts(ctx, ob, offsets, nseq, trans_out, ld, emit_out, init_out, occ_out, loglik_out, status_out));
}

extern "C" int fv_last_counts_stats(const fv_ctx *ctx, fv_counts_stats *out)
{
    if (!ctx || !out) return FV_ERR_ARG;
    if (!ctx->ct_any) return FV_ERR_STATE;
    *out = ctx->ct_stats;
    return FV_OK;
}

extern "C" int fv_last_sumprod_stats(const fv_ctx *ctx, fv_sumprod_stats *out)
{
    if (!ctx || !out) return FV_ERR_ARG;
    if (!ctx->sp_any) return FV_ERR_STATE;
    *out = ctx->sp_stats;
    return FV_OK;
}

extern "C" int fv_set_sparse_sumprod(fv_ctx *ctx, int on)
{
    if (!ctx) return FV_ERR_ARG;
    if (on != 0 && on != 1) { ctx->detail = "fv_set_sparse_sumprod: on is 0 (the default) or 1"; return FV_ERR_ARG; }
    FV_NO_STREAM(ctx);
    ctx->opt_sparse_sumprod = on;
    return FV_OK;
}

extern "C" int fv_test_sumprod_forms(const fv_ctx *ctx, unsigned long long *mask_out)
{
    if (!ctx || !mask_out) return FV_ERR_ARG;
    if (!ctx->sp_any) return FV_ERR_STATE;
    *mask_out = ctx->sp_forms;
    return FV_OK;
}
