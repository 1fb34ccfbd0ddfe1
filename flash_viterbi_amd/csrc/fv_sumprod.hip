// fv_sumprod.hip — fv_loglik / fv_loglik_batch / fv_posteriors: the sum-product kernels and their driver.
// One driver runs forward passes of any number of sequences in lock-step (two float64 rows each); fv_posteriors keeps
// every row of one sequence, runs the backward pass on the transposed table and finishes with the gamma kernel.
#include "fv_internal.h"
#include "flashvit_testing.h"
#include "fv_sumprod_kernels.hip.inc"

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

template <int NB>
void launch_step_nb(fv_ctx *ctx, const StepTask *tasks, const float *tab)
{
    fvs::StepArgs<NB> a;
    for (int b = 0; b < NB; ++b) a.t[b] = tasks[b];
    const int ntiles = (ctx->K + fvk::TILE_W - 1) / fvk::TILE_W;
    hipLaunchKernelGGL(fvs::sumprod_step<NB>, dim3(ntiles), dim3(fvs::BLOCK), step_lds_bytes(NB, ctx->nrows), ctx->stream, a, tab,
                       ctx->K, ctx->nrows, ctx->sp_res.p);
}

// n tasks in launches of the largest instantiation that fits the cap and what is left: every task's bits are those of
// a launch of its own
int launch_steps(fv_ctx *ctx, const std::vector<StepTask> &tasks, const float *tab, int cap, fv_sumprod_stats &st)
{
    size_t at = 0;
    while (at < tasks.size()) {
        int nb = 1;
        while (nb * 2 <= cap && (size_t)nb * 2 <= tasks.size() - at) nb *= 2;
        if (nb == 4) launch_step_nb<4>(ctx, &tasks[at], tab);
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
    if (ctx->csr) {
        ctx->detail = w + ": models set by fv_set_model_sparse are not supported (the backward pass needs the out-edge form "
                          "on the device); set the model with fv_set_model";
        return FV_ERR_UNSUPPORTED;
    }
    if (batch_cap(ctx) < 1) {
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

struct Call {
    clk::time_point t0 = clk::now();
    fv_sumprod_stats st{};
};

int begin_call(fv_ctx *ctx, Call &c, int passes, int cap, size_t nres)
{
    c.st.passes = passes; c.st.batch_cap = cap;
    c.st.table_bytes_per_step = 4ll * ((ctx->K + fvk::TILE_W - 1) / fvk::TILE_W) * ctx->nrows * fvk::TILE_W;
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

    const int K = ctx->K, cap = batch_cap(ctx);
    const size_t tab = (size_t)((K + fvk::TILE_W - 1) / fvk::TILE_W) * ctx->nrows * fvk::TILE_W, nres = fvs::NCOUNTERS + (size_t)nseq;
    fvi::Wants wants;
    wants.what = w + " workspace"; wants.dominant = "linear table " + std::to_string(4ull * tab);
    wants.add(ctx->SPA, tab); wants.add(ctx->sp_rows, (size_t)nseq * 2 * K); wants.add(ctx->sp_res, nres);
    if (int rc = fvi::grant(ctx, wants, true)) return rc;

    Call c;
    int rc = 0;
    if ((rc = begin_call(ctx, c, 1, cap, nres)) || (rc = build_table(ctx, false))) return rc;
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
        if ((rc = launch_steps(ctx, tasks, ctx->SPA.p, cap, c.st))) return rc;
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
    const int K = ctx->K, cap = batch_cap(ctx);
    bool gamma_on_device = false;
    if (gamma_out) {
        const fvi::PointerPlace at = fvi::pointer_place(gamma_out);
        gamma_on_device = at.on_device;
        if (at.on_device && at.device != ctx->device) { ctx->detail = w + ": gamma_out lies on another device than the context"; return FV_ERR_ARG; }
    }
    const size_t tab = (size_t)((K + fvk::TILE_W - 1) / fvk::TILE_W) * ctx->nrows * fvk::TILE_W, nres = fvs::NCOUNTERS + 1;
    const size_t cells = (size_t)T * K;
    fvi::Wants wants;
    wants.what = w + " workspace"; wants.dominant = "alpha and beta rows " + std::to_string(16ull * cells);
    wants.add(ctx->SPA, tab); wants.add(ctx->SPAT, tab); wants.add(ctx->sp_rows, cells); wants.add(ctx->sp_beta, cells);
    wants.add(ctx->sp_res, nres); wants.add(ctx->sp_path, (size_t)T);
    if (gamma_out && !gamma_on_device) wants.add(ctx->sp_gamma, cells);
    if (int rc = fvi::grant(ctx, wants, true)) return rc;

    Call c;
    int rc = 0;
    if ((rc = begin_call(ctx, c, 2, cap, nres)) || (rc = build_table(ctx, false)) || (rc = build_table(ctx, true))) return rc;
    double *alpha = ctx->sp_rows.p, *beta = ctx->sp_beta.p;
    auto emis = [&](int t) { return ctx->view.lb64 + (size_t)ob[t] * K; };
    std::vector<StepTask> one(1);
    one[0] = { ctx->LPi64.p, nullptr, emis(0), alpha };
    if ((rc = launch_small(ctx, one, false))) return rc;
    for (int t = 1; t < T; ++t) {
        one[0] = { alpha + (size_t)(t - 1) * K, nullptr, emis(t), alpha + (size_t)t * K };
        if ((rc = launch_steps(ctx, one, ctx->SPA.p, cap, c.st))) return rc;
    }
    double *d_ll = reinterpret_cast<double *>(ctx->sp_res.p + fvs::NCOUNTERS);
    one[0] = { alpha + (size_t)(T - 1) * K, nullptr, nullptr, d_ll };
    if ((rc = launch_small(ctx, one, true))) return rc;
    one[0] = { nullptr, nullptr, nullptr, beta + (size_t)(T - 1) * K };
    if ((rc = launch_small(ctx, one, false))) return rc;
    for (int t = T - 2; t >= 0; --t) {
        one[0] = { beta + (size_t)(t + 1) * K, emis(t + 1), nullptr, beta + (size_t)t * K };
        if ((rc = launch_steps(ctx, one, ctx->SPAT.p, cap, c.st))) return rc;
    }
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

}  // namespace

int fvi::sumprod_setup(fv_ctx *ctx)
{
    const void *steps[] = { reinterpret_cast<const void *>(&fvs::sumprod_step<1>), reinterpret_cast<const void *>(&fvs::sumprod_step<2>),
                            reinterpret_cast<const void *>(&fvs::sumprod_step<4>) };
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

extern "C" int fv_last_sumprod_stats(const fv_ctx *ctx, fv_sumprod_stats *out)
{
    if (!ctx || !out) return FV_ERR_ARG;
    if (!ctx->sp_any) return FV_ERR_STATE;
    *out = ctx->sp_stats;
    return FV_OK;
}
