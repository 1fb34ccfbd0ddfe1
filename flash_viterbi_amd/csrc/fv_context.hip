// fv_context.hip — context life cycle, model upload, options, workspace and the decode epilogue of libflashvit.so.
// No kernels of its own: the full-state ones live in fv_full.hip, the FLASH-BS ones in fv_beam.hip.
#include "fv_internal.h"
#include "flashvit_testing.h"

namespace fvi {

size_t device_bytes(const fv_ctx *c)
{
    size_t sum = 0;
    c->each_buffer([&](const auto &b) { sum += b.bytes(); });
    return sum;
}

// ints in front of the answers in the result block: the counters (64-bit each), then the scores (one per sequence)
// padded to a multiple of four
inline size_t pack_head(int nscores) { return 2 * FV_NCOUNTERS + (size_t)std::max(4, round_up(nscores, 4)); }

// result block + the staged observations
static size_t pack_ints(const fv_ctx *ctx, int T, int nscores) { return pack_head(nscores) + (size_t)T * std::max(1, ctx->nranks) + (size_t)T; }

int grant(fv_ctx *ctx, const Wants &w, bool check)
{
    if (check) {
        // A batch's working set grows with the total length (arg rows: T * K int32): sized in 64 bits and compared with
        // what the device has free (plus what growing a buffer releases first) before anything is allocated.
        unsigned long long grow = 0, released = 0;
        for (const Wants::Want &x : w.list)
            if (x.n > x.have) { grow += (unsigned long long)x.n * x.elem; released += (unsigned long long)x.have * x.elem; }
        if (grow) {
            size_t free_b = 0, total_b = 0;
            FV_HIP(hipMemGetInfo(&free_b, &total_b));
            if (grow > (unsigned long long)free_b + released) {
                ctx->detail = w.what + ": " + std::to_string(grow) + " bytes needed (" + w.dominant + "), " +
                              std::to_string((unsigned long long)free_b + released) + " bytes of device memory free";
                return FV_ERR_NOMEM;
            }
        }
    }
    for (const Wants::Want &x : w.list) FV_HIP(x.ensure(x.buf, x.n));
    return 0;
}

int ensure_workspace(fv_ctx *ctx, int T, size_t rows_needed, int nscores, Wants w)
{
    const size_t want_rows = rows_needed * 2 * (size_t)ctx->nrows;
    const size_t want_pack = pack_ints(ctx, T, nscores);
    const bool rows_grow = want_rows > ctx->d_rows.n;
    w.add(ctx->d_ob, (size_t)T); w.add(ctx->d_ans, (size_t)T); w.add(ctx->d_bp, (size_t)T * ctx->K);
    w.add(ctx->d_rows, want_rows); w.add(ctx->d_pack, want_pack);
    if (nscores > 1 && w.what.empty()) { w.what = "batch workspace"; w.dominant = "arg rows " + std::to_string(4ull * T * ctx->K); }
    if (int rc = grant(ctx, w, nscores > 1)) return rc;
    if (rows_grow) FV_HIP(hipMemsetAsync(ctx->d_rows.p, 0, want_rows * sizeof(float), ctx->stream));   // row pads stay zero
    FV_HIP(ctx->d_score.ensure((size_t)std::max(4, nscores)));
    FV_HIP(ctx->d_counters.ensure(FV_NCOUNTERS));
    if (ctx->comm || ctx->group) FV_HIP(ctx->d_gather.ensure((size_t)T * ctx->nranks));
    if (want_pack > ctx->h_pin_n) {
        if (ctx->h_pin) { (void)hipHostFree(ctx->h_pin); ctx->h_pin = nullptr; ctx->h_pin_n = 0; }
        FV_HIP(hipHostMalloc(reinterpret_cast<void **>(&ctx->h_pin), want_pack * sizeof(int), hipHostMallocDefault));
        ctx->h_pin_n = want_pack;
    }
    return 0;
}

int ensure_flat_workspace(fv_ctx *ctx, int T, size_t passes, long long arg_rows, int chain_len)
{
    Wants w;
    const size_t want_rows = passes * 2 * (size_t)ctx->nrows;
    const bool rows_grow = want_rows > ctx->d_rows.n;
    w.add(ctx->d_rows, want_rows); w.add(ctx->d_snap, (size_t)T); w.add(ctx->d_flat_bp, (size_t)std::max(arg_rows, 1ll) * ctx->K);
    w.add(ctx->d_chain, (size_t)std::max(chain_len, 1)); w.add(ctx->d_flat, std::max(passes, (size_t)1));
    w.what = "flat generations workspace"; w.dominant = "private arg rows " + std::to_string(4ull * (unsigned long long)arg_rows * ctx->K);
    if (int rc = grant(ctx, w, true)) return rc;
    if (rows_grow) FV_HIP(hipMemsetAsync(ctx->d_rows.p, 0, want_rows * sizeof(float), ctx->stream));   // row pads stay zero
    return 0;
}

// the result block: [counters | nscore scores, padded to `head` | the answers of all sequences, or the gathered answers]
__global__ void pack_result(const unsigned long long *counters, const float *score, int nscore, size_t head, const int *ans,
                            size_t nans, int *out)
{
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nthr = (size_t)gridDim.x * blockDim.x;
    if (tid < 2 * FV_NCOUNTERS) out[tid] = reinterpret_cast<const int *>(counters)[tid];
    for (size_t i = tid; i < (size_t)nscore; i += nthr) out[2 * FV_NCOUNTERS + i] = __float_as_int(score[i]);
    for (size_t i = tid; i < nans; i += nthr) out[head + i] = ans[i];
}

__global__ void clear_outputs(unsigned long long *counters, int *ans, int T)
{
    const int tid = blockIdx.x * blockDim.x + threadIdx.x;
    if (tid < FV_NCOUNTERS) counters[tid] = 0ull;
    for (int i = tid; i < T; i += gridDim.x * blockDim.x) ans[i] = 0;
}

int emission_view(fv_ctx *ctx, const int *&ob, long long T)
{
    if (ob) {
        ctx->view.lb32 = ctx->LB32T.p; ctx->view.lb64 = ctx->LB64T.p; ctx->view.nsym = ctx->M;
        ctx->view.logs_nonpositive = ctx->logs_nonpositive;
        return 0;
    }
    // (a context without a model has nothing staged: fv_set_emissions needs K, the model setters drop the rows)
    if (ctx->emis_rows == 0) { ctx->detail = "ob == NULL: no emission scores are staged (fv_set_emissions)"; return FV_ERR_ARG; }
    if (T < 1 || T > ctx->emis_rows) {
        ctx->detail = "ob == NULL: " + std::to_string(T) + " times asked for, " + std::to_string(ctx->emis_rows) + " rows of emission scores staged";
        return FV_ERR_ARG;
    }
    try {
        for (size_t j = ctx->h_iota.size(); j < (size_t)T; ++j) ctx->h_iota.push_back((int)j);
    } catch (const std::bad_alloc &) { return FV_ERR_NOMEM; }
    ob = ctx->h_iota.data();
    ctx->view.lb32 = ctx->E32.p; ctx->view.lb64 = ctx->E64.p; ctx->view.nsym = (int)ctx->emis_rows;
    ctx->view.logs_nonpositive = ctx->logs_nonpositive && !ctx->emis_positive;
    return 0;
}

int begin_decode(fv_ctx *ctx, const int *ob, int T)
{
    ctx->h_ob.assign(ob, ob + T);
    // (the pinned block's tail is free until the epilogue: the sequence travels through it, one asynchronous copy)
    int *stage = ctx->h_pin + (ctx->h_pin_n - (size_t)T);
    std::memcpy(stage, ob, (size_t)T * sizeof(int));
    FV_HIP(hipMemcpyAsync(ctx->d_ob.p, stage, (size_t)T * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(clear_outputs, dim3(16), dim3(256), 0, ctx->stream, ctx->d_counters.p, ctx->d_ans.p, T);
    FV_HIP(hipGetLastError());
    return 0;
}

int batch_lengths(fv_ctx *ctx, const char *who, const int *&ob, const long long *offsets, int nseq, int n_split, int mode,
                  const int *path_out, std::vector<int> &lengths)
{
    if (!offsets || !path_out || nseq < 1 || n_split < 1) return FV_ERR_ARG;
    if (mode != FV_MODE_REFERENCE && mode != FV_MODE_SINGLE_PASS) return FV_ERR_ARG;
    const std::string w = who;
    if (offsets[0] != 0) { ctx->detail = w + ": offsets[0] must be 0"; return FV_ERR_ARG; }
    lengths.resize((size_t)nseq);
    for (int s = 0; s < nseq; ++s) {
        const long long len = offsets[s + 1] - offsets[s];
        if (len < 0) { ctx->detail = w + ": offsets decrease at sequence " + std::to_string(s); return FV_ERR_ARG; }
        if (len < 2) { ctx->detail = w + ": sequence " + std::to_string(s) + " has fewer than 2 observations"; return FV_ERR_ARG; }
        if (offsets[s + 1] > 0x7fffffffLL) { ctx->detail = w + ": more than 2^31 - 1 observations in all (at sequence " + std::to_string(s) + ")"; return FV_ERR_ARG; }
        lengths[(size_t)s] = (int)len;
    }
    if (int rc = emission_view(ctx, ob, offsets[nseq])) return rc;       // (ob == NULL: sequence s on staged rows offsets[s] ..)
    return ctx->K == 0 ? FV_ERR_STATE : 0;
}

int batch_symbols(fv_ctx *ctx, const char *who, const int *ob, const long long *offsets, int nseq)
{
    for (int s = 0; s < nseq; ++s)
        for (long long j = offsets[s]; j < offsets[s + 1]; ++j)
            if (ob[j] < 0 || ob[j] >= ctx->view.nsym) {
                ctx->detail = std::string(who) + ": sequence " + std::to_string(s) + " holds a symbol outside [0, M) at position " + std::to_string(j - offsets[s]);
                return FV_ERR_ARG;
            }
    return 0;
}

int batch_plan(fv_ctx *ctx, const char *who, const std::vector<int> &lengths, int n_split, int mode, fv::Plan &plan)
{
    int bad = -1;
    const int rc = fv::build_forest(lengths.data(), (int)lengths.size(), n_split, mode, plan, &bad);
    if (rc)
        ctx->detail = std::string(who) + ": sequence " + std::to_string(bad) + " of length " + std::to_string(lengths[(size_t)std::max(bad, 0)]) +
                      " has no plan for n_split = " + std::to_string(n_split) + " (T == 2 * n_split with n_split > 2)";
    return rc;
}

std::vector<std::vector<fv::Pass>> deal_passes(const fv_ctx *ctx, const fv::Plan &plan, size_t *most)
{
    std::vector<std::vector<fv::Pass>> gens(plan.generations());
    for (const fv::Pass &p : plan.passes)
        if (p.owner < 0 || p.owner % ctx->nranks == ctx->rank) gens[p.generation].push_back(p);
    if (most) {
        *most = 1;
        for (const auto &g : gens) *most = std::max(*most, g.size());
    }
    return gens;
}

// statistics of a finished decode: event times and the device counters the result block brought back
static int read_stats(fv_ctx *ctx, const unsigned long long *counters, clk::time_point t0, size_t nprof)
{
    fv_stats &st = ctx->stats;
    st.decode_ms = ms_since(t0);
    float ms = 0.f;
    FV_HIP(hipEventElapsedTime(&ms, ctx->ev_start, ctx->ev_stop)); st.gpu_ms = ms;
    FV_HIP(hipEventElapsedTime(&ms, ctx->ev_start, ctx->ev_top)); st.top_pass_ms = ms;
    FV_HIP(hipEventElapsedTime(&ms, ctx->ev_s0, ctx->ev_s1)); st.top_steps_ms = ms;
    st.step_kernel_ms = 0;
    for (size_t i = 0; i + 1 < nprof; i += 2) {
        FV_HIP(hipEventElapsedTime(&ms, ctx->prof_events[i], ctx->prof_events[i + 1]));
        st.step_kernel_ms += ms;
    }
    st.refine_near = (long long)counters[fvk::CNT_REFINE_NEAR];
    st.refine_rescan = (long long)counters[fvk::CNT_REFINE_RESCAN];
    st.beam_exact_sets = (long long)counters[fvk::CNT_BEAM_EXACT_SETS];
    st.beam_dup_cols = (long long)counters[fvk::CNT_BEAM_DUP_COLS];
    st.beam_dup_steps = (long long)counters[fvk::CNT_BEAM_DUP_STEPS];
    st.beam_ties = (long long)counters[fvk::CNT_BEAM_TIES];
    st.beam_cand_selects = (long long)counters[fvk::CNT_BEAM_CAND_SELECTS];
    st.refine_saturated = (long long)counters[fvk::CNT_REFINE_SATURATED];
    st.beam_spec_steps = (long long)counters[fvk::CNT_BEAM_SPEC_STEPS];
    st.beam_reach_events = (long long)counters[fvk::CNT_BEAM_REACH_EVENTS];
    st.beam_list_short = (long long)counters[fvk::CNT_BEAM_LIST_SHORT];
    st.beam_list_long = (long long)counters[fvk::CNT_BEAM_LIST_LONG];
    st.beam_list_entries = (long long)counters[fvk::CNT_BEAM_LIST_ENTRIES];
    st.beam_chain_cuts = (long long)counters[fvk::CNT_BEAM_CHAIN_CUTS];
    st.bt_restarts = (long long)counters[fvk::BT_COUNTER];
    if (counters[fvk::FLAT_COUNTER]) {               // the resolver of a flat decode met a generation it could not commit
        st.flat_first_miss = (int)(counters[fvk::FLAT_COUNTER] >> 32);
        st.flat_missed = (int)(counters[fvk::FLAT_COUNTER] & 0xffffffffull);
    }
    if (counters[fvk::CNT_HANDSHAKE_TIMEOUT]) { ctx->detail = "heap replay: producer/consumer hand-shake timed out"; return FV_ERR_DEVICE; }
    st.device_bytes = (long long)fvi::device_bytes(ctx);
    st.ranks = ctx->nranks;
    return 0;
}

int finish_decode(fv_ctx *ctx, const fv::Plan &plan, const long long *offsets, int nseq, int *path_out, float *score_out,
                  int *status_out, clk::time_point t0, size_t nprof, bool beam)
{
    const int T = (int)offsets[nseq];
    const bool gathered = (ctx->comm || ctx->group) && !plan.seg_L.empty();      // (never a batch: they take no partition)
    if (gathered)
        if (int rc = gather_answers(ctx, T)) return rc;   // one RCCL all-gather of every rank's answer array (fv_comm.hip)
    FV_HIP(hipEventRecord(ctx->ev_stop, ctx->stream));
    // [counters | scores | answers] in one block, one device-to-host copy into pinned memory
    const size_t nans = gathered ? (size_t)T * ctx->nranks : (size_t)T, head = pack_head(nseq), total = head + nans;
    hipLaunchKernelGGL(pack_result, dim3(64), dim3(256), 0, ctx->stream, ctx->d_counters.p, ctx->d_score.p, nseq, head,
                       gathered ? ctx->d_gather.p : ctx->d_ans.p, nans, ctx->d_pack.p);
    FV_HIP(hipGetLastError());
    FV_HIP(hipMemcpyAsync(ctx->h_pin, ctx->d_pack.p, total * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    FV_HIP(hipStreamSynchronize(ctx->stream));
    for (hipGraphExec_t ge : ctx->graphs) (void)hipGraphExecDestroy(ge);
    ctx->graphs.clear();
    unsigned long long counters[FV_NCOUNTERS];
    std::memcpy(counters, ctx->h_pin, sizeof counters);
    if (gathered) {
        const std::vector<int> host(ctx->h_pin + head, ctx->h_pin + head + nans);
        merge_gathered(plan, host, T, ctx->nranks, path_out);
    } else {
        std::memcpy(path_out, ctx->h_pin + head, nans * sizeof(int));
    }
    if (score_out) std::memcpy(score_out, ctx->h_pin + 2 * FV_NCOUNTERS, (size_t)nseq * sizeof(float));
    if (int rc = read_stats(ctx, counters, t0, nprof)) return rc;
    // entries without a predecessor (beam: after a beam miss), per sequence
    int worst = FV_OK, warn = FV_OK;
    for (int s = 0; s < nseq; ++s) {
        bool neg = false;
        for (long long j = offsets[s]; j < offsets[s + 1]; ++j) neg |= path_out[j] < 0;
        const int st = !neg ? FV_OK : beam ? FV_WARN_BEAM_MISS : FV_ERR_NO_PRED;
        if (status_out) status_out[s] = st;
        worst = std::min(worst, st);
        warn = std::max(warn, st);
    }
    return worst < 0 ? worst : warn;
}

// A decode that fails after its first enqueue must not leave kernels running on ctx->stream: the next call
// may grow (hipFree + hipMalloc) a workspace buffer they still use.  Every entry point funnels its error
// returns through here: end a capture left open, wait for the stream, drop the captured graphs.
int drained(fv_ctx *ctx, int rc)
{
    if (rc >= 0) return rc;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(ctx->stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) {
        hipGraph_t g = nullptr;
        (void)hipStreamEndCapture(ctx->stream, &g);
        if (g) (void)hipGraphDestroy(g);
    }
    (void)hipStreamSynchronize(ctx->stream);
    for (hipStream_t a : ctx->aux) if (a) (void)hipStreamSynchronize(a);
    for (hipGraphExec_t ge : ctx->graphs) (void)hipGraphExecDestroy(ge);
    ctx->graphs.clear();
    (void)hipGetLastError();          // the failure is reported through rc / detail, not left sticky
    return rc;
}

}  // namespace fvi


// ------------------------------------------------------------------ C ABI

extern "C" int fv_create(fv_ctx **out, int device)
{
    if (!out) return FV_ERR_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return FV_ERR_DEVICE;
    fv_ctx *ctx = new (std::nothrow) fv_ctx();
    if (!ctx) return FV_ERR_NOMEM;
    ctx->device = device;
    auto fail = [&](int rc) { fv_destroy(ctx); return rc; };
    if (hipSetDevice(device) != hipSuccess) return fail(FV_ERR_DEVICE);
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) return fail(FV_ERR_DEVICE);
    for (int q = 0; q < fv_ctx::BEAM_AUX; ++q)
        if (hipStreamCreateWithFlags(&ctx->aux[q], hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&ctx->ev_join[q], hipEventDisableTiming) != hipSuccess) return fail(FV_ERR_DEVICE);
    if (hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming) != hipSuccess) return fail(FV_ERR_DEVICE);
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device) == hipSuccess && cus > 0) ctx->num_cus = cus;
    }
    if (hipEventCreate(&ctx->ev_start) != hipSuccess || hipEventCreate(&ctx->ev_stop) != hipSuccess ||
        hipEventCreate(&ctx->ev_top) != hipSuccess || hipEventCreate(&ctx->ev_s0) != hipSuccess ||
        hipEventCreate(&ctx->ev_s1) != hipSuccess)
        return fail(FV_ERR_DEVICE);
    int rc = 0;
    if ((rc = fvi::full_setup(ctx)) || (rc = fvi::beam_setup(ctx)) || (rc = fvi::sumprod_setup(ctx))) return fail(rc);
    *out = ctx;
    return FV_OK;
}

extern "C" void fv_destroy(fv_ctx *ctx)
{
    if (!ctx) return;
    if (ctx->group) {
        // the handle of a multi-device context (member 0) takes the other members and the group with it
        fv_group *g = ctx->group;
        if (ctx->group_rank != 0) return;        // members are owned by the group's handle
        for (fv_ctx *m : g->members) m->group = nullptr;
        for (size_t r = g->members.size(); r-- > 1;) fv_destroy(g->members[r]);
        for (hipEvent_t e : g->ans_ready) if (e) (void)hipEventDestroy(e);
        delete g;
    }
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    fvi::stream_drop(ctx);
    if (ctx->comm) ncclCommDestroy(ctx->comm);
    if (ctx->h_pin) { (void)hipHostFree(ctx->h_pin); ctx->h_pin = nullptr; ctx->h_pin_n = 0; }
    for (hipEvent_t e : ctx->prof_events) (void)hipEventDestroy(e);
    if (ctx->ev_start) (void)hipEventDestroy(ctx->ev_start);
    if (ctx->ev_stop) (void)hipEventDestroy(ctx->ev_stop);
    if (ctx->ev_top) (void)hipEventDestroy(ctx->ev_top);
    if (ctx->ev_s0) (void)hipEventDestroy(ctx->ev_s0);
    if (ctx->ev_s1) (void)hipEventDestroy(ctx->ev_s1);
    if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
    for (int q = 0; q < fv_ctx::BEAM_AUX; ++q) {
        if (ctx->ev_join[q]) (void)hipEventDestroy(ctx->ev_join[q]);
        if (ctx->aux[q]) (void)hipStreamDestroy(ctx->aux[q]);
    }
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;          // (the device buffers free themselves)
}

namespace fvi {      // what a context holds — model, emission map, staged scores: one rule each

// fn(member) for members 0 .. n-1 (or n-1 .. 1 and the handle last); stops at the first non-zero return and copies that
// member's detail to the handle.  Name fn's parameter `ctx`: FV_HIP inside it then reports into the member.
template <class F>
static int for_each_member(fv_ctx *ctx, F &&fn, bool handle_last = false)
{
    const int n = group_size(ctx);
    for (int i = 0; i < n; ++i) {
        fv_ctx *m = group_member(ctx, handle_last ? n - 1 - i : i);
        if (int rc = fn(m)) { if (m != ctx) ctx->detail = m->detail; return rc; }
    }
    return 0;
}

// "Nothing is staged any more" on one member: the rows, and with_map the class count of the emission map as well.
static void drop_emissions(fv_ctx *m, bool with_map) { m->emis_rows = 0; m->emis_positive = false; if (with_map) m->emis_P = 0; }

// ... on every member, and in the handle's statistics: the row count, and with_ms the staging time as well
static void drop_group_emissions(fv_ctx *ctx, bool with_map, bool with_ms)
{
    for_each_member(ctx, [&](fv_ctx *m) { drop_emissions(m, with_map); return 0; });
    ctx->stats.emission_rows = 0;
    if (with_ms) ctx->stats.set_emissions_ms = 0.0;
}

// a host table to the device: the buffer grown to n elements, then one blocking copy
template <typename T>
static int upload(fv_ctx *ctx, DevBuf<T> &buf, const T *data, size_t n)
{
    FV_HIP(buf.ensure(n));
    FV_HIP(hipMemcpy(buf.p, data, n * sizeof(T), hipMemcpyHostToDevice));
    return 0;
}

// What both model setters do first on a device: the context holds NO model from here until every upload has succeeded
// (K = 0 makes every decode return FV_ERR_STATE), so a failure half way (e.g. NOMEM on a larger second model) can never
// pair the old sizes with partly new tables.  Every table that is rebuilt rather than overwritten in place is released;
// keep_dense: the tile-major tables of fv_set_model stay allocated, to be overwritten (log B and log Pi always do).
static void drop_model(fv_ctx *ctx, bool keep_dense)
{
    ctx->K = 0; ctx->M = 0; ctx->nrows = 0; ctx->full_ok = false; ctx->u16_ok = false; ctx->laq16_ready = false;
    ctx->rowq_ready = false; ctx->beam_q16_ready = false; ctx->csr = false;
    drop_emissions(ctx, true);           // staged emission scores belong to the model they were staged under, and so does the map
    (void)hipStreamSynchronize(ctx->stream);
    ctx->LA64R.release(); ctx->LAQ16R.release();
    ctx->SPA.release(); ctx->SPAT.release(); ctx->spa_ready = ctx->spat_ready = false;   // rebuilt by the next fv_loglik / fv_posteriors
    ctx->SPdata.release(); ctx->SPoff.release(); ctx->SPnwb.release();
    ctx->CSk.release(); ctx->CSq.release(); ctx->CS64.release(); ctx->CSoff.release(); ctx->CSnwb.release();
    ctx->CRptr.release(); ctx->CRcol.release(); ctx->CRlog.release(); ctx->csr_nnz = 0; ctx->csr_vectors = 0;
    ctx->CSlin.release(); ctx->CRlin.release(); ctx->cslin_ready = ctx->crlin_ready = false;   // (fv_set_sparse_sumprod: rebuilt on first use)
    ctx->d_csr_acc.release(); ctx->d_csr_tie.release();      // (sized by K; a dense-set model never reads them)
    ctx->EMap.release();
    if (!keep_dense) { ctx->LA32.release(); ctx->LA16.release(); ctx->LAQ16.release(); ctx->LA64.release(); }
}

// ... and last: log B and log Pi, then the sizes that make the context hold the model, and statistics from zero
static int finish_upload(fv_ctx *ctx, const HostTables &e)
{
    ctx->window16 = e.window16; ctx->windowq = e.windowq; ctx->qscale = e.qscale; ctx->density = e.density;
    int rc = 0;
    if ((rc = upload(ctx, ctx->LB64T, e.b64.data(), e.b64.size())) || (rc = upload(ctx, ctx->LB32T, e.b32.data(), e.b32.size())) ||
        (rc = upload(ctx, ctx->LPi64, e.pi64.data(), e.pi64.size())))
        return rc;
    ctx->K = e.K; ctx->M = e.M; ctx->nrows = e.nrows;
    ctx->logs_nonpositive = !e.any_big;
    ctx->stats = fv_stats{};
    ctx->stats.device_bytes = (long long)device_bytes(ctx);
    return FV_OK;
}

// Device side of fv_set_model, once per device: the tables are overwritten in place (grown in the order LAQ16, SP*, LA64, LA32, LA16).
static int upload_tables(fv_ctx *ctx, const HostTables &h)
{
    FV_HIP(hipSetDevice(ctx->device));
    drop_model(ctx, true);
    const size_t tab = h.tab, ntiles = (size_t)h.ntiles;
    int rc = 0;
    if (h.full_ok) {
        if ((rc = upload(ctx, ctx->LAQ16, h.hq.data(), tab))) return rc;
        if (!h.sp.empty())
            if ((rc = upload(ctx, ctx->SPdata, h.sp.data(), h.sp.size())) || (rc = upload(ctx, ctx->SPoff, h.sp_off.data(), ntiles)) ||
                (rc = upload(ctx, ctx->SPnwb, h.sp_nwb.data(), ntiles)))
                return rc;
    }
    FV_HIP(ctx->LA64.ensure(tab));
    if (h.full_ok) {
        if ((rc = upload(ctx, ctx->LA32, h.h32.data(), tab)) || (rc = upload(ctx, ctx->LA16, h.h16.data(), tab))) return rc;
    } else {
        ctx->LA32.release(); ctx->LA16.release(); ctx->LAQ16.release();
    }
    if ((rc = upload(ctx, ctx->LA64, h.h64.data(), tab)) || (rc = finish_upload(ctx, h))) return rc;
    ctx->laq16_ready = h.full_ok;          // beyond the float32 limit: built on first use (fv_full.hip)
    ctx->full_ok = h.full_ok; ctx->u16_ok = h.u16_ok;     // LA64R / LAQ16R: rebuilt on the next beam decode
    return FV_OK;
}

// Device side of fv_set_model_sparse, once per device; as upload_tables, the context holds no model until every upload
// has succeeded.  The dense tables of an earlier fv_set_model are released.
static int upload_csr(fv_ctx *ctx, const HostCsr &h, const long long *row_ptr, const int *col)
{
    const HostTables &e = h.e;
    FV_HIP(hipSetDevice(ctx->device));
    drop_model(ctx, false);
    const size_t nnz = h.rlog.size(), nv = h.ck.size(), ntiles = (size_t)e.ntiles;
    int rc = 0;
    // (an empty model still has tables: one element each)
    FV_HIP(ctx->CSk.ensure(std::max<size_t>(nv, 1)));
    FV_HIP(ctx->CSq.ensure(std::max<size_t>(nv, 1)));
    FV_HIP(ctx->CS64.ensure(std::max<size_t>(nv * 4, 1)));
    if (nv)
        if ((rc = upload(ctx, ctx->CSk, h.ck.data(), nv)) || (rc = upload(ctx, ctx->CSq, h.cq.data(), nv)) ||
            (rc = upload(ctx, ctx->CS64, h.c64.data(), nv * 4)))
            return rc;
    if ((rc = upload(ctx, ctx->CSoff, h.off.data(), ntiles)) || (rc = upload(ctx, ctx->CSnwb, h.nwb.data(), ntiles)) ||
        (rc = upload(ctx, ctx->CRptr, row_ptr, (size_t)e.K + 1)))
        return rc;
    FV_HIP(ctx->CRcol.ensure(std::max<size_t>(nnz, 1)));
    FV_HIP(ctx->CRlog.ensure(std::max<size_t>(nnz, 1)));
    if (nnz)
        if ((rc = upload(ctx, ctx->CRcol, col, nnz)) || (rc = upload(ctx, ctx->CRlog, h.rlog.data(), nnz))) return rc;
    if ((rc = finish_upload(ctx, e))) return rc;
    ctx->csr = true; ctx->csr_nnz = (long long)nnz; ctx->csr_vectors = (long long)nv;
    ctx->stats.density = ctx->density;
    return FV_OK;
}

}  // namespace fvi

// Both model setters: build on the host (fv_model.cpp), then for every member drop and upload.
extern "C" int fv_set_model_sparse(fv_ctx *ctx, const long long *row_ptr, const int *col, const float *val, const float *B,
                                   const float *Pi, int K, int M)
{
    if (!ctx || !row_ptr || !B || !Pi || K < 1 || M < 1) return FV_ERR_ARG;
    FV_NO_STREAM(ctx);
    auto t0 = clk::now();
    fvi::HostCsr h;
    int rc = FV_OK;
    try { rc = fvi::build_host_csr(row_ptr, col, val, B, Pi, K, M, h, ctx->detail); } catch (const std::bad_alloc &) { rc = FV_ERR_NOMEM; }
    if (rc) return rc;
    if ((rc = fvi::for_each_member(ctx, [&](fv_ctx *ctx) { return fvi::upload_csr(ctx, h, row_ptr, col); }))) return rc;
    ctx->stats.set_model_ms = ms_since(t0);
    return FV_OK;
}

extern "C" int fv_set_model(fv_ctx *ctx, const float *A, const float *B, const float *Pi, int K, int M)
{
    if (!ctx || !A || !B || !Pi || K < 1 || M < 1) return FV_ERR_ARG;
    FV_NO_STREAM(ctx);
    auto t0 = clk::now();
    fvi::HostTables h;
    int rc = fvi::build_host_tables(A, B, Pi, K, M, h, ctx->detail);
    if (rc) return rc;
    // a multi-device context uploads the same host tables to every device
    if ((rc = fvi::for_each_member(ctx, [&](fv_ctx *ctx) { return fvi::upload_tables(ctx, h); }))) return rc;
    ctx->stats.set_model_ms = ms_since(t0);
    return FV_OK;
}

namespace fvi {

PointerPlace pointer_place(const void *p)
{
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return { false, -1 }; }
    return { at.type == hipMemoryTypeDevice, at.device };
}

int emis_refusal(fv_ctx *ctx, const char *who, unsigned long long where, long long t_base)
{
    const unsigned long long K = (unsigned long long)ctx->K;
    std::string cls;
    if (ctx->emis_P) {                                      // which score of the caller's row that was
        int p = -1;
        FV_HIP(hipMemcpy(&p, ctx->EMap.p + where % K, sizeof p, hipMemcpyDeviceToHost));
        cls = ", class = " + std::to_string(p);
    }
    ctx->detail = std::string(who) + ": the score at (t = " + std::to_string(t_base + (long long)(where / K)) + ", state = " +
                  std::to_string(where % K) + cls + ") is NaN, +inf or beyond the float32 range; scores are finite or -inf";
    return FV_ERR_ARG;
}

// fv_set_emissions on one device.  A block the kernel cannot read where it lies (host memory; a multi-device context,
// whose members each take a copy) goes into a raw device buffer first, released before the call returns.
static int stage_emissions_on(fv_ctx *ctx, const EmisBlock &b, bool in_place)
{
    FV_HIP(hipSetDevice(ctx->device));
    const size_t cells = (size_t)b.n * (size_t)ctx->K, raw_bytes = in_place ? 0 : emis_raw_bytes(ctx, b);
    {   // sized in 64 bits and compared with the free device memory before anything is allocated
        unsigned long long grow = raw_bytes, released = 0;
        if (cells > ctx->E32.n) { grow += 4ull * cells; released += ctx->E32.bytes(); }
        if (cells > ctx->E64.n) { grow += 8ull * cells; released += ctx->E64.bytes(); }
        size_t free_b = 0, total_b = 0;
        FV_HIP(hipMemGetInfo(&free_b, &total_b));
        if (grow > (unsigned long long)free_b + released) {
            ctx->detail = "fv_set_emissions: " + std::to_string(grow) + " bytes needed (tables " + std::to_string(12ull * cells) +
                          ", raw copy " + std::to_string((unsigned long long)raw_bytes) + "), " +
                          std::to_string((unsigned long long)free_b + released) + " bytes of device memory free";
            return FV_ERR_NOMEM;
        }
    }
    FV_HIP(ctx->E32.ensure(cells));
    FV_HIP(ctx->E64.ensure(cells));
    FV_HIP(ctx->d_emflags.ensure(2));
    DevBuf<unsigned char> raw;
    if (!in_place) FV_HIP(raw.ensure(raw_bytes));
    unsigned long long got[2] = { 0ull, ~0ull };
    auto reset = [&]() -> int {
        FV_HIP(hipMemsetAsync(ctx->d_emflags.p, 0, sizeof(unsigned long long), ctx->stream));               // no flag
        FV_HIP(hipMemsetAsync(ctx->d_emflags.p + 1, 0xFF, sizeof(unsigned long long), ctx->stream));        // no refused index
        return 0;
    };
    if (int rc = stage_block(ctx, b, raw.p, ctx->E32.p, ctx->E64.p, ctx->d_emflags.p, reset)) return rc;
    FV_HIP(hipMemcpyAsync(got, ctx->d_emflags.p, sizeof got, hipMemcpyDeviceToHost, ctx->stream));
    FV_HIP(hipStreamSynchronize(ctx->stream));              // the one sync of the call: copies and kernel are done, `raw` can go
    if (got[0] & FV_EMIS_BAD) return emis_refusal(ctx, "fv_set_emissions", got[1], 0);
    ctx->emis_positive = (got[0] & FV_EMIS_POSITIVE) != 0;
    ctx->emis_rows = b.n;
    return FV_OK;
}

}  // namespace fvi

extern "C" int fv_set_emissions(fv_ctx *ctx, const void *scores, int dtype, int T, long long ld)
{
    if (!ctx) return FV_ERR_ARG;
    FV_NO_STREAM(ctx);
    fvi::drop_group_emissions(ctx, false, true);      // whatever happens next, the rows staged before are gone
    if (ctx->K == 0) { ctx->detail = "fv_set_emissions: no model (the row length K is the model's)"; return FV_ERR_STATE; }
    const fvi::EmisBlock b{ scores, dtype, T, ld };
    if (!fvi::emis_block_ok(ctx, b)) {
        ctx->detail = "fv_set_emissions: scores != NULL, T >= 1, ld >= K (ld >= P while an emission map is set) and dtype "
                      "FV_EMIS_LOG_F32, _F64, _F16 or _BF16";
        return FV_ERR_ARG;
    }
    auto t0 = clk::now();
    const fvi::PointerPlace at = fvi::pointer_place(scores);
    const bool single = fvi::group_size(ctx) == 1;
    const int rc = fvi::for_each_member(ctx, [&](fv_ctx *ctx) {
        const bool in_place = at.on_device && single && at.device == ctx->device;
        return fvi::drained(ctx, fvi::stage_emissions_on(ctx, b, in_place));
    });
    ctx->stats.device_bytes = (long long)fvi::device_bytes(ctx);          // (after a refusal too: the tables may have grown before it)
    if (rc) {
        fvi::for_each_member(ctx, [](fv_ctx *m) { m->emis_rows = 0; return 0; });
        return rc;
    }
    ctx->stats.set_emissions_ms = ms_since(t0);
    ctx->stats.emission_rows = T;
    return FV_OK;
}

// The map is the model's: checked on the host, then 4 * K bytes to every member.  Whatever was staged went through the
// map that is replaced, so it goes; an argument error comes before that and leaves map and rows as they were.
extern "C" int fv_set_emission_map(fv_ctx *ctx, const int *pdf_of_state, int P)
{
    if (!ctx) return FV_ERR_ARG;
    FV_NO_STREAM(ctx);
    if (ctx->K == 0) { ctx->detail = "fv_set_emission_map: no model (the map holds one entry per state of the model)"; return FV_ERR_STATE; }
    if (!pdf_of_state && P != 0) { ctx->detail = "fv_set_emission_map: pdf_of_state == NULL clears the map and takes P == 0"; return FV_ERR_ARG; }
    if (pdf_of_state) {
        if (P < 1) { ctx->detail = "fv_set_emission_map: P >= 1 score classes with a map"; return FV_ERR_ARG; }
        if (fvi::pointer_place(pdf_of_state).on_device) {
            ctx->detail = "fv_set_emission_map: pdf_of_state is a device pointer; the map is read on the host";
            return FV_ERR_ARG;
        }
        for (int i = 0; i < ctx->K; ++i)
            if (pdf_of_state[i] < 0 || pdf_of_state[i] >= P) {
                ctx->detail = "fv_set_emission_map: pdf_of_state[" + std::to_string(i) + "] = " + std::to_string(pdf_of_state[i]) +
                              " (state " + std::to_string(i) + ") lies outside [0, P = " + std::to_string(P) + ")";
                return FV_ERR_ARG;
            }
    }
    fvi::drop_group_emissions(ctx, true, true);
    const int rc = fvi::for_each_member(ctx, [&](fv_ctx *ctx) -> int {
        FV_HIP(hipSetDevice(ctx->device));
        if (!pdf_of_state) { ctx->EMap.release(); return FV_OK; }
        if (int up = fvi::upload(ctx, ctx->EMap, pdf_of_state, (size_t)ctx->K)) return up;
        ctx->emis_P = P;
        return FV_OK;
    });
    if (rc) fvi::drop_group_emissions(ctx, true, true);      // an upload failed: no map anywhere, nothing staged
    ctx->stats.device_bytes = (long long)fvi::device_bytes(ctx);
    return rc;
}

extern "C" int fv_clear_emissions(fv_ctx *ctx)
{
    if (!ctx) return FV_ERR_ARG;
    FV_NO_STREAM(ctx);
    fvi::drop_group_emissions(ctx, false, false);
    fvi::for_each_member(ctx, [](fv_ctx *m) { (void)hipSetDevice(m->device); m->E32.release(); m->E64.release(); return 0; });
    ctx->stats.device_bytes = (long long)fvi::device_bytes(ctx);
    return FV_OK;
}

// include/flashvit_testing.h: device memory for a test that has no HIP runtime of its own
extern "C" int fv_test_device_alloc(fv_ctx *ctx, size_t bytes, const void *host_src, void **out)
{
    if (!ctx || !out || bytes == 0) return FV_ERR_ARG;
    *out = nullptr;
    FV_HIP(hipSetDevice(ctx->device));
    void *p = nullptr;
    FV_HIP(hipMalloc(&p, bytes));
    if (host_src) {
        hipError_t e = hipMemcpy(p, host_src, bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) { (void)hipFree(p); FV_HIP(e); }
    }
    *out = p;
    return FV_OK;
}

extern "C" int fv_test_device_free(fv_ctx *ctx, void *p)
{
    if (!ctx) return FV_ERR_ARG;
    FV_HIP(hipSetDevice(ctx->device));
    if (p) FV_HIP(hipFree(p));
    return FV_OK;
}

// include/flashvit_testing.h: the staging kernel alone between two device events, reps launches back to back
extern "C" int fv_test_stage_emissions_ms(fv_ctx *ctx, const void *dev_scores, int dtype, int T, long long ld, int reps, float *ms_out)
{
    const fvi::EmisBlock b{ dev_scores, dtype, T, ld };
    if (!ctx || !ms_out || reps < 1 || ctx->K == 0 || !fvi::emis_block_ok(ctx, b) || ctx->group) return FV_ERR_ARG;
    FV_NO_STREAM(ctx);
    const fvi::PointerPlace at = fvi::pointer_place(dev_scores);
    if (!at.on_device || at.device != ctx->device) return FV_ERR_ARG;
    FV_HIP(hipSetDevice(ctx->device));
    fvi::drop_group_emissions(ctx, false, false);           // the tables are overwritten: nothing stays staged
    const size_t cells = (size_t)T * (size_t)ctx->K;
    FV_HIP(ctx->E32.ensure(cells));
    FV_HIP(ctx->E64.ensure(cells));
    FV_HIP(ctx->d_emflags.ensure(2));
    FV_HIP(hipMemsetAsync(ctx->d_emflags.p, 0, sizeof(unsigned long long), ctx->stream));
    FV_HIP(hipMemsetAsync(ctx->d_emflags.p + 1, 0xFF, sizeof(unsigned long long), ctx->stream));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    struct Ev { hipEvent_t &a, &b; ~Ev() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); } } ev{ e0, e1 };
    FV_HIP(hipEventCreate(&e0));
    FV_HIP(hipEventCreate(&e1));
    auto keep = [] { return 0; };           // (the words were reset above and are not judged)
    if (int rc = fvi::stage_block(ctx, b, nullptr, ctx->E32.p, ctx->E64.p, ctx->d_emflags.p, keep)) return fvi::drained(ctx, rc);      // warm
    FV_HIP(hipEventRecord(e0, ctx->stream));
    for (int r = 0; r < reps; ++r)
        if (int rc = fvi::stage_block(ctx, b, nullptr, ctx->E32.p, ctx->E64.p, ctx->d_emflags.p, keep)) return fvi::drained(ctx, rc);
    FV_HIP(hipEventRecord(e1, ctx->stream));
    FV_HIP(hipStreamSynchronize(ctx->stream));
    float ms = 0.0f;
    FV_HIP(hipEventElapsedTime(&ms, e0, e1));
    *ms_out = ms / (float)reps;
    ctx->stats.device_bytes = (long long)fvi::device_bytes(ctx);
    return FV_OK;
}

extern "C" int fv_test_flat_poison(fv_ctx *ctx, int t)
{
    if (!ctx || t < -1) return FV_ERR_ARG;
    FV_NO_STREAM(ctx);
    ctx->flat_poison = t;
    return FV_OK;
}

// one member's option
static int set_option_on(fv_ctx *ctx, int key, long long value)
{
    switch (key) {
    case FV_OPT_KERNEL:
        // (FV_KERNEL_SPARSE_CSR is reported, never chosen)
        if ((value < FV_KERNEL_AUTO || value > FV_KERNEL_U16_REFINE) && value != FV_KERNEL_CSR_F64) return FV_ERR_ARG;
        ctx->opt_kernel = (int)value; return FV_OK;
    case FV_OPT_MAX_BATCH:
        if (value < 1 || value > fvk::MAX_BATCH) return FV_ERR_ARG;
        ctx->opt_max_batch = (int)value; return FV_OK;
    case FV_OPT_PROFILE:
        ctx->opt_profile = value ? 1 : 0; return FV_OK;
    case FV_OPT_FLAT_GENERATIONS:
        if (value < 0 || value > 2) return FV_ERR_ARG;
        ctx->opt_flat = (int)value; return FV_OK;
    case FV_OPT_ROW_CODES:
        if (value < 0 || value > 4) return FV_ERR_ARG;
        ctx->opt_row_codes = (int)value; return FV_OK;
    case FV_OPT_SEL_MARGIN:
        if (value < 0 || value > 100000) return FV_ERR_ARG;
        ctx->opt_sel_margin = (float)value * 1e-3f; return FV_OK;
    case FV_OPT_SPARSE_BEAM:
        if (value != 0 && value != 1) return FV_ERR_ARG;
        ctx->opt_sparse_beam = (int)value; return FV_OK;
    case FV_OPT_DEBUG:
#ifndef FV_TIMING_BUILD
        // bits 0, 4, 5, 11, 12 leave a part of a kernel out (to time the rest) and so change results: they exist in
        // the timing build only (libflashvit_timing.so, tools/).  Every bit this library accepts is speed-only.
        if (value & FV_DEBUG_TIMING_ONLY) { ctx->detail = "FV_OPT_DEBUG: result-changing timing switches need the timing build"; return FV_ERR_ARG; }
#endif
        // (bits 27 and 30 are not assigned; bit 31 is kept apart from the int the kernels see)
        if (value < 0 || value >= (1ll << 32) || (value & ((1ll << 27) | (1ll << 30)))) return FV_ERR_ARG;
        ctx->opt_csr_mem = (int)((value >> 31) & 1);
        ctx->opt_debug = (int)(value & 0x3fffffff); return FV_OK;
    default: return FV_ERR_ARG;
    }
}

extern "C" int fv_set_option(fv_ctx *ctx, int key, long long value)
{
    if (!ctx) return FV_ERR_ARG;
    FV_NO_STREAM(ctx);
    if (ctx->group && ctx->group_rank != 0) return set_option_on(ctx, key, value);
    // the handle of a multi-device context: the same option on every member, itself last
    return fvi::for_each_member(ctx, [&](fv_ctx *ctx) -> int { FV_NO_STREAM(ctx); return set_option_on(ctx, key, value); }, true);
}

extern "C" long long fv_checkpoint_memory_bytes(int K, int T, int step)
{
    if (step <= 0) step = (int)std::floor(std::sqrt(1.0 * T));
    const long long nck = (T + step - 1) / step;
    const long long last = T - (nck - 1) * step;
    const long long tsub = nck > 1 && step + 1 > last ? step + 1 : last;       // T_sub, checkpoint Viterbi.c:123
    return 4LL * K + 4LL * K * nck + 4LL * K + 4LL * (T / step + 1) + 8LL * K * tsub;   // :250
}

extern "C" int fv_last_stats(const fv_ctx *ctx, fv_stats *out)
{
    if (!ctx || !out) return FV_ERR_ARG;
    *out = ctx->stats;
    return FV_OK;
}

extern "C" const char *fv_last_error_detail(const fv_ctx *ctx) { return ctx ? ctx->detail.c_str() : ""; }

extern "C" const char *fv_strerror(int rc)
{
    switch (rc) {
    case FV_OK: return "ok";
    case FV_WARN_BEAM_MISS: return "beam miss: path holds -1 entries, as the reference prints";
    case FV_ERR_ARG: return "bad argument";
    case FV_ERR_NOMEM: return "out of memory";
    case FV_ERR_NO_PRED: return "decoded entry has no finite predecessor";
    case FV_ERR_DEVICE: return "HIP error";
    case FV_ERR_STATE: return "call out of order (no model / no communicator)";
    case FV_ERR_UNSUPPORTED: return "size or option not supported by this build";
    case FV_ERR_COMM: return "RCCL error";
    default: return "unknown flashvit error";
    }
}

extern "C" long long fv_reference_memory_bytes(int K, int T, int n_split, int beam_width)
{
    // sizeof(ThreadPool) on x86-64 glibc: mutex 40 + cond 48 + N pthread_t + 3 ints, padded to 8
    const long long N = n_split;
    const long long pool = ((40 + 48 + 8 * N + 12 + 7) / 8) * 8;
    long long mem = 0, tmp;
    const bool nway = N > 2 && T >= 2 * N;
    if (beam_width <= 0) {
        if (nway) mem = 4 * (N - 1) + 2LL * K * 4 + 2 * (N - 1) * (long long)K * 4;    // FLASH:355
        tmp = N * (2LL * K * 4 + 2LL * K * 4);                                         // :364
    } else {
        if (nway) mem = 4 * (N - 1) + 2 * (N - 1) * (long long)(beam_width + 1) * 12;  // FLASH_BS:564
        tmp = N * (2LL * (beam_width + 1) * 12);                                       // :573
    }
    if (tmp > mem) mem = tmp;
    return mem + pool + 8;     // + sizeof(ThreadPool) + sizeof(size_t) (the sizeof(expr) quirk, FLASH:367)
}
