// fv_stream.hip — fv_stream_*: the online full-state decode (include/flashvit.h).
//
// A push queues its steps as the single-task launches of a one-shot whole-sequence pass (fvi::stream_step), into score
// rows and arg rows the stream owns.  What is new is the part that decides ON THE DEVICE, between those launches, that
// a prefix of the path can no longer change: the ancestor row anc[K] (the state at the anchor time on every state's
// survivor path) is advanced by stream_ancestors every check_every steps, and stream_verdict turns its fold into the
// verdict — one ancestor: record the commit and move the anchor; none: the stream is dead.  The host meets the device
// once per push: it reads the last commit record, runs the existing back-track over the committed range and copies
// the piece out.
#include "fv_internal.h"

#include <climits>

namespace fvk {

// The stream's device words.  acc[p]: the fold of check number q (p = q & 1) over the non-negative anc values —
// minimum, maximum, count — accumulated by stream_ancestors with vector atomics; the verdict launch of check q reads
// acc[q & 1] and clears acc[(q + 1) & 1] for the next check, so no launch reads a word that the same launch writes.
struct StreamCtl {
    long long anchor;                 // a: the time anc refers to
    long long rec_time, rec_state;    // the last commit: every decodable path runs through (rec_time, rec_state); -1: none yet
    long long dead;                   // a check found no state with a predecessor
    long long commits;
    unsigned long long bt_restarts;   // the back-tracks' retry counter (fvk::backtrack)
    unsigned long long emflags[2];    // stage_emissions: flag bits, lowest refused index
    int acc[2][4];
    int sym0;                         // the symbol of time 0 (init row); 0 for a stream of score rows
    float score;                      // the end pick's score (close)
};

constexpr int ANC_BLOCK = 256;

__global__ __launch_bounds__(ANC_BLOCK) void stream_reset(StreamCtl *ctl, int *anc, int K)
{
    const int s = blockIdx.x * ANC_BLOCK + threadIdx.x;
    if (s < K) anc[s] = s;
    if (s == 0) {
        ctl->anchor = 0; ctl->rec_time = -1; ctl->rec_state = -1; ctl->dead = 0; ctl->commits = 0; ctl->bt_restarts = 0ull;
        for (int p = 0; p < 2; ++p) { ctl->acc[p][0] = INT_MAX; ctl->acc[p][1] = -1; ctl->acc[p][2] = 0; ctl->acc[p][3] = 0; }
        ctl->sym0 = 0; ctl->score = 0.0f;
    }
}

// One check, first launch: anc_out[s] = anc_in[ bp_{t-r+1}[ ... bp_t[s] ] ] for the r steps since the check before — r
// dependent gathers down the arg rows (bp_new: the row of the current time t, the row of time t - j lies j * K below it)
// and one into the old ancestor row; -1 (no predecessor) ends a chain.  Lanes along s: the first gather is coalesced,
// the others land wherever the survivor paths lead (after a few steps on a handful of states: the same cache lines).
// Then the fold over all K: wave shuffle, LDS across the four waves, one atomic triple per workgroup that saw a live state.
__global__ __launch_bounds__(ANC_BLOCK) void stream_ancestors(const int *bp_new, int r, int K, const int *anc_in, int *anc_out, int *acc)
{
    __shared__ int s_mn[ANC_BLOCK / 64], s_mx[ANC_BLOCK / 64], s_cnt[ANC_BLOCK / 64];
    const int s = blockIdx.x * ANC_BLOCK + threadIdx.x;
    int v = -1;
    if (s < K) {
        int x = s;
        for (int j = 0; j < r && x >= 0; ++j) x = bp_new[x - (long long)j * K];
        v = x >= 0 ? anc_in[x] : -1;
        anc_out[s] = v;
    }
    int mn = v >= 0 ? v : INT_MAX, mx = v, cnt = v >= 0 ? 1 : 0;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        mn = min(mn, __shfl_xor(mn, m));
        mx = max(mx, __shfl_xor(mx, m));
        cnt += __shfl_xor(cnt, m);
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) { s_mn[w] = mn; s_mx[w] = mx; s_cnt[w] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int q = 1; q < ANC_BLOCK / 64; ++q) { mn = min(mn, s_mn[q]); mx = max(mx, s_mx[q]); cnt += s_cnt[q]; }
        if (cnt) { atomicMin(&acc[0], mn); atomicMax(&acc[1], mx); atomicAdd(&acc[2], cnt); }
    }
}

// One check, second launch (the fold is final: the launch before this one has ended).  One ancestor v: thread 0 notes
// the commit (anchor, v) — in the record the host reads after the push and in the stream's path row, where the
// back-track starts (base: the time of path[0]) — and moves the anchor to the current time t; every workgroup
// re-anchors its states: anc[s] = s where the state has a predecessor (bp_t: the arg row of time t), else -1.  No
// live state: dead, for good (every later fold is empty too).  parity: this check's acc; the other one is cleared
// for the next check, which no workgroup of this launch reads.
__global__ __launch_bounds__(ANC_BLOCK) void stream_verdict(StreamCtl *ctl, int parity, long long t, long long base, const int *bp_t,
                                                            int K, int *anc_out, int *path)
{
    const int mn = ctl->acc[parity][0], mx = ctl->acc[parity][1], cnt = ctl->acc[parity][2];
    const bool one = cnt > 0 && mn == mx;
    const int s = blockIdx.x * ANC_BLOCK + threadIdx.x;
    if (one && s < K) anc_out[s] = bp_t[s] >= 0 ? s : -1;
    if (s == 0) {
        int *next = ctl->acc[parity ^ 1];
        next[0] = INT_MAX; next[1] = -1; next[2] = 0;
        if (cnt == 0) ctl->dead = 1;
        else if (one) {
            const long long a = ctl->anchor;
            path[a - base] = mn;
            ctl->rec_time = a; ctl->rec_state = mn; ctl->anchor = t; ctl->commits += 1;
        }
    }
}

}  // namespace fvk

// check_every: a check costs two launches of a few microseconds; a commit delayed by up to check_every steps costs
// that many arg rows of lag.  DESIGN.md 5.6 has the measurement the default was chosen on.
constexpr int STREAM_CHECK_DEFAULT = 16, STREAM_CHECK_MAX = 64;
constexpr long long STREAM_ROWS_DEFAULT = 256;

struct fv_stream {
    int kernel = FV_KERNEL_AUTO, check_every = STREAM_CHECK_DEFAULT;
    enum { UNSET, SYMBOLS, SCORES } kind = UNSET;
    long long times = 0, committed = 0;       // consumed; returned.  The pending times are committed .. times - 1
    long long since_check = 0, nchecks = 0;
    bool dead = false;
    // arg rows [cap][K] and the path row [cap]: pending time j at slot off + (j - committed) of bp, at j - committed of path
    DevBuf<int> bp, path, anc;
    size_t cap = 0, off = 0;
    DevBuf<float> rows;                       // the two score rows, by parity of the time
    DevBuf<fvk::StreamCtl> ctl;
    fvk::StreamCtl *h_ctl = nullptr;          // pinned
    // a push of score rows: its staged chunk (sized for the largest push seen) and the raw copy of a host block
    DevBuf<float> e32;
    DevBuf<double> e64;
    DevBuf<unsigned char> raw;
    fv_stream_stats st{};
};

namespace {

long long pending(const fv_stream *s) { return s->times - s->committed; }

// Room for `n` more arg rows behind the pending ones.  The live rows are moved to the front when the buffer is at
// least twice the need (the slots in front then hold more than the live rows: one copy, nothing overlaps); else the
// buffer is reallocated at twice the need, at least doubled, and the live rows copied over.  A refused allocation
// leaves everything as it was.
int make_room(fv_ctx *ctx, long long n)
{
    fv_stream *s = ctx->strm;
    const size_t live = (size_t)pending(s), need = live + (size_t)n, K = (size_t)ctx->K;
    if (s->off + need <= s->cap) return 0;
    if (s->cap >= 2 * need) {
        if (live) FV_HIP(hipMemcpyAsync(s->bp.p, s->bp.p + s->off * K, live * K * sizeof(int), hipMemcpyDeviceToDevice, ctx->stream));
        s->off = 0;
        return 0;
    }
    const size_t cap = std::max(2 * s->cap, 2 * need);
    DevBuf<int> bp, path;
    if (bp.ensure(cap * K) != hipSuccess || path.ensure(cap) != hipSuccess) {
        (void)hipGetLastError();
        ctx->detail = "fv_stream_push: " + std::to_string((unsigned long long)cap * (K + 1) * sizeof(int)) + " bytes needed for " +
                      std::to_string(cap) + " arg rows (" + std::to_string(need) + " pending and pushed times)";
        return FV_ERR_NOMEM;
    }
    if (live) FV_HIP(hipMemcpyAsync(bp.p, s->bp.p + s->off * K, live * K * sizeof(int), hipMemcpyDeviceToDevice, ctx->stream));
    FV_HIP(hipStreamSynchronize(ctx->stream));
    std::swap(s->bp.p, bp.p); std::swap(s->bp.n, bp.n);
    std::swap(s->path.p, path.p); std::swap(s->path.n, path.n);
    s->cap = cap; s->off = 0;
    s->st.regrows += 1;
    s->st.arg_rows_capacity = (long long)cap;
    return 0;
}

// The n times of an admitted push: the launches, the one meeting with the device, the piece.
// lb32 / lb64: the emission tables, sym[i]: the row of pushed time i in them (NULL: row i).
int run_push(fv_ctx *ctx, const float *lb32, const double *lb64, const int *sym, int n, int *path_out, long long *committed_out)
{
    fv_stream *s = ctx->strm;
    const size_t K = (size_t)ctx->K;
    fvk::StreamCtl *ctl = s->ctl.p;
    const int nblk = (ctx->K + fvk::ANC_BLOCK - 1) / fvk::ANC_BLOCK;
    auto row = [&](long long j) { return s->rows.p + (size_t)(j & 1) * ctx->nrows; };
    auto arg_row = [&](long long j) { return s->bp.p + (s->off + (size_t)(j - s->committed)) * K; };
    for (int i = 0; i < n; ++i) {
        const long long j = s->times + i;
        const size_t e = (size_t)(sym ? sym[i] : i) * K;
        if (j == 0) {
            s->h_ctl->sym0 = sym ? sym[0] : 0;
            FV_HIP(hipMemcpyAsync(&ctl->sym0, &s->h_ctl->sym0, sizeof(int), hipMemcpyHostToDevice, ctx->stream));
            if (int rc = fvi::stream_init_row(ctx, lb64, &ctl->sym0, row(0))) return rc;
        } else {
            if (int rc = fvi::stream_step(ctx, s->kernel, row(j - 1), row(j), lb32 + e, lb64 + e, arg_row(j), (int)(j & 1))) return rc;
            s->since_check += 1;
        }
        if (s->since_check > 0 && (s->since_check == s->check_every || i == n - 1)) {
            const int q = (int)(s->nchecks & 1);
            int *anc_in = s->anc.p + (size_t)q * K, *anc_out = s->anc.p + (size_t)(q ^ 1) * K;
            hipLaunchKernelGGL(fvk::stream_ancestors, dim3(nblk), dim3(fvk::ANC_BLOCK), 0, ctx->stream, arg_row(j), (int)s->since_check,
                               ctx->K, anc_in, anc_out, ctl->acc[q]);
            hipLaunchKernelGGL(fvk::stream_verdict, dim3(nblk), dim3(fvk::ANC_BLOCK), 0, ctx->stream, ctl, q, j, s->committed,
                               arg_row(j), ctx->K, anc_out, s->path.p);
            FV_HIP(hipGetLastError());
            s->nchecks += 1;
            s->since_check = 0;
        }
    }
    s->times += n;
    s->st.times = s->times; s->st.pushes += 1; s->st.checks = s->nchecks;
    FV_HIP(hipMemcpyAsync(s->h_ctl, ctl, sizeof(fvk::StreamCtl), hipMemcpyDeviceToHost, ctx->stream));
    FV_HIP(hipStreamSynchronize(ctx->stream));
    s->st.commits = s->h_ctl->commits;
    *committed_out = 0;
    if (s->h_ctl->dead) {
        s->dead = true;
        ctx->detail = "fv_stream_push: no state of the current time has a predecessor";
        return FV_ERR_NO_PRED;
    }
    if (s->h_ctl->rec_time >= s->committed) {
        // only the last commit of the push matters: its survivor path runs through the earlier ones
        const long long R = s->h_ctl->rec_time - s->committed, count = R + 1;
        if (R > 0)
            if (int rc = fvi::stream_backtrack(ctx, s->bp.p + s->off * K, (int)R, s->path.p, &ctl->bt_restarts)) return rc;
        FV_HIP(hipMemcpyAsync(path_out, s->path.p, (size_t)count * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        FV_HIP(hipMemcpyAsync(&s->h_ctl->bt_restarts, &ctl->bt_restarts, sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
        FV_HIP(hipStreamSynchronize(ctx->stream));
        s->st.bt_restarts = (long long)s->h_ctl->bt_restarts;
        s->committed += count;
        s->off += (size_t)count;              // the committed rows are dropped: their slots are room again (make_room)
        s->st.committed = s->committed;
        *committed_out = count;
    }
    s->st.lag_max = std::max(s->st.lag_max, pending(s));
    return FV_OK;
}

// what every push checks first
int push_admission(fv_ctx *ctx, const char *who, const void *data, int n, const int *path_out, const long long *committed_out, int kind)
{
    fv_stream *s = ctx->strm;
    if (!s) { ctx->detail = std::string(who) + ": no stream is open (fv_stream_open)"; return FV_ERR_STATE; }
    if (s->dead) { ctx->detail = std::string(who) + ": the stream met a time without predecessors: fv_stream_close or fv_stream_abort"; return FV_ERR_STATE; }
    if (!data || n < 1 || !path_out || !committed_out) { ctx->detail = std::string(who) + ": n >= 1 times and non-NULL pointers"; return FV_ERR_ARG; }
    if (s->kind != fv_stream::UNSET && s->kind != kind) {
        ctx->detail = std::string(who) + ": the stream's first push fixed its input (symbols or score rows)";
        return FV_ERR_ARG;
    }
    if (pending(s) + n > INT_MAX / 2) { ctx->detail = std::string(who) + ": more than 2^30 pending times"; return FV_ERR_ARG; }
    return 0;
}

// a refusal after device work has been queued: nothing of it may still run when the caller returns
int refused(fv_ctx *ctx, int rc)
{
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipGetLastError();
    return rc;
}

void end_stream(fv_ctx *ctx)
{
    ctx->strm_stats = ctx->strm->st;
    fvi::stream_drop(ctx);
}

}  // namespace

void fvi::stream_drop(fv_ctx *ctx)
{
    fv_stream *s = ctx->strm;
    if (!s) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    if (s->h_ctl) (void)hipHostFree(s->h_ctl);
    delete s;                                    // (the device buffers free themselves)
    ctx->strm = nullptr;
}

extern "C" int fv_stream_open(fv_ctx *ctx, long long lag_rows_hint, int check_every)
{
    if (!ctx) return FV_ERR_ARG;
    if (ctx->strm) { ctx->detail = "fv_stream_open: a stream is already open on this context"; return FV_ERR_STATE; }
    if (ctx->group || ctx->comm || ctx->nranks > 1) {
        ctx->detail = "fv_stream_open: one device, no communicator and no partition";
        return FV_ERR_UNSUPPORTED;
    }
    if (ctx->K == 0) { ctx->detail = "fv_stream_open: no model"; return FV_ERR_STATE; }
    if (lag_rows_hint < 0 || lag_rows_hint > INT_MAX / 2 || check_every < 0 || check_every > STREAM_CHECK_MAX) {
        ctx->detail = "fv_stream_open: lag_rows_hint >= 0 and check_every in 0 .. 64";
        return FV_ERR_ARG;
    }
    int kernel = FV_KERNEL_AUTO;
    if (int rc = fvi::stream_admit(ctx, kernel)) return rc;
    fv_stream *s = new (std::nothrow) fv_stream();
    if (!s) return FV_ERR_NOMEM;
    ctx->strm = s;
    const int rc = [&]() -> int {
        const size_t K = (size_t)ctx->K;
        s->kernel = kernel;
        s->check_every = check_every ? check_every : STREAM_CHECK_DEFAULT;
        s->cap = (size_t)std::max(2ll, lag_rows_hint ? lag_rows_hint : STREAM_ROWS_DEFAULT);
        FV_HIP(hipSetDevice(ctx->device));
        FV_HIP(ctx->d_counters.ensure(FV_NCOUNTERS));      // (the step kernels' statistics words, as every decode has them)
        FV_HIP(hipMemsetAsync(ctx->d_counters.p, 0, ctx->d_counters.bytes(), ctx->stream));
        FV_HIP(s->bp.ensure(s->cap * K));
        FV_HIP(s->path.ensure(s->cap));
        FV_HIP(s->anc.ensure(2 * K));
        FV_HIP(s->rows.ensure(2 * (size_t)ctx->nrows));
        FV_HIP(s->ctl.ensure(1));
        FV_HIP(hipHostMalloc(reinterpret_cast<void **>(&s->h_ctl), sizeof(fvk::StreamCtl), hipHostMallocDefault));
        FV_HIP(hipMemsetAsync(s->rows.p, 0, s->rows.bytes(), ctx->stream));       // row pads stay zero
        hipLaunchKernelGGL(fvk::stream_reset, dim3((ctx->K + fvk::ANC_BLOCK - 1) / fvk::ANC_BLOCK), dim3(fvk::ANC_BLOCK), 0, ctx->stream,
                           s->ctl.p, s->anc.p, ctx->K);
        FV_HIP(hipGetLastError());
        FV_HIP(hipStreamSynchronize(ctx->stream));
        return 0;
    }();
    if (rc) { (void)hipGetLastError(); fvi::stream_drop(ctx); return rc; }
    s->st.kernel = kernel;
    s->st.arg_rows_capacity = (long long)s->cap;
    ctx->strm_stats = s->st;
    ctx->strm_any = true;
    return FV_OK;
}

extern "C" int fv_stream_push(fv_ctx *ctx, const int *ob, int n, int *path_out, long long *committed_out)
{
    if (!ctx) return FV_ERR_ARG;
    if (int rc = push_admission(ctx, "fv_stream_push", ob, n, path_out, committed_out, fv_stream::SYMBOLS)) return rc;
    for (int i = 0; i < n; ++i)
        if (ob[i] < 0 || ob[i] >= ctx->M) {
            ctx->detail = "fv_stream_push: ob[" + std::to_string(i) + "] = " + std::to_string(ob[i]) + " lies outside [0, M = " + std::to_string(ctx->M) + ")";
            return FV_ERR_ARG;
        }
    auto t0 = clk::now();
    FV_HIP(hipSetDevice(ctx->device));
    if (int rc = make_room(ctx, n)) return refused(ctx, rc);
    ctx->strm->kind = fv_stream::SYMBOLS;
    const int rc = run_push(ctx, ctx->LB32T.p, ctx->LB64T.p, ob, n, path_out, committed_out);
    ctx->strm->st.push_ms_total += ms_since(t0);
    return rc < 0 ? refused(ctx, rc) : rc;
}

extern "C" int fv_stream_push_emissions(fv_ctx *ctx, const void *scores, int dtype, int n, long long ld, int *path_out,
                                        long long *committed_out)
{
    const char *who = "fv_stream_push_emissions";
    if (!ctx) return FV_ERR_ARG;
    if (int rc = push_admission(ctx, who, scores, n, path_out, committed_out, fv_stream::SCORES)) return rc;
    fv_stream *s = ctx->strm;
    const fvi::EmisBlock b{ scores, dtype, n, ld };
    if (!fvi::emis_block_ok(ctx, b)) {
        ctx->detail = std::string(who) + ": ld >= K (ld >= P while an emission map is set) and dtype FV_EMIS_LOG_F32, _F64, _F16 or _BF16";
        return FV_ERR_ARG;
    }
    auto t0 = clk::now();
    FV_HIP(hipSetDevice(ctx->device));
    if (int rc = make_room(ctx, n)) return refused(ctx, rc);
    // the chunk tables and, for a block the kernel cannot read where it lies, its raw copy: as fv_set_emissions
    const fvi::PointerPlace at = fvi::pointer_place(scores);
    const bool in_place = at.on_device && at.device == ctx->device;
    const size_t cells = (size_t)n * (size_t)ctx->K, raw_bytes = in_place ? 0 : fvi::emis_raw_bytes(ctx, b);
    if (s->e32.ensure(cells) != hipSuccess || s->e64.ensure(cells) != hipSuccess || s->raw.ensure(raw_bytes) != hipSuccess) {
        (void)hipGetLastError();
        ctx->detail = std::string(who) + ": " + std::to_string(12ull * cells + raw_bytes) + " bytes needed for the staged chunk";
        return refused(ctx, FV_ERR_NOMEM);
    }
    // the value rules decide whether the push is taken at all: the chunk is staged and its flags are read before any step
    auto reset = [&]() -> int {
        s->h_ctl->emflags[0] = 0ull; s->h_ctl->emflags[1] = ~0ull;
        FV_HIP(hipMemcpyAsync(s->ctl.p->emflags, s->h_ctl->emflags, sizeof s->h_ctl->emflags, hipMemcpyHostToDevice, ctx->stream));
        return 0;
    };
    if (int rc = fvi::stage_block(ctx, b, in_place ? nullptr : s->raw.p, s->e32.p, s->e64.p, s->ctl.p->emflags, reset)) return refused(ctx, rc);
    FV_HIP(hipMemcpyAsync(s->h_ctl->emflags, s->ctl.p->emflags, sizeof s->h_ctl->emflags, hipMemcpyDeviceToHost, ctx->stream));
    FV_HIP(hipStreamSynchronize(ctx->stream));
    const unsigned long long flags = s->h_ctl->emflags[0], where = s->h_ctl->emflags[1];
    if (flags & fvi::FV_EMIS_BAD) return fvi::emis_refusal(ctx, who, where, s->times);
    if ((flags & fvi::FV_EMIS_POSITIVE) && s->kernel != FV_KERNEL_F64_STREAM && s->kernel != FV_KERNEL_CSR_F64) {
        ctx->detail = fvi::filter_range_detail(ctx);
        return FV_ERR_UNSUPPORTED;
    }
    s->kind = fv_stream::SCORES;
    const int rc = run_push(ctx, s->e32.p, s->e64.p, nullptr, n, path_out, committed_out);
    s->st.push_ms_total += ms_since(t0);
    return rc < 0 ? refused(ctx, rc) : rc;
}

extern "C" long long fv_stream_pending(const fv_ctx *ctx)
{
    return ctx && ctx->strm ? pending(ctx->strm) : -1;
}

extern "C" int fv_stream_close(fv_ctx *ctx, int *path_out, long long *n_out, float *score_out)
{
    if (!ctx) return FV_ERR_ARG;
    fv_stream *s = ctx->strm;
    if (!s) { ctx->detail = "fv_stream_close: no stream is open"; return FV_ERR_STATE; }
    if (!path_out || !n_out) { ctx->detail = "fv_stream_close: path_out and n_out"; return FV_ERR_ARG; }
    *n_out = 0;
    int rc = FV_OK;
    if (s->dead) {
        ctx->detail = "fv_stream_close: the stream met a time without predecessors";
        rc = FV_ERR_NO_PRED;
    } else if (s->times > 0) {
        rc = [&]() -> int {
            const long long np = pending(s);
            FV_HIP(hipSetDevice(ctx->device));
            const float *last = s->rows.p + (size_t)((s->times - 1) & 1) * ctx->nrows;
            if (int r = fvi::stream_end_pick(ctx, last, s->path.p + (np - 1), &s->ctl.p->score)) return r;
            if (np > 1)
                if (int r = fvi::stream_backtrack(ctx, s->bp.p + s->off * (size_t)ctx->K, (int)(np - 1), s->path.p, &s->ctl.p->bt_restarts)) return r;
            FV_HIP(hipMemcpyAsync(path_out, s->path.p, (size_t)np * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
            FV_HIP(hipMemcpyAsync(s->h_ctl, s->ctl.p, sizeof(fvk::StreamCtl), hipMemcpyDeviceToHost, ctx->stream));
            FV_HIP(hipStreamSynchronize(ctx->stream));
            s->st.bt_restarts = (long long)s->h_ctl->bt_restarts;
            if (score_out) *score_out = s->h_ctl->score;
            *n_out = np;
            s->committed += np;
            s->st.committed = s->committed;
            for (long long j = 0; j < np; ++j) if (path_out[j] < 0) return FV_ERR_NO_PRED;
            return FV_OK;
        }();
        if (rc < 0 && rc != FV_ERR_NO_PRED) rc = refused(ctx, rc);
    }
    end_stream(ctx);
    return rc;
}

extern "C" int fv_stream_abort(fv_ctx *ctx)
{
    if (!ctx) return FV_ERR_ARG;
    if (!ctx->strm) { ctx->detail = "fv_stream_abort: no stream is open"; return FV_ERR_STATE; }
    end_stream(ctx);
    return FV_OK;
}

extern "C" int fv_stream_last_stats(const fv_ctx *ctx, fv_stream_stats *out)
{
    if (!ctx || !out) return FV_ERR_ARG;
    if (!ctx->strm_any) return FV_ERR_STATE;
    *out = ctx->strm ? ctx->strm->st : ctx->strm_stats;
    return FV_OK;
}
