// fv_stream.hip — fv_stream_* and fv_streams_*: the online full-state decode (include/flashvit.h).
//
// A push queues its steps as the single-task launches of a one-shot whole-sequence pass (fvi::stream_step), into score
// rows and arg rows the stream owns.  What is new is the part that decides ON THE DEVICE, between those launches, that
// a prefix of the path can no longer change: the ancestor row anc[K] (the state at the anchor time on every state's
// survivor path) is advanced by stream_ancestors every check_every steps, and stream_verdict turns its fold into the
// verdict — one ancestor: record the commit and move the anchor; none: the stream is dead.  The host meets the device
// once per push: it reads the last commit record, runs the existing back-track over the committed range and copies
// the piece out.
//
// A set (fv_streams_*) is nslots of that per-sequence state on one context.  The slots named in one push call advance in
// lock-step: their steps share step launches of up to batch_cap tasks (fvi::stream_step_batch), the checks that come
// due in one lock-step share one pair of launches (stream_ancestors_set / stream_verdict_set, a slot per blockIdx.y),
// and the host meets the device twice per call whatever the number of slots.
//
// fv_set_max_lag bounds the commit lag of the streams and sets opened after it: their check is three
// launches (stream_ancestors_lag / stream_decide / stream_apply), and a check that finds more than one ancestor max_lag
// or more steps past the anchor FORCES the commit of the best state's ancestor and prunes the other states.  Without it
// every stream runs the two launches above with the arguments they always had.
#include "fv_internal.h"

#include <climits>
#include <memory>

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
    int sym0;                         // the symbol of time 0 (init row); a stream of score rows: its row in the staged chunk
    float score;                      // the end pick's score (close)
    // a lag-bounded stream (fv_set_max_lag; the words below stay as stream_reset left them in every other stream).
    // best[p]: the arg-max key of the score row at check number q (p = q & 1), double-buffered like acc; decision, vstar:
    // what stream_decide made of acc[p], best[p] and the anchor, read by the apply launch; then the forced commits' counters
    unsigned long long best[2];
    int decision, vstar;
    long long forced, first_forced, last_forced;
    unsigned long long pruned;
};

constexpr int ANC_BLOCK = 256;

// stream_decide's verdicts
enum { DECIDE_NONE = 0, DECIDE_ONE = 1, DECIDE_DEAD = 2, DECIDE_FORCED = 3 };

// The arg-max key of score x at state s: the order-preserving image of the float's bits in the high half, 0x7fffffff - s
// in the low half, so that the maximum over a row carries the LOWEST index among equal scores (the end-pick rule of
// fv_stream_close).  Every key is above 0, the fold's neutral element: -inf maps to 0x007fffff in the high half.  (x + 0.0f:
// a negative zero compares equal to a positive one and must not lose to it on its bits.)
__device__ __forceinline__ unsigned long long best_key(float x, int s)
{
    const unsigned int u = __float_as_uint(x + 0.0f);
    const unsigned int image = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)image << 32) | (unsigned int)(0x7fffffff - s);
}

__global__ __launch_bounds__(ANC_BLOCK) void stream_reset(StreamCtl *ctl, int *anc, int K)
{
    const int s = blockIdx.x * ANC_BLOCK + threadIdx.x;
    if (s < K) anc[s] = s;
    if (s == 0) {
        ctl->anchor = 0; ctl->rec_time = -1; ctl->rec_state = -1; ctl->dead = 0; ctl->commits = 0; ctl->bt_restarts = 0ull;
        for (int p = 0; p < 2; ++p) { ctl->acc[p][0] = INT_MAX; ctl->acc[p][1] = -1; ctl->acc[p][2] = 0; ctl->acc[p][3] = 0; }
        ctl->sym0 = 0; ctl->score = 0.0f;
        ctl->best[0] = ctl->best[1] = 0ull; ctl->decision = DECIDE_NONE; ctl->vstar = -1;
        ctl->forced = 0; ctl->first_forced = ctl->last_forced = -1; ctl->pruned = 0ull;
    }
}

// One check, first launch: anc_out[s] = anc_in[ bp_{t-r+1}[ ... bp_t[s] ] ] for the r steps since the check before — r
// dependent gathers down the arg rows (bp_new: the row of the current time t, the row of time t - j lies j * K below it)
// and one into the old ancestor row; -1 (no predecessor) ends a chain.  Lanes along s: the first gather is coalesced,
// the others land wherever the survivor paths lead (after a few steps on a handful of states: the same cache lines).
// Then the fold over all K: wave shuffle, LDS across the four waves, one atomic triple per workgroup that saw a live state.
// LAG (a lag-bounded stream): the same launch folds the score row of time t into best, the arg-max key of the check's parity
// (best_key: the lowest index among the maxima) — wave shuffle, LDS, one 64-bit vector atomicMax per workgroup.  Rows past
// K take no part.
template <bool LAG>
__device__ __forceinline__ void ancestors_body(const int *bp_new, int r, int K, const int *anc_in, int *anc_out, int *acc,
                                               const float *row, unsigned long long *best)
{
    __shared__ int s_mn[ANC_BLOCK / 64], s_mx[ANC_BLOCK / 64], s_cnt[ANC_BLOCK / 64];
    __shared__ unsigned long long s_key[LAG ? ANC_BLOCK / 64 : 1];
    const int s = blockIdx.x * ANC_BLOCK + threadIdx.x;
    int v = -1;
    unsigned long long key = 0ull;
    if (s < K) {
        int x = s;
        for (int j = 0; j < r && x >= 0; ++j) x = bp_new[x - (long long)j * K];
        v = x >= 0 ? anc_in[x] : -1;
        anc_out[s] = v;
        if constexpr (LAG) key = best_key(row[s], s);
    }
    int mn = v >= 0 ? v : INT_MAX, mx = v, cnt = v >= 0 ? 1 : 0;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        mn = min(mn, __shfl_xor(mn, m));
        mx = max(mx, __shfl_xor(mx, m));
        cnt += __shfl_xor(cnt, m);
        if constexpr (LAG) key = max(key, (unsigned long long)__shfl_xor((long long)key, m));
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) {
        s_mn[w] = mn; s_mx[w] = mx; s_cnt[w] = cnt;
        if constexpr (LAG) s_key[w] = key;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int q = 1; q < ANC_BLOCK / 64; ++q) {
            mn = min(mn, s_mn[q]); mx = max(mx, s_mx[q]); cnt += s_cnt[q];
            if constexpr (LAG) key = max(key, s_key[q]);
        }
        if (cnt) { atomicMin(&acc[0], mn); atomicMax(&acc[1], mx); atomicAdd(&acc[2], cnt); }
        if constexpr (LAG) atomicMax(best, key);
    }
}

__global__ __launch_bounds__(ANC_BLOCK) void stream_ancestors(const int *bp_new, int r, int K, const int *anc_in, int *anc_out, int *acc)
{
    ancestors_body<false>(bp_new, r, K, anc_in, anc_out, acc, nullptr, nullptr);
}

__global__ __launch_bounds__(ANC_BLOCK) void stream_ancestors_lag(const int *bp_new, int r, int K, const int *anc_in, int *anc_out, int *acc,
                                                                  const float *row, unsigned long long *best)
{
    ancestors_body<true>(bp_new, r, K, anc_in, anc_out, acc, row, best);
}

// One check, second launch (the fold is final: the launch before this one has ended).  One ancestor v: thread 0 notes
// the commit (anchor, v) — in the record the host reads after the push and in the stream's path row, where the
// back-track starts (base: the time of path[0]) — and moves the anchor to the current time t; every workgroup
// re-anchors its states: anc[s] = s where the state has a predecessor (bp_t: the arg row of time t), else -1.  No
// live state: dead, for good (every later fold is empty too).  parity: this check's acc; the other one is cleared
// for the next check, which no workgroup of this launch reads.
__device__ __forceinline__ void verdict_body(StreamCtl *ctl, int parity, long long t, long long base, const int *bp_t, int K,
                                             int *anc_out, int *path)
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

__global__ __launch_bounds__(ANC_BLOCK) void stream_verdict(StreamCtl *ctl, int parity, long long t, long long base, const int *bp_t,
                                                            int K, int *anc_out, int *path)
{
    verdict_body(ctl, parity, t, base, bp_t, K, anc_out, path);
}

// The checks of a set that come due in one lock-step, one slot per blockIdx.y: the two launches above over up to
// CHECK_SLOTS descriptors passed by value (scalar loads from the kernel arguments, indexed by a workgroup-uniform
// value).  r differs from slot to slot: the gather loop's trip count is uniform per workgroup, not per grid.  Every
// slot folds into its own StreamCtl::acc[parity], so the rule of the single stream holds slot by slot: no workgroup
// reads a word that another workgroup of the same launch writes.
constexpr int CHECK_SLOTS = 8;
struct CheckSlot {
    const int *bp_new; int r; const int *anc_in; int *anc_out; StreamCtl *ctl; int parity; long long t, base;
    const int *bp_t; int *path;
};
struct CheckArgs { int n, K; CheckSlot s[CHECK_SLOTS]; };

__global__ __launch_bounds__(ANC_BLOCK) void stream_ancestors_set(const CheckArgs a)
{
    if ((int)blockIdx.y >= a.n) return;
    const CheckSlot &c = a.s[blockIdx.y];
    ancestors_body<false>(c.bp_new, c.r, a.K, c.anc_in, c.anc_out, c.ctl->acc[c.parity], nullptr, nullptr);
}

__global__ __launch_bounds__(ANC_BLOCK) void stream_verdict_set(const CheckArgs a)
{
    if ((int)blockIdx.y >= a.n) return;
    const CheckSlot &c = a.s[blockIdx.y];
    verdict_body(c.ctl, c.parity, c.t, c.base, c.bp_t, a.K, c.anc_out, c.path);
}

// ---- the check of a lag-bounded stream (fv_set_max_lag): three launches.  stream_ancestors_lag above;
// stream_decide, one thread, turns the fold into the decision word; stream_apply is the verdict launch driven by that word.
// The decision has a launch of its own because the apply launch moves the anchor and overwrites anc_out in place: it
// cannot read either of them to decide, and no launch reads a word that the same launch writes.
//
// decide: none alive: dead.  One ancestor: the commit of every stream.  More than one and t - anchor >= max_lag: FORCED —
// s* = the lowest index among the maxima of the score row of time t (best), v* = anc_out[s*].  More than one ancestor
// means a state with a predecessor chain back to the anchor, so the maximum is such a state's and v* >= 0; a row that says
// otherwise (scores the step kernels cannot produce) forces nothing.
__device__ __forceinline__ void decide_body(StreamCtl *ctl, int parity, long long t, long long max_lag, const int *anc_out, int K)
{
    const int mn = ctl->acc[parity][0], mx = ctl->acc[parity][1], cnt = ctl->acc[parity][2];
    int decision = DECIDE_NONE, v = -1;
    if (cnt == 0) decision = DECIDE_DEAD;
    else if (mn == mx) { decision = DECIDE_ONE; v = mn; }
    else if (t - ctl->anchor >= max_lag) {
        const unsigned int best = 0x7fffffffu - (unsigned int)(ctl->best[parity] & 0xffffffffull);
        if (best < (unsigned int)K) v = anc_out[best];       // (every fold of K >= 1 states holds a key of one of them)
        if (v >= 0) decision = DECIDE_FORCED;
    }
    ctl->decision = decision; ctl->vstar = v;
}

__global__ void stream_decide(StreamCtl *ctl, int parity, long long t, long long max_lag, const int *anc_out, int K)
{
    if (threadIdx.x == 0) decide_body(ctl, parity, t, max_lag, anc_out, K);
}

// apply.  ONE: verdict_body's commit and re-anchoring.  FORCED: every state whose ancestor is not v* is pruned — its entry
// of the score row of time t becomes -inf, which no later cell can take as its source (its arg entry of time t stays and
// is never read again) — the survivors are re-anchored (anc[s] = s; they have a predecessor: their ancestor is v* >= 0),
// the pruned states with an ancestor are counted (one vector atomic per workgroup that pruned one), and thread 0 records
// (anchor, v*) exactly like any commit, with the forced counters and times.  Each thread reads and writes its own anc_out
// entry only; thread 0 alone reads and moves the anchor; pruned is read by no launch.
// The row belongs to the stream (StreamSeq::rows), outside the context's d_rows: FV_OPT_ROW_CODES never attaches codes to
// it (coded_row_index), and it must stay that way — codes a step wrote beside a row that is pruned afterwards would be wrong.
__device__ __forceinline__ void apply_body(StreamCtl *ctl, int parity, long long t, long long base, const int *bp_t, int K,
                                           int *anc_out, int *path, float *row)
{
    __shared__ int s_cnt[ANC_BLOCK / 64];
    const int decision = ctl->decision, v = ctl->vstar;
    const int s = blockIdx.x * ANC_BLOCK + threadIdx.x;
    if (decision == DECIDE_ONE) {
        if (s < K) anc_out[s] = bp_t[s] >= 0 ? s : -1;
    } else if (decision == DECIDE_FORCED) {              // (uniform over the launch: every thread meets the barrier)
        int cnt = 0;
        if (s < K) {
            const int a = anc_out[s];
            if (a != v) { row[s] = -INFINITY; cnt = a >= 0 ? 1 : 0; }
            anc_out[s] = a == v ? s : -1;
        }
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) cnt += __shfl_xor(cnt, m);
        if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = cnt;
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int q = 1; q < ANC_BLOCK / 64; ++q) cnt += s_cnt[q];
            if (cnt) atomicAdd(&ctl->pruned, (unsigned long long)cnt);
        }
    }
    if (s == 0) {
        int *next = ctl->acc[parity ^ 1];
        next[0] = INT_MAX; next[1] = -1; next[2] = 0;
        ctl->best[parity ^ 1] = 0ull;
        if (decision == DECIDE_DEAD) ctl->dead = 1;
        else if (decision != DECIDE_NONE) {
            const long long a = ctl->anchor;
            path[a - base] = v;
            ctl->rec_time = a; ctl->rec_state = v; ctl->anchor = t; ctl->commits += 1;
            if (decision == DECIDE_FORCED) {
                ctl->forced += 1;
                if (ctl->first_forced < 0) ctl->first_forced = t;
                ctl->last_forced = t;
            }
        }
    }
}

__global__ __launch_bounds__(ANC_BLOCK) void stream_apply(StreamCtl *ctl, int parity, long long t, long long base, const int *bp_t,
                                                          int K, int *anc_out, int *path, float *row)
{
    apply_body(ctl, parity, t, base, bp_t, K, anc_out, path, row);
}

// The set forms, a slot per blockIdx.y as above.  What a lag-bounded slot's check needs besides its CheckSlot lies beside
// it, not in it: the arguments of the two launches of an unbounded set stay as they are.
struct LagSlot { float *row; long long max_lag; };
struct LagArgs { CheckArgs a; LagSlot l[CHECK_SLOTS]; };

__global__ __launch_bounds__(ANC_BLOCK) void stream_ancestors_lag_set(const LagArgs g)
{
    if ((int)blockIdx.y >= g.a.n) return;
    const CheckSlot &c = g.a.s[blockIdx.y];
    ancestors_body<true>(c.bp_new, c.r, g.a.K, c.anc_in, c.anc_out, c.ctl->acc[c.parity], g.l[blockIdx.y].row, &c.ctl->best[c.parity]);
}

__global__ void stream_decide_set(const LagArgs g)
{
    if ((int)blockIdx.y >= g.a.n || threadIdx.x != 0) return;
    const CheckSlot &c = g.a.s[blockIdx.y];
    decide_body(c.ctl, c.parity, c.t, g.l[blockIdx.y].max_lag, c.anc_out, g.a.K);
}

__global__ __launch_bounds__(ANC_BLOCK) void stream_apply_set(const LagArgs g)
{
    if ((int)blockIdx.y >= g.a.n) return;
    const CheckSlot &c = g.a.s[blockIdx.y];
    apply_body(c.ctl, c.parity, c.t, c.base, c.bp_t, g.a.K, c.anc_out, c.path, g.l[blockIdx.y].row);
}

}  // namespace fvk

// check_every: a check costs two launches of a few microseconds; a commit delayed by up to check_every steps costs
// that many arg rows of lag.  DESIGN.md 5.6 has the measurement the default was chosen on.
constexpr int STREAM_CHECK_DEFAULT = 16, STREAM_CHECK_MAX = 64;
constexpr long long STREAM_ROWS_DEFAULT = 256;

// One sequence being decoded online: what the single stream is, and what every slot of a set is.
struct StreamSeq {
    enum { UNSET, SYMBOLS, SCORES } kind = UNSET;
    long long times = 0, committed = 0;       // consumed; returned.  The pending times are committed .. times - 1
    long long since_check = 0, nchecks = 0;
    bool dead = false;
    // arg rows [cap][K] and the path row [cap]: pending time j at slot off + (j - committed) of bp, at j - committed of path
    DevBuf<int> bp, path, anc;
    size_t cap = 0, off = 0;
    DevBuf<float> rows;                       // the two score rows, by parity of the time
    fvk::StreamCtl *d_ctl = nullptr, *h_ctl = nullptr;      // its device words and their pinned mirror (the owner's)
    fv_stream_stats st{};
    long long max_lag = 0;                    // fv_set_max_lag's value at the open; 0: unbounded, two launches per check
    fv_lag_stats lag{};
};

struct fv_stream : StreamSeq {
    int kernel = FV_KERNEL_AUTO, check_every = STREAM_CHECK_DEFAULT;
    DevBuf<fvk::StreamCtl> ctl;
    // a push of score rows: its staged chunk (sized for the largest push seen) and the raw copy of a host block
    DevBuf<float> e32;
    DevBuf<double> e64;
    DevBuf<unsigned char> raw;
};

struct fv_streams {
    int nslots = 0, kernel = FV_KERNEL_AUTO, check_every = STREAM_CHECK_DEFAULT, batch_cap = 1;
    long long max_lag = 0;                    // every slot's
    std::unique_ptr<StreamSeq[]> slot;
    DevBuf<fvk::StreamCtl> ctl;               // [nslots]
    fvk::StreamCtl *h_ctl = nullptr;          // [nslots], pinned
    // a call of score rows: the staged block of all its slots (sized for the largest call seen), the raw copy of a host block
    DevBuf<float> e32;
    DevBuf<double> e64;
    DevBuf<unsigned char> raw;
    fv_streams_stats st{};
};

namespace {

long long pending(const StreamSeq *s) { return s->times - s->committed; }

// Room for `n` more arg rows behind the pending ones.  The live rows are moved to the front when the buffer is at
// least twice the need (the slots in front then hold more than the live rows: one copy, nothing overlaps); else the
// buffer is reallocated at twice the need, at least doubled, and the live rows copied over.  A refused allocation
// leaves everything as it was.  *syncs: the meeting with the device a regrow costs is counted there.
int make_room(fv_ctx *ctx, StreamSeq *s, long long n, const std::string &who, long long *syncs = nullptr)
{
    const size_t live = (size_t)pending(s), need = live + (size_t)n, K = (size_t)ctx->K;
    if (s->off + need <= s->cap) return 0;
    if (s->cap >= 2 * need) {
        if (live) FV_HIP(hipMemcpyAsync(s->bp.p, s->bp.p + s->off * K, live * K * sizeof(int), hipMemcpyDeviceToDevice, ctx->stream));
        s->off = 0;
        return 0;
    }
    // (a lag-bounded sequence's need is bounded — pending <= 2 L + C - 2 — so doubling has nothing to amortise: its buffer
    // stays within twice the largest need, and is regrown only while that need still rises)
    const size_t cap = s->max_lag > 0 ? 2 * need : std::max(2 * s->cap, 2 * need);
    DevBuf<int> bp, path;
    if (bp.ensure(cap * K) != hipSuccess || path.ensure(cap) != hipSuccess) {
        (void)hipGetLastError();
        ctx->detail = who + ": " + std::to_string((unsigned long long)cap * (K + 1) * sizeof(int)) + " bytes needed for " +
                      std::to_string(cap) + " arg rows (" + std::to_string(need) + " pending and pushed times)";
        return FV_ERR_NOMEM;
    }
    if (live) FV_HIP(hipMemcpyAsync(bp.p, s->bp.p + s->off * K, live * K * sizeof(int), hipMemcpyDeviceToDevice, ctx->stream));
    FV_HIP(hipStreamSynchronize(ctx->stream));
    if (syncs) *syncs += 1;
    std::swap(s->bp.p, bp.p); std::swap(s->bp.n, bp.n);
    std::swap(s->path.p, path.p); std::swap(s->path.n, path.n);
    s->cap = cap; s->off = 0;
    s->st.regrows += 1;
    s->st.arg_rows_capacity = (long long)cap;
    return 0;
}

// The commit bookkeeping of a push, once the sequence's control record is on the host (s->h_ctl).  commit_queue: the
// back-track over the range the last commit of the push settles (its survivor path runs through the earlier ones), the
// copy of the piece and of the retry counter, all queued; count: the times they commit, 0: the record has not moved.
int commit_queue(fv_ctx *ctx, StreamSeq *s, int *path_out, long long &count)
{
    count = 0;
    if (s->h_ctl->rec_time < s->committed) return 0;
    const long long R = s->h_ctl->rec_time - s->committed;
    if (R > 0)
        if (int rc = fvi::stream_backtrack(ctx, s->bp.p + s->off * (size_t)ctx->K, (int)R, s->path.p, &s->d_ctl->bt_restarts)) return rc;
    FV_HIP(hipMemcpyAsync(path_out, s->path.p, (size_t)(R + 1) * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    FV_HIP(hipMemcpyAsync(&s->h_ctl->bt_restarts, &s->d_ctl->bt_restarts, sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    count = R + 1;
    return 0;
}

// ... and, after the synchronisation that covers those copies, the counters
void commit_take(StreamSeq *s, long long count)
{
    if (count) {
        s->st.bt_restarts = (long long)s->h_ctl->bt_restarts;
        s->committed += count;
        s->off += (size_t)count;              // the committed rows are dropped: their slots are room again (make_room)
        s->st.committed = s->committed;
    }
    s->st.lag_max = std::max(s->st.lag_max, pending(s));
}

// the forced commits' counters of a sequence whose control record is on the host
void lag_take(StreamSeq *s)
{
    s->lag.forced_commits = s->h_ctl->forced;
    s->lag.pruned_states = (long long)s->h_ctl->pruned;
    s->lag.first_forced_time = s->h_ctl->first_forced;
    s->lag.last_forced_time = s->h_ctl->last_forced;
}

fv_lag_stats lag_fresh(long long max_lag)
{
    fv_lag_stats l{};
    l.max_lag = max_lag; l.first_forced_time = l.last_forced_time = -1;
    return l;
}

// The end of a sequence's input: end pick, back-track of everything pending, the score (fv_stream_close; a slot's close)
int close_seq(fv_ctx *ctx, StreamSeq *s, int *path_out, long long *n_out, float *score_out)
{
    const long long np = pending(s);
    FV_HIP(hipSetDevice(ctx->device));
    const float *last = s->rows.p + (size_t)((s->times - 1) & 1) * ctx->nrows;
    if (int r = fvi::stream_end_pick(ctx, last, s->path.p + (np - 1), &s->d_ctl->score)) return r;
    if (np > 1)
        if (int r = fvi::stream_backtrack(ctx, s->bp.p + s->off * (size_t)ctx->K, (int)(np - 1), s->path.p, &s->d_ctl->bt_restarts)) return r;
    FV_HIP(hipMemcpyAsync(path_out, s->path.p, (size_t)np * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    FV_HIP(hipMemcpyAsync(s->h_ctl, s->d_ctl, sizeof(fvk::StreamCtl), hipMemcpyDeviceToHost, ctx->stream));
    FV_HIP(hipStreamSynchronize(ctx->stream));
    s->st.bt_restarts = (long long)s->h_ctl->bt_restarts;
    if (score_out) *score_out = s->h_ctl->score;
    *n_out = np;
    s->committed += np;
    s->st.committed = s->committed;
    for (long long j = 0; j < np; ++j) if (path_out[j] < 0) return FV_ERR_NO_PRED;
    return FV_OK;
}

// the buffers of one sequence (cap arg rows at first) and its device words set for time 0; queued, not awaited
int seq_alloc(fv_ctx *ctx, StreamSeq *s, size_t cap)
{
    const size_t K = (size_t)ctx->K;
    s->cap = cap;
    FV_HIP(s->bp.ensure(s->cap * K));
    FV_HIP(s->path.ensure(s->cap));
    FV_HIP(s->anc.ensure(2 * K));
    FV_HIP(s->rows.ensure(2 * (size_t)ctx->nrows));
    FV_HIP(hipMemsetAsync(s->rows.p, 0, s->rows.bytes(), ctx->stream));       // row pads stay zero
    return 0;
}

int seq_reset(fv_ctx *ctx, StreamSeq *s)
{
    hipLaunchKernelGGL(fvk::stream_reset, dim3((ctx->K + fvk::ANC_BLOCK - 1) / fvk::ANC_BLOCK), dim3(fvk::ANC_BLOCK), 0, ctx->stream,
                       s->d_ctl, s->anc.p, ctx->K);
    FV_HIP(hipGetLastError());
    return 0;
}

// The n times of an admitted push: the launches, the one meeting with the device, the piece.
// lb32 / lb64: the emission tables, sym[i]: the row of pushed time i in them (NULL: row i).
int run_push(fv_ctx *ctx, const float *lb32, const double *lb64, const int *sym, int n, int *path_out, long long *committed_out)
{
    fv_stream *s = ctx->strm;
    const size_t K = (size_t)ctx->K;
    fvk::StreamCtl *ctl = s->d_ctl;
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
            if (s->max_lag > 0) {
                hipLaunchKernelGGL(fvk::stream_ancestors_lag, dim3(nblk), dim3(fvk::ANC_BLOCK), 0, ctx->stream, arg_row(j),
                                   (int)s->since_check, ctx->K, anc_in, anc_out, ctl->acc[q], row(j), &ctl->best[q]);
                hipLaunchKernelGGL(fvk::stream_decide, dim3(1), dim3(64), 0, ctx->stream, ctl, q, j, s->max_lag, anc_out, ctx->K);
                hipLaunchKernelGGL(fvk::stream_apply, dim3(nblk), dim3(fvk::ANC_BLOCK), 0, ctx->stream, ctl, q, j, s->committed,
                                   arg_row(j), ctx->K, anc_out, s->path.p, row(j));
            } else {
                hipLaunchKernelGGL(fvk::stream_ancestors, dim3(nblk), dim3(fvk::ANC_BLOCK), 0, ctx->stream, arg_row(j), (int)s->since_check,
                                   ctx->K, anc_in, anc_out, ctl->acc[q]);
                hipLaunchKernelGGL(fvk::stream_verdict, dim3(nblk), dim3(fvk::ANC_BLOCK), 0, ctx->stream, ctl, q, j, s->committed,
                                   arg_row(j), ctx->K, anc_out, s->path.p);
            }
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
    lag_take(s);
    *committed_out = 0;
    if (s->h_ctl->dead) {
        s->dead = true;
        ctx->detail = "fv_stream_push: no state of the current time has a predecessor";
        return FV_ERR_NO_PRED;
    }
    long long count = 0;
    if (int rc = commit_queue(ctx, s, path_out, count)) return rc;
    if (count) FV_HIP(hipStreamSynchronize(ctx->stream));
    commit_take(s, count);
    *committed_out = count;
    return FV_OK;
}

// what every push checks first
int push_admission(fv_ctx *ctx, const char *who, const void *data, int n, const int *path_out, const long long *committed_out, int kind)
{
    fv_stream *s = ctx->strm;
    if (!s) { ctx->detail = std::string(who) + ": no stream is open (fv_stream_open)"; return FV_ERR_STATE; }
    if (s->dead) { ctx->detail = std::string(who) + ": the stream met a time without predecessors: fv_stream_close or fv_stream_abort"; return FV_ERR_STATE; }
    if (!data || n < 1 || !path_out || !committed_out) { ctx->detail = std::string(who) + ": n >= 1 times and non-NULL pointers"; return FV_ERR_ARG; }
    if (s->kind != StreamSeq::UNSET && s->kind != kind) {
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
    ctx->strm_lag = ctx->strm->lag;
    fvi::stream_drop(ctx);
}

void drop_set(fv_ctx *ctx)
{
    fv_streams *g = ctx->set;
    if (!g) return;
    ctx->set_stats = g->st;
    ctx->set_lag.clear();
    for (int id = 0; g->slot && id < g->nslots; ++id) ctx->set_lag.push_back(g->slot[id].lag);
    if (g->h_ctl) (void)hipHostFree(g->h_ctl);
    delete g;                                    // (the device buffers free themselves)
    ctx->set = nullptr;
}

// what both opens refuse alike
int open_admission(fv_ctx *ctx, const char *who, long long lag_rows_hint, int check_every, int &kernel)
{
    const std::string w = who;
    if (ctx->strm) { ctx->detail = w + ": a stream is already open on this context"; return FV_ERR_STATE; }
    if (ctx->set) { ctx->detail = w + ": a set of streams is already open on this context"; return FV_ERR_STATE; }
    if (ctx->group || ctx->comm || ctx->nranks > 1) {
        ctx->detail = w + ": one device, no communicator and no partition";
        return FV_ERR_UNSUPPORTED;
    }
    if (ctx->K == 0) { ctx->detail = w + ": no model"; return FV_ERR_STATE; }
    if (lag_rows_hint < 0 || lag_rows_hint > INT_MAX / 2 || check_every < 0 || check_every > STREAM_CHECK_MAX) {
        ctx->detail = w + ": lag_rows_hint >= 0 and check_every in 0 .. 64";
        return FV_ERR_ARG;
    }
    return fvi::stream_admit(ctx, kernel);
}

}  // namespace

void fvi::stream_drop(fv_ctx *ctx)
{
    if (!ctx->strm && !ctx->set) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    drop_set(ctx);
    fv_stream *s = ctx->strm;
    if (!s) return;
    if (s->h_ctl) (void)hipHostFree(s->h_ctl);
    delete s;                                    // (the device buffers free themselves)
    ctx->strm = nullptr;
}

extern "C" int fv_stream_open(fv_ctx *ctx, long long lag_rows_hint, int check_every)
{
    if (!ctx) return FV_ERR_ARG;
    int kernel = FV_KERNEL_AUTO;
    if (int rc = open_admission(ctx, "fv_stream_open", lag_rows_hint, check_every, kernel)) return rc;
    fv_stream *s = new (std::nothrow) fv_stream();
    if (!s) return FV_ERR_NOMEM;
    ctx->strm = s;
    const int rc = [&]() -> int {
        s->kernel = kernel;
        s->check_every = check_every ? check_every : STREAM_CHECK_DEFAULT;
        s->max_lag = ctx->max_lag;
        s->lag = lag_fresh(s->max_lag);
        FV_HIP(hipSetDevice(ctx->device));
        FV_HIP(ctx->d_counters.ensure(FV_NCOUNTERS));      // (the step kernels' statistics words, as every decode has them)
        FV_HIP(hipMemsetAsync(ctx->d_counters.p, 0, ctx->d_counters.bytes(), ctx->stream));
        if (int r = seq_alloc(ctx, s, (size_t)std::max(2ll, lag_rows_hint ? lag_rows_hint : STREAM_ROWS_DEFAULT))) return r;
        FV_HIP(s->ctl.ensure(1));
        FV_HIP(hipHostMalloc(reinterpret_cast<void **>(&s->h_ctl), sizeof(fvk::StreamCtl), hipHostMallocDefault));
        s->d_ctl = s->ctl.p;
        if (int r = seq_reset(ctx, s)) return r;
        FV_HIP(hipStreamSynchronize(ctx->stream));
        return 0;
    }();
    if (rc) { (void)hipGetLastError(); fvi::stream_drop(ctx); return rc; }
    s->st.kernel = kernel;
    s->st.arg_rows_capacity = (long long)s->cap;
    ctx->strm_stats = s->st;
    ctx->strm_lag = s->lag;
    ctx->strm_any = true;
    return FV_OK;
}

extern "C" int fv_stream_push(fv_ctx *ctx, const int *ob, int n, int *path_out, long long *committed_out)
{
    if (!ctx) return FV_ERR_ARG;
    if (int rc = push_admission(ctx, "fv_stream_push", ob, n, path_out, committed_out, StreamSeq::SYMBOLS)) return rc;
    for (int i = 0; i < n; ++i)
        if (ob[i] < 0 || ob[i] >= ctx->M) {
            ctx->detail = "fv_stream_push: ob[" + std::to_string(i) + "] = " + std::to_string(ob[i]) + " lies outside [0, M = " + std::to_string(ctx->M) + ")";
            return FV_ERR_ARG;
        }
    auto t0 = clk::now();
    FV_HIP(hipSetDevice(ctx->device));
    if (int rc = make_room(ctx, ctx->strm, n, "fv_stream_push")) return refused(ctx, rc);
    ctx->strm->kind = StreamSeq::SYMBOLS;
    const int rc = run_push(ctx, ctx->LB32T.p, ctx->LB64T.p, ob, n, path_out, committed_out);
    ctx->strm->st.push_ms_total += ms_since(t0);
    return rc < 0 ? refused(ctx, rc) : rc;
}

extern "C" int fv_stream_push_emissions(fv_ctx *ctx, const void *scores, int dtype, int n, long long ld, int *path_out,
                                        long long *committed_out)
{
    const char *who = "fv_stream_push_emissions";
    if (!ctx) return FV_ERR_ARG;
    if (int rc = push_admission(ctx, who, scores, n, path_out, committed_out, StreamSeq::SCORES)) return rc;
    fv_stream *s = ctx->strm;
    const fvi::EmisBlock b{ scores, dtype, n, ld };
    if (!fvi::emis_block_ok(ctx, b)) {
        ctx->detail = std::string(who) + ": ld >= K (ld >= P while an emission map is set) and dtype FV_EMIS_LOG_F32, _F64, _F16 or _BF16";
        return FV_ERR_ARG;
    }
    auto t0 = clk::now();
    FV_HIP(hipSetDevice(ctx->device));
    if (int rc = make_room(ctx, s, n, "fv_stream_push")) return refused(ctx, rc);
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
        FV_HIP(hipMemcpyAsync(s->d_ctl->emflags, s->h_ctl->emflags, sizeof s->h_ctl->emflags, hipMemcpyHostToDevice, ctx->stream));
        return 0;
    };
    if (int rc = fvi::stage_block(ctx, b, in_place ? nullptr : s->raw.p, s->e32.p, s->e64.p, s->d_ctl->emflags, reset)) return refused(ctx, rc);
    FV_HIP(hipMemcpyAsync(s->h_ctl->emflags, s->d_ctl->emflags, sizeof s->h_ctl->emflags, hipMemcpyDeviceToHost, ctx->stream));
    FV_HIP(hipStreamSynchronize(ctx->stream));
    const unsigned long long flags = s->h_ctl->emflags[0], where = s->h_ctl->emflags[1];
    if (flags & fvi::FV_EMIS_BAD) return fvi::emis_refusal(ctx, who, where, s->times);
    if ((flags & fvi::FV_EMIS_POSITIVE) && s->kernel != FV_KERNEL_F64_STREAM && s->kernel != FV_KERNEL_CSR_F64) {
        ctx->detail = fvi::filter_range_detail(ctx);
        return FV_ERR_UNSUPPORTED;
    }
    s->kind = StreamSeq::SCORES;
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
        rc = close_seq(ctx, s, path_out, n_out, score_out);
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

// ---------------------------------------------------------------------------------------------------------------------
// fv_streams_*: the set

namespace {

// one admitted call: the slots it names and the times each consumes
struct SetCall {
    const char *who;
    int nids;
    const int *ids;
    std::vector<int> n;                       // times of ids[q]
    int maxn = 0;
};

std::string slot_name(int id) { return "slot " + std::to_string(id); }

// What every push call checks first, in this order: the set, the pointers, the ids, dead slots, then lengths, kinds and
// room.  Nothing is changed: a refused call leaves every slot as it was.
int set_admission(fv_ctx *ctx, SetCall &c, const void *data, const long long *offsets, const int *path_out,
                  const long long *path_offsets, const long long *committed_out, int kind)
{
    const std::string w = c.who;
    fv_streams *g = ctx->set;
    if (!g) { ctx->detail = w + ": no set of streams is open (fv_streams_open)"; return FV_ERR_STATE; }
    if (!c.ids || c.nids < 1 || !data || !offsets || !path_out || !path_offsets || !committed_out) {
        ctx->detail = w + ": nids >= 1 slots and non-NULL pointers";
        return FV_ERR_ARG;
    }
    std::vector<char> seen((size_t)g->nslots, 0);
    for (int q = 0; q < c.nids; ++q) {
        const int id = c.ids[q];
        if (id < 0 || id >= g->nslots) { ctx->detail = w + ": ids[" + std::to_string(q) + "] = " + std::to_string(id) + " lies outside the set of " + std::to_string(g->nslots) + " slots"; return FV_ERR_ARG; }
        if (seen[(size_t)id]) { ctx->detail = w + ": " + slot_name(id) + " is named twice"; return FV_ERR_ARG; }
        seen[(size_t)id] = 1;
    }
    for (int q = 0; q < c.nids; ++q)
        if (g->slot[c.ids[q]].dead) {
            ctx->detail = w + ": " + slot_name(c.ids[q]) + " met a time without predecessors: fv_streams_close or fv_streams_abort";
            return FV_ERR_STATE;
        }
    if (offsets[0] != 0) { ctx->detail = w + ": offsets[0] must be 0"; return FV_ERR_ARG; }
    c.n.resize((size_t)c.nids);
    for (int q = 0; q < c.nids; ++q) {
        const StreamSeq &s = g->slot[c.ids[q]];
        const long long len = offsets[q + 1] - offsets[q];
        if (len < 1) { ctx->detail = w + ": " + slot_name(c.ids[q]) + " is given fewer than 1 time (a slot with nothing to push is left out)"; return FV_ERR_ARG; }
        if (offsets[q + 1] > INT_MAX / 2 || pending(&s) + len > INT_MAX / 2) { ctx->detail = w + ": " + slot_name(c.ids[q]) + ": more than 2^30 pushed or pending times"; return FV_ERR_ARG; }
        if (s.kind != StreamSeq::UNSET && s.kind != kind) {
            ctx->detail = w + ": the first push of " + slot_name(c.ids[q]) + "'s sequence fixed its input (symbols or score rows)";
            return FV_ERR_ARG;
        }
        if (path_offsets[q + 1] - path_offsets[q] < pending(&s) + len) {
            ctx->detail = w + ": " + slot_name(c.ids[q]) + " needs room for " + std::to_string(pending(&s) + len) + " path entries (pending + pushed), path_offsets leaves " +
                          std::to_string(path_offsets[q + 1] - path_offsets[q]);
            return FV_ERR_ARG;
        }
        c.n[(size_t)q] = (int)len;
        c.maxn = std::max(c.maxn, (int)len);
    }
    return 0;
}

// Every named slot's room for its pushed times (a refusal leaves the slots that grew before it grown, and nothing else changed).
// A new sequence in a slot (its first push) starts the slot's statistics over; the buffers are the slot's.
int set_room(fv_ctx *ctx, const SetCall &c)
{
    fv_streams *g = ctx->set;
    std::vector<fv_stream_stats> was((size_t)c.nids);
    std::vector<fv_lag_stats> was_lag((size_t)c.nids);
    for (int q = 0; q < c.nids; ++q) {
        StreamSeq &s = g->slot[c.ids[q]];
        was[(size_t)q] = s.st;
        was_lag[(size_t)q] = s.lag;
        if (s.times == 0) {
            s.st = fv_stream_stats{};
            s.st.kernel = g->kernel; s.st.arg_rows_capacity = (long long)s.cap;
            s.lag = lag_fresh(s.max_lag);
        }
        if (int rc = make_room(ctx, &s, c.n[(size_t)q], std::string(c.who) + ": " + slot_name(c.ids[q]), &g->st.syncs)) {
            for (int p = 0; p <= q; ++p)
                if (g->slot[c.ids[p]].times == 0) {       // (the sequences that left keep theirs)
                    g->slot[c.ids[p]].st = was[(size_t)p];
                    g->slot[c.ids[p]].lag = was_lag[(size_t)p];
                    g->slot[c.ids[p]].st.arg_rows_capacity = (long long)g->slot[c.ids[p]].cap;
                }
            return rc;
        }
    }
    return 0;
}

// The call, taken: the lock-steps, the two meetings with the device, the pieces.
// lb32 / lb64: the emission tables; row_of(q, i): the row of slot ids[q]'s pushed time i in them.
template <class RowOf>
int run_set_push(fv_ctx *ctx, const SetCall &c, int kind, const float *lb32, const double *lb64, RowOf &&row_of, int *path_out,
                 const long long *path_offsets, long long *committed_out, int *status_out)
{
    fv_streams *g = ctx->set;
    const size_t K = (size_t)ctx->K;
    const int nblk = (ctx->K + fvk::ANC_BLOCK - 1) / fvk::ANC_BLOCK;
    for (int q = 0; q < c.nids; ++q) g->slot[c.ids[q]].kind = kind == StreamSeq::SYMBOLS ? StreamSeq::SYMBOLS : StreamSeq::SCORES;
    auto row = [&](const StreamSeq &s, long long j) { return s.rows.p + (size_t)(j & 1) * ctx->nrows; };
    auto arg_row = [&](const StreamSeq &s, long long j) { return s.bp.p + (s.off + (size_t)(j - s.committed)) * K; };
    std::vector<fvi::StreamTask> tasks;
    std::vector<int> due;
    for (int i = 0; i < c.maxn; ++i) {
        tasks.clear(); due.clear();
        for (int q = 0; q < c.nids; ++q) {
            if (c.n[(size_t)q] <= i) continue;
            StreamSeq &s = g->slot[c.ids[q]];
            const long long j = s.times + i;
            const size_t e = (size_t)row_of(q, i) * K;
            if (j == 0) {
                s.h_ctl->sym0 = row_of(q, 0);
                FV_HIP(hipMemcpyAsync(&s.d_ctl->sym0, &s.h_ctl->sym0, sizeof(int), hipMemcpyHostToDevice, ctx->stream));
                if (int rc = fvi::stream_init_row(ctx, lb64, &s.d_ctl->sym0, row(s, 0))) return rc;
            } else {
                tasks.push_back(fvi::StreamTask{ row(s, j - 1), row(s, j), lb32 + e, lb64 + e, arg_row(s, j) });
                s.since_check += 1;
            }
            if (s.since_check > 0 && (s.since_check == g->check_every || i == c.n[(size_t)q] - 1)) due.push_back(q);
        }
        for (size_t base = 0; base < tasks.size(); base += (size_t)g->batch_cap) {
            const int nb = (int)std::min(tasks.size() - base, (size_t)g->batch_cap);
            if (int rc = fvi::stream_step_batch(ctx, g->kernel, tasks.data() + base, nb, i & 1)) return rc;
            g->st.step_launches += 1;
            g->st.task_steps += nb;
        }
        for (size_t base = 0; base < due.size(); base += fvk::CHECK_SLOTS) {
            fvk::LagArgs lg;
            fvk::CheckArgs &a = lg.a;
            a.n = (int)std::min(due.size() - base, (size_t)fvk::CHECK_SLOTS);
            a.K = ctx->K;
            for (int d = 0; d < a.n; ++d) {
                const int q = due[base + (size_t)d];
                StreamSeq &s = g->slot[c.ids[q]];
                const long long j = s.times + i;
                const int p = (int)(s.nchecks & 1);
                fvk::CheckSlot &cs = a.s[d];
                cs.bp_new = cs.bp_t = arg_row(s, j);
                cs.r = (int)s.since_check;
                cs.anc_in = s.anc.p + (size_t)p * K; cs.anc_out = s.anc.p + (size_t)(p ^ 1) * K;
                cs.ctl = s.d_ctl; cs.parity = p; cs.t = j; cs.base = s.committed; cs.path = s.path.p;
                lg.l[d] = fvk::LagSlot{ row(s, j), s.max_lag };
                s.nchecks += 1;
                s.since_check = 0;
            }
            for (int d = a.n; d < fvk::CHECK_SLOTS; ++d) { a.s[d] = fvk::CheckSlot{}; lg.l[d] = fvk::LagSlot{}; }
            if (g->max_lag > 0) {                // (fv_set_max_lag holds for every slot of the set)
                hipLaunchKernelGGL(fvk::stream_ancestors_lag_set, dim3(nblk, a.n), dim3(fvk::ANC_BLOCK), 0, ctx->stream, lg);
                hipLaunchKernelGGL(fvk::stream_decide_set, dim3(1, a.n), dim3(64), 0, ctx->stream, lg);
                hipLaunchKernelGGL(fvk::stream_apply_set, dim3(nblk, a.n), dim3(fvk::ANC_BLOCK), 0, ctx->stream, lg);
            } else {
                hipLaunchKernelGGL(fvk::stream_ancestors_set, dim3(nblk, a.n), dim3(fvk::ANC_BLOCK), 0, ctx->stream, a);
                hipLaunchKernelGGL(fvk::stream_verdict_set, dim3(nblk, a.n), dim3(fvk::ANC_BLOCK), 0, ctx->stream, a);
            }
            FV_HIP(hipGetLastError());
            g->st.check_launches += g->max_lag > 0 ? 3 : 2;
            g->st.check_slots += a.n;
        }
    }
    for (int q = 0; q < c.nids; ++q) {
        StreamSeq &s = g->slot[c.ids[q]];
        s.times += c.n[(size_t)q];
        s.st.times = s.times; s.st.pushes += 1; s.st.checks = s.nchecks;
    }
    // first meeting: every slot's control record in one copy
    FV_HIP(hipMemcpyAsync(g->h_ctl, g->ctl.p, (size_t)g->nslots * sizeof(fvk::StreamCtl), hipMemcpyDeviceToHost, ctx->stream));
    FV_HIP(hipStreamSynchronize(ctx->stream));
    g->st.syncs += 1;
    int worst = FV_OK;
    bool moved = false;
    std::vector<long long> count((size_t)c.nids, 0);
    std::string dead_detail;
    for (int q = 0; q < c.nids; ++q) {
        StreamSeq &s = g->slot[c.ids[q]];
        s.st.commits = s.h_ctl->commits;
        lag_take(&s);
        if (s.h_ctl->dead) {
            s.dead = true;
            if (dead_detail.empty()) dead_detail = std::string(c.who) + ": " + slot_name(c.ids[q]) + ": no state of the current time has a predecessor";
            worst = FV_ERR_NO_PRED;
            continue;
        }
        if (int rc = commit_queue(ctx, &s, path_out + path_offsets[q], count[(size_t)q])) return rc;
        moved = moved || count[(size_t)q] > 0;
    }
    // second meeting: the pieces and the retry counters of every slot whose record moved
    if (moved) {
        FV_HIP(hipStreamSynchronize(ctx->stream));
        g->st.syncs += 1;
    }
    for (int q = 0; q < c.nids; ++q) {
        StreamSeq &s = g->slot[c.ids[q]];
        committed_out[q] = count[(size_t)q];
        if (status_out) status_out[q] = s.dead ? FV_ERR_NO_PRED : FV_OK;
        if (!s.dead) commit_take(&s, count[(size_t)q]);
    }
    if (worst) ctx->detail = dead_detail;
    g->st.calls += 1;
    return worst;
}

// the wall time of a taken call goes, undivided, to every slot it named
int set_call_done(fv_ctx *ctx, const SetCall &c, clk::time_point t0, int rc)
{
    fv_streams *g = ctx->set;
    const double ms = ms_since(t0);
    g->st.push_ms_total += ms;
    for (int q = 0; q < c.nids; ++q) g->slot[c.ids[q]].st.push_ms_total += ms;
    return rc < 0 && rc != FV_ERR_NO_PRED ? refused(ctx, rc) : rc;
}

StreamSeq *set_slot(const fv_ctx *ctx, int id)
{
    return ctx && ctx->set && id >= 0 && id < ctx->set->nslots ? &ctx->set->slot[id] : nullptr;
}

// the slot is empty again: host counters and device words as after the open, the buffers and the statistics of the
// sequence that left stay (the next sequence's first push starts them over)
int slot_empty(fv_ctx *ctx, StreamSeq *s)
{
    s->kind = StreamSeq::UNSET;
    s->times = s->committed = 0;
    s->since_check = s->nchecks = 0;
    s->dead = false;
    s->off = 0;
    FV_HIP(hipSetDevice(ctx->device));
    return seq_reset(ctx, s);
}

}  // namespace

extern "C" int fv_streams_open(fv_ctx *ctx, int nslots, long long lag_rows_hint, int check_every)
{
    if (!ctx) return FV_ERR_ARG;
    int kernel = FV_KERNEL_AUTO;
    if (nslots < 1 || nslots > fvk::PASS_CHUNK) {
        ctx->detail = "fv_streams_open: nslots in 1 .. " + std::to_string(fvk::PASS_CHUNK);
        return FV_ERR_ARG;
    }
    if (int rc = open_admission(ctx, "fv_streams_open", lag_rows_hint, check_every, kernel)) return rc;
    fv_streams *g = new (std::nothrow) fv_streams();
    if (!g) return FV_ERR_NOMEM;
    ctx->set = g;
    const int rc = [&]() -> int {
        g->nslots = nslots;
        g->kernel = kernel;
        g->check_every = check_every ? check_every : STREAM_CHECK_DEFAULT;
        g->batch_cap = fvi::stream_batch_cap(ctx, kernel);
        g->max_lag = ctx->max_lag;
        g->slot.reset(new (std::nothrow) StreamSeq[(size_t)nslots]);
        if (!g->slot) return FV_ERR_NOMEM;
        FV_HIP(hipSetDevice(ctx->device));
        FV_HIP(ctx->d_counters.ensure(FV_NCOUNTERS));      // (the step kernels' statistics words, as every decode has them)
        FV_HIP(hipMemsetAsync(ctx->d_counters.p, 0, ctx->d_counters.bytes(), ctx->stream));
        FV_HIP(g->ctl.ensure((size_t)nslots));
        FV_HIP(hipHostMalloc(reinterpret_cast<void **>(&g->h_ctl), (size_t)nslots * sizeof(fvk::StreamCtl), hipHostMallocDefault));
        const size_t cap = (size_t)std::max(2ll, lag_rows_hint ? lag_rows_hint : STREAM_ROWS_DEFAULT);
        for (int id = 0; id < nslots; ++id) {
            StreamSeq *s = &g->slot[id];
            s->d_ctl = g->ctl.p + id; s->h_ctl = g->h_ctl + id;
            s->max_lag = g->max_lag;
            s->lag = lag_fresh(s->max_lag);
            if (int r = seq_alloc(ctx, s, cap)) return r;
            if (int r = seq_reset(ctx, s)) return r;
            s->st.kernel = kernel;
            s->st.arg_rows_capacity = (long long)cap;
        }
        FV_HIP(hipStreamSynchronize(ctx->stream));
        return 0;
    }();
    if (rc) {
        if (rc == FV_ERR_NOMEM && ctx->detail.empty()) ctx->detail = "fv_streams_open: the slots' buffers do not fit the device";
        (void)hipGetLastError();
        fvi::stream_drop(ctx);
        return rc;
    }
    g->st.nslots = nslots; g->st.batch_cap = g->batch_cap; g->st.kernel = kernel;
    ctx->set_stats = g->st;
    ctx->set_any = true;
    return FV_OK;
}

extern "C" int fv_streams_push(fv_ctx *ctx, const int *ids, int nids, const int *ob, const long long *offsets, int *path_out,
                               const long long *path_offsets, long long *committed_out, int *status_out)
{
    if (!ctx) return FV_ERR_ARG;
    SetCall c{ "fv_streams_push", nids, ids, {}, 0 };
    if (int rc = set_admission(ctx, c, ob, offsets, path_out, path_offsets, committed_out, StreamSeq::SYMBOLS)) return rc;
    for (int q = 0; q < nids; ++q)
        for (int i = 0; i < c.n[(size_t)q]; ++i) {
            const int x = ob[offsets[q] + i];
            if (x < 0 || x >= ctx->M) {
                ctx->detail = std::string(c.who) + ": " + slot_name(ids[q]) + ", time " + std::to_string(ctx->set->slot[ids[q]].times + i) + ": the symbol " +
                              std::to_string(x) + " lies outside [0, M = " + std::to_string(ctx->M) + ")";
                return FV_ERR_ARG;
            }
        }
    auto t0 = clk::now();
    FV_HIP(hipSetDevice(ctx->device));
    if (int rc = set_room(ctx, c)) return refused(ctx, rc);
    const int rc = run_set_push(ctx, c, StreamSeq::SYMBOLS, ctx->LB32T.p, ctx->LB64T.p, [&](int q, int i) { return ob[offsets[q] + i]; },
                                path_out, path_offsets, committed_out, status_out);
    return set_call_done(ctx, c, t0, rc);
}

extern "C" int fv_streams_push_emissions(fv_ctx *ctx, const int *ids, int nids, const void *scores, int dtype, const long long *offsets,
                                         long long ld, int *path_out, const long long *path_offsets, long long *committed_out,
                                         int *status_out)
{
    if (!ctx) return FV_ERR_ARG;
    SetCall c{ "fv_streams_push_emissions", nids, ids, {}, 0 };
    if (int rc = set_admission(ctx, c, scores, offsets, path_out, path_offsets, committed_out, StreamSeq::SCORES)) return rc;
    fv_streams *g = ctx->set;
    const std::string w = c.who;
    const int n = (int)offsets[nids];
    const fvi::EmisBlock b{ scores, dtype, n, ld };
    if (!fvi::emis_block_ok(ctx, b)) {
        ctx->detail = w + ": ld >= K (ld >= P while an emission map is set) and dtype FV_EMIS_LOG_F32, _F64, _F16 or _BF16";
        return FV_ERR_ARG;
    }
    auto t0 = clk::now();
    FV_HIP(hipSetDevice(ctx->device));
    if (int rc = set_room(ctx, c)) return refused(ctx, rc);
    // the staged block of the whole call and, for a block the kernel cannot read where it lies, its raw copy
    const fvi::PointerPlace at = fvi::pointer_place(scores);
    const bool in_place = at.on_device && at.device == ctx->device;
    const size_t cells = (size_t)n * (size_t)ctx->K, raw_bytes = in_place ? 0 : fvi::emis_raw_bytes(ctx, b);
    if (g->e32.ensure(cells) != hipSuccess || g->e64.ensure(cells) != hipSuccess || g->raw.ensure(raw_bytes) != hipSuccess) {
        (void)hipGetLastError();
        ctx->detail = w + ": " + std::to_string(12ull * cells + raw_bytes) + " bytes needed for the staged block";
        return refused(ctx, FV_ERR_NOMEM);
    }
    // the value rules decide whether the call is taken at all: one staging launch, its flags (slot 0's words) read before any step
    fvk::StreamCtl *h = g->h_ctl, *d = g->ctl.p;
    auto reset = [&]() -> int {
        h->emflags[0] = 0ull; h->emflags[1] = ~0ull;
        FV_HIP(hipMemcpyAsync(d->emflags, h->emflags, sizeof h->emflags, hipMemcpyHostToDevice, ctx->stream));
        return 0;
    };
    if (int rc = fvi::stage_block(ctx, b, in_place ? nullptr : g->raw.p, g->e32.p, g->e64.p, d->emflags, reset)) return refused(ctx, rc);
    FV_HIP(hipMemcpyAsync(h->emflags, d->emflags, sizeof h->emflags, hipMemcpyDeviceToHost, ctx->stream));
    FV_HIP(hipStreamSynchronize(ctx->stream));
    g->st.syncs += 1;
    const unsigned long long flags = h->emflags[0], where = h->emflags[1];
    if (flags & fvi::FV_EMIS_BAD) {
        // the lowest offending staged index, mapped back to (slot, time counted from that slot's sequence start, state)
        const long long r = (long long)(where / (unsigned long long)ctx->K);
        int q = 0;
        while (q + 1 < nids && offsets[q + 1] <= r) ++q;
        return fvi::emis_refusal(ctx, (w + ": " + slot_name(ids[q])).c_str(), where, g->slot[ids[q]].times - offsets[q]);
    }
    if ((flags & fvi::FV_EMIS_POSITIVE) && g->kernel != FV_KERNEL_F64_STREAM && g->kernel != FV_KERNEL_CSR_F64) {
        ctx->detail = fvi::filter_range_detail(ctx);
        return FV_ERR_UNSUPPORTED;
    }
    const int rc = run_set_push(ctx, c, StreamSeq::SCORES, g->e32.p, g->e64.p, [&](int q, int i) { return (int)offsets[q] + i; },
                                path_out, path_offsets, committed_out, status_out);
    return set_call_done(ctx, c, t0, rc);
}

extern "C" long long fv_streams_pending(const fv_ctx *ctx, int id)
{
    const StreamSeq *s = set_slot(ctx, id);
    return s ? pending(s) : -1;
}

extern "C" int fv_streams_close(fv_ctx *ctx, int id, int *path_out, long long *n_out, float *score_out)
{
    if (!ctx) return FV_ERR_ARG;
    if (!ctx->set) { ctx->detail = "fv_streams_close: no set of streams is open"; return FV_ERR_STATE; }
    StreamSeq *s = set_slot(ctx, id);
    if (!s || !path_out || !n_out) { ctx->detail = "fv_streams_close: a slot of the set, path_out and n_out"; return FV_ERR_ARG; }
    *n_out = 0;
    int rc = FV_OK;
    if (s->dead) {
        ctx->detail = "fv_streams_close: " + slot_name(id) + " met a time without predecessors";
        rc = FV_ERR_NO_PRED;
    } else if (s->times > 0) {
        rc = close_seq(ctx, s, path_out, n_out, score_out);
        ctx->set->st.syncs += 1;
        if (rc < 0 && rc != FV_ERR_NO_PRED) rc = refused(ctx, rc);
    }
    if (s->times > 0 || s->dead)
        if (int r = slot_empty(ctx, s)) return refused(ctx, r);
    return rc;
}

extern "C" int fv_streams_abort(fv_ctx *ctx, int id)
{
    if (!ctx) return FV_ERR_ARG;
    if (!ctx->set) { ctx->detail = "fv_streams_abort: no set of streams is open"; return FV_ERR_STATE; }
    StreamSeq *s = set_slot(ctx, id);
    if (!s) { ctx->detail = "fv_streams_abort: a slot of the set"; return FV_ERR_ARG; }
    if (s->times > 0 || s->dead)
        if (int r = slot_empty(ctx, s)) return refused(ctx, r);
    return FV_OK;
}

extern "C" int fv_streams_end(fv_ctx *ctx)
{
    if (!ctx) return FV_ERR_ARG;
    if (!ctx->set) { ctx->detail = "fv_streams_end: no set of streams is open"; return FV_ERR_STATE; }
    fvi::stream_drop(ctx);
    return FV_OK;
}

extern "C" int fv_streams_slot_stats(const fv_ctx *ctx, int id, fv_stream_stats *out)
{
    if (!ctx || !out) return FV_ERR_ARG;
    if (!ctx->set) return FV_ERR_STATE;
    const StreamSeq *s = set_slot(ctx, id);
    if (!s) return FV_ERR_ARG;
    *out = s->st;
    return FV_OK;
}

extern "C" int fv_streams_last_stats(const fv_ctx *ctx, fv_streams_stats *out)
{
    if (!ctx || !out) return FV_ERR_ARG;
    if (!ctx->set_any) return FV_ERR_STATE;
    *out = ctx->set ? ctx->set->st : ctx->set_stats;
    return FV_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// fv_set_max_lag, fv_last_lag_stats: the bounded commit lag

extern "C" int fv_set_max_lag(fv_ctx *ctx, long long max_lag)
{
    if (!ctx) return FV_ERR_ARG;
    if (max_lag < 0) { ctx->detail = "fv_set_max_lag: max_lag >= 0 (0: unbounded)"; return FV_ERR_ARG; }
    FV_NO_STREAM(ctx);
    ctx->max_lag = max_lag;
    return FV_OK;
}

extern "C" int fv_last_lag_stats(const fv_ctx *ctx, int slot, fv_lag_stats *out)
{
    if (!ctx || !out) return FV_ERR_ARG;
    if (slot < 0) {
        if (!ctx->strm_any) return FV_ERR_STATE;
        *out = ctx->strm ? ctx->strm->lag : ctx->strm_lag;
        return FV_OK;
    }
    if (!ctx->set_any) return FV_ERR_STATE;
    if (ctx->set) {
        const StreamSeq *s = set_slot(ctx, slot);
        if (!s) return FV_ERR_ARG;
        *out = s->lag;
        return FV_OK;
    }
    if ((size_t)slot >= ctx->set_lag.size()) return FV_ERR_ARG;
    *out = ctx->set_lag[(size_t)slot];
    return FV_OK;
}
