// fv_beam_kernels.hip.inc — gfx950 kernels of the FLASH-BS (dynamic beam) path.
// Included by fv_api.hip after fv_kernels.hip.inc.
//
// Reference: src/FLASH_BS_Viterbi_multithread.c.  Per step the reference (a) scores every
// destination state i against the B heap slots in slot order (:437-446), then (b) pushes the K
// scores, in state order, into a fresh B-entry min-heap (generate_state_heap, :167-211).
//
// What is observable of the heap, and how each piece is reproduced:
//   * its MEMBERS (B states + values) feed the next step's scores.  Members are the B largest
//     scores; they are order-free unless the B-th and (B+1)-th largest are equal finite values,
//     in which case which duplicate was evicted depends on the array layout.  `topb_select` finds
//     the members with a radix select (parallel) and falls back to the exact sequential replay
//     inside the same kernel when that duplicate case occurs.
//   * its ARRAY LAYOUT breaks exact ties between beam entries in (a) (lowest slot wins, :440-446)
//     and decides the whole-sequence end pick (slot 1 and slots B/2+2..B only, :456-461).  Layouts
//     are not needed to advance the scores, so they are rebuilt off the critical path:
//     `heap_build_all` replays generate_state_heap exactly for EVERY step of a generation
//     concurrently (two waves per step), `tie_fixup` then re-decides the few (step, state) cells
//     whose maximum was attained by more than one beam entry, and `beam_end_backtrack` reads the
//     last layout.
//   * T3_State (:448) is not stored: each step keeps the predecessor STATE of every destination;
//     back-tracking that chain from the end state yields T3 for every mid at once.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "fv_internal.h"
#include "fv_device_common.h"

namespace fvb {

constexpr int BEAM_COLS = 64;              // destination states per workgroup: one 512-byte run of a float64 row
constexpr int BEAM_WAVES = 16;             // each wave takes every 16th beam entry for the same 64 columns
constexpr int BEAM_BLOCK = BEAM_WAVES * 64;
constexpr int BEAM_UNROLL = 16;            // row gathers in flight per lane
constexpr int BEAM_CHUNK = 24;             // passes per beam_step / beam_end_backtrack launch (descriptors travel as kernel arguments)
constexpr int SEL_BLOCK = 1024;
constexpr int CUT_W = 8;                   // floats per step in the cut array (CUT_* below)
// cut[j] = what the select of step j leaves for the next step kernel, the next select and the resolve code:
constexpr int CUT_THETA = 0;               // cut value theta: the B-th largest score
constexpr int CUT_STATE = 1;               // 0: members exact, no duplicates at the cut; 1: SPECULATIVE — every theta-valued duplicate is in the
                                           // list, the survivors are not decided yet; 2: members exact, decided by the heap replay (slot order)
constexpr int CUT_NEXT = 2;                // lower bound predicted for the NEXT step's cut (+inf: none)
constexpr int CUT_LIST = 3;                // length of the candidate list the select saw
constexpr int CUT_N = 4;                   // entries in hval / hstate [j] (B, or G + E while speculative)
constexpr int CUT_MARGIN = 5;              // margin (in beam spreads) the bound of the NEXT step's candidate list was taken with
// Lazy replays (DESIGN 5.4).  Which of E equal scores at the cut survive in the reference's heap depends on the whole
// push history (the exact replay: sequential, 0.15 - 0.55 ms) — but the survivors only matter in the few columns of the
// NEXT step that a theta-valued entry wins ("doubtful" columns), and those almost never reach the next beam.  The
// select therefore keeps ALL E duplicates (up to BEAM_EXTRA more than B entries), the step kernel lists its doubtful
// columns, and a replay happens only when its result is observable: a doubtful column inside the next beam, the
// layout of the last heap of the whole-sequence pass, a fixed end state that is itself a cut duplicate, a tied cell
// on the back-tracked path.
constexpr int BEAM_EXTRA = 32;             // duplicates beyond B a speculative member list can hold (more: replay at once)
constexpr int DOUBT_CAP = 1024;            // doubtful columns listed per step (more: treated as reaching the beam)
__host__ __device__ inline int beam_pitch(int beam) { return beam + BEAM_EXTRA; }      // entries per step in hval / hstate
// (HNode {value, state}: heap node / select candidate, fv_internal.h)
constexpr int TIE_TAG = 1 << 30;           // set in a provisional back-pointer whose maximum was attained by more than one beam entry

// Row-major copy of the float64 table for row gathers: element (k, i) at k*ld + i, ld = roundup(K, 64),
// pad columns -inf.  A workgroup reads 512 contiguous bytes of every beam entry's row and neighbouring
// workgroups read the neighbouring 512: the rows of the beam are streamed, not sampled.
__global__ void relayout_rows(const double *t4, double *rm, int K, int nrows, int ld)
{
    const size_t n = (size_t)K * ld;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
        const int k = (int)(e / ld), i = (int)(e % ld);
        rm[e] = i < K ? t4[fvk::tab_index<4>(k, i, nrows)] : -__builtin_huge_val();
    }
}

// A model set by fv_set_model_sparse has no LA64R: its beam kernels (FV_OPT_SPARSE_BEAM) read the caller's rows by source
// state — row k = entries ptr[k] .. ptr[k + 1], columns strictly ascending, float64 logs (-inf: a stored 0).
struct CsrRows {
    const long long *ptr = nullptr;    // [K + 1]
    const int *col = nullptr;
    const double *log = nullptr;
};
// log A[state][col] of such a model: the stored log, -inf where the entry is absent (or a stored 0)
__device__ __forceinline__ double csr_log(const CsrRows &m, int state, int col)
{
    long long lo = m.ptr[state];
    const long long end = m.ptr[state + 1];
    long long hi = end;
    while (lo < hi) {                   // first entry whose column is >= col
        const long long mid = (lo + hi) >> 1;
        if (m.col[mid] < col) lo = mid + 1; else hi = mid;
    }
    return (lo < end && m.col[lo] == col) ? m.log[lo] : -__builtin_huge_val();
}

struct BeamSlot {
    const float *sval;     // [B] beam values (any order)
    const int *sstate;     // [B] beam states
    float *scores;         // [K] out: score of every destination state
    int *bp_row;           // [K] out: predecessor state (or -1), provisional where `tie` is set
    const float *tmp_row;  // (float)log B[i][ob[j]]
    int j;                 // absolute time of this step (for the tie list)
    const float *cut;      // [CUT_W] of the previous step's heap (CUT_*): theta, speculative?, lower bound predicted for
                           // THIS step's cut, number of entries in sval / sstate
    int *dupwin;           // per-step flag: a duplicate at the cut won a column (statistics)
    int *doubt;            // [DOUBT_CAP] columns of THIS step won by a theta-valued entry of a speculative list
    int *doubt_count;      // entries appended (may exceed DOUBT_CAP)
};
// Every per-step buffer of a beam decode is indexed by absolute time j, so a pass's select job for lock-step s
// follows from its first position alone (j = passL[q] + s): the select launch carries the bases, the pass list lives
// in device memory, and ONE launch selects for every active pass of a generation (up to T/2 of them) — a launch lasts
// as long as its slowest exact replay, so 24 passes at a time meant up to 22 such waits per lock-step.
struct BeamBase {
    float *scores_all;         // [T][K] scores after consuming ob[j]
    float *hval;               // [T][B] members of the heap built from scores_all[j] (any order)
    int *hstate;
    float *cut;                // [T][CUT_W]
    const int *passL;          // [passes of the generation] first position of each pass, longest pass first
};
struct BeamStepArgs {
    const double *LA64R;
    unsigned int *tie_count;   // number of entries in tie_list
    int2 *tie_list;            // (j, i) cells whose maximum is attained by more than one beam entry
    unsigned int tie_cap;
    unsigned long long *counters;
    const unsigned short *LAQ16R;   // beam_step_q16: row-major fixed-point table, pitch ldq
    const float *qpar;              // beam_step_q16: {qscale = -step, window = 2*max|Lq - L|} (device words, written by build_q16_rows)
    HNode *cand;                    // [T][cand_cap] scores >= the predicted lower bound of the cut, with their states (any order)
    int *cand_count;                // [T] entries appended for step j (may exceed cand_cap: the list is then not used)
    int cand_cap;                   // 0: no candidate lists
    int K, ld, ldq, beam, n;        // ld: row pitch of LA64R
    BeamSlot p[BEAM_CHUNK];         // the step kernels keep their descriptors in the kernel arguments (scalar loads; deriving
                                    // them on the device cost beam_step_q16 15 us per launch)
};

// Epilogue of both step kernels, executed by whole waves whose lanes each hold one finished score (inactive
// lanes: cnd = false): scores that can still be among the B largest of this step — those >= the lower bound the
// previous select predicted for this step's cut — are appended to the step's candidate list, so that the select
// reads a few B entries instead of K.  One returning atomic per wave; the order inside the list is arbitrary
// (members are order-free).  A list that overflows or turns out too short is simply ignored by topb_select.
__device__ __forceinline__ void append_candidates(const BeamStepArgs &args, int j, bool cnd, float v, int state)
{
    const unsigned long long m = __ballot(cnd);
    if (!m) return;
    const int leader = __ffsll((long long)m) - 1;
    int off = 0;
    if ((int)(threadIdx.x & 63) == leader) off = atomicAdd(args.cand_count + j, (int)__popcll(m));
    off = __shfl(off, leader);
    if (cnd) {
        const int pos = off + (int)__popcll(m & ((1ull << (threadIdx.x & 63)) - 1ull));
        if (pos < args.cand_cap) args.cand[(size_t)j * args.cand_cap + pos] = HNode{ v, state };
    }
}

// What every step kernel does with a finished column (beam_step, beam_step_q16 after their wave combine, beam_finish_csr
// after unpacking its accumulator), in one place so that the side outputs cannot drift: r = the column's maximum, a = the
// lowest index of the previous step's list that attains it, t = more than one entry attains it; sval / sst = that list
// (LDS or memory).  Writes the score and the provisional back-pointer, appends the tie list and the doubtful-column
// list, and returns whether the score belongs in the step's candidate list (append_candidates, called by whole waves).
__device__ __forceinline__ bool finish_column(const BeamStepArgs &args, const BeamSlot &ps, const int col, const float r, const int a,
                                              const int t, const float *sval, const int *sst, const bool spec, const float cut_theta)
{
    const bool any = r > -FLT_MAX;                  // score starts at -FLT_MAX, arg = -1 (FLASH_BS:439)
    ps.scores[col] = any ? r : -FLT_MAX;
    ps.bp_row[col] = any ? (t ? (sst[a] | TIE_TAG) : sst[a]) : -1;     // arg = -1 reads heap slot 0: State = -1 (:448, :65-70)
    if (any && t) {
        const unsigned int at = atomicAdd(args.tie_count, 1u);
        if (at < args.tie_cap) args.tie_list[at] = make_int2(ps.j, col);
    }
    // a column won by an entry that may not survive (a theta-valued duplicate of a speculative list): its score
    // is an upper bound and its back-pointer provisional until the replay of the previous step has run
    if (any && spec && sval[a] == cut_theta) {
        const int at = atomicAdd(ps.doubt_count, 1);
        if (at < DOUBT_CAP) ps.doubt[at] = col;
        atomicAdd(&args.counters[fvk::CNT_BEAM_DUP_COLS], 1ull);
        if (atomicExch(ps.dupwin, 1) == 0) atomicAdd(&args.counters[fvk::CNT_BEAM_DUP_STEPS], 1ull);
    }
    return any && r >= ps.cut[CUT_NEXT];
}

// (a): score_i = max over beam entries of (float)((double)(tmp_i + val) + logA[state][i])  (FLASH_BS:443),
// every cell with the float64 table: the reference's expression verbatim.  The value of the maximum does
// not depend on the order of the entries; WHICH entry attains it does only when two attain it exactly,
// and those cells are listed for tie_fixup.   grid = (64-column panels, passes); lane = column, wave w
// takes entries w, w+16, ...; BEAM_UNROLL independent row gathers are in flight per lane.
// NWV waves per workgroup: 16, or 4 for small beams (B <= 64: with 16 waves a wave sweeps at most four entries and most of the
// workgroup's time is the combine over the waves; four waves sweep 16 each, and four times as many workgroups share a CU).
template <int NWV>
__global__ __launch_bounds__(NWV * 64) void beam_step(const BeamStepArgs args)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const BeamSlot &ps = args.p[blockIdx.y];
    const int BP = beam_pitch(args.beam);
    // The previous step's list holds args.beam entries, or up to BEAM_EXTRA more while it is speculative.  Its length is
    // requested now and looked at only after the sweep over the first args.beam entries (a dependent load in front of
    // the sweep cost every step ~3 us): the tail, if any, is swept afterwards.
    const float cut_n = ps.cut[CUT_N], cut_state = ps.cut[CUT_STATE], cut_theta = ps.cut[CUT_THETA];
    float *sval = reinterpret_cast<float *>(smem);               // [BP]
    int *sst = reinterpret_cast<int *>(sval + BP);               // [BP]
    float *redV = reinterpret_cast<float *>(sst + BP);           // [NWV][64]
    int *redK = reinterpret_cast<int *>(redV + NWV * 64);
    int *redT = redK + NWV * 64;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int col = blockIdx.x * BEAM_COLS + lane;               // < ld: pad columns read -inf
    for (int s = tid; s < BP; s += (NWV * 64)) { sval[s] = ps.sval[s]; sst[s] = ps.sstate[s]; }      // (entries beyond the list: never used)
    const float tmp = col < args.K ? ps.tmp_row[col] : 0.0f;
    __syncthreads();
    const double *Lc = args.LA64R + col;
    float best = FV_NEG_INF;
    int arg = INT_MAX, tie = 0;
    auto sweep = [&](const int lo, const int hi) {               // this wave's entries (index = w modulo 16) inside [lo, hi)
        for (int s0 = lo + ((w - lo) & (NWV - 1)); s0 < hi; s0 += NWV * BEAM_UNROLL) {
            double L[BEAM_UNROLL];
#pragma unroll
            for (int u = 0; u < BEAM_UNROLL; ++u) {
                const int s = s0 + u * NWV;               // wave-uniform
                L[u] = s < hi ? Lc[(size_t)sst[s] * args.ld] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < BEAM_UNROLL; ++u) {
                const int s = s0 + u * NWV;
                if (s < hi) {
                    const float y = fvk::exact_cell(tmp, sval[s], L[u]);
                    if (y > best) { best = y; arg = s; tie = 0; }
                    else if (y == best && y > -FLT_MAX) tie = 1;
                }
            }
        }
    };
    sweep(0, args.beam);
    const int nlist = min((int)cut_n, BP);
    if (nlist > args.beam) sweep(args.beam, nlist);              // a speculative list's extra entries
    const bool spec = cut_state == 1.0f;
    redV[w * 64 + lane] = best; redK[w * 64 + lane] = arg; redT[w * 64 + lane] = tie;
    __syncthreads();
    if (w == 0) {
        bool cnd = false;
        float r = best;
        if (col < args.K) {
        // combine the waves: (value desc, entry asc), equal finite maxima => tie
        int a = arg, t = tie;
#pragma unroll
        for (int q = 1; q < NWV; ++q) {
            const float ov = redV[q * 64 + lane];
            const int ok = redK[q * 64 + lane], ot = redT[q * 64 + lane];
            if (ov == r && r > -FLT_MAX) t = 1;
            else if (ov > r) t = ot;
            if (fvk::better(ov, ok, r, a)) { r = ov; a = ok; }
        }
        cnd = finish_column(args, ps, col, r, a, t, sval, sst, spec, cut_theta);
        }
        if (args.cand_cap) append_candidates(args, ps.j, cnd, r, col);
    }
}

static inline size_t beam_step_lds(int beam, int nwv = BEAM_WAVES) { return (size_t)beam_pitch(beam) * 8 + (size_t)nwv * 64 * 12; }

// ---------------------------------------------------------------- beam step on the 16-bit table

// Row-major fixed-point copy of log A for beam_step_q16, built on the device from LA64R:
//   fvk::q16_range: lmax = largest finite |log A|;
//   q16_rows      : the codes and the largest distance actually made, from which q16_params takes the filter window
//                   (fvk::q16_step / q16_quantise: the same construction fv_set_model uses for the dense kernels' table).
__global__ void q16_rows(const double *rm, unsigned short *q, int K, int ld, int ldq, const unsigned long long *lmax_bits,
                         unsigned long long *dmax_bits)
{
    const double stepd = (double)fvk::q16_step(lmax_bits);
    const size_t n = (size_t)K * ldq;
    double dm = 0.0;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
        const int k = (int)(e / ldq), i = (int)(e % ldq);
        unsigned short code = 0xFFFFu;
        if (i < K) {
            const double l = rm[(size_t)k * ld + i];
            if (l > -__builtin_huge_val()) code = fvk::q16_quantise(l, stepd, dm);
        }
        q[e] = code;
    }
    fvk::q16_publish_max(dmax_bits, dm);
}

__global__ void q16_params(const unsigned long long *lmax_bits, const unsigned long long *dmax_bits, float *qpar)
{
    const double dmax = __longlong_as_double((long long)*dmax_bits);
    qpar[0] = -fvk::q16_step(lmax_bits);
    qpar[1] = __uint_as_float(__float_as_uint((float)(2.0 * dmax)) + 1u);      // rounded up
}

constexpr int BEAMQ_COLS = 128;            // destination states per workgroup: lane = 2 columns, one 256-byte run per row

// beam_step with filter + refine (as fvk::trellis_step, NB <= 2 form): the sweep reads 2 bytes per cell,
// y = fma(code, -step, tmp + val); every entry that can attain the exact maximum has y >= max(y) -
// (2*dmax + 3 float steps) and is re-evaluated with the reference expression from LA64R (one 8-byte
// gather); a lane whose second best is inside the window as well re-walks its own entries.  Exact ties
// are found among the re-evaluated values.  Needs every log <= 0 (else beam_step).
// NWV waves per workgroup (wave w takes entries w, w + NWV, ...): 16 for single-pass launches (one workgroup of 16 waves per
// CU and pass keeps the most loads in flight), 8 when the launch has more workgroups than the chip holds at once — four
// 8-wave workgroups share a CU instead of two 16-wave ones, so a batched launch of a small beam (B = 256: one sweep
// iteration per wave, the workgroup's time is mostly its fixed part) needs fewer rounds of workgroups.
template <int NWV>
__global__ __launch_bounds__(NWV * 64) void beam_step_q16(const BeamStepArgs args)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const BeamSlot &ps = args.p[blockIdx.y];
    const int BP = beam_pitch(args.beam);
    const float cut_n = ps.cut[CUT_N], cut_state = ps.cut[CUT_STATE], cut_theta = ps.cut[CUT_THETA];     // looked at after the first sweep (see beam_step)
    float *sval = reinterpret_cast<float *>(smem);               // [BP]
    int *sst = reinterpret_cast<int *>(sval + BP);               // [BP]
    float *redV = reinterpret_cast<float *>(sst + BP);           // [NWV][128]
    int *redK = reinterpret_cast<int *>(redV + NWV * BEAMQ_COLS);
    int *redT = redK + NWV * BEAMQ_COLS;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int col0 = blockIdx.x * BEAMQ_COLS + 2 * lane;         // this lane: columns col0, col0 + 1 (< ldq)
    for (int s = tid; s < BP; s += (NWV * 64)) { sval[s] = ps.sval[s]; sst[s] = ps.sstate[s]; }
    float tmp[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) tmp[c] = col0 + c < args.K ? ps.tmp_row[col0 + c] : 0.0f;
    const float qscale = args.qpar[0], window = args.qpar[1];
    __syncthreads();
    const unsigned int *Lq = reinterpret_cast<const unsigned int *>(args.LAQ16R) + (col0 >> 1);
    const size_t pitch = (size_t)(args.ldq >> 1);
    auto qf = [](unsigned int code) -> float { return code == 0xffffu ? __builtin_huge_valf() : (float)code; };
    float m1[2] = { FV_NEG_INF, FV_NEG_INF }, m2[2] = { FV_NEG_INF, FV_NEG_INF };
    int a1[2] = { -1, -1 };
    auto sweep = [&](const int lo, const int hi) {               // this wave's entries inside [lo, hi): index = w modulo 16 everywhere, so
                                                                 // that the re-walk below (entries w, w + 16, ...) covers exactly what the wave swept
    for (int s0 = lo + ((w - lo) & (NWV - 1)); s0 < hi; s0 += NWV * BEAM_UNROLL) {
        unsigned int L[BEAM_UNROLL];
#pragma unroll
        for (int u = 0; u < BEAM_UNROLL; ++u) {
            const int s = s0 + u * NWV;                   // wave-uniform
            L[u] = s < hi ? Lq[(size_t)sst[s] * pitch] : 0xffffffffu;
        }
#pragma unroll
        for (int u = 0; u < BEAM_UNROLL; ++u) {
            const int s = s0 + u * NWV;
            if (s < hi) {
                const float v = sval[s];
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const float y = __builtin_fmaf(qf(c ? L[u] >> 16 : L[u] & 0xffffu), qscale, tmp[c] + v);
                    const bool gt = y > m1[c];
                    m2[c] = __builtin_amdgcn_fmed3f(y, m1[c], m2[c]);
                    m1[c] = gt ? y : m1[c];
                    a1[c] = gt ? s : a1[c];
                }
            }
        }
    }
    };
    sweep(0, args.beam);
    const int B = min((int)cut_n, BP);                           // entries of the previous step's list
    if (B > args.beam) sweep(args.beam, B);                      // a speculative list's extra entries
    const bool spec = cut_state == 1.0f;
    // column maxima of the filter value over the 16 waves
#pragma unroll
    for (int c = 0; c < 2; ++c) redV[w * BEAMQ_COLS + 2 * lane + c] = m1[c];
    __syncthreads();
    float best[2], thr[2];
    int arg[2], tie[2];
    bool rewalk[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        float M = FV_NEG_INF;
#pragma unroll
        for (int q = 0; q < NWV; ++q) M = fmaxf(M, redV[q * BEAMQ_COLS + 2 * lane + c]);
        best[c] = FV_NEG_INF; arg[c] = INT_MAX; tie[c] = 0; rewalk[c] = false; thr[c] = __builtin_huge_valf();
        const int col = col0 + c;
        // M <= -FLT_MAX/2: every entry is unreachable or has no edge to this column: the cell stays (-FLT_MAX, -1)
        if (col < args.K && M > -0.5f * FLT_MAX) {
            thr[c] = fvk::refine_threshold(M, window);
            if (m2[c] >= thr[c] && m2[c] > FV_NEG_INF) rewalk[c] = true;        // two candidates of this lane's own
            else if (m1[c] >= thr[c] && a1[c] >= 0) {
                best[c] = fvk::exact_cell(tmp[c], sval[a1[c]], args.LA64R[(size_t)sst[a1[c]] * args.ld + col]);
                arg[c] = a1[c];
            }
        }
    }
    // Lanes with two candidates of their own re-walk their entries (ascending, so the first of equals is kept).  The
    // whole wave goes through the loop if any of its lanes has to, so it is the sweep once more — BEAM_UNROLL
    // independent row loads in flight (L2 hits now) — rather than one dependent load per entry: as a serial loop it
    // was the tail of every single-pass launch (cfg5: 69 -> ~50 us per step).
    if (__any(rewalk[0] || rewalk[1])) {
        for (int s0 = w; s0 < B; s0 += NWV * BEAM_UNROLL) {
            unsigned int L[BEAM_UNROLL];
#pragma unroll
            for (int u = 0; u < BEAM_UNROLL; ++u) {
                const int s = s0 + u * NWV;
                L[u] = s < B ? Lq[(size_t)sst[s] * pitch] : 0xffffffffu;
            }
#pragma unroll
            for (int u = 0; u < BEAM_UNROLL; ++u) {
                const int s = s0 + u * NWV;
                if (s < B) {
#pragma unroll
                    for (int c = 0; c < 2; ++c) {
                        const float y = __builtin_fmaf(qf(c ? L[u] >> 16 : L[u] & 0xffffu), qscale, tmp[c] + sval[s]);
                        if (rewalk[c] && y >= thr[c] && y > FV_NEG_INF) {
                            const float x = fvk::exact_cell(tmp[c], sval[s], args.LA64R[(size_t)sst[s] * args.ld + col0 + c]);
                            if (x > best[c]) { best[c] = x; arg[c] = s; tie[c] = 0; }
                            else if (x == best[c] && x > -FLT_MAX) tie[c] = 1;
                        }
                    }
                }
            }
        }
    }
    __syncthreads();                                              // redV is reused
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        redV[w * BEAMQ_COLS + 2 * lane + c] = best[c]; redK[w * BEAMQ_COLS + 2 * lane + c] = arg[c]; redT[w * BEAMQ_COLS + 2 * lane + c] = tie[c];
    }
    __syncthreads();
    if (tid < BEAMQ_COLS) {
        const int col = blockIdx.x * BEAMQ_COLS + tid;
        bool cnd = false;
        float r = FV_NEG_INF;
        if (col < args.K) {
            // combine the waves: (value desc, entry asc), equal finite maxima => tie
            r = redV[tid];
            int a = redK[tid], t = redT[tid];
#pragma unroll
            for (int q = 1; q < NWV; ++q) {
                const float ov = redV[q * BEAMQ_COLS + tid];
                const int ok = redK[q * BEAMQ_COLS + tid], ot = redT[q * BEAMQ_COLS + tid];
                if (ov == r && r > -FLT_MAX) t = 1;
                else if (ov > r) t = ot;
                if (fvk::better(ov, ok, r, a)) { r = ov; a = ok; }
            }
            cnd = finish_column(args, ps, col, r, a, t, sval, sst, spec, cut_theta);
        }
        if (args.cand_cap) append_candidates(args, ps.j, cnd, r, col);
    }
}

static inline size_t beam_step_q16_lds(int beam, int nwv = BEAM_WAVES) { return (size_t)beam_pitch(beam) * 8 + (size_t)nwv * BEAMQ_COLS * 12; }

// ---------------------------------------------------------------- exact heap replay (two waves)

// generate_state_heap for i = 0..K-1 (FLASH_BS:167-211), heap in LDS, 1-based like the reference:
// slots 1..B filled in state order (:172-183), create_min_heap (:96-123: smaller child via '>', stop on
// '<='), then replace_min_heap_element (:131-165) for every later state with v > root, strictly in state
// order (heap_replay_pair below).
// A node is one 8-byte word {value, state}; the two children of slot p are slots 2p and 2p+1 = 16
// aligned bytes, so a sift-down level costs one LDS round trip + one 8-byte write.
__device__ __forceinline__ void sift_hole(HNode *h, int B, int parent, float xv, int xs)
{
    int child = 2 * parent;
    while (child <= B) {
        HNode c0 = h[child];
        const HNode c1 = h[child + 1];            // slot B+1 exists in LDS (padding); ignored when child+1 > B
        if (child + 1 <= B && c0.v > c1.v) { c0 = c1; child++; }       // smaller child, left wins ties
        if (xv <= c0.v) break;                                         // equal keys are not swapped
        h[parent] = c0;
        parent = child;
        child *= 2;
    }
    h[parent] = HNode{ xv, xs };
}

// Lanes of ONE wave exchanging data through LDS need no hardware wait: the wave's DS instructions are
// executed in issue order, so a later ds_read sees an earlier ds_write of any lane.  Only the compiler
// has to be kept from moving or caching LDS accesses across this point.
__device__ __forceinline__ void wave_sync_lds()
{
    __asm__ volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

// The replay, software-pipelined and split over two waves of one workgroup.
//  * Floyd build level by level: nodes of one depth root disjoint subtrees, so their sift-downs
//    commute and run one per lane; depths are taken deepest first, as the reference's node = B/2..1
//    order does.
//  * Replace-root operations overlap: a sift-down only ever touches the node it stands on and that
//    node's children, so operation t+1 may work at depth d once operation t has reached depth d+2.
//    Each lane of the CONSUMER wave carries one operation in flight; a new one starts every second
//    tick.  The accept test of operation t+1 (v > root, :193) needs the root left by operation t, which
//    is final after t's first tick.  Per operation: 2 LDS round trips instead of log2(B).
//  * A single wave issues one instruction every ~5 cycles, so the replay's time is its instruction
//    count.  Everything that is not a tick therefore runs in a second, PRODUCER wave: it streams the
//    scores, drops those that cannot be accepted (v <= a root value the consumer published earlier:
//    the root never decreases, so a stale one only lets more through) and appends the rest, in state
//    order, to a ring in LDS.  The consumer pops 64 candidates at a time into registers, repeats the
//    accept test against the current root and runs the ticks.
//  * Ticks are branch-free.  Slots B+1..2B+1 hold +inf sentinels (a missing child never is the smaller
//    one and always stops the descent), idle lanes carry x = -inf and stand on the unused slot 0, whose
//    "children" are slots 0 and 1: they read harmlessly and write slot 0.
#ifdef FV_REPLAY_PROF
// Experiment builds only (tools/replay_prof.py): where a critical-path replay spends its time.
// [0] replays [1] cycles init+build [2] cycles main loop [3] cycles drain [4] batches [5] operations [6] empty polls [7] candidates popped
__device__ unsigned long long replay_prof[8];
__device__ unsigned long long reach_prof[8];       // select_finish: a reach event by phase
#endif
struct RingCtl { unsigned int tail, head, done, ready; float root; unsigned int pad[3]; };
constexpr int RING_CAP = 1024;             // candidates in flight between the two waves (power of two)
constexpr unsigned int SPIN_LIMIT = 1u << 22;   // every wait is bounded: a broken hand-shake must not hang the GPU

__device__ __forceinline__ unsigned int lds_ld(const unsigned int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void lds_st(unsigned int *p, unsigned int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ float lds_ldf(const float *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void lds_stf(float *p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ float readlane_f(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

static inline size_t heap_lds(int beam) { return (size_t)(2 * beam + 2) * 8 + sizeof(RingCtl) + (size_t)RING_CAP * 8; }

__device__ __forceinline__ HNode *replay_heap(unsigned char *smem) { return reinterpret_cast<HNode *>(smem); }

// Called by waves 0 (consumer) and 1 (producer) of a workgroup, after lane 0 of wave 0 has zeroed the
// RingCtl and a __syncthreads() has been passed.  Returns (in wave 0) with the heap in slots 1..B.
__device__ __forceinline__ void heap_replay_pair(const float *scores, int K, int B, unsigned char *smem, int wave, int lane,
                                                 unsigned long long *err_counter)
{
    HNode *h = replay_heap(smem);
    RingCtl *ctl = reinterpret_cast<RingCtl *>(h + 2 * B + 2);
    HNode *ring = reinterpret_cast<HNode *>(ctl + 1);
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    if (wave == 1) {
        // ---------------- producer
        unsigned int spins = 0;
        // The scores come out of L2 (~1 us away): the next AHEAD groups of 64 are in flight while the current ones
        // are filtered.  The ring's head is re-read only when the ring looks full.
        unsigned int tail = 0, head_seen = 0;
        constexpr int AHEAD = 12;
        float cur[AHEAD], nxt[AHEAD];
#pragma unroll
        for (int q = 0; q < AHEAD; ++q) {
            const int i = B + 64 * q + lane;
            cur[q] = i < K ? scores[i] : FV_NEG_INF;
        }
        // the first groups are on their way while the consumer builds the heap
        while (!lds_ld(&ctl->ready)) { __builtin_amdgcn_s_sleep(2); if (++spins > SPIN_LIMIT) { if (lane == 0) atomicAdd(err_counter, 1ull); return; } }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        for (int base = B; base < K; base += 64 * AHEAD) {
#pragma unroll
            for (int q = 0; q < AHEAD; ++q) {
                const int i = base + 64 * (AHEAD + q) + lane;
                nxt[q] = i < K ? scores[i] : FV_NEG_INF;          // -inf never passes (the root is a real score or -inf)
            }
#pragma unroll
            for (int q = 0; q < AHEAD; ++q) {
                const float root = lds_ldf(&ctl->root);          // as fresh as possible: every candidate kept out of the ring is a pop less
                const bool c = cur[q] > root;
                const unsigned long long m = __ballot(c);
                if (m) {
                    const unsigned int cnt = (unsigned int)__popcll(m);
                    spins = 0;
                    while (tail + cnt - head_seen > (unsigned int)RING_CAP) {
                        head_seen = lds_ld(&ctl->head);
                        if (tail + cnt - head_seen <= (unsigned int)RING_CAP) break;
                        __builtin_amdgcn_s_sleep(2);
                        if (++spins > SPIN_LIMIT) { if (lane == 0) atomicAdd(err_counter, 1ull); return; }
                    }
                    if (c) ring[(tail + (unsigned int)__popcll(m & lt_mask)) & (RING_CAP - 1)] = HNode{ cur[q], base + 64 * q + lane };
                    tail += cnt;
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                    if (lane == 0) lds_st(&ctl->tail, tail);
                }
            }
#pragma unroll
            for (int q = 0; q < AHEAD; ++q) cur[q] = nxt[q];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        if (lane == 0) lds_st(&ctl->done, 1u);
        return;
    }
    // ---------------- consumer
#ifdef FV_REPLAY_PROF
    const unsigned long long pt0 = __builtin_amdgcn_s_memtime();
    unsigned long long pn_batches = 0, pn_ops = 0, pn_empty = 0, pn_pop = 0;
#endif
    for (int i = lane; i < B; i += 64) h[i + 1] = HNode{ scores[i], i };
    for (int i = B + 1 + lane; i <= 2 * B + 1; i += 64) h[i] = HNode{ __builtin_huge_valf(), -1 };
    if (lane == 0) h[0] = HNode{ FV_NEG_INF, -1 };
    wave_sync_lds();
    const int last_inner = B / 2;
    for (int d = 31 - __clz(last_inner > 0 ? last_inner : 1); d >= 0 && last_inner > 0; --d) {
        const int lo = 1 << d, hi = min((2 << d) - 1, last_inner);
        for (int node = lo + lane; node <= hi; node += 64) {
            const HNode t = h[node];
            sift_hole(h, B, node, t.v, t.s);
        }
        wave_sync_lds();
    }
    float root = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(h[1].v)));   // wave-uniform, kept in an SGPR: an operation's first tick fixes the new root
    if (lane == 0) lds_stf(&ctl->root, root);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    if (lane == 0) lds_st(&ctl->ready, 1u);

    int p = 0, xs = 0;
    float xv = FV_NEG_INF;
    const unsigned int h_lds = (unsigned int)__builtin_amdgcn_readfirstlane((int)(unsigned int)(uintptr_t)(__attribute__((address_space(3))) HNode *)h);   // LDS byte address of slot 0 (wave-uniform: an SGPR operand below)
    // One wave alone on its SIMD issues an instruction every ~4.4 cycles, an LDS round trip is ~64 cycles and every
    // hop between the scalar and the vector side (ballot -> s_ff1 -> v_readlane -> v_writelane) costs 10-25 more
    // (tools/micro/lone_wave.hip).  So the whole operation is ONE hand-scheduled block: compares go through VCC
    // (VOP2 selects, no SGPR-pair forwarding), candidates stay in the lane they were popped into (starting an
    // operation = p := 1 in that lane, one masked move), and the only vector -> scalar hop is the new root.
    //   v[20:23] the two children {value, state} x 2, v24 kids address / child slot, v25 own address,
    //   v26 / v27 smaller child -> node to write, v28 value written (the root after an operation's first tick)
#define FV_TICK_READ \
    "v_lshl_add_u32 v24, %[p], 4, %[base]\n\t" \
    "ds_read_b128 v[20:23], v24\n\t"
#define FV_TICK_OWN \
    "v_lshl_add_u32 v25, %[p], 3, %[base]\n\t"
#define FV_TICK_XV \
    "v_cndmask_b32 %[xv], %[ninf], %[xv], vcc\n\t"          /* finished (go = 0): the lane idles with x = -inf */
#define FV_TICK_STEP \
    "s_waitcnt lgkmcnt(0)\n\t" \
    "v_cmp_gt_f32 vcc, v20, v22\n\t"                         /* right child strictly smaller: left wins ties */ \
    "v_cndmask_b32 v26, v20, v22, vcc\n\t" \
    "v_cndmask_b32 v27, v21, v23, vcc\n\t" \
    "v_addc_co_u32 v24, vcc, %[p], %[p], vcc\n\t"            /* child slot = 2p + right */ \
    "v_cmp_gt_f32 vcc, %[xv], v26\n\t"                       /* go: equal keys are not swapped */ \
    "v_cndmask_b32 v28, %[xv], v26, vcc\n\t" \
    "v_cndmask_b32 v27, %[xs], v27, vcc\n\t" \
    "ds_write2_b32 v25, v28, v27 offset1:1\n\t"              /* idle lanes: slot 0 */ \
    "v_cndmask_b32 %[p], 0, v24, vcc\n\t"
    const float neg_inf = FV_NEG_INF;              // in a VGPR: a literal and VCC would be two constant-bus reads
#define FV_TICK_CLOBBERS "v20", "v21", "v22", "v23", "v24", "v25", "v26", "v27", "v28", "vcc", "memory"
    auto tick = [&]() {
        __asm__ volatile(FV_TICK_READ FV_TICK_OWN FV_TICK_STEP FV_TICK_XV
                         : [p] "+v"(p), [xv] "+v"(xv), [xs] "+v"(xs) : [base] "s"(h_lds), [ninf] "v"(neg_inf) : FV_TICK_CLOBBERS);
    };
    unsigned int head = 0, spins = 0;
#ifdef FV_REPLAY_PROF
    const unsigned long long pt1 = __builtin_amdgcn_s_memtime();
#endif
    for (;;) {
        // (readfirstlane: every lane reads the same word; said so, the loop's control flow — and with it the SGPR
        // operands of the block below — is uniform for the compiler too)
        const unsigned int done = (unsigned int)__builtin_amdgcn_readfirstlane((int)lds_ld(&ctl->done));   // read before the tail: done is published after the final tail
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        const unsigned int tail = (unsigned int)__builtin_amdgcn_readfirstlane((int)lds_ld(&ctl->tail));
        if (tail == head) {
            if (done) break;
            __builtin_amdgcn_s_sleep(1);
#ifdef FV_REPLAY_PROF
            ++pn_empty;
#endif
            if (++spins > SPIN_LIMIT) { if (lane == 0) atomicAdd(err_counter, 1ull); break; }
            continue;
        }
        spins = 0;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#ifdef FV_REPLAY_PROF
        ++pn_batches;
#endif
        // The next candidates, in state order, go to the lanes that carry no operation (at most 6 do), lowest lane
        // first: lane order = state order, and a candidate never has to be moved to start its operation.
        const unsigned long long freem = __ballot(p == 0);
        const int ntake = (int)min(min(64u, tail - head), (unsigned int)__popcll(freem));
        const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned int)(freem >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)freem, 0u));
        const bool take = p == 0 && rank < ntake;
        if (take) {
            const HNode e = ring[(head + (unsigned int)rank) & (RING_CAP - 1)];
            xv = e.v; xs = e.s;
        }
        head += (unsigned int)ntake;
#ifdef FV_REPLAY_PROF
        pn_pop += (unsigned long long)ntake;
#endif
        wave_sync_lds();
        if (lane == 0) { lds_stf(&ctl->root, root); lds_st(&ctl->head, head); }     // issued after the reads above (LDS is in order per wave)
        // A candidate passes if v > the CURRENT root (FLASH_BS:193, in state order); the root only grows, so the
        // candidates in front of the first passing one are rejected for good.  Lanes outside `rem` (operations in
        // flight, candidates already decided) are never looked at again; a rejected candidate idles on slot 0 like
        // any idle lane (go = 1, it rewrites slot 0 with itself) until the lane is refilled.
        unsigned long long rem = __ballot(take);
        unsigned long long m = __ballot(xv > root) & rem;
        if (!m) continue;
        int n = __ffsll((long long)m) - 1;
        rem &= ~((2ull << n) - 1ull);
        // The loop over the accepted candidates of a batch is closed inside the block (its own label, aligned to an
        // instruction-cache line: a lone wave feels where its 300-byte loop body starts — builds that differed in
        // nothing else were 3 % apart).
        do {
#ifdef FV_REPLAY_PROF
            ++pn_ops;
#endif
            __asm__ volatile(
#ifndef FV_REPLAY_PROF
                ".p2align 6\n"
                "1:\n\t"
#endif
                "s_lshl_b64 s[20:21], 1, %[n]\n\t"
                "v_cndmask_b32_e64 %[p], %[p], 1, s[20:21]\n\t"               /* the operation starts on the root, in lane n */
                FV_TICK_READ FV_TICK_OWN FV_TICK_STEP
                "v_readlane_b32 %[root], v28, %[n]\n\t"                          /* its first tick fixes the new root */
                FV_TICK_READ FV_TICK_XV FV_TICK_OWN
                "v_cmp_lt_f32_e64 s[20:21], %[root], %[xv]\n\t"                  /* next candidate, in the shadow of the read */
                "s_and_b64 %[m], s[20:21], %[rem]\n\t"
                "s_ff1_i32_b64 %[n], %[m]\n\t"
                "s_lshl_b64 s[20:21], -2, %[n]\n\t"
                "s_and_b64 %[rem], %[rem], s[20:21]\n\t"
                FV_TICK_STEP FV_TICK_XV
#ifndef FV_REPLAY_PROF
                "s_cmp_lg_u64 %[m], 0\n\t"
                "s_cbranch_scc1 1b\n\t"
#endif
                : [p] "+v"(p), [xv] "+v"(xv), [xs] "+v"(xs), [root] "+s"(root), [rem] "+s"(rem), [n] "+s"(n), [m] "=&s"(m)
                : [base] "s"(h_lds), [ninf] "v"(neg_inf)
                : FV_TICK_CLOBBERS, "s20", "s21", "scc");
        } while (m);
    }
#ifdef FV_REPLAY_PROF
    const unsigned long long pt2 = __builtin_amdgcn_s_memtime();
#endif
    while (__ballot(p != 0)) tick();
    wave_sync_lds();
#ifdef FV_REPLAY_PROF
    if (lane == 0 && blockDim.x > 128) {
        const unsigned long long pt3 = __builtin_amdgcn_s_memtime();
        atomicAdd(&replay_prof[0], 1ull); atomicAdd(&replay_prof[1], pt1 - pt0); atomicAdd(&replay_prof[2], pt2 - pt1);
        atomicAdd(&replay_prof[3], pt3 - pt2); atomicAdd(&replay_prof[4], pn_batches); atomicAdd(&replay_prof[5], pn_ops);
        atomicAdd(&replay_prof[6], pn_empty); atomicAdd(&replay_prof[7], pn_pop);
    }
#endif
#undef FV_TICK_READ
#undef FV_TICK_OWN
#undef FV_TICK_XV
#undef FV_TICK_STEP
#undef FV_TICK_CLOBBERS
}

struct HeapRange { int L, R; };            // steps j = L..R of one pass (j = L is the init row)
constexpr int HEAP_CHUNK = 440;            // passes per launch: every replay of a generation in (nearly always) ONE launch,
                                           // whose duration is the slowest single replay
struct HeapAllArgs {
    const float *scores_all;   // [T][K]   scores of every step, by absolute time
    float *slot_val;           // [T][B]   exact heap layout per step, slot order
    int *slot_state;           // [T][B]
    unsigned long long *err_counter;   // broken producer/consumer hand-shake (never expected)
    const int *gate;                   // nullptr, or: run only if the flag of the range's sequence is up (its back-track met a tied cell)
    const int *seq_of;                 // batch decode: [total T] sequence of every absolute time (the flags are per sequence);
                                       // nullptr: one sequence, one flag
    int K, beam, n;
    HeapRange p[HEAP_CHUNK];
};

// Off the critical path: the exact layout of every step's heap, all steps of a generation at once.
// grid = (longest range, passes), two waves each (heap_replay_pair).
__global__ __launch_bounds__(128) void heap_build_all(const HeapAllArgs args)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const HeapRange r = args.p[blockIdx.y];
    if (args.gate && args.gate[args.seq_of ? args.seq_of[r.L] : 0] == 0) return;
    const int j = r.L + (int)blockIdx.x;
    if (j > r.R) return;
    const int B = args.beam;
    HNode *h = replay_heap(smem);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (threadIdx.x == 0) *reinterpret_cast<RingCtl *>(h + 2 * B + 2) = RingCtl{ 0u, 0u, 0u, 0u, 0.0f, { 0u, 0u, 0u } };
    __syncthreads();
    heap_replay_pair(args.scores_all + (size_t)j * args.K, args.K, B, smem, w, lane, args.err_counter);
    if (w != 0) return;
    for (int s = lane; s < B; s += 64) {
        const HNode n = h[s + 1];
        args.slot_val[(size_t)j * B + s] = n.v;
        args.slot_state[(size_t)j * B + s] = n.s;
    }
}

// ---------------------------------------------------------------- top-B members (critical path)

// What the resolve code (an exact replay of an earlier step + the re-evaluation of the doubtful columns it decides)
// works on; every per-step buffer is indexed by absolute time.
struct ResolveCtx {
    unsigned long long *counters;   // fvk::CNT_BEAM_EXACT_SETS exact replays run, CNT_HANDSHAKE_TIMEOUT broken hand-shake, CNT_BEAM_REACH_EVENTS
                                    // selects whose doubtful columns reached the beam, CNT_BEAM_CHAIN_CUTS chains of undecided steps cut
                                    // short by replay_safe
    int K, beam;
    int no_cut;                     // FV_OPT_DEBUG bit 23: always decide the whole trailing run of undecided steps (no replay_safe)
    const double *LA64R; int ld;    // float64 table, row-major, and its pitch
    const float *LB32T; const int *ob;
    int *bp;                        // [T][K]
    int *doubt; int *doubt_count;   // [T][DOUBT_CAP], [T]
    BeamBase b;
    CsrRows csr;                    // the CSR instantiations (patch_doubtful<true>) read these instead of LA64R
};
struct SelJob {
    const float *scores; float *sval; int *sstate;
    float *cut;                // [CUT_W] out (CUT_*)
    const float *prev_cut;     // cut of the previous step of the same pass (nullptr: none)
    const HNode *cand;         // candidate list of this step (beam_step's epilogue), nullptr: none
    int *cand_count;           // entries appended; reset to 0 here once read (the next generation re-uses the slot)
    int j, L;                  // absolute time of this step, first position of its pass
};
struct SelArgs {
    unsigned long long *counters;   // fvk::CNT_BEAM_CAND_SELECTS selects that ran on a candidate list, CNT_BEAM_SPEC_STEPS duplicate steps
                                    // carried speculatively (and the three CNT_BEAM_LIST_* words)
    float margin;                   // lower bound of the next cut = extrapolated theta - margin * (max score - theta)
    int cand_cap;
    int K, beam;
    int s;                          // lock-step: workgroup q works on time passL[q] + s (BeamBase)
    int no_wave;                    // FV_OPT_DEBUG bit 15: never the four-wave form of the select
    int eager;                      // FV_OPT_DEBUG bit 20: every duplicate step replays at once (no speculative lists)
    int quad_dirty;                 // FV_OPT_DEBUG bit 24: four-wave select also for steps that may have to be resolved
    int sb_rounds;                  // rounds per compaction block of the memory-resident selection (64; FV_OPT_DEBUG bit 22: 2)
    int T;                          // length of the sequence (the cut array holds T entries)
    int own_pred;                   // FV_OPT_DEBUG bit 7: predict the next cut from this pass's own last two cuts only
    const HNode *cand;              // [T][cand_cap]
    int *cand_count;                // [T]
    ResolveCtx rc;                  // rc.b: the per-step buffers; LISTED = false: jobs derived from its pass list (any number of passes per launch)
    SelJob p[BEAM_CHUNK];           // LISTED = true: up to BEAM_CHUNK jobs in the kernel arguments (the whole-sequence pass:
                                    // a select whose pointers come straight from the arguments is 15 us faster at cfg5)
};
__device__ __forceinline__ SelJob sel_job(const SelArgs &a, int q)
{
    const int L = __builtin_amdgcn_readfirstlane(a.rc.b.passL[q]);
    const int j = L + a.s;                                                  // wave-uniform by construction: keep every derived pointer in SGPRs
    const int BP = beam_pitch(a.beam);
    SelJob job;
    job.scores = a.rc.b.scores_all + (size_t)j * a.K;
    job.sval = a.rc.b.hval + (size_t)j * BP;
    job.sstate = a.rc.b.hstate + (size_t)j * BP;
    job.cut = a.rc.b.cut + (size_t)j * CUT_W;
    job.prev_cut = a.s >= 1 ? a.rc.b.cut + (size_t)(j - 1) * CUT_W : nullptr;
    job.cand = (a.cand_cap && a.s >= 1) ? a.cand + (size_t)j * a.cand_cap : nullptr;
    job.cand_count = a.cand_count + j;
    job.j = j; job.L = L;
    return job;
}

__device__ __forceinline__ float key2f(unsigned int k)          // inverse of f2key
{
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

__device__ __forceinline__ unsigned int f2key(float f)          // order-preserving float -> uint
{
    const unsigned int u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// Members of the heap generate_state_heap would leave: the B largest scores.
//
// Radix select of the B-th largest key theta, then a stable compaction (ascending state).  Scores of
// one step share sign and exponent, so a radix over the raw key bits would throw nearly every key
// into one bucket of its first passes (K same-address LDS atomics: 50 us at K = 16384).  The keys are
// therefore first rebased to q = key - min(real keys) + 1 (q = 0 for the two "never chosen" values
// -FLT_MAX / -inf, FLASH_BS:444) and the digits are taken from the top of the bits q actually uses:
// ceil(bits / 8) passes, the first of them spread over up to 256 buckets.  Within a wave the most
// frequent digit is added once (ballot), which bounds the cost of heavily tied score rows.
// With G = #{q > theta}, E = #{q == theta}, d = B - G: if d == E the members are exactly {q >= theta}.
// If d < E and theta is a real score, which duplicates survive depends on the heap layout -> wave 0
// replays the heap exactly.  If theta is q = 0 any d of them serve: the first d in state order.
// The compaction is done on ballots: element i = r*1024 + tid (round r, wave w, lane) precedes every
// element of a later (r, w), so per-(r, w) counts, one block-wide scan of them and a popcount of the
// lower lanes give each element's output position without any thread owning a contiguous range
// (coalesced loads, K/1024 elements per thread).
constexpr int SEL_WAVES = SEL_BLOCK / 64;
constexpr int SEL_MAX_ROUNDS = 64;         // K <= 65536

struct SelShared {
    unsigned int hist[256];
    unsigned int red[2 * SEL_WAVES];
    unsigned int sh_sel[3];
    uint2 wcnt[SEL_MAX_ROUNDS * SEL_WAVES];
};

// The selection itself.  REG: the keys live in R registers per thread (every key loaded once, all loads in flight
// together); !REG: every pass re-reads them from memory (no register budget: any K up to SEL_MAX_ROUNDS * 1024 —
// the fall-back of the lean candidate kernel below).  C / use_cand: see topb_select.
// NT threads take part (element i = r*NT + tid): the whole workgroup, or its first NT / 64 waves once the others have
// left the kernel (select_quad).
// Returns (the same value in every participating thread):
//   SEL_DONE    members written (exact: no duplicates straddle the cut);
//   SEL_SPEC    duplicates straddle the cut and the list now holds the scores above it plus ALL of the duplicates
//               (G + E <= B + BEAM_EXTRA entries): speculative, the survivors are decided only if somebody has to know;
//   SEL_REPLAY  duplicates straddle the cut and nothing was written: the caller runs the exact replay now.
constexpr int SEL_DONE = 0, SEL_SPEC = 1, SEL_REPLAY = 2;
template <int R, bool REG, int NT = SEL_BLOCK>
__device__ __forceinline__ int select_body(const SelArgs &args, const SelJob &job, SelShared &sh, const int C, const bool use_cand,
                                           const bool may_speculate)
{
    constexpr int NW = NT / 64;
    auto bsync = [] { if constexpr (NT == 64) wave_sync_lds(); else __syncthreads(); };      // NT < SEL_BLOCK: the other waves have left the kernel
    unsigned int *hist = sh.hist, *red = sh.red, *sh_sel = sh.sh_sel;
    uint2 *wcnt = sh.wcnt;
    const int B = args.beam;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int K = use_cand ? C : args.K;               // elements this select looks at
    const int rounds = (K + NT - 1) / NT;
    const int RR = REG ? R : rounds;                   // loop bound: compile time when the keys are in registers
    const unsigned int JUNK = f2key(-FLT_MAX);
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    auto fetch = [&](int r) -> float {
        const int i = r * NT + tid;
        return (r < rounds && i < K) ? (use_cand ? job.cand[i].v : job.scores[i]) : FV_NEG_INF;   // pads: q = 0, never counted (i >= K is checked)
    };

    // range of the real scores
    float val[REG ? R : 1];
    if constexpr (REG) {
#pragma unroll
        for (int r = 0; r < R; ++r) val[r] = fetch(r);
    }
    auto keyv = [&](int r) -> float { if constexpr (REG) return val[r]; else return fetch(r); };
    unsigned int lo = 0xffffffffu, hi = 0u;
#pragma unroll
    for (int r = 0; r < RR; ++r) {
        const unsigned int key = f2key(keyv(r));
        if (key > JUNK) { lo = min(lo, key); hi = max(hi, key); }
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) { lo = min(lo, (unsigned int)__shfl_xor((int)lo, m)); hi = max(hi, (unsigned int)__shfl_xor((int)hi, m)); }
    if (lane == 0) { red[w] = lo; red[NW + w] = hi; }
    bsync();
    if (tid == 0 && job.cand) *job.cand_count = 0;      // every thread has read it
#pragma unroll
    for (int q = 0; q < NW; ++q) { lo = min(lo, red[q]); hi = max(hi, red[NW + q]); }
    const unsigned int span1 = hi >= lo ? hi - lo + 1u : 0u;            // largest q
    const int nbits = span1 ? 32 - __clz(span1) : 0;
    auto q_of = [&](unsigned int key) -> unsigned int { return key > JUNK ? key - lo + 1u : 0u; };

    unsigned int prefix = 0, need = (unsigned)B, E = (unsigned)K;
    for (int top = nbits; top > 0;) {
        const int sh = max(top - 8, 0);
        const unsigned int dm = (1u << (top - sh)) - 1u;
        for (int i = tid; i < 256; i += NT) hist[i] = 0;
        bsync();
#pragma unroll
        for (int r = 0; r < RR; ++r) {
            if (r < rounds) {                                   // workgroup-uniform
                const int i = r * NT + tid;
                const unsigned int q = q_of(f2key(keyv(r)));
                const bool match = i < K && (top >= nbits || (q >> top) == (prefix >> top));
                const unsigned int digit = (q >> sh) & dm;
                const unsigned long long m = __ballot(match);
                if (m) {
                    const int f = __ffsll((long long)m) - 1;
                    const unsigned int d0 = (unsigned int)__builtin_amdgcn_readlane((int)digit, f);
                    const unsigned long long same = __ballot(match && digit == d0);
                    if (lane == f) atomicAdd(&hist[d0], (unsigned int)__popcll(same));
                    if (match && digit != d0) atomicAdd(&hist[digit], 1u);
                }
            }
        }
        bsync();
        if (w == 0) {
            // bucket holding the need-th largest key: suffix sums over 256 buckets, 4 per lane (lane 63 = top)
            const unsigned int h0 = hist[4 * lane], h1 = hist[4 * lane + 1], h2 = hist[4 * lane + 2], h3 = hist[4 * lane + 3];
            unsigned int own = h0 + h1 + h2 + h3, above = own;
#pragma unroll
            for (int m = 1; m < 64; m <<= 1) {
                const unsigned int o = __shfl_down(above, m);
                if (lane + m < 64) above += o;
            }
            above -= own;                                   // keys in buckets of higher lanes
            const bool here = above < need && above + own >= need;
            if (here) {
                unsigned int acc = above;
                int d = 4 * lane + 3;
                unsigned int hd = h3;
                if (acc + h3 >= need) { d = 4 * lane + 3; hd = h3; }
                else { acc += h3; if (acc + h2 >= need) { d = 4 * lane + 2; hd = h2; }
                else { acc += h2; if (acc + h1 >= need) { d = 4 * lane + 1; hd = h1; }
                else { acc += h1; d = 4 * lane; hd = h0; } } }
                sh_sel[0] = prefix | ((unsigned)d << sh);
                sh_sel[1] = need - acc;        // rank of theta inside bucket d
                sh_sel[2] = hd;
            }
        }
        bsync();
        prefix = sh_sel[0]; need = sh_sel[1]; E = sh_sel[2];
        top = sh;
    }
    const unsigned int theta = prefix, d = need;       // E: keys with q == theta (last pass: every bit resolved)
    const bool junk = theta == 0u;
    const bool replay = d < E && !junk;
    const bool spec = replay && may_speculate && E - d <= (unsigned)BEAM_EXTRA;
    const unsigned int keep = spec ? E : d;            // theta-valued entries written
    if (tid == 0) {
        const float th = key2f(junk ? JUNK : theta - 1u + lo);
        // what the pass of an earlier generation that covered these times left: its cut values (NaN: none — the
        // whole-sequence pass; the array is cleared per decode)
        const float old_this = job.cut[CUT_THETA], old_next = job.j + 1 < args.T ? job.cut[CUT_W + CUT_THETA] : -FLT_MAX;
        job.cut[CUT_THETA] = th;
        job.cut[CUT_STATE] = spec ? 1.0f : 0.0f;           // (a replay sets 2 when it has run)
        job.cut[CUT_N] = (float)((unsigned)B - d + keep);
        // Lower bound for the next step's cut: the cut value extrapolated linearly from the last two steps (the
        // scores of consecutive steps move by a nearly constant amount), minus a margin proportional to the spread
        // max - theta of this step's beam (+ a few float spacings so that a zero spread still leaves room).
        // Only a hint: a list that comes out shorter than B or longer than its capacity is not used.
        // The margin follows the lists it produces: a list of 1.25 B .. 2.5 B entries is what the select wants (2 B .. 4 B
        // for beams below 128: their lists are one round of keys either way) — shorter ones risk missing the cut, longer
        // ones cost rounds and overflow at 8 B (measured: 2 B .. 4 B cfg4 11.82 ms / cfg5 172.4; 1.5 .. 3: 11.67 / 171.1;
        // 1.25 .. 2.5: 11.55 / 170.3; 1.125 .. 2.25: 11.65 / 171.6); the count above the bound grows about e-fold per 0.3
        // spreads, so the margin moves in small factors, except after a miss.
        float next = __builtin_huge_valf(), mg = args.margin;
        if (job.prev_cut && job.prev_cut[CUT_MARGIN] > 0.0f && args.s >= 2) {
            mg = job.prev_cut[CUT_MARGIN];
            if (job.cand) mg *= C < B ? 2.0f : 4 * C < (B < 128 ? 8 : 5) * B ? 1.25f : C > args.cand_cap ? 0.5f : 2 * C > (B < 128 ? 8 : 5) * B ? 0.8f : 1.0f;
            mg = fminf(fmaxf(mg, 0.125f * args.margin), 16.0f * args.margin);
        }
        // The cut moves by nearly the same amount at the same time step in every pass that covers it (same observation,
        // same model), so a pass of a later generation extrapolates with the increment its predecessor saw there — good
        // from its second step on, where its own two cuts (the init row's and the first step's) say nothing yet.
        const bool seeded = !args.own_pred && old_this > -FLT_MAX && old_next > -FLT_MAX && old_this < FLT_MAX && old_next < FLT_MAX;
        if (!junk && (seeded || (job.prev_cut && job.prev_cut[0] > -FLT_MAX))) {
            const float hi_f = key2f(hi), pred = seeded ? th + (old_next - old_this) : th + (th - job.prev_cut[0]);
            const float ulp = fabsf(pred) * 1.1920929e-7f;
            next = pred - (mg * (hi_f - th) + 8.0f * ulp);
        }
        job.cut[CUT_MARGIN] = mg;
        job.cut[CUT_NEXT] = next;
        job.cut[CUT_LIST] = (float)C;
        if (use_cand) { atomicAdd(&args.counters[fvk::CNT_BEAM_CAND_SELECTS], 1ull); atomicAdd(&args.counters[fvk::CNT_BEAM_LIST_ENTRIES], (unsigned long long)C); }
        else if (job.cand && args.s >= 2) atomicAdd(&args.counters[C < B ? fvk::CNT_BEAM_LIST_SHORT : fvk::CNT_BEAM_LIST_LONG], 1ull);      // a list that was too short / overflowed
        if (spec) atomicAdd(&args.counters[fvk::CNT_BEAM_SPEC_STEPS], 1ull);
    }
    if (replay && !spec) return SEL_REPLAY;   // duplicate finite scores straddle the cut and may not be carried: exact replay (caller)
    if constexpr (!REG) {
        // Keys re-read from memory: any number of rounds (K > 65536: the only full-K selection there is), compacted in
        // blocks of up to 64 rounds — the per-(round, wave) counts of one block fill wcnt — with the counts of the earlier
        // blocks carried along; same positions as the one-block form below.
        const int SB = min(max(args.sb_rounds, 1), SEL_MAX_ROUNDS);
        unsigned int base_g = 0, base_e = 0;            // elements > theta / == theta in the blocks before this one
        for (int r0 = 0; r0 < rounds; r0 += SB) {
            const int rb = min(SB, rounds - r0);
            unsigned long long gtm = 0, eqm = 0;
            for (int r = 0; r < rb; ++r) {
                const int i = (r0 + r) * NT + tid;
                const unsigned int q = q_of(f2key(fetch(r0 + r)));
                const bool g = i < K && q > theta, e = i < K && q == theta;
                const unsigned long long bg = __ballot(g), be = __ballot(e);
                gtm |= (unsigned long long)g << r;
                eqm |= (unsigned long long)e << r;
                if (lane == 0) wcnt[r * NW + w] = make_uint2((unsigned int)__popcll(bg), (unsigned int)__popcll(be));
            }
            bsync();
            const int n = rb * NW;                          // <= NT
            const uint2 x = tid < n ? wcnt[tid] : make_uint2(0u, 0u);
            unsigned int ig = x.x, ie = x.y;
#pragma unroll
            for (int m = 1; m < 64; m <<= 1) {
                const unsigned int og = __shfl_up(ig, m), oe = __shfl_up(ie, m);
                if (lane >= m) { ig += og; ie += oe; }
            }
            if (lane == 63) { red[w] = ig; red[NW + w] = ie; }
            bsync();
            unsigned int bg = 0, be = 0, tg = 0, te = 0;
            for (int q = 0; q < NW; ++q) { if (q < w) { bg += red[q]; be += red[NW + q]; } tg += red[q]; te += red[NW + q]; }
            if (tid < n) wcnt[tid] = make_uint2(bg + ig - x.x, be + ie - x.y);
            bsync();
            for (int r = 0; r < rb; ++r) {
                const bool g = (gtm >> r) & 1ull, e = (eqm >> r) & 1ull;
                const unsigned long long mg = __ballot(g), me = __ballot(e);
                if (g || e) {
                    const uint2 o = wcnt[r * NW + w];
                    const unsigned int gb = base_g + o.x + (unsigned int)__popcll(mg & lt_mask);
                    const unsigned int eb = base_e + o.y + (unsigned int)__popcll(me & lt_mask);
                    if (g || eb < keep) {
                        const unsigned int pos = gb + min(eb, keep);
                        const int i = (r0 + r) * NT + tid;
                        job.sval[pos] = fetch(r0 + r);
                        job.sstate[pos] = use_cand ? job.cand[i].s : i;
                    }
                }
            }
            base_g += tg; base_e += te;
            bsync();                                        // wcnt / red are re-used by the next block
        }
        return spec ? SEL_SPEC : SEL_DONE;
    }
    // stable compaction
    unsigned long long gtm = 0, eqm = 0;               // bit r: this thread's element of round r is > / == theta
#pragma unroll
    for (int r = 0; r < RR; ++r) {
        if (r < rounds) {
            const int i = r * NT + tid;
            const unsigned int q = q_of(f2key(keyv(r)));
            const bool g = i < K && q > theta, e = i < K && q == theta;
            const unsigned long long bg = __ballot(g), be = __ballot(e);
            gtm |= (unsigned long long)g << r;
            eqm |= (unsigned long long)e << r;
            if (lane == 0) wcnt[r * NW + w] = make_uint2((unsigned int)__popcll(bg), (unsigned int)__popcll(be));
        }
    }
    bsync();
    {
        const int n = rounds * NW;                      // <= NT: one entry per thread, index order = element order
        const uint2 x = tid < n ? wcnt[tid] : make_uint2(0u, 0u);
        unsigned int ig = x.x, ie = x.y;
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            const unsigned int og = __shfl_up(ig, m), oe = __shfl_up(ie, m);
            if (lane >= m) { ig += og; ie += oe; }
        }
        if (lane == 63) { red[w] = ig; red[NW + w] = ie; }
        bsync();
        unsigned int bg = 0, be = 0;
        for (int q = 0; q < w; ++q) { bg += red[q]; be += red[NW + q]; }
        if (tid < n) wcnt[tid] = make_uint2(bg + ig - x.x, be + ie - x.y);
        bsync();
    }
#pragma unroll
    for (int r = 0; r < RR; ++r) {
        if (r < rounds) {
            const bool g = (gtm >> r) & 1ull, e = (eqm >> r) & 1ull;
            const unsigned long long bg = __ballot(g), be = __ballot(e);
            if (g || e) {
                const uint2 o = wcnt[r * NW + w];
                const unsigned int gb = o.x + (unsigned int)__popcll(bg & lt_mask);
                const unsigned int eb = o.y + (unsigned int)__popcll(be & lt_mask);
                if (g || eb < keep) {
                    const unsigned int pos = gb + min(eb, keep);
                    job.sval[pos] = keyv(r);
                    job.sstate[pos] = use_cand ? job.cand[r * NT + tid].s : r * NT + tid;
                }
            }
        }
    }
    return spec ? SEL_SPEC : SEL_DONE;
}

// ---------------------------------------------------------------- lazy replays: the resolve code

// Flags and counters that one workgroup writes and re-reads within a kernel (or that an earlier kernel of another CU
// wrote) go around the CU's vector cache.
__device__ __forceinline__ float ld_dev(const float *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int ld_dev(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_dev(float *p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// everything this workgroup stored so far is visible to its other waves' loads after the barrier
__device__ __forceinline__ void wg_publish()
{
    // workgroup scope: the waves of a workgroup share their CU's vector cache, and an agent-scope release on this
    // multi-die part writes the die's whole L2 back
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// The scores of step t still hold upper bounds in its doubtful columns: the step before it (of the same pass) is
// speculative and undecided, and a theta-valued entry of its list won at least one column.
__device__ __forceinline__ bool step_dirty(const ResolveCtx &c, int t, int L)
{
    return t > L && ld_dev(c.b.cut + (size_t)(t - 1) * CUT_W + CUT_STATE) == 1.0f && ld_dev(c.doubt_count + t) > 0;
}

// Exact replay of step t (its scores must be exact, or replay_safe(t) must hold): the members, in the heap's slot order, replace the list; waves 0
// (consumer) and 1 (producer) do the work, every live wave of the workgroup must call this.
__device__ __forceinline__ void replay_step(const ResolveCtx &c, int t, unsigned char *smem)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int B = c.beam, BP = beam_pitch(B);
    __syncthreads();                                 // LDS (heap, ring) is free
    if (threadIdx.x == 0) *reinterpret_cast<RingCtl *>(replay_heap(smem) + 2 * B + 2) = RingCtl{ 0u, 0u, 0u, 0u, 0.0f, { 0u, 0u, 0u } };
    __syncthreads();
    if (w < 2) heap_replay_pair(c.b.scores_all + (size_t)t * c.K, c.K, B, smem, w, lane, &c.counters[fvk::CNT_HANDSHAKE_TIMEOUT]);
    if (w == 0) {
        const HNode *h = replay_heap(smem);
        for (int s = lane; s < B; s += 64) { const HNode n = h[s + 1]; c.b.hval[(size_t)t * BP + s] = n.v; c.b.hstate[(size_t)t * BP + s] = n.s; }
        if (lane == 0) {
            st_dev(c.b.cut + (size_t)t * CUT_W + CUT_N, (float)B);
            st_dev(c.b.cut + (size_t)t * CUT_W + CUT_STATE, 2.0f);
            atomicAdd(&c.counters[fvk::CNT_BEAM_EXACT_SETS], 1ull);
        }
    }
    wg_publish();
}

// The doubtful columns of step t against the exact members of step t - 1 (in slot order after replay_step, so the lowest
// slot among equal maxima is the reference's own tie-break, FLASH_BS:440-446: score AND back-pointer come out exact).
// If the list overflowed every column is re-evaluated.  One wave per column, NW waves.
// CSR: the same over a model set by fv_set_model_sparse — log A[state][col] looked up in the state's row (csr_log), one
// lookup per member and column; the dense instantiation is the code below the branch, as it was.
template <bool CSR = false>
__device__ __forceinline__ void patch_doubtful(const ResolveCtx &c, int t, int NW)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int B = c.beam, BP = beam_pitch(B), K = c.K;
    const int listed = ld_dev(c.doubt_count + t);
    const bool all = listed > DOUBT_CAP;
    const int n = all ? K : listed;
    const float *sv = c.b.hval + (size_t)(t - 1) * BP;
    const int *ss = c.b.hstate + (size_t)(t - 1) * BP;
    const float *tmp_row = c.LB32T + (size_t)c.ob[t] * K;
    if constexpr (CSR) {
        for (int e = w; e < n; e += NW) {
            const int col = all ? e : c.doubt[(size_t)t * DOUBT_CAP + e];
            const float tmp = tmp_row[col];
            float best = FV_NEG_INF;
            int arg = INT_MAX;
            for (int sl = lane; sl < B; sl += 64) {       // ascending slots per lane: the first of equals is kept
                const float y = fvk::exact_cell(tmp, sv[sl], csr_log(c.csr, ss[sl], col));
                if (y > best) { best = y; arg = sl; }
            }
            // (fvk::wave_argbest, written out as at the dense site below: the selects and beam_resolve keep their instructions)
#pragma unroll
            for (int m = 1; m < 64; m <<= 1) {
                const float ov = __shfl_xor(best, m);
                const int ok = __shfl_xor(arg, m);
                if (fvk::better(ov, ok, best, arg)) { best = ov; arg = ok; }
            }
            if (lane == 0) {
                const bool any = best > -FLT_MAX;
                c.b.scores_all[(size_t)t * K + col] = any ? best : -FLT_MAX;
                c.bp[(size_t)t * K + col] = any ? ss[arg] : -1;
            }
        }
        wg_publish();
        return;
    }
    // the members are the same for every column: a lane's share of them (slots lane, lane + 64, ...) is fetched once, so that
    // a column costs one round of gathers instead of two dependent ones (B <= 1024; beyond that they are re-read)
    constexpr int HOLD = 16;
    float hv[HOLD];
    size_t hrow[HOLD];
    const bool held = B <= 64 * HOLD;
#pragma unroll
    for (int u = 0; u < HOLD; ++u) {
        const int sl = lane + 64 * u;
        hv[u] = (held && sl < B) ? sv[sl] : 0.0f;
        hrow[u] = (held && sl < B) ? (size_t)ss[sl] * c.ld : 0;
    }
    for (int e = w; e < n; e += NW) {
        const int col = all ? e : c.doubt[(size_t)t * DOUBT_CAP + e];
        const float tmp = tmp_row[col];
        const double *Lt = c.LA64R + col;
        float best = FV_NEG_INF;
        int arg = INT_MAX;
        if (held) {
            double L[HOLD];
#pragma unroll
            for (int u = 0; u < HOLD; ++u) L[u] = lane + 64 * u < B ? Lt[hrow[u]] : 0.0;          // every gather of the column in flight
#pragma unroll
            for (int u = 0; u < HOLD; ++u) {
                const int sl = lane + 64 * u;
                if (sl < B) {
                    const float y = fvk::exact_cell(tmp, hv[u], L[u]);
                    if (y > best) { best = y; arg = sl; }
                }
            }
        } else
        for (int s0 = lane; s0 < B; s0 += 256) {          // four gathers in flight per lane
            double L[4];
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int sl = s0 + 64 * u;
                v[u] = sl < B ? sv[sl] : 0.0f;
                L[u] = sl < B ? Lt[(size_t)ss[sl] * c.ld] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int sl = s0 + 64 * u;
                if (sl < B) {
                    const float y = fvk::exact_cell(tmp, v[u], L[u]);
                    if (y > best) { best = y; arg = sl; }
                }
            }
        }
        // fvk::wave_argbest written out: the call raises topb_select_cand<8 | 16, .., false> from 56 / 64 to 68 / 76 bytes of scratch
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            const float ov = __shfl_xor(best, m);
            const int ok = __shfl_xor(arg, m);
            if (fvk::better(ov, ok, best, arg)) { best = ov; arg = ok; }
        }
        if (lane == 0) {
            const bool any = best > -FLT_MAX;
            c.b.scores_all[(size_t)t * K + col] = any ? best : -FLT_MAX;
            c.bp[(size_t)t * K + col] = any ? ss[arg] : -1;
        }
    }
    wg_publish();
}

// For t = first .. last (ascending): if the scores of step t are not exact yet, decide step t - 1 (exact by then) and
// re-evaluate step t's doubtful columns.  Every live wave of the workgroup calls this; `bcast` is a shared word.
template <bool CSR = false>
__device__ __forceinline__ void resolve_range(const ResolveCtx &c, int L, int first, int last, unsigned char *smem, unsigned int *bcast, int NW)
{
    for (int t = first; t <= last; ++t) {
        __syncthreads();
        if (threadIdx.x == 0) *bcast = step_dirty(c, t, L) ? 1u : 0u;
        __syncthreads();
        if (!*bcast) continue;
        replay_step(c, t - 1, smem);
        patch_doubtful<CSR>(c, t, NW);
    }
}

// Would the exact replay of step t come out the same whatever the exact scores of its doubtful columns are?  What the
// scores hold there are upper bounds.  A push is accepted only if it exceeds the heap's root (FLASH_BS:193) — i.e. only if
// fewer than B of the scores pushed before it are >= it.  If every doubtful column c lies outside the initial build (c >= B)
// and at least B NON-doubtful scores of states < c are >= its upper bound, then in state order: the first doubtful column is
// not accepted (the heap before it holds non-doubtful scores only, its root is >= the bound), with the bound or with any
// smaller exact value — a skipped push leaves the heap untouched — so the same holds for the second, and so on: the heap never
// sees a doubtful column, and the replay of step t is exact although the steps before it are undecided.
// One wave per doubtful column; block-uniform answer.  More than SAFE_MAX doubtful columns: not tried.
constexpr int SAFE_MAX = 64;
__device__ __forceinline__ bool replay_safe(const ResolveCtx &c, int t, unsigned int *bcast, int NW)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int n = ld_dev(c.doubt_count + t);
    __syncthreads();
    if (threadIdx.x == 0) *bcast = n <= SAFE_MAX ? 1u : 0u;
    __syncthreads();
    if (n > SAFE_MAX) return false;
    const float *S = c.b.scores_all + (size_t)t * c.K;
    const int *dl = c.doubt + (size_t)t * DOUBT_CAP;
    auto wave_sum = [](int v) {
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
        return v;
    };
    for (int e = w; e < n; e += NW) {
        const int ce = dl[e];
        const float ue = ld_dev(S + ce);
        bool ok = ce >= c.beam;
        if (ok) {
            // doubtful columns in front of this one do not count
            int sub = 0;
            for (int x = lane; x < n; x += 64) { const int cx = dl[x]; if (cx < ce && ld_dev(S + cx) >= ue) ++sub; }
            const int need = c.beam + wave_sum(sub);
            int cnt = 0, total = 0;
            for (int i0 = 0; i0 < ce && total < need; i0 += 64 * 8) {            // 8 loads in flight per lane, a wave-wide sum per trip
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) { const int i = i0 + 64 * u + lane; v[u] = i < ce ? S[i] : FV_NEG_INF; }
#pragma unroll
                for (int u = 0; u < 8; ++u) cnt += v[u] >= ue ? 1 : 0;
                total = wave_sum(cnt);
            }
            ok = total >= need;
        }
        if (!ok && lane == 0) *bcast = 0u;            // (every writer stores the same value)
    }
    __syncthreads();
    return *bcast != 0u;
}

// Makes the scores of step `target` exact: the trailing run of undecided steps before it is decided, oldest first — the
// whole run back to a step with exact scores, or only back to a step whose replay does not depend on what is undecided
// (replay_safe: that step's members are then decided from its scores as they stand; its own doubtful columns keep their
// upper bounds, which is what any undecided step's hold).
template <bool CSR = false>
__device__ __forceinline__ void resolve_upto(const ResolveCtx &c, int L, int target, unsigned char *smem, unsigned int *bcast, int NW)
{
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = target;
        while (step_dirty(c, t, L)) --t;            // scores of t are exact, those of t + 1 .. target are not
        *bcast = (unsigned int)t;
    }
    __syncthreads();
    int t0 = (int)*bcast;
    if (!c.no_cut) {
        for (int t = target - 1; t > t0; --t) {     // (every one of these steps is undecided; replay_safe starts with a barrier)
            if (replay_safe(c, t, bcast, NW)) {
                if (threadIdx.x == 0) atomicAdd(&c.counters[fvk::CNT_BEAM_CHAIN_CUTS], 1ull);
                t0 = t;
                break;
            }
        }
    }
    resolve_range<CSR>(c, L, t0 + 1, target, smem, bcast, NW);
}

// Does a doubtful column of this step lie inside its beam (score >= theta: its membership, or the value it brings
// into the next step, depends on the undecided survivors)?  Block-uniform answer.
__device__ __forceinline__ bool doubtful_reach(const ResolveCtx &c, const SelJob &job, unsigned int *bcast, int NT)
{
    wg_publish();                                 // the cut value this workgroup's select has just written
    const int listed = ld_dev(c.doubt_count + job.j);
    if (threadIdx.x == 0) *bcast = listed > DOUBT_CAP ? 1u : 0u;
    __syncthreads();
    if (listed <= DOUBT_CAP) {
        const float theta = ld_dev(job.cut + CUT_THETA);
        bool hit = false;
        for (int e = threadIdx.x; e < listed; e += NT) hit |= job.scores[c.doubt[(size_t)job.j * DOUBT_CAP + e]] >= theta;
        if (hit) *bcast = 1u;                     // benign race: every writer stores the same value
    }
    __syncthreads();
    return *bcast != 0u;
}

// Everything after the first selection of a step (whole workgroup alive).  st = what select_body returned.
//   * an immediate replay (duplicates that a list cannot carry) needs exact scores;
//   * so does a step whose doubtful columns reach its beam: the undecided steps before it are decided now, the
//     columns re-evaluated, and the selection repeated on the exact scores (all K of them: the candidate list holds the
//     stale values).
template <int R, bool REG, int NT = SEL_BLOCK, bool CSR = false>
__device__ __forceinline__ void select_finish(const SelArgs &args, const SelJob &job, unsigned char *smem, SelShared &sh, int st, const bool dirty)
{
    const ResolveCtx &c = args.rc;
#ifdef FV_REPLAY_PROF
    // [0] events [1] ticks doubtful_reach [2] resolve_upto [3] repeated selection [4] final replay (if any) [5] final replays
    const unsigned long long q0 = __builtin_amdgcn_s_memtime();
    const bool reach = dirty && (st == SEL_REPLAY || doubtful_reach(c, job, &sh.sh_sel[0], NT));
    const unsigned long long q1 = __builtin_amdgcn_s_memtime();
    if (reach) {
        resolve_upto<CSR>(c, job.L, job.j, smem, &sh.sh_sel[0], NT / 64);
        const unsigned long long q2 = __builtin_amdgcn_s_memtime();
        if (threadIdx.x == 0) atomicAdd(&c.counters[fvk::CNT_BEAM_REACH_EVENTS], 1ull);
        st = select_body<R, REG, NT>(args, job, sh, 0, false, !args.eager);
        const unsigned long long q3 = __builtin_amdgcn_s_memtime();
        if (st == SEL_REPLAY) replay_step(c, job.j, smem);
        const unsigned long long q4 = __builtin_amdgcn_s_memtime();
        if (threadIdx.x == 0) {
            atomicAdd(&reach_prof[0], 1ull); atomicAdd(&reach_prof[1], q1 - q0); atomicAdd(&reach_prof[2], q2 - q1);
            atomicAdd(&reach_prof[3], q3 - q2); atomicAdd(&reach_prof[4], q4 - q3); if (st == SEL_REPLAY) atomicAdd(&reach_prof[5], 1ull);
        }
        return;
    }
    if (st == SEL_REPLAY) replay_step(c, job.j, smem);
    return;
#endif
    if (dirty && (st == SEL_REPLAY || doubtful_reach(c, job, &sh.sh_sel[0], NT))) {
        resolve_upto<CSR>(c, job.L, job.j, smem, &sh.sh_sel[0], NT / 64);
        if (threadIdx.x == 0) atomicAdd(&c.counters[fvk::CNT_BEAM_REACH_EVENTS], 1ull);
        st = select_body<R, REG, NT>(args, job, sh, 0, false, !args.eager);
    }
    if (st == SEL_REPLAY) replay_step(c, job.j, smem);
}

// Short candidate lists (<= QUAD_SEL_ROUNDS * 256 entries: B up to ~400) are selected by waves 0..3 — one per SIMD —
// with the keys in registers: the other twelve leave at once (s_barrier counts surviving waves only), so every one of
// the select's ~17 barriers joins 4 waves instead of 16.  (A single wave, no barrier at all, was slower: 2048 keys
// are 32 rounds of issue-bound work for one wave; measured +10 us per select at cfg4.)  A step that may have to be
// resolved (dirty) can end in a repeated selection over all K scores, which four waves can do for K <= 16384 only
// (64 rounds of 256): beyond that such steps keep the whole workgroup.
constexpr int QUAD_SEL_ROUNDS = 8;
__device__ __forceinline__ bool quad_ok(const SelArgs &args, const int C, const bool use_cand, const bool dirty)
{
    // (a dirty step keeps the whole workgroup: it may end in a resolve — replay, the doubtful columns re-evaluated one wave
    // per column, the selection repeated over all K scores — which four waves do ~70 us slower than sixteen (cfg4: ten such
    // events per decode against 2 us saved on sixty plain selects); args.quad_dirty, FV_OPT_DEBUG bit 24, allows it anyway
    // where four waves can repeat the selection at all: K <= 16384)
    return use_cand && C <= QUAD_SEL_ROUNDS * 256 && !args.no_wave && (!dirty || (args.quad_dirty && args.K <= SEL_MAX_ROUNDS * 256));
}
template <bool CSR = false>
__device__ __forceinline__ void select_quad(const SelArgs &args, const SelJob &job, unsigned char *smem, SelShared &sh, const int C, const bool dirty)
{
    __syncthreads();                                 // every thread has read C (the list's counter is reset below)
    if (threadIdx.x >= 256) return;
    const int st = select_body<QUAD_SEL_ROUNDS, true, 256>(args, job, sh, C, true, !args.eager);
    select_finish<1, false, 256, CSR>(args, job, smem, sh, st, dirty);
}

// R = rounds held in registers (compile time).  Candidate list of this step (beam_step's epilogue: every score >= a
// lower bound predicted for the cut): if it holds at least B entries and did not overflow, the B largest scores of
// the step are the B largest entries of the list, and every score equal to the cut value is in it: the select then
// reads the list instead of K scores.
template <int R, bool LISTED, bool CSR = false>
__global__ __launch_bounds__(SEL_BLOCK) void topb_select(const SelArgs args)
{
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ SelShared sh;
    const SelJob job = LISTED ? args.p[blockIdx.x] : sel_job(args, blockIdx.x);
    const int C = (job.cand && args.cand_cap) ? *job.cand_count : 0;
    const bool use_cand = C >= args.beam && C <= args.cand_cap && C <= R * SEL_BLOCK;
    const bool dirty = step_dirty(args.rc, job.j, job.L);
    if (quad_ok(args, C, use_cand, dirty)) { select_quad<CSR>(args, job, smem, sh, C, dirty); return; }
    const int st = select_body<R, true>(args, job, sh, C, use_cand, !args.eager);
    select_finish<R, true, SEL_BLOCK, CSR>(args, job, smem, sh, st, dirty);
}

// Lean form for the steps that have a candidate list when K needs the 64-round instantiation above (64 key registers
// + bookkeeping per thread do not fit 128 VGPRs: it spills): RC rounds of registers for the list; if the list
// turns out unusable (prediction off: rare), the same selection with the K scores re-read from memory in every pass.
template <int RC, bool LISTED, bool CSR = false>
__global__ __launch_bounds__(SEL_BLOCK) void topb_select_cand(const SelArgs args)
{
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ SelShared sh;
    const SelJob job = LISTED ? args.p[blockIdx.x] : sel_job(args, blockIdx.x);
    const int C = (job.cand && args.cand_cap) ? *job.cand_count : 0;
    const bool use_cand = C >= args.beam && C <= args.cand_cap && C <= RC * SEL_BLOCK;
    const bool dirty = step_dirty(args.rc, job.j, job.L);
    if (quad_ok(args, C, use_cand, dirty)) { select_quad<CSR>(args, job, smem, sh, C, dirty); return; }
    const int st = use_cand ? select_body<RC, true>(args, job, sh, C, true, !args.eager) : select_body<1, false>(args, job, sh, C, false, !args.eager);
    select_finish<1, false, SEL_BLOCK, CSR>(args, job, smem, sh, st, dirty);
}

// End of a generation, before the pass ends are read (one workgroup of four waves per pass).
//   mode 0  what the pass end needs and nothing else: the whole-sequence pass picks its end state from the LAYOUT of its
//           last heap, so that step's scores must be exact; any other pass asks whether its fixed end state is a MEMBER
//           of its last heap (Find_T3_State, FLASH_BS:73-86) — undecided only if that state is one of the theta-valued
//           duplicates of a speculative list, in which case the last step is decided now.
//   mode 1  (only if the flag of the pass's sequence is up: its back-tracked path met a tied cell, every layout of the
//           sequence is about to be rebuilt) every step's scores exact.
struct BeamEnd { int L, R, whole, seq; };   // seq: the sequence the pass belongs to (fv_decode_beam_batch; else 0) — its flag, its score
struct ResolveArgs {
    ResolveCtx rc;
    int mode, n;
    const int *gate;
    const int *ans;
    BeamEnd p[BEAM_CHUNK];
};
constexpr int RESOLVE_BLOCK = 256;
template <bool CSR = false>
__global__ __launch_bounds__(RESOLVE_BLOCK) void beam_resolve(const ResolveArgs args)
{
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ unsigned int bcast;
    const ResolveCtx &c = args.rc;
    const BeamEnd p = args.p[blockIdx.x];
    constexpr int NW = RESOLVE_BLOCK / 64;
    if (args.mode == 1) {
        if (args.gate && args.gate[p.seq] == 0) return;
        resolve_range<CSR>(c, p.L, p.L + 1, p.R, smem, &bcast, NW);
        return;
    }
    if (p.whole) { resolve_upto<CSR>(c, p.L, p.R, smem, &bcast, NW); return; }
    const int BP = beam_pitch(c.beam);
    const float *cut = c.b.cut + (size_t)p.R * CUT_W;
    if (threadIdx.x == 0) bcast = 0u;
    __syncthreads();
    if (ld_dev(cut + CUT_STATE) == 1.0f) {
        const int want = args.ans[p.R], n = min((int)ld_dev(cut + CUT_N), BP);
        const float theta = ld_dev(cut + CUT_THETA);
        for (int s = threadIdx.x; s < n; s += RESOLVE_BLOCK)
            if (c.b.hstate[(size_t)p.R * BP + s] == want && c.b.hval[(size_t)p.R * BP + s] == theta) bcast = 1u;
    }
    __syncthreads();
    if (!bcast) return;
    __syncthreads();
    resolve_upto<CSR>(c, p.L, p.R, smem, &bcast, NW);
    replay_step(c, p.R, smem);
}

// smallest instantiation that holds K (a candidate list is never longer than the scores it was taken from)
typedef void (*SelKernel)(const SelArgs);
// (csr: the instantiations whose resolve code looks log A up in CSR rows, for models set by fv_set_model_sparse)
static inline SelKernel sel_kernel_for(int K, bool listed, bool csr = false)
{
    if (csr) {
        if (K <= 4 * SEL_BLOCK) return listed ? topb_select<4, true, true> : topb_select<4, false, true>;
        if (K <= 16 * SEL_BLOCK) return listed ? topb_select<16, true, true> : topb_select<16, false, true>;
        return listed ? topb_select<SEL_MAX_ROUNDS, true, true> : topb_select<SEL_MAX_ROUNDS, false, true>;
    }
    if (K <= 4 * SEL_BLOCK) return listed ? topb_select<4, true> : topb_select<4, false>;
    if (K <= 16 * SEL_BLOCK) return listed ? topb_select<16, true> : topb_select<16, false>;
    return listed ? topb_select<SEL_MAX_ROUNDS, true> : topb_select<SEL_MAX_ROUNDS, false>;
}

// lean kernel for steps with a candidate list, where the generic one would be the 64-round instantiation
// (always: K beyond the register kernels' 64 rounds — every selection of such a model, listed or not, runs here)
static inline SelKernel sel_cand_kernel_for(int K, int cand_cap, bool listed, bool always = false, bool csr = false)
{
    if (!always && (K <= 16 * SEL_BLOCK || cand_cap <= 0)) return nullptr;
    if (csr) {
        if (cand_cap <= 8 * SEL_BLOCK) return listed ? topb_select_cand<8, true, true> : topb_select_cand<8, false, true>;
        return listed ? topb_select_cand<16, true, true> : topb_select_cand<16, false, true>;
    }
    if (cand_cap <= 8 * SEL_BLOCK) return listed ? topb_select_cand<8, true> : topb_select_cand<8, false>;
    return listed ? topb_select_cand<16, true> : topb_select_cand<16, false>;
}

// Capacity of a step's candidate list: a few B, and no list at all unless it is clearly shorter than K (a list of the
// usual 2 B .. 4 B entries is then a fraction of K: K = 3965 with B <= 256 has lists — 5.5 -> 4.5 ms at B = 32).
static inline int cand_cap_for(int K, int beam)
{
    int cap = (8 * beam + SEL_BLOCK - 1) / SEL_BLOCK * SEL_BLOCK;
    if (cap < SEL_BLOCK) cap = SEL_BLOCK;
    if (cap > 16 * SEL_BLOCK) cap = 16 * SEL_BLOCK;
    return cap * 3 <= 2 * K ? cap : 0;
}

static inline size_t sel_lds(int beam) { return heap_lds(beam); }

// ---------------------------------------------------------------- tie fix-up and pass end

struct FixArgs {
    const double *LA64R;
    const float *LB32T;
    const int *ob;
    const unsigned int *tie_count;
    const int2 *tie_list;
    unsigned int tie_cap;
    const float *slot_val;     // [T][B]
    const int *slot_state;     // [T][B]
    int *bp;                   // [T][K]
    unsigned long long *total; // statistics: cells re-decided, summed over the generations of a decode
    const int *gate;           // nullptr, or: run only if *gate != 0
    const int *seq_of;         // batch decode: [total T] sequence of every absolute time — gate[seq_of[j]] decides per listed
                               // cell (j, i), and `total` counts the cells re-decided; nullptr: one sequence, one flag
    int K, ld, beam;
    CsrRows csr;               // tie_fixup<true>: in place of LA64R
};

// For every listed (j, i): redo the reference's scan over the heap of step j-1 in SLOT order with
// strict '>' (FLASH_BS:440-446) and store the state of the winning slot.  One wave per cell.
// CSR: log A[slot's state][i] looked up in that state's row (csr_log) instead of gathered from LA64R.
template <bool CSR = false>
__global__ __launch_bounds__(256) void tie_fixup(const FixArgs args)
{
    const bool per_seq = args.gate && args.seq_of;
    if (args.gate && !per_seq && *args.gate == 0) return;
    const unsigned int n = min(*args.tie_count, args.tie_cap);
    if (!per_seq && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(args.total, (unsigned long long)n);
    unsigned int mine = 0;             // per_seq: cells this wave re-decided
    const int lane = threadIdx.x & 63;
    const unsigned int wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const unsigned int nwaves = gridDim.x * (blockDim.x >> 6);
    const int B = args.beam;
    for (unsigned int e = wave; e < n; e += nwaves) {
        const int2 cell = args.tie_list[e];
        const int j = cell.x, i = cell.y;
        if (per_seq) {                 // (wave-uniform: one cell per wave)
            if (args.gate[args.seq_of[j]] == 0) continue;
            ++mine;
        }
        const float tmp = args.LB32T[(size_t)args.ob[j] * args.K + i];
        const double *Lt = args.LA64R + i;
        const float *sv = args.slot_val + (size_t)(j - 1) * B;
        const int *ss = args.slot_state + (size_t)(j - 1) * B;
        float best = FV_NEG_INF;
        int arg = INT_MAX;
        // four independent gathers in flight per lane (a serial loop paid one HBM latency per 64 slots: 8 ms at cfg5)
        for (int s0 = lane; s0 < B; s0 += 256) {
            double L[4];
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int s = s0 + 64 * u;
                v[u] = s < B ? sv[s] : 0.0f;
                if constexpr (CSR) L[u] = s < B ? csr_log(args.csr, ss[s], i) : 0.0;
                else L[u] = s < B ? Lt[(size_t)ss[s] * args.ld] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int s = s0 + 64 * u;
                if (s < B) {
                    const float y = fvk::exact_cell(tmp, v[u], L[u]);
                    if (y > best) { best = y; arg = s; }
                }
            }
        }
        fvk::wave_argbest(best, arg);
        if (lane == 0 && best > -FLT_MAX) args.bp[(size_t)j * args.K + i] = ss[arg];
    }
    if (per_seq && lane == 0 && mine) atomicAdd(args.total, (unsigned long long)mine);
}

struct BeamEndArgs {
    int K, beam, n;
    int lazy;          // 1: first attempt, on provisional back-pointers: a tied cell on the path raises the flag of the pass's
                       //    sequence (flag[p.seq])
                       // 0: after tie_fixup; runs only if that flag is up
    int *flag;         // one per sequence of the call
    unsigned long long *restarts;      // counter fvk::BT_COUNTER: retries of the chunk walk
    BeamEnd p[BEAM_CHUNK];
};

// End of each pass + back-track, one wave per pass.
//  * whole-sequence pass: the end pick of FLASH_BS:456-461 over the exact LAYOUT of the last heap (slot 1, then slots
//    B/2+2..B, strict '>': the lowest slot among the maxima);
//  * other passes: the fixed end state must be a MEMBER of the last heap (Find_T3_State's scan, :73-86), else -1.
// The walk then follows the back-pointers.  Those are exact except in cells whose maximum two beam entries attained
// (TIE_TAG): which entry wins there depends on the heap layout of the step before.  Rebuilding every step's layout
// (heap_build_all + tie_fixup: a full replay per step, 5 % of cfg4) is needed only if the PATH runs through such a cell
// — 0.03 % of the cells at cfg4 — so the walk is first tried on the provisional pointers (lazy = 1); if it meets a
// tagged cell it raises the flag, and the gated heap_build_all / tie_fixup / second walk (queued behind it) do the work.
// In a batch decode the flags are per sequence (a tie on one sequence's path rebuilds that sequence's layouts only) and
// the whole-sequence pass of sequence s writes score_out[s].
__global__ __launch_bounds__(64) void beam_end_backtrack(const BeamEndArgs args, const float *slot_val, const int *slot_state,
                                                         const int *member_state, const float *cut, const int *bp, int *ans, float *score_out)
{
    const BeamEnd &p = args.p[blockIdx.x];
    int *const flag = args.flag + p.seq;
    if (!args.lazy && *flag == 0) return;
    const int B = args.beam, lane = threadIdx.x;
    int stt;
    if (p.whole) {
        const float *hval = slot_val + (size_t)p.R * B;
        const int *hstate = slot_state + (size_t)p.R * B;
        float score = FV_NEG_INF;
        int arg = INT_MAX;
        for (int i = lane; i < B; i += 64) {
            if (i != 0 && i < B / 2 + 1) continue;
            const float v = hval[i];
            if (fvk::better(v, i, score, arg)) { score = v; arg = i; }
        }
        fvk::wave_argbest(score, arg);
        stt = hstate[arg];
        if (lane == 0) { ans[p.R] = stt; score_out[p.seq] = score; }
    } else {
        // members of the last heap: B entries, or the scores above the cut plus every cut-valued duplicate while the
        // step is still speculative (beam_resolve has decided it if `want` is one of those duplicates)
        const int want = ans[p.R];
        const int BP = beam_pitch(B), n = min((int)cut[(size_t)p.R * CUT_W + CUT_N], BP);
        const int *hs = member_state + (size_t)p.R * BP;
        bool found = false;
        for (int s = lane; s < n; s += 64) found |= hs[s] == want;
        stt = __any(found) ? want : -1;
    }
    // state at time j -> state at time j - 1; a tagged (tied) cell yields its provisional state and sets `tag`
    const bool met_tag = fvk::chunk_walk(p.L, p.R, stt, ans + p.L, args.restarts, [&](int st, int j, bool &tag) {
        if (st < 0) return -1;
        int nx = bp[(size_t)j * args.K + st];
        if (nx >= 0 && (nx & TIE_TAG)) { tag = true; nx &= ~TIE_TAG; }
        return nx;
    });
    // (not lazy: tie_fixup has rewritten every listed cell.)  A lazy walk is finished even when it met a tag: what it
    // wrote below the tagged cell is provisional, and the gated second walk rewrites the whole range.
    if (met_tag && args.lazy && lane == 0) atomicExch(flag, 1);
}

// ---------------------------------------------------------------- beam step over CSR rows (FV_OPT_SPARSE_BEAM)

// The step of a model set by fv_set_model_sparse: there is no row of K cells to gather, so the sweep is turned round.
// Every entry s of the previous step's list scatters its row's stored transitions into a per-column accumulator, and a
// K-wide finish turns the accumulators into what beam_step leaves (DESIGN.md 5.4c).  The cell is the reference
// expression on the stored float64 log, so there is no condition on the values.
//   acc[j][col]     max over the entries of (ordered(y) << 32) | (0xFFFFFFFF - s); 0: no entry reaches the column.  The
//                   maximum does not depend on the order of the atomics, and among equal y the lowest s wins the low
//                   word — beam_step's provisional arg.
//   tieval[j][col]  max of ordered(y) over the entries that found their own y already in acc's high word.  Of two
//                   entries that attain the column's maximum the later one finds it there, and an equal pair below the
//                   maximum leaves a smaller value: the column is tied at its maximum iff tieval == high word of acc.
// y is canonicalised (y + 0.0f) first: beam_step compares with ==, for which -0.0 equals +0.0, bit keys would not.
struct BeamCsrArgs {
    BeamStepArgs a;                // LA64R / LAQ16R / qpar unused
    CsrRows m;
    unsigned long long *acc;       // [T][K], all zero between launches (beam_finish_csr clears what it read)
    unsigned int *tieval;          // [T][K]
};
constexpr int CSR_SCATTER_WAVES = 4;       // list entries per workgroup: one wave each
constexpr int CSR_FINISH_BLOCK = 256;      // columns per workgroup of the finish

// entries of the previous step's list the step sweeps: args.beam, or up to BEAM_EXTRA more while it is speculative (beam_step)
__device__ __forceinline__ int step_list_len(const BeamStepArgs &args, const BeamSlot &ps)
{
    return max(args.beam, min((int)ps.cut[CUT_N], beam_pitch(args.beam)));
}

// grid = (entry groups, passes); a wave takes one list entry and walks its row with its lanes
__global__ __launch_bounds__(CSR_SCATTER_WAVES * 64) void beam_scatter_csr(const BeamCsrArgs ca)
{
    const BeamStepArgs &args = ca.a;
    const BeamSlot &ps = args.p[blockIdx.y];
    const int lane = threadIdx.x & 63;
    const int s = blockIdx.x * CSR_SCATTER_WAVES + (int)(threadIdx.x >> 6);      // wave-uniform
    if (s >= step_list_len(args, ps)) return;
    const int k = ps.sstate[s];
    if (k < 0 || k >= args.K) return;                  // (a list holds states; never follow anything else into the row table)
    const float v = ps.sval[s];
    const long long e1 = ca.m.ptr[k + 1];
    unsigned long long *acc = ca.acc + (size_t)ps.j * args.K;
    unsigned int *tieval = ca.tieval + (size_t)ps.j * args.K;
    for (long long e = ca.m.ptr[k] + lane; e < e1; e += 64) {
        const double L = ca.m.log[e];
        const int col = ca.m.col[e];
        if (!(L > -__builtin_huge_val()) || col < 0 || col >= args.K) continue;      // a stored 0 never wins (FLASH:171)
        const float y = fvk::exact_cell(ps.tmp_row[col], v, L) + 0.0f;
        if (y > -FLT_MAX) {
            const unsigned int hi = f2key(y);
            const unsigned long long old = atomicMax(acc + col, ((unsigned long long)hi << 32) | (0xFFFFFFFFu - (unsigned int)s));
            if ((unsigned int)(old >> 32) == hi) atomicMax(tieval + col, hi);
        }
    }
}

// grid = (K / CSR_FINISH_BLOCK, passes); lane = column
__global__ __launch_bounds__(CSR_FINISH_BLOCK) void beam_finish_csr(const BeamCsrArgs ca)
{
    const BeamStepArgs &args = ca.a;
    const BeamSlot &ps = args.p[blockIdx.y];
    const int col = blockIdx.x * CSR_FINISH_BLOCK + threadIdx.x;
    const float cut_state = ps.cut[CUT_STATE], cut_theta = ps.cut[CUT_THETA];
    bool cnd = false;
    float r = FV_NEG_INF;
    if (col < args.K) {
        const size_t at = (size_t)ps.j * args.K + col;
        const unsigned long long key = ca.acc[at];
        const unsigned int tv = ca.tieval[at];
        int a = INT_MAX, t = 0;
        if (key) {
            const unsigned int hi = (unsigned int)(key >> 32);
            r = key2f(hi);
            a = (int)(0xFFFFFFFFu - (unsigned int)key);
            t = tv == hi ? 1 : 0;
            ca.acc[at] = 0ull;                         // one memset per decode, not per step
            if (tv) ca.tieval[at] = 0u;
        }
        cnd = finish_column(args, ps, col, r, a, t, ps.sval, ps.sstate, cut_state == 1.0f, cut_theta);
    }
    if (args.cand_cap) append_candidates(args, ps.j, cnd, r, col);
}

static inline int allow_big_lds(std::string &detail)
{
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&beam_step<16>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, fvk::LDS_LIMIT);
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(&beam_step<4>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, fvk::LDS_LIMIT);

    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(&beam_step_q16<16>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, fvk::LDS_LIMIT);
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(&beam_step_q16<8>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, fvk::LDS_LIMIT);

    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(&heap_build_all),
                                hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(&beam_resolve<false>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(&beam_resolve<true>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
    const void *sel[] = { reinterpret_cast<const void *>(&topb_select<4, true, true>), reinterpret_cast<const void *>(&topb_select<4, false, true>),
                          reinterpret_cast<const void *>(&topb_select<16, true, true>), reinterpret_cast<const void *>(&topb_select<16, false, true>),
                          reinterpret_cast<const void *>(&topb_select<SEL_MAX_ROUNDS, true, true>), reinterpret_cast<const void *>(&topb_select<SEL_MAX_ROUNDS, false, true>),
                          reinterpret_cast<const void *>(&topb_select_cand<8, true, true>), reinterpret_cast<const void *>(&topb_select_cand<8, false, true>),
                          reinterpret_cast<const void *>(&topb_select_cand<16, true, true>), reinterpret_cast<const void *>(&topb_select_cand<16, false, true>), reinterpret_cast<const void *>(&topb_select<4, true>), reinterpret_cast<const void *>(&topb_select<4, false>),
                          reinterpret_cast<const void *>(&topb_select<16, true>), reinterpret_cast<const void *>(&topb_select<16, false>),
                          reinterpret_cast<const void *>(&topb_select<SEL_MAX_ROUNDS, true>), reinterpret_cast<const void *>(&topb_select<SEL_MAX_ROUNDS, false>),
                          reinterpret_cast<const void *>(&topb_select_cand<8, true>), reinterpret_cast<const void *>(&topb_select_cand<8, false>),
                          reinterpret_cast<const void *>(&topb_select_cand<16, true>), reinterpret_cast<const void *>(&topb_select_cand<16, false>) };
    for (const void *f : sel)
        if (e == hipSuccess) e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
    if (e != hipSuccess) { detail = std::string("hipFuncSetAttribute(beam): ") + hipGetErrorString(e); return FV_ERR_DEVICE; }
    return 0;
}

}  // namespace fvb
