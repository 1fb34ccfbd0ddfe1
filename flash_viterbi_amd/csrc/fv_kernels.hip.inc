// fv_kernels.hip.inc — gfx950 kernels of the full-state FLASH Viterbi path.
// Included by fv_full.hip only (fv_device_common.h holds what the FLASH-BS kernels share).  wave = 64 lanes everywhere in this file.
//
// Data layout in HBM (built once by fv_set_model):
//   LA32 float  (float)log((double)A[k][i])   k = source state (row), i = destination (column)
//   LA64 double log((double)A[k][i])
//   LA16 half   log A rounded to IEEE binary16;  LAQ16 u16 fixed point -(code*step), 0xffff = -inf
//        all tile-major with an R-row interleave (R = 4 for f32/f64, 8 for f16): element (k, i) at
//            (i/16) * nrows*16  +  ((k/R)*16 + i%16) * R  +  k%R          (tab_index<R> below)
//        nrows = roundup(K,32).  One 16-column tile is one contiguous run (254 KB of f32 at
//        K=3965), so a workgroup streams a single linear range; a lane's 16-byte load holds 4
//        consecutive source rows of ONE destination column, so it feeds one running argmax.
//        Pad rows / pad columns hold -inf: no bounds checks in the sweep (-inf never wins).
//   LB32T[M][K] float  (float)log((double)B[i][o])   (transposed: one contiguous row per symbol)
//   LB64T[M][K] double log((double)B[i][o]),  LPi64[K] double log((double)Pi[i])
//
// The trellis cell, reference src/FLASH_Viterbi_multithread.c:167-173 (== :233-239):
//     tmp = (float)log(B[i][o]);  s = tmp + T1[cur][k]  (float add)
//     ktmp = (float)((double)s + log((double)A[k][i]))   (double add, one rounding)
//     if (ktmp > score) { arg = k; score = ktmp; }        from score = -FLT_MAX, arg = -1
#pragma once

#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>
#include <cstdint>
#include <type_traits>

#include "fv_device_common.h"

// FV_OPT_DEBUG bits that leave a part of a kernel out to time the rest (0 refine, 4 launch only, 5 no score-row
// staging, 11 no sweep, 12 no refine) change results: they exist in the timing build only (build.py, timing=True).
#ifdef FV_TIMING_BUILD
#define FV_TIMING_BIT(debug, bit) (((debug) & (bit)) != 0)
#else
#define FV_TIMING_BIT(debug, bit) false
#endif

namespace fvk {


struct TaskSlot {
    const float *t1_in;   // [nrows] scores entering the step (16-byte aligned, entries >= K are zero)
    float *t1_out;        // [nrows] scores leaving it (only entries < K are written)
    int *bp_out;          // [K] arg row of this step
    const float *tmp_row; // LB32T + ob[j]*K: (float)log B[i][ob[j]] for the symbol this step consumes
    const double *tmp64_row; // LB64T + ob[j]*K (vanilla arithmetic only)
};

// FV_OPT_ROW_CODES (trellis_step_u16 only; NULL where a row has no code row beside it): the 16-bit codes of a slot's rows,
// linear in k and relative to the maximum of their own 16-column tile, and those tile maxima.  (Beside TaskSlot, not in it:
// the arguments of the kernels that never read them stay as they are.)
struct CodeSlot {
    const unsigned short *c_in;   // [nrows] codes of t1_in (read only when StepArgs::codes bit 0 is set)
    const float *tmax_in;         // [nrows / 16]
    unsigned short *c_out;        // [nrows] codes of t1_out (written only when StepArgs::codes bit 1 is set)
    float *tmax_out;              // [nrows / 16]
};

template <int NB>
struct StepArgs {
    const void *LA;          // LA32 or LA64
    const double *LA64;      // exact table for the refine gathers
    unsigned long long *counters;   // [0] near-tie candidates, [1] lane rescans, [8] columns whose window reached the code range's end
    int K;
    int reverse;             // sweep source rows high->low (alternates per step: the rows a step touched
                             // last are the first the next step reads, so they are still in the XCD's L2)
    int debug;               // bit0: timing-only build of the tail (skip the float64 refine)
    float window;            // 2*max|Lq - L| of the streamed table (0 for f32: covered by the ulp term)
    float qscale;            // q16 table: -step (value = code * qscale)
    int vanilla;             // float64 kernel only: the baseline's rounding order (vanilla Viterbi.c:140)
    int nrows;               // roundup(K, 16): rows swept
    int ntiles;              // ceil(K / TILE_W)
    int tiles_per_xcd;       // ceil(ntiles / 8)
    int nb;                  // active slots, 1..NB
    // trellis_step only — a model whose score row does not fit LDS is swept in SLABS of source rows, one launch per slab
    // (fv_full.hip, launch_step_nb): rows [row_lo, row_lo + srows) of every tile; merge != 0: t1_out / bp_out already hold the
    // result of the slabs below row_lo, which stands unless a row of this slab is strictly greater (strict '>', ascending k).
    // Every launch leaves the EXACT best of its rows (the filter kernels refine inside the slab), so the merge is exact.
    int row_lo, srows, merge;
    // trellis_step_u16 only — FV_OPT_ROW_CODES.  bit 0: every slot's incoming row has its codes beside it (c_in / tmax_in):
    // the prologue copies them instead of quantising the float row.  bit 1: write the codes of the outgoing rows.
    int codes;
    TaskSlot t[NB];
    CodeSlot c[NB];
};


// Threshold of the filter kernels.  The streamed value of a cell is y = fl(T1[k] + Lq) (one rounding),
// the exact one ktmp = fl(fl(tmp + T1[k]) + L) (two roundings); every log is <= 0, so |T1[k] + Lq| and
// |tmp + T1[k]| are <= |ktmp| (up to dmax) and each of the three roundings is at most U/2, U = the float
// spacing at the largest |ktmp| in play.  For the true winner a and the cell b holding the filter maximum M:
//     y_b - y_a <= (ktmp_b - ktmp_a) + 2*dmax + 6 * U/2 <= 2*dmax + 3U
// so every cell that can attain the exact maximum has y >= M - (window + 3U); window = 2*dmax comes from
// the host (the f32 table's own rounding, <= U/2 per entry, is one more U).  U is taken at |M + tmp| +
// window + 1 (an upper bound of |ktmp| for anything inside the window), one more U and two float steps are
// slack for the arithmetic of this function itself.
template <bool F32TAB>
__device__ __forceinline__ float filter_threshold(float M, float tmp, float window)
{
    const float z = fabsf(M + tmp) + window + 1.0f;
    const unsigned int eb = __float_as_uint(z) & 0x7f800000u;
    const float U = eb > (24u << 23) ? __uint_as_float(eb - (23u << 23)) : FLT_MIN;
    return ord2f(f2ord(M - (window + (F32TAB ? 5.0f : 4.0f) * U)) - 2);
}


// Score rows in LDS: T1s[k][NB] (task-fastest).  For NB >= 4 a row is NB/4 16-byte slots and the slot
// index is XOR-swizzled with its next three bits: without it the staging writes (lanes 4 rows = 128 B
// apart) are a 32-way bank conflict and the four row groups of a wave read the same banks (measured at
// NB = 8: 57 % of all LDS cycles were conflict cycles).
template <int NB> __device__ __forceinline__ int t1_swz(int slot) { return NB >= 4 ? (slot ^ ((slot >> 3) & 7)) : slot; }

template <int NB>
__device__ __forceinline__ float t1_at(const float *T1s, int k, int t)
{
    if constexpr (NB >= 4) return T1s[(size_t)t1_swz<NB>(k * (NB / 4) + (t >> 2)) * 4 + (t & 3)];
    else return T1s[(size_t)k * NB + t];
}

// rows base .. base+3 (base a multiple of 4) share one swizzle term: hoist it out of the row loop
template <int NB>
__device__ __forceinline__ void load_t1_row4(const float *T1s, int base, int r, float (&v)[NB])
{
    if constexpr (NB >= 4) {
        const int swz = ((base * (NB / 4)) >> 3) & 7;
#pragma unroll
        for (int q = 0; q < NB / 4; ++q) {
            float4 x = reinterpret_cast<const float4 *>(T1s)[((base + r) * (NB / 4) + q) ^ swz];
            v[4 * q] = x.x; v[4 * q + 1] = x.y; v[4 * q + 2] = x.z; v[4 * q + 3] = x.w;
        }
    } else if constexpr (NB == 2) {
        float2 x = reinterpret_cast<const float2 *>(T1s)[base + r]; v[0] = x.x; v[1] = x.y;
    } else {
        v[0] = T1s[base + r];
    }
}

template <int NB>
__device__ __forceinline__ void load_t1(const float *T1s, int k, float (&v)[NB])
{
    if constexpr (NB == 1) { v[0] = T1s[k]; }
    else if constexpr (NB == 2) { float2 x = reinterpret_cast<const float2 *>(T1s)[k]; v[0] = x.x; v[1] = x.y; }
    else {
#pragma unroll
        for (int q = 0; q < NB / 4; ++q) {
            float4 x = reinterpret_cast<const float4 *>(T1s)[t1_swz<NB>(k * (NB / 4) + q)];
            v[4 * q] = x.x; v[4 * q + 1] = x.y; v[4 * q + 2] = x.z; v[4 * q + 3] = x.w;
        }
    }
}

// Stage NB score rows (global, 16-byte aligned, nrows floats each, pads zero) into T1s: one 16-byte
// global load per task per thread, all issued before the first LDS write.
// (DEAD_TO_INF, trellis_step_csr only: a score of -FLT_MAX — a state no finite entry reached — is staged as -inf, see there)
__device__ __forceinline__ float dead_to_inf(float x) { return x > -FLT_MAX ? x : FV_NEG_INF; }

template <int NB, int NTHREADS, bool DEAD_TO_INF = false>
__device__ __forceinline__ void stage_rows(float *T1s, const TaskSlot (&slots)[NB], int nrows, int tid, int row_lo = 0)
{
    const int nq4 = nrows >> 2;
    for (int q0 = 0; q0 < nq4; q0 += NTHREADS) {
        const int q = q0 + tid;
        float4 v[NB];
#pragma unroll
        for (int t = 0; t < NB; ++t) {
            v[t] = q < nq4 ? reinterpret_cast<const float4 *>(slots[t].t1_in + row_lo)[q] : make_float4(0.f, 0.f, 0.f, 0.f);
            if constexpr (DEAD_TO_INF) v[t] = make_float4(dead_to_inf(v[t].x), dead_to_inf(v[t].y), dead_to_inf(v[t].z), dead_to_inf(v[t].w));
        }
        if (q < nq4) {
            if constexpr (NB >= 4) {
                float4 *dst = reinterpret_cast<float4 *>(T1s);
#pragma unroll
                for (int h = 0; h < NB / 4; ++h) {
                    dst[t1_swz<NB>((4 * q + 0) * (NB / 4) + h)] = make_float4(v[4 * h].x, v[4 * h + 1].x, v[4 * h + 2].x, v[4 * h + 3].x);
                    dst[t1_swz<NB>((4 * q + 1) * (NB / 4) + h)] = make_float4(v[4 * h].y, v[4 * h + 1].y, v[4 * h + 2].y, v[4 * h + 3].y);
                    dst[t1_swz<NB>((4 * q + 2) * (NB / 4) + h)] = make_float4(v[4 * h].z, v[4 * h + 1].z, v[4 * h + 2].z, v[4 * h + 3].z);
                    dst[t1_swz<NB>((4 * q + 3) * (NB / 4) + h)] = make_float4(v[4 * h].w, v[4 * h + 1].w, v[4 * h + 2].w, v[4 * h + 3].w);
                }
            } else {
                float *dst = T1s + (size_t)q * 4 * NB;
#pragma unroll
                for (int t = 0; t < NB; ++t) {
                    dst[0 * NB + t] = v[t].x; dst[1 * NB + t] = v[t].y;
                    dst[2 * NB + t] = v[t].z; dst[3 * NB + t] = v[t].w;
                }
            }
        }
    }
}

// Table element types.  half_t is IEEE binary16 storage (converted with v_cvt_f32_f16).
struct half_t { unsigned short bits; };
// q16_t: unsigned 16-bit fixed point, L ~ -(code * step) for codes 0..65534, code 65535 = -inf.
struct q16_t { unsigned short bits; };

template <typename TA> struct Tab;
template <> struct Tab<float>  { static constexpr int R = 4; using Vec = float4;  static constexpr bool exact = false; };
template <> struct Tab<double> { static constexpr int R = 4; using Vec = double4; static constexpr bool exact = true; };
template <> struct Tab<half_t> { static constexpr int R = 8; using Vec = uint4;   static constexpr bool exact = false; };
template <> struct Tab<q16_t>  { static constexpr int R = 8; using Vec = uint4;   static constexpr bool exact = false; };

__device__ __forceinline__ float h2f(unsigned short b) { return (float)__builtin_bit_cast(_Float16, b); }

__device__ __forceinline__ void unpack(const float4 &v, float (&a)[4]) { a[0] = v.x; a[1] = v.y; a[2] = v.z; a[3] = v.w; }
__device__ __forceinline__ void unpack(const double4 &v, double (&a)[4]) { a[0] = v.x; a[1] = v.y; a[2] = v.z; a[3] = v.w; }
__device__ __forceinline__ void unpack(const uint4 &v, float (&a)[8])
{
    a[0] = h2f((unsigned short)(v.x & 0xffffu)); a[1] = h2f((unsigned short)(v.x >> 16));
    a[2] = h2f((unsigned short)(v.y & 0xffffu)); a[3] = h2f((unsigned short)(v.y >> 16));
    a[4] = h2f((unsigned short)(v.z & 0xffffu)); a[5] = h2f((unsigned short)(v.z >> 16));
    a[6] = h2f((unsigned short)(v.w & 0xffffu)); a[7] = h2f((unsigned short)(v.w >> 16));
}
// fixed-point code -> float factor: the cell is y = fma(code, -step, s); the sentinel becomes +inf so that
// fma(+inf, -step, s) = -inf
__device__ __forceinline__ float q2f(unsigned int code) { return code == 0xffffu ? __builtin_huge_valf() : (float)code; }
__device__ __forceinline__ void unpack_q(const uint4 &v, float (&a)[8])
{
    a[0] = q2f(v.x & 0xffffu); a[1] = q2f(v.x >> 16); a[2] = q2f(v.y & 0xffffu); a[3] = q2f(v.y >> 16);
    a[4] = q2f(v.z & 0xffffu); a[5] = q2f(v.z >> 16); a[6] = q2f(v.w & 0xffffu); a[7] = q2f(v.w >> 16);
}
__device__ __forceinline__ float tab_load(const float *p) { return *p; }
__device__ __forceinline__ float tab_load(const half_t *p) { return h2f(p->bits); }
__device__ __forceinline__ float tab_load(const q16_t *p) { return q2f(p->bits); }

// The kind-2 rescan of trellis_step / trellis_step_u16.  Lane L of this wave holds two candidates of its own inside the
// window: the whole wave re-walks that lane's rows together, one row per lane, with the reference expression on the
// float64 entry of EVERY row (a superset of the candidates): one gather latency, no filter pass in front of it.  Lane L's
// rows are those of the wave's nj row blocks (w, w + NWV, ...: R rows of row group L / 16 in each); rows >= kend are
// left out.  Two rows per lane and trip, and all loads of a trip — score(k), the incoming score of row k, and the
// table entries — are requested before the first is used (the rescan is the tail of its launch: a serial loop paid
// one memory latency per 64 rows).  L64tile: the tile's float64 table (T4 layout) from the first row the kernel numbers 0;
// tmp: this lane's own log B.  Every lane returns the best (value, row) of lane L's rows.
template <int R, int NWV, typename Score>
__device__ __forceinline__ void rescan_lane_rows(const double *L64tile, int L, int nj, int kend, float tmp, Score score, float &bx, int &bk)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int cL = L & (TILE_W - 1), rgL = L >> 4;
    const float tmpL = __shfl(tmp, L);
    const int nlane_rows = nj * R;
    bx = FV_NEG_INF;
    bk = INT_MAX;
    for (int e0 = 0; e0 < nlane_rows; e0 += 128) {
        int kk[2];
        float tt[2];
        double LL[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int e = e0 + 64 * u + lane;
            const int k = (w + NWV * (e / R)) * (4 * R) + rgL * R + (e % R);
            kk[u] = (e < nlane_rows && k < kend) ? k : -1;
            const int ks = kk[u] >= 0 ? k : 0;
            tt[u] = score(ks);
            LL[u] = L64tile[(size_t)(ks >> 2) * (TILE_W * 4) + cL * 4 + (ks & 3)];
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (kk[u] >= 0) {
                const float x = exact_cell(tmpL, tt[u], LL[u]);
                if (better(x, kk[u], bx, bk)) { bx = x; bk = kk[u]; }
            }
        }
    }
    wave_argbest(bx, bk);
}

// One trellis step for up to NB independent tasks that share one sweep of the table.
//
// Work split: workgroup = TILE_W destination states x all source rows (no cross-workgroup
// reduction, one launch per step); lane = (column c, row group rg); a wave-wide 16-byte-per-lane
// load covers row block q = 4R source rows x 16 columns (R = rows per lane load: 4 for f32/f64,
// 8 for f16); wave w owns row blocks q = w, w+16, ...  The workgroup->tile map gives each XCD a
// contiguous slab of tiles (blockIdx % 8 is the XCD under round-robin dispatch: speed only).
//
// TA = double: the reference expression verbatim per cell (8 B/cell streamed).
// TA = float / half_t / q16_t ("filter + refine"): per cell y = (tmp + T1[k]) + (float)Lq (one rounding; for
//   q16_t y = fma(code, -step, tmp + T1[k])), Lq = log A rounded to the table type; the batched kernels
//   (NB >= 4, VALU-bound) leave tmp, common to a column, out of the sweep.  With every log <= 0 there is
//   no cancellation, and every k that can attain the exact maximum has y >= max(y) - (2*dmax + a few
//   float spacings) (3 steps with tmp inside, filter_threshold above without; dmax = max |Lq - L| over
//   the table, measured on the host).  Lanes keep (best, arg, second best); after the
//   sweep the candidates inside that window are re-evaluated from the float64 table with the
//   reference expression and reduced with (value desc, k asc); a lane whose second best is also
//   inside the window re-walks its own rows.  Output: the same bits as TA = double at 1/2 (f32) or
//   1/4 (f16) of the streamed bytes.
template <typename TA, int NB, int U, bool DB, int NWV = NWAVES>
__global__ __launch_bounds__(NWV * 64) void trellis_step(const StepArgs<NB> args)
{
    constexpr int R = Tab<TA>::R;
    constexpr int RBR = 4 * R;                                  // rows per row block
    constexpr bool EXACT = Tab<TA>::exact;
    // Batched filter kernels are VALU-bound: they do not carry the arg row per cell (compare + select)
    // but only which row block last raised the running maximum (one compare + select per 4R cells);
    // the few lanes that end up inside the refine window re-derive the row from that block.
    constexpr bool COARSE = !EXACT && NB >= 4;
    constexpr bool FACTOR = COARSE;                             // tmp left out of the per-cell filter value
    using Vec = typename Tab<TA>::Vec;
    using AV = typename std::conditional<EXACT, double, float>::type;

    extern __shared__ __align__(16) unsigned char smem[];
    const int nrows = args.nrows;
    // source rows this launch sweeps: all of them, or (K beyond one LDS row) the slab [row_lo, row_lo + srows); row numbers are
    // slab-local until the result is written
    const int srows = args.srows;
    const int row_lo = args.row_lo;
    float *T1s = reinterpret_cast<float *>(smem);              // [srows][NB], task-fastest
    float *redV = T1s + (size_t)srows * NB;                    // [NB][TILE_W][NWV] wave maxima of y
    float *redR = redV + NB * NWV * TILE_W;                 // [NB][TILE_W][NWV] wave-best exact value
    int *redK = reinterpret_cast<int *>(redR + NB * NWV * TILE_W);       // ... and its source row
    float *colM = reinterpret_cast<float *>(redK + NB * NWV * TILE_W);   // [NB][TILE_W]

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int c = lane & (TILE_W - 1), rg = lane >> 4;
    const int tile = (blockIdx.x & 7) * args.tiles_per_xcd + (blockIdx.x >> 3);
    if (tile >= args.ntiles) return;                          // workgroup-uniform
    const int col = tile * TILE_W + c;
    const int K = args.K;
    const bool rev = args.reverse != 0;
    const TA *tile_base = reinterpret_cast<const TA *>(args.LA) + (size_t)tile * nrows * TILE_W;
    const Vec *LAt = reinterpret_cast<const Vec *>(tile_base) + (size_t)(row_lo / RBR) * (4 * TILE_W) + rg * TILE_W + c;
    const int nq = srows / RBR;
    const int nj = nq > w ? (nq - w + NWV - 1) / NWV : 0;      // row blocks of this wave
    // sweep position p = 0..nj-1 -> j = p (forward) or nj-1-p (reverse); q = w + 16 j
    auto block_of = [&](int p) { return w + NWV * (rev ? nj - 1 - p : p); };

    // table loads do not depend on the incoming scores: get them in flight first.  DB = false: the
    // wave's whole share of the tile (nj <= U loads per lane) is requested up front and the score row
    // is staged while it streams in; DB = true: chunks of U loads, double-buffered in registers.
    Vec cur[U], nxt[DB ? U : 1];
#pragma unroll
    for (int u = 0; u < U; ++u)
        if (u < nj) cur[u] = LAt[(size_t)block_of(u) * (4 * TILE_W)];

    float tmp[NB];
    stage_rows<NB, NWV * 64>(T1s, args.t, srows, tid, row_lo);
#pragma unroll
    for (int t = 0; t < NB; ++t) tmp[t] = (t < args.nb && col < K) ? args.t[t].tmp_row[col] : 0.0f;
    // vanilla arithmetic (reference baseline, Base_line/C implementations/vanilla Viterbi.c:140):
    //   tmp2 = (float)( ((double)T1[k] + log A[k][i]) + log B[i][o] )   two double adds, one rounding
    double tmp64[NB];
#pragma unroll
    for (int t = 0; t < NB; ++t) tmp64[t] = 0.0;
    if constexpr (EXACT) {
        if (args.vanilla) {
#pragma unroll
            for (int t = 0; t < NB; ++t)
                if (t < args.nb && col < K) tmp64[t] = args.t[t].tmp64_row[col];
        }
    }
    __syncthreads();

    float m1[NB], m2[NB];
    int a1[NB];
#pragma unroll
    for (int t = 0; t < NB; ++t) { m1[t] = FV_NEG_INF; m2[t] = FV_NEG_INF; a1[t] = -1; }

    for (int p0 = 0; p0 < (DB ? nj : 1); p0 += U) {
        if constexpr (DB) {
            if (p0 + U < nj) {
#pragma unroll
                for (int u = 0; u < U; ++u)
                    if (p0 + U + u < nj) nxt[u] = LAt[(size_t)block_of(p0 + U + u) * (4 * TILE_W)];
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (p0 + u < nj) {
                const int qb = block_of(p0 + u);
                const int k0 = qb * RBR + rg * R;
                float mb[NB];
#pragma unroll
                for (int t = 0; t < NB; ++t) mb[t] = m1[t];
                AV av[R];
                if constexpr (std::is_same<TA, q16_t>::value) unpack_q(cur[u], av);
                else unpack(cur[u], av);
#pragma unroll
                for (int hh = 0; hh < R / 4; ++hh) {
                    // descending sweep of the exact kernel: rows high->low and '>=' so that the lowest k
                    // among equal values still wins; the filter kernels are order-free (ties are refined)
                    const int h = (EXACT && rev) ? R / 4 - 1 - hh : hh;
                    float tv[4][NB];
#pragma unroll
                    for (int r = 0; r < 4; ++r) load_t1_row4<NB>(T1s, k0 + 4 * h, r, tv[r]);
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr) {
                        const int r = (EXACT && rev) ? 3 - rr : rr;
                        const int k = k0 + 4 * h + r;
#pragma unroll
                        for (int t = 0; t < NB; ++t) {
                            if constexpr (EXACT) {
                                const float s = tmp[t] + tv[r][t];
                                const float y = args.vanilla ? (float)(((double)tv[r][t] + av[4 * h + r]) + tmp64[t])
                                                             : (float)((double)s + av[4 * h + r]);
                                const bool gt = rev ? (y >= m1[t]) : (y > m1[t]);
                                m1[t] = gt ? y : m1[t];
                                a1[t] = gt ? k : a1[t];
                            } else {
                                // the filter ranks the cells of one column: tmp is the same for all of them and the
                                // VALU-bound batched kernels leave it out (FACTOR; wider window, filter_threshold)
                                const float s = FACTOR ? tv[r][t] : tmp[t] + tv[r][t];
                                float y;
                                if constexpr (std::is_same<TA, q16_t>::value) y = __builtin_fmaf(av[4 * h + r], args.qscale, s);
                                else y = s + av[4 * h + r];
                                if constexpr (COARSE) {
                                    m2[t] = __builtin_amdgcn_fmed3f(y, m1[t], m2[t]);
                                    m1[t] = __builtin_amdgcn_fmed3f(y, m1[t], __builtin_huge_valf());   // max(y, m1)
                                } else {
                                    const bool gt = y > m1[t];
                                    m2[t] = __builtin_amdgcn_fmed3f(y, m1[t], m2[t]);
                                    m1[t] = gt ? y : m1[t];
                                    a1[t] = gt ? k : a1[t];
                                }
                            }
                        }
                    }
                }
                if constexpr (COARSE) {
#pragma unroll
                    for (int t = 0; t < NB; ++t) a1[t] = m1[t] > mb[t] ? qb : a1[t];
                }
            }
        }
        if constexpr (DB) {
#pragma unroll
            for (int u = 0; u < U; ++u) cur[u] = nxt[u];
        }
    }

    // ---- per-column reduction over the 64 lanes (4 row groups x 16 waves) that share a column
    float M1v[NB];
#pragma unroll
    for (int t = 0; t < NB; ++t) M1v[t] = FV_NEG_INF;
    if constexpr (!EXACT) {
#pragma unroll
        for (int t = 0; t < NB; ++t) {
            float v = m1[t];
            v = fmaxf(v, __shfl_xor(v, 16));
            v = fmaxf(v, __shfl_xor(v, 32));
            if (lane < TILE_W) redV[(t * TILE_W + c) * NWV + w] = v;
        }
        __syncthreads();
        if constexpr (NB <= 2) {
            // every lane reduces its own column's 16 wave maxima: no second barrier
#pragma unroll
            for (int t = 0; t < NB; ++t) {
                const float4 *q = reinterpret_cast<const float4 *>(redV + (t * TILE_W + c) * NWV);
                float v = FV_NEG_INF;
#pragma unroll
                for (int x = 0; x < NWV / 4; ++x) {
                    const float4 f = q[x];
                    v = fmaxf(fmaxf(v, fmaxf(f.x, f.y)), fmaxf(f.z, f.w));
                }
                M1v[t] = v;
            }
        } else {
            if (w < NB) {
                const float4 f = *reinterpret_cast<const float4 *>(redV + (w * TILE_W + c) * NWV + (rg * 4) % NWV);
                float v = fmaxf(fmaxf(f.x, f.y), fmaxf(f.z, f.w));
                v = fmaxf(v, __shfl_xor(v, 16));
                v = fmaxf(v, __shfl_xor(v, 32));
                if (lane < TILE_W) colM[w * TILE_W + c] = v;
            }
            __syncthreads();
#pragma unroll
            for (int t = 0; t < NB; ++t) M1v[t] = colM[t * TILE_W + c];
        }
    }

    // Candidates inside the window: request every task's float64 entry first (independent 8-byte
    // gathers, one HBM latency for the whole batch), evaluate afterwards.
    float rr[NB];
    int rk[NB];
    if constexpr (EXACT) {
#pragma unroll
        for (int t = 0; t < NB; ++t) {
            rr[t] = a1[t] >= 0 ? m1[t] : FV_NEG_INF;
            rk[t] = a1[t] >= 0 ? a1[t] + row_lo : INT_MAX;
        }
    } else {
        const double *L64t = args.LA64 + (size_t)tile * nrows * TILE_W + (size_t)(row_lo >> 2) * (TILE_W * 4) + c * 4;     // T4 layout of the f64 table, from the slab's first row
        double Lc[NB];
        int kind[NB];          // 0 nothing, 1 single candidate, 2 rescan, 3 timing-only
        float thr[NB];
#pragma unroll
        for (int t = 0; t < NB; ++t) {
            const float M1 = M1v[t];
            kind[t] = 0; Lc[t] = 0.0; thr[t] = FV_NEG_INF;
            // M1 <= -FLT_MAX/2: every predecessor is unreachable (-FLT_MAX / -inf), the cell stays (-FLT_MAX, -1)
            if (t < args.nb && M1 > (FACTOR ? -0.5f * FLT_MAX : FV_NEG_INF) && col < K) {
                // !FACTOR: y and ktmp share the rounding of tmp + T1[k] (refine_threshold; the f32 table's own
                // rounding, <= U/2 per entry, is inside its slack)
                thr[t] = FACTOR ? filter_threshold<std::is_same<TA, float>::value>(M1, tmp[t], args.window)
                                : refine_threshold(M1, args.window);
                if (FV_TIMING_BIT(args.debug, 1)) kind[t] = (m1[t] == M1 && a1[t] >= 0) ? 3 : 0;
                else if (m2[t] >= thr[t] && m2[t] > FV_NEG_INF) kind[t] = 2;
                else if (m1[t] >= thr[t] && a1[t] >= 0) {
                    kind[t] = 1;
                    if constexpr (!COARSE) Lc[t] = L64t[(size_t)(a1[t] >> 2) * (TILE_W * 4) + (a1[t] & 3)];
                }
            }
        }
        if constexpr (COARSE) {
            // a1 holds a row block: re-read this lane's 16 bytes of it and find the row that produced m1
            // (the same operations on the same inputs give the same float); rows descending so that the
            // lowest one is kept.  A second row with y == m1 means m2 == m1, i.e. kind 2, not this path.
            Vec ce[NB];
#pragma unroll
            for (int t = 0; t < NB; ++t)
                if (kind[t] == 1) ce[t] = LAt[(size_t)a1[t] * (4 * TILE_W)];
#pragma unroll
            for (int t = 0; t < NB; ++t) {
                if (kind[t] == 1) {
                    AV cv[R];
                    if constexpr (std::is_same<TA, q16_t>::value) unpack_q(ce[t], cv);
                    else unpack(ce[t], cv);
                    const int k0 = a1[t] * RBR + rg * R;
                    int found = k0;
#pragma unroll
                    for (int r = R - 1; r >= 0; --r) {
                        const float s = t1_at<NB>(T1s, k0 + r, t);
                        float y;
                        if constexpr (std::is_same<TA, q16_t>::value) y = __builtin_fmaf(cv[r], args.qscale, s);
                        else y = s + cv[r];
                        found = y == m1[t] ? k0 + r : found;
                    }
                    a1[t] = found;
                    Lc[t] = L64t[(size_t)(found >> 2) * (TILE_W * 4) + (found & 3)];
                }
            }
        }
#pragma unroll
        for (int t = 0; t < NB; ++t) {
            float r = FV_NEG_INF;
            int kb = INT_MAX;
            if (kind[t] == 1) {
                r = exact_cell(tmp[t], t1_at<NB>(T1s, a1[t], t), Lc[t]);
                kb = a1[t];
                if (m1[t] != M1v[t]) atomicAdd(&args.counters[CNT_REFINE_NEAR], 1ull);
            } else if (kind[t] == 3) {
                r = m1[t]; kb = a1[t];                    // timing-only build: no refine
            }
            rr[t] = r; rk[t] = kb;
        }
        // Lanes with two candidates of their own inside the window (kind 2): rescan_lane_rows over the slab's rows (scores
        // from the LDS row, every slab row real or a -inf pad).  Wave-uniform loop over the (rare) lanes that need it.
        const double *L64tile = args.LA64 + (size_t)tile * nrows * TILE_W + (size_t)(row_lo >> 2) * (TILE_W * 4);
#pragma unroll
        for (int t = 0; t < NB; ++t) {
            unsigned long long need = __ballot(kind[t] == 2);
            while (need) {
                const int L = __ffsll((long long)need) - 1;
                need &= need - 1;
                float bx;
                int bk;
                rescan_lane_rows<R, NWV>(L64tile, L, nj, srows, tmp[t], [&](int k) { return t1_at<NB>(T1s, k, t); }, bx, bk);
                if (lane == L) { rr[t] = bx; rk[t] = bk; }
                if (lane == 0) atomicAdd(&args.counters[CNT_REFINE_RESCAN], 1ull);
            }
        }
#pragma unroll
        for (int t = 0; t < NB; ++t) rk[t] = rk[t] != INT_MAX ? rk[t] + row_lo : INT_MAX;       // slab-local row -> row
    }

    // column_fold written out: the call raises trellis_step<double, 8, 2, true, 16> from 100 to 104 bytes of scratch
#pragma unroll
    for (int t = 0; t < NB; ++t) {
        float r = rr[t];
        int kb = rk[t];
        rowgroup_argbest(r, kb);
        if (lane < TILE_W) { redR[(t * TILE_W + c) * NWV + w] = r; redK[(t * TILE_W + c) * NWV + w] = kb; }
    }
    __syncthreads();
    if (w < NB && w < args.nb) {
        const float4 fv = *reinterpret_cast<const float4 *>(redR + (w * TILE_W + c) * NWV + (rg * 4) % NWV);
        const int4 fk = *reinterpret_cast<const int4 *>(redK + (w * TILE_W + c) * NWV + (rg * 4) % NWV);
        float r = fv.x;
        int kb = fk.x;
        if (better(fv.y, fk.y, r, kb)) { r = fv.y; kb = fk.y; }
        if (better(fv.z, fk.z, r, kb)) { r = fv.z; kb = fk.z; }
        if (better(fv.w, fk.w, r, kb)) { r = fv.w; kb = fk.w; }
        rowgroup_argbest(r, kb);
        if (lane < TILE_W && col < K) {
            if (args.merge) {             // the slabs below this one: their row is lower, so it stays unless beaten strictly
                const float pv = args.t[w].t1_out[col];
                const int pk = args.t[w].bp_out[col];
                if (pk >= 0 && !(r > pv)) { r = pv; kb = pk; }
            }
            // reference: score starts at -FLT_MAX with arg = -1 and only a strictly greater ktmp replaces it
            const bool any = r > -FLT_MAX;
            args.t[w].t1_out[col] = any ? r : -FLT_MAX;
            args.t[w].bp_out[col] = any ? kb : -1;
        }
    }
}

// ---------------------------------------------------------------- packed 16-bit filter kernel

// The filter kernels above are VALU-issue-bound, not memory-bound: a wave64 VALU instruction occupies its SIMD
// for 4 cycles (PMC, profiles/r02_pmc_batch.txt: the four waves of a SIMD keep its issue slot >100 % booked in
// the NB = 8 launches, 75 % at NB = 1), and the f32 filter costs fma + med3 + max per cell plus 3 instructions
// to turn each 16-bit table code into a float.  Here the filter runs in the table's own fixed point, two cells per
// instruction (VOP3P v_pk_add_u16 clamp / v_pk_max_u16 / v_pk_min_u16):
//   * the incoming score row v_k is quantised while it is staged: c_T(k) = rne((Mx - v_k) / step), Mx = the row
//     maximum (every workgroup stages the whole row, so it reduces it itself: a global atomicMax by the producing
//     kernel was tried first and cost 1-12 us per launch — 248 workgroups x 8 tasks on one cache line), the same step as the table codes
//     c_A(k, i) = rne(-log A / step); 65535 = unreachable / -inf / further than 65534 steps below Mx;
//   * per cell z = c_T + c_A (saturating): step * z = (Mx + tmp) - S + e, S = tmp + v_k + log A the real-valued
//     score, |e| <= 0.51 step + dmax; the smallest z marks the best cell;
//   * a lane's 16-byte table load holds the codes of 8 consecutive source rows of one column as 4 (even, odd) pairs,
//     the score codes sit in LDS in the same pairing, so one packed instruction advances two rows.
// Window.  ktmp = fl(fl(tmp + v_k) + L) is within U of S (two roundings, U = float spacing at the largest
// magnitude in play).  For the true winner a (or any cell tying with it) and the cell b with the smallest z:
// ktmp_a >= ktmp_b  =>  S_a >= S_b - 2U  =>  z_a <= z_b + (1.02 step + 2 dmax + 2U) / step.  Every lane whose
// smallest z is inside that window re-evaluates the cell with the reference expression from the float64 table
// (one gather, plus the float score from the row in global memory), a lane with two cells inside it re-walks its
// rows, exactly as the f32 filter kernels do.  If the column minimum sits within a window of saturation, cells
// whose sum saturated could still matter: every lane of that column re-walks its rows (rare: a column none of
// whose live predecessors lies within 65534 steps ~ max|log A| of the row maximum).
//
// FV_OPT_ROW_CODES (StepArgs::codes).  Every workgroup of a launch used to quantise the whole incoming row for itself
// (ntiles times the same work per task).  Instead the workgroup that PRODUCES a 16-column tile w of a row leaves, beside
// the floats, tmax[w] = the maximum of the tile's real columns (-FLT_MAX if none is reachable) and the codes
// p(k) = score_code(tmax[w], v_k) relative to it; the consumer takes Mx = max_w tmax[w] (the exact row maximum: the same
// bits as the fold over the floats), d_w = score_code(Mx, tmax[w]) and stages c'(k) = p(k) (+sat) d_w.
//   * Distance.  p and d_w are each one rne of a float quotient whose own arithmetic error is below 0.012 step (the
//     "0.51" above is 0.5 + that), so |step c'(k) - (Mx - v_k)| <= 1.024 step where neither saturated: twice today's term.
//     Per cell |e| <= 1.03 step + dmax, and the window grows by one rounding on each side of the comparison:
//     z_a <= z_b + (2.05 step + 2 dmax + 2U) / step.  The refine adds 3.1 code units to (2 dmax + 2U) / step where 1.02 are
//     needed; a launch on this route adds 4.2 where 2.05 are: the same slack of two units, a window 1.1 units wider, and
//     only on launches that take the route (the others keep 3.1).
//   * Saturation.  c'(k) = 65535 in three cases: v_k unreachable (never a winner, unless nothing is: then Zc = 65535 and
//     every row is walked); p(k) saturated, i.e. (tmax[w] - v_k) / step >= 65534.5; or the add did, p(k) + d_w >= 65535
//     (d_w = 65535, a tile further than the code range below Mx, included).  In the last two the unclamped code
//     rne((tmax - v_k) / step) + rne((Mx - tmax) / step) is >= 65534, it obeys the distance bound as any other, and so does
//     its unclamped sum z* >= 65534 with the table code: if such a cell can attain the exact maximum, Zc + (2.05 + ...) >=
//     z* >= 65534, and with the two units of slack thr = Zc + W >= 65535 — the guard that walks every row exactly.  The
//     guard therefore covers every cell whose code saturated, wherever it did.
//
// Second smallest.  The refine asks one thing of a lane beyond its smallest z (m1, row block a1, parity half par): does
// the lane hold a SECOND cell with z <= thr (a tie counted as two cells)?  Then its rows are re-walked (kind 2).  The sweep
// used to answer with the exact second smallest z per half, three packed instructions per pair of cells.  It now keeps, per
// half h, the smallest and second smallest BLOCK MINIMUM bm_h(j) = min of the four z of half h in row block j: four adds, a
// tree of three mins and three instructions of update per block and task.  m1p is what it was (a minimum of minima).  m2p_h
// = the second smallest of the bm_h(j), a tie between two blocks counted twice = the smallest z of half h outside the
// block a_h that gave m1p_h (a_h: the first block that reached it; a later block that ties has bm == m1p and sets m2p_h =
// m1p_h).  A second cell with z <= thr lies, relative to the smallest cell (half par, block a1),
//   * in the other half: then that half's minimum max(lo, hi) <= thr — the term m2' has always had (lo == hi included: two
//     cells tie, m2' = m1, the rows are re-walked);
//   * in the same half, another block: then m2p_par <= thr;
//   * in the same half of block a1: the only place the sweep no longer sees.  `locate` decodes exactly that block to find
//     the row, and returns the second smallest of the half's four z, equal sums counted twice, as `second`.
// With m2' = min(max(lo, hi), m2p_lo, m2p_hi) (m2p of the other half is >= its minimum: never the smaller term) the old
// m2 is min(m2', second), bit for bit: no pair of cells inside the window escapes, none is invented, and kinds, results and
// the refine_near / refine_rescan / refine_saturated counts are what they were.  Where the located block is decoded before
// the kinds are decided (SPEC below) `second` is folded into m2; elsewhere a lane first becomes a candidate from m2' and m1
// and turns into kind 2 behind `locate` if second <= thr (a candidate has m1 <= thr < 65535, so a1 is a real block).
typedef unsigned short fv_u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned int pk_adds(unsigned int a, unsigned int b)
{
    return __builtin_bit_cast(unsigned int, __builtin_elementwise_add_sat(__builtin_bit_cast(fv_u16x2, a), __builtin_bit_cast(fv_u16x2, b)));
}
__device__ __forceinline__ unsigned int pk_minu(unsigned int a, unsigned int b)
{
    return __builtin_bit_cast(unsigned int, __builtin_elementwise_min(__builtin_bit_cast(fv_u16x2, a), __builtin_bit_cast(fv_u16x2, b)));
}
__device__ __forceinline__ unsigned int pk_maxu(unsigned int a, unsigned int b)
{
    return __builtin_bit_cast(unsigned int, __builtin_elementwise_max(__builtin_bit_cast(fv_u16x2, a), __builtin_bit_cast(fv_u16x2, b)));
}

// code of one incoming score: 65535 for an unreachable state (-FLT_MAX / -inf) or a distance beyond the code range
__device__ __forceinline__ unsigned int score_code(float mx, float v, float inv_step)
{
    const float q = (mx - v) * inv_step;                   // >= 0; +inf / NaN for unreachable entries or an empty row
    return (v > -0.5f * FLT_MAX && q < 65534.5f) ? (unsigned int)__float2uint_rn(q) : 65535u;
}

// FV_OPT_ROW_CODES: every form but one has both prologues.  The 16-wave whole-tile form at eight tasks (FV_OPT_DEBUG bit 13
// only) stands at 120 of its 128 VGPRs and spills with a second prologue in it: it keeps the one it has (the host clears
// bit 0 of StepArgs::codes for it) and still writes the codes of its outgoing rows.
template <int NB, bool DB, int NWV> constexpr bool u16_takes_codes() { return !(NB == 8 && NWV == 16 && !DB); }

// CODES = false: the form for launches that neither read nor write codes (StepArgs::codes == 0: under auto every single-task
// launch) — the copying prologue and the code-writing tail are not compiled into it, StepArgs::c is never touched.
template <int NB, int U, bool DB, int NWV, bool CODES = true>
__global__ __launch_bounds__(NWV * 64) void trellis_step_u16(const StepArgs<NB> args)
{
    constexpr int R = 8, RBR = 32;
    extern __shared__ __align__(16) unsigned char smem[];
    const int nrows = args.nrows, npairs = nrows >> 1;
    unsigned int *T1c = reinterpret_cast<unsigned int *>(smem);                 // [NB][npairs] (even, odd) score codes
    unsigned int *redZ = T1c + (size_t)NB * npairs;                             // [NB][TILE_W][NWV] wave minima of z
    float *redR = reinterpret_cast<float *>(redZ + NB * NWV * TILE_W);       // [NB][TILE_W][NWV] wave-best exact value
    int *redK = reinterpret_cast<int *>(redR + NB * NWV * TILE_W);           // ... and its source row
    unsigned int *colZ = reinterpret_cast<unsigned int *>(redK + NB * NWV * TILE_W);   // [NB][TILE_W]

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int c = lane & (TILE_W - 1), rg = lane >> 4;
    const int tile = (blockIdx.x & 7) * args.tiles_per_xcd + (blockIdx.x >> 3);
    if (tile >= args.ntiles) return;                          // workgroup-uniform
    const int col = tile * TILE_W + c;
    const int K = args.K;
    const bool rev = args.reverse != 0;
    const unsigned short *tile_base = reinterpret_cast<const unsigned short *>(args.LA) + (size_t)tile * nrows * TILE_W;
    const uint4 *LAt = reinterpret_cast<const uint4 *>(tile_base) + rg * TILE_W + c;
    const int nq = nrows / RBR;
    const int nj = nq > w ? (nq - w + NWV - 1) / NWV : 0;      // row blocks of this wave
    auto block_of = [&](int p) { return w + NWV * (rev ? nj - 1 - p : p); };

    // Load order: vmcnt retires in issue order, so whatever is requested first is what can be consumed first.  The
    // incoming score rows (and their maxima) are needed before anything else can happen; the table is needed only
    // after they have been quantised and staged.  Rows first, then the table: the staging waits for the rows
    // alone and the table streams in behind it.
    float Mx[NB], tmp[NB];
    const float step = -args.qscale, inv_step = 1.0f / step;
    const int nq4 = nrows >> 2;
    // quads (4 consecutive rows) of each score row held by this thread: QPT per task cover 4096 rows, any more are
    // re-read in a loop (K > 4096)
    constexpr int QPT = 1024 / (NWV * 64);
    uint4 cur[U], nxt[DB ? U : 1];
    // the first table loads and the emission terms, requested behind a launch's row loads on either route below
    auto request_table = [&]() {
        // keep the scheduler from sinking loads next to their uses (it would, to save registers: one full memory
        // latency per task instead of one for all of them) or from hoisting the table loads above the rows
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (u < nj) cur[u] = LAt[(size_t)block_of(u) * (4 * TILE_W)];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < NB; ++t) tmp[t] = args.t[t].tmp_row[min(col, K - 1)];          // not needed before the refine; pad columns: never stored
        __builtin_amdgcn_sched_barrier(0);
    };
    // FV_OPT_ROW_CODES (workgroup-uniform): the rows came with their codes.  A thread copies chunks of 8 codes (16 bytes; chunk
    // ch lies in tile ch / 2), the first held in registers as v0 is on the other route, and every wave reads the tile maxima for
    // itself — four per lane cover 256 tiles, an index past the last tile repeats it, which a maximum does not mind.  (The
    // two routes are two whole branches, table request included: registers of the one are not live in the other.)
    const bool coded = CODES && u16_takes_codes<NB, DB, NWV>() && (args.codes & 1) != 0;
    const int nch = nrows >> 3;
    if (coded) {
        uint4 cv[NB];
        float tw[NB], tm[NB][4];
        const int ch = min(tid, nch - 1);
#pragma unroll
        for (int t = 0; t < NB; ++t) cv[t] = reinterpret_cast<const uint4 *>(args.c[t].c_in)[ch];
        auto request_maxima = [&]() {
#pragma unroll
            for (int t = 0; t < NB; ++t) {
                tw[t] = args.c[t].tmax_in[ch >> 1];
#pragma unroll
                for (int j = 0; j < 4; ++j) tm[t][j] = args.c[t].tmax_in[min(lane + 64 * j, args.ntiles - 1)];
            }
        };
        // (eight tasks: the 40 maxima are requested behind the table instead — ahead of it the 16-wave whole-tile form runs out of registers)
        if constexpr (NB < 8) request_maxima();
        request_table();
        if constexpr (NB >= 8) request_maxima();
        // the row maximum from the tile maxima, in every wave for itself: no LDS round, no barrier
#pragma unroll
        for (int t = 0; t < NB; ++t) {
            float x = fmaxf(fmaxf(tm[t][0], tm[t][1]), fmaxf(tm[t][2], tm[t][3]));
            for (int i = 256 + lane; i < args.ntiles; i += 64) x = fmaxf(x, args.c[t].tmax_in[i]);       // K > 4096 only
#pragma unroll
            for (int m = 1; m < 64; m <<= 1) x = fmaxf(x, __shfl_xor(x, m));
            Mx[t] = x;
        }
        // codes relative to the tile maximum -> relative to the row maximum: one saturating add of d_w per pair
        auto put = [&](int ch, int t, const uint4 &p, float tmax_w) {
            const unsigned int d = score_code(Mx[t], tmax_w, inv_step), dd = d | (d << 16);
            *reinterpret_cast<uint4 *>(T1c + (size_t)t * npairs + 4 * ch) = make_uint4(pk_adds(p.x, dd), pk_adds(p.y, dd), pk_adds(p.z, dd), pk_adds(p.w, dd));
        };
        if (tid < nch) {
#pragma unroll
            for (int t = 0; t < NB; ++t) put(tid, t, cv[t], tw[t]);
        }
        for (int ch = NWV * 64 + tid; ch < nch; ch += NWV * 64) {       // more rows than 8 per thread
#pragma unroll
            for (int t = 0; t < NB; ++t) put(ch, t, reinterpret_cast<const uint4 *>(args.c[t].c_in)[ch], args.c[t].tmax_in[ch >> 1]);
        }
    } else {
        float4 v0[QPT][NB];
#pragma unroll
        for (int h = 0; h < QPT; ++h) {
            const int q = min(h * (NWV * 64) + tid, nq4 - 1);
#pragma unroll
            for (int t = 0; t < NB; ++t) v0[h][t] = reinterpret_cast<const float4 *>(args.t[t].t1_in)[q];
        }
        request_table();
        // row maxima over the K real entries (pads of a score row are zero: excluded)
        float *redM = reinterpret_cast<float *>(redZ);           // [NB][NWV], free until the column reduction
        float pm[NB];
        auto fold = [&](int q, const float4 &v, float &m) {
            const int r0 = 4 * q;
            m = r0 < K ? fmaxf(m, v.x) : m;
            m = r0 + 1 < K ? fmaxf(m, v.y) : m;
            m = r0 + 2 < K ? fmaxf(m, v.z) : m;
            m = r0 + 3 < K ? fmaxf(m, v.w) : m;
        };
#pragma unroll
        for (int t = 0; t < NB; ++t) {
            pm[t] = FV_NEG_INF;
#pragma unroll
            for (int h = 0; h < QPT; ++h)
                if (h * (NWV * 64) + tid < nq4) fold(h * (NWV * 64) + tid, v0[h][t], pm[t]);
        }
        for (int q = 1024 + tid; q < nq4; q += NWV * 64) {       // K > 4096 only
#pragma unroll
            for (int t = 0; t < NB; ++t) fold(q, reinterpret_cast<const float4 *>(args.t[t].t1_in)[q], pm[t]);
        }
#pragma unroll
        for (int t = 0; t < NB; ++t) {
#pragma unroll
            for (int m = 1; m < 64; m <<= 1) pm[t] = fmaxf(pm[t], __shfl_xor(pm[t], m));
            if (lane == 0) redM[t * NWV + w] = pm[t];
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < NB; ++t) {
            float x = redM[t * NWV + (lane & (NWV - 1))];
#pragma unroll
            for (int m = 1; m < NWV; m <<= 1) x = fmaxf(x, __shfl_xor(x, m));
            Mx[t] = x;
        }
        auto put = [&](int q, int t, const float4 &v) {
            // rows >= K of a score row are zero pads: never a real predecessor (their table codes are 65535)
            uint2 wd;
            wd.x = score_code(Mx[t], v.x, inv_step) | (score_code(Mx[t], v.y, inv_step) << 16);
            wd.y = score_code(Mx[t], v.z, inv_step) | (score_code(Mx[t], v.w, inv_step) << 16);
            *reinterpret_cast<uint2 *>(T1c + (size_t)t * npairs + 2 * q) = wd;
        };
#pragma unroll
        for (int h = 0; h < QPT; ++h)
            if (h * (NWV * 64) + tid < nq4) {
#pragma unroll
                for (int t = 0; t < NB; ++t) put(h * (NWV * 64) + tid, t, v0[h][t]);
            }
        for (int q = 1024 + tid; q < nq4; q += NWV * 64) {       // K > 4096 only
#pragma unroll
            for (int t = 0; t < NB; ++t) put(q, t, reinterpret_cast<const float4 *>(args.t[t].t1_in)[q]);
        }
    }
    __syncthreads();

    unsigned int m1p[NB], m2p[NB];
    int alo[NB], ahi[NB];
#pragma unroll
    for (int t = 0; t < NB; ++t) { m1p[t] = 0xffffffffu; m2p[t] = 0xffffffffu; alo[t] = -1; ahi[t] = -1; }

    for (int p0 = 0; p0 < (FV_TIMING_BIT(args.debug, 2048) ? 0 : (DB ? nj : 1)); p0 += U) {     // FV_OPT_DEBUG bit 11: timing without the sweep
        if constexpr (DB) {
            if (p0 + U < nj) {
#pragma unroll
                for (int u = 0; u < U; ++u)
                    if (p0 + U + u < nj) nxt[u] = LAt[(size_t)block_of(p0 + U + u) * (4 * TILE_W)];
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (p0 + u < nj) {
                const int qb = block_of(p0 + u);
                const unsigned int ca[4] = { cur[u].x, cur[u].y, cur[u].z, cur[u].w };
                const int pb = qb * (RBR / 2) + rg * (R / 2);           // first (even, odd) pair of this lane's 8 rows
#pragma unroll
                for (int t = 0; t < NB; ++t) {
                    const uint4 ct4 = *reinterpret_cast<const uint4 *>(T1c + (size_t)t * npairs + pb);
                    const unsigned int ct[4] = { ct4.x, ct4.y, ct4.z, ct4.w };
                    const unsigned int old = m1p[t];
                    // the block's minimum per half, then (smallest, second smallest) over the block minima
                    const unsigned int bm = pk_minu(pk_minu(pk_adds(ca[0], ct[0]), pk_adds(ca[1], ct[1])),
                                                    pk_minu(pk_adds(ca[2], ct[2]), pk_adds(ca[3], ct[3])));
                    m2p[t] = pk_minu(m2p[t], pk_maxu(bm, m1p[t]));
                    m1p[t] = pk_minu(m1p[t], bm);
                    const unsigned int x = m1p[t] ^ old;                 // which half found a smaller z in this row block
                    alo[t] = (x & 0xffffu) ? qb : alo[t];
                    ahi[t] = (x >> 16) ? qb : ahi[t];
                }
            }
        }
        if constexpr (DB) {
#pragma unroll
            for (int u = 0; u < U; ++u) cur[u] = nxt[u];
        }
    }

    // lane summary: smallest z, the half (row parity) and row block it came from, and m2' = the second smallest z with the
    // rest of block a1's own half left out (locate adds that: see "Second smallest" above pk_adds)
    unsigned int m1[NB], m2[NB];
    int a1[NB], par[NB];
#pragma unroll
    for (int t = 0; t < NB; ++t) {
        const unsigned int lo = m1p[t] & 0xffffu, hi = m1p[t] >> 16;
        par[t] = hi < lo ? 1 : 0;                                       // lo == hi: two cells tie, m2 == m1, rows are re-walked
        m1[t] = par[t] ? hi : lo;
        a1[t] = par[t] ? ahi[t] : alo[t];
        m2[t] = min(max(lo, hi), min(m2p[t] & 0xffffu, m2p[t] >> 16));
    }

    // Single-/two-task launches with the whole tile share still in registers: every lane locates its own best cell
    // now, picking the block's codes out of the registers the sweep used (select chain over the U loads) instead of
    // re-reading them after the column reduction: one memory latency less in the refine.  (Also requesting that
    // cell's float64 entry and float score here, speculatively for all lanes, was measured: 10.7 instead of 9.0 us per
    // step — half a million scattered reads per launch cost more than the latency they hide.)
    constexpr bool SPEC = !DB && NB <= 2;
    double Lc[NB];
    float tv[NB];
    const double *L64t = args.LA64 + (size_t)tile * nrows * TILE_W + c * 4;     // T4 layout of the f64 table
    const int blk0 = nj > 0 ? block_of(0) : 0;          // a wave without row blocks (tiny K) uses block 0: always inside the tile
    // row of block blk (parity par) whose z equals m1: unique when m2 > m1.  second: the second smallest of the four z of that
    // half of the block, a tie counted twice (the pair update the sweep used to make for every cell, here for one block)
    auto locate = [&](int t, int blk, const uint4 &ce, unsigned int &second) -> int {
        const unsigned int ca[4] = { ce.x, ce.y, ce.z, ce.w };
        const uint4 ct4 = *reinterpret_cast<const uint4 *>(T1c + (size_t)t * npairs + blk * (RBR / 2) + rg * (R / 2));
        const unsigned int ct[4] = { ct4.x, ct4.y, ct4.z, ct4.w };
        const int k0 = blk * RBR + rg * R;
        int found = k0 + par[t];
        unsigned int b1 = 0xffffffffu, b2 = 0xffffffffu;
#pragma unroll
        for (int i = 3; i >= 0; --i) {
            const unsigned int z = pk_adds(ca[i], ct[i]);
            b2 = pk_minu(b2, pk_maxu(z, b1));
            b1 = pk_minu(b1, z);
            const unsigned int zh = par[t] ? (z >> 16) : (z & 0xffffu);
            found = zh == m1[t] ? k0 + 2 * i + par[t] : found;
        }
        second = par[t] ? (b2 >> 16) : (b2 & 0xffffu);
        return found;
    };
    if constexpr (SPEC) {
#pragma unroll
        for (int t = 0; t < NB; ++t) {
            const int blk = a1[t] >= 0 ? a1[t] : blk0;
            const int jj = (blk - w) / NWV;
            const int pos = rev ? nj - 1 - jj : jj;               // where the sweep met this block: cur[pos]
            uint4 ce = cur[0];
#pragma unroll
            for (int u = 1; u < U; ++u) {
                const bool hit = u == pos;
                ce.x = hit ? cur[u].x : ce.x; ce.y = hit ? cur[u].y : ce.y; ce.z = hit ? cur[u].z : ce.z; ce.w = hit ? cur[u].w : ce.w;
            }
            unsigned int second;
            const int found = locate(t, blk, ce, second);
            m2[t] = a1[t] >= 0 ? min(m2[t], second) : m2[t];      // (no block: blk0 need not be this wave's)
            a1[t] = a1[t] >= 0 ? found : -1;
        }
    }

    // ---- column minima over the 64 lanes (4 row groups x 16 waves) that share a column
    unsigned int Zc[NB];
#pragma unroll
    for (int t = 0; t < NB; ++t) {
        unsigned int v = m1[t];
        v = min(v, (unsigned int)__shfl_xor((int)v, 16));
        v = min(v, (unsigned int)__shfl_xor((int)v, 32));
        if (lane < TILE_W) redZ[(t * TILE_W + c) * NWV + w] = v;
    }
    __syncthreads();
    if constexpr (NB <= 2) {
#pragma unroll
        for (int t = 0; t < NB; ++t) {
            const uint4 *q = reinterpret_cast<const uint4 *>(redZ + (t * TILE_W + c) * NWV);
            unsigned int v = 0xffffffffu;
#pragma unroll
            for (int x = 0; x < NWV / 4; ++x) {
                const uint4 f = q[x];
                v = min(min(v, min(f.x, f.y)), min(f.z, f.w));
            }
            Zc[t] = v;
        }
    } else {
        if (w < NB) {
            const uint4 f = *reinterpret_cast<const uint4 *>(redZ + (w * TILE_W + c) * NWV + (rg * 4) % NWV);
            unsigned int v = min(min(f.x, f.y), min(f.z, f.w));
            v = min(v, (unsigned int)__shfl_xor((int)v, 16));
            v = min(v, (unsigned int)__shfl_xor((int)v, 32));
            if (lane < TILE_W) colZ[w * TILE_W + c] = v;
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < NB; ++t) Zc[t] = colZ[t * TILE_W + c];
    }

    // ---- refine: float64 gathers for the candidates inside the window (all tasks' gathers in flight together)
    float rr[NB];
    int rk[NB];
    {
        int kind[NB];          // 0 nothing, 1 single candidate, 2 re-walk this lane's rows
        unsigned int thrs[NB];
#pragma unroll
        for (int t = 0; t < NB; ++t) {
            kind[t] = 0;
            thrs[t] = 0;
            if (t < args.nb && col < K && !FV_TIMING_BIT(args.debug, 4096)) {       // FV_OPT_DEBUG bit 12: timing without the refine
                // float spacing at the largest magnitude in play: no cell that matters lies further than the code
                // range (65535 steps) below Mx + tmp
                const float zz = fabsf(Mx[t] + tmp[t]) + 65536.0f * step + 1.0f;
                const unsigned int eb = __float_as_uint(zz) & 0x7f800000u;
                const float Uf = (eb > (24u << 23) && eb < 0x7f800000u) ? __uint_as_float(eb - (23u << 23)) : (eb >= 0x7f800000u ? 0.0f : FLT_MIN);
                const float wf = (2.0f * Uf + args.window) * inv_step + (coded ? 4.2f : 3.1f);     // (two roundings per score code on the row-codes route)
                const unsigned int W = wf < 65535.0f ? (unsigned int)wf + 1u : 65535u;
                const unsigned int thr = Zc[t] + W;
                thrs[t] = thr;
                if (thr >= 65535u) {                              // saturated sums could matter: exact walk of every row
                    kind[t] = 2;
                    if (w == 0 && rg == 0) atomicAdd(&args.counters[CNT_REFINE_SATURATED], 1ull);      // statistics: columns that took this branch
                }
                else if (m2[t] <= thr) kind[t] = 2;
                else if (m1[t] <= thr && a1[t] >= 0) kind[t] = 1;
            }
        }
        if constexpr (SPEC) {
            // the rows are known already: only the candidates request their float64 entry and float score
#pragma unroll
            for (int t = 0; t < NB; ++t) {
                Lc[t] = 0.0; tv[t] = 0.0f;
                if (kind[t] == 1) {
                    Lc[t] = L64t[(size_t)(a1[t] >> 2) * (TILE_W * 4) + (a1[t] & 3)];
                    tv[t] = args.t[t].t1_in[a1[t]];
                }
            }
        } else {
            // kind 1: the one cell of row block a1 (parity par) whose z equals m1 — unique, if m2' > m1 and the block's own
            // half holds no second cell inside the window: that is known only here, where the block's codes are re-read
            // (lanes without a candidate read their first block: every load unconditional, all tasks' loads in flight
            // together); a lane that has one becomes kind 2.  Then the float64 entry and the float score of the row are
            // gathered (for a lane that just became kind 2 too: unused).
            uint4 ce[NB];
#pragma unroll
            for (int t = 0; t < NB; ++t) ce[t] = LAt[(size_t)(kind[t] == 1 ? a1[t] : blk0) * (4 * TILE_W)];
#pragma unroll
            for (int t = 0; t < NB; ++t) {
                unsigned int second;
                const int found = locate(t, kind[t] == 1 ? a1[t] : blk0, ce[t], second);
                kind[t] = (kind[t] == 1 && second <= thrs[t]) ? 2 : kind[t];
                a1[t] = found;
                Lc[t] = L64t[(size_t)(found >> 2) * (TILE_W * 4) + (found & 3)];
                tv[t] = args.t[t].t1_in[found];
            }
        }
#pragma unroll
        for (int t = 0; t < NB; ++t) {
            float r = FV_NEG_INF;
            int kb = INT_MAX;
            if (kind[t] == 1) {
                r = exact_cell(tmp[t], tv[t], Lc[t]);
                kb = a1[t];
                if (m1[t] != Zc[t]) atomicAdd(&args.counters[CNT_REFINE_NEAR], 1ull);
            }
            rr[t] = r; rk[t] = kb;
        }
        // kind 2: rescan_lane_rows over the real rows (k < K), scores from the float row in global memory
        const double *L64tile = args.LA64 + (size_t)tile * nrows * TILE_W;
#pragma unroll
        for (int t = 0; t < NB; ++t) {
            unsigned long long need = __ballot(kind[t] == 2);
            while (need) {
                const int L = __ffsll((long long)need) - 1;
                need &= need - 1;
                const float *t1g = args.t[t].t1_in;
                float bx;
                int bk;
                rescan_lane_rows<R, NWV>(L64tile, L, nj, K, tmp[t], [&](int k) { return t1g[k]; }, bx, bk);
                if (lane == L) { rr[t] = bx; rk[t] = bk; }
                if (lane == 0) atomicAdd(&args.counters[CNT_REFINE_RESCAN], 1ull);
            }
        }
    }

    float r;
    int kb;
    if (column_fold<NB, NWV>(rr, rk, redR, redK, args.nb, r, kb, lane, w, c, rg)) {
        const bool any = r > -FLT_MAX;
        if (lane < TILE_W && col < K) {
            // reference: score starts at -FLT_MAX with arg = -1 and only a strictly greater ktmp replaces it
            args.t[w].t1_out[col] = any ? r : -FLT_MAX;
            args.t[w].bp_out[col] = any ? kb : -1;
        }
        if (CODES && (args.codes & 2)) {
            // FV_OPT_ROW_CODES: the tile's maximum over its real columns and every column's code relative to it, beside the floats
            // (every lane holds its column's result after column_fold; pad columns count as unreachable)
            const float val = (col < K && any) ? r : -FLT_MAX;
            float tmx = val;
#pragma unroll
            for (int m = 1; m < TILE_W; m <<= 1) tmx = fmaxf(tmx, __shfl_xor(tmx, m));
            if (lane < TILE_W) {
                args.c[w].c_out[col] = (unsigned short)score_code(tmx, val, inv_step);
                if (lane == 0) args.c[w].tmax_out[tile] = tmx;
            }
        }
    }
}

// 16-bit table for models beyond the f32 kernels' LDS limit, built on the device from the float64 table (the host
// builds it for smaller models, together with the f32 / f16 / sparse forms): q16_range over the table, then the codes
// by the rule of fv_device_common.h (q16_step / q16_quantise).
__global__ void q16_tile_codes(const double *t4, unsigned short *q8, int K, int nrows, int ntiles,
                               const unsigned long long *lmax_bits, unsigned long long *dmax_bits)
{
    const double stepd = (double)q16_step(lmax_bits);
    const size_t n = (size_t)ntiles * nrows * TILE_W;           // one thread per (tile, row, column) of the padded table
    double dm = 0.0;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
        const int tile = (int)(e / ((size_t)nrows * TILE_W));
        const int rem = (int)(e % ((size_t)nrows * TILE_W));
        const int k = rem / TILE_W, col = tile * TILE_W + rem % TILE_W;
        unsigned short code = 0xFFFFu;
        const double l = t4[tab_index<4>(k, col, nrows)];
        if (k < K && col < K && l > -__builtin_huge_val()) code = q16_quantise(l, stepd, dm);
        q8[tab_index<8>(k, col, nrows)] = code;
    }
    q16_publish_max(dmax_bits, dm);
}

// ---------------------------------------------------------------- sparse transition table

// generate_data transition matrices are sparse random graphs (Binomial(K,p) out-edges per state,
// reference generate_data/data_script.py:11-24; p = 0.112 .. 0.253 in every reference config), i.e.
// 1-p of all log A entries are -inf.  A -inf candidate can never win (ktmp = -inf is not > -FLT_MAX,
// FLASH:171) nor change any other candidate, so only the finite entries need to be visited: the
// result is bit-identical to the dense sweep by construction.
//
// Layout ("CSC-Q16"): per 16-column tile, per column the finite entries in ascending source state k as
// 32-bit words (k << 16 | q16 code); a lane's 16-byte load holds 4 consecutive entries of ONE column;
// one wave-wide load = 4 chunks (row groups) x 16 columns = 1 KiB contiguous; columns are padded to the
// tile's longest column with (k = 0, code = 0xffff -> -inf).  K=3965, p=0.112: 7.6 MB instead of
// 31.5 MB (q16) / 62.9 MB (f32): an XCD's share (0.95 MB) stays in its 4 MiB L2 from step to step.
constexpr int SP_WAVES = 8;
constexpr int SP_BLOCK = SP_WAVES * 64;

template <int NB>
struct SparseArgs {
    const uint4 *data;        // all tiles back to back
    const int *tile_off;      // [ntiles] first uint4 of each tile
    const int *tile_nwb;      // [ntiles] wave-blocks (1 KiB) in each tile
    const double *LA64;       // dense T4 float64 table for the refine gathers
    unsigned long long *counters;
    int K, nrows, ntiles, tiles_per_xcd, nb, debug;
    float window, qscale;
    TaskSlot t[NB];
};

template <int NB>
__global__ __launch_bounds__(SP_BLOCK) void trellis_step_sparse(const SparseArgs<NB> args)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const int nrows = args.nrows;
    float *T1s = reinterpret_cast<float *>(smem);              // [nrows][NB]
    float *redV = T1s + (size_t)nrows * NB;                    // [NB][TILE_W][SP_WAVES]
    float *redR = redV + NB * SP_WAVES * TILE_W;
    int *redK = reinterpret_cast<int *>(redR + NB * SP_WAVES * TILE_W);

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int c = lane & (TILE_W - 1), rg = lane >> 4;
    const int tile = (blockIdx.x & 7) * args.tiles_per_xcd + (blockIdx.x >> 3);
    if (tile >= args.ntiles) return;
    if (FV_TIMING_BIT(args.debug, 16)) return;                              // timing experiment: launch cost only
    const int col = tile * TILE_W + c;
    const int K = args.K;
    const uint4 *base = args.data + args.tile_off[tile] + rg * TILE_W + c;
    const int nwb = args.tile_nwb[tile];
    const int nj = nwb > w ? (nwb - w + SP_WAVES - 1) / SP_WAVES : 0;     // wave-blocks of this wave
    constexpr int U = 4;
    uint4 cur[U];
#pragma unroll
    for (int u = 0; u < U; ++u)
        if (u < nj) cur[u] = base[(size_t)(w + SP_WAVES * u) * (4 * TILE_W)];

    float tmp[NB];
    if (!FV_TIMING_BIT(args.debug, 32)) stage_rows<NB, SP_BLOCK>(T1s, args.t, nrows, tid);     // bit 5: timing without the score-row staging
#pragma unroll
    for (int t = 0; t < NB; ++t) tmp[t] = (t < args.nb && col < K) ? args.t[t].tmp_row[col] : 0.0f;
    __syncthreads();

    float m1[NB], m2[NB];
    int a1[NB];
#pragma unroll
    for (int t = 0; t < NB; ++t) { m1[t] = FV_NEG_INF; m2[t] = FV_NEG_INF; a1[t] = -1; }

    auto visit = [&](unsigned int word) {
        const int k = (int)(word >> 16);
        const float qf = q2f(word & 0xffffu);
        float tv[NB];
        load_t1<NB>(T1s, k, tv);
#pragma unroll
        for (int t = 0; t < NB; ++t) {
            const float y = __builtin_fmaf(qf, args.qscale, tmp[t] + tv[t]);
            const bool gt = y > m1[t];
            m2[t] = __builtin_amdgcn_fmed3f(y, m1[t], m2[t]);
            m1[t] = gt ? y : m1[t];
            a1[t] = gt ? k : a1[t];
        }
    };
    for (int p0 = 0; p0 < nj; p0 += U) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (p0 + u < nj) {
                const uint4 e = cur[u];
                visit(e.x); visit(e.y); visit(e.z); visit(e.w);
            }
        }
        if (p0 + U < nj) {
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (p0 + U + u < nj) cur[u] = base[(size_t)(w + SP_WAVES * (p0 + U + u)) * (4 * TILE_W)];
        }
    }

    // column maxima over 4 row groups x SP_WAVES waves
    float M1v[NB];
#pragma unroll
    for (int t = 0; t < NB; ++t) {
        float v = m1[t];
        v = fmaxf(v, __shfl_xor(v, 16));
        v = fmaxf(v, __shfl_xor(v, 32));
        if (lane < TILE_W) redV[(t * TILE_W + c) * SP_WAVES + w] = v;
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < NB; ++t) {
        const float4 *q = reinterpret_cast<const float4 *>(redV + (t * TILE_W + c) * SP_WAVES);
        const float4 f0 = q[0], f1 = q[1];
        M1v[t] = fmaxf(fmaxf(fmaxf(f0.x, f0.y), fmaxf(f0.z, f0.w)), fmaxf(fmaxf(f1.x, f1.y), fmaxf(f1.z, f1.w)));
    }

    // refine: same window and same float64 re-evaluation as the dense filter kernels
    const double *L64t = args.LA64 + (size_t)tile * nrows * TILE_W + c * 4;
    float rr[NB];
    int rk[NB];
    double Lc[NB];
    int kind[NB];
    float thr[NB];
#pragma unroll
    for (int t = 0; t < NB; ++t) {
        const float M1 = M1v[t];
        kind[t] = 0; Lc[t] = 0.0; thr[t] = FV_NEG_INF;
        if (t < args.nb && M1 > FV_NEG_INF && col < K) {
            thr[t] = refine_threshold(M1, args.window);
            if (FV_TIMING_BIT(args.debug, 1)) kind[t] = (m1[t] == M1 && a1[t] >= 0) ? 3 : 0;
            else if (m2[t] >= thr[t] && m2[t] > FV_NEG_INF) kind[t] = 2;
            else if (m1[t] >= thr[t] && a1[t] >= 0) {
                kind[t] = 1;
                Lc[t] = L64t[(size_t)(a1[t] >> 2) * (TILE_W * 4) + (a1[t] & 3)];
            }
        }
    }
#pragma unroll
    for (int t = 0; t < NB; ++t) {
        float r = FV_NEG_INF;
        int kb = INT_MAX;
        if (kind[t] == 1) {
            r = exact_cell(tmp[t], t1_at<NB>(T1s, a1[t], t), Lc[t]);
            kb = a1[t];
            if (m1[t] != M1v[t]) atomicAdd(&args.counters[CNT_REFINE_NEAR], 1ull);
        } else if (kind[t] == 3) {
            r = m1[t]; kb = a1[t];
        } else if (kind[t] == 2) {
            // two candidates in this lane: it owns only a handful of entries, re-walk them (ascending k)
            for (int j0 = 0; j0 < nj; j0 += 4) {         // four vectors requested before the first is used
                uint4 ev[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) ev[u] = base[(size_t)(w + SP_WAVES * min(j0 + u, nj - 1)) * (4 * TILE_W)];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                if (j0 + u >= nj) break;
                const uint4 e = ev[u];
                const unsigned int words[4] = { e.x, e.y, e.z, e.w };
                for (int q = 0; q < 4; ++q) {
                    const int k = (int)(words[q] >> 16);
                    const float qf = q2f(words[q] & 0xffffu);
                    const float t1 = t1_at<NB>(T1s, k, t);
                    const float y = __builtin_fmaf(qf, args.qscale, tmp[t] + t1);
                    if (y >= thr[t] && y > FV_NEG_INF) {
                        const float x = exact_cell(tmp[t], t1, L64t[(size_t)(k >> 2) * (TILE_W * 4) + (k & 3)]);
                        if (better(x, k, r, kb)) { r = x; kb = k; }
                    }
                }
                }
            }
            atomicAdd(&args.counters[CNT_REFINE_RESCAN], 1ull);
        }
        rr[t] = r; rk[t] = kb;
    }
    float r;
    int kb;
    if (column_fold<NB, SP_WAVES>(rr, rk, redR, redK, args.nb, r, kb, lane, w, c, rg)) {
        if (lane < TILE_W && col < K) {
            const bool any = r > -FLT_MAX;
            args.t[w].t1_out[col] = any ? r : -FLT_MAX;
            args.t[w].bp_out[col] = any ? kb : -1;
        }
    }
}

template <int NB>
static inline size_t sparse_lds_bytes(int nrows)
{
    return (size_t)nrows * NB * 4 + (size_t)NB * SP_WAVES * TILE_W * 12;
}

// ---------------------------------------------------------------- models set in CSR form (fv_set_model_sparse)
//
// The same walk over the stored finite entries as trellis_step_sparse, for a model that never had a dense table.
// Layout ("CSC-32"): 16-column tiles, per column the stored finite entries in ascending source state, 4 entries of
// ONE column per lane load, one wave-wide load = 4 chunks (row groups) x 16 columns, columns padded to the tile's
// longest column rounded up to a wave-block (16 entries) — three arrays addressed by the same vector index v:
//     ck[v]  uint4  the 4 source states (32 bit each; pad: 0)
//     cq[v]  uint2  their 4 Q16 codes (pad: 0xffff = -inf)
//     c64[4 * v + q] double  log A of entry q (pad: -inf) — read by the refine only, never streamed
// A step streams 6 bytes per (padded) entry.  tile_off is 64-bit: nothing here is indexed by K * K.
// MEM = false: the NB score rows are staged into LDS as trellis_step_sparse does (nrows * NB * 4 bytes).
// MEM = true: every score is read from the row in memory (a row of K = 262144 is 1 MB: it stays in the XCD's L2 for the
// whole step) — the form of every K beyond the LDS limit, and of any K under FV_OPT_DEBUG bit 31.
// Dead sources.  A state no finite entry reached carries the score -FLT_MAX (the reference's initial value).  With every
// log <= 0 (the condition of every filter kernel) its cells evaluate to exact_cell(tmp, -FLT_MAX, L) <= -FLT_MAX, which
// the strict '>' from -FLT_MAX can never take: they are read as -inf and drop out of the filter like absent entries.  It
// matters here as it does not for the dense-set walk: a right-hand pass starts from ONE state, and at tens of edges per
// state most of its first rows are dead; left at -FLT_MAX they would all lie inside each other's window (the float
// spacing at 3e38 is 2e31) and every lane would re-walk its entries in float64 (measured at K = 262144: 20 ms per launch
// instead of 0.1).
// The running argmax keeps the entry's POSITION in the lane's share of the column (ascending with k), so that the
// refine finds both the source state and the float64 log of its candidate at that position.
template <int NB>
struct CsrArgs {
    const uint4 *ck;
    const uint2 *cq;
    const double *c64;
    const long long *tile_off;   // [ntiles] first vector of each tile
    const int *tile_nwb;         // [ntiles] wave-blocks (64 vectors) in each tile
    unsigned long long *counters;
    int K, nrows, ntiles, tiles_per_xcd, nb, debug;
    float window, qscale;
    TaskSlot t[NB];
};

template <int NB, bool MEM>
__global__ __launch_bounds__(SP_BLOCK) void trellis_step_csr(const CsrArgs<NB> args)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const int nrows = args.nrows;
    float *T1s = reinterpret_cast<float *>(smem);              // [nrows][NB] (MEM: absent)
    float *redV = T1s + (MEM ? (size_t)0 : (size_t)nrows * NB);  // [NB][TILE_W][SP_WAVES]
    float *redR = redV + NB * SP_WAVES * TILE_W;
    int *redK = reinterpret_cast<int *>(redR + NB * SP_WAVES * TILE_W);

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int c = lane & (TILE_W - 1), rg = lane >> 4;
    const int tile = (blockIdx.x & 7) * args.tiles_per_xcd + (blockIdx.x >> 3);
    if (tile >= args.ntiles) return;
    const int col = tile * TILE_W + c;
    const int K = args.K;
    const size_t v0 = (size_t)args.tile_off[tile] + rg * TILE_W + c;      // this lane's vector of wave-block 0
    const uint4 *kb = args.ck + v0;
    const uint2 *qb = args.cq + v0;
    const int nwb = args.tile_nwb[tile];
    const int nj = nwb > w ? (nwb - w + SP_WAVES - 1) / SP_WAVES : 0;     // wave-blocks of this wave
    auto vec = [&](int j) { return (size_t)(w + SP_WAVES * j) * (4 * TILE_W); };
    constexpr int U = 4;
    uint4 curk[U];
    uint2 curq[U];
#pragma unroll
    for (int u = 0; u < U; ++u)
        if (u < nj) { curk[u] = kb[vec(u)]; curq[u] = qb[vec(u)]; }

    float tmp[NB];
    if constexpr (!MEM) stage_rows<NB, SP_BLOCK, true>(T1s, args.t, nrows, tid);
#pragma unroll
    for (int t = 0; t < NB; ++t) tmp[t] = (t < args.nb && col < K) ? args.t[t].tmp_row[col] : 0.0f;
    __syncthreads();

    auto scores = [&](int k, float (&tv)[NB]) {
        if constexpr (MEM) {
#pragma unroll
            for (int t = 0; t < NB; ++t) tv[t] = dead_to_inf(args.t[t].t1_in[k]);
        } else {
            load_t1<NB>(T1s, k, tv);
        }
    };
    auto score1 = [&](int k, int t) -> float {
        if constexpr (MEM) return dead_to_inf(args.t[t].t1_in[k]);
        else return t1_at<NB>(T1s, k, t);
    };

    float m1[NB], m2[NB];
    int e1[NB];                      // position of the lane's best entry: 4 * (its wave-block j) + q
#pragma unroll
    for (int t = 0; t < NB; ++t) { m1[t] = FV_NEG_INF; m2[t] = FV_NEG_INF; e1[t] = -1; }

    auto visit = [&](unsigned int k, unsigned int code, int id) {
        const float qf = q2f(code);
        float tv[NB];
        scores((int)k, tv);
#pragma unroll
        for (int t = 0; t < NB; ++t) {
            const float y = __builtin_fmaf(qf, args.qscale, tmp[t] + tv[t]);
            const bool gt = y > m1[t];
            m2[t] = __builtin_amdgcn_fmed3f(y, m1[t], m2[t]);
            m1[t] = gt ? y : m1[t];
            e1[t] = gt ? id : e1[t];
        }
    };
    for (int p0 = 0; p0 < nj; p0 += U) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (p0 + u < nj) {
                const uint4 k4 = curk[u];
                const uint2 q2 = curq[u];
                const int id = 4 * (p0 + u);
                visit(k4.x, q2.x & 0xffffu, id); visit(k4.y, q2.x >> 16, id + 1);
                visit(k4.z, q2.y & 0xffffu, id + 2); visit(k4.w, q2.y >> 16, id + 3);
            }
        }
        if (p0 + U < nj) {
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (p0 + U + u < nj) { curk[u] = kb[vec(p0 + U + u)]; curq[u] = qb[vec(p0 + U + u)]; }
        }
    }

    // column maxima over 4 row groups x SP_WAVES waves
    float M1v[NB];
#pragma unroll
    for (int t = 0; t < NB; ++t) {
        float v = m1[t];
        v = fmaxf(v, __shfl_xor(v, 16));
        v = fmaxf(v, __shfl_xor(v, 32));
        if (lane < TILE_W) redV[(t * TILE_W + c) * SP_WAVES + w] = v;
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < NB; ++t) {
        const float4 *q = reinterpret_cast<const float4 *>(redV + (t * TILE_W + c) * SP_WAVES);
        const float4 f0 = q[0], f1 = q[1];
        M1v[t] = fmaxf(fmaxf(fmaxf(f0.x, f0.y), fmaxf(f0.z, f0.w)), fmaxf(fmaxf(f1.x, f1.y), fmaxf(f1.z, f1.w)));
    }

    // refine: the window and the float64 re-evaluation of the other filter kernels; source state and float64 log of a
    // candidate are read at its position in the table
    const unsigned int *kw = reinterpret_cast<const unsigned int *>(args.ck);
    float rr[NB];
    int rk[NB];
#pragma unroll
    for (int t = 0; t < NB; ++t) {
        const float M1 = M1v[t];
        float r = FV_NEG_INF;
        int kbest = INT_MAX;
        if (t < args.nb && M1 > FV_NEG_INF && col < K) {
            const float thr = refine_threshold(M1, args.window);
            if (m2[t] >= thr && m2[t] > FV_NEG_INF) {
                // two candidates in this lane: it owns only a handful of entries, re-walk them (ascending k)
                for (int j = 0; j < nj; ++j) {
                    const size_t v = v0 + vec(j);
                    const uint4 k4 = args.ck[v];
                    const uint2 q2 = args.cq[v];
                    const unsigned int ks[4] = { k4.x, k4.y, k4.z, k4.w };
                    const unsigned int cs[4] = { q2.x & 0xffffu, q2.x >> 16, q2.y & 0xffffu, q2.y >> 16 };
                    for (int q = 0; q < 4; ++q) {
                        const int k = (int)ks[q];
                        const float t1 = score1(k, t);
                        const float y = __builtin_fmaf(q2f(cs[q]), args.qscale, tmp[t] + t1);
                        if (y >= thr && y > FV_NEG_INF) {
                            const float x = exact_cell(tmp[t], t1, args.c64[4 * v + q]);
                            if (better(x, k, r, kbest)) { r = x; kbest = k; }
                        }
                    }
                }
                atomicAdd(&args.counters[CNT_REFINE_RESCAN], 1ull);
            } else if (m1[t] >= thr && e1[t] >= 0) {
                const size_t pos = 4 * (v0 + vec(e1[t] >> 2)) + (e1[t] & 3);
                const int k = (int)kw[pos];
                r = exact_cell(tmp[t], score1(k, t), args.c64[pos]);
                kbest = k;
                if (m1[t] != M1) atomicAdd(&args.counters[CNT_REFINE_NEAR], 1ull);
            }
        }
        rr[t] = r; rk[t] = kbest;
    }
    float r;
    int kbest;
    if (column_fold<NB, SP_WAVES>(rr, rk, redR, redK, args.nb, r, kbest, lane, w, c, rg)) {
        if (lane < TILE_W && col < K) {
            const bool any = r > -FLT_MAX;
            args.t[w].t1_out[col] = any ? r : -FLT_MAX;
            args.t[w].bp_out[col] = any ? kbest : -1;
        }
    }
}

template <int NB>
static inline size_t csr_lds_bytes(int nrows, bool mem)
{
    return (mem ? (size_t)0 : (size_t)nrows * NB * 4) + (size_t)NB * SP_WAVES * TILE_W * 12;
}

// The float64 walk over the same CSC-32 table (FV_KERNEL_CSR_F64): every stored entry is evaluated with the reference
// expression from its float64 log — what trellis_step<double, ...> does for every cell of a dense table, the absent
// entries being that table's -inf cells, which a strict '>' never takes.  No filter, no window, no refine, and so no
// condition on the sign of a log or of an emission score: the walk of a model with entries above 1 and of staged scores
// above 0.  It streams ck (16 B per 4 entries) and c64 (32 B per 4 entries: two 16-byte loads per lane) — 12 B per
// padded entry — and never reads cq.
// A lane's entries ascend in k with its position (chunk 4 * wave-block + rg of its column), so the strict '>' within the
// lane and `better` across lanes, waves and the workgroup give the reference's lowest-k winner.  Pads hold k = 0 and a
// log of -inf: -inf never wins.
// Dead sources are NOT read as -inf here: with a log or a score above 0 a source at -FLT_MAX can yield a cell above
// -FLT_MAX, which the dense float64 kernel takes.
// args.vanilla (uniform per launch): the baseline's rounding order, (float)(((double)T1[k] + log A) + log B), as
// trellis_step<double, ...> carries it.
template <int NB>
struct CsrF64Args {
    const uint4 *ck;
    const double *c64;
    const long long *tile_off;   // [ntiles] first vector of each tile
    const int *tile_nwb;         // [ntiles] wave-blocks (64 vectors) in each tile
    int K, nrows, ntiles, tiles_per_xcd, nb, vanilla;
    TaskSlot t[NB];
};

template <int NB, bool MEM>
__global__ __launch_bounds__(SP_BLOCK) void trellis_step_csr_f64(const CsrF64Args<NB> args)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const int nrows = args.nrows;
    float *T1s = reinterpret_cast<float *>(smem);              // [nrows][NB] (MEM: absent)
    float *redR = T1s + (MEM ? (size_t)0 : (size_t)nrows * NB);  // [NB][TILE_W][SP_WAVES]
    int *redK = reinterpret_cast<int *>(redR + NB * SP_WAVES * TILE_W);

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int c = lane & (TILE_W - 1), rg = lane >> 4;
    const int tile = (blockIdx.x & 7) * args.tiles_per_xcd + (blockIdx.x >> 3);
    if (tile >= args.ntiles) return;                          // workgroup-uniform
    const int col = tile * TILE_W + c;
    const int K = args.K;
    const size_t v0 = (size_t)args.tile_off[tile] + rg * TILE_W + c;      // this lane's vector of wave-block 0
    const uint4 *kb = args.ck + v0;
    const double2 *lb = reinterpret_cast<const double2 *>(args.c64) + 2 * v0;
    const int nwb = args.tile_nwb[tile];
    const int nj = nwb > w ? (nwb - w + SP_WAVES - 1) / SP_WAVES : 0;     // wave-blocks of this wave
    auto vec = [&](int j) { return (size_t)(w + SP_WAVES * j) * (4 * TILE_W); };
    constexpr int U = 4;
    uint4 curk[U];
    double2 curl[U][2];
#pragma unroll
    for (int u = 0; u < U; ++u)
        if (u < nj) { curk[u] = kb[vec(u)]; curl[u][0] = lb[2 * vec(u)]; curl[u][1] = lb[2 * vec(u) + 1]; }

    const bool vanilla = args.vanilla != 0;
    float tmp[NB];
    double tmp64[NB];
    if constexpr (!MEM) stage_rows<NB, SP_BLOCK>(T1s, args.t, nrows, tid);
#pragma unroll
    for (int t = 0; t < NB; ++t) {
        tmp[t] = (t < args.nb && col < K) ? args.t[t].tmp_row[col] : 0.0f;
        tmp64[t] = (vanilla && t < args.nb && col < K) ? args.t[t].tmp64_row[col] : 0.0;
    }
    __syncthreads();

    float m1[NB];
    int k1[NB];
#pragma unroll
    for (int t = 0; t < NB; ++t) { m1[t] = FV_NEG_INF; k1[t] = INT_MAX; }

    auto visit = [&](unsigned int k, double L) {
        float tv[NB];
        if constexpr (MEM) {
#pragma unroll
            for (int t = 0; t < NB; ++t) tv[t] = args.t[t].t1_in[k];
        } else {
            load_t1<NB>(T1s, (int)k, tv);
        }
#pragma unroll
        for (int t = 0; t < NB; ++t) {
            const float y = vanilla ? (float)(((double)tv[t] + L) + tmp64[t]) : exact_cell(tmp[t], tv[t], L);
            const bool gt = y > m1[t];
            m1[t] = gt ? y : m1[t];
            k1[t] = gt ? (int)k : k1[t];
        }
    };
    for (int p0 = 0; p0 < nj; p0 += U) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (p0 + u < nj) {
                const uint4 k4 = curk[u];
                visit(k4.x, curl[u][0].x); visit(k4.y, curl[u][0].y);
                visit(k4.z, curl[u][1].x); visit(k4.w, curl[u][1].y);
            }
        }
        if (p0 + U < nj) {
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (p0 + U + u < nj) {
                    curk[u] = kb[vec(p0 + U + u)];
                    curl[u][0] = lb[2 * vec(p0 + U + u)]; curl[u][1] = lb[2 * vec(p0 + U + u) + 1];
                }
        }
    }

    float r;
    int kbest;
    if (column_fold<NB, SP_WAVES>(m1, k1, redR, redK, args.nb, r, kbest, lane, w, c, rg)) {
        if (lane < TILE_W && col < K) {
            // a column no finite entry reaches: the reference's initial (-FLT_MAX, -1), as last_column_csr leaves it
            const bool any = r > -FLT_MAX;
            args.t[w].t1_out[col] = any ? r : -FLT_MAX;
            args.t[w].bp_out[col] = any ? kbest : -1;
        }
    }
}

template <int NB>
static inline size_t csr_f64_lds_bytes(int nrows, bool mem)
{
    return (mem ? (size_t)0 : (size_t)nrows * NB * 4) + (size_t)NB * SP_WAVES * TILE_W * 8;
}

// ---------------------------------------------------------------- small kernels


// Init row of each pass, reference FLASH:138-151 / :208-222:
//   T1[0][i] = (float)( log(X) + log(B[i][ob[L]]) ),  X = Pi[i] if L == 0 else A[Ans[L-1]][i]   (double add)
// A negative Ans[L-1] (beam miss, FLASH_BS only) selects the Pi row: the reference reads A[-1][i],
// which aliases Pi[i] in its VIT struct.
__global__ void init_rows(const PassChunk ch, const double *LA64, int nrows, const double *LB64T,
                          const double *LPi64, const int *ob, const int *ans, float *rows, int K,
                          unsigned short *codes, float *tmax, float inv_step)
{
    const PassDesc p = ch.p[blockIdx.y];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    float v = FV_NEG_INF;
    if (i < K) {
        int st = p.from_pi ? -1 : ans[p.L - 1];
        const double x = st < 0 ? LPi64[i] : LA64[tab_index<4>(st, i, nrows)];
        v = (float)(x + LB64T[(size_t)ob[p.L] * K + i]);
        rows[p.row_off + i] = v;
    }
    // FV_OPT_ROW_CODES (codes != NULL): the row's 16-bit codes per 16-column tile and the tile maxima, as trellis_step_u16
    // leaves them beside every row it writes (16 consecutive lanes hold a tile; its pad columns count as unreachable)
    if (codes) {
        float tmx = v;
#pragma unroll
        for (int m = 1; m < TILE_W; m <<= 1) tmx = fmaxf(tmx, __shfl_xor(tmx, m));
        if (i < (K + TILE_W - 1) / TILE_W * TILE_W) {
            codes[p.row_off + i] = (unsigned short)score_code(tmx, v, inv_step);
            if ((i & (TILE_W - 1)) == 0) tmax[(p.row_off + i) / TILE_W] = tmx;
        }
    }
}

// End state of the whole-sequence pass, reference FLASH:186-196: ascending scan with strict '>'
// from i = 0, i.e. the lowest index among the maxima.  One workgroup of 1024 threads per row: per thread an ascending scan
// with strict '>', then the (value, lowest index) order of `better` across lanes and waves (block_argbest).
__device__ __forceinline__ void end_pick(const float *row, int K, int *ans_out, float *score_out)
{
    __shared__ float sv[16];
    __shared__ int sk[16];
    float v = FV_NEG_INF;
    int k = INT_MAX;
    for (int i = threadIdx.x; i < K; i += 1024) {
        const float x = row[i];
        if (x > v) { v = x; k = i; }
    }
    block_argbest<16>(v, k, sv, sk);
    if (threadIdx.x == 0) {
        *ans_out = k;
        *score_out = v;
    }
}

__global__ __launch_bounds__(1024) void final_argmax(const float *row, int K, int *ans_last, float *score_out)
{
    end_pick(row, K, ans_last, score_out);
}

// The same end pick for every whole-sequence pass of a batch decode's generation 0 in ONE launch (a launch costs
// 1.5-3 us; a batch has one whole pass per sequence): workgroup b takes job b — its pass's last score row — and writes
// ans[R] and score[seq].
struct ArgmaxJob { int row; int R; int seq; };          // row: index of the K-float row in units of `nrows` floats
constexpr int ARGMAX_CHUNK = 256;
struct ArgmaxArgs { const float *rows; int *ans; float *score; int K, nrows, n; ArgmaxJob j[ARGMAX_CHUNK]; };

__global__ __launch_bounds__(1024) void final_argmax_batch(const ArgmaxArgs args)
{
    if ((int)blockIdx.x >= args.n) return;             // workgroup-uniform
    const ArgmaxJob job = args.j[blockIdx.x];
    end_pick(args.rows + (size_t)job.row * args.nrows, args.K, args.ans + job.R, args.score + job.seq);
}

// Last step of a pass whose end state is already fixed (every pass except the whole-sequence one):
// the back-track only ever reads bp[R][Ans[R]], so only that one destination column is evaluated —
// K cells instead of K*K — with the reference expression from the float64 table.  One workgroup per pass.
struct ColJob { const float *t1_in; const float *tmp_row; int *bp_row; int R; };
constexpr int COL_CHUNK = 48;
struct ColArgs { const double *LA64; const int *ans; int K, nrows, n; ColJob p[COL_CHUNK]; };

// What last_column and last_column_csr do with their threads' (best, arg) — each the strict-'>' best of the thread's own
// ascending rows: the workgroup's (256 threads) lowest row among the maxima, or -1 where no row is reachable.
__device__ __forceinline__ void last_column_tail(float best, int arg, int *bp_cell)
{
    __shared__ float sv[4];
    __shared__ int sk[4];
    block_argbest<4>(best, arg, sv, sk);
    if (threadIdx.x == 0) *bp_cell = best > -FLT_MAX ? arg : -1;
}

__global__ __launch_bounds__(256) void last_column(const ColArgs args)
{
    const ColJob job = args.p[blockIdx.x];
    const int i = args.ans[job.R];
    if (i < 0 || i >= args.K) return;                  // workgroup-uniform
    const float tmp = job.tmp_row[i];
    const double *col = args.LA64 + (size_t)(i >> 4) * args.nrows * TILE_W + (i & 15) * 4;
    float best = FV_NEG_INF;
    int arg = INT_MAX;
    for (int k0 = threadIdx.x; k0 < args.K; k0 += 256 * 4) {          // four gathers in flight per thread
        float t1[4];
        double L[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = k0 + 256 * u, ks = k < args.K ? k : 0;
            t1[u] = job.t1_in[ks];
            L[u] = col[(size_t)(ks >> 2) * (TILE_W * 4) + (ks & 3)];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = k0 + 256 * u;
            if (k < args.K) {
                const float y = exact_cell(tmp, t1[u], L[u]);
                if (y > best) { best = y; arg = k; }       // k ascending per thread
            }
        }
    }
    last_column_tail(best, arg, job.bp_row + i);
}

// init_rows for a CSR-set model: row Ans[L-1] of log A is the caller's CSR row scattered into a -inf row — column i
// looks itself up in the row's ascending column list (a row holds tens of entries: a handful of probes).
__global__ void init_rows_csr(const PassChunk ch, const long long *rptr, const int *rcol, const double *rlog,
                              const double *LB64T, const double *LPi64, const int *ob, const int *ans, float *rows, int K)
{
    const PassDesc p = ch.p[blockIdx.y];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= K) return;
    const int st = p.from_pi ? -1 : ans[p.L - 1];
    double x;
    if (st < 0) {
        x = LPi64[i];
    } else {
        long long lo = rptr[st], hi = rptr[st + 1];         // first entry with column >= i
        const long long end = hi;
        while (lo < hi) {
            const long long mid = lo + (hi - lo) / 2;
            if (rcol[mid] < i) lo = mid + 1; else hi = mid;
        }
        x = (lo < end && rcol[lo] == i) ? rlog[lo] : -__builtin_huge_val();
    }
    rows[p.row_off + i] = (float)(x + LB64T[(size_t)ob[p.L] * K + i]);
}

// last_column for a CSR-set model: the one destination column is a column of the CSC-32 table (ascending source
// states, then pads of -inf), evaluated with the reference expression from its float64 logs.
struct CsrColArgs {
    const uint4 *ck; const double *c64; const long long *tile_off; const int *tile_nwb;
    const int *ans; int K, n; ColJob p[COL_CHUNK];
};

__global__ __launch_bounds__(256) void last_column_csr(const CsrColArgs args)
{
    const ColJob job = args.p[blockIdx.x];
    const int i = args.ans[job.R];
    if (i < 0 || i >= args.K) return;                  // workgroup-uniform
    const float tmp = job.tmp_row[i];
    const int tile = i >> 4, c = i & 15;
    const size_t v0 = (size_t)args.tile_off[tile] + c;
    const int nent = args.tile_nwb[tile] * 16;         // (padded) entries of the column
    const unsigned int *kw = reinterpret_cast<const unsigned int *>(args.ck);
    float best = FV_NEG_INF;
    int arg = INT_MAX;
    for (int n0 = threadIdx.x; n0 < nent; n0 += 256 * 4) {           // four gathers in flight per thread
        float t1[4];
        double L[4];
        int ks[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int n = n0 + 256 * u, ns = n < nent ? n : 0;
            const size_t pos = 4 * (v0 + (size_t)(ns >> 2) * TILE_W) + (ns & 3);
            ks[u] = (int)kw[pos];
            L[u] = args.c64[pos];
            t1[u] = job.t1_in[ks[u]];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (n0 + 256 * u < nent) {
                const float y = exact_cell(tmp, t1[u], L[u]);
                if (y > best) { best = y; arg = ks[u]; }       // k ascending per thread (pads are -inf: never taken)
            }
        }
    }
    last_column_tail(best, arg, job.bp_row + i);
}

// Back-track of each pass from its (already fixed) end state: c[j-1] = bp[j][c[j]], by the chunk walk of
// fv_device_common.h.  Writes c[L..R-1]; later generations overwrite the positions they own.
// bp is the arg row of time L + 1 (the row of time j at bp + (j - L - 1) * K); no cell of a full-state arg row is tagged.
__device__ __forceinline__ void backtrack_walk(int L, int R, const int *bp, int K, int end, int *out, unsigned long long *restarts)
{
    chunk_walk(L, R, end, out, restarts, [&](int st, int j, bool &) { return st >= 0 ? bp[(size_t)(j - L - 1) * K + st] : -1; });
}

__global__ __launch_bounds__(64) void backtrack(const PassChunk ch, const int *bp, int K, int *ans, unsigned long long *restarts)
{
    const PassDesc p = ch.p[blockIdx.x];
    backtrack_walk(p.L, p.R, bp + (size_t)(p.L + 1) * K, K, ans[p.R], ans + p.L, restarts);
}

// ---------------------------------------------------------------- flat generations (FV_OPT_FLAT_GENERATIONS)

// S = the answer array after the whole-sequence pass's back-track: the states every right-hand pass of the flat set is
// conditioned on.  poison >= 0 (fv_test_flat_poison): S[poison] is replaced by another state.
__global__ void flat_snapshot(const int *ans, int *S, int T, int poison, int K)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= T) return;
    const int s = ans[i];
    S[i] = i == poison ? (s + 1) % K : s;
}

// The back-track of every pass of the flat set in one launch, a wave each: arg rows at the pass's private rows (or, for a
// generation-1 pass, at its own times of the by-time array), end state from S, chain into the pass's slot.
__global__ __launch_bounds__(64) void backtrack_flat(const FlatDesc *desc, const int *bp, const int *flat_bp, int K, const int *S, int *chains,
                                                      unsigned long long *restarts)
{
    const FlatDesc p = desc[blockIdx.x];
    const int *rows = p.arg_row < 0 ? bp + (size_t)(p.L + 1) * K : flat_bp + (size_t)p.arg_row * K;
    backtrack_walk(p.L, p.R, rows, K, S[p.R], chains + p.chain, restarts);
}

// The resolver, one workgroup.  Generation by generation: a pass ran from S[L-1] and S[R]; the generation-by-generation
// decode would have run it from the answers the generations before it left there.  While the two agree for every pass of
// a generation, its chains are what that decode produces and are committed to ans[L..R-1].  At the first generation where
// a pass disagrees nothing more is committed: counter = generation << 32 | disagreeing passes, and ans is exact through
// the generation before.
__global__ __launch_bounds__(1024) void flat_resolve(const FlatDesc *desc, const FlatGens gens, const int *S, const int *chains, int *ans,
                                                     unsigned long long *counter)
{
    __shared__ int miss;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    for (int g = 0; g < gens.ngen; ++g) {
        const int b0 = gens.begin[g], b1 = gens.begin[g + 1];
        if (threadIdx.x == 0) miss = 0;
        __syncthreads();
        int m = 0;
        for (int i = b0 + threadIdx.x; i < b1; i += blockDim.x) {
            const FlatDesc p = desc[i];
            if ((p.L > 0 && S[p.L - 1] != ans[p.L - 1]) || S[p.R] != ans[p.R]) ++m;
        }
        if (m) atomicAdd(&miss, m);
        __syncthreads();
        if (miss) {                                      // workgroup-uniform
            if (threadIdx.x == 0) *counter = ((unsigned long long)(g + 1) << 32) | (unsigned int)miss;
            return;
        }
        if (b1 - b0 >= (int)blockDim.x) {                // many short passes: a thread each
            for (int i = b0 + threadIdx.x; i < b1; i += blockDim.x) {
                const FlatDesc p = desc[i];
                for (int j = p.L; j < p.R; ++j) ans[j] = chains[p.chain + j - p.L];
            }
        } else {                                         // few long ones: a wave each
            for (int i = b0 + wave; i < b1; i += nwaves) {
                const FlatDesc p = desc[i];
                for (int j = p.L + lane; j < p.R; j += 64) ans[j] = chains[p.chain + j - p.L];
            }
        }
        __syncthreads();                                 // the next generation's check reads these answers
    }
}

// fv_set_emissions: the caller's block of log scores (row pitch ld elements) into the two per-time tables the step
// kernels read in place of log B: E32[t][i] = (float)x, E64[t][i] = (double)x.  TIN is double, float, _Float16 (IEEE
// binary16) or bf16_bits (bfloat16); every widening to double is exact.  Workgroups stride over rows (y) and over states
// (x), lanes along the state index.  !TIED: rows of K scores, x = row[i]: coalesced loads and stores, nothing beyond
// column K - 1 of a row is read.  TIED (fv_set_emission_map): rows of P scores shared by the K states, x = row[map[i]]:
// a lane keeps its state and walks the rows, so map[i] is loaded once per state (coalesced) and every row's gather
// comes from a few KB the whole grid row shares in L2; map[i] was checked on the host; a column no state maps to is
// never read.  Elements are loaded one by one (2-byte ones need no more than their own alignment).  flags[0] collects
// FV_EMIS_BAD (1: NaN, +inf, or a finite value whose float is infinite) and FV_EMIS_POSITIVE (2: above 0); flags[1]
// the lowest t * K + i of a refused value.  One atomic pair per workgroup that saw anything, through LDS.
constexpr int EMIS_BLOCK = 256;
struct bf16_bits { unsigned short u; };
__device__ inline double emis_widen(double x) { return x; }
__device__ inline double emis_widen(float x) { return (double)x; }
__device__ inline double emis_widen(_Float16 x) { return (double)x; }
__device__ inline double emis_widen(bf16_bits x) { return (double)__uint_as_float((unsigned int)x.u << 16); }
// one cell: the two stores and the value rules
__device__ inline void emis_cell(double x, size_t e, float *E32, double *E64, unsigned int &f, unsigned long long &bad)
{
    const float xf = (float)x;
    // accepted: -inf and every value whose float is finite (NaN fails both comparisons)
    const bool ok = xf < HUGE_VALF && (xf > -HUGE_VALF || x == -HUGE_VAL);
    if (!ok) { f |= 1u; bad = min(bad, (unsigned long long)e); }
    if (x > 0.0) f |= 2u;
    E32[e] = xf;
    E64[e] = x;
}
template <typename TIN, bool TIED>
__global__ __launch_bounds__(EMIS_BLOCK) void stage_emissions(const TIN *src, long long ld, int T, int K, const int *map,
                                                              float *E32, double *E64, unsigned long long *flags)
{
    __shared__ unsigned int s_flags;
    __shared__ unsigned long long s_bad;
    if (threadIdx.x == 0) { s_flags = 0u; s_bad = ~0ull; }
    __syncthreads();
    unsigned int f = 0u;
    unsigned long long bad = ~0ull;
    if constexpr (TIED) {
        for (int i = blockIdx.x * EMIS_BLOCK + threadIdx.x; i < K; i += gridDim.x * EMIS_BLOCK) {
            const TIN *col = src + map[i];
            for (int t = blockIdx.y; t < T; t += gridDim.y)
                emis_cell(emis_widen(col[(size_t)t * (size_t)ld]), (size_t)t * K + i, E32, E64, f, bad);
        }
    } else {
        for (int t = blockIdx.y; t < T; t += gridDim.y) {
            const TIN *row = src + (size_t)t * (size_t)ld;
            for (int i = blockIdx.x * EMIS_BLOCK + threadIdx.x; i < K; i += gridDim.x * EMIS_BLOCK)
                emis_cell(emis_widen(row[i]), (size_t)t * K + i, E32, E64, f, bad);
        }
    }
    if (f) atomicOr(&s_flags, f);
    if (bad != ~0ull) atomicMin(&s_bad, bad);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_flags) atomicOr(&flags[0], (unsigned long long)s_flags);
        if (s_bad != ~0ull) atomicMin(&flags[1], s_bad);
    }
}

}  // namespace fvk
