// fv_device_common.h — device helpers shared by the full-state and the FLASH-BS kernels.
#pragma once

#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>
#include <cstdint>

#include "fv_layout.h"

#define FV_NEG_INF (-__builtin_huge_valf())

namespace fvk {

// Monotone map float -> int (and back): adjacent floats are adjacent integers.
__device__ __forceinline__ int f2ord(float f)
{
    int i = __float_as_int(f);
    return i >= 0 ? i : (int)(0x80000000u - (unsigned)i);
}
__device__ __forceinline__ float ord2f(int o)
{
    if (o < -0x7F800000) o = -0x7F800000;          // clamp at -inf
    return __int_as_float(o >= 0 ? o : (int)(0x80000000u - (unsigned)o));
}

// (value desc, index asc): the order in which the reference's ascending strict-'>' scan ranks candidates.
__device__ __forceinline__ bool better(float v1, int k1, float v2, int k2)
{
    return v1 > v2 || (v1 == v2 && k1 < k2);
}

// ---------------------------------------------------------------- arg-max folds
// One tie rule for every fold below: `better` — of equal values the lowest index stays, whichever lane, wave or LDS
// slot held it.  The folds take their partner's pair only if it is strictly better, so no order of lanes matters.

// lanes that differ in the bits M0 .. 32 of their number end up holding the best pair among them
template <int M0>
__device__ __forceinline__ void lanes_argbest(float &v, int &k)
{
#pragma unroll
    for (int m = M0; m < 64; m <<= 1) {
        const float ov = __shfl_xor(v, m);
        const int ok = __shfl_xor(k, m);
        if (better(ov, ok, v, k)) { v = ov; k = ok; }
    }
}
// all 64 lanes of a wave: every lane holds the wave's best pair
__device__ __forceinline__ void wave_argbest(float &v, int &k) { lanes_argbest<1>(v, k); }
// the four row groups of a column (lane = row group * 16 + column, fv_layout.h): each lane holds its column's best pair
__device__ __forceinline__ void rowgroup_argbest(float &v, int &k) { lanes_argbest<TILE_W>(v, k); }

// A workgroup of NW waves: lane 0 of each wave to LDS (sv / sk: NW entries), barrier, thread 0 folds the waves in
// ascending order.  The result is valid in thread 0 only.
template <int NW>
__device__ __forceinline__ void block_argbest(float &v, int &k, float *sv, int *sk)
{
    wave_argbest(v, k);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) { sv[w] = v; sk[w] = k; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int q = 1; q < NW; ++q)
            if (better(sv[q], sk[q], v, k)) { v = sv[q]; k = sk[q]; }
    }
}

// The column epilogue of a step kernel (trellis_step, _u16, _sparse, _csr, _csr_f64).  A workgroup of NWV waves holds, per
// task t and lane (column c, row group rg), the best exact (value, row) of the lane's own rows in rr[t] / rk[t]
// (nothing: -inf, INT_MAX).  Each wave folds its row groups and leaves its result in redR / redK[(t * TILE_W + c) * NWV + w];
// behind the barrier wave w < nb takes task w: a lane folds four waves' results of its column through one 16-byte load
// (the row groups share the NWV results between them: (rg * 4) % NWV), then the row groups fold again.
// Returns true in the waves that own a task, with the column's (r, k) in all four of its lanes; what is done with it —
// the slab merge, the row codes, the plain write of (any ? r : -FLT_MAX, any ? k : -1) — is the caller's.
// (lane, w, c, rg are the caller's own: derived again in here they cost five step-kernel forms two VGPRs and a wave per SIMD.)
template <int NB, int NWV>
__device__ __forceinline__ bool column_fold(const float (&rr)[NB], const int (&rk)[NB], float *redR, int *redK, int nb, float &r, int &k, int lane, int w, int c, int rg)
{
#pragma unroll
    for (int t = 0; t < NB; ++t) {
        float v = rr[t];
        int kb = rk[t];
        rowgroup_argbest(v, kb);
        if (lane < TILE_W) { redR[(t * TILE_W + c) * NWV + w] = v; redK[(t * TILE_W + c) * NWV + w] = kb; }
    }
    __syncthreads();
    if (!(w < NB && w < nb)) return false;
    const float4 fv = *reinterpret_cast<const float4 *>(redR + (w * TILE_W + c) * NWV + (rg * 4) % NWV);
    const int4 fk = *reinterpret_cast<const int4 *>(redK + (w * TILE_W + c) * NWV + (rg * 4) % NWV);
    r = fv.x;
    k = fk.x;
    if (better(fv.y, fk.y, r, k)) { r = fv.y; k = fk.y; }
    if (better(fv.z, fk.z, r, k)) { r = fv.z; k = fk.z; }
    if (better(fv.w, fk.w, r, k)) { r = fv.w; k = fk.w; }
    rowgroup_argbest(r, k);
    return true;
}

// ---------------------------------------------------------------- the chunk walk of the back-tracks
// Back-track of one pass [L, R] from its (already fixed) end state: c[j-1] = hop(c[j], j).  Equivalent to the forward
// propagation of T2 in the reference (FLASH:242, :176-179) followed by the read-off (:261, :198-201).
//
// A chain of T dependent loads is latency-bound (64 us at T = 256, 1 ms at T = 4096 for one lane).  Survivor paths
// merge within a few steps (every state's best predecessor is one of the few best-scoring states), so long chains are
// walked by 64 lanes at once: lane c walks chunk c of the time axis, starting BT_WARMUP steps above it from a guessed
// state; by the time it enters its chunk it has (almost always) merged with the true chain.  Nothing is assumed: a
// chunk's result stands only if the state it entered with equals the state the chunk above it — itself verified —
// left with (the map is deterministic: equal at one time means equal from there on); the first chunk that fails
// restarts from the verified state, and the others are walked again behind it.
//
// One wave (64 threads) per pass.  `end` is the state at time R, out[j - L] receives c[j] for j = L .. R-1, and
// hop(state, time, tag&) gives the state one step earlier (a state < 0 stays < 0) and may set `tag` for the cell it read.
// Returns, in lane 0, whether a tagged cell lay on the path: a tag counts only if it lies on a verified chunk (tags met
// in the warm-up above a chunk belong to the chunk above).  `restarts` (counter BT_COUNTER) counts the retries: one
// atomic of lane 0 per failed verification, nothing on the way of a walk whose chunks all stand.
template <typename Hop>
__device__ __forceinline__ bool chunk_walk(int L, int R, int end, int *out, unsigned long long *restarts, Hop hop)
{
    const int lane = threadIdx.x, len = R - L;
    bool met_tag = false;
    if (len < BT_MIN_PARALLEL) {
        if (lane != 0) return false;
        int st = end;
        for (int j = R; j > L; --j) { st = hop(st, j, met_tag); out[j - 1 - L] = st; }
        return met_tag;
    }
    const int cs = (len + 63) / 64;                      // times per chunk; chunk c: from time top(c) down to top(c + 1)
    auto top = [&](int c) { return max(R - c * cs, L); };
    int base = 0, exact = end;                           // chunks below `base` are final; `exact` = state at time top(base)
    while (base < 64 && top(base) > L) {                 // (wave-uniform)
        int x = -2, y = -2;                              // state this lane entered its chunk with / left it with
        bool tag = false;
        if (lane >= base && top(lane) > L) {
            const int t_hi = top(lane), t_lo = top(lane + 1);
            int t = min(top(base), t_hi + BT_WARMUP), st = exact;     // at top(base) `exact` is the true state; above the chunk it is a guess
            bool warm_tag = false;
            for (; t > t_hi; --t) st = hop(st, t, warm_tag);
            x = st;
            for (; t > t_lo; --t) { st = hop(st, t, tag); out[t - 1 - L] = st; }
            y = st;
        }
        const int y_above = __shfl_up(y, 1);
        // lanes whose walk started at top(base) started from the true state: consistent by construction
        const bool ok = lane <= base || top(lane) <= L || min(top(base), top(lane) + BT_WARMUP) == top(base) || x == y_above;
        const unsigned long long bad = ~__ballot(ok);
        const int f = bad ? __ffsll((long long)bad) - 1 : 64;        // first chunk that entered with the wrong state: base .. f - 1 are final
        met_tag |= __any(tag && lane >= base && lane < f);
        if (!bad) break;
        if (lane == 0) atomicAdd(restarts, 1ull);
        exact = __shfl(y, f - 1);
        base = f;
    }
    return met_tag;
}

// ---------------------------------------------------------------- the 16-bit table rule (device side)
// step = (float)(largest finite |log A| / 65534), code = clamp(nearbyint(-l / step), 0, 65534), 0xffff = -inf, and the
// filter window comes from the largest |-code * step - l| actually made.  The host states the same rule as Q16Rule
// (fv_model.cpp); the device builds the tables the host does not.  lmax / dmax travel as the bit patterns of
// non-negative doubles (monotone as integers), folded with atomicMax.
__device__ __forceinline__ float q16_step(const unsigned long long *lmax_bits)
{
    const double lmax = __longlong_as_double((long long)*lmax_bits);
    return lmax > 0.0 ? (float)(lmax / 65534.0) : 1.0f;
}
// code of one finite l; dmax keeps the largest distance between l and what the code stands for
__device__ __forceinline__ unsigned short q16_quantise(double l, double step, double &dmax)
{
    double c = nearbyint(-l / step);
    c = c < 0.0 ? 0.0 : (c > 65534.0 ? 65534.0 : c);
    const double d = fabs(-c * step - l);
    dmax = d > dmax ? d : dmax;
    return (unsigned short)c;
}
// a wave's maximum of m (>= 0) into *bits
__device__ __forceinline__ void q16_publish_max(unsigned long long *bits, double m)
{
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) { const double o = __shfl_xor(m, k); m = o > m ? o : m; }
    if ((threadIdx.x & 63) == 0 && m > 0.0) atomicMax(bits, (unsigned long long)__double_as_longlong(m));
}
// lmax over the n entries of a float64 log table, whatever its layout (-inf entries do not count)
static __global__ void q16_range(const double *tab, size_t n, unsigned long long *lmax_bits)
{
    double m = 0.0;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
        const double l = tab[e];
        if (l > -__builtin_huge_val() && -l > m) m = -l;
    }
    q16_publish_max(lmax_bits, m);
}

// Threshold of the filter kernels that keep tmp inside the per-cell value (NB <= 2, the sparse walk, beam_step_q16):
// y = fl(s + Lq) and ktmp = fl(s + L) share s = fl(tmp + T1[k]), so for the true winner a and the cell b holding
// the filter maximum M:  y_b - y_a <= 2*dmax + (ulp(y_a) + ulp(ktmp_a) + ulp(y_b) + ulp(ktmp_b)) / 2.  The four
// spacings are NOT all the spacing at M: when the candidates straddle a power of two (every long decode crosses
// -1024, -2048, ...) the ones on the far side have twice the spacing.  U is therefore the float spacing at an
// upper bound of every magnitude in play (|M| + window + 1): the bound is 2*dmax + 2U; half a U more covers the
// rounding of the subtraction below and one float step the rounding of window + 2.5 U.  (A wider margin is not
// free: at T = 4096, where U = 2^-8 dwarfs the table's 2*dmax, 4U + 2 steps made the whole-sequence pass 20 % slower.)
__device__ __forceinline__ float refine_threshold(float M, float window)
{
    const float z = fabsf(M) + window + 1.0f;
    const unsigned int eb = __float_as_uint(z) & 0x7f800000u;
    const float U = eb > (24u << 23) ? __uint_as_float(eb - (23u << 23)) : FLT_MIN;
    return ord2f(f2ord(M - (window + 2.5f * U)) - 1);
}

__device__ __forceinline__ float exact_cell(float tmp, float t1, double logA)
{
    float s = tmp + t1;                       // float add
    return (float)((double)s + logA);         // double add, one rounding to float
}

}  // namespace fvk
