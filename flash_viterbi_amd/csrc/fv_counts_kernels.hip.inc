// fv_counts_kernels.hip.inc — the Baum-Welch E-step kernels of fv_expected_counts (DESIGN.md 5.8).  Included by
// fv_sumprod.hip only, after fv_sumprod_kernels.hip.inc.  They read what fv_posteriors' two passes left for one sequence:
// alpha and beta (T x K float64), the sequence's loglik on the device, the emission rows, and the table A as float32 (SPA).
// Every output cell has one owning thread and one fixed order of additions (times ascending, then one add into the call's
// accumulator): no kernel here reduces with floating-point atomics, and a sequence's contribution to a cell is a complete
// float64 value before it meets the accumulator, so a batch is the left-to-right sum of its sequences' own results.
// A sequence whose loglik is -inf is skipped by every kernel (the host never waits to learn it).
#pragma once

namespace fvc {

constexpr int TILE = 64;                   // the xi kernel's square tile of the K x K accumulator
constexpr int XI_BLOCK = 256;              // 16 x 16 threads, 4 x 4 cells each (rows ty + 16 r, columns tx + 16 c)
constexpr int XI_TT = 16;                  // times staged in LDS per trip: 2 * 16 * 64 doubles = 16 KB
constexpr int SCALE_BLOCK = 256;
constexpr int GAMMA_BLOCK = 128;
// A time whose w_t = max_i alpha[t][i] + max_j (e[t+1][j] + beta[t+1][j]) - loglik is above this is left out of the outer
// product and added per cell in the exact form.  Below it, what the linear form P[t][i] * Q[t][j] * A[i][j] can drop or
// denormalise: a factor below 2^-1022 = e^-708.4 (P <= 1, Q <= e^w_t), hence a term below e^(-708 + 500) * 2^128 < 2^-171
// for every float32 entry; a product P * Q that underflows although neither factor did is below 2^-1022 * 2^128 = 2^-894.
constexpr double WIDE_ABOVE = 500.0;

// One workgroup per time t of one sequence (t = 0 .. T - 2).  eb(j) = e[t+1][j] + beta[t+1][j], e the row of symbol
// ob[t+1] (elb + ob * K).  Ordinary time: P[t][i] = exp(alpha[t][i] - a_t), Q[t][j] = exp(eb(j) - b_t + w_t), wide[t] = 0.
// Wide time: the logs themselves, P[t][i] = alpha[t][i] - loglik and Q[t][j] = eb(j), wide[t] = 1, one more in *nwide.
// A time with no finite alpha or no finite eb (it cannot be when loglik is finite) gives zero rows.
__global__ __launch_bounds__(SCALE_BLOCK) void counts_scale(const double *__restrict__ alpha, const double *__restrict__ beta,
                                                            const double *__restrict__ elb, const int *__restrict__ ob,
                                                            const double *loglik, int K, double *__restrict__ P, double *__restrict__ Q,
                                                            int *__restrict__ wide, unsigned long long *nwide)
{
    __shared__ double sha[SCALE_BLOCK / 64], shb[SCALE_BLOCK / 64];
    const double ll = *loglik;
    if (!(ll > -HUGE_VAL)) return;
    const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double *al = alpha + (size_t)t * K, *be = beta + (size_t)(t + 1) * K, *e = elb + (size_t)ob[t + 1] * K;
    double a = -HUGE_VAL, b = -HUGE_VAL;
    for (int k = tid; k < K; k += SCALE_BLOCK) { a = fmax(a, al[k]); b = fmax(b, e[k] + be[k]); }
    a = fvs::wave_max(a); b = fvs::wave_max(b);
    if (lane == 0) { sha[wave] = a; shb[wave] = b; }
    __syncthreads();
    a = sha[0]; b = shb[0];
    for (int w = 1; w < SCALE_BLOCK / 64; ++w) { a = fmax(a, sha[w]); b = fmax(b, shb[w]); }
    const bool live = a > -HUGE_VAL && b > -HUGE_VAL;
    const double w = live ? a + b - ll : 0.0;
    const bool is_wide = live && w > WIDE_ABOVE;
    if (tid == 0) { wide[t] = is_wide ? 1 : 0; if (is_wide) atomicAdd(nwide, 1ull); }
    double *p = P + (size_t)t * K, *q = Q + (size_t)t * K;
    for (int k = tid; k < K; k += SCALE_BLOCK) {
        const double x = e[k] + be[k];
        if (!live) { p[k] = 0.0; q[k] = 0.0; }
        else if (is_wide) { p[k] = al[k] - ll; q[k] = x; }
        else { p[k] = exp(al[k] - a); q[k] = exp(x - b + w); }
    }
}

// The xi kernel.  Workgroup (bx, by) owns cells [by * 64, +64) x [bx * 64, +64) of the accumulator; thread (ty, tx) the 16
// cells (ty + 16 r, tx + 16 c).  It sums P[t][i] * Q[t][j] over the ordinary times t = 0 .. nt - 1 in ascending order, one
// float64 fma per cell and time, the two 64-wide slices of XI_TT times at a trip through LDS; multiplies once by
// (double)A[i][j]; adds the wide times in ascending order as exp(P[t][i] + log A[i][j] + Q[t][j]) from the logs counts_scale
// left and the stored float64 table (nothing where A[i][j] == 0); and does one load-add-store into acc[i * ld + j].
__global__ __launch_bounds__(XI_BLOCK) void counts_xi(const double *__restrict__ P, const double *__restrict__ Q,
                                                      const int *__restrict__ wide, const double *loglik, int nt, int K, int nrows,
                                                      const float *__restrict__ spa, const double *__restrict__ la64,
                                                      double *__restrict__ acc, long long ld)
{
    __shared__ double sp[XI_TT][TILE], sq[XI_TT][TILE];
    __shared__ int sw[XI_TT];
    if (!(*loglik > -HUGE_VAL)) return;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int i0 = blockIdx.y * TILE, j0 = blockIdx.x * TILE;
    double c[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int s = 0; s < 4; ++s) c[r][s] = 0.0;
    bool any_wide = false;
    for (int t0 = 0; t0 < nt; t0 += XI_TT) {
        const int n = min(XI_TT, nt - t0);
        __syncthreads();
        for (int x = tid; x < XI_TT * TILE; x += XI_BLOCK) {
            const int tt = x / TILE, k = x % TILE;
            const bool on = tt < n && !wide[t0 + tt];
            sp[tt][k] = (on && i0 + k < K) ? P[(size_t)(t0 + tt) * K + i0 + k] : 0.0;
            sq[tt][k] = (on && j0 + k < K) ? Q[(size_t)(t0 + tt) * K + j0 + k] : 0.0;
        }
        if (tid < XI_TT) sw[tid] = tid < n ? wide[t0 + tid] : 0;
        __syncthreads();
#pragma unroll
        for (int tt = 0; tt < XI_TT; ++tt) {
            any_wide |= sw[tt] != 0;
            double p[4], q[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) { p[r] = sp[tt][ty + 16 * r]; q[r] = sq[tt][tx + 16 * r]; }
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int s = 0; s < 4; ++s) c[r][s] = fma(p[r], q[s], c[r][s]);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = i0 + ty + 16 * r;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int j = j0 + tx + 16 * s;
            if (i >= K || j >= K) continue;
            const size_t at = fvk::tab_index<4>(i, j, nrows);
            const float a = spa[at];
            double v = c[r][s] * (double)a;
            if (any_wide && a > 0.0f) {
                const double la = la64[at];
                for (int t = 0; t < nt; ++t)
                    if (wide[t]) v = v + exp(P[(size_t)t * K + i] + la + Q[(size_t)t * K + j]);
            }
            double *cell = acc + (size_t)i * (size_t)ld + j;
            *cell = *cell + v;
        }
    }
}

// The gamma sums of one sequence, one thread per state j, t ascending: g = exp(alpha[t][j] + beta[t][j] - loglik) in
// float64 (0 where either term is -inf).  init[j] += g_0 and occ[j] += sum_t g_t (each a complete per-sequence value,
// added once), and emit_seq[j * M + ob[t]] += g_t into the sequence's own zeroed K x M block, which counts_add then adds
// to the call's.  Any of the three may be NULL.
__global__ __launch_bounds__(GAMMA_BLOCK) void counts_gamma(const double *__restrict__ alpha, const double *__restrict__ beta,
                                                            const double *loglik, const int *__restrict__ ob, int T, int K, int M,
                                                            double *__restrict__ init, double *__restrict__ occ, double *__restrict__ emit_seq)
{
    const double ll = *loglik;
    if (!(ll > -HUGE_VAL)) return;
    const int j = blockIdx.x * GAMMA_BLOCK + threadIdx.x;
    if (j >= K) return;
    double sum = 0.0;
    for (int t = 0; t < T; ++t) {
        const double x = alpha[(size_t)t * K + j] + beta[(size_t)t * K + j];
        const double g = x > -HUGE_VAL ? exp(x - ll) : 0.0;
        sum = sum + g;
        if (t == 0 && init) init[j] = init[j] + g;
        if (emit_seq) { double *cell = emit_seq + (size_t)j * M + ob[t]; *cell = *cell + g; }
    }
    if (occ) occ[j] = occ[j] + sum;
}

// acc[k] += seq[k]: the sequence's finished emission sums into the call's
__global__ void counts_add(double *__restrict__ acc, const double *__restrict__ seq, const double *loglik, size_t n)
{
    if (!(*loglik > -HUGE_VAL)) return;
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) acc[k] = acc[k] + seq[k];
}

}  // namespace fvc
