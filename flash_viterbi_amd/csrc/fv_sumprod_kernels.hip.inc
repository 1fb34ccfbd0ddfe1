// fv_sumprod_kernels.hip.inc — the sum-product (forward-backward) kernels of fv_loglik / fv_posteriors (DESIGN.md 5.7).
// Included by fv_sumprod.hip only.  Everything is float64 but the streamed table, which holds A itself as float32 in the
// tile-major layout of LA32 (fv_layout.h, tab_index<4>), pads 0.  No kernel here reduces with floating-point atomics: every
// sum has one fixed order per task, whatever the launch form, so the same task gives the same bits in every launch.
#pragma once

namespace fvs {

constexpr int BLOCK = fvk::BLOCK, NWAVES = fvk::NWAVES, TILE_W = fvk::TILE_W;
constexpr int MAX_NB = 4;                  // tasks of one step launch (float64 rows in LDS: 32 KB each at K = 3965)
constexpr int SMALL_NB = 8;                // tasks of one init / final launch
// A column whose linear sum s falls below this is re-evaluated in the exact form.  What the linear sum can have lost: a
// p[i] below 2^-1022 (flushed to 0, or a denormal with an absolute error up to 2^-1075), times a table entry below 2^128
// (any float32), in fewer than 2^15 rows (K <= 20192): less than 2^-879 in all, which is below u * s = 2^-53 * s for
// every s >= 2^-800, whatever the model's entries.
constexpr double REFINE_BELOW = 0x1p-800;
enum : int { CNT_REFINE_COLUMNS = 0, CNT_REFINE_FINITE = 1, NCOUNTERS = 2 };

// One task of a step launch: out[j] = eout[j] + log sum_i exp(in[i] + ein[i] + log T[i][j]); ein / eout may be NULL (0).
// Forward: T = A, eout = the emission row of the time written.  Backward: T = A transposed, ein = the emission row of
// the time read.
struct StepTask { const double *in, *ein, *eout; double *out; };
template <int NB> struct StepArgs { StepTask t[NB]; };

__host__ __device__ inline size_t step_lds_doubles(int nb, int nrows) { return (size_t)nb * ((size_t)nrows + NWAVES * TILE_W + 2 * NWAVES); }

__device__ inline double wave_max(double v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}
__device__ inline double wave_sum(double v)      // butterfly: every lane ends with the same bits
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = v + __shfl_xor(v, o);
    return v;
}

__device__ inline double task_in(const StepTask &t, int k) { return t.ein ? t.in[k] + t.ein[k] : t.in[k]; }

// The sweep: one workgroup per tile of 16 destination columns, all source rows, NB tasks sharing the table's bytes.
// Prologue: m = max of the incoming row, p[i] = exp(in[i] - m) staged in LDS (K exp calls, not K * K).  Sweep: one
// convert and one float64 fma per cell.  Epilogue: out = eout + (m + log s); a column with s < 2^-800 (the terms that
// exp flushed could matter) is re-evaluated by one wave per column as max_i + log sum_i exp(. - max_i) from the same
// table's logs, and counted.
template <int NB>
__global__ __launch_bounds__(BLOCK) void sumprod_step(StepArgs<NB> a, const float *__restrict__ tab, int K, int nrows,
                                                      unsigned long long *counters)
{
    extern __shared__ double lds[];
    double *p = lds;                                          // [NB][nrows]
    double *red = p + (size_t)NB * nrows;                     // [NB][NWAVES][TILE_W]
    double *wmax = red + NB * NWAVES * TILE_W;                // [NB][NWAVES]
    int *need = reinterpret_cast<int *>(wmax + NB * NWAVES);  // [NB][TILE_W] (NB * NWAVES doubles of room)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, tile = blockIdx.x;
    const float4 *base = reinterpret_cast<const float4 *>(tab + (size_t)tile * nrows * TILE_W);
    const int nvec = nrows * (TILE_W / 4);                    // one float4: four consecutive source rows of one column

    double m[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        double mx = -HUGE_VAL;
        for (int k = tid; k < K; k += BLOCK) mx = fmax(mx, task_in(a.t[b], k));
        mx = wave_max(mx);
        if (lane == 0) wmax[b * NWAVES + wave] = mx;
    }
    if (tid < NB * TILE_W) need[tid] = 0;
    __syncthreads();
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        double mx = wmax[b * NWAVES];
        for (int w = 1; w < NWAVES; ++w) mx = fmax(mx, wmax[b * NWAVES + w]);
        m[b] = mx;
        for (int k = tid; k < nrows; k += BLOCK)
            p[(size_t)b * nrows + k] = (k < K && mx > -HUGE_VAL) ? exp(task_in(a.t[b], k) - mx) : 0.0;
    }
    __syncthreads();

    double acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] = 0.0;
    auto cell4 = [&](const float4 t4, int v) {
        const int k0 = (v >> 4) * 4;
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const double *pp = p + (size_t)b * nrows + k0;
            acc[b] = fma(pp[0], (double)t4.x, acc[b]);
            acc[b] = fma(pp[1], (double)t4.y, acc[b]);
            acc[b] = fma(pp[2], (double)t4.z, acc[b]);
            acc[b] = fma(pp[3], (double)t4.w, acc[b]);
        }
    };
#pragma unroll 4
    for (int v = tid; v < nvec; v += BLOCK) cell4(base[v], v);
    // lanes c, c + 16, c + 32, c + 48 of a wave hold the same column: fold them, then the waves in order
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        double s = acc[b] + __shfl_xor(acc[b], 16);
        s = s + __shfl_xor(s, 32);
        if (lane < TILE_W) red[(b * NWAVES + wave) * TILE_W + lane] = s;
    }
    __syncthreads();
    if (tid < NB * TILE_W) {
        const int b = tid / TILE_W, c = tid % TILE_W, col = tile * TILE_W + c;
        double s = 0.0;
        for (int w = 0; w < NWAVES; ++w) s = s + red[(b * NWAVES + w) * TILE_W + c];
        double mb = m[0];
#pragma unroll
        for (int q = 1; q < NB; ++q) if (b == q) mb = m[q];
        if (col < K) {
            const StepTask &t = a.t[b];
            if (!(mb > -HUGE_VAL)) t.out[col] = -HUGE_VAL;                    // nothing comes in: nothing to refine
            else if (s >= REFINE_BELOW) { const double r = mb + log(s); t.out[col] = t.eout ? t.eout[col] + r : r; }
            else need[tid] = 1;
        }
    }
    __syncthreads();
    // the exact column: wave c of the workgroup takes column c of every task that asked
    if (wave < TILE_W) {
        const int c = wave, col = tile * TILE_W + c;
        const float *colbase = tab + (size_t)tile * nrows * TILE_W;
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            if (!need[b * TILE_W + c]) continue;
            const StepTask &t = a.t[b];
            double mx = -HUGE_VAL;
            for (int k = lane; k < K; k += 64) {
                const float x = colbase[((size_t)(k >> 2) * TILE_W + c) * 4 + (k & 3)];
                if (x > 0.0f) mx = fmax(mx, task_in(t, k) + log((double)x));
            }
            mx = wave_max(mx);
            double r = -HUGE_VAL;
            if (mx > -HUGE_VAL) {
                double s = 0.0;
                for (int k = lane; k < K; k += 64) {
                    const float x = colbase[((size_t)(k >> 2) * TILE_W + c) * 4 + (k & 3)];
                    if (x > 0.0f) s = s + exp(task_in(t, k) + log((double)x) - mx);
                }
                s = wave_sum(s);
                r = mx + log(s);
            }
            if (lane == 0) {
                t.out[col] = (t.eout && r > -HUGE_VAL) ? t.eout[col] + r : r;
                atomicAdd(&counters[CNT_REFINE_COLUMNS], 1ull);
                if (r > -HUGE_VAL) atomicAdd(&counters[CNT_REFINE_FINITE], 1ull);
            }
        }
    }
}

// The linear table from the stored logs: (float)exp(log((double)a)) returns a's bits (the double exp is within 1e-14,
// relative, of a: far inside half a float ulp).  transpose: entry (k, col) holds A[col][k], the backward pass's table.
__global__ void sumprod_build_table(const double *__restrict__ la64, float *__restrict__ out, int K, int nrows, int ntiles, int transpose)
{
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x, tab = (size_t)ntiles * nrows * TILE_W;
    if (e >= tab) return;
    if (!transpose) { out[e] = (float)exp(la64[e]); return; }
    // invert tab_index<4>: e = tile * nrows * 16 + ((k / 4) * 16 + c) * 4 + k % 4
    const size_t in_tile = e % ((size_t)nrows * TILE_W);
    const int tile = (int)(e / ((size_t)nrows * TILE_W)), k = (int)(in_tile / (4 * TILE_W)) * 4 + (int)(in_tile & 3);
    const int col = tile * TILE_W + (int)((in_tile >> 2) & (TILE_W - 1));
    out[e] = (k < K && col < K) ? (float)exp(la64[fvk::tab_index<4>(col, k, nrows)]) : 0.0f;
}

// Init rows of up to SMALL_NB tasks (blockIdx.y): out = in + eout with in = log Pi (forward), or 0 (backward: both NULL).
__global__ void sumprod_init(StepArgs<SMALL_NB> a, int K)
{
    const StepTask &t = a.t[blockIdx.y];
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < K) t.out[j] = t.in ? t.in[j] + t.eout[j] : 0.0;
}

// log sum_j exp(in[j]) of up to SMALL_NB tasks, one workgroup each, into *out: strided partial sums, the butterfly, the
// waves in order.
__global__ __launch_bounds__(BLOCK) void sumprod_final(StepArgs<SMALL_NB> a, int K)
{
    __shared__ double sh[NWAVES];
    const StepTask &t = a.t[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double mx = -HUGE_VAL;
    for (int k = tid; k < K; k += BLOCK) mx = fmax(mx, t.in[k]);
    mx = wave_max(mx);
    if (lane == 0) sh[wave] = mx;
    __syncthreads();
    mx = sh[0];
    for (int w = 1; w < NWAVES; ++w) mx = fmax(mx, sh[w]);
    __syncthreads();
    double s = 0.0;
    if (mx > -HUGE_VAL)
        for (int k = tid; k < K; k += BLOCK) s = s + exp(t.in[k] - mx);
    s = wave_sum(s);
    if (lane == 0) sh[wave] = s;
    __syncthreads();
    if (tid == 0) {
        double tot = 0.0;
        for (int w = 0; w < NWAVES; ++w) tot = tot + sh[w];
        *t.out = mx > -HUGE_VAL ? mx + log(tot) : -HUGE_VAL;
    }
}

// gamma[t][j] = exp(alpha + beta - loglik) as float32 and path[t] = the lowest index among the maxima of alpha + beta:
// one workgroup per time.  loglik == -inf: nothing is written (the host fills the path with -1).
__global__ __launch_bounds__(BLOCK) void sumprod_gamma(const double *__restrict__ alpha, const double *__restrict__ beta,
                                                       const double *loglik, int K, float *gamma, long long ld, int *path)
{
    __shared__ double shv[NWAVES];
    __shared__ int shi[NWAVES];
    const double ll = *loglik;
    if (!(ll > -HUGE_VAL)) return;
    const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double *al = alpha + (size_t)t * K, *be = beta + (size_t)t * K;
    double best = -HUGE_VAL;
    int arg = 0x7fffffff;
    for (int j = tid; j < K; j += BLOCK) {
        const double g = al[j] + be[j];
        if (gamma) gamma[(size_t)t * (size_t)ld + j] = g > -HUGE_VAL ? (float)exp(g - ll) : 0.0f;
        if (g > best || (g == best && j < arg)) { best = g; arg = j; }
    }
    if (!path) return;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const double ob = __shfl_xor(best, o);
        const int oa = __shfl_xor(arg, o);
        if (ob > best || (ob == best && oa < arg)) { best = ob; arg = oa; }
    }
    if (lane == 0) { shv[wave] = best; shi[wave] = arg; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < NWAVES; ++w)
            if (shv[w] > best || (shv[w] == best && shi[w] < arg)) { best = shv[w]; arg = shi[w]; }
        path[t] = arg;
    }
}

}  // namespace fvs
