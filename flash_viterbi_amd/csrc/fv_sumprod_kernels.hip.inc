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

// ---------------------------------------------------------------- models set by fv_set_model_sparse (DESIGN.md 5.7b)
//
// The same recurrences on the stored transitions: the forward step walks the CSC-32 table of trellis_step_csr
// (fv_kernels.hip.inc: ck[v] the four source states of vector v, tile_off / tile_nwb the tiles' extents) with CSlin, the
// stored values themselves as float32 at the index of CS64 (pads 0); the backward step walks the caller's rows
// (CRptr / CRcol) with CRlin at the index of CRlog.  Both stream 8 bytes per entry and do one convert and one explicit
// float64 fma per entry and task.
// The scaled row p[i] = exp(in[i] + ein[i] - m), m the row maximum, comes in one of two forms.  MEM = false: every
// workgroup folds m and stages its NB rows in LDS, as sumprod_step does.  MEM = true: sumprod_rowmax and sumprod_scale
// leave p and m in workspace rows once per step and task, and the step gathers p from memory — no workgroup of a step
// reads a whole row.  The maximum is exact in any order and exp is the same call on the same argument, so p has the
// same bits in both forms.
// Order of the sums (guarantee 3): it is a function of the table layout alone — not of NB, of how a batch is grouped or
// of MEM.  Forward: a lane sums its entries in ascending wave-block order, the four lanes of a column are folded by two
// fixed shuffles, the waves in index order through LDS.  Backward: the stored entries of a row that are not 0 are dealt
// in their order to the 16 lanes of the row's sub-wave (the entry of rank r to lane r % 16, which sums its share in
// ascending r), and one fixed butterfly joins the lanes; a stored 0 therefore changes nothing, as it changes nothing in
// the CSC-32 table, which never holds one.
// The threshold.  A column (row) whose linear sum s is below 2^-800 is re-evaluated in the exact per-column form from the
// stored logs (CS64 / CRlog at the same positions) and counted.  What the linear sum can have lost: a p[i] below 2^-1022
// (flushed to 0, or a denormal with an absolute error up to 2^-1075), times an entry below 2^128 (any float32), in fewer
// than 2^31 terms (any K the ABI can express): less than 2^-1022 * 2^128 * 2^31 = 2^-863 in all, which is below
// u * s = 2^-53 * s for every s >= 2^-800 (2^-853), whatever the model's entries and whatever K.
constexpr int CSR_WAVES = 8, CSR_BLOCK = CSR_WAVES * 64;      // the workgroup of trellis_step_csr
constexpr int BACK_SUB = 16;                                  // lanes per source row of sumprod_back_csr: four rows per wave
constexpr int BACK_ROWS = BLOCK / BACK_SUB;                   // rows per workgroup (64)
constexpr int SCALE_PARTS = 64, SCALE_BLOCK = 256;            // partial maxima per row; threads of the two scale kernels
constexpr int SCALE_PER_THREAD = 4;

// MEM: the NB rows sumprod_scale left, K doubles apart, and their NB maxima (one base each: the tasks' own pointers fill the
// scalar registers of an NB = 4 launch already)
struct ScaledRows { const double *p, *m; };

__host__ __device__ inline size_t csr_step_lds_doubles(int nb, int nrows, bool mem)
{
    return (size_t)nb * ((mem ? (size_t)0 : (size_t)nrows) + CSR_WAVES * TILE_W + 2 * CSR_WAVES);
}
__host__ __device__ inline size_t csr_back_lds_doubles(int nb, int nrows, bool mem)
{
    return (size_t)nb * ((mem ? (size_t)0 : (size_t)nrows) + NWAVES);
}

// m[b] and the NB scaled rows in LDS, by the whole workgroup of NT threads (wmax: [NB][NT / 64]); ends with a barrier
template <int NB, int NT>
__device__ inline void stage_scaled(const StepTask *t, int K, int nrows, double *p, double *wmax, double (&m)[NB])
{
    constexpr int NW = NT / 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        double mx = -HUGE_VAL;
        for (int k = tid; k < K; k += NT) mx = fmax(mx, task_in(t[b], k));
        mx = wave_max(mx);
        if (lane == 0) wmax[b * NW + wave] = mx;
    }
    __syncthreads();
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        double mx = wmax[b * NW];
        for (int w = 1; w < NW; ++w) mx = fmax(mx, wmax[b * NW + w]);
        m[b] = mx;
        for (int k = tid; k < nrows; k += NT)
            p[(size_t)b * nrows + k] = (k < K && mx > -HUGE_VAL) ? exp(task_in(t[b], k) - mx) : 0.0;
    }
    __syncthreads();
}

template <int NB>
struct CsrStepArgs {
    const uint4 *ck;
    const float *clin;
    const double *c64;
    const long long *tile_off;   // [ntiles] first vector of each tile
    const int *tile_nwb;         // [ntiles] wave-blocks (64 vectors) in each tile
    unsigned long long *counters;
    int K, nrows, ntiles, tiles_per_xcd;
    ScaledRows s;
    StepTask t[NB];
};

// Forward: one workgroup per 16-column tile, the geometry of trellis_step_csr.  Pads hold state 0 and the value 0: they
// add p[0] * 0 = 0.  Epilogue: sumprod_step's.
template <int NB, bool MEM>
__global__ __launch_bounds__(CSR_BLOCK) void sumprod_step_csr(const CsrStepArgs<NB> a)
{
    extern __shared__ double lds[];
    const int nrows = a.nrows, K = a.K;
    double *p = lds;                                                  // [NB][nrows] (MEM: absent)
    double *red = p + (MEM ? (size_t)0 : (size_t)NB * nrows);         // [NB][CSR_WAVES][TILE_W]
    double *wmax = red + NB * CSR_WAVES * TILE_W;                     // [NB][CSR_WAVES]
    int *need = reinterpret_cast<int *>(wmax + NB * CSR_WAVES);       // [NB][TILE_W] (NB * CSR_WAVES doubles of room)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & (TILE_W - 1), rg = lane >> 4;
    const int tile = (blockIdx.x & 7) * a.tiles_per_xcd + (blockIdx.x >> 3);
    if (tile >= a.ntiles) return;                                     // workgroup-uniform
    const size_t off = (size_t)a.tile_off[tile], v0 = off + rg * TILE_W + c;      // this lane's vector of wave-block 0
    const uint4 *kb = a.ck + v0;
    const float4 *lb = reinterpret_cast<const float4 *>(a.clin) + v0;
    const int nwb = a.tile_nwb[tile];
    const int nj = nwb > wave ? (nwb - wave + CSR_WAVES - 1) / CSR_WAVES : 0;     // wave-blocks of this wave
    auto vec = [&](int j) { return (size_t)(wave + CSR_WAVES * j) * (4 * TILE_W); };

    double m[NB];
    if (tid < NB * TILE_W) need[tid] = 0;
    if constexpr (MEM) {
#pragma unroll
        for (int b = 0; b < NB; ++b) m[b] = a.s.m[b];
    } else {
        stage_scaled<NB, CSR_BLOCK>(a.t, K, nrows, p, wmax, m);
    }

    double acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] = 0.0;
    auto cell = [&](unsigned int k, float x) {
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            double pv;
            if constexpr (MEM) pv = a.s.p[(size_t)b * K + k];
            else pv = p[(size_t)b * nrows + k];
            acc[b] = fma(pv, (double)x, acc[b]);
        }
    };
#pragma unroll 4
    for (int j = 0; j < nj; ++j) {
        const uint4 k4 = kb[vec(j)];
        const float4 x4 = lb[vec(j)];
        cell(k4.x, x4.x); cell(k4.y, x4.y); cell(k4.z, x4.z); cell(k4.w, x4.w);
    }
    // lanes c, c + 16, c + 32, c + 48 of a wave hold the same column: fold them, then the waves in order
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        double s = acc[b] + __shfl_xor(acc[b], 16);
        s = s + __shfl_xor(s, 32);
        if (lane < TILE_W) red[(b * CSR_WAVES + wave) * TILE_W + lane] = s;
    }
    __syncthreads();
    if (tid < NB * TILE_W) {
        const int b = tid / TILE_W, cc = tid % TILE_W, col = tile * TILE_W + cc;
        double s = 0.0;
        for (int w = 0; w < CSR_WAVES; ++w) s = s + red[(b * CSR_WAVES + w) * TILE_W + cc];
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
    // the exact column: wave w takes columns w and w + CSR_WAVES of every task that asked.  Entry e of column c2 lies in
    // wave-block e / 16, chunk (e / 4) % 4, at place e % 4 of its vector.
    const unsigned int *kw = reinterpret_cast<const unsigned int *>(a.ck);
    const int nent = nwb * 16;
    for (int c2 = wave; c2 < TILE_W; c2 += CSR_WAVES) {
        const int col = tile * TILE_W + c2;
        auto place = [&](int e) { return 4 * (off + (size_t)(e >> 4) * (4 * TILE_W) + (size_t)((e >> 2) & 3) * TILE_W + c2) + (e & 3); };
#pragma nounroll                 // (one task's pointers in scalar registers at a time: unrolled, NB = 4 spills two)
        for (int b = 0; b < NB; ++b) {
            if (!need[b * TILE_W + c2]) continue;
            const StepTask &t = a.t[b];
            double mx = -HUGE_VAL;
            for (int e = lane; e < nent; e += 64) {
                const double L = a.c64[place(e)];
                if (L > -HUGE_VAL) mx = fmax(mx, task_in(t, (int)kw[place(e)]) + L);
            }
            mx = wave_max(mx);
            double r = -HUGE_VAL;
            if (mx > -HUGE_VAL) {
                double s = 0.0;
                for (int e = lane; e < nent; e += 64) {
                    const double L = a.c64[place(e)];
                    if (L > -HUGE_VAL) s = s + exp(task_in(t, (int)kw[place(e)]) + L - mx);
                }
                s = wave_sum(s);
                r = mx + log(s);
            }
            if (lane == 0) {
                t.out[col] = (t.eout && r > -HUGE_VAL) ? t.eout[col] + r : r;
                atomicAdd(&a.counters[CNT_REFINE_COLUMNS], 1ull);
                if (r > -HUGE_VAL) atomicAdd(&a.counters[CNT_REFINE_FINITE], 1ull);
            }
        }
    }
}

template <int NB>
struct CsrBackArgs {
    const long long *rptr;       // [K + 1] the caller's rows
    const int *rcol;
    const float *rlin;
    const double *rlog;
    unsigned long long *counters;
    int K, nrows;
    ScaledRows s;
    StepTask t[NB];
};

// The chunk of 16 consecutive stored entries a sub-wave holds one per lane, `mask` its entries that are not 0, cnt the
// row's non-zero entries before the chunk: lane l takes the chunk's non-zero entry of rank n = (l - cnt) mod 16, if
// there is one (has), and finds it in lane `src` of the sub-wave.
__device__ inline int deal_source(unsigned int mask, int cnt, int l, bool &has)
{
    const int n = (l - cnt) & (BACK_SUB - 1);
    has = n < __popc(mask);
    if ((mask & (mask + 1)) == 0 || !has) return has ? n : 0;     // the non-zero entries are the chunk's first ones
    for (int i = 0; i < n; ++i) mask &= mask - 1;
    return __ffs((int)mask) - 1;
}

// Backward: out[i] = m + log sum_{e in row i} CRlin[e] * q[CRcol[e]], q the scaled row of the time read.  A sub-wave of
// 16 lanes per source row, four rows per wave, 64 per workgroup; the row's entries come in chunks of 16, one per lane.
template <int NB, bool MEM>
__global__ __launch_bounds__(BLOCK) void sumprod_back_csr(const CsrBackArgs<NB> a)
{
    extern __shared__ double lds[];
    const int nrows = a.nrows, K = a.K;
    double *q = lds;                                                  // [NB][nrows] (MEM: absent)
    double *wmax = q + (MEM ? (size_t)0 : (size_t)NB * nrows);        // [NB][NWAVES]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sub = lane / BACK_SUB, l = lane % BACK_SUB, first = sub * BACK_SUB;
    const int row = blockIdx.x * BACK_ROWS + wave * (64 / BACK_SUB) + sub;

    double m[NB];
    if constexpr (MEM) {
#pragma unroll
        for (int b = 0; b < NB; ++b) m[b] = a.s.m[b];
    } else {
        stage_scaled<NB, BLOCK>(a.t, K, nrows, q, wmax, m);
    }
    if (row >= K) return;                                             // (uniform in the sub-wave; no barrier follows)
    const long long beg = a.rptr[row], end = a.rptr[row + 1];

    double acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] = 0.0;
    int cnt = 0;
    // every branch below is uniform in the sub-wave, and a sub-wave reads its own 16 bits of a ballot and its own lanes only
    for (long long base = beg; base < end; base += BACK_SUB) {
        const long long e = base + l;
        const float x = e < end ? a.rlin[e] : 0.0f;
        const int j = e < end ? a.rcol[e] : 0;
        const unsigned int mask = (unsigned int)(__ballot(x != 0.0f) >> first) & 0xffffu;
        double qv[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            if constexpr (MEM) qv[b] = a.s.p[(size_t)b * K + j];
            else qv[b] = q[(size_t)b * nrows + j];
        }
        if ((mask & (mask + 1)) == 0 && (cnt & (BACK_SUB - 1)) == 0) {
            // the chunk's non-zero entries are its first ones and their ranks start at a multiple of 16 (every chunk of a
            // model that stores no 0): lane l takes its own entry, and a lane without one adds q * 0, which changes nothing
#pragma unroll
            for (int b = 0; b < NB; ++b) acc[b] = fma(qv[b], (double)x, acc[b]);
        } else {
            bool has;
            const int src = first + deal_source(mask, cnt, l, has);
            const float xs = __shfl(x, src);
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                const double qs = __shfl(qv[b], src);
                if (has) acc[b] = fma(qs, (double)xs, acc[b]);
            }
        }
        cnt += __popc(mask);
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        double s = acc[b];
#pragma unroll
        for (int o = BACK_SUB / 2; o >= 1; o >>= 1) s = s + __shfl_xor(s, o);      // butterfly: the 16 lanes end with the same bits
        const StepTask &t = a.t[b];
        double r;
        if (!(m[b] > -HUGE_VAL)) r = -HUGE_VAL;                        // nothing comes in: nothing to refine
        else if (s >= REFINE_BELOW) r = m[b] + log(s);
        else {
            // the exact row, by its own sub-wave: the maximum, then the terms dealt to the lanes as above
            double mx = -HUGE_VAL;
            for (long long e = beg + l; e < end; e += BACK_SUB) {
                const double L = a.rlog[e];
                if (L > -HUGE_VAL) mx = fmax(mx, task_in(t, a.rcol[e]) + L);
            }
#pragma unroll
            for (int o = BACK_SUB / 2; o >= 1; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o));
            r = -HUGE_VAL;
            if (mx > -HUGE_VAL) {
                double sx = 0.0;
                int seen = 0;
                for (long long base = beg; base < end; base += BACK_SUB) {
                    const long long e = base + l;
                    const double L = e < end ? a.rlog[e] : -HUGE_VAL;
                    const double term = L > -HUGE_VAL ? exp(task_in(t, a.rcol[e]) + L - mx) : 0.0;
                    const unsigned int mask = (unsigned int)(__ballot(L > -HUGE_VAL) >> first) & 0xffffu;
                    if (mask) {
                        bool has;
                        const int src = first + deal_source(mask, seen, l, has);
                        const double ts = __shfl(term, src);
                        if (has) sx = sx + ts;
                    }
                    seen += __popc(mask);
                }
#pragma unroll
                for (int o = BACK_SUB / 2; o >= 1; o >>= 1) sx = sx + __shfl_xor(sx, o);
                r = mx + log(sx);
            }
            if (l == 0) {
                atomicAdd(&a.counters[CNT_REFINE_COLUMNS], 1ull);
                if (r > -HUGE_VAL) atomicAdd(&a.counters[CNT_REFINE_FINITE], 1ull);
            }
        }
        if (l == 0) t.out[row] = (t.eout && r > -HUGE_VAL) ? t.eout[row] + r : r;
    }
}

// The scale launch of the memory form, two kernels.  sumprod_rowmax: part[task][g] = the maximum of the slice of the
// incoming row that block g strides over (grid SCALE_PARTS x tasks).
__global__ __launch_bounds__(SCALE_BLOCK) void sumprod_rowmax(StepArgs<MAX_NB> a, int K, double *part)
{
    __shared__ double sh[SCALE_BLOCK / 64];
    const StepTask &t = a.t[blockIdx.y];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double mx = -HUGE_VAL;
    for (long long k = (long long)blockIdx.x * SCALE_BLOCK + tid; k < K; k += (long long)SCALE_PARTS * SCALE_BLOCK) mx = fmax(mx, task_in(t, (int)k));
    mx = wave_max(mx);
    if (lane == 0) sh[wave] = mx;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < SCALE_BLOCK / 64; ++w) mx = fmax(mx, sh[w]);
        part[blockIdx.y * SCALE_PARTS + blockIdx.x] = mx;
    }
}

// sumprod_scale: m[task] = the maximum of the partial maxima, p[task][k] = exp(in[k] + ein[k] - m), 0 when m is -inf
// (grid ceil(K / (SCALE_BLOCK * SCALE_PER_THREAD)) x tasks; pitch: doubles between the tasks' rows of p).
__global__ __launch_bounds__(SCALE_BLOCK) void sumprod_scale(StepArgs<MAX_NB> a, int K, const double *part, double *p, size_t pitch, double *m)
{
    __shared__ double sh;
    const StepTask &t = a.t[blockIdx.y];
    const int tid = threadIdx.x;
    if (tid < 64) {
        const double mx = wave_max(tid < SCALE_PARTS ? part[blockIdx.y * SCALE_PARTS + tid] : -HUGE_VAL);
        if (tid == 0) { sh = mx; if (blockIdx.x == 0) m[blockIdx.y] = mx; }
    }
    __syncthreads();
    const double mx = sh;
    const long long k0 = (long long)blockIdx.x * (SCALE_BLOCK * SCALE_PER_THREAD) + tid;
#pragma unroll
    for (int i = 0; i < SCALE_PER_THREAD; ++i) {
        const long long k = k0 + (long long)i * SCALE_BLOCK;
        if (k < K) p[blockIdx.y * pitch + (size_t)k] = mx > -HUGE_VAL ? exp(task_in(t, (int)k) - mx) : 0.0;
    }
}

// CSlin / CRlin from the stored logs, as sumprod_build_table does it: (float)exp(log((double)a)) returns a's bits; a pad's
// log of -inf gives 0.
__global__ void sumprod_build_lin(const double *__restrict__ logs, float *__restrict__ out, size_t n)
{
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n) out[e] = (float)exp(logs[e]);
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
