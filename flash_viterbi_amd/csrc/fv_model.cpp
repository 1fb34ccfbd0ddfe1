// fv_model.cpp — the host side of fv_set_model and fv_set_model_sparse: value checks, log() of every entry and the table
// encodings, built once per model and uploaded to every device of a context by fv_context.hip.  No HIP call in this
// file: the builders run (and are tested, fv_test_model_digest) without a context and without a GPU.
#include "fv_internal.h"
#include "flashvit_testing.h"

namespace {

// a loop over rows on several host threads
template <typename F>
void parallel_rows(int rows, F &&fn)
{
    unsigned hw = std::thread::hardware_concurrency();
    int nt = (int)std::min<unsigned>(hw ? hw : 4, 16);
    if (rows < 256) nt = 1;
    if (nt <= 1) { fn(0, rows); return; }
    std::vector<std::thread> th;
    int per = (rows + nt - 1) / nt;
    for (int t = 0; t < nt; ++t) {
        int a = t * per, b = std::min(rows, a + per);
        if (a >= b) break;
        th.emplace_back([=, &fn] { fn(a, b); });
    }
    for (auto &x : th) x.join();
}

// The value check of every model entry.  BAD: negative, NaN or +inf — refused.  BIG: above 1 — no filter kernel decodes it.
enum { ENTRY_BAD = 1, ENTRY_BIG = 2 };
inline int entry_flags(float x) { return ((!(x >= 0.0f) || std::isinf(x)) ? ENTRY_BAD : 0) | (x > 1.0f ? ENTRY_BIG : 0); }

inline float window_of(double dmax) { return std::nextafter((float)(2.0 * dmax), HUGE_VALF); }     // 2 * the largest error, rounded up

// The fixed-point (Q16) rule: step = (largest finite |log A|) / 65534 as a float, code = round(-L / step) clamped to
// 0 .. 65534 (0xffff stands for -inf).  The kernels evaluate fma(code, -step, s) with step as a float, so the error is
// measured against exactly that product (code * (double)(float)step is exact in double).  Both builders take codes,
// windowq and qscale from here: a dense-set and a CSR-set model of the same matrix agree bit for bit.
// (The device side of the same rule: q16_step / q16_quantise, fv_device_common.h.)
struct Q16Rule {
    float stepf;
    double stepd;
    explicit Q16Rule(double lmax) : stepf(lmax > 0.0 ? (float)(lmax / 65534.0) : 1.0f), stepd((double)stepf) {}
    double code(double l) const { return std::min(std::max(std::nearbyint(-l / stepd), 0.0), 65534.0); }
    double error(double l) const { return std::fabs(-code(l) * stepd - l); }
    float qscale() const { return -stepf; }
};

// log B (transposed: one row per symbol) and log Pi; returns the OR of their entries' flags
int log_emissions(const float *B, const float *Pi, int K, int M, fvi::HostTables &h)
{
    int flags = 0;
    h.b64.assign((size_t)M * K, 0.0); h.pi64.assign(K, 0.0);
    h.b32.assign((size_t)M * K, 0.0f);
    for (int i = 0; i < K; ++i) {
        for (int o = 0; o < M; ++o) {
            const float x = B[(size_t)i * M + o];
            flags |= entry_flags(x);
            const double l = std::log((double)x);
            h.b64[(size_t)o * K + i] = l; h.b32[(size_t)o * K + i] = (float)l;
        }
        flags |= entry_flags(Pi[i]);
        h.pi64[i] = std::log((double)Pi[i]);
    }
    return flags;
}

}  // namespace

namespace fvi {

// Host side of fv_set_model: log() of every entry in double with the host libm (the calls the reference makes per
// cell, FLASH:142,150,167,170) and the table encodings.
int build_host_tables(const float *A, const float *B, const float *Pi, int K, int M, HostTables &h, std::string &detail)
{
    h.K = K; h.M = M;
    const int nrows = h.nrows = round_up(K, fvk::ROW_ALIGN);
    const int ntiles = h.ntiles = (K + fvk::TILE_W - 1) / fvk::TILE_W;
    // the full-state step kernels keep one score row in LDS: beyond that K only the beam path is available
    // (it needs the float64 table alone, which also keeps the host footprint at 8 B per entry)
    const bool full_ok = h.full_ok = fvk::step_lds_bytes<1>(nrows) <= (size_t)fvk::LDS_LIMIT;
    h.u16_ok = fvk::u16_lds_bytes<1, 8>(nrows) <= (size_t)fvk::LDS_LIMIT && K <= 65536;

    const size_t tab = h.tab = (size_t)ntiles * nrows * fvk::TILE_W;
    std::vector<double> &h64 = h.h64;
    std::vector<float> &h32 = h.h32;
    std::vector<unsigned short> &h16 = h.h16;
    try {
        h64.assign(tab, -HUGE_VAL);
        if (full_ok) { h32.assign(tab, -HUGE_VALF); h16.assign(tab, 0xFC00u /* -inf */); }
    } catch (...) { return FV_ERR_NOMEM; }
    std::vector<double> dmax_row(K, 0.0);
    std::vector<int> flags_row(K, 0);
    parallel_rows(K, [&](int a, int b) {
        for (int k = a; k < b; ++k) {
            const float *src = A + (size_t)k * K;
            int flags = 0;
            for (int i = 0; i < K; ++i) {
                const float x = src[i];
                flags |= entry_flags(x);
                const double l = std::log((double)x);
                const size_t e = fvk::tab_index<4>(k, i, nrows);
                h64[e] = l;
                if (!full_ok) continue;
                h32[e] = (float)l;
                const _Float16 hl = (_Float16)l;          // round to nearest even; -inf stays -inf
                unsigned short hb;
                std::memcpy(&hb, &hl, 2);
                h16[fvk::tab_index<8>(k, i, nrows)] = hb;
                if (std::isfinite(l)) {
                    // a finite log that overflows binary16 (< -65504) would become -inf: cannot happen for
                    // float32 inputs (log >= -104), but keep the bound honest
                    const double d = std::isfinite((double)hl) ? std::fabs((double)hl - l) : HUGE_VAL;
                    if (d > dmax_row[k]) dmax_row[k] = d;
                }
            }
            flags_row[k] = flags;
        }
    });
    int flags = log_emissions(B, Pi, K, M, h);
    for (int k = 0; k < K; ++k) flags |= flags_row[k];
    h.any_big = (flags & ENTRY_BIG) != 0;
    if (flags & ENTRY_BAD) { detail = "model entries must be finite and >= 0"; return FV_ERR_ARG; }

    double dmax = 0.0;
    for (int k = 0; k < K; ++k) dmax = std::max(dmax, dmax_row[k]);
    h.window16 = window_of(dmax);
    h.density = 1.0; h.windowq = 0.0f; h.qscale = -1.0f;
    if (!full_ok) return FV_OK;
    // fixed-point table (Q16Rule)
    std::vector<unsigned short> &hq = h.hq;
    try { hq.assign(tab, 0xFFFFu); } catch (...) { return FV_ERR_NOMEM; }
    double lmax = 0.0;
    for (size_t e = 0; e < tab; ++e) if (std::isfinite(h64[e])) lmax = std::max(lmax, -h64[e]);
    const Q16Rule q16(lmax);
    std::vector<double> dq_row(K, 0.0);
    parallel_rows(K, [&](int a, int b) {
        for (int k = a; k < b; ++k)
            for (int i = 0; i < K; ++i) {
                const double l = h64[fvk::tab_index<4>(k, i, nrows)];
                if (!std::isfinite(l)) continue;
                hq[fvk::tab_index<8>(k, i, nrows)] = (unsigned short)q16.code(l);
                const double d = q16.error(l);
                if (d > dq_row[k]) dq_row[k] = d;
            }
    });
    double dqmax = 0.0;
    for (int k = 0; k < K; ++k) dqmax = std::max(dqmax, dq_row[k]);
    h.windowq = window_of(dqmax);
    h.qscale = q16.qscale();
    // sparse form of the same codes (CSC-Q16, see trellis_step_sparse): per tile, per column, the finite
    // entries in ascending k as (k << 16 | code), 4 per lane load, columns padded to the tile's longest
    if (K <= 65536) {
        std::vector<int> &off = h.sp_off, &nwbv = h.sp_nwb;
        off.assign(ntiles, 0); nwbv.assign(ntiles, 0);
        std::vector<std::vector<uint32_t>> cols((size_t)ntiles * fvk::TILE_W);
        parallel_rows(ntiles, [&](int a, int b) {
            for (int tl = a; tl < b; ++tl)
                for (int c = 0; c < fvk::TILE_W; ++c) {
                    const int i = tl * fvk::TILE_W + c;
                    if (i >= K) continue;
                    std::vector<uint32_t> &v = cols[(size_t)tl * fvk::TILE_W + c];
                    for (int k = 0; k < K; ++k) {
                        const unsigned short code = hq[fvk::tab_index<8>(k, i, nrows)];
                        if (code != 0xFFFFu) v.push_back(((uint32_t)k << 16) | code);
                    }
                }
        });
        size_t nnz = 0, total = 0;
        for (int tl = 0; tl < ntiles; ++tl) {
            size_t longest = 0;
            for (int c = 0; c < fvk::TILE_W; ++c) {
                const size_t n = cols[(size_t)tl * fvk::TILE_W + c].size();
                nnz += n; longest = std::max(longest, n);
            }
            const int nch = (int)((longest + 3) / 4);
            nwbv[tl] = (nch + 3) / 4;
            off[tl] = (int)total;
            total += (size_t)nwbv[tl] * 4 * fvk::TILE_W;
        }
        h.density = (double)nnz / ((double)K * K);
        if (total < (size_t)1 << 30 && total > 0) {
            std::vector<uint4> &sp = h.sp;
            try { sp.resize(total); } catch (...) { return FV_ERR_NOMEM; }
            const uint32_t pad = 0x0000FFFFu;           // k = 0, code = 0xffff (-inf)
            parallel_rows(ntiles, [&](int a, int b) {
                for (int tl = a; tl < b; ++tl)
                    for (int j = 0; j < nwbv[tl] * 4; ++j)
                        for (int c = 0; c < fvk::TILE_W; ++c) {
                            const std::vector<uint32_t> &v = cols[(size_t)tl * fvk::TILE_W + c];
                            uint32_t e[4];
                            for (int q = 0; q < 4; ++q) e[q] = (size_t)(4 * j + q) < v.size() ? v[4 * j + q] : pad;
                            sp[(size_t)off[tl] + (size_t)j * fvk::TILE_W + c] = make_uint4(e[0], e[1], e[2], e[3]);
                        }
            });
        }
    }
    return FV_OK;
}

// Host side of fv_set_model_sparse.  Checks the CSR arrays, takes log((double)x) of every stored entry with the host libm
// (per entry the call build_host_tables makes) and applies the same Q16Rule to the finite ones: the absent entries are
// the dense table's -inf cells, which take part in neither step nor window.
int build_host_csr(const long long *row_ptr, const int *col, const float *val, const float *B, const float *Pi, int K, int M,
                   HostCsr &h, std::string &detail)
{
    HostTables &e = h.e;
    e.K = K; e.M = M;
    e.nrows = round_up(K, fvk::ROW_ALIGN);
    const int ntiles = e.ntiles = (K + fvk::TILE_W - 1) / fvk::TILE_W;
    if (row_ptr[0] != 0) { detail = "fv_set_model_sparse: row_ptr[0] must be 0 (row 0)"; return FV_ERR_ARG; }
    for (int k = 0; k < K; ++k)
        if (row_ptr[k + 1] < row_ptr[k]) { detail = "fv_set_model_sparse: row_ptr decreases at row " + std::to_string(k); return FV_ERR_ARG; }
    const long long nnz = row_ptr[K];
    if (nnz > 0 && (!col || !val)) return FV_ERR_ARG;
    // (a row holds at most K entries once its columns are strictly ascending, so nnz <= K * K without a check of its own)
    enum { COL_RANGE = 1, COL_ORDER = 2, VALUE_SHIFT = 2 };      // per row; the entries' flags above them
    std::vector<int> bad_row(K, 0);
    std::vector<double> lmax_row(K, 0.0);
    try { h.rlog.resize((size_t)nnz); } catch (...) { return FV_ERR_NOMEM; }
    parallel_rows(K, [&](int a, int b) {
        for (int k = a; k < b; ++k) {
            int prev = -1;
            for (long long p = row_ptr[k]; p < row_ptr[k + 1]; ++p) {
                const int i = col[p];
                const float x = val[p];
                if (i < 0 || i >= K) bad_row[k] |= COL_RANGE;
                else if (i <= prev) bad_row[k] |= COL_ORDER;
                prev = i;
                bad_row[k] |= entry_flags(x) << VALUE_SHIFT;
                const double l = std::log((double)x);
                h.rlog[(size_t)p] = l;
                if (std::isfinite(l)) lmax_row[k] = std::max(lmax_row[k], -l);
            }
        }
    });
    for (int k = 0; k < K; ++k) {
        if (bad_row[k] & COL_RANGE) { detail = "fv_set_model_sparse: row " + std::to_string(k) + " holds a column outside [0, K)"; return FV_ERR_ARG; }
        if (bad_row[k] & COL_ORDER) { detail = "fv_set_model_sparse: the columns of row " + std::to_string(k) + " are not strictly ascending"; return FV_ERR_ARG; }
    }
    int flags = log_emissions(B, Pi, K, M, e);
    for (int k = 0; k < K; ++k) {
        if (bad_row[k] & (ENTRY_BAD << VALUE_SHIFT)) { detail = "model entries must be finite and >= 0 (row " + std::to_string(k) + ")"; return FV_ERR_ARG; }
        flags |= bad_row[k] >> VALUE_SHIFT;
    }
    e.any_big = (flags & ENTRY_BIG) != 0;
    if (flags & ENTRY_BAD) { detail = "model entries must be finite and >= 0"; return FV_ERR_ARG; }

    double lmax = 0.0;
    for (int k = 0; k < K; ++k) lmax = std::max(lmax, lmax_row[k]);
    const Q16Rule q16(lmax);
    // per destination column: the number of finite entries, then the tiles' extents (columns padded to the tile's
    // longest, rounded up to a wave-block of 4 chunks x 4 entries)
    std::vector<int> cnt((size_t)ntiles * fvk::TILE_W, 0);
    long long nfin = 0;
    double dqmax = 0.0;
    for (long long p = 0; p < nnz; ++p) {
        const double l = h.rlog[(size_t)p];
        if (!std::isfinite(l)) continue;
        ++cnt[(size_t)col[p]];
        ++nfin;
        dqmax = std::max(dqmax, q16.error(l));
    }
    e.windowq = window_of(dqmax);
    e.qscale = q16.qscale();
    e.window16 = 0.0f;                   // (no binary16 table)
    e.density = (double)nfin / ((double)K * K);
    h.off.assign(ntiles, 0); h.nwb.assign(ntiles, 0);
    long long total = 0;
    for (int tl = 0; tl < ntiles; ++tl) {
        int longest = 0;
        for (int c = 0; c < fvk::TILE_W; ++c) longest = std::max(longest, cnt[(size_t)tl * fvk::TILE_W + c]);
        h.nwb[tl] = (longest + 15) / 16;
        h.off[tl] = total;
        total += (long long)h.nwb[tl] * 4 * fvk::TILE_W;
    }
    try {
        h.ck.assign((size_t)total, make_uint4(0u, 0u, 0u, 0u));
        h.cq.assign((size_t)total, make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu));
        h.c64.assign((size_t)total * 4, -HUGE_VAL);
    } catch (...) { return FV_ERR_NOMEM; }
    // rows in ascending k: every column fills in ascending source state
    std::fill(cnt.begin(), cnt.end(), 0);
    unsigned int *kw = reinterpret_cast<unsigned int *>(h.ck.data());
    unsigned short *qw = reinterpret_cast<unsigned short *>(h.cq.data());
    for (int k = 0; k < K; ++k)
        for (long long p = row_ptr[k]; p < row_ptr[k + 1]; ++p) {
            const double l = h.rlog[(size_t)p];
            if (!std::isfinite(l)) continue;
            const int i = col[p], n = cnt[(size_t)i]++;
            const size_t pos = 4 * ((size_t)h.off[i / fvk::TILE_W] + (size_t)(n >> 2) * fvk::TILE_W + (i % fvk::TILE_W)) + (n & 3);
            kw[pos] = (unsigned int)k;
            qw[pos] = (unsigned short)q16.code(l);
            h.c64[pos] = l;
        }
    return FV_OK;
}

}  // namespace fvi

// FNV-1a, 64 bit, over the bytes of a host table
template <typename T>
static unsigned long long fnv1a(const std::vector<T> &v)
{
    unsigned long long h = 0xcbf29ce484222325ull;
    const unsigned char *p = reinterpret_cast<const unsigned char *>(v.data());
    for (size_t i = 0, n = v.size() * sizeof(T); i < n; ++i) { h ^= p[i]; h *= 0x100000001b3ull; }
    return h;
}

// include/flashvit_testing.h: the host builders alone, their tables as digests
extern "C" int fv_test_model_digest(const float *A, const long long *row_ptr, const int *col, const float *val, const float *B, const float *Pi,
                                    int K, int M, unsigned long long *digests, double *params, char *detail, int detail_cap)
{
    if ((!A && !row_ptr) || !B || !Pi || K < 1 || M < 1 || !digests || !params) return FV_ERR_ARG;
    fvi::HostTables h;
    fvi::HostCsr c;
    const fvi::HostTables &e = A ? h : c.e;
    std::string text;
    int rc = FV_OK, n = 0;
    try {
        rc = A ? fvi::build_host_tables(A, B, Pi, K, M, h, text) : fvi::build_host_csr(row_ptr, col, val, B, Pi, K, M, c, text);
    } catch (const std::bad_alloc &) { rc = FV_ERR_NOMEM; }
    auto put = [&](auto &&...v) { ((digests[n++] = fnv1a(v)), ...); };
    if (A) put(h.h64, h.h32, h.h16, h.hq, h.sp, h.sp_off, h.sp_nwb);
    else put(c.ck, c.cq, c.c64, c.off, c.nwb, c.rlog);
    put(e.b64, e.b32, e.pi64);
    params[0] = e.window16; params[1] = e.windowq; params[2] = e.qscale; params[3] = e.density; params[4] = e.any_big ? 1.0 : 0.0;
    if (detail && detail_cap > 0) std::snprintf(detail, (size_t)detail_cap, "%s", text.c_str());
    return rc;
}
