// fv_layout.h — table layout, workgroup geometry and LDS budgets of the full-state kernels: the part of
// fv_kernels.hip.inc the host-only translation units (model upload, workspace sizing) need as well.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

namespace fvk {

constexpr int TILE_W = 16;                 // destination states (columns) per workgroup: 64 B of f32 per row
constexpr int ROWG = 64 / TILE_W;          // source rows covered by one wave-wide load (4)
constexpr int NWAVES = 16;
constexpr int BLOCK = NWAVES * 64;         // 1024 threads: one workgroup per CU keeps 64+ KB of loads in flight
constexpr int ROW_ALIGN = 32;              // nrows = roundup(K, 32): whole row blocks for every table type
constexpr int MAX_BATCH = 8;               // independent tasks sharing one sweep of the table
constexpr int LDS_LIMIT = 160 * 1024;      // bytes of LDS one workgroup may ask for (gfx950: all of a CU's 160 KB)
constexpr int BEAM_LDS_LIMIT = 150 * 1024; // the smaller bound the beam path admits a beam width by (fv_beam.hip, beam_admit_k)

// Tile-major layout with an R-row interleave: R = 4 for the f32 / f64 tables, 8 for the f16 table.
template <int R>
__host__ __device__ inline size_t tab_index(int k, int col, int nrows)
{
    return (size_t)(col >> 4) * nrows * TILE_W + ((size_t)(k / R) * TILE_W + (col & 15)) * R + (k % R);
}
// back-tracks of at least BT_MIN_PARALLEL steps are walked by 64 lanes, each starting BT_WARMUP steps above its chunk (fvk::backtrack)
constexpr int BT_WARMUP = 32, BT_MIN_PARALLEL = 128;
struct PassDesc { int L, R, from_pi, whole; long long row_off; };   // row_off: float offset of the pass's 2 score rows
constexpr int PASS_CHUNK = 64;
struct PassChunk { int n; PassDesc p[PASS_CHUNK]; };
// FV_OPT_FLAT_GENERATIONS: one right-hand pass of the flat set as the back-track and the resolver see it (fv_schedule.h, FlatPass)
struct FlatDesc { int L, R, generation, chain; long long arg_row; };
constexpr int FLAT_MAX_GENS = 40;          // (a generation halves the pass length: T < 2^31 has at most 32)
struct FlatGens { int ngen; int begin[FLAT_MAX_GENS + 1]; };   // passes [begin[g], begin[g + 1]) are generation g + 1
// The device statistics words (ctx->d_counters), named after the fv_stats field each one feeds (read_stats, fv_context.hip).
enum : int {
    CNT_REFINE_NEAR = 0, CNT_REFINE_RESCAN, CNT_BEAM_EXACT_SETS, CNT_BEAM_DUP_COLS, CNT_BEAM_DUP_STEPS,
    CNT_HANDSHAKE_TIMEOUT,                 // = 5: a heap replay's producer / consumer hand-shake timed out (FV_ERR_DEVICE, no field)
    CNT_BEAM_TIES, CNT_BEAM_CAND_SELECTS, CNT_REFINE_SATURATED, CNT_BEAM_SPEC_STEPS, CNT_BEAM_REACH_EVENTS, CNT_BEAM_LIST_SHORT,
    CNT_BEAM_LIST_LONG, CNT_BEAM_LIST_ENTRIES, CNT_BEAM_CHAIN_CUTS,
    FLAT_COUNTER,                          // = 15, the resolver: first-miss generation << 32 | missed passes
    BT_COUNTER,                            // = 16, the back-tracks: passes through the retry branch of the chunk walk (fv_stats.bt_restarts)
    NCOUNTERS
};
static_assert(CNT_HANDSHAKE_TIMEOUT == 5 && FLAT_COUNTER == 15 && BT_COUNTER == 16 && NCOUNTERS == 17, "the words keep their places");

// LDS of one trellis_step / trellis_step_u16 workgroup (score rows + reduction scratch)
template <int NB>
static inline size_t step_lds_bytes(int nrows)
{
    return (size_t)nrows * NB * 4 + (size_t)NB * NWAVES * TILE_W * 12 + (size_t)NB * TILE_W * 4;
}

template <int NB, int NWV>
static inline size_t u16_lds_bytes(int nrows)
{
    return (size_t)nrows * NB * 2 + (size_t)NB * NWV * TILE_W * 12 + (size_t)NB * TILE_W * 4;
}

}  // namespace fvk
