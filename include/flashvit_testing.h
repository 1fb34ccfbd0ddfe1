/*
 * flashvit_testing.h — test hooks of libflashvit.so.  NOT part of the drop-in ABI of flashvit.h: no host program
 * or driver calls them, and they may change with the kernels they expose.  They exist so that the test suite can
 * compare whole step outputs (every column of every score and back-pointer row) with a restatement of the
 * recurrence, instead of the T entries of a decoded path.
 *
 * The hooks add no work to a decode: what they need on the decode path is a host-side branch on a flag that only
 * a hook call sets (the launch helpers record which step-kernel instantiation they launched).
 */
#ifndef FLASHVIT_TESTING_H
#define FLASHVIT_TESTING_H

#include "flashvit.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One full-state forward pass: steps j = L+1 .. R.  init_state < 0 starts from Pi (only at L = 0); otherwise the
 * initial row is log A[init_state][*] + log B[*][ob[L]] (only at L > 0: the state at time L-1 lives in the answer
 * array, which has no entry for time -1). */
typedef struct { int L, R, init_state; } fv_test_pass;

/* Runs the passes as ONE generation of the full-state driver (the lock-step loop fv_decode_full uses), under the
 * current FV_OPT_KERNEL, FV_OPT_MAX_BATCH and FV_OPT_DEBUG, and through the same admission, kernel choice and
 * table setup as fv_decode_full (what it refuses, this refuses).  No pass is the whole-sequence pass, so the
 * right-hand forms of the driver run (batched and forked launches); every last step is a full step (FV_OPT_DEBUG
 * bit 3 is OR-ed in for the duration of the call).
 *   rows_out[npasses*K]  the score row after step R of each pass, in the caller's order;
 *   bp_out[T*K]          back-pointer rows L+1 .. R of each pass at their absolute times (-1: no finite predecessor);
 *                        the other rows are left as they are;
 *   variants_out         (may be NULL) the FV_TV_* bits of every step-kernel instantiation that launched.
 * FV_ERR_ARG: R <= L, R >= T, overlapping [L, R] ranges, init_state outside [0, K) where one is needed or given at
 * L = 0, a symbol outside [0, M), or a multi-device context.  The answer array is overwritten, and fv_last_stats
 * afterwards describes this call (kernel, passes, step launches; no timings), not a decode. */
int fv_test_forward(fv_ctx *ctx, const int *ob, int T, const fv_test_pass *passes, int npasses,
                    float *rows_out, int *bp_out, unsigned long long *variants_out);

/* One slot set of a beam step: n entries {val[e], state[e]} (states in [0, K)), beam <= n <= beam + 32. */
typedef struct { const float *val; const int *state; int n; } fv_test_beam_set;
/* One entry of a candidate list: a score and its destination state. */
typedef struct { float value; int state; } fv_test_cand;

/* One launch of the FLASH-BS step kernel over nsets (1 .. 24) slot sets, set q consuming symbol sym[q], with the kernel
 * fv_decode_beam would choose for such a launch under the current FV_OPT_DEBUG (same admission of `beam`, same
 * row-major tables).  Every set is given the same previous-step cut record: n entries, speculative (every entry equal to
 * theta is an undecided duplicate of the cut) or not, theta, and next_bound (the lower bound of candidate scores;
 * +inf: none).  Outputs, per set q at offset q*K (scores, back-pointers) or as listed:
 *   scores_out[nsets*K]   the step's scores (-FLT_MAX where no entry reaches a column);
 *   bp_out[nsets*K]       the winning entry's state, | FV_TEST_TIE_TAG where more than one entry attains the maximum, -1;
 *   ties_out[2*nsets*K]   *tie_count_out pairs (q, column) of the tagged cells, in any order;
 *   doubt_out[nsets*1024] columns won by a theta-valued entry of a speculative set; doubt_counts[nsets] their number
 *                         (may exceed 1024: only the first 1024 are listed);
 *   cand_out[nsets*cand_cap], cand_counts[nsets]  (cand_cap > 0) scores >= next_bound with their columns, in any order;
 *                         the count may exceed cand_cap (then the list holds cand_cap of them);
 *   variants_out          (may be NULL) the FV_TV_BEAM_* bit of the kernel that ran.
 * Overwrites the decode's per-step beam buffers and statistics counters. */
#define FV_TEST_TIE_TAG (1 << 30)
int fv_test_beam_step(fv_ctx *ctx, int beam, const fv_test_beam_set *sets, int nsets, const int *sym, int speculative,
                      float theta, float next_bound, int cand_cap, float *scores_out, int *bp_out, int *ties_out,
                      int *tie_count_out, int *doubt_out, int *doubt_counts, fv_test_cand *cand_out, int *cand_counts,
                      unsigned long long *variants_out);

/* Step-kernel instantiations (variants_out).  U = 16-byte loads per lane and chunk, DB = double-buffered in
 * registers (else the whole tile is requested up front), NWV = waves per workgroup.  Every one is reachable on an
 * MI355X (256 CUs).  The whole-tile forms of the 16-bit tables and of the packed kernel need ntiles = ceil(K / 16) <= 256
 * and a tile a workgroup's registers hold (nrows <= 8192 / 4096); the whole-tile form of the float32 table is taken only
 * under FV_OPT_DEBUG bit 2 and needs nrows <= 4096, with no condition on the CU count.  The others are selected by K, the
 * batch size and FV_OPT_DEBUG bits 2, 13, 14, 18 and 21; the beam step kernels by the launch size, B and bits 8, 9, 25, 26. */
#define FV_TV_F64_NB1        (1ull << 0)    /* trellis_step<double, 1, 2, true> */
#define FV_TV_F64_NB2        (1ull << 1)    /* trellis_step<double, 2, 2, true> */
#define FV_TV_F64_NB4        (1ull << 2)    /* trellis_step<double, 4, 2, true> */
#define FV_TV_F64_NB8        (1ull << 3)    /* trellis_step<double, 8, 2, true> */
#define FV_TV_F32_NB1        (1ull << 4)    /* trellis_step<float, 1, 4, true> */
#define FV_TV_F32_NB2        (1ull << 5)    /* trellis_step<float, 2, 4, true> */
#define FV_TV_F32_NB4        (1ull << 6)    /* trellis_step<float, 4, 4, true> */
#define FV_TV_F32_NB8        (1ull << 7)    /* trellis_step<float, 8, 4, true> */
#define FV_TV_F32_UP_NB1     (1ull << 8)    /* trellis_step<float, 1, 16, false> */
#define FV_TV_F32_UP_NB2     (1ull << 9)    /* trellis_step<float, 2, 16, false> */
#define FV_TV_F16_NB1        (1ull << 10)   /* trellis_step<half_t, 1, 2, true> */
#define FV_TV_F16_NB2        (1ull << 11)   /* trellis_step<half_t, 2, 2, true> */
#define FV_TV_F16_NB4        (1ull << 12)   /* trellis_step<half_t, 4, 2, true> */
#define FV_TV_F16_NB8        (1ull << 13)   /* trellis_step<half_t, 8, 2, true> */
#define FV_TV_F16_UP_NB1     (1ull << 14)   /* trellis_step<half_t, 1, 16, false> */
#define FV_TV_F16_UP_NB2     (1ull << 15)   /* trellis_step<half_t, 2, 16, false> */
#define FV_TV_Q16_NB1        (1ull << 16)   /* trellis_step<q16_t, 1, 2, true> */
#define FV_TV_Q16_NB2        (1ull << 17)   /* trellis_step<q16_t, 2, 2, true> */
#define FV_TV_Q16_NB4        (1ull << 18)   /* trellis_step<q16_t, 4, 2, true> */
#define FV_TV_Q16_NB8        (1ull << 19)   /* trellis_step<q16_t, 8, 2, true> */
#define FV_TV_Q16_UP_NB1     (1ull << 20)   /* trellis_step<q16_t, 1, 16, false> */
#define FV_TV_Q16_UP_NB2     (1ull << 21)   /* trellis_step<q16_t, 2, 16, false> */
#define FV_TV_SLAB_F64       (1ull << 22)   /* trellis_step<double, *> in slabs of source rows */
#define FV_TV_SLAB_F32       (1ull << 23)   /* trellis_step<float, *> in slabs of source rows */
#define FV_TV_SLAB_F16       (1ull << 24)   /* trellis_step<half_t, *> in slabs of source rows */
#define FV_TV_SLAB_Q16       (1ull << 25)   /* trellis_step<q16_t, *> in slabs of source rows */
#define FV_TV_U16_W16_UP_NB1 (1ull << 26)   /* trellis_step_u16<1, 8, false, 16> */
#define FV_TV_U16_W16_UP_NB2 (1ull << 27)   /* trellis_step_u16<2, 8, false, 16> */
#define FV_TV_U16_W16_UP_NB4 (1ull << 28)   /* trellis_step_u16<4, 8, false, 16> */
#define FV_TV_U16_W16_UP_NB8 (1ull << 29)   /* trellis_step_u16<8, 8, false, 16> */
#define FV_TV_U16_W16_NB1    (1ull << 30)   /* trellis_step_u16<1, 2, true, 16> */
#define FV_TV_U16_W16_NB2    (1ull << 31)   /* trellis_step_u16<2, 2, true, 16> */
#define FV_TV_U16_W16_NB4    (1ull << 32)   /* trellis_step_u16<4, 2, true, 16> */
#define FV_TV_U16_W16_NB8    (1ull << 33)   /* trellis_step_u16<8, 2, true, 16> */
#define FV_TV_U16_W8_UP_NB1  (1ull << 34)   /* trellis_step_u16<1, 16, false, 8> */
#define FV_TV_U16_W8_UP_NB2  (1ull << 35)   /* trellis_step_u16<2, 16, false, 8> */
#define FV_TV_U16_W8_UP_NB4  (1ull << 36)   /* trellis_step_u16<4, 16, false, 8> */
#define FV_TV_U16_W8_UP_NB8  (1ull << 37)   /* trellis_step_u16<8, 16, false, 8> */
#define FV_TV_U16_W8_NB1     (1ull << 38)   /* trellis_step_u16<1, 2, true, 8> */
#define FV_TV_U16_W8_NB2     (1ull << 39)   /* trellis_step_u16<2, 2, true, 8> */
#define FV_TV_U16_W8_NB4     (1ull << 40)   /* trellis_step_u16<4, 2, true, 8> */
#define FV_TV_U16_W8_NB8     (1ull << 41)   /* trellis_step_u16<8, 2, true, 8> */
#define FV_TV_SPARSE_NB1     (1ull << 42)   /* trellis_step_sparse<1> */
#define FV_TV_SPARSE_NB2     (1ull << 43)   /* trellis_step_sparse<2> */
#define FV_TV_SPARSE_NB4     (1ull << 44)   /* trellis_step_sparse<4> */
#define FV_TV_SPARSE_NB8     (1ull << 45)   /* trellis_step_sparse<8> */
#define FV_TV_BEAM_W4        (1ull << 46)   /* beam_step<4> */
#define FV_TV_BEAM_W16       (1ull << 47)   /* beam_step<16> */
#define FV_TV_BEAM_Q16_W8    (1ull << 48)   /* beam_step_q16<8> */
#define FV_TV_BEAM_Q16_W16   (1ull << 49)   /* beam_step_q16<16> */
/* Models set by fv_set_model_sparse: trellis_step_csr<NB, MEM> (MEM: score rows read from memory instead of LDS — K beyond
 * one LDS row, a batch whose NB rows do not fit, or FV_OPT_DEBUG bit 31).  No dense-set model launches them. */
#define FV_TV_CSR_SHIFT      50
#define FV_TV_CSR_LDS_NB1    (1ull << (FV_TV_CSR_SHIFT + 0))   /* trellis_step_csr<1, false> */
#define FV_TV_CSR_LDS_NB2    (1ull << (FV_TV_CSR_SHIFT + 1))   /* trellis_step_csr<2, false> */
#define FV_TV_CSR_LDS_NB4    (1ull << (FV_TV_CSR_SHIFT + 2))   /* trellis_step_csr<4, false> */
#define FV_TV_CSR_LDS_NB8    (1ull << (FV_TV_CSR_SHIFT + 3))   /* trellis_step_csr<8, false> */
#define FV_TV_CSR_MEM_NB1    (1ull << (FV_TV_CSR_SHIFT + 4))   /* trellis_step_csr<1, true> */
#define FV_TV_CSR_MEM_NB2    (1ull << (FV_TV_CSR_SHIFT + 5))   /* trellis_step_csr<2, true> */
#define FV_TV_CSR_MEM_NB4    (1ull << (FV_TV_CSR_SHIFT + 6))   /* trellis_step_csr<4, true> */
#define FV_TV_CSR_MEM_NB8    (1ull << (FV_TV_CSR_SHIFT + 7))   /* trellis_step_csr<8, true> */

#ifdef __cplusplus
}
#endif
#endif
