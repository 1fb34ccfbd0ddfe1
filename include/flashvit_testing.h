/*
 * flashvit_testing.h — test hooks of libflashvit.so.  NOT part of the drop-in ABI of flashvit.h: no host program
 * or driver calls them, and they may change with the kernels they expose.  They exist so that the test suite can
 * compare whole step outputs (every column of every score and back-pointer row, every member and slot of a step's
 * heap) with a restatement of the recurrence, instead of the T entries of a decoded path.
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
/* (ob == NULL: the passes read the rows staged by fv_set_emissions, row t for time t, as the decodes do; T <= staged rows.) */

/* FV_OPT_FLAT_GENERATIONS: a deterministic mis-speculation.  Before the right-hand passes of a flat decode start, entry t of
 * the snapshot S of the whole-sequence chain is replaced by (S[t] + 1) % K, so every pass that reads position t (as its
 * L - 1 or its R) runs from a wrong state, the resolver reports its generation, and the decode finishes generation by
 * generation from there.  Results never change.  t = -1 clears; the setting stays until cleared. */
int fv_test_flat_poison(fv_ctx *ctx, int t);

/* Device memory for tests of the calls that take a device pointer (fv_set_emissions): the test process has no HIP
 * runtime of its own to allocate with.  `bytes` of device memory on the context's GPU in *out, filled from host_src
 * unless that is NULL; the copy is complete on return.  The free hook waits for nothing but the device. */
int fv_test_device_alloc(fv_ctx *ctx, size_t bytes, const void *host_src, void **out);
int fv_test_device_free(fv_ctx *ctx, void *p);

/* The staging kernel of fv_set_emissions alone, timed on the device: one warm launch, then `reps` launches back to back
 * of stage_emissions<TIN, TIED> between two events on the context's stream, over the T x K block at dev_scores (a device
 * pointer on the context's GPU, row pitch ld, dtype as for fv_set_emissions, the 16-bit types included); while an
 * emission map is set it is the tied form over a T x P block, ld >= P.  *ms_out is the mean per launch, dispatch
 * gaps included.  Nothing is staged afterwards (the tables are overwritten and the values are not judged).  FV_ERR_ARG: no
 * model, a host pointer, T < 1, ld < K (ld < P with a map), reps < 1, a bad dtype, a multi-device context.  For
 * tools/bench_emissions.py and tools/bench_emissions_tied.py. */
int fv_test_stage_emissions_ms(fv_ctx *ctx, const void *dev_scores, int dtype, int T, long long ld, int reps, float *ms_out);

/* The host builders of fv_set_model (A != NULL) or fv_set_model_sparse (A == NULL: row_ptr, col, val) alone: no context, no
 * GPU.  Returns the builder's return code and, of every host table it made, the FNV-1a 64-bit digest of its bytes:
 *   dense  digests[10]  h64 h32 h16 hq sp sp_off sp_nwb b64 b32 pi64   (the tile-major tables of log A in float64, float32,
 *                       binary16 and Q16 codes, the CSC-Q16 table with its tile offsets and wave-block counts, log B, log Pi)
 *   CSR    digests[9]   ck cq c64 off nwb rlog b64 b32 pi64             (source states, codes and logs by destination column,
 *                       the tiles' offsets and wave-block counts, the logs in the caller's order)
 *   params[5]           window16, windowq, qscale, density, any_big (0 / 1)
 *   detail              (may be NULL) the refusal's sentence, at most detail_cap - 1 characters; empty without one.
 * A table the builder did not make (a refusal, K beyond a kernel's limit) digests as the empty string.  FV_ERR_ARG without
 * a sentence: a NULL array, K < 1 or M < 1. */
int fv_test_model_digest(const float *A, const long long *row_ptr, const int *col, const float *val, const float *B,
                         const float *Pi, int K, int M, unsigned long long *digests, double *params, char *detail,
                         int detail_cap);

/* The two passes of fv_posteriors alone (same admission, same kernels, same launches), then their T x K float64 rows copied
 * back: alpha_out[t * K + j] and beta_out[t * K + i] as defined in flashvit.h.  Either pointer may be NULL.  Returns what
 * fv_posteriors returns (FV_ERR_NO_PRED with the rows still copied).  It exists so that a failing step can be located. */
int fv_test_sumprod_rows(fv_ctx *ctx, const int *ob, int T, double *alpha_out, double *beta_out);

/* The step-kernel instantiations the last fv_loglik, fv_loglik_batch, fv_posteriors or fv_test_sumprod_rows launched, as FV_SPF_*
 * bits (recorded on the host, launch by launch; scale launches, init rows, final sums and the gamma kernel are not step
 * kernels).  FV_ERR_ARG: a NULL pointer; FV_ERR_STATE: no such call has run.  Three bits per family, for NB = 1, 2, 4 tasks:
 * bit (shift + 0), (shift + 1), (shift + 2). */
#define FV_SPF_DENSE_SHIFT         0    /* sumprod_step<NB>: a model set by fv_set_model, forward and backward */
#define FV_SPF_CSR_FWD_LDS_SHIFT   3    /* sumprod_step_csr<NB, false>: fv_set_sparse_sumprod, scaled rows staged in LDS */
#define FV_SPF_CSR_FWD_MEM_SHIFT   6    /* sumprod_step_csr<NB, true>: scaled rows left in memory by the scale launch */
#define FV_SPF_CSR_BACK_LDS_SHIFT  9    /* sumprod_back_csr<NB, false> */
#define FV_SPF_CSR_BACK_MEM_SHIFT  12   /* sumprod_back_csr<NB, true> */
#define FV_SPF_FAMILY(shift)       (7ull << (shift))
int fv_test_sumprod_forms(const fv_ctx *ctx, unsigned long long *mask_out);

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

/* One row of a select launch: K scores and, optionally, the candidate list beam_step's epilogue would have left for the
 * step — cand_count entries {value, state} in any order, states in [0, K).  cand_count may exceed the list capacity
 * (*cand_cap_out): cand then holds capacity entries, as an overflowed list does.  cand = NULL: no list. */
typedef struct { const float *scores; const fv_test_cand *cand; int cand_count; } fv_test_select_set;

/* One select launch of a FLASH-BS lock-step — everything between "a step's K scores are finished" and "the next step's slot
 * set is staged" — over nsets (1 .. 64) caller-given score rows of K states each, through the launch rule fv_decode_beam
 * uses (launch_beam_select: kernel family and instantiation by K, beam, s, the number of rows and the list capacity;
 * FV_OPT_DEBUG bits 7, 10, 15, 20, 22, 24; FV_OPT_SEL_MARGIN) and the admission of `beam` it uses, with the hook's K in
 * place of the model's.  The context needs no model: a selection reads no table.  More than 24 rows take the form whose
 * jobs are derived on the device from the pass list.
 *   s            lock-step of the launch: 0 no previous cut; 1 a previous cut, the predictor's margin not carried; 2 as a
 *                decode's steps >= 2 (list kernels, margin carried, lists counted as short / long);
 *   prev_theta, prev_margin   (s >= 1) the previous step's cut record, always non-speculative, CUT_N = beam;
 *   seed         NULL, or {the cut an earlier generation's pass left at this time, the one it left at the next time}: what
 *                the seeded predictor reads.  NULL leaves both NaN, as the whole-sequence pass finds them.
 * Every row is a clean step (no doubtful columns, the previous step decided), at a time slot of its own in the context's
 * per-step buffers such that no row's records — its cut, the previous one, the next slot the predictor reads — are another's.
 * Lists are taken only where a decode has one: *cand_cap_out > 0 (cand_cap_for(K, beam), 0 under FV_OPT_DEBUG bit 10) and
 * s >= 1.  nsets = 0 makes no launch and reports *cand_cap_out only.
 * Outputs (P = beam + 32, the pitch of a member list):
 *   cut_out[nsets*8]            the cut record: [0] theta, [1] state (0 exact / 1 speculative / 2 exact, replayed: slot
 *                               order), [2] the bound predicted for the next cut, [3] list length seen, [4] N, [5] margin;
 *   member_val_out[nsets*P], member_state_out[nsets*P]   the N member entries in the order written; the rest NaN / -1;
 *   counters_out[8]             totals of the device counters 2 (exact replays), 5 (broken hand-shakes), 7 (selects on a list),
 *                               9 (speculative steps), 10 (reach events), 11 / 12 (lists too short / overflowed), 13 (list entries);
 *   slot_val_out[nsets*beam], slot_state_out[nsets*beam]   (want_layout) the exact heap layout of every row, slot order:
 *                               heap_build_all over the same rows with no gate;
 *   selects_out                 (may be NULL) the FV_TS_* bits of the kernels that launched.
 * FV_ERR_ARG / FV_ERR_UNSUPPORTED before any device work: beam < 2, beam > K, a beam the beam path does not admit, s
 * outside 0 .. 2, nsets outside 0 .. 64, a list where a decode has none, a negative count, a list state outside [0, K), a
 * multi-device context.
 * What needs real consecutive steps of a model — dirty steps, doubtful_reach, resolve_upto, patch_doubtful, beam_resolve,
 * tie_fixup, beam_end_backtrack — is exposed by fv_test_beam_forward below.
 * Overwrites the decode's per-step beam buffers and statistics counters. */
int fv_test_beam_select(fv_ctx *ctx, int K, int beam, int s, const fv_test_select_set *sets, int nsets, float prev_theta,
                        float prev_margin, const float *seed, int want_layout, int *cand_cap_out, float *cut_out,
                        float *member_val_out, int *member_state_out, unsigned long long *counters_out, float *slot_val_out,
                        int *slot_state_out, unsigned long long *selects_out);

/* One FLASH-BS pass over [L, R].  init_state < 0: the init row starts from Pi (at L > 0 too: what a pass reads after a beam
 * miss, Ans[L-1] == -1); else from row init_state of log A.  end_state: the fixed end state the pass back-tracks from
 * (-1: none is a member, the pass misses); ignored by the whole-sequence form. */
typedef struct { int L, R, init_state, end_state; } fv_test_beam_pass;

/* What fv_test_beam_forward copies out.  Every pointer may be NULL; every array is indexed by absolute time t and is written
 * in the passes' ranges only (P = beam + 32, the pitch of a member list):
 *   scores[T*K]          rows L .. R: the init row, then every step's scores as the device holds them after the generation
 *                        (upper bounds in the doubtful columns of a step that stayed dirty);
 *   bp[T*K]              rows L+1 .. R, raw: | FV_TEST_TIE_TAG where the device still holds a tagged cell, -1 no predecessor;
 *   cut[T*8]             rows L .. R, the cut records (layout as for fv_test_beam_select);
 *   member_val[T*P], member_state[T*P]   rows L .. R, the member lists; cut[t][4] entries of row t are meaningful;
 *   doubt[T*1024], doubt_count[T]        rows L .. R: the doubtful columns each step listed (the count may exceed 1024);
 *   slot_val[T*beam], slot_state[T*beam] rows L .. R of the layout buffers: what heap_build_all left there — every row once
 *                        the layouts ran (*gate != 0 or FV_OPT_DEBUG bit 19), the last row of a whole-sequence pass always,
 *                        otherwise whatever an earlier call left;
 *   path[T]              entries L .. R of the answer array (R: the end state, picked or given);
 *   score                the whole-sequence pass's score (otherwise not written);
 *   gate                 the tie gate after the generation: != 0 if a pass's walk met a tagged cell (or under bit 19);
 *   variants, selects    the FV_TV_BEAM_* / FV_TS_* bits of the step and select kernels that launched. */
typedef struct {
    float *scores; int *bp; float *cut; float *member_val; int *member_state; int *doubt; int *doubt_count;
    float *slot_val; int *slot_state; int *path; float *score; int *gate;
    unsigned long long *variants, *selects;
} fv_test_beam_tables;

/* The caller's passes as ONE generation of the FLASH-BS driver (beam_forward + beam_pass_ends, through the sorting, the dealing to
 * stream groups and the pass-list upload a decode's generations get), then the per-step buffers copied out.  No kernel is
 * launched that a decode would not launch; the copies are made after the generation has finished.  Admission, tables and
 * workspace are fv_decode_beam's (same refusals, same symbol check; ob == NULL reads the rows staged by fv_set_emissions);
 * FV_OPT_DEBUG, FV_OPT_SEL_MARGIN and FV_OPT_SPARSE_BEAM apply as they do to a decode.  Two forms:
 *   whole        npasses == 1, L = 0, R = T - 1, init_state < 0, end_state < 0: run as generation 0 runs (end pick from the
 *                last heap's layout, score written);
 *   right-hand   1 .. 64 passes, 0 <= L < R < T, non-overlapping: run as a right-hand generation (sorted longest first,
 *                dealt to the stream groups FV_OPT_DEBUG bits 16 / 17 choose; more than 24 passes split the step launches
 *                and take the select's derived-job form).  Before the generation starts end_state is written to ans[R] and
 *                init_state to ans[L-1] (L > 0), where the init rows and the pass ends read them; two passes whose ranges
 *                touch must agree on the entry they share (the left one's end_state is the right one's init_state).
 * Returns FV_OK, or FV_WARN_BEAM_MISS if a pass's answer entries hold -1.  FV_ERR_ARG: a bad range or overlap, a state outside
 * [-1, K), init_state >= 0 at L = 0, touching passes that disagree, a symbol outside [0, M), or a multi-device, partitioned
 * or communicator context.  fv_last_stats afterwards describes this call (the beam counters included). */
int fv_test_beam_forward(fv_ctx *ctx, const int *ob, int T, int beam, const fv_test_beam_pass *passes, int npasses,
                         const fv_test_beam_tables *out);

/* Select-kernel instantiations (selects_out): recorded on the host, only during a hook call.  R = rounds of 1024 keys held in
 * registers; LISTED: job descriptors in the kernel arguments (<= 24 rows), DERIVED: from the pass list on the device. */
#define FV_TS_SEL4_LISTED     (1ull << 0)    /* topb_select<4, true>: K <= 4096 */
#define FV_TS_SEL4_DERIVED    (1ull << 1)    /* topb_select<4, false> */
#define FV_TS_SEL16_LISTED    (1ull << 2)    /* topb_select<16, true>: K <= 16384 */
#define FV_TS_SEL16_DERIVED   (1ull << 3)    /* topb_select<16, false> */
#define FV_TS_SEL64_LISTED    (1ull << 4)    /* topb_select<64, true>: K <= 65536, steps without a list */
#define FV_TS_SEL64_DERIVED   (1ull << 5)    /* topb_select<64, false> */
#define FV_TS_CAND8_LISTED    (1ull << 6)    /* topb_select_cand<8, true>: K > 16384 at s >= 2, any step at K > 65536 or under bit 22 */
#define FV_TS_CAND8_DERIVED   (1ull << 7)    /* topb_select_cand<8, false> */
#define FV_TS_CAND16_LISTED   (1ull << 8)    /* topb_select_cand<16, true>: the same with a list capacity above 8192 (beam > 1024) */
#define FV_TS_CAND16_DERIVED  (1ull << 9)    /* topb_select_cand<16, false> */
#define FV_TS_HEAP_BUILD_ALL  (1ull << 10)   /* heap_build_all (want_layout) */
#define FV_TS_ALL             ((1ull << 11) - 1)

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
/* A model set by fv_set_model_sparse under FV_OPT_SPARSE_BEAM: beam_scatter_csr + beam_finish_csr, whatever the launch size
 * (same outputs as documented for fv_test_beam_step).  Every position of the 64-bit mask is assigned, so the route is
 * reported as the PAIR of the two float64 beam-step bits, which no launch of the dense kernels sets together (a launch
 * runs one instantiation). */
#define FV_TV_BEAM_CSR       (FV_TV_BEAM_W4 | FV_TV_BEAM_W16)
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
/* The float64 walk of the same models (FV_KERNEL_CSR_F64): trellis_step_csr_f64<NB, MEM>.  Six bits were left, so the
 * NB x MEM grid above does not fit: one bit per NB, and FV_TV_CSR64_MEM set IN ADDITION by every launch that read its
 * score rows from memory. */
#define FV_TV_CSR64_SHIFT    58
#define FV_TV_CSR64_NB1      (1ull << (FV_TV_CSR64_SHIFT + 0))   /* trellis_step_csr_f64<1, *> */
#define FV_TV_CSR64_NB2      (1ull << (FV_TV_CSR64_SHIFT + 1))   /* trellis_step_csr_f64<2, *> */
#define FV_TV_CSR64_NB4      (1ull << (FV_TV_CSR64_SHIFT + 2))   /* trellis_step_csr_f64<4, *> */
#define FV_TV_CSR64_NB8      (1ull << (FV_TV_CSR64_SHIFT + 3))   /* trellis_step_csr_f64<8, *> */
#define FV_TV_CSR64_MEM      (1ull << (FV_TV_CSR64_SHIFT + 4))   /* trellis_step_csr_f64<*, true> */
/* Not an instantiation but a route: set IN ADDITION by every trellis_step_u16 launch whose prologue copied the score codes
 * its producers left (FV_OPT_ROW_CODES) instead of quantising the float rows.  Never set while that option resolves to off,
 * as it does for fv_test_forward under auto.  While the option is off no launch reads or writes codes, and a single-task
 * bit (FV_TV_U16_*_NB1) WITHOUT this one stands for the instantiation that has no code for the route at all
 * (trellis_step_u16<1, *, *, *, false>); beside FV_TV_ROW_CODES the same bit stands for the form that holds both
 * prologues and the code-writing tail. */
#define FV_TV_ROW_CODES_SHIFT 63
#define FV_TV_ROW_CODES      (1ull << FV_TV_ROW_CODES_SHIFT)

#ifdef __cplusplus
}
#endif
#endif
