/*
 * flashvit.h — C ABI of libflashvit.so, the MI355X (gfx950) implementation of the
 * FLASH / FLASH-BS Viterbi hot path.  extern "C", plain pointers and sizes only.
 *
 * The reference has no library API: its seam is `void calc(void)` over the globals
 * `VIT *vit; ThreadPool pool;` (reference src/FLASH_Viterbi_multithread.c:45-46,338-368;
 * src/FLASH_BS_Viterbi_multithread.c:47-48,548-577), called once from main() inside
 * the clock_gettime bracket (:375-377).  Each entry point below names the piece of
 * that seam it replaces.  Caller owns every host buffer passed in or out; the
 * library never frees caller memory; one ctx is not thread-safe; functions return
 * 0 on success, >0 for warnings that still deliver the reference's result, <0 for
 * errors (never abort, never perror-and-continue as the reference's loader does).
 */
#ifndef FLASHVIT_H
#define FLASHVIT_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fv_ctx fv_ctx;

enum {
    FV_OK = 0,
    /* Find_T3_State returned -1 in some task (FLASH_BS:73-86,466-471): the path holds -1
     * entries and later tasks restart from Pi, exactly what the reference binary prints. */
    FV_WARN_BEAM_MISS = 1,
    FV_ERR_ARG = -1,         /* bad pointer / size; T == 2*n_split with n_split > 2 */
    FV_ERR_NOMEM = -2,       /* host or device allocation failed */
    FV_ERR_NO_PRED = -3,     /* a decoded entry has no finite predecessor (reference: T2[cur][-1], UB) */
    FV_ERR_DEVICE = -4,      /* a HIP call failed; fv_last_error_detail() has the text */
    FV_ERR_STATE = -5,       /* decode before fv_set_model, comm calls out of order */
    FV_ERR_UNSUPPORTED = -6, /* size or kernel choice outside what the kernels are built for: a filter kernel forced for a model it
                                cannot take (entries above 1; a score row beyond LDS), a beam width whose heap does not fit LDS.
                                K itself is bounded by device memory only */
    FV_ERR_COMM = -7,        /* RCCL failure */
};

/* `mode` argument of the decode calls. */
enum {
    /* Replays the reference's divide-and-conquer task tree pass for pass (top-level N-way
     * pass, then every bisection task whose rounding history differs from its parent's),
     * so every float the reference compares is reproduced: bit-exact paths by construction. */
    FV_MODE_REFERENCE = 0,
    /* One forward pass over [0,T-1] with full back-pointers + one backtrack.  Equal to the
     * reference in exact arithmetic; float rounding histories of right-hand sub-tasks differ,
     * so equality with the reference binary is empirical (it held on every fixture).
     * fv_decode_beam: ordinary one-pass beam search — NOT the reference's result, whose right-hand
     * tasks re-run the beam conditioned on Ans[mid] and can leave the first pass's beam. */
    FV_MODE_SINGLE_PASS = 1,
};

/* fv_set_option keys. */
enum {
    FV_OPT_KERNEL = 1,      /* FV_KERNEL_* : which trellis-step kernel streams the transition table */
    FV_OPT_MAX_BATCH = 2,   /* 1..8: most independent tasks advanced by one step launch */
    FV_OPT_PROFILE = 3,     /* 0/1: bracket every step launch with HIP events (fills step_kernel_ms) */
    FV_OPT_SEL_MARGIN = 4,  /* FLASH-BS: margin, in 1/1000 of the beam spread (max - cut value), below the extrapolated cut value
                               from which the step kernels collect the next select's candidates (default 300; the margin then follows the
                               length of the lists it produces); speed only */
    FV_OPT_FLAT_GENERATIONS = 5, /* fv_decode_full, FV_MODE_REFERENCE: 0 off, 1 auto (default), 2 on.  On: after the whole-sequence
                               pass the right-hand passes of ALL generations run as one independent set, each conditioned on the
                               states the whole-sequence chain holds at L-1 and R instead of the answers of the generation before;
                               a one-workgroup resolver then commits the chains generation by generation for as long as those
                               states equal the committed answers, and from the first generation where one differs the decode
                               finishes generation by generation as with 0.  A pass is a function of (L, R,
                               start state, end state, observations), so the result is bit for bit that of 0: speed only.  Auto:
                               on for the packed 16-bit kernel's three-stream form when K >= 512, T <= 1024 and the plan has more than one
                               right-hand generation (where it was measured to win; longer sequences gain little and pay a whole
                               fall-back for one missed pass).  Never taken (today's path instead) by multi-rank, partitioned or multi-device contexts,
                               fv_decode_full_batch, FV_OPT_PROFILE, FV_MODE_SINGLE_PASS, fv_decode_vanilla / _checkpoint,
                               FV_OPT_DEBUG bit 6, or when the device has no room for the extra workspace (score rows of all
                               right-hand passes, private arg rows of the generations >= 2, the snapshot and the chains) */
    FV_OPT_ROW_CODES = 6,   /* the packed 16-bit step kernel (FV_KERNEL_U16_REFINE): 0 off, 1 auto (default), 2 on wherever that kernel
                               runs.  On: the kernel leaves, beside every score row it writes, the row's 16-bit codes relative to the
                               maximum of their 16-column tile and those maxima, and a launch all of whose incoming rows have them
                               copies them (one saturating add per pair) instead of folding the row maximum and quantising the
                               float row again in every workgroup.  The refine window of such a launch is 1.1 code
                               units wider; paths, scores and return codes are those of 0: speed only.  Auto: the batched launches
                               (right-hand passes) of fv_decode_full of one sequence at K >= 2048, where the route was measured to
                               win; the single-task launches of the whole-sequence pass lose on it and keep their prologue.  Smaller
                               models, fv_decode_full_batch and the test hooks take the route under 2 only.  3 / 4 (measurements):
                               only single-task / only batched launches take it.  Costs 2.25 bytes per score-row entry of device memory where taken */
    FV_OPT_SPARSE_BEAM = 7, /* models set by fv_set_model_sparse: 0 (default) fv_decode_beam, fv_decode_beam_batch and fv_test_beam_step
                               answer FV_ERR_UNSUPPORTED; 1 they run, on the stored transitions: every entry of a
                               step's beam scatters its CSR row into per-column accumulators with vector atomics and a K-wide finish
                               turns them into the step's scores, back-pointers and lists; the cells the resolve code and the tie
                               fix-up re-evaluate are looked up in the rows.  Per sequence the path (with its -1 entries), the score
                               and the return / status code are bit for bit those of the same model set by fv_set_model, in both
                               modes, for every n_split and admitted beam width, ob != NULL and ob == NULL, any model values and
                               staged scores (the cell is the float64 reference expression: no filter, no condition); admission
                               is the dense-set model's.  fv_stats.kernel reports FV_KERNEL_CSR_F64, table_bytes_per_step the
                               ESTIMATE 12 * beam * nnz / K (12 bytes per stored entry of an average row; the rows actually walked
                               are the beam's).  Costs 12 bytes of device memory per (observation, state).  Any other value:
                               FV_ERR_ARG.  On a model set by fv_set_model the option changes nothing.  The default is 0 because the
                               refusals and their texts are pinned by the suite of the sparse-set model; a later change may flip it */
    FV_OPT_DEBUG = 100,     /* UNSTABLE: kernel-tuning switches (a bit mask) that select alternative forms of a kernel or of the
                               launch schedule.  Every bit the library accepts is speed-only — the parity tests run each
                               alternative against the same goldens (tests/test_boundary.py checks that no accepted value
                               changes a result).  The switches that leave a part of a kernel out to time the rest (bits 0, 4, 5,
                               11, 12 = FV_DEBUG_TIMING_ONLY) change results; they exist only in the separate timing build
                               (libflashvit_timing.so, used by tools/), and this library answers FV_ERR_ARG to them.
                               Full-state: 1 no reverse sweep, 2 alternate load schedule, 3 full last step instead of one
                               column, 6 hipGraph replay of a generation, 13 packed kernel in 16-wave workgroups, 14 packed
                               kernel for every batched launch, 18 right-hand generations on one stream, 21 F64 / F32 / F16 / Q16
                               kernels in three slabs of source rows (the route of K > 65536) at any size, 28 fv_decode_full_batch: the whole-sequence
                               passes (generation 0) in single-stream launches of up to FV_OPT_MAX_BATCH tasks instead of the
                               three-stream, four-task form (bit 27 is not assigned and refused).  FLASH-BS: 29 fv_decode_beam_batch: the whole-sequence passes
                               (generation 0) in the launch form that is not the default (one stream / dealt to the four stream groups), 7 the cut predictor uses the pass's own
                               cuts only, 8 / 9
                               float64 / 16-bit step kernel always, 10 no candidate lists, 15 whole-workgroup select for short
                               lists too, 16 / 17 pass groups on one stream / on four streams whatever the size, 19 every heap
                               layout rebuilt and every tie re-decided whether or not the path needs it, 20 every duplicate
                               step replays its heap at once (no speculative member lists), 22 every selection in the memory-resident
                               form (the route of K > 65536), 23 runs of undecided steps always decided in full, 24 four-wave select also on steps that may have to be resolved,
                               25 / 26 the 16-bit step kernel in 16-wave / 8-wave workgroups whatever the launch size (25 also: the float64
                               step kernel in 16-wave workgroups for small beams too).  Models set by fv_set_model_sparse: 31 the
                               step kernels read their score rows from memory at any K (the form of K beyond one LDS row); bit 30
                               is not assigned and refused */
};
#define FV_DEBUG_TIMING_ONLY ((1 << 0) | (1 << 4) | (1 << 5) | (1 << 11) | (1 << 12))
enum {
    FV_KERNEL_AUTO = 0,        /* every model entry in [0,1]: SPARSE_Q16 if <= 35 % of A is non-zero, else U16_REFINE;
                                  otherwise F64_STREAM */
    FV_KERNEL_F64_STREAM = 1,  /* streams log A as float64 (8 B/cell): the reference expression verbatim; any K (score rows
                                  beyond LDS are swept in slabs of source rows, one launch per slab) */
    FV_KERNEL_F32_REFINE = 2,  /* streams (float)log A (4 B/cell), brackets the winner within 2 ulp,
                                  then re-evaluates the few candidates in float64: same bits out */
    FV_KERNEL_F16_REFINE = 3,  /* same scheme with log A rounded to binary16 (2 B/cell) and a window of
                                  2*max|half(L)-L| + 3 ulp: same bits out, a quarter of the float64 bytes; the wider
                                  window costs more refines than the bytes save at K=3965 */
    FV_KERNEL_Q16_REFINE = 4,  /* same scheme with 16-bit fixed point (step = max|log A|/65534): 2 B/cell and
                                  a window ~ step: same bits out; any K (slabs of source rows, as F64_STREAM) */
    FV_KERNEL_U16_REFINE = 6,  /* the Q16 table again, but the filter itself runs in 16-bit fixed point, two cells per packed
                                  instruction (the score row is quantised with the table's step while it is staged into LDS);
                                  candidates inside the window are re-evaluated in float64 as above: same bits out.  Used
                                  for single-task launches (the whole-sequence pass) and for models whose float32 rows do not
                                  fit LDS (K up to 65536; beyond that AUTO takes Q16_REFINE in slabs); batched launches take the
                                  Q16_REFINE filter (same table, same bits) */
    FV_KERNEL_SPARSE_Q16 = 5,  /* the Q16 codes of the NON-ZERO transitions only (per destination column, ascending
                                  source state): log 0 = -inf can never win (FLASH:171), so skipping those cells
                                  changes no bit; 7.6 MB instead of 31.5 MB at K=3965, p=0.112 */
    FV_KERNEL_SPARSE_CSR = 7,  /* REPORTED ONLY (fv_stats.kernel; fv_set_option answers FV_ERR_ARG to it): the walk over the
                                  stored transitions of a model set by fv_set_model_sparse — the scheme of SPARSE_Q16 with
                                  32-bit source states, no dense table behind it */
    FV_KERNEL_CSR_F64 = 8,     /* models set by fv_set_model_sparse only: the float64 walk over the stored transitions — the
                                  reference expression on every stored entry from its float64 log (12 B per entry: 32-bit
                                  source state + float64 log), no filter and so no condition on the values: the kernel
                                  of a sparse-set model with entries above 1 or with staged emission scores above 0.  Same
                                  bits out as the same model set by fv_set_model under F64_STREAM.  On a model set by
                                  fv_set_model the full-state decodes answer FV_ERR_UNSUPPORTED to it */
};

typedef struct {
    double set_model_ms;      /* host log() tables + H2D of the last fv_set_model */
    double decode_ms;         /* host wall time of the last decode call (enqueue .. final sync) */
    double gpu_ms;            /* HIP-event time from first to last kernel of the last decode */
    double top_pass_ms;       /* HIP-event time of generation 0 (the whole-sequence pass incl. init/argmax/backtrack) */
    double top_steps_ms;      /* HIP-event time around generation 0's T-1 back-to-back step launches only */
    double step_kernel_ms;    /* sum of per-launch event times of the step kernel (FV_OPT_PROFILE=1) */
    long long step_launches;  /* trellis-step kernel launches in the last decode */
    long long task_steps;     /* sum over launches of tasks advanced by a full K*K (or K*beam) step */
    long long column_steps;   /* last steps of passes evaluated for the one destination column the back-track reads */
    long long cells;          /* add-compare cells: task_steps * K * K + column_steps * K (full) or task_steps * K * beam */
    long long alg_bytes;      /* 4 bytes per cell */
    long long table_bytes_per_step; /* bytes of transition table one step launch streams */
    long long device_bytes;   /* device working set (tables + workspace) */
    long long refine_near;    /* filter kernels: candidates inside the window besides a column's best */
    long long refine_rescan;  /* filter kernels: lanes that had to rescan their rows */
    long long beam_exact_sets;/* FLASH-BS: exact heap replays run for member sets (duplicate scores at the cut whose survivors mattered) */
    long long beam_ties;      /* FLASH-BS: (step, state) cells re-decided by slot order; 0 unless a back-tracked path met a cell
                                 whose maximum two beam entries attained (only then are the heap layouts rebuilt) */
    long long beam_dup_cols;  /* FLASH-BS statistics: columns won by an entry whose value equals a duplicated cut value */
    long long beam_dup_steps; /* ... and the number of steps in which that happened at least once */
    long long beam_cand_selects; /* FLASH-BS: top-B selections that ran on a step's candidate list instead of all K scores */
    double density;           /* non-zero fraction of the transition matrix */
    int passes;               /* forward passes run (reference mode: one per right-hand task) */
    int generations;          /* dependent batches of passes */
    int kernel;               /* FV_KERNEL_* actually used */
    int ranks;                /* ranks sharing the decode (1 without fv_comm_init) */
    long long refine_saturated; /* packed 16-bit filter: (step, column) pairs whose window reached the end of the code range, so that
                                   every source row was re-evaluated exactly (score rows spread wider than max|log A|) */
    long long beam_spec_steps;  /* FLASH-BS: steps whose cut fell on duplicated scores and that were carried speculatively (all duplicates
                                   in the member list, survivors undecided) instead of replaying the heap at once */
    long long beam_reach_events;/* FLASH-BS: selects at which an undecided duplicate's column reached the beam, so that the steps before
                                   it had to be decided (exact replays, counted in beam_exact_sets) and the selection repeated */
    long long beam_list_short;  /* FLASH-BS: selects (third step of a pass on) whose candidate list held fewer than B entries ... */
    long long beam_list_long;   /* ... or more than its capacity: both re-read all K scores */
    long long beam_list_entries;/* FLASH-BS: total length of the candidate lists the selects ran on (beam_cand_selects of them) */
    long long beam_chain_cuts;  /* FLASH-BS: runs of undecided steps that were decided only back to a step whose replay provably does not
                                   depend on the undecided columns (instead of back to the last step with exact scores) */
    int flat_passes;            /* FV_OPT_FLAT_GENERATIONS: right-hand passes run speculatively from the whole-sequence chain (0: the decode
                                   ran generation by generation) */
    int flat_missed;            /* ... passes of the first generation with a miss whose conditioning states differed from the committed
                                   answers (0: every chain was committed) */
    int flat_first_miss;        /* ... that generation (-1: none); the generations from it on were run again generation by generation, and
                                   the other statistics cover both parts */
    double set_emissions_ms;    /* host wall time of the last fv_set_emissions (copy, staging kernel, its one sync), 0 after a refused one; kept across decodes */
    long long emission_rows;    /* rows staged by fv_set_emissions (0: none); kept across decodes */
    long long bt_restarts;      /* back-tracks of 128 steps or more are walked by 64 lanes from guessed states and verified chunk by chunk:
                                   the times a chunk had entered with the wrong state and the walk below it was run again, summed over every
                                   back-track launch of the call (a flat decode's speculative passes, committed or not, and both walks of a
                                   FLASH-BS pass included); 0 when every survivor path had merged inside the warm-up */
} fv_stats;

/* Device + stream + workspace owner.  Replaces `vit = create_vit()`'s allocation role
 * (FLASH:97-107) and the ThreadPool globals (:36-46). */
int fv_create(fv_ctx **out, int device);
void fv_destroy(fv_ctx *ctx);

/* One host process, several GPUs: the reference is one process whose MAX_THREADS workers share one task queue
 * (FLASH:316-335, calc :338-368); here the workers are devices.  The returned context is used like any other
 * (fv_set_model uploads to every device, fv_set_option applies to all): a decode runs the whole-sequence pass on
 * every device (the same deterministic computation, no communication), deals the n_split top-level segments
 * (:349-353) round-robin to the devices — one host thread and one stream set per device — and merges the answer
 * arrays with ONE grouped ncclAllGather (ncclCommInitAll) of T int32 over xGMI.  A device may be listed more than
 * once (a 1-GPU lease): the control flow is the same, with device-to-device copies in place of RCCL (two RCCL ranks
 * cannot share a device).  ndev = 1 gives a plain fv_create context.  fv_last_stats reports the first device's
 * decode and `ranks` = ndev.  fv_device_count: GPUs visible to the process (0 if none). */
int fv_create_multi(fv_ctx **out, const int *devices, int ndev);
int fv_device_count(void);

/* Model upload.  A is K*K row-major A[from][to], B is K*M row-major B[state][symbol],
 * Pi is K — the VIT fields of FLASH:26-28 as InitElement filled them (:82-93).  Takes
 * log() of every entry in double with the host libm (the calls the reference makes per
 * cell, :142,150,167,170) and ships the tables; the caller keeps ownership of A/B/Pi. */
int fv_set_model(fv_ctx *ctx, const float *A, const float *B, const float *Pi, int K, int M);

/* The same model given by its non-zero transitions only, in compressed sparse row form by SOURCE state: row k is
 * A[k][col[e]] = val[e] for e in [row_ptr[k], row_ptr[k+1]).  row_ptr has K + 1 non-decreasing entries, row_ptr[0] == 0;
 * the columns of a row are strictly ascending (no duplicates) and lie in [0, K); every transition not stored is 0, and a
 * stored 0 is the same as an absent entry (log 0 = -inf can never win, FLASH:171).  B and Pi as in fv_set_model.  Value
 * rules and errors are fv_set_model's (finite, >= 0); a malformed CSR answers FV_ERR_ARG with the offending row in
 * fv_last_error_detail.  An argument error leaves the previous model in place; a failure during the upload leaves the
 * context with no model.  log((double)x) is taken per stored entry with the host libm, and the Q16 step and refine
 * window come from the finite entries alone, so a decode delivers bit for bit what the same model gives through
 * fv_set_model.  Host and device memory are O(nnz + K*M): no K*K table exists on this path (about 30 bytes of device
 * memory per stored entry), so K is bounded by the number of transitions, not by 8*K^2.
 * The context remembers how its model was set; a later fv_set_model replaces a sparse-set model and the other way round.
 * On a sparse-set model:
 *   - fv_decode_full, fv_decode_full_batch, fv_set_partition, fv_create_multi contexts and fv_test_forward work as on
 *     any model; fv_stats.kernel reports FV_KERNEL_SPARSE_CSR.  FV_OPT_KERNEL values FV_KERNEL_AUTO and
 *     FV_KERNEL_SPARSE_Q16 select that walk, FV_KERNEL_CSR_F64 the float64 walk (reported as such); any other (a kernel
 *     that streams a dense table) answers FV_ERR_UNSUPPORTED at decode.
 *   - A model with an entry above 1 is accepted here, as by fv_set_model, but under FV_KERNEL_AUTO / FV_KERNEL_SPARSE_Q16
 *     its decode answers FV_ERR_UNSUPPORTED: that walk is a filter kernel (its error bracket needs every log <= 0) and
 *     there is no dense float64 table to fall back to.  The same holds once a staged emission score is above 0.
 *     FV_KERNEL_CSR_F64 decodes both: any model values, any staged scores, ob != NULL and ob == NULL, both modes, every
 *     FV_OPT_MAX_BATCH, bit for bit what fv_set_model + FV_KERNEL_F64_STREAM deliver (path with its -1 entries, score,
 *     return code) — and so, for a model within [0,1], what the filter walk delivers.
 *   - fv_decode_vanilla: FV_ERR_UNSUPPORTED unless FV_KERNEL_CSR_F64 is selected; then the float64 walk runs with the
 *     baseline's rounding order and delivers what fv_decode_vanilla delivers on the dense-set model.
 *   - fv_decode_beam, fv_decode_beam_batch, fv_test_beam_step and fv_decode_checkpoint answer FV_ERR_UNSUPPORTED before
 *     any device work under every FV_OPT_KERNEL value, FV_KERNEL_CSR_F64 included: their kernels gather rows of the
 *     dense table.
 *   - FV_OPT_SPARSE_BEAM = 1 lifts that for the three beam calls (not for fv_decode_checkpoint): they then run on the
 *     stored rows and deliver what the dense-set model delivers, whatever FV_OPT_KERNEL says; see the option. */
int fv_set_model_sparse(fv_ctx *ctx, const long long *row_ptr, const int *col, const float *val,
                        const float *B, const float *Pi, int K, int M);

/* Per-time emission scores in place of observation symbols: for continuous-observation HMMs, neural acoustic / alignment
 * models and profile HMMs, which hold one log score per (time, state) and have no symbol alphabet.  `scores` is T rows of
 * K log scores (K is the model's), row t, state i at scores[t * ld + i], ld >= K in elements; what lies beyond K in a row
 * is never interpreted (a host block is copied as one piece up to the last row's K-th element, pads included).  dtype is
 * FV_EMIS_LOG_F32 (float), FV_EMIS_LOG_F64 (double), FV_EMIS_LOG_F16 (IEEE binary16) or FV_EMIS_LOG_BF16 (bfloat16);
 * rows of the 2-byte types need no more than 2-byte alignment (an odd ld, a block entered at an odd element).  `scores`
 * may be a host pointer or a device pointer
 * (hipPointerGetAttributes decides); work producing a device block must be complete before the call; the call returns
 * after staging, so the caller may free `scores` at once.
 *   The library keeps two device tables, E32[t][i] = (float)x in the part of (float)log(B[i][o]) (FLASH:167) and
 * E64[t][i] = (double)x in the part of log((double)B[i][o]) (init rows, vanilla / checkpoint arithmetic): for
 * FV_EMIS_LOG_F64 input of log((double)b) values exactly the tables fv_set_model builds from b.  FV_EMIS_LOG_F32,
 * FV_EMIS_LOG_F16 and FV_EMIS_LOG_BF16 are the same as passing (double)x: each of these widenings is exact.
 *   Tied scores (fv_set_emission_map): while a map is set, a row holds P class scores in place of K state scores, row t,
 * class p at scores[t * ld + p], ld >= P, and state i takes x = scores[t * ld + pdf_of_state[i]].  The tables stay T x K
 * and hold exactly what staging the expanded T x K block without a map would have put there, so everything said here of
 * values, decodes and ob == NULL holds unchanged.  A class that no state maps to is never interpreted, as a pad column.
 *   Values: finite or -inf.  A NaN, a +inf or a finite double whose float conversion is infinite answers FV_ERR_ARG, with
 * the lowest offending (t, state) in fv_last_error_detail (and its class, through a map).  A score above 0 (a density
 * above 1) is accepted and handled
 * as a B entry above 1: decodes on these emissions take FV_KERNEL_F64_STREAM under AUTO, answer FV_ERR_UNSUPPORTED to a
 * forced filter kernel and on a model set by fv_set_model_sparse (unless FV_KERNEL_CSR_F64 is selected there), and the beam
 * path takes its float64 step kernel.
 *   Returns FV_ERR_STATE without a model, FV_ERR_ARG for T < 1, ld < K (ld < P with a map), a bad dtype or a NULL pointer,
 * FV_ERR_NOMEM (the byte count in the detail, before anything is allocated) when 12 * T * K bytes plus the raw copy
 * (((T - 1) * ld + K) elements; P for K with a map) exceed the free device
 * memory.  A failed call leaves the context with no staged emissions.
 *   Use: every decode call — and fv_test_forward — given ob == NULL reads row t for time t.  The single decodes need
 * T <= staged rows; the batch decodes put sequence s on rows offsets[s] .. offsets[s+1]) and need offsets[nseq] <= staged
 * rows.  The symbol-range check does not apply; every other admission rule does.  ob == NULL with nothing staged is
 * FV_ERR_ARG.  A call with ob != NULL ignores the staged rows and decodes symbols through the model's B.
 * fv_set_model and fv_set_model_sparse drop the staged emissions; fv_clear_emissions drops them and frees the tables.
 * A fv_create_multi context stages on every member; with fv_set_partition / fv_comm_init every rank stages its own copy. */
enum { FV_EMIS_LOG_F32 = 0, FV_EMIS_LOG_F64 = 1 };
int fv_set_emissions(fv_ctx *ctx, const void *scores, int dtype, int T, long long ld);
int fv_clear_emissions(fv_ctx *ctx);
enum { FV_EMIS_LOG_F16 = 2, FV_EMIS_LOG_BF16 = 3 };
/* The emission map of a model whose K states share P score classes (senones, pdf ids, match / insert columns):
 * pdf_of_state is a HOST array of K entries in [0, P), P >= 1.  It belongs to the model as B does: uploaded once (4 * K
 * bytes per device, to every member of a fv_create_multi context), kept until replaced or cleared (pdf_of_state == NULL
 * with P == 0), dropped by fv_set_model and fv_set_model_sparse.  While it is set fv_set_emissions reads rows of P scores
 * (see there).  Setting, replacing or clearing the map drops the staged rows: they were expanded through the old one.
 *   Returns FV_ERR_STATE without a model; FV_ERR_ARG, before any device work and with a detail text, for P < 1 with a
 * map, P != 0 without one, an entry outside [0, P) (the lowest such state is named) and a device pointer
 * (hipPointerGetAttributes decides) — an argument error leaves the previous map and the staged rows in place.  An upload
 * failure leaves no map and nothing staged. */
int fv_set_emission_map(fv_ctx *ctx, const int *pdf_of_state, int P);

int fv_set_option(fv_ctx *ctx, int key, long long value);

/* calc() of FLASH_Viterbi_multithread.c:338-368 with MAX_THREADS = n_split:
 * ob[T] = vit->Obroute, path_out[T] = vit->Ans, *score_out = T1[cur][Ans[T-1]] of the
 * whole-sequence pass (the reference never prints it). */
int fv_decode_full(fv_ctx *ctx, const int *ob, int T, int n_split, int mode,
                   int *path_out, float *score_out);

/* nseq observation sequences against the model of ctx, decoded together: the reference is one process, one sequence
 * (main :370-380); a caller with many sequences for one model would run it nseq times.  Here the forward passes of
 * different sequences share the step launches (up to FV_OPT_MAX_BATCH passes per sweep of the transition table).
 * ob holds the sequences back to back; sequence s is ob[offsets[s] .. offsets[s+1]) (offsets[0] == 0, nseq + 1
 * non-decreasing entries, lengths may differ, the total below 2^31).  path_out has the same layout.  score_out (may
 * be NULL) and status_out (may be NULL) have nseq entries: per sequence exactly what
 * fv_decode_full(ctx, ob + offsets[s], T_s, n_split, mode, ...) delivers in *score_out and as its return code —
 * FV_OK, or FV_ERR_NO_PRED with the -1 entries in that sequence's path (the other sequences are intact).
 * Return: 0, or the most negative per-sequence status.  A sequence fv_decode_full would refuse (T_s < 2, a symbol
 * outside [0,M), T_s == 2*n_split with n_split > 2) fails the whole call with FV_ERR_ARG before any device work;
 * fv_last_error_detail names its index.  A context with a communicator, a partition or several devices answers
 * FV_ERR_UNSUPPORTED.  fv_last_stats reports the batch as one decode (counters are totals, `generations` the largest
 * of any sequence). */
int fv_decode_full_batch(fv_ctx *ctx, const int *ob, const long long *offsets, int nseq, int n_split, int mode,
                         int *path_out, float *score_out, int *status_out);

/* calc() of FLASH_BS_Viterbi_multithread.c:548-577 with MAX_THREADS = n_split and
 * BeamSearchWidth = beam_width (2 <= beam_width <= K). */
int fv_decode_beam(fv_ctx *ctx, const int *ob, int T, int n_split, int beam_width, int mode,
                   int *path_out, float *score_out);

/* nseq observation sequences through FLASH-BS in one call: the layout contract of fv_decode_full_batch (sequences back
 * to back, offsets[0] == 0, nseq + 1 non-decreasing entries, ragged lengths, the total below 2^31; score_out and
 * status_out may be NULL).  Per sequence s exactly what fv_decode_beam(ctx, ob + offsets[s], T_s, n_split, beam_width,
 * mode, ...) delivers: the path including the -1 entries after a beam miss, the float32 score, and in status_out[s] that
 * call's return code (FV_OK or FV_WARN_BEAM_MISS).  Return: the most negative per-sequence status if any is negative,
 * else FV_WARN_BEAM_MISS if any sequence has it, else 0.  The passes of all sequences run in lock-step and share the
 * step and select launches; the "path met a tied cell" gate that triggers the exact heap rebuilds is per sequence.
 * Refused before any device work, with the sequence index in fv_last_error_detail: T_s < 2, a symbol outside [0,M),
 * T_s == 2*n_split with n_split > 2; also a beam_width fv_decode_beam refuses, bad pointers / offsets / mode, nseq < 1
 * (FV_ERR_ARG), no model (FV_ERR_STATE), a context with a communicator, a partition or several devices
 * (FV_ERR_UNSUPPORTED), and a working set beyond the free device memory (FV_ERR_NOMEM with the byte count; the
 * per-step buffers grow with the total length: about 16 bytes per (observation, state) — DESIGN.md 5.4b).
 * fv_last_stats reports the batch as one decode (counters are totals, `generations` the largest of any sequence). */
int fv_decode_beam_batch(fv_ctx *ctx, const int *ob, const long long *offsets, int nseq, int n_split,
                         int beam_width, int mode, int *path_out, float *score_out, int *status_out);

/* GPU form of the reference's baseline programs Base_line/C implementations/vanilla Viterbi.c:125-173 and
 * checkpoint Viterbi.c (same recurrence, hence the same output): one forward pass with the BASELINE's
 * rounding order, tmp2 = (float)(((double)T1[k] + log A[k][i]) + log B[i][o]) (:140), lowest-index
 * end state, plain back-track.  An independent cross-check of the FLASH paths (its scores may differ from
 * FLASH's in the last ulp, its path equals FLASH's on every fixture) and the measure of what the
 * divide-and-conquer schedule costs on a device where T*K back-pointers fit trivially. */
int fv_decode_vanilla(fv_ctx *ctx, const int *ob, int T, int *path_out, float *score_out);

/* GPU form of Base_line/C implementations/checkpoint Viterbi.c:176-251 (viterbi_checkpoint(vit, step); step
 * <= 0 selects floor(sqrt(T)), what its main passes): a first pass that keeps the score row of every
 * step-th time only, then every segment re-run from its kept row with arg rows.  The arithmetic is
 * vanilla's, so path and score equal fv_decode_vanilla's; what differs is the work (about 2x) and the
 * memory the CPU program needs, reported by fv_checkpoint_memory_bytes as that program computes it (:250). */
int fv_decode_checkpoint(fv_ctx *ctx, const int *ob, int T, int step, int *path_out, float *score_out);
long long fv_checkpoint_memory_bytes(int K, int T, int step);

/* Online full-state decode: one stream per context consumes a sequence in pushes of any length >= 1, given
 * as symbols or as emission-score rows, and hands the decoded path back piece by piece, each piece as soon as no later
 * input can change it.  The concatenation of all pieces (the pushes', then the close's), the final score and the final
 * return code are bit for bit those of fv_decode_full(ctx, ob, T, 1, FV_MODE_SINGLE_PASS, ...) on the concatenated
 * input whenever that call returns FV_OK — for every chunking, every check interval, every FV_OPT_KERNEL value the
 * one-shot call admits for the model, dense-set and CSR-set models.  A piece, once returned, is final.  Device memory
 * is O((largest push + lag) * K), lag = times consumed and not yet committed: never O(T * K).
 *   The rule.  The device keeps the two score rows, the arg rows of the uncommitted times and one row anc[K]: the state
 * at the anchor time a on the survivor path of every state of the current time (a = 0, anc[s] = s at first; after a
 * step with arg row bp, anc'[s] = bp[s] >= 0 ? anc[bp[s]] : -1).  A check — every check_every steps counted from the
 * check before, and after the last step of every push — looks at the set V of non-negative anc values.  One element v:
 * every path that can still be decoded runs through (a, v), so the times up to a are committed by a back-track from
 * (a, v), their arg rows are dropped, and the anchor moves to the current time.  V empty: no state has a predecessor
 * (below).  Otherwise nothing happens.  The check runs on the device, between the steps of a push, without the host.
 *   fv_stream_open: needs a model; the step kernel and its admission are fv_decode_full's for that model under the
 * FV_OPT_KERNEL in force (FV_ERR_UNSUPPORTED with the same detail), fixed for the stream's life.  lag_rows_hint: arg
 * rows to allocate at first (0: a default; the buffer doubles whenever a push needs more).  check_every: 1..64, 0: the
 * default (16).  FV_ERR_STATE: no model, or a stream is already open.  FV_ERR_UNSUPPORTED: multi-device, partitioned
 * and communicator contexts.  FV_ERR_ARG: lag_rows_hint < 0, check_every outside 0..64.
 *   fv_stream_push: n >= 1 times given as symbols of [0, M).  fv_stream_push_emissions: n >= 1 times given as score
 * rows — dtype, ld, host or device pointer, emission map (rows of P classes while one is set) and value rules exactly
 * as fv_set_emissions; the context's staged emissions are left alone.  The first push fixes which of the two the stream
 * takes; the other kind afterwards is FV_ERR_ARG.  path_out must hold fv_stream_pending(ctx) + n entries;
 * *committed_out of them are written: the next piece of the path, possibly none.
 *   A refused push consumes nothing, runs no step and leaves the stream as it was: FV_ERR_ARG for a bad pointer, n < 1,
 * a symbol outside [0, M), ld or dtype as fv_set_emissions refuses them, a NaN / +inf / out-of-range score (the detail
 * names its time, counted from the stream's start, and state); FV_ERR_UNSUPPORTED for a score above 0 when the stream's
 * kernel is a filter kernel (select FV_KERNEL_F64_STREAM, or FV_KERNEL_CSR_F64 on a CSR-set model, before the open);
 * FV_ERR_NOMEM, with the byte count, when the arg rows cannot grow.  FV_ERR_STATE without a stream.
 *   V empty at a check: the push returns FV_ERR_NO_PRED, as the one-shot decode of any sequence with this prefix
 * does.  The pieces already returned stand; the stream then accepts only fv_stream_close, which returns FV_ERR_NO_PRED
 * and delivers nothing, and fv_stream_abort; a push answers FV_ERR_STATE.
 *   fv_stream_pending: times consumed and not yet committed; < 0 without a stream.
 *   fv_stream_close: the end of the input — the end pick (lowest index among the maxima of the current score row), the
 * back-track of everything pending into path_out (fv_stream_pending entries, *n_out their number), *score_out as
 * fv_decode_full's (score_out may be NULL).  A stream that consumed one time delivers that time's end pick on the
 * init row; one that consumed nothing delivers nothing.  Frees the stream's buffers, whatever it returns.
 *   fv_stream_abort: drops the stream and delivers nothing.  fv_destroy frees an open stream.
 *   While a stream is open the decode calls, fv_set_model, fv_set_model_sparse, fv_set_option, fv_set_emissions,
 * fv_clear_emissions, fv_set_emission_map, fv_set_partition, fv_comm_init and the test hooks (all but
 * fv_test_device_alloc / fv_test_device_free, which a push from a device block needs) answer FV_ERR_STATE.
 * fv_last_stats keeps reporting the last decode; the stream has its own statistics. */
int fv_stream_open(fv_ctx *ctx, long long lag_rows_hint, int check_every);
int fv_stream_push(fv_ctx *ctx, const int *ob, int n, int *path_out, long long *committed_out);
int fv_stream_push_emissions(fv_ctx *ctx, const void *scores, int dtype, int n, long long ld,
                             int *path_out, long long *committed_out);
long long fv_stream_pending(const fv_ctx *ctx);
int fv_stream_close(fv_ctx *ctx, int *path_out, long long *n_out, float *score_out);
int fv_stream_abort(fv_ctx *ctx);

/* Statistics of the open stream, or of the last one closed or aborted (FV_ERR_STATE: there never was one). */
typedef struct {
    long long times;             /* times consumed */
    long long committed;         /* times whose path entry has been returned */
    long long pushes;            /* accepted pushes */
    long long checks;            /* checks run (a check is two small launches: the ancestor walk and its verdict) */
    long long commits;           /* checks that found one ancestor and moved the anchor */
    long long lag_max;           /* largest number of pending times at the end of a push */
    long long arg_rows_capacity; /* arg rows allocated */
    long long regrows;           /* times the arg rows were reallocated at twice the need */
    long long bt_restarts;       /* as fv_stats.bt_restarts, summed over the stream's back-tracks */
    double push_ms_total;        /* host wall time of the accepted pushes, their synchronisations included */
    int kernel;                  /* FV_KERNEL_* the steps run on */
} fv_stream_stats;
int fv_stream_last_stats(const fv_ctx *ctx, fv_stream_stats *out);

/* Many online streams on one context.
 * A set of nslots online streams ("slots", ids 0 .. nslots-1) on one context: fv_stream_*'s contract per slot, the steps of
 * the slots named in one push call sharing their step launches and checks.
 *   The contract.  Per slot — whatever the other slots do, however the calls group the slots, whatever batch_cap is — the
 * pieces, the committed count after every call the slot took part in, the final score and the return codes are bit for bit
 * those of the same pushes through fv_stream_* on a context of its own, so their concatenation is
 * fv_decode_full(..., 1, FV_MODE_SINGLE_PASS)'s result; the slot's fv_stream_stats counters times, committed, pushes, checks,
 * commits, lag_max and bt_restarts equal that stream's.  The check rule is per slot and unchanged: a check every check_every
 * steps of that slot counted from its last check, and after the last step of each of its pushes.
 *   fv_streams_open: nslots in 1 .. 64; lag_rows_hint and check_every exactly as fv_stream_open, applied to every slot;
 * admission and kernel choice as there, fixed for the set's life.  batch_cap, the tasks one step launch takes, is the
 * smaller of FV_OPT_MAX_BATCH at the open and what fv_decode_full_batch would take for the model (with FV_OPT_MAX_BATCH = 1
 * every step is a single-task launch).  A set and the single stream exclude each other: each open answers FV_ERR_STATE
 * while the other is open, and while a set is open everything that answers FV_ERR_STATE under an open stream does so too.
 * FV_ERR_UNSUPPORTED: multi-device, partitioned and communicator contexts.
 *   fv_streams_push: ids[0 .. nids) are distinct slots; slot ids[q] consumes ob[offsets[q] .. offsets[q+1]) — the offsets
 * contract of the batch decodes (offsets[0] = 0), every length >= 1; a slot with nothing to push is left out of the call.
 * The first push into an empty slot starts a new sequence there (time 0 from Pi) and fixes its kind, symbols or score
 * rows.  path_offsets has nids + 1 entries: slot ids[q]'s piece is written at path_out + path_offsets[q], committed_out[q]
 * is its length, and the room path_offsets[q+1] - path_offsets[q] must be at least fv_streams_pending(ctx, ids[q]) + n_q.
 * status_out[q] (status_out may be NULL) is what fv_stream_push would return for that slot, FV_OK or FV_ERR_NO_PRED; the
 * call returns the most negative status.  A dead slot does not disturb the others; it then accepts only fv_streams_close
 * (FV_ERR_NO_PRED, nothing delivered) and fv_streams_abort, and naming it in a push refuses the call with FV_ERR_STATE.
 *   A refused call consumes nothing in any slot, runs no step and leaves every slot as it was: FV_ERR_ARG for bad
 * pointers, nids < 1, an id outside the set or named twice, a length below 1, a symbol outside [0, M), the other kind of
 * input for a slot that has one, too little room; FV_ERR_NOMEM for a refused growth of arg rows.  fv_last_error_detail
 * names the slot and, where it applies, the time counted from that slot's sequence start.
 *   fv_streams_push_emissions: scores is one block, slot ids[q]'s rows are its rows offsets[q] .. offsets[q+1]), one dtype
 * and one ld; host or device pointer, emission map and value rules exactly as fv_stream_push_emissions.  The block is
 * staged in one launch and its flags are read once, before any step: a NaN, a +inf or an out-of-range score anywhere
 * refuses the whole call (FV_ERR_ARG; the detail names slot, time and state of the lowest offending staged index), a
 * score above 0 under a filter kernel refuses it with FV_ERR_UNSUPPORTED.
 *   fv_streams_pending: times slot id consumed and has not yet committed; < 0 without a set or for an id outside it.
 *   fv_streams_close: fv_stream_close's work on slot id — end pick, back-track of everything pending, the score — and
 * the slot is empty and ready for a new sequence, its buffers kept: sequences come and go while other slots are in
 * mid-sequence.  An empty slot delivers nothing and returns FV_OK.  fv_streams_abort drops slot id's sequence.
 * fv_streams_end frees the whole set, whatever its slots hold; so does fv_destroy.
 *   fv_streams_slot_stats: fv_stream_stats of slot id's sequence, or of the last one that left the slot.  push_ms_total
 * of a slot is the wall time of the calls it took part in, undivided: the slots of one call all count the whole call. */
int fv_streams_open(fv_ctx *ctx, int nslots, long long lag_rows_hint, int check_every);
int fv_streams_push(fv_ctx *ctx, const int *ids, int nids, const int *ob, const long long *offsets,
                    int *path_out, const long long *path_offsets, long long *committed_out, int *status_out);
int fv_streams_push_emissions(fv_ctx *ctx, const int *ids, int nids, const void *scores, int dtype,
                              const long long *offsets, long long ld,
                              int *path_out, const long long *path_offsets, long long *committed_out, int *status_out);
long long fv_streams_pending(const fv_ctx *ctx, int id);
int fv_streams_close(fv_ctx *ctx, int id, int *path_out, long long *n_out, float *score_out);
int fv_streams_abort(fv_ctx *ctx, int id);      /* drops slot id's sequence; the slot is empty again */
int fv_streams_end(fv_ctx *ctx);                /* frees the whole set, whatever its slots hold */
int fv_streams_slot_stats(const fv_ctx *ctx, int id, fv_stream_stats *out);
/* The open set, or the last one ended (FV_ERR_STATE: there never was one), summed over its life.  The launch counters
 * are bare launches: step_launches of task_steps tasks in all; check_launches, two per pair (in a lag-bounded set,
 * fv_set_max_lag, the pair becomes three launches: ancestors and best, decide, apply), serving check_slots slot-checks;
 * syncs: the times the host waited for the device (at most two per symbol push call, three per score push call, one more
 * per regrow, one per close). */
typedef struct { long long calls, step_launches, task_steps, check_launches, check_slots, syncs; int nslots, batch_cap, kernel; double push_ms_total; } fv_streams_stats;
int fv_streams_last_stats(const fv_ctx *ctx, fv_streams_stats *out);

/* Online decodes with a bounded commit lag.
 * A stream commits a piece only when every survivor path has merged into one ancestor at the anchor.  On models whose
 * paths never merge (near-deterministic aligners, disconnected components, ties) that never happens: nothing is delivered
 * before the close and the arg rows grow with T.  max_lag = L >= 1 bounds both, at the price of exactness.
 *   The rule.  Checks happen when they happen without it (every check_every = C steps and after the last step of a
 * push).  At a check at time t with anchor a and the set V of the ancestors of the states that have one: V empty, the
 * stream is dead; one ancestor v, the commit (a, v) of every stream; more than one and t - a >= L, a FORCED commit: s* is
 * the lowest index among the maxima of the score row of time t (fv_stream_close's end pick), v* its ancestor; every state
 * whose ancestor is not v* is PRUNED — its score of time t becomes -inf, so no later cell can take it as its source —
 * (a, v*) is committed exactly like a natural commit, the anchor moves to t and the survivors are re-anchored.
 *   What this guarantees.
 *   Connected path: the pieces and the close's piece concatenate to one path, every transition of which has a finite log.
 *   Exact for the pruned model: path, float32 score and return code are bit for bit those of
 * fv_decode_full(..., 1, FV_MODE_SINGLE_PASS) on the same input with the emission score of every pruned (t, s) cell set
 * to -inf (pruning a cell after the step equals a -inf emission at that cell; every other cell of every row keeps its bits).
 *   Bounded lag: after every accepted push fv_stream_pending <= 2 L + C - 2.  After any check either a commit just moved
 * the anchor to t or t - a <= L - 1; consecutive checks lie at most C steps apart, so a commit at t_c settles the times
 * up to an old anchor with t_c - a_old <= L - 1 + C; pending at a push end is (t - t_c) + (t_c - a_old), and before the
 * first commit at most L.  Device memory is therefore O((largest push + 2 L + C) K) whatever the model.
 *   What it costs.  The result is no longer the Viterbi path of the whole input.  It depends on where the checks fall, and
 * so on how the input is cut into pushes (with check_every = 1 it does not).  A forced commit can end in FV_ERR_NO_PRED
 * where the exact decode finds a path, because the best state of time t may be a dead end, as with any pruning; the stream
 * then behaves like any dead stream.
 *   No forced commit, nothing changes: with max_lag = 0, or a max_lag that is never reached, pieces, counts, score, return
 * codes and every fv_stream_stats counter are those of the stream without a bound.
 *
 * fv_set_max_lag: 0 (default): unbounded.  >= 1: streams and sets opened afterwards force commits by the rule above.
 * FV_ERR_ARG for a negative value, FV_ERR_STATE while a stream or a set is open (as fv_set_option).  Kept across
 * fv_set_model*; applies to every slot of a set. */
int fv_set_max_lag(fv_ctx *ctx, long long max_lag);

typedef struct {
    long long max_lag;            /* in force for this stream / slot */
    long long forced_commits;     /* commits that were forced (counted in fv_stream_stats.commits too) */
    long long pruned_states;      /* states with anc >= 0 and anc != v*, summed over the forced commits */
    long long first_forced_time;  /* time t of the first forced commit, -1: none */
    long long last_forced_time;
} fv_lag_stats;
/* slot < 0: the single stream (open, or the last closed/aborted); else slot of the set (open, or the last ended).
 * FV_ERR_STATE: there never was one; FV_ERR_ARG: a slot outside the set. */
int fv_last_lag_stats(const fv_ctx *ctx, int slot, fv_lag_stats *out);

/* Forward-backward on the device: how probable an observation sequence is under the model (fv_loglik,
 * fv_loglik_batch) and how sure the model is of a state at a time (fv_posteriors).  The reference has neither: it answers
 * the arg-max question only.  The sum-product recurrences run on the context's own float64 tables.
 *   Definitions.  All values are float64.  LPi[j] = log((double)Pi[j]), LA[i][j] = log((double)A[i][j]).  The emission
 * term e[t][j] is log((double)B[j][ob[t]]); with ob == NULL it is the staged E64[t][j] (fv_set_emissions), under exactly
 * the ob == NULL rules of the decode calls, an emission map included (the staged tables are T x K).
 *     alpha[0][j] = LPi[j] + e[0][j]           alpha[t][j] = e[t][j] + log sum_i exp(alpha[t-1][i] + LA[i][j])
 *     beta[T-1][i] = 0                         beta[t][i] = log sum_j exp(LA[i][j] + e[t+1][j] + beta[t+1][j])
 *     loglik = log sum_j exp(alpha[T-1][j])    gamma[t][j] = exp(alpha[t][j] + beta[t][j] - loglik)
 * gamma is rounded to float32 and is 0 where either term is -inf.  gamma_out[t * ld + j], ld >= K in elements, is a host
 * or a device pointer (hipPointerGetAttributes decides, as in fv_set_emissions; a device block on the context's GPU) and
 * may be NULL; what lies beyond K in a row is not touched.  path_out[t] (may be NULL) is the lowest index among the maxima
 * over j of the float64 value alpha[t][j] + beta[t][j] that the device holds: posterior decoding.  loglik_out may be NULL
 * in fv_posteriors.  T >= 1.
 *   fv_loglik_batch: the offsets contract of fv_decode_full_batch (sequences back to back, offsets[0] == 0, nseq + 1
 * non-decreasing entries, the total below 2^31; ob == NULL: sequence s on staged rows offsets[s] .. offsets[s+1]), but
 * every length >= 1 is allowed.  loglik_out[s] and status_out[s] (may be NULL) are per sequence exactly what fv_loglik on
 * that sequence delivers, the other sequences are intact, and the return value is the most negative status.  The
 * sequences advance in lock-step and share the step launches, up to batch_cap tasks per sweep of the table.
 *   Return codes.  FV_OK.  FV_ERR_NO_PRED when loglik is -inf (the model gives the sequence probability 0): then
 * *loglik_out = -inf, path_out is filled with -1 and gamma_out is not written.  Refused before any device work, with a
 * detail text: T < 1, bad pointers or offsets, a symbol outside [0, M), ob == NULL with too few staged rows, ld < K
 * (FV_ERR_ARG); no model, or an open stream or set (FV_ERR_STATE); multi-device, partitioned and communicator contexts
 * (FV_ERR_UNSUPPORTED); a model set by fv_set_model_sparse (FV_ERR_UNSUPPORTED, below); K > 20192, the largest K whose
 * float64 score row the step kernel can stage in LDS (FV_ERR_UNSUPPORTED); a working set beyond the free device memory
 * (FV_ERR_NOMEM, with the byte count, before anything is allocated).  Model entries above 1 and emission scores above 0
 * are accepted: nothing here is a filter.
 *   Memory.  The step streams A itself as float32 (4 bytes per cell, tile-major as the float32 log table, pads 0), built
 * on the device from the stored logs by the first call; fv_posteriors' backward pass streams the transposed table, built
 * by the first fv_posteriors.  Both tables belong to the model, cost 4 * K^2 bytes each and are dropped by fv_set_model
 * and fv_set_model_sparse.  fv_loglik keeps two float64 rows per sequence, fv_posteriors 16 * T * K bytes of alpha and
 * beta (plus 4 * T * K for a host gamma_out).
 *   Guarantees.
 *   1. Accuracy.  Let u = 2^-53 and Amax the largest finite |alpha| or |beta| of the call.  Every finite alpha[t][j] lies
 * within 2 * (t + 1) * (K + 1024) * u * max(1, Amax) of the exact value, beta[t][i] within the same bound with T - t in
 * place of t + 1, loglik within the bound at t = T - 1.  The bound is derived, not measured: a sum of K non-negative terms
 * has relative error at most K * u in any order, an exp argument of magnitude up to 745 carries a relative error of at
 * most 745 * u, and an error carried in from the row before passes through a convex combination without growing, so the
 * errors add once per step.  -inf comes out where, and only where, the exact value is -inf.
 *   2. No flush.  The step works in linear space on p[i] = exp(alpha[i] - max alpha); a column all of whose probability
 * comes from states more than 745 below the row's maximum still comes out finite and within the bound: a column whose
 * linear sum falls below 2^-800 is re-evaluated per column as max_i + log sum_i exp(alpha[i] + LA[i][j] - max_i).  The
 * threshold holds for every float32 model entry: what exp flushed, times an entry below 2^128, over K <= 20192 rows, is
 * less than 2^-879, below u times any sum that is not re-evaluated.
 *   3. Reproducible bits.  The same call twice gives the same bits; fv_loglik_batch gives, per sequence, the bits of
 * fv_loglik, whatever the grouping and whatever FV_OPT_MAX_BATCH; fv_posteriors' *loglik_out has the bits of fv_loglik.
 * A task's summation order does not depend on the launch form, and no reduction uses floating-point atomics.
 *   Out of scope.  Models set by fv_set_model_sparse are refused unless fv_set_sparse_sumprod (below) has switched their
 * route on; the refusal's text is the one this library always gave.  Multi-device contexts, streaming likelihoods and
 * Baum-Welch accumulators (xi) are not offered either. */
int fv_loglik(fv_ctx *ctx, const int *ob, int T, double *loglik_out);
int fv_loglik_batch(fv_ctx *ctx, const int *ob, const long long *offsets, int nseq,
                    double *loglik_out, int *status_out);
int fv_posteriors(fv_ctx *ctx, const int *ob, int T, float *gamma_out, long long ld,
                  int *path_out, double *loglik_out);
/* The last fv_loglik, fv_loglik_batch or fv_posteriors that ran (FV_ERR_STATE: there never was one). */
typedef struct {
    double call_ms;                 /* host wall time of the call (enqueue .. final sync) */
    double gpu_ms;                  /* HIP-event time from its first to its last kernel */
    long long step_launches;        /* launches of the sum-product step kernel */
    long long task_steps;           /* sum over launches of the tasks advanced by one K * K step */
    long long table_bytes_per_step; /* bytes of the linear table one step launch streams (4 per cell) */
    long long device_bytes;         /* device working set of the context after the call */
    long long refine_columns;       /* columns re-evaluated in the exact per-column form (linear sum below 2^-800) */
    long long refine_finite;        /* ... those that came out finite */
    int passes;                     /* 1: forward only (loglik), 2: forward and backward (posteriors) */
    int batch_cap;                  /* most tasks one step launch takes: the smallest of FV_OPT_MAX_BATCH, 4 and the float64 rows 160 KiB of LDS hold */
} fv_sumprod_stats;
int fv_last_sumprod_stats(const fv_ctx *ctx, fv_sumprod_stats *out);
/* fv_loglik, fv_loglik_batch and fv_posteriors on a model set by fv_set_model_sparse.  on = 0 (the
 * default): such a model is refused, as above, and every call behaves as it did before this function existed.  on = 1: the
 * three calls run on the stored transitions, with the definitions, return codes, ob == NULL rules (emission maps
 * included), gamma_out / ld rules and FV_ERR_NO_PRED behaviour above; model entries above 1 and staged scores above 0 are
 * accepted.  Any other value: FV_ERR_ARG.  While a stream or a set of streams is open: FV_ERR_STATE, as fv_set_option.  The
 * setting is kept across fv_set_model and fv_set_model_sparse; on a model set by fv_set_model it changes nothing.
 * Multi-device, partitioned and communicator contexts stay refused.
 *   K.  The K <= 20192 limit does not apply to this route: K is bounded by memory.  The forward step walks the CSC-32 table the
 * decodes walk, the backward step the caller's rows; both stream 8 bytes per entry: the source state or column and the
 * stored value itself as float32 (CSlin, CRlin: built on the device from the stored float64 logs by the first call that
 * needs each, 4 bytes per padded entry and 4 bytes per stored entry; they belong to the model and are dropped by
 * fv_set_model and fv_set_model_sparse).  While NB float64 score rows fit LDS a step stages them there; beyond (every K
 * above 20192), or under FV_OPT_DEBUG bit 31, a small scale launch leaves p[i] = exp(row[i] - max) in workspace rows
 * (8 * 4 * K bytes) and the step gathers from memory.  fv_sumprod_stats.table_bytes_per_step is 8 bytes per padded entry
 * of the CSC-32 table, batch_cap in the memory form the smaller of FV_OPT_MAX_BATCH and 4; step_launches and task_steps
 * count step kernels, not scale launches.
 *   Guarantees 1 to 3 hold unchanged.  The 2^-800 threshold holds for any K < 2^31: what exp flushed, times an entry below
 * 2^128, over fewer than 2^31 terms, is less than 2^-863, below u * 2^-800.  Order rule: a task's summation order is a
 * function of the stored table alone; it does not depend on the number of tasks in a launch, on FV_OPT_MAX_BATCH, on how a
 * batch is grouped, or on whether the score rows were staged in LDS or read from memory, and stored entries equal to 0 change
 * no bit of any result: they are the same as absent entries. */
int fv_set_sparse_sumprod(fv_ctx *ctx, int on);

/* Baum-Welch E-step accumulators on the device: the expected counts a re-estimation of the model needs,
 * summed over the sequences of one call.  This is what is now offered of the accumulators the block above leaves out; the
 * M-step (normalising the rows) is the caller's.
 *   Definitions, on top of alpha, beta, e and loglik above, all float64.  For one sequence of length T,
 *     xi_t[i][j] = exp(alpha[t][i] + LA[i][j] + e[t+1][j] + beta[t+1][j] - loglik)   for t = 0 .. T-2,
 *     g_t[j]     = exp(alpha[t][j] + beta[t][j] - loglik)                            for t = 0 .. T-1.
 * The sums run over the live sequences s of the call, in sequence order:
 *     trans_out[i * ld + j] = sum_s sum_t xi_t[i][j]          ld >= K in elements; a host or a device pointer on the
 *                                                             context's GPU, as gamma_out; beyond K a row is not touched
 *     emit_out[j * M + m]   = sum_s sum_{t : ob[t] = m} g_t[j]   K x M, host
 *     init_out[j]           = sum_s g_0[j]                       host
 *     occ_out[j]            = sum_s sum_t g_t[j]                 host
 *     loglik_out[s], status_out[s]: as fv_loglik_batch           host
 * Any output pointer may be NULL.  Outputs are overwritten, not added to.  The offsets contract is fv_loglik_batch's; every
 * length >= 1 is allowed, and a sequence of length 1 contributes to init, occ and emit only.  ob == NULL works as in
 * fv_posteriors (sequence s on staged rows offsets[s] .. offsets[s+1], an emission map included); emit_out must then be
 * NULL, because there is no symbol alphabet (FV_ERR_ARG).  A sequence of probability 0 (loglik = -inf) has status
 * FV_ERR_NO_PRED and contributes nothing, the others are intact, and the return value is the most negative status.
 *   Refused before any device work, with a detail text: the argument errors of fv_loglik_batch, ld < K, a trans_out on
 * another device, a non-NULL emit_out with ob == NULL (FV_ERR_ARG); no model, or an open stream or set (FV_ERR_STATE);
 * multi-device, partitioned and communicator contexts, and K > 20192 (FV_ERR_UNSUPPORTED); a model set by
 * fv_set_model_sparse, whether or not fv_set_sparse_sumprod is on (FV_ERR_UNSUPPORTED: the CSR route of the counts is a
 * follow-up); a working set beyond the free device memory (FV_ERR_NOMEM, with the byte count, before anything is
 * allocated).  Model entries above 1 and emission scores above 0 are accepted.  fv_last_sumprod_stats and fv_last_stats
 * keep reporting their own last calls.
 *   How.  Sequence by sequence the two passes of fv_posteriors run unchanged (the same kernels, the same bits).  A scale
 * launch then leaves, per time, P[t][i] = exp(alpha[t][i] - a_t) and Q[t][j] = exp(e[t+1][j] + beta[t+1][j] - b_t + w_t),
 * a_t and b_t the two row maxima and w_t = a_t + b_t - loglik; the xi kernel sums the outer products P[t] Q[t]^T over the
 * times in registers, one float64 fma per cell and time, and multiplies once by (double)A[i][j]; one kernel sums gamma.
 * Memory: 32 * T * K bytes for the longest sequence (alpha, beta, P, Q), 8 * K^2 for a host trans_out, 16 * K * M for
 * emit_out, beside the two tables of fv_posteriors.
 *   Guarantees.
 *   G1. Accuracy.  Let R = 3 * tol(T - 1), tol(t) = 2 * (t + 1) * (K + 1024) * u * max(1, Amax) the bound of guarantee 1
 * above and T the longest sequence of the call: alpha's share, beta's share and loglik's (exp arguments and the sum over
 * the times sit inside the third).  Every count lies within R * exact + n * 2^-160 of the exact value, n the number of times
 * summed.  A transition count is exactly 0 where A[i][j] == 0.
 *   G2. No flush.  A time with w_t above 500 is a wide time: the cells that carry its mass can have P or Q flushed by exp,
 * so it is left out of the outer product and added per cell in the exact form of the definition (K^2 exp calls for that
 * time); fv_counts_stats.wide_times counts them.  Below the threshold no term of the linear form that is dropped or
 * denormalised exceeds 2^-160, for every float32 model entry: a flushed factor is below e^-708, the other at most e^500, the
 * entry below 2^128, and e^(-708 + 500) * 2^128 < 2^-171.  Ordinary models have wide_times == 0.
 *   G3. Reproducible bits.  The same call twice gives the same bits.  A batch gives, for every output, bit for bit the
 * left-to-right float64 sum of the single-sequence calls' outputs (the first term stands alone), whatever FV_OPT_MAX_BATCH
 * is; loglik_out[s] has the bits of fv_loglik.  Every cell has exactly one owner and a fixed order: times ascending within
 * a sequence (the ordinary times, then the wide ones), one add of the finished per-sequence value into the accumulator,
 * sequences in order.  No floating-point atomics anywhere.
 *   Identities, within G1: sum_j trans[i][j] = occ[i] - sum_s g_{T_s - 1}[i]; sum_ij trans = sum_s (T_s - 1); sum_j init =
 * the number of live sequences; sum_m emit[j][m] = occ[j].
 *   Out of scope: CSR-set models, lock-step passes across the sequences of a batch, accumulating across calls, per-time
 * xi output, multi-device contexts. */
int fv_expected_counts(fv_ctx *ctx, const int *ob, const long long *offsets, int nseq,
                       double *trans_out, long long ld, double *emit_out, double *init_out, double *occ_out,
                       double *loglik_out, int *status_out);
/* The last fv_expected_counts that ran (FV_ERR_STATE: there never was one). */
typedef struct {
    double call_ms;                 /* host wall time of the call (enqueue .. final sync) */
    double gpu_ms;                  /* HIP-event time from its first to its last kernel */
    long long sequences;            /* sequences of the call */
    long long dead_sequences;       /* ... those of probability 0 */
    long long times;                /* sum of T over the live sequences */
    long long step_launches;        /* launches of the sum-product step kernel, forward and backward together */
    long long task_steps;           /* sum over those launches of the tasks advanced by one K * K step */
    long long xi_launches;          /* launches of the xi kernel: one per sequence of length >= 2 when trans_out is given */
    long long wide_times;           /* times added in the exact per-cell form (w_t above 500) */
    long long device_bytes;         /* device working set of the context after the call */
} fv_counts_stats;
int fv_last_counts_stats(const fv_ctx *ctx, fv_counts_stats *out);

int fv_last_stats(const fv_ctx *ctx, fv_stats *out);
const char *fv_strerror(int rc);
const char *fv_last_error_detail(const fv_ctx *ctx);

/* vit->memory_bytes as the reference computes it (FLASH:355,364-367; FLASH_BS:564,573-576)
 * — a sizeof formula, not a measurement; beam_width = 0 selects the full variant. */
long long fv_reference_memory_bytes(int K, int T, int n_split, int beam_width);

/* Multi-GPU: one process per GPU.  Rank 0 calls fv_comm_unique_id and hands the 128 bytes
 * to every rank by any means (bench.py uses torch.distributed); every rank then calls
 * fv_comm_init.  After that each decode call is collective: the whole-sequence pass runs
 * on every rank, the n_split top-level segments (FLASH:349-353) are dealt round-robin to
 * ranks, and one RCCL all-gather over xGMI merges the per-rank path slices.  Replaces the
 * shared-memory work queue of worker() (FLASH:264-308). */
#define FV_UNIQUE_ID_BYTES 128
int fv_comm_unique_id(void *id_out);
int fv_comm_init(fv_ctx *ctx, int rank, int nranks, const void *id);

/* Sharding without a communicator: the decode calls run the whole-sequence pass plus only the
 * segments rank `rank` of `nranks` owns and return that rank's answer array (positions owned by other
 * ranks hold the whole-pass chain); the caller gathers the nranks arrays by its own means and applies
 * fv_merge_paths.  For hosts that already have a collective layer (bench.py falls back to this with
 * torch.distributed if fv_comm_init fails). */
int fv_set_partition(fv_ctx *ctx, int rank, int nranks);

/* The merge applied after the all-gather, exposed for CPU tests: gathered = nranks arrays of T
 * answers (rank-major); position j is taken from the rank owning the top-level segment that
 * contains it, segment end points from rank 0. */
int fv_merge_paths(int T, int n_split, int nranks, const int *gathered, int *path_out);

/* Host-side schedule, exposed so it can be tested without a GPU.  Fills at most `cap`
 * entries of (L, R, generation, owner_rank) per forward pass, in launch order, and returns
 * the number of passes (or <0).  Pass 0 is always the whole-sequence pass. */
typedef struct { int L, R, generation, owner; } fv_pass_info;
int fv_plan_passes(int T, int n_split, int mode, int nranks, fv_pass_info *out, int cap);

/* The flat schedule of FV_OPT_FLAT_GENERATIONS for one rank (mode FV_MODE_REFERENCE): every pass of generation >= 1, in the
 * order of fv_plan_passes, dealt in batches of at most batch_cap passes of one length to nstreams streams.  arg_row: the
 * first of the pass's R - L private arg rows (-1: a generation-1 pass, which writes the rows of its own times); chain: the
 * first of its R - L chain entries; batch: -1 for a one-step pass (a single-column job only).  Returns the number of
 * passes (or <0). */
typedef struct { int L, R, generation, batch, stream, chain; long long arg_row; } fv_flat_info;
int fv_plan_flat(int T, int n_split, int batch_cap, int nstreams, fv_flat_info *out, int cap);

/* The schedule of fv_decode_full_batch: the passes of all sequences in launch order (sorted by generation), L and R
 * as positions in the concatenated time axis (sequence s starts at lengths[0] + .. + lengths[s-1]), `owner` = index
 * of the sequence the pass belongs to.  Returns the number of passes (or <0). */
int fv_plan_passes_batch(const int *lengths, int nseq, int n_split, int mode, fv_pass_info *out, int cap);

#ifdef __cplusplus
}
#endif
#endif
