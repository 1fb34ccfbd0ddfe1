// fv_schedule.h — host-side task tree of the FLASH divide-and-conquer (no HIP here).
#pragma once
#include <vector>

namespace fv {

struct Pass {
    int L, R;          // time range; steps j = L+1 .. R
    bool from_pi;      // init row from Pi (L == 0) instead of A[Ans[L-1]][*]
    bool whole;        // the whole-sequence pass: end state = argmax of the last row
    int generation;    // passes of one generation are mutually independent
    int owner;         // rank that runs it (-1: every rank)
    int seq = 0;       // batch decode: index of the sequence the pass belongs to (L and R are positions in the
                       // concatenated time axis of the batch)
};

struct Plan {
    std::vector<Pass> passes;             // sorted by generation
    std::vector<int> gen_begin;           // passes[gen_begin[g] .. gen_begin[g+1]) is generation g
    std::vector<int> midpoints;           // top-level split points (empty when no N-way split)
    std::vector<int> seg_L, seg_R, seg_owner;   // top-level segments and their ranks
    int generations() const { return (int)gen_begin.size() - 1; }
};

// Even split of [L,R] into N parts — reference FLASH_Viterbi_multithread.c:129-136.
void split_points(int L, int R, int N, std::vector<int> &mid);

// mode 0: the reference's task tree (calc :338-368 + worker :284-302), with every task
// whose forward pass repeats a prefix of an already-run pass folded into that pass.
// mode 1: one pass over [0,T-1].
// Returns 0 or a negative FV_ERR_* code.
int build_plan(int T, int n_split, int mode, int nranks, Plan &plan);

// A batch of sequences laid end to end on one time axis: build_plan of every sequence (one rank), shifted to the
// sequence's offset; generation g of the forest is the union of generation g of every sequence, in sequence order.
// midpoints / seg_* stay empty (they serve the multi-rank merge).  On failure *bad_seq (may be null) is the index of
// the sequence build_plan refused.
int build_forest(const int *lengths, int nseq, int n_split, int mode, Plan &plan, int *bad_seq);

// The right-hand passes of ALL generations of a one-rank plan as one independent set (fv_full.hip, run_flat_full): every
// pass takes its two conditioning states from the whole-sequence chain instead of from the generation before it, so
// nothing orders the passes but the streams they are dealt to.
struct FlatPass {
    int L, R, generation;
    long long arg_row;   // first of its R - L private arg rows (passes of different generations overlap in time); -1: a
                         // generation-1 pass, which keeps the rows of its own times in the by-time array
    int chain;           // first of its R - L chain entries c[L..R-1]
    int batch;           // index into FlatPlan::batches; -1: a one-step pass (its only step is the single-column one)
    int stream;          // stream that carries every launch of the pass
};
struct FlatBatch {
    std::vector<int> pass;   // indices into FlatPlan::passes, longest first, at most `cap` of them
    int len, stream;         // len: steps of the longest
};
struct FlatPlan {
    std::vector<FlatPass> passes;     // in the order of Plan::passes (sorted by generation), the whole-sequence pass left out
    std::vector<int> gen_begin;       // passes[gen_begin[g - 1] .. gen_begin[g]) is generation g >= 1
    std::vector<FlatBatch> batches;   // longest first
    std::vector<std::vector<int>> stream_batches;   // per stream: its batches in launch order
    long long arg_rows = 0;           // private arg rows in all
    int chain_len = 0;                // chain entries in all
    int nstreams = 1;
};
// cap: most passes per batch; nstreams: streams the batches are dealt to, longest batch first to the stream with the
// least step launches so far (equal sums of length, none idles); one-step passes go to the stream with the least.
void build_flat(const Plan &plan, int cap, int nstreams, FlatPlan &flat);

}  // namespace fv
