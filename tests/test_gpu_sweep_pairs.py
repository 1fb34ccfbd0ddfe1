"""GPU: the packed kernel's sweep keeps block minima, and the second cell of a lane inside the refine window is found where
it really is — in the other parity half, in another row block, or (new) in the same half of the block that is decoded for
the candidate anyway (fv_kernels.hip.inc, "Second smallest"; tests/test_sweep_summary.py restates the argument on the CPU).

Models made for it: every column i has exactly two finite predecessors, r(i) and r(i) + d, with equal probability, B and Pi
are uniform — so all reachable scores tie, the two cells of a column have the same 16-bit sum z, and the reference takes the
lower row.  The kernel must see two cells in the window and re-walk the lane; if it saw one it would answer r(i) + d half the
time.  d places the rival: 1 the same (even, odd) pair, 2 and 6 the same half of the same 8-row block, 256 the lane's next
row block in the 8-wave forms (another wave in the 16-wave forms), 512 the block after that (the next trip of the double-
buffered sweep; the next block at 16 waves).  One column, K - 1, has two far less likely predecessors: it sets the code range,
or every finite code would be 65534 and every column would be decided by the saturation guard; state K - 1 is nobody's
predecessor, so its lower score touches nothing (its own column is the one the guard does decide).  The near-tie variants
give r(i) + d a probability 1.5 code steps lower: not tied, one or two code units behind, inside the window.  In both the
lower row is the answer, which is also the row `locate` names when it takes a tie for a single candidate; the "flip" variants
are the ones a missed second cell gets wrong: r(i) + d is 0.2 code steps MORE likely — the same code, the same z, but the
reference now takes the higher row, and only a re-walk finds it.

Bar: every score row bit-equal and every back-pointer equal to the oracle's full_forward, for the packed forms x the row-codes
option x pass sets of 1, 2 and 4 passes (tests/test_gpu_row_codes.py: forward_everywhere); decodes equal to the oracle's, with
lane re-walks counted (refine_rescan > 0: a decode's right-hand passes start from one state, their unreachable columns are
re-walked by the guard and counted too — the equality of the tables is what tells).  refine_near counts single candidates that are not their column's smallest z: two
cells of ONE lane inside the window make a re-walk, never such a candidate, so the near-tie models assert refine_rescan > 0
as well, and refine_near > 0 where the rival does sit in another lane (d = 256 in the 16-wave form)."""
import numpy as np
import pytest

import oracle
from conftest import load_goldens, golden_model
from flash_viterbi_amd import decoder, hostio
from test_gpu_row_codes import DBUF, PACKED, W16, forward_everywhere, sets_for

pytestmark = pytest.mark.gpu

D = decoder
FORMS = (0, W16, DBUF, PACKED, PACKED | W16, PACKED | DBUF)
P, P_RANGE = 0.5, 2.0 ** -8          # the tied probability; the one that sets the code range
M = 4
TV_U16_NB1 = (1 << 26) | (1 << 30) | (1 << 34) | (1 << 38)       # FV_TV_U16_*_NB1: the single-task forms of the packed kernel


def code_step():
    """the documented table code: step = (float32) largest finite |log A| / 65534, code = rne(-log A / step)"""
    return float(np.float32(-np.log(np.float64(np.float32(P_RANGE))) / 65534.0))


def codes(a):
    return np.rint(-np.log(np.asarray(a, dtype=np.float64)) / code_step()).astype(np.int64)


def pair_model(K, d, variant, seed):
    rs = np.random.RandomState(seed)
    p2 = np.float32(P * np.exp({"tied": 0.0, "near": -1.5, "flip": 0.2}[variant] * code_step()))
    A = np.zeros((K, K), dtype=np.float32)
    if d < 8:
        # r and r + d inside one 8-row group; d = 1: r even, the two rows are one (even, odd) pair
        slots = [g * 8 + o for g in range((K - 1) // 8) for o in range(0, 8 - d, 2 if d == 1 else 1) if g * 8 + o + d < K - 1]
    else:
        slots = list(range(K - 1 - d))
    r = rs.choice(slots, K)
    for i in range(K):
        A[r[i], i], A[r[i] + d, i] = (P_RANGE, P_RANGE) if i == K - 1 else (P, p2)
    Bm = np.full((K, M), 1.0 / M)
    Pi = np.full(K, 1.0 / K)
    return hostio.quantize_text16(A), hostio.quantize_text16(Bm), hostio.quantize_text16(Pi), r


def lane(k, nwv):
    """(wave, row group) that sweeps source row k, the lane's block number, the row inside the block's 8 rows"""
    blk = k // 32
    return (blk % nwv, (k % 32) // 8), blk // nwv, k % 8


def construction_holds(A, Bm, Pi, r, d, variant, ob):
    """what the module text claims of the model, shown on the CPU"""
    K = A.shape[0]
    assert ((A > 0).sum(axis=0) == 2).all() and not (A[K - 1] > 0).any()
    ca = codes(np.where(A > 0, A, 1.0))
    for i in range(K):
        a, b = int(r[i]), int(r[i]) + d
        assert A[a, i] > 0 and A[b, i] > 0
        gap = int(ca[b, i] - ca[a, i])
        assert (1 <= gap <= 2) if variant == "near" and i < K - 1 else gap == 0   # within 3 code units: tied, or 1-2 behind
        (la, ja, ka), (lb, jb, kb) = lane(a, 8), lane(b, 8)
        assert la == lb                                                        # one lane of the 8-wave forms
        if d == 1:
            assert ja == jb and ka // 2 == kb // 2 and kb == ka + 1            # the same pair
        elif d < 8:
            assert ja == jb and kb == ka + d and ka % 2 == kb % 2              # the same half of the same block
        else:
            assert ka == kb and jb - ja == d // 256                            # the next block (256), the one after (512)
            (wa, _, _), (wb, _, _) = lane(a, 16), lane(b, 16)
            assert (wa != wb) if d == 256 else (wa == wb)                       # 16 waves: 256 another lane, 512 the next block
    assert 1000 < ca[ca > 0].min() and ca.max() == 65534                       # far from the end of the code range
    # the scores that enter a step tie (all but state K - 1): with equal table codes the two cells of a column have equal z
    om = oracle.OracleModel(A, Bm, Pi)
    try:
        row, args = om.full_forward(ob, 0, 3, -1)
    finally:
        om.close()
    assert np.unique(row[:K - 1]).size == 1 and row[K - 1] < row[0]
    # the reference takes the lower row everywhere; flip: the higher one (but in column K - 1, a tie in every variant)
    assert (args[-1] == (np.where(np.arange(K) < K - 1, r + d, r) if variant == "flip" else r)).all()


def decode_counts(A, Bm, Pi, ob, debug, n_split):
    om = oracle.OracleModel(A, Bm, Pi)
    fv = decoder.FlashViterbi(0)
    try:
        fv.set_model(A, Bm, Pi)
        fv.set_option(D.OPT_KERNEL, D.KERNEL_U16_REFINE)
        fv.set_option(D.OPT_DEBUG, debug)
        want_path, want_score, _, want_rc = om.full_decode(ob, n_split, check=False)
        path, score, rc = fv.decode_full(ob, n_split, D.MODE_REFERENCE)
        st = fv.stats()
        assert rc == want_rc == 0 and path.tolist() == want_path.tolist() and score == want_score, (debug, n_split)
        print(f"K={A.shape[0]} debug={debug} n_split={n_split}: refine_near {st['refine_near']} refine_rescan {st['refine_rescan']} "
              f"refine_saturated {st['refine_saturated']}")
        return st
    finally:
        fv.close()
        om.close()


CASES = [(77, 1, "tied"), (77, 2, "tied"), (77, 6, "tied"), (77, 2, "near"), (77, 1, "flip"), (77, 6, "flip"),
         (1100, 2, "tied"), (1100, 256, "tied"), (1100, 512, "tied"), (1100, 256, "near"), (1100, 2, "flip"), (1100, 512, "flip")]


@pytest.mark.parametrize("K,d,variant", CASES, ids=[f"K{K}-d{d}-{v}" for K, d, v in CASES])
def test_rival_in_the_same_lane(K, d, variant):
    sets, need = sets_for(K, 300 + d, (1, 2, 4))
    A, Bm, Pi, r = pair_model(K, d, variant, 7000 + K + d)
    ob = np.random.RandomState(K + d).randint(0, M, need + 1).astype(np.int32)
    construction_holds(A, Bm, Pi, r, d, variant, ob)
    forward_everywhere(A, Bm, Pi, ob, sets, forms=FORMS)
    # decodes: the single-task forms in the whole-sequence pass (n_split 1), the batched ones on the right-hand passes
    for debug, n_split in ((0, 1), (DBUF, 1), (PACKED, 4)):
        st = decode_counts(A, Bm, Pi, ob, debug, n_split)
        assert st["refine_rescan"] > 0, (debug, n_split, st)
    if variant == "near" and d == 256:
        st = decode_counts(A, Bm, Pi, ob, W16, 1)
        assert st["refine_near"] > 0, st


def test_golden_decode_runs_the_code_free_single_task_form():
    """A small golden through fv_decode_full with the packed kernel: path, score and rc equal to the oracle's (and to the
    stored reference run).  FV_OPT_ROW_CODES is at its default, which leaves K = 512 without the route: the single-task
    launches neither read nor write codes, and fv_test_forward of one pass on the same context shows the form that ran — a
    single-task bit of the packed kernel without FV_TV_ROW_CODES: trellis_step_u16<1, *, *, *, false>."""
    g = next(x for x in load_goldens() if x["name"] == "ds_K512_T64")
    A, Bm, Pi, ob = golden_model(g)
    om = oracle.OracleModel(A, Bm, Pi)
    fv = decoder.FlashViterbi(0)
    try:
        fv.set_model(A, Bm, Pi)
        fv.set_option(D.OPT_KERNEL, D.KERNEL_U16_REFINE)
        for n in (1, 8):
            want_path, want_score, _, want_rc = om.full_decode(ob, n, check=False)
            path, score, rc = fv.decode_full(ob, n, D.MODE_REFERENCE)
            assert rc == want_rc == 0 and path.tolist() == want_path.tolist() and score == want_score, n
            ref = next((x for x in g["runs"] if x["algo"] == "flash" and x["N"] == n), None)
            if ref is not None:
                assert path.tolist() == ref["path"] and np.float32(score) == np.float32(ref["score"])
        for debug in (0, DBUF, W16, W16 | DBUF):
            fv.set_option(D.OPT_DEBUG, debug)
            rows, bp, var = fv.test_forward(ob, [(0, 6, -1)], -2)
            want_row, want_bp = om.full_forward(ob, 0, 6, -1)
            assert np.array_equal(rows[0].view(np.uint32), want_row.view(np.uint32)) and np.array_equal(bp[1:7], want_bp)
            assert var & TV_U16_NB1 and not var & D.TV_ROW_CODES, f"debug={debug} variants {var:#x}"
    finally:
        fv.close()
        om.close()
