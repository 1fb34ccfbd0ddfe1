"""GPU: FV_OPT_ROW_CODES — the packed 16-bit kernel takes the 16-bit codes of its incoming score rows from the launch that
wrote them (codes relative to the maximum of their 16-column tile, plus those maxima) instead of quantising the float row
again in every workgroup.

Bar: equality.  Every score row and every back-pointer of fv_test_forward equal between the option at 0 and at 2 and equal
to the oracle's single-pass primitive, for every launch form of the packed kernel; every decode equal in path, score and
return code between 0 and 2.  FV_TV_ROW_CODES in the hook's variant mask tells that the new prologue really ran.
tests/test_row_codes_bound.py checks the arithmetic of the codes on the CPU."""
import ctypes

import numpy as np
import pytest

import modelgen
import oracle
from conftest import golden_model, load_goldens
from flash_viterbi_amd import decoder, hostio
from test_gpu_adversarial import WIDE
from test_gpu_step_tables import build_model, pass_set

pytestmark = pytest.mark.gpu

D = decoder
CODES = D.OPT_ROW_CODES
BP_FILL = -2
TV_Q16_ANY = 0x3F << 16                  # trellis_step<q16_t, *>: the f32 filter on the 16-bit table
TV_U16_ANY = 0xFFFF << 26                # trellis_step_u16<*>
# FV_OPT_DEBUG: 14 packed kernel for every batched launch, 13 its 16-wave form, 2 the double-buffered form, 18 one stream
PACKED, W16, DBUF, ONE_STREAM = 1 << 14, 1 << 13, 1 << 2, 1 << 18
FORMS = (0, W16, DBUF, PACKED, PACKED | W16, PACKED | DBUF, PACKED | W16 | DBUF, PACKED | ONE_STREAM)
# passes of unequal lengths: batches re-form as passes finish, and the longest is alone for its last four steps — with the
# f32 filter in the batched launches it changes to the packed kernel there, first on a row without codes, then on its own
BATCH_SETS = {1: (6,), 2: (7, 3), 3: (8, 4, 2), 4: (9, 5, 3, 1), 5: (10, 6, 5, 3, 2), 8: (13, 9, 8, 6, 5, 4, 2, 1)}


def forward_everywhere(A, Bm, Pi, ob, pass_sets, forms=FORMS):
    """fv_test_forward over pass sets x forms with the option at 0 and at 2: both equal to the oracle in every column"""
    om = oracle.OracleModel(A, Bm, Pi)
    fv = decoder.FlashViterbi(0)
    try:
        fv.set_model(A, Bm, Pi)
        fv.set_option(D.OPT_KERNEL, D.KERNEL_U16_REFINE)
        for passes in pass_sets:
            want = [om.full_forward(ob, L, R, s) for L, R, s in passes]
            for debug in forms:
                fv.set_option(D.OPT_DEBUG, debug)
                got = {}
                for opt in (0, 2):
                    fv.set_option(CODES, opt)
                    rows, bp, var = fv.test_forward(ob, passes, BP_FILL)
                    where = f"K={A.shape[0]} passes={len(passes)} debug={debug} option={opt}"
                    for q, (L, R, s) in enumerate(passes):
                        row, args = want[q]
                        assert np.array_equal(rows[q].view(np.uint32), row.view(np.uint32)), where + f": final row of pass {L}..{R}"
                        assert np.array_equal(bp[L + 1:R + 1], args), where + f": back-pointers of pass {L}..{R}"
                    assert bool(var & D.TV_ROW_CODES) == (opt == 2), where + f": variants {var:#x}"
                    assert var & TV_U16_ANY, where
                    if len(passes) > 1 and not debug & PACKED and len(passes) <= 4:
                        # the mixed case: f32-filter launches and packed launches in one call (more than four passes: forked,
                        # all packed)
                        assert var & TV_Q16_ANY, where + f": variants {var:#x}"
                    got[opt] = (rows, bp)
                assert np.array_equal(got[0][0].view(np.uint32), got[2][0].view(np.uint32)) and np.array_equal(got[0][1], got[2][1])
    finally:
        fv.close()
        om.close()


def sets_for(K, seed, sizes):
    out, T = [], 0
    for n in sizes:
        passes, need = pass_set(BATCH_SETS[n], K, seed + n)
        out.append(passes)
        T = max(T, need)
    return out, T


@pytest.mark.parametrize("K,T", [(5, 0), (9, 0), (77, 0), (200, 100), (512, 64)])
def test_step_tables_equal_with_and_without_row_codes(K, T):
    """K = 5, 9: one tile, waves without row blocks; 77: the last tile is half pads; batches of 1, 2, 3, 4, 5 and 8 passes."""
    sets, need = sets_for(K, 40 + K, (1, 2, 3, 4, 5, 8))
    A, Bm, Pi, ob = build_model("data_script", K, max(T, need + 1), 900 + K)
    forward_everywhere(A, Bm, Pi, ob, sets)


def test_step_tables_more_than_256_tiles():
    """K = 4112: 257 tiles (the tile-maximum loop past 256) and 516 chunks of codes (the staging loop past one per thread)."""
    K = 4112
    sets, need = sets_for(K, 77, (1, 4))
    A, Bm, Pi, ob = modelgen.model32(dict(kind="sparse_fast", K=K, M=8, T=need + 1, prob=0.02, seed=4112))
    forward_everywhere(A, Bm, Pi, ob, sets, forms=(0, PACKED, PACKED | W16, PACKED | DBUF))


def band_model(K, reach, M, T, seed, dead_end):
    """State i moves to i+1 .. i+reach only; Pi sits on the first eight states: everything from state 8 + reach * t on is
    unreachable at time t (whole 16-column tiles without a finite score).  dead_end: the band does not wrap and the last
    state has no successor, so from step K on no state is reachable at all."""
    rs = np.random.RandomState(seed)
    A = np.zeros((K, K))
    for i in range(K):
        for d in range(1, reach + 1):
            j = i + d
            if j < K or not dead_end:
                A[i, j % K] = rs.uniform(0.1, 1.0)
    s = A.sum(axis=1, keepdims=True)
    A = np.divide(A, s, out=np.zeros_like(A), where=s > 0)
    Bm = rs.uniform(0.1, 1.0, (K, M))
    Bm /= Bm.sum(axis=1, keepdims=True)
    Pi = np.zeros(K)
    Pi[:8] = 0.125
    ob = rs.randint(0, M, T).astype(np.int32)
    return hostio.quantize_text16(A), hostio.quantize_text16(Bm), hostio.quantize_text16(Pi), ob


def raw_full(fv, ob, N):
    """fv_decode_full without the wrapper's exception: FV_ERR_NO_PRED keeps its path and score"""
    o = np.ascontiguousarray(ob, dtype=np.int32)
    path = np.empty(o.size, dtype=np.int32)
    score = ctypes.c_float(0)
    rc = fv._L.fv_decode_full(fv._h, decoder._p(o), o.size, N, D.MODE_REFERENCE, decoder._p(path), ctypes.byref(score))
    return path.tolist(), np.float32(score.value).view(np.uint32), rc


def decodes_equal(A, Bm, Pi, ob, splits, expect_rc=None):
    om = oracle.OracleModel(A, Bm, Pi)
    fv = decoder.FlashViterbi(0)
    try:
        fv.set_model(A, Bm, Pi)
        fv.set_option(D.OPT_KERNEL, D.KERNEL_U16_REFINE)
        for N in splits:
            opath, oscore, _, orc = om.full_decode(ob, N, check=False)
            for debug in (0, PACKED, PACKED | ONE_STREAM):
                fv.set_option(D.OPT_DEBUG, debug)
                got = {}
                for opt in (0, 2):
                    fv.set_option(CODES, opt)
                    got[opt] = raw_full(fv, ob, N)
                assert got[0] == got[2], (N, debug)
                path, score, rc = got[2]
                if expect_rc is not None:
                    assert rc == expect_rc and orc == expect_rc, (N, debug, rc, orc)
                if orc == 0:
                    assert rc == 0 and path == opath.tolist() and score == np.float32(oscore).view(np.uint32), (N, debug)
                else:
                    assert rc == orc == D.ERR_NO_PRED and min(path) < 0, (N, debug, rc, orc)
    finally:
        fv.close()
        om.close()


def test_unreachable_tiles():
    """48 steps from eight live states, three states further per step: at least 32 consecutive states — whole tiles — have no
    finite score for the first steps, in the row init_rows writes and in the rows the kernel writes."""
    K = 160
    A, Bm, Pi, ob = band_model(K, 3, 5, 50, 31, dead_end=False)
    sets, _ = sets_for(K, 5, (1, 3))
    sets = [[(L, R, s if s < 0 else 2) for L, R, s in passes] for passes in sets]          # later passes start from state 2
    forward_everywhere(A, Bm, Pi, ob, sets, forms=(0, PACKED, PACKED | W16, PACKED | DBUF))
    first = oracle.OracleModel(A, Bm, Pi)
    row, _ = first.full_forward(ob, 0, 4, -1)
    first.close()
    dead = row <= -np.finfo(np.float32).max
    assert dead[32:].all() and dead.sum() >= 128           # the case is what it claims
    decodes_equal(A, Bm, Pi, ob, (1, 4))


def test_every_state_unreachable_after_some_step():
    """A band that ends: from step 48 on no state has a finite score, the rows are all -FLT_MAX (every tile maximum says
    "unreachable", the row maximum too) and the decode answers FV_ERR_NO_PRED, as the oracle does."""
    A, Bm, Pi, ob = band_model(48, 2, 4, 64, 32, dead_end=True)
    decodes_equal(A, Bm, Pi, ob, (1, 4), expect_rc=D.ERR_NO_PRED)


def test_saturated_branch_runs_on_the_route_too():
    """The adversarial suite's shape that proves the saturated branch runs (wideB, K = 600): it runs with the option on as well,
    with the same paths."""
    kind, K, M, T, seed = next(w for w in WIDE if w[0] == "wideB" and w[1] == 600)
    A, Bm, Pi, ob = modelgen.wide_model(kind, K, M, T, seed)
    om = oracle.OracleModel(A, Bm, Pi)
    fv = decoder.FlashViterbi(0)
    try:
        fv.set_model(A, Bm, Pi)
        fv.set_option(D.OPT_KERNEL, D.KERNEL_U16_REFINE)
        for N in (1, 4):
            opath, oscore, _, orc = om.full_decode(ob, N, check=False)
            assert orc == 0
            for debug in (0, PACKED, PACKED | W16):
                fv.set_option(D.OPT_DEBUG, debug)
                sat = {}
                for opt in (0, 2):
                    fv.set_option(CODES, opt)
                    path, score, rc = fv.decode_full(ob, N)
                    assert rc == 0 and path.tolist() == opath.tolist() and score == oscore, (N, debug, opt)
                    sat[opt] = fv.stats()["refine_saturated"]
                print(f"wideB K=600 N={N} debug={debug}: saturated columns option 0 / 2: {sat[0]} / {sat[2]}")
                assert sat[0] > 0 and sat[2] > 0, (N, debug, sat)
    finally:
        fv.close()
        om.close()


def test_tile_further_below_the_row_maximum_than_the_code_range():
    """Transitions in [0.1, 1] (the code range is |log 0.1| = 2.3 wide), and one tile of states whose every emission is 1e-10:
    that tile's maximum lies ten code ranges below the row maximum in every row, so d_w itself saturates."""
    K, M, T = 96, 4, 24
    rs = np.random.RandomState(77)
    A = rs.uniform(0.1, 1.0, (K, K))                      # (as the wide-range models: the reference does not need normalised rows)
    Bm = rs.uniform(0.2, 1.0, (K, M))
    Bm[32:48] = 1e-10
    Pi = rs.uniform(0.1, 0.4, K)
    ob = rs.randint(0, M, T).astype(np.int32)
    A, Bm, Pi = hostio.quantize_text16(A), hostio.quantize_text16(Bm), hostio.quantize_text16(Pi)
    sets, _ = sets_for(K, 9, (1, 3))
    forward_everywhere(A, Bm, Pi, ob, sets, forms=(0, PACKED, PACKED | W16))
    om = oracle.OracleModel(A, Bm, Pi)
    row, _ = om.full_forward(ob, 0, 3, -1)
    om.close()
    step = np.log(10.0) / 65534
    assert (row.max() - row[32:48].max()) / step > 65535 * 5          # the case is what it claims
    decodes_equal(A, Bm, Pi, ob, (1, 4))


SMALL = load_goldens()
BIG = [g for g in load_goldens(include_big=True) if g["spec"]["K"] > 1024 and any(r["algo"] == "flash" for r in g["runs"])]


def decode_both(fv, ob, n, flat):
    fv.set_option(D.OPT_FLAT_GENERATIONS, flat)
    out = {}
    for opt in (0, 2):
        fv.set_option(CODES, opt)
        path, score, rc = fv.decode_full(ob, n, D.MODE_REFERENCE)
        st = fv.stats()
        out[opt] = (path.tolist(), np.float32(score).view(np.uint32), rc)
        print(f"n_split {n} flat {flat} option {opt}: refine candidates {st['refine_near']} rescans {st['refine_rescan']} saturated {st['refine_saturated']}")
    assert out[0] == out[2], (n, flat)
    return out[2]


@pytest.mark.parametrize("g", SMALL, ids=[g["name"] for g in SMALL])
def test_decodes_equal_on_every_golden(g):
    A, Bm, Pi, ob = golden_model(g)
    fv = decoder.FlashViterbi(0)
    try:
        fv.set_model(A, Bm, Pi)
        fv.set_option(D.OPT_KERNEL, D.KERNEL_U16_REFINE)
        for n in (1, 2, 8):
            for flat in (0, 2):
                path, score, rc = decode_both(fv, ob, n, flat)
                ref = next((r for r in g["runs"] if r["algo"] == "flash" and r["N"] == n), None)
                if ref is not None:
                    assert rc == 0 and path == ref["path"] and score == np.float32(ref["score"]).view(np.uint32), (n, flat)
        if g["name"] == "ds_K512_T64":
            # the flat form's fall-back: a poisoned snapshot entry, the decode finishes generation by generation
            ref = next(r for r in g["runs"] if r["algo"] == "flash" and r["N"] == 8)
            fv.test_flat_poison(20)
            try:
                path, score, rc = decode_both(fv, ob, 8, 2)
            finally:
                fv.test_flat_poison(-1)
            assert rc == 0 and path == ref["path"] and fv.stats()["flat_first_miss"] >= 1
    finally:
        fv.close()


@pytest.mark.parametrize("g", BIG, ids=[g["name"] for g in BIG])
def test_decodes_equal_on_the_bench_models(g):
    """cfg2 / cfg2b (K = 3965, T = 256): once each, at the bench's n_split, flat form on, against the golden"""
    A, Bm, Pi, ob = golden_model(g)
    fv = decoder.FlashViterbi(0)
    try:
        fv.set_model(A, Bm, Pi)
        fv.set_option(D.OPT_KERNEL, D.KERNEL_U16_REFINE)
        n = 8 if any(r["N"] == 8 for r in g["runs"] if r["algo"] == "flash") else next(r["N"] for r in g["runs"] if r["algo"] == "flash")
        ref = next(r for r in g["runs"] if r["algo"] == "flash" and r["N"] == n)
        path, score, rc = decode_both(fv, ob, n, 2)
        assert rc == 0 and path == ref["path"] and score == np.float32(ref["score"]).view(np.uint32)
    finally:
        fv.close()
