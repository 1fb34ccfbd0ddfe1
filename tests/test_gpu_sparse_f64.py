"""GPU: FV_KERNEL_CSR_F64, the float64 walk over the stored entries of a model set through fv_set_model_sparse.  It
decodes what the filter walk refuses (model entries above 1, staged emission scores above 0) to the bits the same model
gives through fv_set_model under FV_KERNEL_F64_STREAM: goldens, whole step tables against the oracle, the forked
generation, the entry points side by side, emissions, a dead source under a huge score, the vanilla rounding order,
batch / partition / multi-device forms, one K beyond an LDS score row, and the refusals."""
import ctypes

import numpy as np
import pytest

import modelgen
import oracle
from conftest import golden_model, golden_runs, load_goldens
from flash_viterbi_amd import decoder
from test_gpu_sparse_model import (BATCH_SET, BP_FILL, FORK_SET, csr_to_dense, dead_end_model, interleaved_blocks, pass_set,
                                   raw_full, unreachable_model)

pytestmark = pytest.mark.gpu

D = decoder
MEM = D.DEBUG_CSR_ROWS_IN_MEMORY
K8 = D.KERNEL_CSR_F64
TV_NB, TV_MEM = D.TV_CSR64_NB, D.TV_CSR64_MEM
PAIRS, IDS = golden_runs(include_big=True, algo="flash")


def above_one(x, frac, seed):
    """A copy of x with about `frac` of its non-zero entries replaced by values in (1, 50]."""
    rs = np.random.RandomState(seed)
    x = np.array(x, dtype=np.float32, copy=True)
    flat = x.reshape(-1)
    nz = np.nonzero(flat)[0]
    pick = nz[rs.uniform(size=nz.size) < frac]
    if pick.size == 0:
        pick = nz[:1]
    flat[pick] = np.maximum(rs.uniform(1.0, 50.0, pick.size).astype(np.float32), np.nextafter(np.float32(1), np.float32(2)))
    assert (flat[pick] > 1).all() and (x <= 50).all()
    return x


def sparse8(A, B, Pi, device=0, csr=None):
    fv = decoder.FlashViterbi(device)
    fv.set_model_sparse(*(csr if csr is not None else decoder.dense_to_csr(A)), B, Pi)
    fv.set_option(D.OPT_KERNEL, K8)
    return fv


def dense64(A, B, Pi):
    fv = decoder.FlashViterbi(0)
    fv.set_model(A, B, Pi)
    fv.set_option(D.OPT_KERNEL, D.KERNEL_F64_STREAM)
    return fv


def raw_staged(fv, T, N, mode=D.MODE_REFERENCE):
    """fv_decode_full on the staged emission rows (ob == NULL) without the wrapper's exception."""
    path = np.empty(T, dtype=np.int32)
    score = ctypes.c_float(0)
    rc = fv._L.fv_decode_full(fv._h, None, T, N, mode, decoder._p(path), ctypes.byref(score))
    return path, np.float32(score.value), rc


def same_bits(a, b):
    return a[2] == b[2] and a[0].tolist() == b[0].tolist() and np.float32(a[1]).view(np.uint32) == np.float32(b[1]).view(np.uint32)


def refused(call, rc, text=None):
    with pytest.raises(decoder.FlashVitError) as e:
        call()
    assert e.value.rc == rc, str(e.value)
    if text is not None:
        assert text in str(e.value), str(e.value)


# ---------------------------------------------------------------- 1. goldens

@pytest.fixture(scope="module")
def ctxs():
    cache = {}

    def get(g):
        if g["name"] not in cache:
            A, B, Pi, ob = golden_model(g)
            cache[g["name"]] = (sparse8(A, B, Pi), ob)
        return cache[g["name"]]
    yield get
    for sp, _ in cache.values():
        sp.close()


@pytest.mark.parametrize("g,r", PAIRS, ids=IDS)
def test_goldens_under_the_float64_walk(ctxs, g, r):
    sp, ob = ctxs(g)
    try:
        for batch in (1, 8):
            for dbg in (0, MEM):
                sp.set_option(D.OPT_MAX_BATCH, batch)
                sp.set_option(D.OPT_DEBUG, dbg)
                where = f"max_batch={batch} debug={dbg}"
                path, score, rc = sp.decode_full(ob, r["N"], D.MODE_REFERENCE)
                assert rc == 0 and path.tolist() == r["path"] and score == np.float32(r["score"]), where
                assert sp.stats()["kernel"] == K8 == 8, where
    finally:
        sp.set_option(D.OPT_MAX_BATCH, 8)
        sp.set_option(D.OPT_DEBUG, 0)


# ---------------------------------------------------------------- 2. whole step tables

def table_model(kind, K, T, seed):
    if kind == "dense70":
        # columns of about 700 entries: 44 wave-blocks per tile, more than four per wave — the chunked loop reloads
        A, Bm, Pi, ob = modelgen.model32(dict(kind="sparse_fast", K=K, M=8, T=T, prob=0.7, seed=seed))
        return above_one(A, 0.05, seed), Bm, Pi, ob
    if kind == "unreachable":
        return unreachable_model(K, 8, T, seed)
    if kind == "ties_all":
        return modelgen.model32(dict(kind="ties_all", K=K, M=8, T=T, prob=0.5, seed=seed))
    A, Bm, Pi, ob = modelgen.model32(dict(kind="sparse_fast", K=K, M=8, T=T, prob=0.05, seed=seed))
    return above_one(A, 0.05, seed), Bm, Pi, ob


def oracle_tables(om, ob, passes):
    return [om.full_forward(ob, L, R, s) for L, R, s in passes]


def check_tables(want, passes, rows, bp, where):
    covered = np.zeros(bp.shape[0], dtype=bool)
    for q, (L, R, s) in enumerate(passes):
        row, args = want[q]
        bad = np.nonzero(rows[q].view(np.uint32) != row.view(np.uint32))[0]
        assert bad.size == 0, f"{where} pass ({L},{R},{s}): final score row differs in {bad.size} columns, first {bad[:8].tolist()}"
        diff = np.argwhere(bp[L + 1:R + 1] != args)
        assert diff.size == 0, (f"{where} pass ({L},{R},{s}): {len(diff)} back-pointers differ, first at time "
                                f"{L + 1 + diff[0][0]} column {diff[0][1]}")
        covered[L + 1:R + 1] = True
    assert (bp[~covered] == BP_FILL).all(), f"{where}: the hook wrote back-pointer rows outside its passes"


TABLE_MODELS = [("sparse_fast", 33), ("sparse_fast", 257), ("sparse_fast", 1000), ("dense70", 1000), ("ties_all", 512),
                ("unreachable", 300)]


@pytest.mark.parametrize("kind,K", TABLE_MODELS, ids=[f"{k}-K{n}" for k, n in TABLE_MODELS])
def test_whole_step_tables_against_the_oracle(kind, K):
    passes, T = pass_set(BATCH_SET, K, 300 + K)
    A, Bm, Pi, ob = table_model(kind, K, T + 2, 400 + K)
    om = oracle.OracleModel(A, Bm, Pi)
    fv = sparse8(A, Bm, Pi)
    try:
        want = oracle_tables(om, ob, passes)
        if kind == "unreachable":
            assert any((args == -1).any() for _, args in want)
        if kind in ("sparse_fast", "dense70"):
            assert (A > 1).any()
        for dbg in (0, MEM):
            for batch in (1, 2, 4, 8):
                fv.set_option(D.OPT_DEBUG, dbg)
                fv.set_option(D.OPT_MAX_BATCH, batch)
                rows, bp, var = fv.test_forward(ob, passes, BP_FILL)
                where = f"{kind} K={K} debug={dbg} batch={batch}"
                assert fv.stats()["kernel"] == K8, where
                check_tables(want, passes, rows, bp, where)
                # launches of up to `batch` tasks: exactly the instantiations NB <= batch, and the memory bit with bit 31 only
                bits = sum(b for b, nb in zip(TV_NB, (1, 2, 4, 8)) if nb <= batch) | (TV_MEM if dbg else 0)
                assert var == bits, f"{where}: instantiations {var:#x}, want {bits:#x}"
    finally:
        fv.close()
        om.close()


# ---------------------------------------------------------------- 3. forked generation

def test_forked_generation_step_tables():
    """Six passes of 64+ steps: batches of four on three streams, both score-row forms, and the single-stream form."""
    K = 257
    passes, T = pass_set(FORK_SET, K, 77)
    A, Bm, Pi, ob = table_model("sparse_fast", K, T + 1, 78)
    om = oracle.OracleModel(A, Bm, Pi)
    fv = sparse8(A, Bm, Pi)
    try:
        want = oracle_tables(om, ob, passes)
        for dbg in (0, MEM, 1 << 18, (1 << 18) | MEM):
            fv.set_option(D.OPT_DEBUG, dbg)
            rows, bp, var = fv.test_forward(ob, passes, BP_FILL)
            check_tables(want, passes, rows, bp, f"fork debug={dbg}")
            assert fv.stats()["kernel"] == K8
            assert var & sum(TV_NB) and not var & ~(sum(TV_NB) | TV_MEM) and bool(var & TV_MEM) == bool(dbg & MEM)
    finally:
        fv.close()
        om.close()


# ---------------------------------------------------------------- 4. entry points agree

def compare_entry_points(A, Bm, Pi, ob, splits, expect_rc=None):
    """sparse-set context under the float64 walk, dense-set context under F64_STREAM and the oracle: path, score bits and
    return code, both score-row forms."""
    om = oracle.OracleModel(A, Bm, Pi)
    de = dense64(A, Bm, Pi)
    sp = sparse8(A, Bm, Pi)
    out = []
    try:
        for N in splits:
            opath, oscore, _, orc = om.full_decode(ob, N, check=False)
            dense = raw_full(de, ob, N)
            assert de.stats()["kernel"] == D.KERNEL_F64_STREAM
            for dbg in (0, MEM):
                sp.set_option(D.OPT_DEBUG, dbg)
                got = raw_full(sp, ob, N)
                where = f"N={N} debug={dbg}"
                assert got[2] in (0, D.ERR_NO_PRED) and same_bits(got, dense), where
                assert sp.stats()["kernel"] == K8, where
                if expect_rc is not None:
                    assert got[2] == expect_rc, where
                if orc == 0:
                    assert got[2] == 0 and got[0].tolist() == opath.tolist() and got[1] == oscore, where
                else:
                    assert got[2] == D.ERR_NO_PRED and (got[0] < 0).any(), where
                out.append(got)
    finally:
        sp.close()
        de.close()
        om.close()
    return out


@pytest.mark.parametrize("which", ["A", "B", "AB"])
def test_models_above_one_equal_the_dense_float64_kernel_and_the_oracle(which):
    for K, T, seed in ((600, 48, 5), (257, 90, 6)):
        A, Bm, Pi, ob = modelgen.model32(dict(kind="sparse_fast", K=K, M=8, T=T, prob=0.05, seed=seed))
        if "A" in which:
            A = above_one(A, 0.05, seed + 10)
        if "B" in which:
            Bm = above_one(Bm, 0.05, seed + 20)
        compare_entry_points(A, Bm, Pi, ob, splits=(1, 4), expect_rc=0)


def test_no_predecessor_sequence_equals_the_dense_float64_kernel():
    A, Bm, Pi = dead_end_model()
    bad = np.array([0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0], np.int32)
    out = compare_entry_points(A, Bm, Pi, bad, splits=(1, 2), expect_rc=D.ERR_NO_PRED)
    assert all((p < 0).any() for p, _, _ in out)


# ---------------------------------------------------------------- 5. emission scores above 0

def test_emission_scores_above_zero():
    """The inputs of test_gpu_emissions.py::test_scores_above_zero_take_the_float64_kernels on a sparse-set context."""
    from test_gpu_emissions import free_emissions, golden, libm_log
    g = golden("ds_K200_T100")
    A, _, Pi, ob = golden_model(g)
    K, T = A.shape[0], len(ob)
    E = free_emissions(T, K)
    rs = np.random.RandomState(8)
    up = rs.uniform(size=(T, K)) < 0.05
    big = rs.uniform(1.0, 50.0, size=int(up.sum())).astype(np.float32)
    big[big <= 1] = 50
    E[up] = big                                             # densities in (1, 50]
    assert (E[up] > 1).all() and (E <= 50).all()
    logE = libm_log(E)
    t = np.arange(T, dtype=np.int32)
    B = np.full((K, 2), 0.5, np.float32)
    om = oracle.OracleModel(A, np.ascontiguousarray(E.T), Pi)
    de = dense64(A, B, Pi)
    sp = decoder.FlashViterbi(0)
    try:
        sp.set_model_sparse(*decoder.dense_to_csr(A), B, Pi)
        for staged in (logE, logE.astype(np.float32)):
            de.set_emissions(staged)
            sp.set_emissions(staged)
            sp.set_option(D.OPT_KERNEL, D.KERNEL_AUTO)
            refused(lambda: sp.decode_full(None, 4, T=T), D.ERR_UNSUPPORTED, "[0,1]")
            sp.set_option(D.OPT_KERNEL, K8)
            for N in (1, 4):
                for dbg in (0, MEM):
                    sp.set_option(D.OPT_DEBUG, dbg)
                    got = raw_staged(sp, T, N)
                    where = f"{staged.dtype} N={N} debug={dbg}"
                    assert same_bits(got, raw_staged(de, T, N)), where
                    assert sp.stats()["kernel"] == K8 and de.stats()["kernel"] == D.KERNEL_F64_STREAM, where
                    if staged.dtype == np.float64:          # (the oracle takes probabilities: it has no float32-rounded logs)
                        opath, oscore, _, orc = om.full_decode(t, N)
                        assert got[2] == orc == 0 and got[0].tolist() == opath.tolist() and got[1] == oscore, where
            # a symbol decode of the same context is within [0, 1]: the filter walk takes it again
            sp.set_option(D.OPT_KERNEL, D.KERNEL_AUTO)
            assert sp.decode_full(np.zeros(T, np.int32), 4)[2] == 0 and sp.stats()["kernel"] == D.KERNEL_SPARSE_CSR
    finally:
        de.close()
        sp.close()
        om.close()


# ---------------------------------------------------------------- 6. a dead source under a huge score

def test_dead_source_with_a_huge_score_equals_the_dense_float64_kernel():
    """Column 5's only stored predecessor is state 7, which nothing reaches and Pi excludes: from time 1 on its score is
    -FLT_MAX.  Under a staged score of 1e32 at (time 2, column 5) the cell evaluates above -FLT_MAX (the float spacing
    there is 2e31), and the reference's strict '>' from -FLT_MAX takes it: the float64 kernels must not read a dead
    source as -inf.  The oracle takes probabilities and cannot express a score of 1e32: the dense float64 kernel judges."""
    K, T = 33, 6
    rs = np.random.RandomState(66)
    A = (rs.uniform(0.1, 1.0, (K, K)) * (rs.uniform(0, 1, (K, K)) < 0.3)).astype(np.float32)
    A[np.arange(K), (np.arange(K) + 1) % K] = 0.5
    A[:, 7] = 0.0
    A[:, 5] = 0.0
    A[7, 5] = 0.5
    Pi = np.full(K, 1.0 / K, np.float32)
    Pi[7] = 0.0
    B = np.full((K, 2), 0.5, np.float32)
    logE = np.log(rs.uniform(0.1, 1.0, (T, K)))
    logE[2, 5] = 1e32
    passes = [(0, T - 1, -1)]
    sp = sparse8(A, B, Pi)
    de = dense64(A, B, Pi)
    try:
        for staged in (logE, logE.astype(np.float32)):
            de.set_emissions(staged)
            sp.set_emissions(staged)
            drows, dbp, _ = de.test_forward(None, passes, BP_FILL, T=T)
            assert dbp[1, 7] == -1 and dbp[2, 5] == 7 and dbp[2, 7] == -1, "the input must put the dead source to use"
            for dbg in (0, MEM):
                sp.set_option(D.OPT_DEBUG, dbg)
                rows, bp, var = sp.test_forward(None, passes, BP_FILL, T=T)
                where = f"{staged.dtype} debug={dbg}"
                assert np.array_equal(rows.view(np.uint32), drows.view(np.uint32)) and np.array_equal(bp, dbp), where
                assert var == TV_NB[0] | (TV_MEM if dbg else 0), where
                for N in (1, 2):
                    assert same_bits(raw_staged(sp, T, N), raw_staged(de, T, N)), f"{where} N={N}"
    finally:
        sp.close()
        de.close()


# ---------------------------------------------------------------- 7. vanilla

def vanilla_case(A, Bm, Pi, ob, golden_path=None):
    om = oracle.OracleModel(A, Bm, Pi)
    de = dense64(A, Bm, Pi)
    sp = sparse8(A, Bm, Pi)
    try:
        want = om.vanilla_decode(ob)
        dense = de.decode_vanilla(ob)
        for dbg in (0, MEM):
            sp.set_option(D.OPT_DEBUG, dbg)
            got = sp.decode_vanilla(ob)
            assert same_bits(got, dense) and same_bits(got, want), f"debug={dbg}"
            assert sp.stats()["kernel"] == K8
            if golden_path is not None:
                assert got[0].tolist() == golden_path
        # the walk's own rounding order is back afterwards
        assert same_bits(raw_full(sp, ob, 1), raw_full(de, ob, 1))
        sp.set_option(D.OPT_KERNEL, D.KERNEL_AUTO)
        refused(lambda: sp.decode_vanilla(ob), D.ERR_UNSUPPORTED, "fv_set_model_sparse")
    finally:
        sp.close()
        de.close()
        om.close()


@pytest.mark.parametrize("name", ["ds_K200_T100", "ties_semi_K96_T80"])
def test_vanilla_on_goldens(name):
    g = [x for x in load_goldens(True) if x["name"] == name][0]
    run = next(r for r in g["runs"] if r["algo"] == "vanilla")
    vanilla_case(*golden_model(g), golden_path=run["path"])


def test_vanilla_on_a_model_above_one():
    A, Bm, Pi, ob = modelgen.model32(dict(kind="sparse_fast", K=300, M=6, T=70, prob=0.05, seed=91))
    vanilla_case(above_one(A, 0.05, 92), above_one(Bm, 0.05, 93), Pi, ob)


# ---------------------------------------------------------------- 8. batch, partition, multi-device

def test_batch_of_ragged_sequences_equals_single_decodes():
    A, Bm, Pi, ob = modelgen.model32(dict(kind="sparse_fast", K=500, M=7, T=300, prob=0.04, seed=31))
    A = above_one(A, 0.05, 33)
    seqs = [ob[:200], ob[50:57], ob[100:300], ob[:2], ob[7:140], ob[3:90], ob[:64], ob[200:231], ob[1:100]]
    fv = sparse8(A, Bm, Pi)
    de = dense64(A, Bm, Pi)
    try:
        for mode, N in ((D.MODE_REFERENCE, 4), (D.MODE_SINGLE_PASS, 1)):
            fv.set_option(D.OPT_DEBUG, 0)
            fv.set_option(D.OPT_MAX_BATCH, 8)
            want = [fv.decode_full(o, N, mode) for o in seqs]
            assert same_bits(want[0], de.decode_full(seqs[0], N, mode))
            for batch in (1, 3, 8):
                for dbg in (0, MEM, 1 << 28):
                    fv.set_option(D.OPT_MAX_BATCH, batch)
                    fv.set_option(D.OPT_DEBUG, dbg)
                    paths, scores, statuses = fv.decode_full_batch(seqs, N, mode)
                    where = f"mode={mode} N={N} batch={batch} debug={dbg}"
                    assert not statuses.any() and fv.stats()["kernel"] == K8, where
                    for s, (p, sc, _) in enumerate(want):
                        assert paths[s].tolist() == p.tolist() and scores[s] == sc, f"{where} sequence {s}"
    finally:
        fv.close()
        de.close()


def test_batch_with_one_no_predecessor_sequence():
    A, Bm, Pi = dead_end_model()
    good = np.zeros(20, np.int32)
    bad = good.copy()
    bad[9] = 1
    fv = sparse8(A, Bm, Pi)
    de = dense64(A, Bm, Pi)
    try:
        for dbg in (0, MEM):
            fv.set_option(D.OPT_DEBUG, dbg)
            paths, scores, statuses = fv.decode_full_batch([good, bad, good[:11]], 2)
            dpaths, dscores, dstatuses = de.decode_full_batch([good, bad, good[:11]], 2)
            assert statuses.tolist() == [0, D.ERR_NO_PRED, 0] == dstatuses.tolist()
            assert (paths[1] < 0).any() and fv.stats()["kernel"] == K8
            for s, o in enumerate((good, bad, good[:11])):
                assert paths[s].tolist() == dpaths[s].tolist() and scores[s].view(np.uint32) == dscores[s].view(np.uint32)
                single = raw_full(fv, o, 2)
                assert single[2] == statuses[s] and single[0].tolist() == paths[s].tolist() and single[1] == scores[s]
    finally:
        fv.close()
        de.close()


def test_partition_of_three_ranks_merges_to_the_one_rank_path():
    A, Bm, Pi, ob = modelgen.model32(dict(kind="sparse_fast", K=400, M=6, T=96, prob=0.05, seed=41))
    A = above_one(A, 0.05, 42)
    N, nranks = 6, 3
    fv = sparse8(A, Bm, Pi)
    try:
        whole, score, rc = fv.decode_full(ob, N)
        assert rc == 0
        gathered = []
        for rank in range(nranks):
            fv.set_partition(rank, nranks)
            p, sc, rc = fv.decode_full(ob, N)
            assert rc == 0 and sc == score and fv.stats()["kernel"] == K8
            gathered.append(p)
        fv.set_partition(0, 1)
        merged = decoder.merge_paths(ob.size, N, nranks, np.stack(gathered))
        assert merged.tolist() == whole.tolist()
        om = oracle.OracleModel(A, Bm, Pi)
        assert om.full_decode(ob, N)[0].tolist() == whole.tolist()
        om.close()
    finally:
        fv.close()


def test_multi_device_context_equals_the_plain_one():
    A, Bm, Pi, ob = modelgen.model32(dict(kind="sparse_fast", K=400, M=6, T=96, prob=0.05, seed=43))
    A = above_one(A, 0.05, 44)
    plain = sparse8(A, Bm, Pi)
    group = sparse8(A, Bm, Pi, device=[0, 0])
    try:
        for N in (1, 4, 8):
            a, b = plain.decode_full(ob, N), group.decode_full(ob, N)
            assert a[2] == b[2] == 0 and a[0].tolist() == b[0].tolist() and a[1] == b[1]
        assert group.stats()["kernel"] == K8 and group.stats()["ranks"] == 2
    finally:
        plain.close()
        group.close()


# ---------------------------------------------------------------- 9. beyond one LDS score row

def test_beyond_one_lds_score_row_equals_the_best_block_of_the_oracle():
    """K = 45056 = 64 interleaved blocks of 704 states: a float32 score row (180 KB) does not fit LDS, so every launch reads
    its rows from memory without FV_OPT_DEBUG bit 31.  The blocks never exchange score, so the decode of the whole model
    is the decode of the block with the largest whole-sequence score (asserted unique), mapped through s * 64 + b."""
    NB_, Kb, M, T = 64, 704, 6, 8
    (ip, ix, dt, Bm, Pi), blocks = interleaved_blocks(NB_, Kb, M, 515)
    K = NB_ * Kb
    dt = above_one(dt, 0.01, 516)
    assert (dt > 1).any()
    ob = np.random.RandomState(517).randint(0, M, T).astype(np.int32)
    fv = sparse8(None, Bm, Pi, csr=(ip, ix, dt))
    got = {}
    try:
        for N in (3, 1):
            got[N] = fv.decode_full(ob, N)
            assert fv.stats()["kernel"] == K8
        _, _, var = fv.test_forward(ob, [(0, 3, -1), (4, 6, 17)])
        assert var == TV_NB[0] | TV_NB[1] | TV_MEM          # launches of two tasks and of one, rows in memory
    finally:
        fv.close()
    row_of = np.repeat(np.arange(K, dtype=np.int64), np.diff(ip))
    want = {3: [], 1: []}
    for b, (bip, bix, _, Bb, Pib) in enumerate(blocks):
        # block b's entries are rows b, b + 64, ... of the whole model, in the block's own order
        om = oracle.OracleModel(csr_to_dense(bip, bix, dt[row_of % NB_ == b], Kb), Bb, Pib)
        for N in (3, 1):
            want[N].append(om.full_decode(ob, N))
        om.close()
    for N in (3, 1):
        scores = np.array([r[1] for r in want[N]])
        b = int(np.argmax(scores))
        assert (scores == scores[b]).sum() == 1, "the best block's score must be unique (a condition on the input)"
        assert all(r[3] == 0 for r in want[N])
        wpath = want[N][b][0].astype(np.int64) * NB_ + b
        path, score, rc = got[N]
        assert rc == 0 and path.tolist() == wpath.tolist() and score == scores[b], f"N={N}"


# ---------------------------------------------------------------- 10. refusals and unchanged behaviour

def test_float64_walk_on_a_dense_set_model_is_refused():
    g = [x for x in load_goldens() if x["name"] == "ds_K77_M7_T33"][0]
    A, Bm, Pi, ob = golden_model(g)
    flash = next(r for r in g["runs"] if r["algo"] == "flash")
    fv = decoder.FlashViterbi(0)
    try:
        fv.set_model(A, Bm, Pi)
        fv.set_option(D.OPT_KERNEL, K8)
        refused(lambda: fv.decode_full(ob, flash["N"]), D.ERR_UNSUPPORTED, "fv_set_model_sparse")
        refused(lambda: fv.decode_full_batch([ob, ob], flash["N"]), D.ERR_UNSUPPORTED, "fv_set_model_sparse")
        refused(lambda: fv.test_forward(ob, [(0, 5, -1)]), D.ERR_UNSUPPORTED, "fv_set_model_sparse")
        fv.set_option(D.OPT_KERNEL, D.KERNEL_AUTO)
        path, score, rc = fv.decode_full(ob, flash["N"])
        assert rc == 0 and path.tolist() == flash["path"] and score == np.float32(flash["score"])
        for bad in (7, 9):
            refused(lambda: fv.set_option(D.OPT_KERNEL, bad), D.ERR_ARG)
    finally:
        fv.close()


def test_out_of_scope_calls_stay_refused_and_auto_refuses_again():
    g = [x for x in load_goldens() if x["name"] == "ds_K77_M7_T33"][0]
    A, Bm, Pi, ob = golden_model(g)
    flash = next(r for r in g["runs"] if r["algo"] == "flash")
    fv = sparse8(A, Bm, Pi)
    try:
        for what, call in (("checkpoint", lambda: fv.decode_checkpoint(ob)), ("beam", lambda: fv.decode_beam(ob, 4, 16)),
                           ("beam batch", lambda: fv.decode_beam_batch([ob, ob], 4, 16))):
            refused(call, D.ERR_UNSUPPORTED, "fv_set_model_sparse")
        assert fv.decode_full(ob, flash["N"])[0].tolist() == flash["path"] and fv.stats()["kernel"] == K8
        # an above-1 model: decoded under the float64 walk, refused again under AUTO and SPARSE_Q16 with the old words
        big = above_one(A, 0.05, 7)
        fv.set_model_sparse(*decoder.dense_to_csr(big), Bm, Pi)
        assert fv.decode_full(ob, 2)[2] == 0 and fv.stats()["kernel"] == K8
        for kernel in (D.KERNEL_AUTO, D.KERNEL_SPARSE_Q16):
            fv.set_option(D.OPT_KERNEL, kernel)
            refused(lambda: fv.decode_full(ob, 2), D.ERR_UNSUPPORTED, "[0,1]")
            refused(lambda: fv.decode_full_batch([ob, ob], 2), D.ERR_UNSUPPORTED, "[0,1]")
        fv.set_option(D.OPT_KERNEL, D.KERNEL_F64_STREAM)
        refused(lambda: fv.decode_full(ob, 2), D.ERR_UNSUPPORTED, "fv_set_model_sparse")
    finally:
        fv.close()
