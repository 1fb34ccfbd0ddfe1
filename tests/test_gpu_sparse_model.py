"""GPU: models set through fv_set_model_sparse (CSR, no K x K table anywhere) decode to the bits the same model gives
through fv_set_model: goldens, whole step tables against the oracle, structure the generators do not draw, batch /
partition / multi-device forms, one K beyond an LDS score row, one K beyond what fv_set_model can hold, and the
refusals."""
import ctypes
import time

import numpy as np
import pytest

import modelgen
import oracle
from conftest import golden_model, golden_runs
from flash_viterbi_amd import decoder
from flash_viterbi_amd.generate_data import data_script

pytestmark = pytest.mark.gpu

D = decoder
MEM = D.DEBUG_CSR_ROWS_IN_MEMORY
PAIRS, IDS = golden_runs(include_big=True, algo="flash")
FLT_MAX = np.finfo(np.float32).max
# FV_TV_CSR_* of include/flashvit_testing.h: trellis_step_csr<NB, MEM>, NB = 1, 2, 4, 8
TV_LDS = [1 << (50 + q) for q in range(4)]
TV_MEM = [1 << (54 + q) for q in range(4)]


def _log(msg):
    print(f"[sparse-model] {msg}", flush=True)


def csr_to_dense(indptr, indices, data, K):
    A = np.zeros((K, K), dtype=np.float32)
    A[np.repeat(np.arange(K), np.diff(indptr)), indices] = data
    return A


def sparse_ctx(A, B, Pi, device=0):
    fv = decoder.FlashViterbi(device)
    fv.set_model_sparse(*decoder.dense_to_csr(A), B, Pi)
    return fv


def dense_ctx(A, B, Pi):
    fv = decoder.FlashViterbi(0)
    fv.set_model(A, B, Pi)
    return fv


# ---------------------------------------------------------------- 2. goldens

@pytest.fixture(scope="module")
def ctxs():
    cache = {}

    def get(g):
        if g["name"] not in cache:
            A, B, Pi, ob = golden_model(g)
            cache[g["name"]] = (sparse_ctx(A, B, Pi), dense_ctx(A, B, Pi), ob)
        return cache[g["name"]]
    yield get
    for sp, de, _ in cache.values():
        sp.close()
        de.close()


@pytest.mark.parametrize("g,r", PAIRS, ids=IDS)
def test_goldens_through_the_sparse_entry_point(ctxs, g, r):
    sp, de, ob = ctxs(g)
    de.set_option(D.OPT_KERNEL, D.KERNEL_AUTO)
    want_single = de.decode_full(ob, r["N"], D.MODE_SINGLE_PASS)
    try:
        for batch in (1, 8):
            for dbg in (0, MEM):
                sp.set_option(D.OPT_MAX_BATCH, batch)
                sp.set_option(D.OPT_DEBUG, dbg)
                where = f"max_batch={batch} debug={dbg}"
                path, score, rc = sp.decode_full(ob, r["N"], D.MODE_REFERENCE)
                assert rc == 0 and path.tolist() == r["path"] and score == np.float32(r["score"]), where
                st = sp.stats()
                assert st["kernel"] == D.KERNEL_SPARSE_CSR == 7, where
                assert st["density"] == pytest.approx(np.count_nonzero(golden_model(g)[0]) / float(sp.K) ** 2), where
                path, score, rc = sp.decode_full(ob, r["N"], D.MODE_SINGLE_PASS)
                assert rc == want_single[2] and path.tolist() == want_single[0].tolist() and score == want_single[1], where
    finally:
        sp.set_option(D.OPT_MAX_BATCH, 8)
        sp.set_option(D.OPT_DEBUG, 0)


# ---------------------------------------------------------------- 3. whole step tables

BP_FILL = -2
BATCH_SET = (9, 8, 6, 5, 4, 3, 2, 1)        # a batch limit of 8 gives launches of 8, 7, ... 1 tasks: every NB
FORK_SET = (70, 64, 66, 80, 64, 65)         # five or more passes of 64+ steps: batches of four dealt to three streams


def pass_set(lengths, K, seed):
    rs = np.random.RandomState(seed)
    passes, L = [], 0
    for n in lengths:
        passes.append((L, L + n, -1 if L == 0 else int(rs.randint(0, K))))
        L += n + 1 + int(rs.randint(0, 2))
    order = rs.permutation(len(passes))
    return [passes[i] for i in order], L


unreachable_model = modelgen.unreachable_fast        # every 7th column of A zero, a third of Pi zero


def table_model(kind, K, T, seed):
    if kind in ("wideB", "wideAB"):
        return modelgen.wide_model(kind, K, 8, T, seed)
    if kind == "unreachable":
        return unreachable_model(K, 8, T, seed)
    if kind == "ties_all":
        return modelgen.model32(dict(kind="ties_all", K=K, M=8, T=T, prob=0.5, seed=seed))
    return modelgen.model32(dict(kind="sparse_fast", K=K, M=8, T=T, prob=0.05, seed=seed))


def check_tables(om, ob, passes, rows, bp, where):
    covered = np.zeros(bp.shape[0], dtype=bool)
    for q, (L, R, s) in enumerate(passes):
        row, args = om.full_forward(ob, L, R, s)
        bad = np.nonzero(rows[q].view(np.uint32) != row.view(np.uint32))[0]
        assert bad.size == 0, f"{where} pass ({L},{R},{s}): final score row differs in {bad.size} columns, first {bad[:8].tolist()}"
        diff = np.argwhere(bp[L + 1:R + 1] != args)
        assert diff.size == 0, (f"{where} pass ({L},{R},{s}): {len(diff)} back-pointers differ, first at time "
                                f"{L + 1 + diff[0][0]} column {diff[0][1]}")
        covered[L + 1:R + 1] = True
    assert (bp[~covered] == BP_FILL).all(), f"{where}: the hook wrote back-pointer rows outside its passes"


TABLE_MODELS = [("sparse_fast", 1000), ("sparse_fast", 257), ("sparse_fast", 33), ("ties_all", 512), ("unreachable", 300),
                ("wideB", 600)]


@pytest.mark.parametrize("kind,K", TABLE_MODELS, ids=[f"{k}-K{n}" for k, n in TABLE_MODELS])
def test_whole_step_tables_against_the_oracle(kind, K):
    passes, T = pass_set(BATCH_SET, K, 300 + K)
    A, Bm, Pi, ob = table_model(kind, K, T + 2, 400 + K)
    om = oracle.OracleModel(A, Bm, Pi)
    fv = sparse_ctx(A, Bm, Pi)
    try:
        if kind == "unreachable":
            assert any((om.full_forward(ob, L, R, s)[1] == -1).any() for L, R, s in passes)
        for dbg, bits in ((0, TV_LDS), (MEM, TV_MEM)):
            seen = 0
            for batch in (1, 2, 4, 8):
                fv.set_option(D.OPT_DEBUG, dbg)
                fv.set_option(D.OPT_MAX_BATCH, batch)
                rows, bp, var = fv.test_forward(ob, passes, BP_FILL)
                rows2, bp2, var2 = fv.test_forward(ob, passes, BP_FILL)
                where = f"{kind} K={K} debug={dbg} batch={batch}"
                assert np.array_equal(rows.view(np.uint32), rows2.view(np.uint32)) and np.array_equal(bp, bp2) and var == var2, where
                assert fv.stats()["kernel"] == 7
                check_tables(om, ob, passes, rows, bp, where)
                # launches of up to `batch` tasks: exactly the instantiations NB <= batch of this form, nothing else
                want = sum(b for b, nb in zip(bits, (1, 2, 4, 8)) if nb <= batch)
                assert var == want, f"{where}: instantiations {var:#x}, want {want:#x}"
                seen |= var
            assert seen == sum(bits)
    finally:
        fv.close()
        om.close()


def test_forked_generation_step_tables():
    """Six passes of 64+ steps: batches of four on three streams, both score-row forms, and the single-stream form."""
    K = 257
    passes, T = pass_set(FORK_SET, K, 77)
    A, Bm, Pi, ob = table_model("sparse_fast", K, T + 1, 78)
    om = oracle.OracleModel(A, Bm, Pi)
    fv = sparse_ctx(A, Bm, Pi)
    try:
        for dbg in (0, MEM, 262144, 262144 | MEM):
            fv.set_option(D.OPT_DEBUG, dbg)
            rows, bp, var = fv.test_forward(ob, passes, BP_FILL)
            check_tables(om, ob, passes, rows, bp, f"fork debug={dbg}")
            assert var & sum(TV_MEM if dbg & MEM else TV_LDS) and not var & sum(TV_LDS if dbg & MEM else TV_MEM)
    finally:
        fv.close()
        om.close()


# ---------------------------------------------------------------- 4. same bits as the dense entry point

def raw_full(fv, ob, N, mode=D.MODE_REFERENCE):
    """fv_decode_full without the wrapper's exception: FV_ERR_NO_PRED keeps its path with the -1 entries."""
    o = np.ascontiguousarray(ob, dtype=np.int32)
    path = np.empty(o.size, dtype=np.int32)
    score = ctypes.c_float(0)
    rc = fv._L.fv_decode_full(fv._h, decoder._p(o), o.size, N, mode, decoder._p(path), ctypes.byref(score))
    return path, np.float32(score.value), rc


def compare_entry_points(A, Bm, Pi, ob, splits=(1, 3), csr=None, expect_rc=None):
    """dense-set context, sparse-set context and the oracle: path, score and return code, both score-row forms."""
    om = oracle.OracleModel(A, Bm, Pi)
    de = dense_ctx(A, Bm, Pi)
    sp = decoder.FlashViterbi(0)
    sp.set_model_sparse(*(csr if csr is not None else decoder.dense_to_csr(A)), Bm, Pi)
    out = []
    try:
        for N in splits:
            opath, oscore, _, orc = om.full_decode(ob, N, check=False)
            for kernel in (D.KERNEL_AUTO, D.KERNEL_F64_STREAM):
                de.set_option(D.OPT_KERNEL, kernel)
                dpath, dscore, drc = raw_full(de, ob, N)
                for dbg in (0, MEM):
                    sp.set_option(D.OPT_DEBUG, dbg)
                    spath, sscore, src = raw_full(sp, ob, N)
                    where = f"N={N} dense kernel={kernel} debug={dbg}"
                    assert src == drc and src in (0, D.ERR_NO_PRED), where
                    assert spath.tolist() == dpath.tolist(), where
                    assert sscore.view(np.uint32) == dscore.view(np.uint32), where
                    if expect_rc is not None:
                        assert src == expect_rc, where
                    if orc == 0:
                        assert src == 0 and spath.tolist() == opath.tolist() and sscore == oscore, where
                    else:
                        assert src == D.ERR_NO_PRED and (spath < 0).any(), where
                    assert sp.stats()["kernel"] == 7
                    out.append((src, spath.copy()))
    finally:
        sp.close()
        de.close()
        om.close()
    return out


@pytest.mark.parametrize("kind", ["wideB", "wideAB"])
def test_wide_range_models_equal_the_dense_entry_point(kind):
    for K, T, seed in ((600, 48, 5), (257, 90, 6)):
        compare_entry_points(*modelgen.wide_model(kind, K, 8, T, seed), splits=(1, 4))


def test_stored_zeros_equal_absent_entries():
    A, Bm, Pi, ob = modelgen.model32(dict(kind="sparse_fast", K=300, M=6, T=40, prob=0.05, seed=21))
    indptr, indices, data = decoder.dense_to_csr(A)
    # the same matrix with every fourth absent entry of each row stored as an explicit 0
    rows, cols = np.nonzero(A == 0)
    keep = np.arange(rows.size) % 4 == 0
    A2 = A.copy()
    marker = np.float32(7.0)
    A2[rows[keep], cols[keep]] = marker
    ip2, ix2, dt2 = decoder.dense_to_csr(A2)
    dt2 = dt2.copy()
    dt2[dt2 == marker] = 0.0
    assert ip2[-1] > indptr[-1] and (dt2 == 0).sum() == keep.sum()
    a = compare_entry_points(A, Bm, Pi, ob)
    b = compare_entry_points(A, Bm, Pi, ob, csr=(ip2, ix2, dt2))
    assert all(x[0] == y[0] and x[1].tolist() == y[1].tolist() for x, y in zip(a, b))
    fv = decoder.FlashViterbi(0)
    try:
        fv.set_model_sparse(ip2, ix2, dt2, Bm, Pi)
        fv.decode_full(ob, 1)
        assert fv.stats()["density"] == pytest.approx(np.count_nonzero(A) / 300.0 ** 2)
    finally:
        fv.close()


def structured_model(K, seed):
    """Structure no generator draws: column 3 has in-degree K, columns 5, 6 and K - 1 have no in-edge, states 10 .. 19
    have no out-edge (rows empty but for the full column), the rest is a sparse random graph."""
    rs = np.random.RandomState(seed)
    A = rs.uniform(0.1, 1.0, (K, K)) * (rs.uniform(0, 1, (K, K)) < 0.04)
    A[10:20] = 0.0
    A[:, 3] = rs.uniform(0.1, 1.0, K)
    A[:, [5, 6, K - 1]] = 0.0
    A /= np.maximum(A.sum(axis=1), 1e-30)[:, None]
    Bm = rs.uniform(0.1, 1.0, (K, 5))
    Bm /= Bm.sum(axis=1)[:, None]
    Pi = np.full(K, 1.0 / K)
    q = modelgen.hostio.quantize_text16
    return q(A), q(Bm), q(Pi), rs.randint(0, 5, 60).astype(np.int32)


@pytest.mark.parametrize("K", [64, 333, 1000])
def test_hand_built_structure_equals_the_dense_entry_point(K):
    A, Bm, Pi, ob = structured_model(K, 900 + K)
    assert np.count_nonzero(A[:, 3]) == K and not A[:, 5].any() and np.count_nonzero(A[12]) == 1
    compare_entry_points(A, Bm, Pi, ob, splits=(1, 2, 5), expect_rc=0)


def dead_end_model():
    """Symbol 1 can only be emitted by state 2, which no state reaches and Pi excludes: a sequence holding symbol 1 after
    time 0 has entries without a finite predecessor (FV_ERR_NO_PRED, -1 entries in the path)."""
    K = 40
    rs = np.random.RandomState(4)
    A = rs.uniform(0.1, 1.0, (K, K)) * (rs.uniform(0, 1, (K, K)) < 0.2)
    A[np.arange(K), (np.arange(K) + 1) % K] = 0.5
    A[:, 2] = 0.0
    A /= A.sum(axis=1)[:, None]
    Bm = np.zeros((K, 2))
    Bm[:, 0] = 1.0
    Bm[2] = (0.5, 0.5)
    Pi = np.full(K, 1.0 / (K - 1))
    Pi[2] = 0.0
    q = modelgen.hostio.quantize_text16
    return q(A), q(Bm), q(Pi)


def test_no_predecessor_sequence_equals_the_dense_entry_point():
    A, Bm, Pi = dead_end_model()
    bad = np.array([0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0], np.int32)
    out = compare_entry_points(A, Bm, Pi, bad, splits=(1, 2), expect_rc=D.ERR_NO_PRED)
    assert all((p < 0).any() for _, p in out)
    compare_entry_points(A, Bm, Pi, np.zeros(16, np.int32), splits=(1, 2), expect_rc=0)


# ---------------------------------------------------------------- 5. batch, partition, group

def test_batch_equals_single_decodes():
    A, Bm, Pi, ob = modelgen.model32(dict(kind="sparse_fast", K=500, M=7, T=300, prob=0.04, seed=31))
    rs = np.random.RandomState(32)
    seqs = [ob[:200], ob[50:57], ob[100:300], ob[:2], ob[7:140], ob[3:90], ob[:64], ob[200:231], ob[1:100]]
    fv = sparse_ctx(A, Bm, Pi)
    try:
        for mode in (D.MODE_REFERENCE, D.MODE_SINGLE_PASS):
            for N in (1, 4):
                fv.set_option(D.OPT_DEBUG, 0)
                fv.set_option(D.OPT_MAX_BATCH, 8)
                want = [fv.decode_full(o, N, mode) for o in seqs]
                for batch in (1, 3, 8):
                    for dbg in (0, MEM, 1 << 28, MEM | (1 << 28)):
                        fv.set_option(D.OPT_MAX_BATCH, batch)
                        fv.set_option(D.OPT_DEBUG, dbg)
                        paths, scores, statuses = fv.decode_full_batch(seqs, N, mode)
                        where = f"mode={mode} N={N} batch={batch} debug={dbg}"
                        assert not statuses.any() and fv.stats()["kernel"] == 7, where
                        for s, (p, sc, _) in enumerate(want):
                            assert paths[s].tolist() == p.tolist() and scores[s] == sc, f"{where} sequence {s}"
    finally:
        fv.close()
    del rs


def test_batch_with_one_no_predecessor_sequence():
    A, Bm, Pi = dead_end_model()
    good = np.zeros(20, np.int32)
    bad = good.copy()
    bad[9] = 1
    fv = sparse_ctx(A, Bm, Pi)
    de = dense_ctx(A, Bm, Pi)
    try:
        for dbg in (0, MEM):
            fv.set_option(D.OPT_DEBUG, dbg)
            paths, scores, statuses = fv.decode_full_batch([good, bad, good[:11]], 2)
            dpaths, dscores, dstatuses = de.decode_full_batch([good, bad, good[:11]], 2)
            assert statuses.tolist() == [0, D.ERR_NO_PRED, 0] == dstatuses.tolist()
            assert (paths[1] < 0).any()
            for s in range(3):
                assert paths[s].tolist() == dpaths[s].tolist() and scores[s].view(np.uint32) == dscores[s].view(np.uint32)
            p, sc, rc = fv.decode_full(good, 2)
            assert rc == 0 and p.tolist() == paths[0].tolist() and sc == scores[0]
    finally:
        fv.close()
        de.close()


def test_partition_of_three_ranks_merges_to_the_one_rank_path():
    A, Bm, Pi, ob = modelgen.model32(dict(kind="sparse_fast", K=400, M=6, T=96, prob=0.05, seed=41))
    N, nranks = 6, 3
    fv = sparse_ctx(A, Bm, Pi)
    try:
        whole, score, rc = fv.decode_full(ob, N)
        assert rc == 0
        gathered = []
        for rank in range(nranks):
            fv.set_partition(rank, nranks)
            p, sc, rc = fv.decode_full(ob, N)
            assert rc == 0 and sc == score
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
    plain = sparse_ctx(A, Bm, Pi)
    group = sparse_ctx(A, Bm, Pi, device=[0, 0])
    try:
        for N in (1, 4, 8):
            a, b = plain.decode_full(ob, N), group.decode_full(ob, N)
            assert a[2] == b[2] == 0 and a[0].tolist() == b[0].tolist() and a[1] == b[1]
        assert group.stats()["kernel"] == 7 and group.stats()["ranks"] == 2
        # the other way round on the group: dense, then sparse again
        group.set_model(A, Bm, Pi)
        assert group.decode_full(ob, 4)[0].tolist() == plain.decode_full(ob, 4)[0].tolist()
        assert group.stats()["kernel"] != 7
        group.set_model_sparse(*decoder.dense_to_csr(A), Bm, Pi)
        assert group.decode_full(ob, 4)[0].tolist() == plain.decode_full(ob, 4)[0].tolist()
    finally:
        plain.close()
        group.close()


# ---------------------------------------------------------------- 6. beyond one LDS score row

def test_beyond_one_lds_score_row_equals_oracle_and_dense():
    """K = 45000: a float32 score row (180 KB) does not fit LDS, so every launch reads its rows from memory."""
    K, T, N = 45000, 7, 2
    t0 = time.time()
    A, Bm, Pi, ob = modelgen.model32(dict(kind="sparse_fast", K=K, M=8, T=T, prob=40.0 / K, seed=61))
    csr = decoder.dense_to_csr(A)
    _log(f"K={K} model and CSR built in {time.time() - t0:.1f}s, nnz {csr[0][-1]}")
    sp = decoder.FlashViterbi(0)
    try:
        sp.set_model_sparse(*csr, Bm, Pi)
        spath, sscore, src = sp.decode_full(ob, N)
        st = sp.stats()
        assert st["kernel"] == 7
        _log(f"K={K} sparse-set: device_bytes {st['device_bytes']} set_model_ms {st['set_model_ms']:.1f} gpu_ms {st['gpu_ms']:.2f}")
        rows, bp, var = sp.test_forward(ob, [(0, 3, -1), (4, 6, 17)])
        assert var == TV_MEM[0] | TV_MEM[1]         # launches of two tasks and of one, rows in memory; no LDS form
    finally:
        sp.close()
    de = decoder.FlashViterbi(0)
    try:
        de.set_model(A, Bm, Pi)
        dpath, dscore, drc = de.decode_full(ob, N)
    finally:
        de.close()
    om = oracle.OracleModel(A, Bm, Pi)
    opath, oscore, _, orc = om.full_decode(ob, N)
    want = [om.full_forward(ob, 0, 3, -1), om.full_forward(ob, 4, 6, 17)]
    om.close()
    assert src == drc == orc == 0
    assert spath.tolist() == opath.tolist() == dpath.tolist() and sscore == oscore == dscore
    for q, (row, args) in enumerate(want):
        assert np.array_equal(rows[q].view(np.uint32), row.view(np.uint32))
    assert np.array_equal(bp[1:4], want[0][1]) and np.array_equal(bp[5:7], want[1][1])


# ---------------------------------------------------------------- 7. beyond what fv_set_model can take

NBLOCKS, BLOCK_K, BLOCK_M, BLOCK_T, BLOCK_SEED = 64, 4096, 6, 12, 2024


def interleaved_blocks(nblocks, Kb, M, seed, degree=32):
    """nblocks independent sparse models of Kb states; state s of block b is global state s * nblocks + b.  Returns the
    global CSR model and the blocks' dense models."""
    blocks = [data_script.make_model_csr(Kb, M, seed + b, degree) for b in range(nblocks)]
    K = nblocks * Kb
    deg = np.zeros(K, dtype=np.int64)
    for b, (ip, _, _, _, _) in enumerate(blocks):
        deg[b::nblocks] = np.diff(ip)
    indptr = np.zeros(K + 1, dtype=np.int64)
    np.cumsum(deg, out=indptr[1:])
    indices = np.empty(indptr[-1], dtype=np.int32)
    data = np.empty(indptr[-1], dtype=np.float32)
    Bm = np.empty((K, M), dtype=np.float32)
    Pi = np.empty(K, dtype=np.float32)
    for b, (ip, ix, dt, Bb, Pib) in enumerate(blocks):
        row = np.repeat(np.arange(Kb, dtype=np.int64), np.diff(ip))
        dest = indptr[row * nblocks + b] + (np.arange(ix.size, dtype=np.int64) - ip[row])
        indices[dest] = ix.astype(np.int64) * nblocks + b
        data[dest] = dt
        Bm[b::nblocks] = Bb
        Pi[b::nblocks] = Pib
    return (indptr, indices, data, Bm, Pi), blocks


def test_interleaved_blocks_helper_on_a_small_case():
    """The construction itself, where the dense oracle of the whole model is affordable: 5 blocks of 60 states."""
    (ip, ix, dt, Bm, Pi), blocks = interleaved_blocks(5, 60, 4, 9, degree=6)
    K = 300
    A = csr_to_dense(ip, ix, dt, K)
    ob = np.random.RandomState(1).randint(0, 4, 20).astype(np.int32)
    om = oracle.OracleModel(A, Bm, Pi)
    wpath, wscore, _, wrc = om.full_decode(ob, 3)
    om.close()
    best = None
    for b, (bip, bix, bdt, Bb, Pib) in enumerate(blocks):
        ob_m = oracle.OracleModel(csr_to_dense(bip, bix, bdt, 60), Bb, Pib)
        p, s, _, rc = ob_m.full_decode(ob, 3)
        ob_m.close()
        if best is None or s > best[1]:
            best = (p * 5 + b, s, rc)
    assert wrc == best[2] == 0 and wpath.tolist() == best[0].tolist() and wscore == best[1]
    fv = decoder.FlashViterbi(0)
    try:
        fv.set_model_sparse(ip, ix, dt, Bm, Pi)
        path, score, rc = fv.decode_full(ob, 3)
        assert rc == 0 and path.tolist() == wpath.tolist() and score == wscore
    finally:
        fv.close()


def test_quarter_million_states_equal_the_best_block_of_the_oracle():
    """K = 262144 = 64 blocks of 4096 states with about 32 in-edges per state: 8 * K * K would be 550 GB.  The blocks
    never exchange score, so the decode of the whole model is the decode of the block with the largest whole-sequence
    score (asserted unique), mapped through s * 64 + b."""
    K = NBLOCKS * BLOCK_K
    t0 = time.time()
    (ip, ix, dt, Bm, Pi), blocks = interleaved_blocks(NBLOCKS, BLOCK_K, BLOCK_M, BLOCK_SEED)
    ob = np.random.RandomState(BLOCK_SEED).randint(0, BLOCK_M, BLOCK_T).astype(np.int32)
    _log(f"K={K}: {ip[-1]} stored transitions built in {time.time() - t0:.1f}s")
    fv = decoder.FlashViterbi(0)
    got = {}
    try:
        fv.set_model_sparse(ip, ix, dt, Bm, Pi)
        for N in (3, 1):
            got[N] = fv.decode_full(ob, N)
            st = fv.stats()
            assert st["kernel"] == 7
            assert st["device_bytes"] < 8 * K * K / 100
            _log(f"K={K} N={N}: device_bytes {st['device_bytes']} set_model_ms {st['set_model_ms']:.1f} gpu_ms {st['gpu_ms']:.2f} "
                 f"table_bytes_per_step {st['table_bytes_per_step']}")
            got[N, "batch"] = fv.decode_full_batch([ob, ob], N)
            _log(f"K={K} N={N} batch of 2: gpu_ms {fv.stats()['gpu_ms']:.2f}")
    finally:
        fv.close()
    t0 = time.time()
    want = {3: [], 1: []}
    for b, (bip, bix, bdt, Bb, Pib) in enumerate(blocks):
        om = oracle.OracleModel(csr_to_dense(bip, bix, bdt, BLOCK_K), Bb, Pib)
        for N in (3, 1):
            want[N].append(om.full_decode(ob, N))
        om.close()
    _log(f"oracle over {NBLOCKS} blocks: {time.time() - t0:.1f}s")
    for N in (3, 1):
        scores = np.array([r[1] for r in want[N]])
        b = int(np.argmax(scores))
        assert (scores == scores[b]).sum() == 1, "the best block's score must be unique (a condition on the input)"
        assert all(r[3] == 0 for r in want[N])
        wpath = want[N][b][0].astype(np.int64) * NBLOCKS + b
        path, score, rc = got[N]
        assert rc == 0 and path.tolist() == wpath.tolist() and score == scores[b], f"N={N}"
        paths, bscores, statuses = got[N, "batch"]
        for s in (0, 1):
            assert statuses[s] == 0 and paths[s].tolist() == wpath.tolist() and bscores[s] == scores[b], f"N={N} batch {s}"


# ---------------------------------------------------------------- 8. refusals

def test_malformed_csr_is_refused_and_the_previous_model_still_decodes():
    A, Bm, Pi, ob = modelgen.model32(dict(kind="sparse_fast", K=120, M=5, T=30, prob=0.1, seed=71))
    ip, ix, dt = decoder.dense_to_csr(A)
    om = oracle.OracleModel(A, Bm, Pi)
    want = om.full_decode(ob, 2)
    om.close()
    row = 50
    lo, hi = int(ip[row]), int(ip[row + 1])
    assert hi - lo >= 3

    def mutate(what):
        p, x, d = ip.copy(), ix.copy(), dt.copy()
        if what == "first pointer":
            p[0] = 1
        elif what == "decreasing pointer":
            p[row + 1] = p[row] - 1
        elif what == "column out of range":
            x[hi - 1] = 120
        elif what == "negative column":
            x[lo] = -1
        elif what == "unsorted":
            x[lo], x[lo + 1] = x[lo + 1], x[lo]
        elif what == "duplicate":
            x[lo + 1] = x[lo]
        elif what == "negative value":
            d[lo + 1] = -0.25
        elif what == "nan":
            d[lo + 1] = np.nan
        elif what == "inf":
            d[lo + 1] = np.inf
        return p, x, d

    for start in ("sparse", "dense"):
        fv = decoder.FlashViterbi(0)
        try:
            if start == "sparse":
                fv.set_model_sparse(ip, ix, dt, Bm, Pi)
            else:
                fv.set_model(A, Bm, Pi)
            for what in ("first pointer", "decreasing pointer", "column out of range", "negative column", "unsorted", "duplicate",
                         "negative value", "nan", "inf"):
                with pytest.raises(decoder.FlashVitError) as e:
                    fv.set_model_sparse(*mutate(what), Bm, Pi)
                assert e.value.rc == D.ERR_ARG, what
                assert f"row {0 if what == 'first pointer' else row}" in str(e.value), (what, str(e.value))
                path, score, rc = fv.decode_full(ob, 2)
                assert rc == 0 and path.tolist() == want[0].tolist() and score == want[1], what
                assert (fv.stats()["kernel"] == 7) == (start == "sparse")
            for badB, badPi in ((Bm * -1, Pi), (Bm, np.full_like(Pi, np.nan))):
                with pytest.raises(decoder.FlashVitError) as e:
                    fv.set_model_sparse(ip, ix, dt, badB, badPi)
                assert e.value.rc == D.ERR_ARG
            assert fv.decode_full(ob, 2)[0].tolist() == want[0].tolist()
        finally:
            fv.close()


def test_entries_above_one_are_accepted_and_refused_at_decode():
    """The walk is a filter kernel (its error bracket needs every log <= 0) and a sparse-set model has no float64 table:
    fv_set_model_sparse takes the model as fv_set_model does, the decode answers FV_ERR_UNSUPPORTED."""
    A, Bm, Pi, ob = modelgen.model32(dict(kind="sparse_fast", K=64, M=4, T=20, prob=0.2, seed=72))
    ip, ix, dt = decoder.dense_to_csr(A)
    dt = dt.copy()
    dt[3] = 1.5
    fv = decoder.FlashViterbi(0)
    try:
        fv.set_model_sparse(ip, ix, dt, Bm, Pi)
        with pytest.raises(decoder.FlashVitError) as e:
            fv.decode_full(ob, 2)
        assert e.value.rc == D.ERR_UNSUPPORTED and "[0,1]" in str(e.value)
        with pytest.raises(decoder.FlashVitError) as e:
            fv.decode_full_batch([ob, ob], 2)
        assert e.value.rc == D.ERR_UNSUPPORTED
        fv.set_model_sparse(*decoder.dense_to_csr(A), Bm, Pi)
        assert fv.decode_full(ob, 2)[2] == 0
    finally:
        fv.close()


@pytest.mark.parametrize("name", ["cfg1_K128_T256", "ties_semi_K96_T80"])
def test_out_of_scope_calls_are_refused_until_a_dense_model_is_set(name):
    from conftest import load_goldens
    g = [x for x in load_goldens(True) if x["name"] == name][0]
    A, Bm, Pi, ob = golden_model(g)
    runs = {}
    for r in g["runs"]:
        runs.setdefault(r["algo"], r)
    fv = sparse_ctx(A, Bm, Pi)
    try:
        beamB = runs["flashbs"]["B"]
        calls = {"beam": lambda: fv.decode_beam(ob, 4, beamB), "beam batch": lambda: fv.decode_beam_batch([ob, ob], 4, beamB),
                 "vanilla": lambda: fv.decode_vanilla(ob), "checkpoint": lambda: fv.decode_checkpoint(ob)}
        for what, call in calls.items():
            with pytest.raises(decoder.FlashVitError) as e:
                call()
            assert e.value.rc == D.ERR_UNSUPPORTED and "fv_set_model_sparse" in str(e.value), what
        for kernel in (D.KERNEL_F64_STREAM, D.KERNEL_F32_REFINE, D.KERNEL_F16_REFINE, D.KERNEL_Q16_REFINE, D.KERNEL_U16_REFINE):
            fv.set_option(D.OPT_KERNEL, kernel)
            with pytest.raises(decoder.FlashVitError) as e:
                fv.decode_full(ob, 4)
            assert e.value.rc == D.ERR_UNSUPPORTED and "fv_set_model_sparse" in str(e.value), kernel
        with pytest.raises(decoder.FlashVitError) as e:
            fv.set_option(D.OPT_KERNEL, 7)                    # reported, never chosen
        assert e.value.rc == D.ERR_ARG
        for bad in (1 << 27, 1 << 30, MEM | (1 << 30), 1 << 32):
            with pytest.raises(decoder.FlashVitError) as e:
                fv.set_option(D.OPT_DEBUG, bad)
            assert e.value.rc == D.ERR_ARG
        flash = runs["flash"]
        for kernel in (D.KERNEL_SPARSE_Q16, D.KERNEL_AUTO):
            fv.set_option(D.OPT_KERNEL, kernel)
            path, score, rc = fv.decode_full(ob, flash["N"])
            assert rc == 0 and path.tolist() == flash["path"] and fv.stats()["kernel"] == 7
        # a dense model on the same context: everything works again and matches its golden
        fv.set_model(A, Bm, Pi)
        path, score, rc = fv.decode_full(ob, flash["N"])
        assert rc == 0 and path.tolist() == flash["path"] and score == np.float32(flash["score"]) and fv.stats()["kernel"] != 7
        for r in g["runs"]:
            if r["algo"] == "flashbs":
                path, score, rc = fv.decode_beam(ob, r["N"], r["B"])
                assert path.tolist() == r["path"], r
                paths, _, _ = fv.decode_beam_batch([ob, ob], r["N"], r["B"])
                assert paths[0].tolist() == r["path"] == paths[1].tolist()
            elif r["algo"] == "vanilla":
                assert fv.decode_vanilla(ob)[0].tolist() == r["path"]
            elif r["algo"] == "checkpoint":
                assert fv.decode_checkpoint(ob, r.get("step", 0))[0].tolist() == r["path"]
        fv.set_option(D.OPT_KERNEL, D.KERNEL_F64_STREAM)
        assert fv.decode_full(ob, flash["N"])[0].tolist() == flash["path"]
        # and back
        fv.set_model_sparse(*decoder.dense_to_csr(A), Bm, Pi)
        with pytest.raises(decoder.FlashVitError):
            fv.decode_vanilla(ob)
        fv.set_option(D.OPT_KERNEL, D.KERNEL_AUTO)
        assert fv.decode_full(ob, flash["N"])[0].tolist() == flash["path"]
    finally:
        fv.close()
