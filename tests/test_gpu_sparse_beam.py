"""GPU: FV_OPT_SPARSE_BEAM — the FLASH-BS calls on a model set through fv_set_model_sparse.  Every comparison is an
equality: per sequence the path (with its -1 entries), the float32 score's bits and the return / status code are those of
the same model set through fv_set_model — the goldens, fresh models with both contexts alive, beams wider than the reach,
values outside [0, 1], whole step tables through fv_test_beam_step, the batch call, a K beyond the dense path's selects,
and the switch itself.  Every test fails on a library without the option (key 7: FV_ERR_ARG)."""
import math

import numpy as np
import pytest

import modelgen
from conftest import golden_model, golden_runs
from flash_viterbi_amd import decoder

pytestmark = pytest.mark.gpu

D = decoder
EAGER, ALL_LAYOUTS, NOCUT, MANY, NOLISTS = 1 << 20, 1 << 19, 1 << 23, 1 << 22, 1 << 10
DEBUGS = (0, EAGER, ALL_LAYOUTS, NOCUT, MANY, NOLISTS)
PAIRS, IDS = golden_runs(include_big=True, algo="flashbs")
FLT_MAX = np.finfo(np.float32).max


def sparse_ctx(csr, B, Pi, option=1):
    fv = decoder.FlashViterbi(0)
    fv.set_model_sparse(*csr, B, Pi)
    if option is not None:
        fv.set_option(D.OPT_SPARSE_BEAM, option)
    return fv


def dense_ctx(A, B, Pi):
    fv = decoder.FlashViterbi(0)
    fv.set_model(A, B, Pi)
    return fv


def csr_to_dense(indptr, indices, data, K):
    A = np.zeros((K, K), dtype=np.float32)
    A[np.repeat(np.arange(K), np.diff(indptr)), indices] = data
    return A


def bits(x):
    return int(np.float32(x).view(np.uint32))


def same(a, b):
    return a[2] == b[2] and a[0].tolist() == b[0].tolist() and bits(a[1]) == bits(b[1])


def refused(call, rc, text=None):
    with pytest.raises(decoder.FlashVitError) as e:
        call()
    assert e.value.rc == rc, str(e.value)
    if text is not None:
        assert text in str(e.value), str(e.value)


def outcome(call):
    """("refused", rc) or ("ok", paths, score bits, codes) of a decode call, for comparing two contexts."""
    try:
        p, s, rc = call()
    except decoder.FlashVitError as e:
        return ("refused", e.rc)
    if isinstance(p, list):
        return ("ok", [x.tolist() for x in p], [bits(x) for x in s], [int(x) for x in rc])
    return ("ok", p.tolist(), bits(s), int(rc))


def side_by_side(de, sp, ob, N, B, modes=(D.MODE_REFERENCE, D.MODE_SINGLE_PASS), debugs=(0,), T=None, ties=True):
    """The same decode on the dense-set and on the sparse-set context; returns the dense results."""
    out = []
    for mode in modes:
        for dbg in debugs:
            where = f"N={N} B={B} mode={mode} debug={dbg}"
            de.set_option(D.OPT_DEBUG, dbg)
            sp.set_option(D.OPT_DEBUG, dbg)
            try:
                want = de.decode_beam(ob, N, B, mode, T=T)
                want_ties = de.stats()["beam_ties"]
                got = sp.decode_beam(ob, N, B, mode, T=T)
                st = sp.stats()
            finally:
                de.set_option(D.OPT_DEBUG, 0)
                sp.set_option(D.OPT_DEBUG, 0)
            assert same(got, want), f"{where}: sparse {got[2]} {bits(got[1]):#x} dense {want[2]} {bits(want[1]):#x}, first differing time " \
                                    f"{np.nonzero(got[0] != want[0])[0][:1].tolist()}"
            assert st["kernel"] == D.KERNEL_CSR_F64, where
            if ties:
                assert st["beam_ties"] == want_ties, where
            out.append(want)
    return out


# ---------------------------------------------------------------- 1. goldens

@pytest.fixture(scope="module")
def ctxs():
    cache = {}

    def get(g):
        if g["name"] not in cache:
            A, B, Pi, ob = golden_model(g)
            cache[g["name"]] = (sparse_ctx(decoder.dense_to_csr(A), B, Pi), ob)
        return cache[g["name"]]
    yield get
    for sp, _ in cache.values():
        sp.close()


@pytest.mark.parametrize("g,r", PAIRS, ids=IDS)
def test_goldens_on_the_sparse_set_model(ctxs, g, r):
    sp, ob = ctxs(g)
    for dbg in DEBUGS:
        sp.set_option(D.OPT_DEBUG, dbg)
        try:
            path, score, rc = sp.decode_beam(ob, r["N"], r["B"], D.MODE_REFERENCE)
        finally:
            sp.set_option(D.OPT_DEBUG, 0)
        assert path.tolist() == r["path"], dbg
        assert score == np.float32(r["score"]), dbg
        assert rc == (D.WARN_BEAM_MISS if -1 in r["path"] else 0), dbg
        assert sp.stats()["kernel"] == D.KERNEL_CSR_F64


# ---------------------------------------------------------------- 2. fresh models, both contexts alive

FRESH = [("data_script", 300, 70, 4, 20), ("data_script", 1000, 40, 3, 128), ("ties_semi", 1200, 40, 4, 50),
         ("ties_all", 600, 30, 3, 33), ("ties_semi", 7000, 24, 3, 64)]


@pytest.mark.parametrize("kind,K,T,N,B", FRESH, ids=[f"{c[0]}-K{c[1]}-B{c[4]}" for c in FRESH])
def test_dense_set_against_sparse_set(kind, K, T, N, B):
    A, Bm, Pi, ob = modelgen.model32(dict(kind=kind, K=K, M=8, T=T, prob=0.1 if K <= 1000 else 0.05, seed=500 + K))
    de, sp = dense_ctx(A, Bm, Pi), sparse_ctx(decoder.dense_to_csr(A), Bm, Pi)
    try:
        side_by_side(de, sp, ob, N, B)
    finally:
        de.close()
        sp.close()


# ---------------------------------------------------------------- 3. reach smaller than the beam

def thin_model(seed):
    """About three out-edges per state: a beam of 128 reaches fewer than 128 columns after a few steps."""
    return modelgen.model32(dict(kind="sparse_fast", K=300, M=8, T=40, prob=0.01, seed=seed))


def holes_model(seed, dead):
    """CSR with a state that has no out-edges (an empty row), a row made of stored zeros only, and explicit stored zeros
    inside other rows.  dead: symbol 7 is emitted by the state without out-edges alone and observed once, at time 20 — every
    score after it is -FLT_MAX, the heaps hold -FLT_MAX members and the path -1 entries.  Returns (csr, dense A, B, Pi, ob)."""
    K, T = 300, 40
    A, Bm, Pi, ob = modelgen.model32(dict(kind="sparse_fast", K=K, M=8, T=T, prob=0.01, seed=seed))
    A, Bm, ob = A.copy(), Bm.copy(), np.where(ob == 7, 6, ob).astype(np.int32)
    A[1::3, 5] = np.float32(0.2)                                   # the state without out-edges is easy to reach
    Bm[np.arange(K) != 5, 7] = 0.0
    if dead:
        ob[20] = 7
    indptr, indices, data = decoder.dense_to_csr(A)
    rs = np.random.RandomState(seed)
    rows = []
    for k in range(K):
        cols, vals = indices[indptr[k]:indptr[k + 1]].tolist(), data[indptr[k]:indptr[k + 1]].tolist()
        if k == 5:
            cols, vals = [], []                                    # no out-edges
        elif k == 9:
            vals = [0.0] * len(vals)                               # stored zeros only
        elif k % 3 == 0:
            extra = [c for c in rs.choice(K, 3, replace=False).tolist() if c not in cols]
            cols, vals = cols + extra, vals + [0.0] * len(extra)  # stored zeros among real entries
        order = np.argsort(cols)
        rows.append((np.asarray(cols, np.int32)[order], np.asarray(vals, np.float32)[order]))
    ip = np.zeros(K + 1, dtype=np.int64)
    np.cumsum([r[0].size for r in rows], out=ip[1:])
    ix = np.concatenate([r[0] for r in rows]).astype(np.int32)
    dt = np.concatenate([r[1] for r in rows]).astype(np.float32)
    assert (dt == 0).sum() > 50 and ip[6] == ip[5]
    return (ip, ix, dt), csr_to_dense(ip, ix, dt, K), Bm, Pi, ob


# Checked on the CPU with the oracle (oracle.OracleModel.beam_decode, N = 4, B = 128) before these were kept: the thin
# models decode without a miss (twelve seeds tried, none missed: a right-hand pass that reaches fewer than B columns keeps
# every reached state), the holes model with the dead symbol decodes with -1 entries and WARN_BEAM_MISS, without it clean.
THIN_SEEDS = ((2008, False), (2010, False))
HOLES_SEEDS = ((2003, True), (2003, False))


@pytest.mark.parametrize("seed,miss", THIN_SEEDS)
def test_reach_smaller_than_the_beam(seed, miss):
    A, Bm, Pi, ob = thin_model(seed)
    de, sp = dense_ctx(A, Bm, Pi), sparse_ctx(decoder.dense_to_csr(A), Bm, Pi)
    try:
        for want in side_by_side(de, sp, ob, 4, 128, modes=(D.MODE_REFERENCE,), debugs=(0, EAGER)):
            assert (want[2] == D.WARN_BEAM_MISS) == miss and ((want[0] < 0).any() == miss)
        side_by_side(de, sp, ob, 1, 128, modes=(D.MODE_SINGLE_PASS,))
    finally:
        de.close()
        sp.close()


@pytest.mark.parametrize("seed,miss", HOLES_SEEDS)
def test_empty_rows_and_stored_zeros(seed, miss):
    csr, A, Bm, Pi, ob = holes_model(seed, miss)
    de, sp = dense_ctx(A, Bm, Pi), sparse_ctx(csr, Bm, Pi)
    try:
        for want in side_by_side(de, sp, ob, 4, 128, modes=(D.MODE_REFERENCE,), debugs=(0, EAGER)):
            assert (want[2] == D.WARN_BEAM_MISS) == miss and ((want[0] < 0).any() == miss)
        side_by_side(de, sp, ob, 1, 128, modes=(D.MODE_SINGLE_PASS,))
    finally:
        de.close()
        sp.close()


# ---------------------------------------------------------------- 4. values outside [0, 1]

def above_one(x, frac, seed):
    """A copy of x with about `frac` of its non-zero entries replaced by values in (1, 50]."""
    rs = np.random.RandomState(seed)
    x = np.array(x, dtype=np.float32, copy=True)
    flat = x.reshape(-1)
    nz = np.nonzero(flat)[0]
    pick = nz[rs.uniform(size=nz.size) < frac]
    flat[pick] = np.maximum(rs.uniform(1.0, 50.0, pick.size).astype(np.float32), np.nextafter(np.float32(1), np.float32(2)))
    assert pick.size and (flat[pick] > 1).all() and (x <= 50).all()
    return x


def test_model_entries_above_one():
    A, Bm, Pi, ob = modelgen.model32(dict(kind="sparse_fast", K=1000, M=8, T=40, prob=0.05, seed=611))
    A = above_one(A, 0.05, 612)
    de, sp = dense_ctx(A, Bm, Pi), sparse_ctx(decoder.dense_to_csr(A), Bm, Pi)
    try:
        side_by_side(de, sp, ob, 3, 100, debugs=(0, EAGER))
    finally:
        de.close()
        sp.close()


def test_staged_emission_scores_above_zero():
    K, T = 1000, 40
    A, Bm, Pi, _ = modelgen.model32(dict(kind="sparse_fast", K=K, M=8, T=T, prob=0.05, seed=621))
    rs = np.random.RandomState(622)
    E = rs.uniform(-6.0, 0.0, (T, K)).astype(np.float32)
    hot = rs.uniform(size=E.shape) < 0.03
    E[hot] = rs.uniform(0.0, 3.0, int(hot.sum())).astype(np.float32)
    assert (E > 0).any()
    de, sp = dense_ctx(A, Bm, Pi), sparse_ctx(decoder.dense_to_csr(A), Bm, Pi)
    try:
        de.set_emissions(E)
        sp.set_emissions(E)
        side_by_side(de, sp, None, 3, 100, debugs=(0, EAGER), T=T)
    finally:
        de.close()
        sp.close()


# ---------------------------------------------------------------- 5. step tables through fv_test_beam_step

@pytest.fixture(scope="module")
def step_models():
    made = {}

    def get(K):
        if K not in made:
            if K == 500:
                A, Bm, Pi, _ = modelgen.model32(dict(kind="ties_semi", K=K, M=8, T=4, prob=0.5, seed=700))
            else:
                A, Bm, Pi, _ = modelgen.model32(dict(kind="sparse_fast", K=K, M=8, T=4, prob=0.02, seed=701))
            made[K] = (dense_ctx(A, Bm, Pi), sparse_ctx(decoder.dense_to_csr(A), Bm, Pi))
        return made[K]
    yield get
    for de, sp in made.values():
        de.close()
        sp.close()


def slot_sets(rs, K, B, extra, nsets):
    """nsets slot sets of B + extra entries with many equal values; with extra > 0 the last 1 + extra (shuffled in) equal theta."""
    theta = np.float32(-6.0)
    sets = []
    for _ in range(nsets):
        n = B + extra
        vals = rs.choice(np.array([-3.0, -3.5, -4.0, -4.25], np.float32), n).astype(np.float32)
        if extra:
            vals[B - 1:] = theta
        order = rs.permutation(n)
        sets.append((vals[order], rs.choice(K, n, replace=False).astype(np.int32)[order]))
    return sets, float(theta)


@pytest.mark.parametrize("K", [500, 4100])
@pytest.mark.parametrize("B", [16, 64, 300])
def test_step_tables_equal_the_dense_kernels(step_models, K, B):
    de, sp = step_models(K)
    rs = np.random.RandomState(K + B)
    syms = [0, 3, 7]
    for spec in (False, True):
        sets, theta = slot_sets(rs, K, B, 5 if spec else 0, 3)
        cap = 2 * B + 7
        probe = de.test_beam_step(B, sets, syms, spec, theta)
        fin = np.sort(probe["scores"][0][probe["scores"][0] > -FLT_MAX])
        assert fin.size > 4
        bound = float(fin[-min(fin.size, B + B // 2)])
        want = de.test_beam_step(B, sets, syms, spec, theta, bound, cap)
        got = sp.test_beam_step(B, sets, syms, spec, theta, bound, cap)
        where = f"K={K} B={B} speculative={spec}"
        assert got["variants"] == D.TV_BEAM_CSR and want["variants"] != D.TV_BEAM_CSR, where
        assert np.array_equal(got["scores"].view(np.uint32), want["scores"].view(np.uint32)), where
        assert np.array_equal(got["bp"], want["bp"]), where
        assert got["ties"] == want["ties"], where
        for q in range(3):
            (gc, gl), (wc, wl) = got["doubt"][q], want["doubt"][q]
            assert gc == wc and (gc > 1024 or (len(gl) == gc and set(gl) == set(wl))), f"{where} set {q}: doubtful columns"
            assert spec or gc == 0
            (gc, gl), (wc, wl) = got["cand"][q], want["cand"][q]
            assert gc == wc and (gc > cap or {(bits(v), c) for v, c in gl} == {(bits(v), c) for v, c in wl}), f"{where} set {q}: candidates"
        if K == 500:
            assert want["ties"], where                     # dyadic weights and four slot values: tied cells exist
        if spec:
            assert any(c for c, _ in want["doubt"]), where


# ---------------------------------------------------------------- 6. batch

def test_batch_equals_single_decodes_and_the_dense_batch():
    K, B, N = 1200, 50, 3
    A, Bm, Pi, _ = modelgen.model32(dict(kind="ties_semi", K=K, M=8, T=4, prob=0.5, seed=801))
    rs = np.random.RandomState(802)
    obs = [rs.randint(0, 8, n).astype(np.int32) for n in (2, 7, 23, 41, 70)]
    de, sp = dense_ctx(A, Bm, Pi), sparse_ctx(decoder.dense_to_csr(A), Bm, Pi)
    try:
        for mode in (D.MODE_REFERENCE, D.MODE_SINGLE_PASS):
            wp, ws, wst = de.decode_beam_batch(obs, N, B, mode)
            gp, gs, gst = sp.decode_beam_batch(obs, N, B, mode)
            assert sp.stats()["kernel"] == D.KERNEL_CSR_F64
            for s, ob in enumerate(obs):
                where = f"mode={mode} sequence {s}"
                assert gp[s].tolist() == wp[s].tolist() and bits(gs[s]) == bits(ws[s]) and gst[s] == wst[s], where
                one = sp.decode_beam(ob, N, B, mode)
                assert one[0].tolist() == gp[s].tolist() and bits(one[1]) == bits(gs[s]) and one[2] == gst[s], where
    finally:
        de.close()
        sp.close()


# ---------------------------------------------------------------- 7. beyond the dense path

def banded_csr(K, M, seed):
    """About 16 out-edges per state, built directly as CSR: a band of eight successors and eight random columns."""
    rs = np.random.RandomState(seed)
    band = (np.arange(K, dtype=np.int64)[:, None] + np.arange(1, 9)[None, :]) % K
    cols = np.sort(np.concatenate([band, rs.randint(0, K, (K, 8))], axis=1), axis=1)
    keep = np.ones(cols.shape, dtype=bool)
    keep[:, 1:] = cols[:, 1:] != cols[:, :-1]
    w = rs.uniform(0.01, 1.0, cols.shape) * keep
    w /= w.sum(axis=1)[:, None]
    indptr = np.zeros(K + 1, dtype=np.int64)
    np.cumsum(keep.sum(axis=1), out=indptr[1:])
    Bm = rs.uniform(0.1, 1.0, (K, M))
    Bm /= Bm.sum(axis=1)[:, None]
    return (indptr, cols[keep].astype(np.int32), w[keep].astype(np.float32)), Bm.astype(np.float32), np.full(K, 1.0 / K, np.float32)


def test_k_beyond_the_dense_beam_path():
    K, M, T, B = 70000, 4, 24, 256
    csr, Bm, Pi = banded_csr(K, M, 900)
    indptr, indices, data = csr
    assert 14 * K < indptr[-1] <= 16 * K and (data > 0).all()
    ob = np.random.RandomState(901).randint(0, M, T).astype(np.int32)
    sp = sparse_ctx(csr, Bm, Pi)
    try:
        path, score, rc = sp.decode_beam(ob, 1, B, D.MODE_SINGLE_PASS)
        assert rc == 0 and (path >= 0).all()
        logB = lambda i, o: math.log(float(Bm[i, o]))
        val = np.float32(math.log(float(Pi[path[0]])) + logB(path[0], ob[0]))
        for j in range(1, T):
            a, b = int(path[j - 1]), int(path[j])
            e = indptr[a] + np.searchsorted(indices[indptr[a]:indptr[a + 1]], b)
            assert e < indptr[a + 1] and indices[e] == b, f"time {j}: {a} -> {b} is not a stored transition"
            tmp = np.float32(logB(b, ob[j]))
            val = np.float32(np.float64(np.float32(tmp + val)) + math.log(float(data[e])))
        assert bits(val) == bits(score), f"score along the path {val!r}, returned {score!r}"
        runs = []
        for dbg in (0, EAGER, ALL_LAYOUTS):
            sp.set_option(D.OPT_DEBUG, dbg)
            try:
                runs.append(sp.decode_beam(ob, 3, B, D.MODE_REFERENCE))
            finally:
                sp.set_option(D.OPT_DEBUG, 0)
        assert same(runs[0], runs[1]) and same(runs[0], runs[2])
        assert sp.stats()["kernel"] == D.KERNEL_CSR_F64
    finally:
        sp.close()


# ---------------------------------------------------------------- 8. the switch

def test_switch_values_and_refusals():
    A, Bm, Pi, ob = modelgen.model32(dict(kind="sparse_fast", K=300, M=8, T=20, prob=0.05, seed=1001))
    sp = sparse_ctx(decoder.dense_to_csr(A), Bm, Pi, option=None)
    sets = [(np.full(8, -1.0, np.float32), np.arange(8, dtype=np.int32))]
    try:
        for _ in range(2):
            refused(lambda: sp.decode_beam(ob, 2, 8), D.ERR_UNSUPPORTED, "fv_set_model_sparse")
            refused(lambda: sp.decode_beam_batch([ob, ob[:7]], 2, 8), D.ERR_UNSUPPORTED, "fv_set_model_sparse")
            refused(lambda: sp.test_beam_step(8, sets, [0]), D.ERR_UNSUPPORTED, "fv_set_model_sparse")
            refused(lambda: sp.set_option(D.OPT_SPARSE_BEAM, 2), D.ERR_ARG)
            refused(lambda: sp.set_option(D.OPT_SPARSE_BEAM, -1), D.ERR_ARG)
            sp.set_option(D.OPT_SPARSE_BEAM, 0)                      # (explicitly: the default again)
        sp.set_option(D.OPT_SPARSE_BEAM, 1)
        on = sp.decode_beam(ob, 2, 8)
        refused(lambda: sp.decode_checkpoint(ob), D.ERR_UNSUPPORTED, "fv_set_model_sparse")     # out of scope: stays refused
        odd = [outcome(lambda: sp.decode_beam(ob, 10, 8)),           # T == 2 * n_split
               outcome(lambda: sp.decode_beam(ob, 2, 301)),          # beam > K
               outcome(lambda: sp.decode_beam(ob, 2, 1)),
               outcome(lambda: sp.decode_beam(np.where(ob == 3, 8, ob), 2, 8)),      # a symbol outside the model's
               outcome(lambda: sp.decode_beam_batch([ob, ob[:20]], 10, 8))]
        sp.set_option(D.OPT_SPARSE_BEAM, 0)
        refused(lambda: sp.decode_beam(ob, 2, 8), D.ERR_UNSUPPORTED, "fv_set_model_sparse")
        de = dense_ctx(A, Bm, Pi)
        try:
            assert same(on, de.decode_beam(ob, 2, 8))
            # admission is the dense-set model's: the same input is refused or accepted alike
            assert odd == [outcome(lambda: de.decode_beam(ob, 10, 8)), outcome(lambda: de.decode_beam(ob, 2, 301)),
                           outcome(lambda: de.decode_beam(ob, 2, 1)), outcome(lambda: de.decode_beam(np.where(ob == 3, 8, ob), 2, 8)),
                           outcome(lambda: de.decode_beam_batch([ob, ob[:20]], 10, 8))]
            assert sum(o[0] == "refused" for o in odd) >= 3
        finally:
            de.close()
    finally:
        sp.close()


def test_multi_device_context_passes_the_option_to_its_members():
    """Three members on one device: fv_decode_beam deals the segments to them, fv_decode_beam_batch is refused as on a
    dense-set model."""
    A, Bm, Pi, ob = modelgen.model32(dict(kind="ties_semi", K=400, M=8, T=48, prob=0.5, seed=1051))
    de = dense_ctx(A, Bm, Pi)
    want = de.decode_beam(ob, 4, 40)
    de.close()
    fv = decoder.FlashViterbi([0, 0, 0])
    try:
        fv.set_model_sparse(*decoder.dense_to_csr(A), Bm, Pi)
        refused(lambda: fv.decode_beam(ob, 4, 40), D.ERR_UNSUPPORTED, "fv_set_model_sparse")
        refused(lambda: fv.set_option(D.OPT_SPARSE_BEAM, 2), D.ERR_ARG)
        fv.set_option(D.OPT_SPARSE_BEAM, 1)
        assert same(fv.decode_beam(ob, 4, 40), want)
        refused(lambda: fv.decode_beam_batch([ob, ob[:9]], 4, 40), D.ERR_UNSUPPORTED, "one device")
    finally:
        fv.close()


def test_option_changes_nothing_on_a_dense_set_model():
    g, r = PAIRS[0]
    A, Bm, Pi, ob = golden_model(g)
    de = dense_ctx(A, Bm, Pi)
    try:
        before = de.decode_beam(ob, r["N"], r["B"])
        kernel = de.stats()["kernel"]
        de.set_option(D.OPT_SPARSE_BEAM, 1)
        after = de.decode_beam(ob, r["N"], r["B"])
        assert same(before, after) and after[0].tolist() == r["path"] and de.stats()["kernel"] == kernel == D.KERNEL_F64_STREAM
    finally:
        de.close()


def test_model_replaced_in_both_orders():
    A1, B1, Pi1, ob1 = modelgen.model32(dict(kind="ties_semi", K=400, M=8, T=30, prob=0.5, seed=1101))
    A2, B2, Pi2, ob2 = modelgen.model32(dict(kind="sparse_fast", K=700, M=8, T=30, prob=0.03, seed=1102))
    ref = []
    for A, Bm, Pi, ob in ((A1, B1, Pi1, ob1), (A2, B2, Pi2, ob2)):
        de = dense_ctx(A, Bm, Pi)
        ref.append(de.decode_beam(ob, 3, 40))
        de.close()
    fv = decoder.FlashViterbi(0)
    try:
        fv.set_option(D.OPT_SPARSE_BEAM, 1)
        fv.set_model_sparse(*decoder.dense_to_csr(A1), B1, Pi1)
        assert same(fv.decode_beam(ob1, 3, 40), ref[0])
        fv.set_model(A2, B2, Pi2)                                    # dense replaces sparse
        assert same(fv.decode_beam(ob2, 3, 40), ref[1]) and fv.stats()["kernel"] == D.KERNEL_F64_STREAM
        fv.set_model_sparse(*decoder.dense_to_csr(A2), B2, Pi2)      # sparse replaces dense, same model
        assert same(fv.decode_beam(ob2, 3, 40), ref[1]) and fv.stats()["kernel"] == D.KERNEL_CSR_F64
        fv.set_model(A1, B1, Pi1)
        assert same(fv.decode_beam(ob1, 3, 40), ref[0])
        fv.set_model_sparse(*decoder.dense_to_csr(A1), B1, Pi1)      # a smaller sparse model after a larger one
        assert same(fv.decode_beam(ob1, 3, 40), ref[0])
    finally:
        fv.close()
