"""GPU: fv_decode_full_batch — several observation sequences against one model in one call.

Bar: for every sequence of a batch, path (int32) and score (float32, ==) are exactly what fv_decode_full returns for
that sequence alone on the same context with the same options — which the rest of the suite pins to the reference
binaries' goldens and to the oracle — whatever the kernel, FV_OPT_MAX_BATCH, FV_OPT_DEBUG value, order or size of the
batch; per-sequence failures stay per sequence; refusals leave nothing running."""
import ctypes

import numpy as np
import pytest

import modelgen
import oracle
from conftest import golden_model, golden_runs
from flash_viterbi_amd import decoder

pytestmark = pytest.mark.gpu

PAIRS, IDS = golden_runs(include_big=True, algo="flash")
KERNELS = [decoder.KERNEL_F64_STREAM, decoder.KERNEL_F32_REFINE, decoder.KERNEL_F16_REFINE, decoder.KERNEL_Q16_REFINE,
           decoder.KERNEL_SPARSE_Q16, decoder.KERNEL_U16_REFINE]
GEN0 = decoder.DEBUG_BATCH_GEN0_SERIAL         # FV_OPT_DEBUG bit 28: the other launch form of a batch's generation 0
# the accepted full-state bits 1, 3, 13, 14, 18, 21, each with generation 0 in either form
DEBUGS = [base | g0 for base in (0, 1 << 1, 1 << 3, 1 << 13, 1 << 14, 1 << 18, 1 << 21, (1 << 14) | (1 << 13), (1 << 18) | (1 << 14))
          for g0 in (0, GEN0)]


def legal(t, n_split):
    """a length next to t that build_plan takes (T == 2N with N > 2 is the one shape it refuses)"""
    t = max(t, 2)
    return t + 1 if (n_split > 2 and t == 2 * n_split) else t


def same(got, want):
    (gp, gs, gst), (wp, ws, wst) = got, want
    if wst < 0:         # the checker refused the sequence: only the status is compared (the path has its own test below)
        return gst == wst
    return gst == wst and gp.dtype == np.int32 and gp.tolist() == list(np.asarray(wp).tolist()) and np.float32(gs) == np.float32(ws)


def singles(fv, obs, n_split, mode=decoder.MODE_REFERENCE):
    """(path, score, status) of every sequence decoded alone by the existing entry point; a sequence it refuses with
    FV_ERR_NO_PRED (a random partner on a model with symbols few states emit) keeps that status, as the batch reports it"""
    out = []
    for o in obs:
        try:
            p, s, rc = fv.decode_full(o, n_split, mode)
        except decoder.FlashVitError as e:
            if e.rc != decoder.ERR_NO_PRED:
                raise
            p, s, rc = np.empty(0, np.int32), np.float32(0), e.rc
        out.append((p, s, rc))
    return out


def batch(fv, obs, n_split, mode=decoder.MODE_REFERENCE):
    paths, scores, statuses = fv.decode_full_batch(obs, n_split, mode)
    assert len(paths) == len(obs) and scores.dtype == np.float32 and statuses.dtype == np.int32
    return [(paths[s], scores[s], int(statuses[s])) for s in range(len(obs))]


def assert_same(got, want, what=""):
    assert len(got) == len(want)
    for s, (g, w) in enumerate(zip(got, want)):
        assert same(g, w), (what, s, len(w[0]), g[2], w[2], float(g[1]), float(w[1]))


@pytest.fixture(scope="module")
def golden_ctx():
    cache = {}

    def get(g):
        if g["name"] not in cache:
            A, B, Pi, ob = golden_model(g)
            fv = decoder.FlashViterbi(0)
            fv.set_model(A, B, Pi)
            cache[g["name"]] = (fv, oracle.OracleModel(A, B, Pi), np.asarray(ob, dtype=np.int32), B.shape[1], {})
        return cache[g["name"]]
    yield get
    for fv, om, _, _, _ in cache.values():
        fv.close()
        om.close()


@pytest.mark.parametrize("g,r", PAIRS, ids=IDS)
def test_goldens_with_batch_partners(golden_ctx, g, r):
    """The golden's own sequence next to fresh seeded sequences of other lengths: its slot holds the reference
    binary's path and score, every slot the oracle's, every slot the single call's — on each of the six kernels."""
    fv, om, ob, M, want_cache = golden_ctx(g)
    N, T = r["N"], len(ob)
    rs = np.random.RandomState(4242 + N)
    lens = [legal(T // 2 + 1, N), legal(3, N), legal(2 * T, N), legal(T - 1, N)]
    obs = [rs.randint(0, M, lens[0]).astype(np.int32), rs.randint(0, M, lens[1]).astype(np.int32), ob,
           rs.randint(0, M, lens[2]).astype(np.int32), rs.randint(0, M, lens[3]).astype(np.int32)]
    if N not in want_cache:
        want_cache[N] = []
        for o in obs:
            p, s, _, rc = om.full_decode(o, N, check=False)
            want_cache[N].append((p, s, min(rc, 0)))
    want = want_cache[N]
    assert want[2][0].tolist() == r["path"] and want[2][1] == np.float32(r["score"])
    try:
        for kernel in KERNELS:
            fv.set_option(decoder.OPT_KERNEL, kernel)
            got = batch(fv, obs, N)
            assert fv.stats()["kernel"] == kernel
            assert got[2][2] == 0 and got[2][0].tolist() == r["path"] and got[2][1] == np.float32(r["score"]), kernel
            assert_same(got, want, ("oracle", kernel))
            assert_same(got, singles(fv, obs, N), ("single", kernel))
        fv.set_option(decoder.OPT_KERNEL, decoder.KERNEL_AUTO)
        assert_same(batch(fv, obs, N, decoder.MODE_SINGLE_PASS), singles(fv, obs, N, decoder.MODE_SINGLE_PASS), "single-pass mode")
    finally:
        fv.set_option(decoder.OPT_KERNEL, decoder.KERNEL_AUTO)


@pytest.mark.parametrize("kernel", [decoder.KERNEL_U16_REFINE, decoder.KERNEL_SPARSE_Q16, decoder.KERNEL_F64_STREAM, decoder.KERNEL_AUTO],
                         ids=["u16refine", "sparseq16", "f64stream", "auto"])
def test_order_size_batch_limit_and_debug_forms(kernel):
    """One set of 20 ragged sequences as one batch, reversed, and cut into batches of 1, 7 and 13: identical results per
    sequence, for FV_OPT_MAX_BATCH 1, 2, 4, 8 and the accepted full-state FV_OPT_DEBUG bits with generation 0 in either
    launch form."""
    spec = dict(kind="data_script", K=300, M=12, T=8, prob=0.2, seed=77)
    A, B, Pi, _ = modelgen.model32(spec)
    rs = np.random.RandomState(5)
    N = 4
    lens = [legal(int(t), N) for t in [2, 3, 150, 97, 5, 64, 65, 9, 33, 2, 120, 17, 80, 4, 7, 150, 31, 12, 66, 100]]
    obs = [rs.randint(0, 12, t).astype(np.int32) for t in lens]
    om = oracle.OracleModel(A, B, Pi)
    want = []
    for o in obs:
        p, s, _, rc = om.full_decode(o, N, check=False)
        want.append((p, s, min(rc, 0)))
    om.close()
    fv = decoder.FlashViterbi(0)
    fv.set_model(A, B, Pi)
    fv.set_option(decoder.OPT_KERNEL, kernel)
    try:
        assert_same(singles(fv, obs, N), want, "single calls against the oracle")
        for mb in (8, 4, 2, 1):
            fv.set_option(decoder.OPT_MAX_BATCH, mb)
            for dbg in DEBUGS:
                fv.set_option(decoder.OPT_DEBUG, dbg)
                assert_same(batch(fv, obs, N), want, (mb, dbg, "whole"))
                assert_same(batch(fv, obs[::-1], N), want[::-1], (mb, dbg, "reversed"))
                for size in (7, 13) + ((1,) if dbg in (0, GEN0) else ()):
                    got = []
                    for lo in range(0, len(obs), size):
                        got += batch(fv, obs[lo:lo + size], N)
                    assert_same(got, want, (mb, dbg, size))
    finally:
        fv.close()


def test_more_sequences_than_task_slots_against_the_oracle():
    """nseq = 33 at K = 600: generation 0 alone is five launches per lock-step at eight tasks a launch."""
    spec = dict(kind="data_script", K=600, M=20, T=8, prob=0.15, seed=21)
    A, B, Pi, _ = modelgen.model32(spec)
    rs = np.random.RandomState(6)
    N = 8
    obs = [rs.randint(0, 20, legal(int(t), N)).astype(np.int32) for t in rs.randint(2, 90, 33)]
    om = oracle.OracleModel(A, B, Pi)
    want = []
    for o in obs:
        p, s, _, rc = om.full_decode(o, N, check=False)
        want.append((p, s, min(rc, 0)))
    om.close()
    fv = decoder.FlashViterbi(0)
    fv.set_model(A, B, Pi)
    try:
        for kernel in (decoder.KERNEL_AUTO, decoder.KERNEL_U16_REFINE, decoder.KERNEL_SPARSE_Q16, decoder.KERNEL_F64_STREAM):
            fv.set_option(decoder.OPT_KERNEL, kernel)
            for dbg in (0, GEN0):
                fv.set_option(decoder.OPT_DEBUG, dbg)
                assert_same(batch(fv, obs, N), want, (kernel, dbg))
    finally:
        fv.close()


def test_bench_shape_nine_sequences_against_single_calls():
    """K = 3965, T = 256, N = 8 (bench.py's default workload), nine distinct sequences: one more than a launch holds."""
    spec = dict(kind="data_script", K=3965, M=50, T=256, prob=0.112, seed=12)
    A, B, Pi, ob = modelgen.model32(spec)
    rs = np.random.RandomState(7)
    obs = [np.asarray(ob, dtype=np.int32)] + [rs.randint(0, 50, 256).astype(np.int32) for _ in range(8)]
    fv = decoder.FlashViterbi(0)
    fv.set_model(A, B, Pi)
    try:
        for kernel in (decoder.KERNEL_AUTO, decoder.KERNEL_U16_REFINE):
            fv.set_option(decoder.OPT_KERNEL, kernel)
            fv.set_option(decoder.OPT_DEBUG, 0)
            want = singles(fv, obs, 8)
            assert all(w[2] == 0 for w in want)
            for dbg in (0, GEN0):
                fv.set_option(decoder.OPT_DEBUG, dbg)
                assert_same(batch(fv, obs, 8), want, (kernel, dbg))
    finally:
        fv.close()


def test_beyond_one_lds_row_against_single_calls():
    """K = 44000: a float32 score row no longer fits LDS — the packed 16-bit kernel one task a launch,
    the float64 kernel and the f32 filter on the 16-bit table in slabs of source rows, at most four tasks a launch."""
    spec = dict(kind="sparse_fast", K=44000, M=20, T=8, prob=0.02, seed=31)
    A, Bm, Pi, ob = modelgen.model32(spec)
    rs = np.random.RandomState(8)
    obs = [np.asarray(ob, dtype=np.int32), rs.randint(0, 20, 5).astype(np.int32), rs.randint(0, 20, 8).astype(np.int32)]
    fv = decoder.FlashViterbi(0)
    try:
        fv.set_model(A, Bm, Pi)
        for kernel in (decoder.KERNEL_AUTO, decoder.KERNEL_F64_STREAM, decoder.KERNEL_Q16_REFINE):
            fv.set_option(decoder.OPT_KERNEL, kernel)
            want = singles(fv, obs, 3)
            assert all(w[2] == 0 for w in want)
            assert_same(batch(fv, obs, 3), want, kernel)
    finally:
        fv.close()


ADVERSARIAL = [("wideA", 600, 6, 60, 401), ("wideB", 600, 6, 60, 402), ("wideAB", 600, 6, 60, 403), ("ties_all", 512, 4, 48, 404)]


@pytest.mark.parametrize("kind,K,M,T,seed", ADVERSARIAL)
def test_adversarial_arithmetic_with_batch_partners(kind, K, M, T, seed):
    """Wide dynamic range (the packed filter's saturated window) and all-ties models (the path is decided by
    tie-breaking only), as tests/test_gpu_adversarial.py builds them: five sequences a batch against the oracle."""
    if kind == "ties_all":
        A, Bm, Pi = (np.asarray(x, dtype=np.float32) for x in modelgen._ties_all(K, M, seed))
        first = np.random.RandomState(seed).randint(0, M, T).astype(np.int32)
    else:
        A, Bm, Pi, first = modelgen.wide_model(kind, K, M, T, seed)
    rs = np.random.RandomState(seed + 1000)
    N = 4
    obs = [np.asarray(first, dtype=np.int32)] + [rs.randint(0, M, legal(t, N)).astype(np.int32) for t in (T // 2 + 1, 3, 2 * T, T - 7)]
    om = oracle.OracleModel(A, Bm, Pi)
    want = []
    for o in obs:
        p, s, _, rc = om.full_decode(o, N, check=False)
        want.append((p, s, min(rc, 0)))
    om.close()
    fv = decoder.FlashViterbi(0)
    fv.set_model(A, Bm, Pi)
    saturated = 0
    try:
        for kernel in KERNELS:
            fv.set_option(decoder.OPT_KERNEL, kernel)
            for dbg in (0, GEN0, 1 << 14, (1 << 14) | GEN0):
                fv.set_option(decoder.OPT_DEBUG, dbg)
                for mb in (8, 2):
                    fv.set_option(decoder.OPT_MAX_BATCH, mb)
                    assert_same(batch(fv, obs, N), want, (kernel, dbg, mb))
                    if kernel == decoder.KERNEL_U16_REFINE:
                        saturated += fv.stats()["refine_saturated"]
    finally:
        fv.close()
    if kind == "wideB":
        assert saturated > 0, "the saturated-window branch did not run with batch partners"


def dead_symbol_model(K=40, M=6, seed=3):
    """A model in which symbol M - 1 cannot be emitted by any state (B[i][M-1] = 0: log 0 = -inf): a sequence that
    holds it has no finite score from that position on."""
    rs = np.random.RandomState(seed)
    A = rs.uniform(0.05, 1.0, (K, K))
    A /= A.sum(1, keepdims=True)
    B = rs.uniform(0.05, 1.0, (K, M))
    B[:, M - 1] = 0.0
    B /= B.sum(1, keepdims=True)
    Pi = rs.uniform(0.05, 1.0, K)
    Pi /= Pi.sum()
    return A.astype(np.float32), B.astype(np.float32), Pi.astype(np.float32)


def test_a_sequence_without_predecessor_fails_alone():
    A, B, Pi = dead_symbol_model()
    M = B.shape[1]
    rs = np.random.RandomState(9)
    N = 4
    obs = [rs.randint(0, M - 1, t).astype(np.int32) for t in (30, 41, 17, 2, 55)]
    obs[2][9] = M - 1                              # the one sequence that holds the dead symbol
    fv = decoder.FlashViterbi(0)
    fv.set_model(A, B, Pi)
    L = decoder.load_library()
    try:
        # the single call: FV_ERR_NO_PRED, the path it wrote holds -1 entries
        with pytest.raises(decoder.FlashVitError) as ei:
            fv.decode_full(obs[2], N)
        assert ei.value.rc == decoder.ERR_NO_PRED == -3
        lone = np.full(obs[2].size, -7, dtype=np.int32)
        lone_score = ctypes.c_float(0)
        vp = ctypes.c_void_p
        rc = L.fv_decode_full(fv._h, obs[2].ctypes.data_as(vp), obs[2].size, N, 0, lone.ctypes.data_as(vp), ctypes.byref(lone_score))
        assert rc == decoder.ERR_NO_PRED and (lone == -1).any() and not (lone == -7).any()
        want = [fv.decode_full(o, N) for s, o in enumerate(obs) if s != 2]
        for dbg in (0, GEN0):
            fv.set_option(decoder.OPT_DEBUG, dbg)
            # raw call: the return code is the most negative status
            cat = np.concatenate(obs)
            offsets = np.concatenate([[0], np.cumsum([o.size for o in obs])]).astype(np.int64)
            path = np.full(cat.size, -7, dtype=np.int32)
            scores = np.zeros(len(obs), dtype=np.float32)
            statuses = np.full(len(obs), 99, dtype=np.int32)
            rc = L.fv_decode_full_batch(fv._h, cat.ctypes.data_as(vp), offsets.ctypes.data_as(vp), len(obs), N, 0,
                                        path.ctypes.data_as(vp), scores.ctypes.data_as(vp), statuses.ctypes.data_as(vp))
            assert rc == decoder.ERR_NO_PRED
            assert statuses.tolist() == [0, 0, decoder.ERR_NO_PRED, 0, 0]
            assert path[offsets[2]:offsets[3]].tolist() == lone.tolist()
            assert scores[2] == np.float32(lone_score.value)
            # the wrapper does not raise on it and delivers the others intact
            got = batch(fv, obs, N)
            assert got[2][2] == decoder.ERR_NO_PRED and got[2][0].tolist() == lone.tolist()
            assert_same([x for s, x in enumerate(got) if s != 2], want, dbg)
            # NULL score / status pointers are allowed
            rc = L.fv_decode_full_batch(fv._h, cat.ctypes.data_as(vp), offsets.ctypes.data_as(vp), len(obs), N, 0,
                                        path.ctypes.data_as(vp), None, None)
            assert rc == decoder.ERR_NO_PRED
    finally:
        fv.close()


def test_refusals_leave_the_context_usable():
    A, B, Pi = dead_symbol_model()
    M = B.shape[1]
    rs = np.random.RandomState(10)
    obs = [rs.randint(0, M - 1, t).astype(np.int32) for t in (20, 9, 14, 30)]
    fv = decoder.FlashViterbi(0)
    L = decoder.load_library()
    vp = ctypes.c_void_p
    try:
        with pytest.raises(decoder.FlashVitError) as ei:
            fv.decode_full_batch(obs, 2)                       # no model yet
        assert ei.value.rc == decoder.ERR_STATE
        fv.set_model(A, B, Pi)
        want = singles(fv, obs, 2)
        bad = [o.copy() for o in obs]
        bad[2][5] = M                                          # a symbol outside [0, M) in sequence 2
        with pytest.raises(decoder.FlashVitError) as ei:
            fv.decode_full_batch(bad, 2)
        assert ei.value.rc == decoder.ERR_ARG and "sequence 2" in str(ei.value)
        assert_same(batch(fv, obs, 2), want, "after a bad symbol")         # nothing was left running
        for wrong, n_split, needle in ((obs[:1] + [obs[1][:1]] + obs[2:], 2, "sequence 1"),        # T_s < 2
                                       (obs[:3] + [obs[3][:8]], 4, "sequence 3")):                 # T_s == 2 * n_split, n_split > 2
            with pytest.raises(decoder.FlashVitError) as ei:
                fv.decode_full_batch(wrong, n_split)
            assert ei.value.rc == decoder.ERR_ARG and needle in str(ei.value)
        with pytest.raises(decoder.FlashVitError) as ei:
            fv.decode_full_batch([], 2)                        # nseq < 1
        assert ei.value.rc == decoder.ERR_ARG
        cat = np.concatenate(obs)
        offsets = np.concatenate([[0], np.cumsum([o.size for o in obs])]).astype(np.int64)
        path = np.empty(cat.size, dtype=np.int32)
        args = lambda off: (fv._h, cat.ctypes.data_as(vp), off, len(obs), 2, 0, path.ctypes.data_as(vp), None, None)  # noqa: E731
        down = offsets.copy()
        down[2] = down[1] - 3                                  # non-monotone offsets
        assert L.fv_decode_full_batch(*args(down.ctypes.data_as(vp))) == decoder.ERR_ARG
        shifted = offsets + 1                                  # offsets[0] != 0
        assert L.fv_decode_full_batch(*args(shifted.ctypes.data_as(vp))) == decoder.ERR_ARG
        assert L.fv_decode_full_batch(*args(None)) == decoder.ERR_ARG
        assert L.fv_decode_full_batch(fv._h, None, offsets.ctypes.data_as(vp), len(obs), 2, 0, path.ctypes.data_as(vp), None, None) == decoder.ERR_ARG
        assert L.fv_decode_full_batch(fv._h, cat.ctypes.data_as(vp), offsets.ctypes.data_as(vp), len(obs), 2, 0, None, None, None) == decoder.ERR_ARG
        assert L.fv_decode_full_batch(fv._h, cat.ctypes.data_as(vp), offsets.ctypes.data_as(vp), len(obs), 2, 7, path.ctypes.data_as(vp), None, None) == decoder.ERR_ARG
        assert_same(batch(fv, obs, 2), want, "after the refusals")
        assert_same(batch(fv, obs[:1], 2), want[:1], "nseq == 1 is the single call")
    finally:
        fv.close()
    multi = decoder.FlashViterbi([0, 0])
    try:
        multi.set_model(A, B, Pi)
        with pytest.raises(decoder.FlashVitError) as ei:
            multi.decode_full_batch(obs, 2)
        assert ei.value.rc == decoder.ERR_UNSUPPORTED and "one device" in str(ei.value)
        p, s, rc = multi.decode_full(obs[0], 2)                # the context still decodes
        assert rc == 0 and p.tolist() == want[0][0].tolist()
    finally:
        multi.close()
    part = decoder.FlashViterbi(0)
    try:
        part.set_model(A, B, Pi)
        part.set_partition(0, 2)
        with pytest.raises(decoder.FlashVitError) as ei:
            part.decode_full_batch(obs, 2)
        assert ei.value.rc == decoder.ERR_UNSUPPORTED
    finally:
        part.close()


def test_stats_report_the_batch_as_one_decode():
    """Counters are totals, `generations` the largest of any sequence; the one structural statement that sequences share
    table sweeps: a batch of eight equal sequences takes fewer step launches than eight single decodes."""
    spec = dict(kind="data_script", K=333, M=20, T=96, prob=0.15, seed=9)
    A, B, Pi, ob = modelgen.model32(spec)
    rs = np.random.RandomState(11)
    N = 4
    obs = [np.asarray(ob, dtype=np.int32), rs.randint(0, 20, 40).astype(np.int32), rs.randint(0, 20, 7).astype(np.int32)]
    fv = decoder.FlashViterbi(0)
    fv.set_model(A, B, Pi)
    keys = ("cells", "task_steps", "column_steps", "alg_bytes", "passes", "refine_near", "refine_rescan", "refine_saturated")
    try:
        for kernel in (decoder.KERNEL_AUTO, decoder.KERNEL_U16_REFINE, decoder.KERNEL_F64_STREAM):
            fv.set_option(decoder.OPT_KERNEL, kernel)
            for dbg in (0, GEN0):
                fv.set_option(decoder.OPT_DEBUG, dbg)
                one = []
                for o in obs:
                    fv.decode_full(o, N)
                    one.append(fv.stats())
                batch(fv, obs, N)
                st = fv.stats()
                for k in ("cells", "task_steps", "column_steps", "alg_bytes", "passes"):
                    assert st[k] == sum(x[k] for x in one), (k, kernel, dbg)
                assert st["generations"] == max(x["generations"] for x in one)
                assert st["kernel"] == one[0]["kernel"] and st["ranks"] == 1
                assert st["step_launches"] <= sum(x["step_launches"] for x in one)
                eight = [obs[0]] * 8
                batch(fv, eight, N)
                st8 = fv.stats()
                assert st8["cells"] == 8 * one[0]["cells"] and st8["passes"] == 8 * one[0]["passes"]
                assert st8["step_launches"] < 8 * one[0]["step_launches"], (kernel, dbg)
                assert st8["generations"] == one[0]["generations"]
        assert keys
    finally:
        fv.close()


def test_single_decode_is_untouched_by_a_batch_before_it():
    """One context alternates between batch and single calls of different sizes (workspace buffers grow and are
    reused); the single call keeps returning what it returned before the first batch."""
    spec = dict(kind="data_script", K=333, M=20, T=96, prob=0.15, seed=9)
    A, B, Pi, ob = modelgen.model32(spec)
    rs = np.random.RandomState(12)
    obs = [np.asarray(ob, dtype=np.int32)] + [rs.randint(0, 20, int(t)).astype(np.int32) for t in (200, 3, 50, 77)]
    fv = decoder.FlashViterbi(0)
    fv.set_model(A, B, Pi)
    try:
        before = singles(fv, obs, 4)
        for _ in range(2):
            assert_same(batch(fv, obs, 4), before)
            assert_same(singles(fv, obs, 4), before)
            assert_same(batch(fv, obs[1:3], 4), before[1:3])
            bp, bs, brc = fv.decode_beam(obs[0], 4, 32)          # the beam driver shares the workspace
            assert_same(batch(fv, obs[::-1], 4), before[::-1])
    finally:
        fv.close()


def test_run_hip_batch_prints_one_path_line_per_file(tmp_path, monkeypatch, capsys):
    """run_hip.py --batch FILE...: the model of parameters[0] read from the files the host programs open, one
    fv_decode_full_batch call, one `path:` line per observation file — the golden's own file prints the reference path."""
    import importlib.util
    import os
    import re
    import sys
    from conftest import ROOT, load_goldens
    spec_ = importlib.util.spec_from_file_location("run_hip", os.path.join(ROOT, "flash_viterbi_amd", "src", "run_hip.py"))
    run_hip = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(run_hip)
    g = next(x for x in load_goldens() if x["name"] == "cfg1_K128_T256")
    spec = g["spec"]
    rf = next(x for x in g["runs"] if x["algo"] == "flash" and x["N"] == 8)
    data_dir = str(tmp_path / "data") + os.sep
    modelgen.write_text(spec, data_dir)
    A, B, Pi, ob = golden_model(g)
    rs = np.random.RandomState(13)
    extra = [rs.randint(0, spec["M"], t).astype(np.int32) for t in (40, 300)]
    files = [os.path.join(data_dir, f"ob_K{spec['K']}_T{spec['T']}_prob{spec['prob']}.txt")]
    for i, o in enumerate(extra):
        files.append(str(tmp_path / f"extra{i}.txt"))
        with open(files[-1], "w") as fh:
            fh.write(" ".join(str(int(x)) for x in o))
    p = {"K_STATE": spec["K"], "T_STATE": spec["M"], "obserRouteLEN": spec["T"], "prob": spec["prob"], "MAX_THREADS": 8, "BeamSearchWidth": 32}
    monkeypatch.setattr(run_hip, "data_path", data_dir)
    monkeypatch.setattr(run_hip, "parameters", [p])
    monkeypatch.setattr(sys, "argv", ["run_hip.py", "--batch"] + files)
    with pytest.raises(SystemExit) as ei:
        run_hip.main()
    assert ei.value.code == 0
    out = capsys.readouterr().out
    paths = [[int(x) for x in m.split()] for m in re.findall(r"path: \[([^\]]*)\]", out)]
    assert len(paths) == 3 and re.search(r"time: [\d.]+", out)
    assert paths[0] == rf["path"]
    om = oracle.OracleModel(A, B, Pi)
    for got, o in zip(paths[1:], extra):
        assert got == om.full_decode(o, 8)[0].tolist()
    om.close()
