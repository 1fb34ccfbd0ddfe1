"""GPU: fv_set_emissions — decodes from per-time emission scores (ob=None) against the reference binaries' goldens and
the oracle.

A model with M = T, B'[i][t] = E[t][i] and ob = 0..T-1 is the oracle's restatement of a decode on emission rows E, so
every check is bit-exact: paths equal, float32 scores equal, return codes equal.  Log scores are taken per element with
math.log (the host libm's log, which is what fv_set_model and the oracle call); numpy's vectorised log differs from it
in the last bit for some inputs and would show up as false mismatches.
"""
import math
import re

import numpy as np
import pytest

import modelgen
import oracle
from conftest import golden_model, golden_runs, load_goldens
from flash_viterbi_amd import decoder

pytestmark = pytest.mark.gpu

D = decoder
FREE = ["ds_K200_T100", "ds_K77_M7_T33", "ds_K512_T64", "ties_semi_K96_T80"]


def libm_log(x):
    """float64 log of every float32 entry of x through math.log; log 0 = -inf"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    vals, inv = np.unique(x.reshape(-1), return_inverse=True)
    table = np.array([math.log(float(v)) if v > 0 else -math.inf for v in vals], dtype=np.float64)
    return table[inv].reshape(x.shape)


def golden(name):
    return next(g for g in load_goldens() if g["name"] == name)


def free_emissions(T, K, seed=7):
    """the issue's recipe: entries of {1e-16, 1e-8, 1e-3, U(0.1, 1)}, five percent of them 0"""
    rs = np.random.RandomState(seed)
    E = modelgen._classes(rs, (T, K)).astype(np.float32)
    E[rs.uniform(size=(T, K)) < 0.05] = 0
    return E


class Free:
    """A and Pi of a golden with free per-time emissions E[T][K]: context, oracle model (M = T) and the staged log scores."""

    def __init__(self, name, E=None):
        g = golden(name)
        self.A, _, self.Pi, ob = golden_model(g)
        self.K = self.A.shape[0]
        self.E = free_emissions(len(ob), self.K) if E is None else E
        self.T = self.E.shape[0]
        self.logE = libm_log(self.E)
        self.om = oracle.OracleModel(self.A, np.ascontiguousarray(self.E.T), self.Pi)
        self.t = np.arange(self.T, dtype=np.int32)
        self.fv = decoder.FlashViterbi(0)
        # B only gives the model its shape here: ob=None decodes never read it
        self.fv.set_model(self.A, np.full((self.K, 2), 0.5, np.float32), self.Pi)
        self.fv.set_emissions(self.logE)

    def close(self):
        self.fv.close()
        self.om.close()


@pytest.fixture(scope="module")
def free():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Free(name)
        return cache[name]
    yield get
    for c in cache.values():
        c.close()


def same(got, want):
    return got[0].tolist() == want[0].tolist() and got[1] == want[1] and got[2] == want[2]


# ---------------------------------------------------------------- 1. goldens through emissions

@pytest.fixture(scope="module")
def gctx():
    cache = {}

    def get(g):
        if g["name"] not in cache:
            A, B, Pi, ob = golden_model(g)
            fv = decoder.FlashViterbi(0)
            fv.set_model(A, B, Pi)
            logB = libm_log(B)                              # [K][M]
            fv.set_emissions(np.ascontiguousarray(logB[:, ob].T))      # logE64[t][i] = log(B[i][ob[t]])
            cache[g["name"]] = (fv, ob)
        return cache[g["name"]]
    yield get
    for fv, _ in cache.values():
        fv.close()


GPAIRS, GIDS = golden_runs()


@pytest.mark.parametrize("g,r", GPAIRS, ids=GIDS)
def test_golden_runs_through_emissions(gctx, g, r):
    """ob=None on logE[t][i] = log(B[i][ob[t]]) gives the reference binary's stored path, and the score and return code of
    the symbol decode bit for bit; flash runs under F64_STREAM and AUTO with FV_OPT_MAX_BATCH 1 and 8."""
    fv, ob = gctx(g)
    T = len(ob)
    assert fv.stats()["emission_rows"] == T                # the fixture staged T rows; decodes keep the count
    try:
        if r["algo"] == "flash":
            for kernel in (D.KERNEL_F64_STREAM, D.KERNEL_AUTO):
                for batch in (1, 8):
                    fv.set_option(D.OPT_KERNEL, kernel)
                    fv.set_option(D.OPT_MAX_BATCH, batch)
                    sym = fv.decode_full(ob, r["N"])
                    sym_kernel = fv.stats()["kernel"]
                    got = fv.decode_full(None, r["N"], T=T)
                    assert got[0].tolist() == r["path"], (kernel, batch)
                    assert same(got, sym) and got[2] == 0, (kernel, batch)
                    assert fv.stats()["kernel"] == sym_kernel      # the same step kernel on both routes
                    assert fv.stats()["emission_rows"] == T
        elif r["algo"] == "flashbs":
            sym = fv.decode_beam(ob, r["N"], r["B"])
            got = fv.decode_beam(None, r["N"], r["B"], T=T)
            assert got[0].tolist() == r["path"] and same(got, sym)
        elif r["algo"] == "vanilla":
            sym = fv.decode_vanilla(ob)
            got = fv.decode_vanilla(None, T=T)
            assert got[0].tolist() == r["path"] and same(got, sym) and got[1] == np.float32(r["score"])
        else:
            sym = fv.decode_checkpoint(ob, r["step"])
            got = fv.decode_checkpoint(None, r["step"], T=T)
            assert got[0].tolist() == r["path"] and same(got, sym) and got[1] == np.float32(r["score"])
    finally:
        fv.set_option(D.OPT_KERNEL, D.KERNEL_AUTO)
        fv.set_option(D.OPT_MAX_BATCH, 8)


# ---------------------------------------------------------------- 2. free emissions against the oracle

@pytest.mark.parametrize("name", FREE)
def test_free_emissions_match_oracle(free, name):
    c = free(name)
    fv, om, T = c.fv, c.om, c.T
    for N in (1, 4, 8):
        if T == 2 * N:
            continue
        opath, oscore, _, orc = om.full_decode(c.t, N)
        assert orc == 0
        assert same(fv.decode_full(None, N, T=T), (opath, oscore, 0)), N
    for B in (8, 32):
        for N in (1, 4):
            opath, oscore, _, orc = om.beam_decode(c.t, N, B)
            if (name, B, N) == ("ds_K512_T64", 8, 4):
                # the one beam miss of these cases: 20 entries of -1, kept on purpose
                assert orc == D.WARN_BEAM_MISS and int((opath == -1).sum()) == 20
            else:
                assert orc == 0
            assert same(fv.decode_beam(None, N, B, T=T), (opath, oscore, orc)), (B, N)
    vp, vs, vrc = om.vanilla_decode(c.t)
    assert vrc == 0 and same(fv.decode_vanilla(None, T=T), (vp, vs, 0))
    cp, cs, crc = om.checkpoint_decode(c.t, 0)
    assert crc == 0 and same(fv.decode_checkpoint(None, 0, T=T), (cp, cs, 0))


# ---------------------------------------------------------------- 3. float32 input

def test_float32_input_is_its_widening(free):
    c = free("ds_K200_T100")
    log32 = c.logE.astype(np.float32)                       # some float32 scores (not exact logs of anything)
    fv = decoder.FlashViterbi(0)
    try:
        fv.set_model(c.A, np.full((c.K, 2), 0.5, np.float32), c.Pi)
        res = []
        for arr in (log32, log32.astype(np.float64)):
            fv.set_emissions(arr)
            res.append((fv.decode_full(None, 4, T=c.T), fv.decode_beam(None, 4, 32, T=c.T), fv.decode_vanilla(None, T=c.T)))
        for a, b in zip(*res):
            assert same(a, b)
    finally:
        fv.close()


# ---------------------------------------------------------------- 4. device pointer and pitch

@pytest.mark.parametrize("name,ld,dtype", [("ds_K77_M7_T33", 80, np.float32), ("ds_K512_T64", 512, np.float64)])
def test_device_pointer_and_pitch(free, name, ld, dtype):
    c = free(name)
    K, T = c.K, c.T
    dense = np.ascontiguousarray(c.logE.astype(dtype))
    padded = np.full((T, ld), np.nan, dtype=dtype)          # the pad columns hold NaN: never interpreted
    padded[:, :K] = dense
    fv = decoder.FlashViterbi(0)
    try:
        fv.set_model(c.A, np.full((K, 2), 0.5, np.float32), c.Pi)
        fv.set_emissions(dense)
        want = (fv.decode_full(None, 4, T=T), fv.decode_beam(None, 4, 32, T=T), fv.decode_vanilla(None, T=T))
        if dtype == np.float64:
            opath, oscore, _, _ = c.om.full_decode(c.t, 4)
            assert same(want[0], (opath, oscore, 0))
        fv.clear_emissions()
        fv.set_emissions(padded)                            # host pointer with the pitch
        assert same(fv.decode_full(None, 4, T=T), want[0])
        fv.clear_emissions()
        ptr = fv.test_device_alloc(padded)
        try:
            fv.set_emissions((ptr, dtype, T, ld))           # (raises on FV_ERR_ARG)
        finally:
            fv.test_device_free(ptr)                        # staged: the caller's block may go at once
        got = (fv.decode_full(None, 4, T=T), fv.decode_beam(None, 4, 32, T=T), fv.decode_vanilla(None, T=T))
        for a, b in zip(got, want):
            assert same(a, b)
    finally:
        fv.close()


# ---------------------------------------------------------------- 5. whole step tables

def test_forward_tables_on_emissions_match_oracle(free):
    c = free("ds_K200_T100")
    passes = [(0, 30, -1), (31, 60, 5), (61, 99, 117)]      # one pass from Pi, two right-hand passes
    want = [c.om.full_forward(c.t, L, R, s) for L, R, s in passes]
    try:
        for kernel in (D.KERNEL_AUTO, D.KERNEL_F64_STREAM):
            c.fv.set_option(D.OPT_KERNEL, kernel)
            rows, bp, _ = c.fv.test_forward(None, passes, -2, T=c.T)
            for q, (L, R, s) in enumerate(passes):
                row, args = want[q]
                assert np.array_equal(rows[q].view(np.uint32), row.view(np.uint32)), (kernel, q)
                assert np.array_equal(bp[L + 1:R + 1], args), (kernel, q)
    finally:
        c.fv.set_option(D.OPT_KERNEL, D.KERNEL_AUTO)


# ---------------------------------------------------------------- 6. batches

def test_batches_on_one_staged_block():
    lengths = [33, 2, 64, 17]
    total = sum(lengths)
    g = golden("ds_K77_M7_T33")
    A, _, Pi, _ = golden_model(g)
    K = A.shape[0]
    E = free_emissions(total, K, seed=11)
    logE = libm_log(E)
    offs = np.concatenate([[0], np.cumsum(lengths)])
    fv = decoder.FlashViterbi(0)
    try:
        fv.set_model(A, np.full((K, 2), 0.5, np.float32), Pi)
        single_full, single_beam, want_full, want_beam = [], [], [], []
        for s, n in enumerate(lengths):
            sl = slice(offs[s], offs[s + 1])
            om = oracle.OracleModel(A, np.ascontiguousarray(E[sl].T), Pi)
            t = np.arange(n, dtype=np.int32)
            p, sc, _, rc = om.full_decode(t, 4)
            want_full.append((p, sc, rc))
            p, sc, _, rc = om.beam_decode(t, 4, 16)
            want_beam.append((p, sc, rc))
            om.close()
            fv.set_emissions(np.ascontiguousarray(logE[sl]))
            single_full.append(fv.decode_full(None, 4, T=n))
            single_beam.append(fv.decode_beam(None, 4, 16, T=n))
        fv.set_emissions(logE)
        paths, scores, statuses = fv.decode_full_batch(None, 4, lengths=lengths)
        for s in range(len(lengths)):
            got = (paths[s], scores[s], int(statuses[s]))
            assert same(got, single_full[s]) and same(got, want_full[s]), s
        paths, scores, statuses = fv.decode_beam_batch(None, 4, 16, lengths=lengths)
        for s in range(len(lengths)):
            got = (paths[s], scores[s], int(statuses[s]))
            assert same(got, single_beam[s]) and same(got, want_beam[s]), s
        for call in (lambda: fv.decode_full_batch(None, 4, lengths=[33, 2, 64, 18]),
                     lambda: fv.decode_beam_batch(None, 4, 16, lengths=[33, 2, 64, 18])):
            with pytest.raises(decoder.FlashVitError) as e:
                call()
            assert e.value.rc == D.ERR_ARG
    finally:
        fv.close()


# ---------------------------------------------------------------- 7. CSR-set model

def test_sparse_set_model_decodes_emissions(free):
    c = free("ds_K200_T100")
    want = [c.fv.decode_full(None, N, T=c.T) for N in (1, 4)]
    fv = decoder.FlashViterbi(0)
    try:
        fv.set_model_sparse(*decoder.dense_to_csr(c.A), np.full((c.K, 2), 0.5, np.float32), c.Pi)
        fv.set_emissions(c.logE)
        for dbg in (0, D.DEBUG_CSR_ROWS_IN_MEMORY):         # both score-row forms of the walk
            fv.set_option(D.OPT_DEBUG, dbg)
            for N, w in zip((1, 4), want):
                assert same(fv.decode_full(None, N, T=c.T), w), (dbg, N)
            assert fv.stats()["kernel"] == D.KERNEL_SPARSE_CSR
        fv.set_option(D.OPT_DEBUG, 0)
        with pytest.raises(decoder.FlashVitError) as e:
            fv.decode_beam(None, 4, 32, T=c.T)
        assert e.value.rc == D.ERR_UNSUPPORTED
    finally:
        fv.close()


# ---------------------------------------------------------------- 8. scores above 0

def test_scores_above_zero_take_the_float64_kernels():
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
    om = oracle.OracleModel(A, np.ascontiguousarray(E.T), Pi)
    fv = decoder.FlashViterbi(0)
    sp = decoder.FlashViterbi(0)
    try:
        B = np.full((K, 2), 0.5, np.float32)
        fv.set_model(A, B, Pi)
        fv.set_emissions(logE)
        opath, oscore, _, orc = om.full_decode(t, 4)
        assert same(fv.decode_full(None, 4, T=T), (opath, oscore, orc))
        assert fv.stats()["kernel"] == D.KERNEL_F64_STREAM
        opath, oscore, _, orc = om.beam_decode(t, 4, 32)
        assert same(fv.decode_beam(None, 4, 32, T=T), (opath, oscore, orc))
        vp, vs, vrc = om.vanilla_decode(t)
        assert same(fv.decode_vanilla(None, T=T), (vp, vs, vrc))
        fv.set_option(D.OPT_KERNEL, D.KERNEL_Q16_REFINE)
        with pytest.raises(decoder.FlashVitError) as e:
            fv.decode_full(None, 4, T=T)
        assert e.value.rc == D.ERR_UNSUPPORTED
        # the model itself is within [0, 1]: a symbol decode still takes the forced filter kernel
        assert fv.decode_full(np.zeros(T, np.int32), 4)[2] == 0 and fv.stats()["kernel"] == D.KERNEL_Q16_REFINE
        sp.set_model_sparse(*decoder.dense_to_csr(A), B, Pi)
        sp.set_emissions(logE)
        with pytest.raises(decoder.FlashVitError) as e:
            sp.decode_full(None, 4, T=T)
        assert e.value.rc == D.ERR_UNSUPPORTED
    finally:
        fv.close()
        sp.close()
        om.close()


# ---------------------------------------------------------------- 9. life cycle and refusals

def refused(call, rc):
    with pytest.raises(decoder.FlashVitError) as e:
        call()
    assert e.value.rc == rc, str(e.value)
    return str(e.value)


def test_life_cycle_and_refusals(free):
    g = golden("ds_K77_M7_T33")
    A, B, Pi, ob = golden_model(g)
    K, T = A.shape[0], len(ob)
    want = next(r for r in g["runs"] if r["algo"] == "flash")
    logE = libm_log(free_emissions(T, K))
    fv = decoder.FlashViterbi(0)
    try:
        refused(lambda: fv.set_emissions(logE), D.ERR_STATE)                    # before set_model: K is the model's
        fv.set_model(A, B, Pi)
        refused(lambda: fv.decode_full(None, 1, T=T), D.ERR_ARG)                # nothing staged
        fv.set_emissions(logE)
        st = fv.stats()
        assert st["emission_rows"] == T and st["set_emissions_ms"] > 0 and st["device_bytes"] >= 12 * T * K
        fv.decode_full(None, 1, T=T)
        fv.decode_full(None, 1, T=T - 5)                                        # fewer times than rows: fine
        st2 = fv.stats()
        assert st2["emission_rows"] == T and st2["set_emissions_ms"] == st["set_emissions_ms"]      # kept across decodes
        refused(lambda: fv.decode_full(None, 1, T=T + 1), D.ERR_ARG)            # beyond the staged rows
        for call in (lambda: fv.decode_beam(None, 1, 8, T=T + 1), lambda: fv.decode_vanilla(None, T=T + 1),
                     lambda: fv.decode_checkpoint(None, 0, T=T + 1), lambda: fv.test_forward(None, [(0, T, -1)], T=T + 1)):
            refused(call, D.ERR_ARG)
        # while emissions are staged a symbol decode is what it was
        path, score, rc = fv.decode_full(ob, want["N"])
        assert rc == 0 and path.tolist() == want["path"] and score == np.float32(want["score"])
        # refused values: the detail names the lowest (t, state); nothing stays staged
        for bad, dtype in ((np.nan, np.float64), (np.inf, np.float64), (-1e300, np.float64), (np.nan, np.float32), (np.inf, np.float32)):
            fv.set_emissions(logE)
            x = logE.astype(dtype)
            x[20, 3] = bad
            x[5, 17] = bad
            x[5, 40] = bad
            msg = refused(lambda: fv.set_emissions(x), D.ERR_ARG)
            assert re.search(r"t = 5, state = 17\b", msg), msg
            st = fv.stats()                                                     # a refused call reports nothing staged
            assert st["emission_rows"] == 0 and st["set_emissions_ms"] == 0 and st["device_bytes"] >= 12 * T * K
            refused(lambda: fv.decode_full(None, 1, T=T), D.ERR_ARG)
        fv.set_emissions(logE)
        refused(lambda: fv.set_emissions((1 << 20, np.float64, T, K - 1)), D.ERR_ARG)       # ld < K (checked before the pointer is touched)
        refused(lambda: fv.decode_full(None, 1, T=T), D.ERR_ARG)                            # a failed call leaves nothing staged
        refused(lambda: fv.set_emissions((logE.ctypes.data, 7, T, K)), D.ERR_ARG)           # bad dtype
        refused(lambda: fv.set_emissions((logE.ctypes.data, np.float64, 0, K)), D.ERR_ARG)  # T < 1
        refused(lambda: fv.set_emissions((0, np.float64, T, K)), D.ERR_ARG)                 # NULL
        # fv_set_model and fv_clear_emissions drop the rows
        fv.set_emissions(logE)
        fv.set_model(A, B, Pi)
        refused(lambda: fv.decode_full(None, 1, T=T), D.ERR_ARG)
        assert fv.stats()["emission_rows"] == 0
        fv.set_emissions(logE)
        with_tables = fv.stats()["device_bytes"]
        fv.clear_emissions()
        without_tables = fv.stats()["device_bytes"]
        assert fv.stats()["emission_rows"] == 0 and 0 < without_tables <= with_tables - 12 * T * K
        refused(lambda: fv.decode_full(None, 1, T=T), D.ERR_ARG)
        refused(lambda: fv.decode_full_batch(None, 1, lengths=[T]), D.ERR_ARG)
        # a refused call that grew the tables first counts them
        x = logE.copy()
        x[0, 0] = np.nan
        refused(lambda: fv.set_emissions(x), D.ERR_ARG)
        assert fv.stats()["device_bytes"] >= without_tables + 12 * T * K
        # the timing hook of the staging kernel: device blocks only, and nothing stays staged
        fv.set_emissions(logE)
        ptr = fv.test_device_alloc(logE)
        try:
            assert fv.test_stage_emissions_ms(ptr, np.float64, T, K, 2) > 0
            refused(lambda: fv.decode_full(None, 1, T=T), D.ERR_ARG)
            refused(lambda: fv.test_stage_emissions_ms(logE.ctypes.data, np.float64, T, K, 2), D.ERR_ARG)      # a host pointer
            refused(lambda: fv.test_stage_emissions_ms(ptr, np.float64, T, K - 1, 2), D.ERR_ARG)               # ld < K
        finally:
            fv.test_device_free(ptr)
        fv.set_emissions(logE)
        fv.set_model_sparse(*decoder.dense_to_csr(A), B, Pi)
        refused(lambda: fv.decode_full(None, 1, T=T), D.ERR_ARG)
    finally:
        fv.close()


# ---------------------------------------------------------------- 10. sharding

def test_partitions_and_multi_device_context(free):
    c = free("ds_K200_T100")
    T, N = c.T, 8
    want_full = c.fv.decode_full(None, N, T=T)
    want_beam = c.fv.decode_beam(None, N, 32, T=T)
    B = np.full((c.K, 2), 0.5, np.float32)
    parts_full, parts_beam = [], []
    for rank in range(3):
        fv = decoder.FlashViterbi(0)
        try:
            fv.set_model(c.A, B, c.Pi)
            fv.set_partition(rank, 3)
            fv.set_emissions(c.logE)                        # each rank stages its own copy
            parts_full.append(fv.decode_full(None, N, T=T)[0])
            parts_beam.append(fv.decode_beam(None, N, 32, T=T)[0])
        finally:
            fv.close()
    assert decoder.merge_paths(T, N, 3, np.stack(parts_full)).tolist() == want_full[0].tolist()
    assert decoder.merge_paths(T, N, 3, np.stack(parts_beam)).tolist() == want_beam[0].tolist()
    group = decoder.FlashViterbi([0, 0])
    try:
        group.set_model(c.A, B, c.Pi)
        group.set_emissions(c.logE)
        assert same(group.decode_full(None, N, T=T), want_full)
        assert same(group.decode_beam(None, N, 32, T=T), want_beam)
        ptr = c.fv.test_device_alloc(c.logE)                # a device block: one copy per member
        try:
            group.set_emissions((ptr, np.float64, T, c.K))
        finally:
            c.fv.test_device_free(ptr)
        assert same(group.decode_full(None, N, T=T), want_full)
    finally:
        group.close()
