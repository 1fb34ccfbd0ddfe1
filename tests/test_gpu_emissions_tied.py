"""GPU: fv_set_emission_map (tied scores: K states share P classes) and the 16-bit score types of fv_set_emissions.

The staged tables are defined as what staging the caller's own expansion / widening would have staged, so every check
is an equality: paths with their -1 entries, float32 scores, return codes, and whole step tables through test_forward.
The decodes are called through the C functions directly, so that a path of a decode that answers FV_ERR_NO_PRED is
compared as well (the wrapper raises on it).
"""
import ctypes
import json
import re
import subprocess
import sys

import numpy as np
import pytest

import oracle
from conftest import ROOT, golden_model
from flash_viterbi_amd import decoder
from test_gpu_emissions import free_emissions, golden, libm_log, refused

pytestmark = pytest.mark.gpu

D = decoder
F16_NAN, BF16_NAN = 0x7E00, 0x7FC0


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def raw(fv, what, T, *a):
    """(path, score, rc) of one decode on the staged rows, whatever rc is"""
    path = np.full(T, -7, dtype=np.int32)
    score = ctypes.c_float(0)
    L, h, s = fv._L, fv._h, ctypes.byref(score)
    if what == "full":
        rc = L.fv_decode_full(h, None, T, a[0], D.MODE_REFERENCE, _p(path), s)
    elif what == "beam":
        rc = L.fv_decode_beam(h, None, T, a[0], a[1], D.MODE_REFERENCE, _p(path), s)
    elif what == "vanilla":
        rc = L.fv_decode_vanilla(h, None, T, _p(path), s)
    else:
        rc = L.fv_decode_checkpoint(h, None, T, a[0], _p(path), s)
    return path.tolist(), np.float32(score.value), rc


def eq(a, b):
    """bit-exact: float scores by value (-inf equals -inf), everything else by =="""
    return a[0] == b[0] and a[1] == b[1] and a[2] == b[2]


def vs_oracle(got, want):
    """eq(), but for FV_ERR_NO_PRED (P = 1: a time whose one score is -inf): there the oracle restates the return code and
    the score and leaves its path undefined, so the path is only asked to hold its -1 entries — the convention of
    test_gpu_sparse_f64.compare_entry_points.  (Against the expanded route on the GPU such a path is compared in full.)"""
    if want[2] == D.ERR_NO_PRED:
        return got[2] == want[2] and got[1] == want[1] and -1 in got[0] and -7 not in got[0]
    return eq(got, want)


def full_runs(fv, T, splits=(1, 4, 8)):
    """{(kernel, batch, N): decode_full}: AUTO and F64_STREAM, FV_OPT_MAX_BATCH 1 and 8"""
    out = {}
    try:
        for kernel in (D.KERNEL_AUTO, D.KERNEL_F64_STREAM):
            for batch in (1, 8):
                fv.set_option(D.OPT_KERNEL, kernel)
                fv.set_option(D.OPT_MAX_BATCH, batch)
                for N in splits:
                    out[("full", kernel, batch, N)] = raw(fv, "full", T, N)
    finally:
        fv.set_option(D.OPT_KERNEL, D.KERNEL_AUTO)
        fv.set_option(D.OPT_MAX_BATCH, 8)
    return out


def all_runs(fv, T):
    """every decode of a dense-set model on the staged rows"""
    out = full_runs(fv, T)
    for B in (8, 32):
        for N in (1, 4):
            out[("beam", N, B)] = raw(fv, "beam", T, N, B)
    out[("vanilla",)] = raw(fv, "vanilla", T)
    out[("checkpoint",)] = raw(fv, "checkpoint", T, 0)
    return out


def tables(fv, T, K):
    """score and back-pointer rows of three passes under both kernel choices, every column, as bytes"""
    passes = [(0, T // 3, -1), (T // 3 + 1, 2 * T // 3, 5 % K), (2 * T // 3 + 1, T - 1, (K * 3) // 5)]
    out = {}
    try:
        for kernel in (D.KERNEL_AUTO, D.KERNEL_F64_STREAM):
            fv.set_option(D.OPT_KERNEL, kernel)
            rows, bp, _ = fv.test_forward(None, passes, -2, T=T)
            out[kernel] = (rows.tobytes(), bp.tobytes())
    finally:
        fv.set_option(D.OPT_KERNEL, D.KERNEL_AUTO)
    return out


def assert_same_runs(got, want, tag=""):
    assert got.keys() == want.keys()
    for k in want:
        assert eq(got[k], want[k]), (tag, k, got[k][1:], want[k][1:])


def bf16_to_f32(U):
    return (U.astype(np.uint32) << 16).view(np.float32)


def f32_to_bf16_bits(x):
    """the high halves of float32 values (truncation: any bfloat16 block will do)"""
    return (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16)


def dense_ctx(name):
    g = golden(name)
    A, _, Pi, ob = golden_model(g)
    K = A.shape[0]
    fv = decoder.FlashViterbi(0)
    fv.set_model(A, np.full((K, 2), 0.5, np.float32), Pi)      # (B gives the model its shape: ob=None decodes never read it)
    return fv, A, Pi, K, len(ob)


def stage_bits(fv, bits, code, T, ld):
    """a uint16 block of binary16 / bfloat16 bit patterns from the host, through the pointer form"""
    fv.set_emissions((bits.ctypes.data, code, T, ld))


# ---------------------------------------------------------------- 1. tied equals expanded, against the oracle

@pytest.mark.parametrize("name", ["ds_K77_M7_T33", "ds_K200_T100"])
def test_tied_equals_expanded_and_oracle(name):
    fv, A, Pi, K, T = dense_ctx(name)
    t = np.arange(T, dtype=np.int32)
    try:
        for P in (1, 7, K, K + 5):
            rs = np.random.RandomState(100 + P)
            used = min(P, K)
            pdf = rs.randint(0, used, size=K).astype(np.int32)
            pdf[rs.permutation(K)[:used]] = np.arange(used)          # every one of the first `used` classes is used
            S = free_emissions(T, P)
            logS = libm_log(S)
            staged = logS.copy()
            staged[:, used:] = np.nan                                # P = K + 5: five columns no state maps to
            assert int(np.isnan(staged).all(axis=0).sum()) == P - used
            fv.set_emission_map(pdf, P)
            assert fv.P == P
            fv.set_emissions(staged)
            got = all_runs(fv, T)
            fv.set_emission_map(None)
            fv.set_emissions(np.ascontiguousarray(logS[:, pdf]))
            assert_same_runs(got, all_runs(fv, T), ("expanded", P))
            om = oracle.OracleModel(A, np.ascontiguousarray(S[:, pdf].T), Pi)      # M = T, B'[i][t] = S[t][pdf[i]]
            try:
                for key, res in got.items():
                    if key[0] == "full":
                        p, s, _, rc = om.full_decode(t, key[3], check=False)
                    elif key[0] == "beam":
                        p, s, _, rc = om.beam_decode(t, key[1], key[2], check=False)
                    elif key[0] == "vanilla":
                        p, s, rc = om.vanilla_decode(t, check=False)
                    else:
                        p, s, rc = om.checkpoint_decode(t, 0, check=False)
                    assert vs_oracle(res, (p.tolist(), s, rc)), ("oracle", P, key, res[1:], (s, rc))
            finally:
                om.close()
    finally:
        fv.close()


# ---------------------------------------------------------------- 2. 16-bit equals its widening

def sixteen_bit_blocks(K, T, positive):
    """(H float16 [T][K], U uint16 bfloat16 bits [T][K]) from the log of free emissions, with the corner values"""
    logE = libm_log(free_emissions(T, K))
    H = logE.astype(np.float16)
    H[1, 2] = np.float16(-6e-8)                                      # a subnormal
    H[2, 3] = np.float16(65504.0 if positive else -65504.0)          # the largest finite binary16
    assert np.isneginf(H).any() and 0 < abs(float(H[1, 2])) < 6.2e-5 and abs(float(H[2, 3])) == 65504.0
    U = f32_to_bf16_bits(logE.astype(np.float32))
    U[2, 3] = 0xFF7F                                                 # the largest finite bfloat16, negated
    if positive:
        U[1, 2] = 0x4120                                             # 10.0
    assert (U == 0xFF80).any()                                       # -inf
    return H, U


@pytest.mark.parametrize("positive", [False, True])
@pytest.mark.parametrize("name,ld", [("ds_K77_M7_T33", 79), ("ds_K512_T64", 515)])
def test_sixteen_bit_equals_its_widening(name, ld, positive):
    fv, A, Pi, K, T = dense_ctx(name)
    try:
        H, U = sixteen_bit_blocks(K, T, positive)
        for bits, code, wide, nan in ((H.view(np.uint16), D.EMIS_LOG_F16, H.astype(np.float32), F16_NAN),
                                      (U, D.EMIS_LOG_BF16, bf16_to_f32(U), BF16_NAN)):
            fv.set_emissions(wide)
            assert wide.dtype == np.float32
            want, want_tab = all_runs(fv, T), tables(fv, T, K)
            if positive:
                fv.decode_full(None, 4, T=T)
                assert fv.stats()["kernel"] == D.KERNEL_F64_STREAM   # a 16-bit score above 0 counts as any other
            padded = np.full((T, ld), nan, dtype=np.uint16)          # odd pitch, NaN pads
            padded[:, :K] = bits
            shifted = np.concatenate([np.array([nan], np.uint16), padded.reshape(-1)])      # entered one element in
            ptr, ptr1 = fv.test_device_alloc(padded), fv.test_device_alloc(shifted)
            try:
                routes = {"host": lambda: stage_bits(fv, np.ascontiguousarray(bits), code, T, K),
                          "host pitch": lambda: stage_bits(fv, padded, code, T, ld),
                          "device odd pitch": lambda: fv.set_emissions((ptr, code, T, ld)),
                          "device 2-byte aligned": lambda: fv.set_emissions((ptr1 + 2, code, T, ld))}
                if code == D.EMIS_LOG_F16:
                    routes["numpy float16"] = lambda: fv.set_emissions(H)
                for tag, stage in routes.items():
                    fv.clear_emissions()
                    stage()
                    assert fv.stats()["emission_rows"] == T
                    assert_same_runs(all_runs(fv, T), want, (code, tag))
                    assert tables(fv, T, K) == want_tab, (code, tag)
            finally:
                fv.test_device_free(ptr)
                fv.test_device_free(ptr1)
    finally:
        fv.close()


# ---------------------------------------------------------------- 3. both together, every dtype, CSR-set model

def typed_blocks(logS):
    """{name: (array to stage (uint16 bits for the 16-bit types), dtype code, the float64 widening of what it holds)}"""
    h = logS.astype(np.float16)
    u = f32_to_bf16_bits(logS.astype(np.float32))
    f = logS.astype(np.float32)
    return {"f16": (h.view(np.uint16), D.EMIS_LOG_F16, h.astype(np.float64)),
            "bf16": (u, D.EMIS_LOG_BF16, bf16_to_f32(u).astype(np.float64)),
            "f32": (f, D.EMIS_LOG_F32, f.astype(np.float64)),
            "f64": (logS, D.EMIS_LOG_F64, logS)}


def csr_runs(fv, T, lengths):
    out = {}
    try:
        for dbg in (0, D.DEBUG_CSR_ROWS_IN_MEMORY):                  # both score-row forms of the walk
            fv.set_option(D.OPT_DEBUG, dbg)
            for N in (1, 4):
                out[(dbg, N)] = raw(fv, "full", T, N)
            paths, scores, statuses = fv.decode_full_batch(None, 4, lengths=lengths)
            for s in range(len(lengths)):
                out[(dbg, "batch", s)] = (paths[s].tolist(), scores[s], int(statuses[s]))
    finally:
        fv.set_option(D.OPT_DEBUG, 0)
    return out


def test_tied_every_dtype_on_a_sparse_set_model():
    g = golden("ds_K200_T100")
    A, _, Pi, ob = golden_model(g)
    K, T, P = A.shape[0], len(ob), 37
    lengths = [33, 2, 48, 17]
    rs = np.random.RandomState(5)
    pdf = rs.randint(0, P, size=K).astype(np.int32)
    S = free_emissions(T, P)
    fv = decoder.FlashViterbi(0)
    try:
        fv.set_model_sparse(*decoder.dense_to_csr(A), np.full((K, 2), 0.5, np.float32), Pi)
        for name, (block, code, wide) in typed_blocks(libm_log(S)).items():
            padded = np.full((T, P + 3), np.nan if block.dtype.kind == "f" else (F16_NAN if code == D.EMIS_LOG_F16 else BF16_NAN),
                             dtype=block.dtype)
            padded[:, :P] = block
            fv.set_emission_map(pdf, P)
            fv.set_emissions((padded.ctypes.data, code, T, P + 3))
            got = csr_runs(fv, T, lengths)
            assert fv.stats()["kernel"] == D.KERNEL_SPARSE_CSR
            ptr = fv.test_device_alloc(padded)
            try:
                fv.set_emissions((ptr, code, T, P + 3))
            finally:
                fv.test_device_free(ptr)
            assert_same_runs(csr_runs(fv, T, lengths), got, (name, "device"))
            fv.set_emission_map(None)
            fv.set_emissions(np.ascontiguousarray(wide[:, pdf]))
            assert_same_runs(got, csr_runs(fv, T, lengths), (name, "expanded"))
            if name == "f64":                                        # exact logs: the oracle's model
                om = oracle.OracleModel(A, np.ascontiguousarray(S[:, pdf].T), Pi)
                try:
                    for N in (1, 4):
                        p, s, _, rc = om.full_decode(np.arange(T, dtype=np.int32), N, check=False)
                        assert vs_oracle(got[(0, N)], (p.tolist(), s, rc)), N
                finally:
                    om.close()
    finally:
        fv.close()


# ---------------------------------------------------------------- 4. row striding

def test_rows_beyond_the_grid_are_strided():
    """T = 300 > 2048 / ceil(2100 / 256) = 227: workgroups take more than one row (and, tied, lanes more than one)."""
    K, T, P = 2100, 300, 64
    assert T > 2048 // ((K + 255) // 256)
    rs = np.random.RandomState(21)
    k = np.arange(K)
    cols = np.sort(np.stack([k, (k + 1) % K, (k * 7 + 3) % K, (k * 13 + 5) % K], axis=1), axis=1)
    indptr, indices, data = [0], [], []
    for r in range(K):
        c = np.unique(cols[r])
        v = rs.uniform(0.05, 1.0, size=c.size)
        indices.extend(c.tolist())
        data.extend((v / v.sum()).tolist())
        indptr.append(len(indices))
    Pi = rs.uniform(0.1, 1.0, size=K).astype(np.float32)
    Pi /= Pi.sum()
    pdf = rs.randint(0, P, size=K).astype(np.int32)
    U = f32_to_bf16_bits(libm_log(free_emissions(T, P, seed=3)).astype(np.float32))
    passes = [(0, 149, -1), (150, T - 1, 11)]
    fv = decoder.FlashViterbi(0)
    try:
        fv.set_model_sparse(np.array(indptr, np.int64), np.array(indices, np.int32), np.array(data, np.float32),
                            np.full((K, 2), 0.5, np.float32), Pi)
        fv.set_emissions(np.ascontiguousarray(bf16_to_f32(U)[:, pdf]))                  # the expanded float32 route
        want = (fv.test_forward(None, passes, -2, T=T)[:2], raw(fv, "full", T, 4), raw(fv, "full", T, 1))
        fv.set_emission_map(pdf, P)
        stage_bits(fv, U, D.EMIS_LOG_BF16, T, P)
        got = (fv.test_forward(None, passes, -2, T=T)[:2], raw(fv, "full", T, 4), raw(fv, "full", T, 1))
        assert got[0][0].tobytes() == want[0][0].tobytes() and got[0][1].tobytes() == want[0][1].tobytes()
        assert eq(got[1], want[1]) and eq(got[2], want[2])
        assert got[1][2] in (0, D.ERR_NO_PRED)
    finally:
        fv.close()


# ---------------------------------------------------------------- 5. values

def test_values_through_the_map():
    fv, A, Pi, K, T = dense_ctx("ds_K77_M7_T33")
    P = K + 5
    rs = np.random.RandomState(9)
    pdf = rs.randint(0, K, size=K).astype(np.int32)                  # classes K .. K + 4 are unmapped
    logS = libm_log(free_emissions(T, P))
    ca = int(pdf[40])
    cb = int(pdf[np.flatnonzero(pdf != ca)[-1]])
    lowest = min(int(np.flatnonzero(pdf == c)[0]) for c in (ca, cb))
    sp = decoder.FlashViterbi(0)
    try:
        fv.set_emission_map(pdf, P)
        fv.set_emissions(logS)
        want = all_runs(fv, T)
        for bad in (np.nan, np.inf):
            for dtype in (np.float64, np.float32, np.float16):
                x = logS.astype(dtype)
                x[:, K:] = bad                                       # unmapped columns: never interpreted
                x[0, K + 1] = np.nan
                fv.set_emissions(x)
                if dtype == np.float64:
                    assert_same_runs(all_runs(fv, T), want, ("unmapped", bad))
                x[20, ca] = bad
                x[5, ca] = bad
                x[5, cb] = bad
                msg = refused(lambda: fv.set_emissions(x), D.ERR_ARG)
                assert re.search(r"t = 5, state = %d\b" % lowest, msg), msg
                assert re.search(r"class = %d\b" % int(pdf[lowest]), msg), msg
                assert fv.stats()["emission_rows"] == 0
                refused(lambda: fv.decode_full(None, 1, T=T), D.ERR_ARG)          # nothing stays staged
        # a binary16 score above 0: FV_KERNEL_F64_STREAM under AUTO, the filter kernels refuse
        h = logS.astype(np.float16)
        h[:, K:] = 0
        fv.set_emissions(h)
        fv.decode_full(None, 4, T=T)
        assert fv.stats()["kernel"] != D.KERNEL_F64_STREAM
        h[3, ca] = np.float16(0.5)
        fv.set_emissions(h)
        assert fv.decode_full(None, 4, T=T)[2] in (0,) and fv.stats()["kernel"] == D.KERNEL_F64_STREAM
        fv.set_option(D.OPT_KERNEL, D.KERNEL_Q16_REFINE)
        refused(lambda: fv.decode_full(None, 4, T=T), D.ERR_UNSUPPORTED)
        fv.set_option(D.OPT_KERNEL, D.KERNEL_AUTO)
        f64_path = raw(fv, "full", T, 4)
        # a CSR-set model: refused unless FV_KERNEL_CSR_F64 is selected
        sp.set_model_sparse(*decoder.dense_to_csr(A), np.full((K, 2), 0.5, np.float32), Pi)
        sp.set_emission_map(pdf, P)
        sp.set_emissions(h)
        refused(lambda: sp.decode_full(None, 4, T=T), D.ERR_UNSUPPORTED)
        sp.set_option(D.OPT_KERNEL, D.KERNEL_CSR_F64)
        assert eq(raw(sp, "full", T, 4), f64_path)
        assert sp.stats()["kernel"] == D.KERNEL_CSR_F64
    finally:
        fv.close()
        sp.close()


# ---------------------------------------------------------------- 6. life cycle and refusals

def test_life_cycle_and_refusals():
    g = golden("ds_K77_M7_T33")
    A, B, Pi, ob = golden_model(g)
    K, T, P = A.shape[0], len(ob), 20
    rs = np.random.RandomState(2)
    pdf = rs.randint(0, P, size=K).astype(np.int32)
    pdf2 = (pdf + 1) % P
    logS = libm_log(free_emissions(T, P))
    fv = decoder.FlashViterbi(0)
    try:
        refused(lambda: fv._check(fv._L.fv_set_emission_map(fv._h, _p(pdf), P)), D.ERR_STATE)      # no model
        fv.set_model(A, B, Pi)
        fv.set_emission_map(pdf, P)
        fv.set_emissions(logS)                                       # ld = P < K is accepted with a map
        want = raw(fv, "full", T, 4)
        refused(lambda: fv.set_emissions((logS.ctypes.data, np.float64, T, P - 1)), D.ERR_ARG)      # ld < P
        refused(lambda: fv.decode_full(None, 4, T=T), D.ERR_ARG)     # (a refused fv_set_emissions leaves nothing staged)
        fv.set_emissions(logS)

        # argument errors of the map call: the previous map and the staged rows stay usable
        def still_usable():
            assert eq(raw(fv, "full", T, 4), want)
            fv.set_emissions(logS)                                   # rows of P scores are still what is read
            assert eq(raw(fv, "full", T, 4), want)
        for entry in (-1, P):
            m = pdf.copy()
            m[50] = entry
            m[31] = entry
            msg = refused(lambda: fv.set_emission_map(m, P), D.ERR_ARG)
            assert re.search(r"state 31\b", msg), msg
            still_usable()
        refused(lambda: fv.set_emission_map(pdf, 0), D.ERR_ARG)      # P = 0 with a map
        still_usable()
        refused(lambda: fv._check(fv._L.fv_set_emission_map(fv._h, None, 3)), D.ERR_ARG)           # no map with P != 0
        still_usable()
        ptr = fv.test_device_alloc(pdf)
        try:
            msg = refused(lambda: fv._check(fv._L.fv_set_emission_map(fv._h, ctypes.c_void_p(ptr), P)), D.ERR_ARG)
            assert "device pointer" in msg
        finally:
            fv.test_device_free(ptr)
        still_usable()
        assert fv.P == P

        # setting, replacing and clearing the map each drop the staged rows
        fv.set_emission_map(pdf2, P)                                 # replaced
        refused(lambda: fv.decode_full(None, 4, T=T), D.ERR_ARG)
        assert fv.stats()["emission_rows"] == 0
        fv.set_emissions(logS)
        other = raw(fv, "full", T, 4)
        fv.set_emission_map(None)                                    # cleared
        assert fv.P == 0
        refused(lambda: fv.decode_full(None, 4, T=T), D.ERR_ARG)
        refused(lambda: fv.set_emissions(logS), D.ERR_ARG)           # no map: ld = P < K again
        fv.set_emissions(np.ascontiguousarray(logS[:, pdf2]))
        assert eq(raw(fv, "full", T, 4), other)
        fv.set_emission_map(pdf, P)                                  # set
        refused(lambda: fv.decode_full(None, 4, T=T), D.ERR_ARG)
        fv.set_emissions(logS)
        assert eq(raw(fv, "full", T, 4), want)

        # the model setters drop the map
        fv.set_model(A, B, Pi)
        assert fv.P == 0
        refused(lambda: fv.set_emissions(logS), D.ERR_ARG)
        fv.set_emission_map(pdf, P)
        fv.set_model_sparse(*decoder.dense_to_csr(A), B, Pi)
        refused(lambda: fv.set_emissions(logS), D.ERR_ARG)
        fv.set_emission_map(pdf, P)
        fv.set_emissions(logS)
        assert eq(raw(fv, "full", T, 4), want)                       # (the CSR walk delivers what the dense kernels do)
        refused(lambda: fv.set_emissions((logS.ctypes.data, 7, T, P)), D.ERR_ARG)                  # dtype 7
        refused(lambda: fv.set_emissions((logS.ctypes.data, -1, T, P)), D.ERR_ARG)
        # the timing hook: the tied form over a T x P device block, the new dtypes, its refusals
        h = logS.astype(np.float16)
        ptr = fv.test_device_alloc(h)
        try:
            assert fv.test_stage_emissions_ms(ptr, np.float16, T, P, 2) > 0
            assert fv.test_stage_emissions_ms(ptr, D.EMIS_LOG_BF16, T, P, 2) > 0
            refused(lambda: fv.test_stage_emissions_ms(ptr, np.float16, T, P - 1, 2), D.ERR_ARG)
            refused(lambda: fv.test_stage_emissions_ms(ptr, 7, T, P, 2), D.ERR_ARG)
            refused(lambda: fv.decode_full(None, 4, T=T), D.ERR_ARG)                               # nothing stays staged
        finally:
            fv.test_device_free(ptr)
    finally:
        fv.close()


@pytest.mark.parametrize("name,ld,dtype", [("ds_K77_M7_T33", 80, np.float32), ("ds_K512_T64", 512, np.float64)])
def test_without_a_map_nothing_changed(name, ld, dtype):
    """test_gpu_emissions.test_device_pointer_and_pitch, on a context whose map was set and cleared"""
    fv, A, Pi, K, T = dense_ctx(name)
    try:
        logE = libm_log(free_emissions(T, K))
        dense = np.ascontiguousarray(logE.astype(dtype))
        padded = np.full((T, ld), np.nan, dtype=dtype)
        padded[:, :K] = dense
        fv.set_emission_map(np.zeros(K, np.int32), 1)
        fv.set_emission_map(None)
        fv.set_emissions(dense)
        want = all_runs(fv, T)
        if dtype == np.float64:
            om = oracle.OracleModel(A, np.ascontiguousarray(free_emissions(T, K).T), Pi)
            try:
                p, s, _, rc = om.full_decode(np.arange(T, dtype=np.int32), 4, check=False)
                assert vs_oracle(want[("full", D.KERNEL_AUTO, 8, 4)], (p.tolist(), s, rc))
            finally:
                om.close()
        fv.clear_emissions()
        fv.set_emissions(padded)
        assert_same_runs(all_runs(fv, T), want, "host pitch")
        fv.clear_emissions()
        ptr = fv.test_device_alloc(padded)
        try:
            fv.set_emissions((ptr, dtype, T, ld))
        finally:
            fv.test_device_free(ptr)
        assert_same_runs(all_runs(fv, T), want, "device")
        refused(lambda: fv.set_emissions((padded.ctypes.data, dtype, T, K - 1)), D.ERR_ARG)        # ld < K
    finally:
        fv.close()


def test_partitions_and_multi_device_context():
    fv, A, Pi, K, T = dense_ctx("ds_K200_T100")
    P, N = 23, 8
    rs = np.random.RandomState(4)
    pdf = rs.randint(0, P, size=K).astype(np.int32)
    U = f32_to_bf16_bits(libm_log(free_emissions(T, P)).astype(np.float32))
    B = np.full((K, 2), 0.5, np.float32)
    try:
        fv.set_emission_map(pdf, P)
        stage_bits(fv, U, D.EMIS_LOG_BF16, T, P)
        want_full, want_beam = raw(fv, "full", T, N), raw(fv, "beam", T, N, 32)
        parts_full, parts_beam = [], []
        for rank in range(3):
            part = decoder.FlashViterbi(0)
            try:
                part.set_model(A, B, Pi)
                part.set_partition(rank, 3)
                part.set_emission_map(pdf, P)
                stage_bits(part, U, D.EMIS_LOG_BF16, T, P)
                parts_full.append(part.decode_full(None, N, T=T)[0])
                parts_beam.append(part.decode_beam(None, N, 32, T=T)[0])
            finally:
                part.close()
        assert decoder.merge_paths(T, N, 3, np.stack(parts_full)).tolist() == want_full[0]
        assert decoder.merge_paths(T, N, 3, np.stack(parts_beam)).tolist() == want_beam[0]
        group = decoder.FlashViterbi([0, 0])
        try:
            group.set_model(A, B, Pi)
            group.set_emission_map(pdf, P)                           # to every member
            stage_bits(group, U, D.EMIS_LOG_BF16, T, P)
            assert eq(raw(group, "full", T, N), want_full) and eq(raw(group, "beam", T, N, 32), want_beam)
            ptr = fv.test_device_alloc(U)                            # a device block: one copy per member
            try:
                group.set_emissions((ptr, D.EMIS_LOG_BF16, T, P))
            finally:
                fv.test_device_free(ptr)
            assert eq(raw(group, "full", T, N), want_full)
            group.set_emission_map(None)
            refused(lambda: group.decode_full(None, N, T=T), D.ERR_ARG)
            group.set_emissions(np.ascontiguousarray(bf16_to_f32(U)[:, pdf]))
            assert eq(raw(group, "full", T, N), want_full)
        finally:
            group.close()
    finally:
        fv.close()


# ---------------------------------------------------------------- 7. torch tensors

TORCH_CHILD = r"""
import json, sys
import numpy as np
import torch                      # first: the library then shares the one HIP runtime torch has loaded
if not torch.cuda.is_available():
    print("NO_GPU")
    sys.exit(0)
sys.path.insert(0, sys.argv[1])
from flash_viterbi_amd import decoder as D

K, T, P = 77, 33, 20
rs = np.random.RandomState(17)
A = rs.uniform(0.01, 1.0, (K, K)).astype(np.float32) * (rs.uniform(size=(K, K)) < 0.4)
A[np.arange(K), np.arange(K)] = 0.5
Pi = rs.uniform(0.1, 1.0, K).astype(np.float32)
pdf = rs.randint(0, P, size=K).astype(np.int32)
logS = np.log(rs.uniform(1e-6, 1.0, (T, P))).astype(np.float32)
logS[rs.uniform(size=(T, P)) < 0.05] = -np.inf
U = (logS.view(np.uint32) >> 16).astype(np.uint16)
H = logS.astype(np.float16)
fv = D.FlashViterbi(0)
fv.set_model(A, np.full((K, 2), 0.5, np.float32), Pi)
fv.set_emission_map(pdf, P)

def runs():
    out = [fv.decode_full(None, 4, T=T), fv.decode_beam(None, 4, 16, T=T), fv.decode_vanilla(None, T=T)]
    rows, bp, _ = fv.test_forward(None, [(0, 11, -1), (12, T - 1, 3)], -2, T=T)
    return [(p.tolist(), float(s), int(rc)) for p, s, rc in out] + [rows.tobytes().hex(), bp.tobytes().hex()]

res = {}
fv.set_emissions((U.ctypes.data, D.EMIS_LOG_BF16, T, P))            # the numpy uint16 route
want_bf16 = runs()
wide = np.full((T, P + 8), 0x7FC0, dtype=np.uint16)                  # NaN beyond column P
wide[:, :P] = U
big = torch.from_numpy(wide.view(np.int16)).view(torch.bfloat16).cuda()
view = big[:, :P]
res["view_is_strided_no_copy"] = (view.data_ptr() == big.data_ptr() and tuple(view.stride()) == (P + 8, 1)
                                  and not view.is_contiguous() and view.dtype == torch.bfloat16 and view.is_cuda)
fv.clear_emissions()
fv.set_emissions(view)
res["bf16_device_tensor_equal"] = runs() == want_bf16
fv.set_emissions(H)                                                  # the np.float16 route
want_f16 = runs()
fv.clear_emissions()
cpu = torch.from_numpy(H.copy())
res["f16_cpu_tensor"] = cpu.dtype == torch.float16 and not cpu.is_cuda
fv.set_emissions(cpu)
res["f16_cpu_tensor_equal"] = runs() == want_f16
for name, bad in (("transposed", big.t()), ("every_other_column", big[:, ::2]), ("int16", torch.zeros(T, P, dtype=torch.int16)),
                  ("one_dim", torch.zeros(P, dtype=torch.float32))):
    try:
        fv.set_emissions(bad)
        res["typeerror_" + name] = False
    except TypeError:
        res["typeerror_" + name] = True
res["still_staged_after_typeerror"] = runs() == want_f16
fv.close()
print("RESULT " + json.dumps(res))
"""


def test_torch_tensors():
    """In a child process of its own: torch's wheel carries its own HIP runtime, which must not be initialised in the
    process the other GPU tests run in.  The child is a fresh interpreter that loads torch and the library only."""
    child = subprocess.run([sys.executable, "-c", TORCH_CHILD, ROOT], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert child.returncode == 0, child.stderr[-3000:]
    if child.stdout.strip().endswith("NO_GPU"):
        pytest.skip("torch.cuda.is_available() is false")
    line = next(ln for ln in child.stdout.splitlines() if ln.startswith("RESULT "))
    res = json.loads(line[len("RESULT "):])
    assert len(res) == 9 and all(res.values()), res
