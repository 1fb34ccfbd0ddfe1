"""GPU: what a context holds after its setters — model, emission map, staged score rows — and what it says when one of them
refuses: return codes, the exact sentences, and the state left behind.

The expected sentences and the RECORDED statistics were taken from the library as it stood before this layer was given
one staging path, one member loop and one "nothing is staged" rule; the file passes against that library and against this
one.  Every shape is tiny (K <= 130, T <= 16).

Asserted elsewhere and not repeated here: decodes on staged rows against the goldens (test_gpu_emissions.py), every input
form and pitch of a block (test_gpu_emissions.py, test_gpu_emissions_tied.py), every chunking of a stream and the
substring forms of its refusals (test_gpu_stream.py: test_refused_score_pushes_leave_the_stream_usable), device_bytes
against the buffer sizes (test_gpu_device_bytes.py), multi-device decodes of symbols (test_gpu_multi_device.py)."""
import numpy as np
import pytest

import oracle
from flash_viterbi_amd import decoder
from test_gpu_emissions import libm_log
from modelgen import plain_model as make_model

pytestmark = pytest.mark.gpu

D = decoder
T = 16
NOT_STAGED = "ob == NULL: no emission scores are staged (fv_set_emissions)"
BAD_SCORE = " is NaN, +inf or beyond the float32 range; scores are finite or -inf"
SET_EMIS_ARGS = ("fv_set_emissions: scores != NULL, T >= 1, ld >= K (ld >= P while an emission map is set) and dtype "
                 "FV_EMIS_LOG_F32, _F64, _F16 or _BF16")
DENSE_RANGE = "the filter+refine kernels need every model entry in [0,1] (and every staged emission score <= 0)"
CSR_RANGE = ("fv_set_model_sparse: the walk over the stored entries is a filter kernel and needs every model entry in [0,1] "
             "(and every staged emission score <= 0); FV_KERNEL_CSR_F64 decodes such input")


def refusal(call):
    """(rc, detail) of a call that must raise"""
    with pytest.raises(D.FlashVitError) as e:
        call()
    return e.value.rc, str(e.value).split("): ", 1)[1] if "): " in str(e.value) else ""


def bits(x):
    return int(np.float32(x).view(np.uint32))


def model(K, seed=3):
    """a model of density 0.6 with entries in [0, 1) and T symbols"""
    A, B, Pi = make_model(K, 4, 0.6, seed=seed)
    ob = np.random.default_rng(seed).integers(0, 4, T).astype(np.int32)
    return A, B, Pi, ob


def scores(K, width=None, seed=5):
    """E[T][width] in (0.05, 1) and its float64 logs by the host libm"""
    E = np.random.default_rng(seed).uniform(0.05, 1.0, (T, width or K)).astype(np.float32)
    return E, libm_log(E)


def oracle_full(A, B, Pi, ob, n_split):
    om = oracle.OracleModel(A, B, Pi)
    try:
        path, score, _, _ = om.full_decode(ob, n_split)
        return path.tolist(), bits(score)
    finally:
        om.close()


def decoded(fv, ob, n_split, **kw):
    path, score, rc = fv.decode_full(ob, n_split, D.MODE_REFERENCE, **kw)
    assert rc == 0
    return path.tolist(), bits(score)


@pytest.fixture
def fv():
    f = D.FlashViterbi(0)
    yield f
    f.close()


# ---------------------------------------------------------------- a refused model setter

@pytest.mark.parametrize("sparse_refusal", [False, True])
def test_refused_set_model_keeps_the_model_before_it(fv, sparse_refusal):
    """Both setters build and check on the host before any device is touched, so a refusal of the VALUES (all a caller can
    provoke) returns before drop_model: the library as recorded keeps the earlier model and decodes it as before.  "No
    model" (ERR_STATE) is the state between drop_model and the last upload, reached only when an upload itself fails
    (an allocation refused by the device), which no test provokes."""
    A, B, Pi, ob = model(37)
    fv.set_model(A, B, Pi)
    assert decoded(fv, ob, 2) == oracle_full(A, B, Pi, ob, 2)
    bad = A.copy()
    bad[4, 1] = np.nan
    if sparse_refusal:
        assert refusal(lambda: fv.set_model_sparse(*D.dense_to_csr(bad), B, Pi)) == (D.ERR_ARG, "model entries must be finite and >= 0 (row 4)")
    else:
        assert refusal(lambda: fv.set_model(bad, B, Pi)) == (D.ERR_ARG, "model entries must be finite and >= 0")
    assert decoded(fv, ob, 2) == oracle_full(A, B, Pi, ob, 2)
    empty = D.FlashViterbi(0)                          # ... and a context that never had one still has none
    try:
        assert refusal(lambda: empty.set_model(bad, B, Pi))[0] == D.ERR_ARG
        assert refusal(lambda: empty.decode_full(ob, 2))[0] == D.ERR_STATE
    finally:
        empty.close()
    # a larger model afterwards: every table grows
    A2, B2, Pi2, ob2 = model(130, seed=4)
    if sparse_refusal:
        fv.set_model_sparse(*D.dense_to_csr(A2), B2, Pi2)
    else:
        fv.set_model(A2, B2, Pi2)
    assert decoded(fv, ob2, 4) == oracle_full(A2, B2, Pi2, ob2, 4)


# ---------------------------------------------------------------- fv_set_emissions

def nothing_staged(fv):
    st = fv.stats()
    return (refusal(lambda: fv.decode_full(None, 1, T=T)), st["emission_rows"], st["set_emissions_ms"]) == ((D.ERR_ARG, NOT_STAGED), 0, 0.0)


def test_set_emissions_argument_refusals(fv):
    K, P = 37, 7
    _, logs = scores(K)
    block = np.ascontiguousarray(logs, dtype=np.float32)
    assert refusal(lambda: fv.set_emissions(block)) == (D.ERR_STATE, "fv_set_emissions: no model (the row length K is the model's)")
    A, B, Pi, _ = model(K)
    fv.set_model(A, B, Pi)
    ptr = block.ctypes.data
    for form in ((ptr, D.EMIS_LOG_F32, T, K - 1), (ptr, 7, T, K), (ptr, D.EMIS_LOG_F32, 0, K)):
        fv.set_emissions(block)                         # something is staged: the refusal drops it
        assert fv.stats()["emission_rows"] == T
        assert refusal(lambda: fv.set_emissions(form)) == (D.ERR_ARG, SET_EMIS_ARGS), form
        assert nothing_staged(fv), form
    fv.set_emission_map((np.arange(K) * 3 + 1) % P, P)
    assert refusal(lambda: fv.set_emissions((ptr, D.EMIS_LOG_F32, T, P - 1))) == (D.ERR_ARG, SET_EMIS_ARGS)
    assert nothing_staged(fv)
    fv.set_emissions((ptr, D.EMIS_LOG_F32, T, P))       # ld >= P is enough with a map
    assert fv.stats()["emission_rows"] == T


@pytest.mark.parametrize("tied", [False, True])
@pytest.mark.parametrize("form", ["f32", "f64", "f16", "device"])
def test_set_emissions_value_refusal_names_the_lowest_index(fv, form, tied):
    K, P = 37, 7
    A, B, Pi, _ = model(K)
    fv.set_model(A, B, Pi)
    pdf = ((np.arange(K) * 3 + 1) % P).astype(np.int32)          # class 6: states 4, 11, 18, ...
    if tied:
        fv.set_emission_map(pdf, P)
    _, logs = scores(K, P if tied else K)
    good = logs.astype({"f64": np.float64, "f16": np.float16}.get(form, np.float32))
    bad = good.copy()
    bad[3, 6 if tied else 4] = np.nan
    bad[3, 2 if tied else 9] = np.inf                  # a higher index of the same row (tied: class 2 is first used by state 5)
    bad[5, 1] = np.inf                                 # ... and one of a later row
    want = "fv_set_emissions: the score at (t = 3, state = 4" + (", class = 6" if tied else "") + ")" + BAD_SCORE
    fv.set_emissions(good)
    assert fv.stats()["emission_rows"] == T and fv.stats()["set_emissions_ms"] > 0
    ptr = fv.test_device_alloc(bad) if form == "device" else None
    try:
        arg = (ptr, D.EMIS_LOG_F32, T, bad.shape[1]) if form == "device" else bad
        assert refusal(lambda: fv.set_emissions(arg)) == (D.ERR_ARG, want)
    finally:
        if ptr:
            fv.test_device_free(ptr)
    assert nothing_staged(fv)


# ---------------------------------------------------------------- fv_set_emission_map

def test_emission_map_refusals_keep_map_and_rows_and_clearing_drops_the_rows(fv):
    K, P = 37, 7
    A, B, Pi, _ = model(K)
    E, logs = scores(K, P)
    pdf = ((np.arange(K) * 3 + 1) % P).astype(np.int32)
    fv.set_model(A, B, Pi)
    fv.set_emission_map(pdf, P)
    fv.set_emissions(logs)
    want = oracle_full(A, np.ascontiguousarray(E[:, pdf].T), Pi, np.arange(T, dtype=np.int32), 2)
    assert decoded(fv, None, 2, T=T) == want
    ms = fv.stats()["set_emissions_ms"]

    def raw(ptr, classes):
        rc = fv._L.fv_set_emission_map(fv._h, ptr, classes)
        return rc, fv._L.fv_last_error_detail(fv._h).decode()
    outside = pdf.copy()
    outside[5] = 9
    who = "fv_set_emission_map: "
    assert raw(outside.ctypes.data, P) == (D.ERR_ARG, who + "pdf_of_state[5] = 9 (state 5) lies outside [0, P = 7)")
    outside[5] = -1
    assert raw(outside.ctypes.data, P) == (D.ERR_ARG, who + "pdf_of_state[5] = -1 (state 5) lies outside [0, P = 7)")
    assert raw(pdf.ctypes.data, 0) == (D.ERR_ARG, who + "P >= 1 score classes with a map")
    assert raw(None, 3) == (D.ERR_ARG, who + "pdf_of_state == NULL clears the map and takes P == 0")
    # map and rows are as they were: the same decode, and a block of P scores per row is still what is taken
    assert decoded(fv, None, 2, T=T) == want
    fv.set_emissions(logs)
    assert fv.stats()["emission_rows"] == T and ms > 0
    assert refusal(lambda: fv.set_emissions((logs.ctypes.data, D.EMIS_LOG_F64, T, P - 1))) == (D.ERR_ARG, SET_EMIS_ARGS)
    fv.set_emissions(logs)
    fv.set_emission_map(None)                          # clearing: the rows went through the map that is gone
    assert nothing_staged(fv)
    assert refusal(lambda: fv.set_emissions((logs.ctypes.data, D.EMIS_LOG_F64, T, P))) == (D.ERR_ARG, SET_EMIS_ARGS)      # rows of K again
    fresh = D.FlashViterbi(0)
    try:
        rc = fresh._L.fv_set_emission_map(fresh._h, pdf.ctypes.data, P)
        assert (rc, fresh._L.fv_last_error_detail(fresh._h).decode()) == \
            (D.ERR_STATE, who + "no model (the map holds one entry per state of the model)")
    finally:
        fresh.close()


# ---------------------------------------------------------------- a stream's pushes of score rows

@pytest.mark.parametrize("sparse", [False, True])
def test_stream_score_pushes_refused_and_taken(sparse):
    K = 37
    A, B, Pi, _ = model(K)
    _, logs = scores(K)
    block = np.ascontiguousarray(logs, dtype=np.float32)
    pair = (D.FlashViterbi(0), D.FlashViterbi(0))
    try:
        for f in pair:
            if sparse:
                f.set_model_sparse(*D.dense_to_csr(A), B, Pi)
            else:
                f.set_model(A, B, Pi)
        fv, ref = pair
        ref.set_emissions(block)
        path, score, rc = ref.decode_full(None, 1, D.MODE_SINGLE_PASS, T=T)
        fv.stream_open(0, 4)
        pieces = [fv.stream_push(scores=block[:5]).tolist()]
        pending = fv.stream_pending()
        rows = block[5:9].copy()
        rows[2, 8] = np.nan
        rows[3, 0] = np.inf
        assert refusal(lambda: fv.stream_push(scores=rows)) == \
            (D.ERR_ARG, "fv_stream_push_emissions: the score at (t = 7, state = 8)" + BAD_SCORE)
        assert fv.stream_pending() == pending and fv.stream_stats()["times"] == 5
        rows = block[5:9].copy()
        rows[1, 2] = 0.25                              # above 0 under a filter kernel
        assert refusal(lambda: fv.stream_push(scores=rows)) == (D.ERR_UNSUPPORTED, CSR_RANGE if sparse else DENSE_RANGE)
        assert fv.stream_pending() == pending and fv.stream_stats()["times"] == 5
        assert refusal(lambda: fv.stream_push(scores=(block.ctypes.data, D.EMIS_LOG_F32, 3, K - 1))) == \
            (D.ERR_ARG, "fv_stream_push_emissions: ld >= K (ld >= P while an emission map is set) and dtype FV_EMIS_LOG_F32, _F64, _F16 or _BF16")
        pieces.append(fv.stream_push(scores=block[5:9]).tolist())
        pieces.append(fv.stream_push(scores=block[9:]).tolist())
        last, got_score, got_rc = fv.stream_close()
        pieces.append(last.tolist())
        assert ([x for p in pieces for x in p], bits(got_score), got_rc) == (path.tolist(), bits(score), rc)
    finally:
        for f in pair:
            f.close()


# ---------------------------------------------------------------- a two-member context on one GPU

def test_two_members_on_one_gpu_follow_every_setter():
    K, P = 130, 11
    A, B, Pi, _ = model(K, seed=6)
    E, logs = scores(K, P)
    pdf = ((np.arange(K) * 5 + 2) % P).astype(np.int32)
    one, two = D.FlashViterbi(0), D.FlashViterbi([0, 0])
    try:
        for f in (one, two):
            f.set_model(A, B, Pi)
            f.set_emission_map(pdf, P)
            f.set_emissions(logs)                      # a host block: every member takes its copy
            f.set_option(D.OPT_KERNEL, D.KERNEL_F32_REFINE)
        want = oracle_full(A, np.ascontiguousarray(E[:, pdf].T), Pi, np.arange(T, dtype=np.int32), 4)
        assert decoded(one, None, 4, T=T) == want
        assert decoded(two, None, 4, T=T) == want
        assert (two.stats()["kernel"], two.stats()["ranks"], two.stats()["emission_rows"]) == (D.KERNEL_F32_REFINE, 2, T)
        # an option a member refuses is refused for the context
        assert refusal(lambda: two.set_option(D.OPT_MAX_BATCH, 0))[0] == D.ERR_ARG
        two.clear_emissions()
        assert refusal(lambda: two.decode_full(None, 4, T=T)) == (D.ERR_ARG, NOT_STAGED)
        assert two.stats()["emission_rows"] == 0
        # the map outlives the rows: a block of P scores per row is staged again, on both members
        two.set_emissions(logs)
        assert decoded(two, None, 4, T=T) == want
    finally:
        one.close()
        two.close()


# ---------------------------------------------------------------- statistics after each setter

def setter_stats(K):
    """(density, device_bytes) after each setter of a fresh context, in the order they are called"""
    A, B, Pi, _ = model(K)
    _, logs = scores(K, 7)
    pdf = ((np.arange(K) * 3 + 1) % 7).astype(np.int32)
    fv = D.FlashViterbi(0)
    out = []

    def note(what):
        st = fv.stats()
        out.append((what, float(st["density"]).hex(), int(st["device_bytes"])))
    try:
        fv.set_model(A, B, Pi); note("set_model")
        fv.set_emission_map(pdf, 7); note("set_emission_map")
        fv.set_emissions(logs); note("set_emissions")
        fv.set_emissions(np.ascontiguousarray(logs[:5], dtype=np.float16)); note("set_emissions, fewer rows")
        bad = logs.copy()
        bad[2, 3] = np.nan
        refusal(lambda: fv.set_emissions(bad)); note("set_emissions refused")
        fv.clear_emissions(); note("clear_emissions")
        fv.set_model_sparse(*D.dense_to_csr(A), B, Pi); note("set_model_sparse")
        fv.set_emissions(np.ascontiguousarray(logs[:, pdf])); note("set_emissions after set_model_sparse")
        fv.set_model(A, B, Pi); note("set_model again")
    finally:
        fv.close()
    return out


RECORDED = {
    37: [
        ('set_model', '0x0.0p+0', 57392),
        ('set_emission_map', '0x0.0p+0', 57540),
        ('set_emissions', '0x0.0p+0', 64660),
        ('set_emissions, fewer rows', '0x0.0p+0', 64660),
        ('set_emissions refused', '0x0.0p+0', 64660),
        ('clear_emissions', '0x0.0p+0', 57556),
        ('set_model_sparse', '0x1.2a1312e303ed5p-1', 33496),
        ('set_emissions after set_model_sparse', '0x1.2a1312e303ed5p-1', 40600),
        ('set_model again', '0x0.0p+0', 64512),
    ],
    130: [
        ('set_model', '0x0.0p+0', 431288),
        ('set_emission_map', '0x0.0p+0', 431808),
        ('set_emissions', '0x0.0p+0', 456784),
        ('set_emissions, fewer rows', '0x0.0p+0', 456784),
        ('set_emissions refused', '0x0.0p+0', 456784),
        ('clear_emissions', '0x0.0p+0', 431824),
        ('set_model_sparse', '0x1.3478f0e9a443ap-1', 324172),
        ('set_emissions after set_model_sparse', '0x1.3478f0e9a443ap-1', 349132),
        ('set_model again', '0x0.0p+0', 456264),
    ],
}


@pytest.mark.parametrize("K", [37, 130])
def test_density_and_device_bytes_after_each_setter(K):
    assert setter_stats(K) == RECORDED[K]
