"""GPU: fv_loglik / fv_loglik_batch / fv_posteriors on models set by fv_set_model_sparse under fv_set_sparse_sumprod, against
the float64 CPU model (tests/sumprod_model.py on the dense form of the same transitions) within the bound of guarantee 1, in
both score-row forms (staged in LDS, and read from memory under FV_OPT_DEBUG bit 31 or beyond one LDS row): the flush
models, the bit equalities of guarantee 3 extended to the row form and to stored zeros, probability 0, values outside
[0, 1], one K beyond 20192, the switch itself, and the context left as it was.

Shapes: K = 5 (less than one tile), 37 (pads), 64 and 333 (a column of in-degree K, columns without an in-edge, rows without
an out-edge), 1030 (65 tiles, 17 workgroups of the backward walk, rows of more than 16 entries), once K = 21120."""
import ctypes
import math
import time

import numpy as np
import pytest

import sumprod_model as sp
from flash_viterbi_amd import decoder
from test_gpu_sparse_model import csr_to_dense, dead_end_model, interleaved_blocks, structured_model
from test_gpu_sumprod import bits, check_rows, device_read, live_bytes, model, observations, refused, scores, stats_state

pytestmark = pytest.mark.gpu

D = decoder
MEM = D.DEBUG_CSR_ROWS_IN_MEMORY
FORMS = {"dense": D.spf_family(D.SPF_DENSE_SHIFT),
         ("fwd", 0): D.spf_family(D.SPF_CSR_FWD_LDS_SHIFT), ("fwd", MEM): D.spf_family(D.SPF_CSR_FWD_MEM_SHIFT),
         ("back", 0): D.spf_family(D.SPF_CSR_BACK_LDS_SHIFT), ("back", MEM): D.spf_family(D.SPF_CSR_BACK_MEM_SHIFT)}
UNSUPPORTED_DETAIL = "models set by fv_set_model_sparse are not supported"


def sparse_ctx(csr, B, Pi, on=1, debug=0):
    fv = D.FlashViterbi(0)
    fv.set_model_sparse(*csr, B, Pi)
    if on is not None:
        fv.set_sparse_sumprod(on)
    fv.set_option(D.OPT_DEBUG, debug)
    return fv


def named(name):
    """(A, B, Pi, ob or None) of the models of case 1"""
    if name.startswith("structured"):
        K = int(name[len("structured"):])
        return structured_model(K, 900 + K)
    return model(name) + (None,)


_truth = {}


def truth(key, A, Pi, e):
    """sumprod_model.run, once per key"""
    if key not in _truth:
        K = A.shape[0]
        back = csr_to_dense(*D.dense_to_csr(A), K)           # (the transitions as the sparse setter receives them)
        assert back.tobytes() == np.ascontiguousarray(A, dtype=np.float32).tobytes()
        _truth[key] = sp.run(back, Pi, e)
    return _truth[key]


def expect_forms(fv, T, debug, passes=2):
    """the hook: CSR kernels of the row form `debug` selects, forward (and backward), and no other step kernel"""
    mask = fv.test_sumprod_forms()
    allowed = FORMS[("fwd", debug)] | (FORMS[("back", debug)] if passes == 2 else 0)
    assert mask & ~allowed == 0 and mask & FORMS["dense"] == 0, hex(mask)
    if T > 1:
        assert mask & FORMS[("fwd", debug)] and (passes == 1 or mask & FORMS[("back", debug)]), hex(mask)
    else:
        assert mask == 0


def check_call(fv, r, K, ob, T, tag, debug):
    """test_gpu_sumprod.check_call's checks of the hook's rows, loglik, gamma and path against the model's run r, and the
    forms hook after each call"""
    a_max = sp.amax(r)
    ta, tb = sp.tol_rows(T, K, a_max)
    tol = sp.tol_alpha(T - 1, K, a_max)
    tt = None if ob is not None else T
    alpha, beta, rc = fv.test_sumprod_rows(ob, T=tt)
    expect_forms(fv, T, debug)
    check_rows(alpha, r["alpha"], ta, tag + " alpha")
    check_rows(beta, r["beta"], tb, tag + " beta")
    gamma, path, ll = fv.posteriors(ob, T=tt)
    expect_forms(fv, T, debug)
    assert math.isfinite(r["loglik"]) and rc == 0, tag
    print(f"{tag}: loglik {ll!r} model {r['loglik']!r} bound {tol:.3e}")
    assert abs(ll - r["loglik"]) <= tol, tag
    assert fv.loglik(ob, T=tt) == ll, tag
    expect_forms(fv, T, debug, passes=1)
    assert gamma.dtype == np.float32 and gamma.shape == (T, K)
    assert np.abs(gamma.astype(np.float64) - r["gamma"]).max() <= 2.0 ** -23 + 3 * tol, tag
    assert (gamma[r["gamma"] == 0] == 0).all(), tag
    assert np.abs(gamma.astype(np.float64).sum(axis=1) - 1.0).max() <= K * 2.0 ** -24 + 3 * tol, tag
    ab = r["ab"]
    best = ab.max(axis=1)
    assert (ab[np.arange(T), path] >= best - 2 * tol).all(), tag
    second = np.sort(ab, axis=1)[:, -2] if K > 1 else np.full(T, -np.inf)
    clear = best - second > 2 * tol
    assert (path[clear] == r["path"][clear]).all(), tag
    return ll, alpha, beta


@pytest.fixture(scope="module")
def ctx():
    made = {}

    def get(name, debug=0):
        if name not in made:
            A, B, Pi = named(name)[:3]
            made[name] = sparse_ctx(D.dense_to_csr(A), B, Pi)
        fv = made[name]
        fv.set_option(D.OPT_MAX_BATCH, 8)
        fv.set_option(D.OPT_DEBUG, debug)
        return fv
    yield get
    for fv in made.values():
        fv.close()


# ---------------------------------------------------------------- 1. against the CPU model

CASES = [("ds_K5_T3", 1), ("ds_K5_T3", 2), ("ds_K5_T3", 3), ("plain37", 1), ("plain37", 3), ("plain37", 40),
         ("structured64", 2), ("structured64", 40), ("structured333", 3), ("structured333", 40), ("plain1030", 12)]


@pytest.mark.parametrize("debug", [0, MEM], ids=["lds", "mem"])
@pytest.mark.parametrize("name,T", CASES)
def test_symbols_against_the_model(ctx, name, T, debug):
    A, B, Pi, ob = named(name)
    K = A.shape[0]
    if name.startswith("structured"):
        assert np.count_nonzero(A[:, 3]) == K and not A[:, 5].any() and np.count_nonzero(A[12]) == 1
    ob = observations(B.shape[1], T, 100 + T) if ob is None else ob[:T]
    r = truth((name, T), A, Pi, sp.emission_rows(B, ob))
    fv = ctx(name, debug)
    check_call(fv, r, K, ob, T, f"{name} T={T} debug={debug:#x}", debug)
    st = fv.sumprod_stats()
    assert st["passes"] == 1 and st["step_launches"] == T - 1 == st["task_steps"]      # (the last call was loglik; scale launches do not count)
    # 8 bytes per padded entry of the CSC-32 table: per tile its longest column rounded up to 16, times 16 columns
    indeg = np.zeros((K + 15) // 16 * 16, dtype=np.int64)
    indeg[:K] = np.count_nonzero(A, axis=0)
    assert st["table_bytes_per_step"] == 8 * 16 * int(((indeg.reshape(-1, 16).max(axis=1) + 15) // 16 * 16).sum())


# ---------------------------------------------------------------- 2. the flush models

@pytest.mark.parametrize("debug", [0, MEM], ids=["lds", "mem"])
@pytest.mark.parametrize("which", ["forward", "backward"])
def test_flush_models_come_out_finite(which, debug):
    A, B, Pi, e = sp.flush_forward() if which == "forward" else sp.flush_backward()
    fv = sparse_ctx(D.dense_to_csr(A), B, Pi, debug=debug)
    try:
        fv.set_emissions(e)
        r = truth(("flush", which), A, Pi, e)
        ll, _, _ = check_call(fv, r, A.shape[0], None, sp.FLUSH_T, f"flush {which} debug={debug:#x}", debug)
        assert math.isfinite(ll)
        forward_only = fv.sumprod_stats()["refine_finite"]          # (the last call, fv_loglik: the forward pass alone)
        gamma, path, _ = fv.posteriors(None, T=sp.FLUSH_T)
        st = fv.sumprod_stats()
        if which == "forward":
            assert forward_only >= 1
            assert gamma[2, 36] == 1 and gamma[3, 35] == 1 and (path[2], path[3]) == (36, 35)
        else:
            assert st["passes"] == 2 and st["refine_finite"] - forward_only >= 1      # the backward pass's own
            assert gamma[sp.FLUSH_T - 3, 36] == 1 and gamma[sp.FLUSH_T - 4, 35] == 1
        assert st["refine_columns"] >= st["refine_finite"]
    finally:
        fv.close()


# ---------------------------------------------------------------- 3. bits

@pytest.mark.parametrize("name", ["plain37", "plain1030", "structured333"])
def test_bits_do_not_depend_on_the_launch_form(ctx, name):
    A, B, Pi = named(name)[:3]
    M = B.shape[1]
    lengths = [1, 9, 3, 7, 2, 5, 4]
    obs = [observations(M, n, 40 + i) for i, n in enumerate(lengths)]
    got = {}
    for debug in (0, MEM):
        fv = ctx(name, debug)
        single = [fv.loglik(o) for o in obs]
        assert all(math.isfinite(x) for x in single)
        assert bits(single) == bits([fv.loglik(o) for o in obs])                 # the same call twice
        for cap in (1, 2, 4, 8):
            fv.set_option(D.OPT_MAX_BATCH, cap)
            ll, status = fv.loglik_batch(obs)
            assert bits(ll) == bits(single), (debug, cap)
            assert status.tolist() == [0] * len(obs)
            st = fv.sumprod_stats()
            assert st["batch_cap"] == min(cap, 4) and st["task_steps"] == sum(n - 1 for n in lengths)
            if cap == 1:
                assert st["step_launches"] == st["task_steps"]
            expect_forms(fv, 9, debug, passes=1)
        fv.set_option(D.OPT_MAX_BATCH, 8)
        ll, _ = fv.loglik_batch(obs[::-1])                                        # another grouping of the same sequences
        assert bits(ll) == bits(single[::-1])
        alpha, beta, _ = fv.test_sumprod_rows(obs[1])
        gamma, path, pll = fv.posteriors(obs[1])
        assert bits(pll) == bits(single[1])                                       # fv_posteriors' loglik has fv_loglik's bits
        got[debug] = (single, alpha, beta, gamma, path)
    # the LDS form and the memory form: loglik, every alpha and beta, gamma and the path
    assert bits(got[0][0]) == bits(got[MEM][0])
    for q in (1, 2, 3):
        assert got[0][q].tobytes() == got[MEM][q].tobytes()
    assert got[0][4].tolist() == got[MEM][4].tolist()


# ---------------------------------------------------------------- 4. stored zeros equal absent entries

def with_stored_zeros(A, seed):
    """the CSR form of A with entries equal to 0 stored at a fifth of the absent places, and the whole of row 1 stored"""
    rng = np.random.default_rng(seed)
    stored = (A != 0) | (rng.random(A.shape) < 0.2)
    stored[1] = True
    rows, cols = np.nonzero(stored)
    indptr = np.zeros(A.shape[0] + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=A.shape[0]), out=indptr[1:])
    data = np.ascontiguousarray(A[rows, cols], dtype=np.float32)
    assert (data == 0).sum() > A.shape[0]
    return indptr, cols.astype(np.int32), data


@pytest.mark.parametrize("name,T", [("plain37", 9), ("plain1030", 4), ("structured333", 5)])
def test_stored_zeros_equal_absent_entries(ctx, name, T):
    A, B, Pi = named(name)[:3]
    ob = observations(B.shape[1], T, 5)
    zeros = sparse_ctx(with_stored_zeros(A, 77), B, Pi)
    try:
        for debug in (0, MEM):
            plain = ctx(name, debug)
            zeros.set_option(D.OPT_DEBUG, debug)
            assert bits(zeros.loglik(ob)) == bits(plain.loglik(ob))
            a0, b0, _ = plain.test_sumprod_rows(ob)
            a1, b1, _ = zeros.test_sumprod_rows(ob)
            assert a0.tobytes() == a1.tobytes() and b0.tobytes() == b1.tobytes(), debug
            assert zeros.sumprod_stats()["table_bytes_per_step"] == plain.sumprod_stats()["table_bytes_per_step"]
    finally:
        zeros.close()


# ---------------------------------------------------------------- 5. probability 0

@pytest.mark.parametrize("debug", [0, MEM], ids=["lds", "mem"])
def test_probability_zero(debug):
    A, Bm, Pi = dead_end_model()
    K = A.shape[0]
    bad = np.array([0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0], np.int32)
    good = [np.zeros(n, np.int32) for n in (5, 1, 8)]
    fv = sparse_ctx(D.dense_to_csr(A), Bm, Pi, debug=debug)
    try:
        assert truth("dead", A, Pi, sp.emission_rows(Bm, bad))["loglik"] == -math.inf
        single = [fv.loglik(o) for o in good]
        r = truth("alive", A, Pi, sp.emission_rows(Bm, good[2]))
        assert abs(single[2] - r["loglik"]) <= sp.tol_alpha(7, K, sp.amax(r))
        assert fv.loglik(bad) == -math.inf
        out = ctypes.c_double(0)
        assert fv._L.fv_loglik(fv._h, decoder._p(bad), bad.size, ctypes.byref(out)) == D.ERR_NO_PRED
        gamma = np.full((bad.size, K), 7.0, dtype=np.float32)
        path = np.zeros(bad.size, dtype=np.int32)
        assert fv._L.fv_posteriors(fv._h, decoder._p(bad), bad.size, decoder._p(gamma), K, decoder._p(path), ctypes.byref(out)) == D.ERR_NO_PRED
        assert out.value == -math.inf and (path == -1).all() and (gamma == 7.0).all()      # gamma_out is not written
        ll, status = fv.loglik_batch([good[0], good[1], bad, good[2]])
        assert status.tolist() == [0, 0, D.ERR_NO_PRED, 0]
        assert ll[2] == -math.inf and bits(np.delete(ll, 2)) == bits(single)
    finally:
        fv.close()


# ---------------------------------------------------------------- 6. values outside [0, 1], emission forms, gamma on the device

@pytest.mark.parametrize("debug", [0, MEM], ids=["lds", "mem"])
def test_entries_above_one_scores_above_zero_and_the_emission_forms(debug):
    name, T = "structured333", 12
    A, B, Pi, ob = named(name)
    K = A.shape[0]
    rng = np.random.default_rng(3)
    A = A.copy()
    rows, cols = np.nonzero(A)
    pick = rng.random(rows.size) < 0.01
    A[rows[pick], cols[pick]] = (1 + 49 * (1 - rng.random(int(pick.sum())))).astype(np.float32)
    assert pick.sum() >= 10 and A.max() > 1 and A.max() <= 50
    fv = sparse_ctx(D.dense_to_csr(A), B, Pi, debug=debug)
    try:
        check_call(fv, truth("big symbols", A, Pi, sp.emission_rows(B, ob[:T])), K, ob[:T], T, "entries above 1", debug)
        x = rng.random((T, K)) * 4 - 1                # emission scores in [-1, 3)
        assert x.max() > 0
        fv.set_emissions(x)
        check_call(fv, truth("big scores", A, Pi, x), K, None, T, "scores above 0", debug)
        for dtype in (np.float32, np.float64):
            y = scores(T, K, 7 * T, dtype)
            y[0, 0] = 0.0                   # (a live start, whatever the draw)
            fv.set_emissions(y)
            check_call(fv, truth(("staged", np.dtype(dtype).name), A, Pi, y.astype(np.float64)), K, None, T, f"staged {np.dtype(dtype).name}", debug)
        # an emission map with P < K
        P = 23
        pdf = (np.arange(K) * 7 % P).astype(np.int32)
        z = scores(3, P, 5, np.float32)
        z[:, 0] = -1.0
        fv.set_emission_map(pdf, P)
        try:
            fv.set_emissions(z)
            check_call(fv, truth("tied", A, Pi, z.astype(np.float64)[:, pdf]), K, None, 3, "tied", debug)
        finally:
            fv.set_emission_map(None)
        # a device gamma_out at ld = K + 3: the host result's bytes, pads untouched
        host, hpath, hll = fv.posteriors(ob[:T])
        ld = K + 3
        dev = fv.test_device_alloc(np.full((T, ld), 9.0, dtype=np.float32))
        try:
            gamma, path, ll = fv.posteriors(ob[:T], out=(dev, ld))
            assert gamma is None and path.tolist() == hpath.tolist() and bits(ll) == bits(hll)
            back = device_read(dev, T * ld * 4).view(np.float32).reshape(T, ld)
            assert back[:, :K].tobytes() == host.tobytes() and (back[:, K:] == 9.0).all()
        finally:
            fv.test_device_free(dev)
    finally:
        fv.close()


# ---------------------------------------------------------------- 7. beyond one LDS row, no debug bit

BIG_BLOCKS, BIG_KB, BIG_M, BIG_T, BIG_SEED = 22, 960, 5, 6, 31       # (the 22 block models cost the CPU model about 4 s)


def test_beyond_one_lds_row():
    """K = 22 * 960 = 21120 > 20192: the blocks exchange nothing, so alpha and beta are the blocks' own, loglik is the
    log-sum-exp of the blocks' logliks and gamma[t, s * 22 + b] = gamma_b[t, s] * exp(ll_b - ll)."""
    nb, Kb, T = BIG_BLOCKS, BIG_KB, BIG_T
    K = nb * Kb
    assert K > 20192
    (ip, ix, dt, Bm, Pi), blocks = interleaved_blocks(nb, Kb, BIG_M, BIG_SEED, degree=8)
    ob = observations(BIG_M, T, 12)
    t0 = time.time()
    alpha, beta, gam = np.empty((T, K)), np.empty((T, K)), np.empty((T, K))
    lls = []
    for b, (bip, bix, bdt, Bb, Pib) in enumerate(blocks):
        r = sp.run(csr_to_dense(bip, bix, bdt, Kb), Pib, sp.emission_rows(Bb, ob))
        alpha[:, b::nb], beta[:, b::nb], gam[:, b::nb] = r["alpha"], r["beta"], r["gamma"]
        lls.append(r["loglik"])
    lls = np.array(lls)
    want = sp.lse(lls)
    gam *= np.exp(np.tile(lls, Kb) - want)[None, :]             # column s * nb + b belongs to block b
    print(f"K={K}: the {nb} block models took {time.time() - t0:.1f}s on the CPU")
    both = np.concatenate([alpha.reshape(-1), beta.reshape(-1)])
    a_max = float(np.abs(both[np.isfinite(both)]).max())
    ta, tb = sp.tol_rows(T, K, a_max)
    tol = sp.tol_alpha(T - 1, K, a_max)
    fv = sparse_ctx((ip, ix, dt), Bm, Pi)
    try:
        got_a, got_b, rc = fv.test_sumprod_rows(ob)
        assert rc == 0
        expect_forms(fv, T, MEM)                            # the memory form, with no debug bit set
        check_rows(got_a, alpha, ta, "K=21120 alpha")
        check_rows(got_b, beta, tb, "K=21120 beta")
        gamma, path, ll = fv.posteriors(ob)
        print(f"K={K}: loglik {ll!r} model {want!r} bound {tol:.3e}")
        assert abs(ll - want) <= tol
        assert np.abs(gamma.astype(np.float64) - gam).max() <= 2.0 ** -23 + 3 * tol
        assert np.abs(gamma.astype(np.float64).sum(axis=1) - 1.0).max() <= K * 2.0 ** -24 + 3 * tol
        ab = alpha + beta
        assert (ab[np.arange(T), path] >= ab.max(axis=1) - 2 * tol).all()
        assert bits(fv.loglik(ob)) == bits(ll)
        st = fv.sumprod_stats()
        assert st["batch_cap"] == 4 and st["step_launches"] == T - 1
        ll2, _ = fv.loglik_batch([ob, ob[:3], ob[:5]])
        assert bits(ll2[0]) == bits(ll)
    finally:
        fv.close()


# ---------------------------------------------------------------- 8. the switch

def test_the_switch():
    A, B, Pi = model("ds_K9_T7")
    ob = observations(B.shape[1], 7, 2)
    calls = lambda f: (lambda: f.loglik(ob), lambda: f.loglik_batch([ob, ob]), lambda: f.posteriors(ob), lambda: f.test_sumprod_rows(ob))
    never = sparse_ctx(D.dense_to_csr(A), B, Pi, on=None)
    back = sparse_ctx(D.dense_to_csr(A), B, Pi, on=1)
    dense = D.FlashViterbi(0)
    try:
        want = back.loglik(ob)
        r = truth("switch", A, Pi, sp.emission_rows(B, ob))
        assert abs(want - r["loglik"]) <= sp.tol_alpha(6, A.shape[0], sp.amax(r))
        back.set_sparse_sumprod(0)
        for f, before in ((never, (D.ERR_STATE, None)), (back, stats_state(back))):
            held = live_bytes(f, ob)
            for c in calls(f):
                refused(f, c, D.ERR_UNSUPPORTED, before)
                detail = f._L.fv_last_error_detail(f._h).decode()
                assert UNSUPPORTED_DETAIL in detail and "the backward pass needs the out-edge form on the device" in detail
            assert live_bytes(f, ob) == held
        back.set_sparse_sumprod(1)
        assert bits(back.loglik(ob)) == bits(want)
        # the value 2, and a NULL-free negative
        for bad in (2, -1):
            with pytest.raises(D.FlashVitError) as e:
                back.set_sparse_sumprod(bad)
            assert e.value.rc == D.ERR_ARG
        assert bits(back.loglik(ob)) == bits(want)          # (the setting is as it was)
        # FV_ERR_STATE while a stream or a set is open
        for opener, closer in ((back.stream_open, back.stream_abort), (lambda: back.streams_open(2), back.streams_end)):
            opener()
            for on in (0, 1):
                with pytest.raises(D.FlashVitError) as e:
                    back.set_sparse_sumprod(on)
                assert e.value.rc == D.ERR_STATE
            closer()
        # the setting survives fv_set_model_sparse
        back.set_model_sparse(*D.dense_to_csr(A), B, Pi)
        assert bits(back.loglik(ob)) == bits(want)
        # a dense-set model: the same bits with 0 and 1, and only dense step kernels
        dense.set_model(A, B, Pi)
        ll0 = dense.loglik(ob)
        dense.set_sparse_sumprod(1)
        assert bits(dense.loglik(ob)) == bits(ll0)
        assert dense.test_sumprod_forms() & ~FORMS["dense"] == 0 and dense.test_sumprod_forms() & FORMS["dense"]
        dense.set_sparse_sumprod(0)
        assert bits(dense.loglik(ob)) == bits(ll0)
        # ... and the setting survives fv_set_model too: the sparse model set next is admitted
        dense.set_sparse_sumprod(1)
        dense.set_model(A, B, Pi)
        dense.set_model_sparse(*D.dense_to_csr(A), B, Pi)
        assert bits(dense.loglik(ob)) == bits(want)
    finally:
        for f in (never, back, dense):
            f.close()


# ---------------------------------------------------------------- 9. the context is left as it was

def test_decodes_are_unchanged_and_set_model_sparse_drops_the_tables():
    name = "structured333"
    A, B, Pi, ob = named(name)
    csr = D.dense_to_csr(A)
    nnz = csr[1].size
    fv = sparse_ctx(csr, B, Pi)
    try:
        fv.set_option(D.OPT_SPARSE_BEAM, 1)
        bytes_model = fv.stats()["device_bytes"]
        full = fv.decode_full(ob, 3, D.MODE_REFERENCE)
        beam = fv.decode_beam(ob, 2, 16, D.MODE_REFERENCE)
        fv.loglik(ob[:40])
        cslin = fv.sumprod_stats()["table_bytes_per_step"] // 2          # 4 of the 8 bytes per padded entry
        one_table = fv.sumprod_stats()["device_bytes"]
        fv.posteriors(ob[:40])
        fv.loglik_batch([ob[:7], ob[:3]])
        two_tables = fv.sumprod_stats()["device_bytes"]
        assert two_tables >= one_table + 4 * nnz
        for before, after in ((full, fv.decode_full(ob, 3, D.MODE_REFERENCE)), (beam, fv.decode_beam(ob, 2, 16, D.MODE_REFERENCE))):
            assert (after[0].tolist(), np.float32(after[1]).view(np.uint32), after[2]) == (before[0].tolist(), np.float32(before[1]).view(np.uint32), before[2])
        grown = fv.stats()["device_bytes"]                 # (the decodes' workspace and the sum-product buffers)
        fv.set_model_sparse(*csr, B, Pi)
        after_set = fv.stats()["device_bytes"]
        assert bytes_model <= after_set <= grown - cslin - 4 * nnz        # CSlin and CRlin went with the model
        fv.loglik(ob[:40])
        assert fv.sumprod_stats()["device_bytes"] == after_set + cslin    # ... and the next call builds CSlin only
    finally:
        fv.close()


# ---------------------------------------------------------------- 10. NOMEM

def test_a_working_set_beyond_the_device_is_refused_before_anything_is_allocated(ctx):
    """fv_posteriors keeps 16 * T * K bytes of rows: K = 1030 and T = 30 million are 494 GB, more than the device has"""
    name, T = "plain1030", 30_000_000
    fv = ctx(name)
    small = observations(6, 5, 1)
    fv.posteriors(small)
    before, held = stats_state(fv), live_bytes(fv, small)
    refused(fv, lambda: fv.posteriors(np.zeros(T, dtype=np.int32), want_gamma=False), D.ERR_NOMEM, before)
    detail = fv._L.fv_last_error_detail(fv._h).decode()
    assert "fv_posteriors workspace" in detail and "bytes needed" in detail and str(16 * T * 1030) in detail
    assert int(detail.split(": ")[1].split(" bytes needed")[0]) >= 16 * T * 1030
    assert live_bytes(fv, small) == held
    assert bits(fv.posteriors(small)[2]) == bits(fv.loglik(small))
