"""GPU: fv_loglik / fv_loglik_batch / fv_posteriors against the float64 CPU model (tests/sumprod_model.py) within the
bound of guarantee 1 of include/flashvit.h, the two flush models of guarantee 2, the bit equalities of guarantee 3, the
refusals, and the context left as it was.

Shapes: K = 5 (less than one tile), 37 (pads in tile and row block), 200, 1030 (more source rows than threads, 65
tiles), once K = 3965 with T = 16; T in {1, 2, 3, 40}."""
import ctypes
import math
import os

import numpy as np
import pytest

import modelgen
import sumprod_model as sp
from conftest import golden_model, load_goldens
from flash_viterbi_amd import decoder

pytestmark = pytest.mark.gpu

D = decoder


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64).tolist()


def golden(name, big=False):
    return next(g for g in load_goldens(big) if g["name"] == name)


_models = {}


def model(name):
    """float32 (A, B, Pi) by name, built once"""
    if name not in _models:
        if name.startswith("plain"):
            K, M, dens, seed = {"plain37": (37, 4, 0.5, 11), "plain200": (200, 5, 0.3, 12), "plain1030": (1030, 6, 0.2, 13)}[name]
            _models[name] = modelgen.plain_model(K, M, dens, seed)
        else:
            _models[name] = golden_model(golden(name, big=True))[:3]
    return _models[name]


@pytest.fixture(scope="module")
def ctx():
    made = {}

    def get(name):
        if name not in made:
            fv = D.FlashViterbi(0)
            fv.set_model(*model(name))
            made[name] = fv
        fv = made[name]
        fv.set_option(D.OPT_MAX_BATCH, 8)
        return fv
    yield get
    for fv in made.values():
        fv.close()


def observations(M, T, seed):
    return np.random.default_rng(seed).integers(0, M, T).astype(np.int32)


def scores(T, K, seed, dtype=np.float64):
    """log scores in about [-7, 0], a tenth of them -inf"""
    rng = np.random.default_rng(seed)
    x = np.log(rng.random((T, K)) + 1e-3)
    x[rng.random((T, K)) < 0.1] = -np.inf
    return x.astype(dtype)


def check_rows(got, want, tol, tag):
    """-inf where, and only where, the model's value is -inf; the finite ones within the row's tolerance"""
    assert (np.isneginf(got) == np.isneginf(want)).all(), tag
    assert not np.isnan(got).any() and not np.isposinf(got).any(), tag
    fin = np.isfinite(want)
    err = np.where(fin, np.abs(np.where(fin, got, 0.0) - np.where(fin, want, 0.0)), 0.0)
    worst = (err / tol).max()
    print(f"{tag}: worst error / bound = {worst:.3e} (bound at the last row {float(tol.max()):.3e})")
    assert (err <= tol).all(), tag


def check_call(fv, A, Pi, e, ob, T, tag):
    """the hook's rows, loglik, gamma and path of one input against the model"""
    K = A.shape[0]
    r = sp.run(A, Pi, e)
    a_max = sp.amax(r)
    ta, tb = sp.tol_rows(T, K, a_max)
    tol = sp.tol_alpha(T - 1, K, a_max)
    alpha, beta, rc = fv.test_sumprod_rows(ob, T=None if ob is not None else T)
    check_rows(alpha, r["alpha"], ta, tag + " alpha")
    check_rows(beta, r["beta"], tb, tag + " beta")
    gamma, path, ll = fv.posteriors(ob, T=None if ob is not None else T)
    assert math.isfinite(r["loglik"]) and rc == 0, tag
    print(f"{tag}: loglik {ll!r} model {r['loglik']!r} bound {tol:.3e}")
    assert abs(ll - r["loglik"]) <= tol, tag
    assert fv.loglik(ob, T=None if ob is not None else T) == ll, tag
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
    return r, ll


# ---------------------------------------------------------------- 1. forward and backward against the model

@pytest.mark.parametrize("name,T", [("ds_K5_T3", 1), ("ds_K5_T3", 2), ("ds_K5_T3", 3), ("plain37", 1), ("plain37", 3), ("plain37", 40),
                                    ("ds_K200_T100", 40), ("plain1030", 2), ("plain1030", 12)])
def test_symbols_against_the_model(ctx, name, T):
    A, B, Pi = model(name)
    fv = ctx(name)
    ob = observations(B.shape[1], T, 100 + T)
    check_call(fv, A, Pi, sp.emission_rows(B, ob), ob, T, f"{name} T={T}")
    st = fv.sumprod_stats()
    assert st["passes"] == 1 and st["step_launches"] == T - 1 == st["task_steps"]      # (the last call was loglik)
    assert st["table_bytes_per_step"] == 4 * ((A.shape[0] + 15) // 16) * 16 * ((A.shape[0] + 31) // 32 * 32)


def test_cfg2_once(ctx):
    name, T = "cfg2_K3965_T256", 16
    A, B, Pi = model(name)
    ob = np.asarray(golden(name, big=True)["ob"][:T], dtype=np.int32)
    check_call(ctx(name), A, Pi, sp.emission_rows(B, ob), ob, T, name)
    assert ctx(name).sumprod_stats()["refine_finite"] == 0


@pytest.mark.parametrize("name,T,dtype", [("plain37", 40, np.float32), ("plain37", 3, np.float64), ("plain200", 40, np.float64),
                                          ("plain1030", 3, np.float32)])
def test_staged_emissions_against_the_model(ctx, name, T, dtype):
    A, B, Pi = model(name)
    fv = ctx(name)
    x = scores(T, A.shape[0], 7 * T, dtype)
    x[0, 0] = 0.0                       # (a live start, whatever the draw)
    fv.set_emissions(x)
    try:
        check_call(fv, A, Pi, x.astype(np.float64), None, T, f"{name} staged {np.dtype(dtype).name} T={T}")
    finally:
        fv.clear_emissions()


def test_emission_map_against_the_model(ctx):
    name, T, P = "plain200", 3, 23
    A, B, Pi = model(name)
    fv = ctx(name)
    K = A.shape[0]
    pdf = (np.arange(K) * 7 % P).astype(np.int32)
    x = scores(T, P, 5, np.float32)
    x[:, 0] = -1.0
    fv.set_emission_map(pdf, P)
    try:
        fv.set_emissions(x)
        check_call(fv, A, Pi, x.astype(np.float64)[:, pdf], None, T, "plain200 tied")
    finally:
        fv.set_emission_map(None)


# ---------------------------------------------------------------- 2 - 4. the flush models, and an ordinary one

@pytest.mark.parametrize("which", ["forward", "backward"])
def test_flush_models_come_out_finite(which):
    A, B, Pi, e = sp.flush_forward() if which == "forward" else sp.flush_backward()
    fv = D.FlashViterbi(0)
    try:
        fv.set_model(A, B, Pi)
        fv.set_emissions(e)
        r, ll = check_call(fv, A, Pi, e, None, sp.FLUSH_T, "flush " + which)
        assert math.isfinite(ll)
        if which == "forward":
            assert fv.sumprod_stats()["refine_finite"] >= 1        # (the last call, fv_loglik: the forward pass alone)
            gamma, path, _ = fv.posteriors(None, T=sp.FLUSH_T)
            assert gamma[2, 36] == 1 and gamma[3, 35] == 1 and (path[2], path[3]) == (36, 35)
        else:
            fv.loglik(None, T=sp.FLUSH_T)
            forward_only = fv.sumprod_stats()["refine_finite"]
            gamma, path, _ = fv.posteriors(None, T=sp.FLUSH_T)
            st = fv.sumprod_stats()
            assert st["passes"] == 2 and st["refine_finite"] - forward_only >= 1      # the backward pass's own
            assert gamma[sp.FLUSH_T - 3, 36] == 1 and gamma[sp.FLUSH_T - 4, 35] == 1
        assert fv.sumprod_stats()["refine_columns"] >= fv.sumprod_stats()["refine_finite"]
    finally:
        fv.close()


def test_ordinary_model_refines_nothing_finite(ctx):
    name = "ds_K200_T100"
    fv = ctx(name)
    ob = np.asarray(golden(name)["ob"][:40], dtype=np.int32)
    fv.posteriors(ob)
    st = fv.sumprod_stats()
    assert st["refine_finite"] == 0 and st["passes"] == 2 and st["step_launches"] == 2 * 39


# ---------------------------------------------------------------- 5. batch

def dead_symbol_model():
    """plain37 with one more symbol that no state emits: a sequence holding it has probability 0"""
    A, B, Pi = model("plain37")
    return A, np.concatenate([B, np.zeros((B.shape[0], 1), dtype=np.float32)], axis=1), Pi


@pytest.mark.parametrize("name", ["plain37", "plain1030"])
def test_batch_has_the_bits_of_single_calls(ctx, name):
    A, B, Pi = model(name)
    fv = ctx(name)
    lengths = [1, 7, 3, 12, 1, 9, 2, 12, 5] if name == "plain37" else [1, 4, 2, 5, 1, 3, 2, 5, 4]
    obs = [observations(B.shape[1], n, 40 + i) for i, n in enumerate(lengths)]
    single = [fv.loglik(o) for o in obs]
    assert all(math.isfinite(x) for x in single)
    r = sp.run(A, Pi, sp.emission_rows(B, obs[3]))
    assert abs(single[3] - r["loglik"]) <= sp.tol_alpha(lengths[3] - 1, A.shape[0], sp.amax(r))
    for cap in (1, 4, 8):
        fv.set_option(D.OPT_MAX_BATCH, cap)
        for nseq in (1, 3, 8, 9):
            ll, status = fv.loglik_batch(obs[:nseq])
            assert bits(ll) == bits(single[:nseq]), (cap, nseq)
            assert status.tolist() == [0] * nseq
            st = fv.sumprod_stats()
            assert st["batch_cap"] == min(cap, 4) and st["passes"] == 1
            assert st["task_steps"] == sum(n - 1 for n in lengths[:nseq])
            if cap == 1:
                assert st["step_launches"] == st["task_steps"]
    fv.set_option(D.OPT_MAX_BATCH, 8)
    ll, _ = fv.loglik_batch(obs[::-1])                      # another grouping of the same sequences
    assert bits(ll) == bits(single[::-1])


def test_batch_with_a_zero_probability_sequence():
    A, B, Pi = dead_symbol_model()
    fv = D.FlashViterbi(0)
    try:
        fv.set_model(A, B, Pi)
        M = B.shape[1]
        obs = [observations(M - 1, n, 60 + n) for n in (5, 1, 8, 3)]
        dead = obs[2].copy()
        dead[4] = M - 1
        single = [fv.loglik(o) for o in obs]
        assert fv.loglik(dead) == -math.inf
        ll, status = fv.loglik_batch([obs[0], obs[1], dead, obs[3]])
        assert status.tolist() == [0, 0, D.ERR_NO_PRED, 0]
        assert ll[2] == -math.inf and bits(np.delete(ll, 2)) == bits([single[0], single[1], single[3]])
        rc = fv._L.fv_loglik_batch(fv._h, decoder._p(dead), decoder._p(np.array([0, 8], dtype=np.int64)), 1, decoder._p(np.zeros(1)), None)
        assert rc == D.ERR_NO_PRED
        gamma = np.full((8, A.shape[0]), 7.0, dtype=np.float32)
        path = np.zeros(8, dtype=np.int32)
        out = ctypes.c_double(0)
        assert fv._L.fv_posteriors(fv._h, decoder._p(dead), 8, decoder._p(gamma), A.shape[0], decoder._p(path), ctypes.byref(out)) == D.ERR_NO_PRED
        assert out.value == -math.inf and (path == -1).all() and (gamma == 7.0).all()      # gamma_out is not written
    finally:
        fv.close()


# ---------------------------------------------------------------- 6. guarantee 3

def device_read(ptr, nbytes):
    hip = ctypes.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    out = np.empty(nbytes, dtype=np.uint8)
    assert hip.hipMemcpy(decoder._p(out), ctypes.c_void_p(ptr), nbytes, 2) == 0       # hipMemcpyDeviceToHost
    return out


@pytest.mark.parametrize("name,T", [("plain37", 40), ("plain1030", 3)])
def test_reproducible_bits_and_gamma_destinations(ctx, name, T):
    A, B, Pi = model(name)
    fv = ctx(name)
    K = A.shape[0]
    ob = observations(B.shape[1], T, 77)
    first = fv.posteriors(ob)
    again = fv.posteriors(ob)
    assert first[0].tobytes() == again[0].tobytes() and first[1].tolist() == again[1].tolist() and bits(first[2]) == bits(again[2])
    assert bits(fv.loglik(ob)) == bits(first[2]) == bits(fv.loglik(ob))
    a1, b1, _ = fv.test_sumprod_rows(ob)
    a2, b2, _ = fv.test_sumprod_rows(ob)
    assert a1.tobytes() == a2.tobytes() and b1.tobytes() == b2.tobytes()
    # host and device gamma_out at ld > K: equal bytes, pads untouched
    ld = K + 5
    host = np.full((T, ld), 9.0, dtype=np.float32)
    out = ctypes.c_double(0)
    assert fv._L.fv_posteriors(fv._h, decoder._p(ob), T, decoder._p(host), ld, None, ctypes.byref(out)) == 0
    assert bits(out.value) == bits(first[2])
    assert host[:, :K].tobytes() == first[0].tobytes() and (host[:, K:] == 9.0).all()
    dev = fv.test_device_alloc(np.full((T, ld), 9.0, dtype=np.float32))
    try:
        gamma, path, ll = fv.posteriors(ob, out=(dev, ld))
        assert gamma is None and path.tolist() == first[1].tolist() and bits(ll) == bits(first[2])
        assert device_read(dev, T * ld * 4).tobytes() == host.tobytes()
    finally:
        fv.test_device_free(dev)
    # gamma_out == NULL and path_out == NULL are accepted
    assert fv._L.fv_posteriors(fv._h, decoder._p(ob), T, None, 0, None, ctypes.byref(out)) == 0 and bits(out.value) == bits(first[2])
    assert fv._L.fv_posteriors(fv._h, decoder._p(ob), T, None, 0, None, None) == 0
    gamma, path, _ = fv.posteriors(ob, want_gamma=False)
    assert gamma is None and path.tolist() == first[1].tolist()


# ---------------------------------------------------------------- 7. values

def test_entries_above_one_and_scores_above_zero():
    K, T = 37, 12
    rng = np.random.default_rng(3)
    A = (1 + 49 * rng.random((K, K))).astype(np.float32)
    B = (1 + 3 * rng.random((K, 3))).astype(np.float32)
    Pi = (1 + 9 * rng.random(K)).astype(np.float32)
    x = rng.random((T, K)) * 4 - 1                # emission scores in [-1, 3)
    fv = D.FlashViterbi(0)
    try:
        fv.set_model(A, B, Pi)
        assert A.max() > 1 and A.max() <= 50 and x.max() > 0
        ob = observations(3, T, 4)
        check_call(fv, A, Pi, sp.emission_rows(B, ob), ob, T, "entries above 1")
        fv.set_emissions(x)
        check_call(fv, A, Pi, x, None, T, "scores above 0")
    finally:
        fv.close()


def test_unreachable_states_have_gamma_zero():
    A, B, Pi, ob = modelgen.unreachable_fast(77, 5, 9, 21)
    fv = D.FlashViterbi(0)
    try:
        fv.set_model(A, B, Pi)
        r, _ = check_call(fv, A, Pi, sp.emission_rows(B, ob), ob, len(ob), "unreachable")
        gone = np.isneginf(r["alpha"]).all(axis=0)
        assert gone.sum() >= 3
        gamma, _, _ = fv.posteriors(ob)
        assert (gamma[:, gone] == 0).all()
    finally:
        fv.close()


def test_permutation_model_sums_its_only_path():
    K, T = 37, 40
    rng = np.random.default_rng(8)
    perm = rng.permutation(K)
    A = np.zeros((K, K), dtype=np.float32)
    A[np.arange(K), perm] = 1.0
    Pi = np.zeros(K, dtype=np.float32)
    Pi[5] = 0.25
    B = np.full((K, 2), 0.5, dtype=np.float32)
    x = np.log(rng.random((T, K)) + 1e-3)
    fv = D.FlashViterbi(0)
    try:
        fv.set_model(A, B, Pi)
        fv.set_emissions(x)
        state, total, states = 5, math.log(0.25), []
        for t in range(T):
            states.append(state)
            total += x[t, state]
            state = perm[state]
        gamma, path, ll = fv.posteriors(None, T=T)
        r = sp.run(A, Pi, x)
        assert abs(ll - total) <= sp.tol_alpha(T - 1, K, sp.amax(r))
        assert path.tolist() == states and (gamma[np.arange(T), states] == 1).all() and gamma.sum() == T
    finally:
        fv.close()


SMALL_GOLDENS = [g["name"] for g in load_goldens()]


@pytest.mark.parametrize("name", SMALL_GOLDENS)
def test_loglik_is_at_least_the_viterbi_score(name):
    g = golden(name)
    A, B, Pi, ob = golden_model(g)
    score = next(r["score"] for r in g["runs"] if r["algo"] == "flash")
    T, K = len(ob), A.shape[0]
    fv = D.FlashViterbi(0)
    try:
        fv.set_model(A, B, Pi)
        ll = fv.loglik(ob)
        alpha = sp.forward(A, Pi, sp.emission_rows(B, ob))
        a_max = float(np.abs(alpha[np.isfinite(alpha)]).max())
        tol = sp.tol_alpha(T - 1, K, a_max)
        print(f"{name}: loglik {ll!r} Viterbi score {score!r}")
        assert ll >= score - (T * 2.0 ** -23 * abs(score) + tol)
        assert abs(ll - sp.lse(alpha[T - 1])) <= tol
    finally:
        fv.close()


# ---------------------------------------------------------------- 8. refusals

def refused(fv, call, rc, stats_before):
    with pytest.raises(D.FlashVitError) as e:
        call()
    assert e.value.rc == rc, e.value
    assert fv._L.fv_last_error_detail(fv._h).decode() != ""
    st = D.SumprodStats()                              # no device work: the refused call is not the last call
    got = fv._L.fv_last_sumprod_stats(fv._h, ctypes.byref(st))
    assert (got, st.as_dict() if got == 0 else None) == stats_before


def stats_state(fv):
    st = D.SumprodStats()
    got = fv._L.fv_last_sumprod_stats(fv._h, ctypes.byref(st))
    return (got, st.as_dict() if got == 0 else None)


def live_bytes(fv, ob):
    """the context's device working set as a decode finds it (fv_stats.device_bytes is added up at the end of a decode): a
    refused call that had grown a buffer or built a table would show here"""
    fv.decode_full(ob, 1, D.MODE_SINGLE_PASS)
    return fv.stats()["device_bytes"]


def test_refusals():
    """Every refusal of the header but two.  K > 20192 is not run: a model of that size costs fv_set_model ten seconds and
    more of host logs and table encodings (8 * K^2 = 3.3 GB for the float64 table alone); the rule itself, one LDS row, is
    the batch_cap the other tests read back.  FV_ERR_NOMEM has a test of its own below."""
    A, B, Pi = model("ds_K9_T7")
    ob = np.asarray(golden("ds_K9_T7")["ob"], dtype=np.int32)
    calls = lambda f: (lambda: f.loglik(ob), lambda: f.loglik_batch([ob, ob]), lambda: f.posteriors(ob), lambda: f.test_sumprod_rows(ob))
    sparse, part, group, plain = D.FlashViterbi(0), D.FlashViterbi(0), D.FlashViterbi([0, 0]), D.FlashViterbi(0)
    try:
        for f in (plain, sparse, part, group):
            assert stats_state(f) == (D.ERR_STATE, None)
        for c in calls(plain):
            refused(plain, c, D.ERR_STATE, (D.ERR_STATE, None))                 # no model
        sparse.set_model_sparse(*D.dense_to_csr(A), B, Pi)
        for f in (part, group, plain):
            f.set_model(A, B, Pi)
        part.set_partition(0, 2)
        for f in (sparse, part, group):
            held = live_bytes(f, ob)
            for c in calls(f):
                refused(f, c, D.ERR_UNSUPPORTED, (D.ERR_STATE, None))
            assert live_bytes(f, ob) == held
        assert "fv_set_model_sparse" in sparse._L.fv_last_error_detail(sparse._h).decode()
        want = plain.loglik(ob)
        before = stats_state(plain)
        held = live_bytes(plain, ob)
        plain.stream_open()
        for c in calls(plain):
            refused(plain, c, D.ERR_STATE, before)
        plain.stream_abort()
        plain.streams_open(2)
        for c in calls(plain):
            refused(plain, c, D.ERR_STATE, before)
        plain.streams_end()
        bad = ob.copy()
        bad[3] = B.shape[1]
        neg = ob.copy()
        neg[0] = -1
        for c in (lambda: plain.loglik(np.zeros(0, dtype=np.int32)), lambda: plain.posteriors(np.zeros(0, dtype=np.int32)),
                  lambda: plain.loglik(None, T=0), lambda: plain.loglik_batch([ob, np.zeros(0, dtype=np.int32)]),
                  lambda: plain.loglik(bad), lambda: plain.posteriors(neg), lambda: plain.loglik_batch([ob, bad]),
                  lambda: plain.test_sumprod_rows(bad),
                  lambda: plain.loglik(None, T=4), lambda: plain.posteriors(None, T=4), lambda: plain.loglik_batch(None, lengths=[2, 2]),
                  lambda: plain.posteriors(ob, out=(1 << 20, A.shape[0] - 1))):                          # ld < K
            refused(plain, c, D.ERR_ARG, before)
        assert live_bytes(plain, ob) == held            # nothing grew, no table was built by any refused call
        plain.set_emissions(np.zeros((3, A.shape[0]), dtype=np.float32))
        refused(plain, lambda: plain.loglik(None, T=4), D.ERR_ARG, before)          # too few staged rows
        assert math.isfinite(plain.loglik(None, T=3))
        assert bits(plain.loglik(ob)) == bits(want)
    finally:
        for f in (sparse, part, group, plain):
            f.close()


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


# ---------------------------------------------------------------- 9. the context is left as it was

def test_decodes_are_unchanged_and_set_model_drops_the_tables(ctx):
    name = "ds_K200_T100"
    A, B, Pi = model(name)
    ob = np.asarray(golden(name)["ob"], dtype=np.int32)
    fv = D.FlashViterbi(0)
    try:
        fv.set_model(A, B, Pi)
        bytes_model = fv.stats()["device_bytes"]
        full = fv.decode_full(ob, 3, D.MODE_REFERENCE)
        beam = fv.decode_beam(ob, 2, 16, D.MODE_REFERENCE)
        fv.loglik(ob[:40])
        table = fv.sumprod_stats()["table_bytes_per_step"]
        one_table = fv.sumprod_stats()["device_bytes"]
        fv.posteriors(ob[:40])
        fv.loglik_batch([ob[:7], ob[:3]])
        two_tables = fv.sumprod_stats()["device_bytes"]
        assert two_tables >= one_table + table
        for before, after in ((full, fv.decode_full(ob, 3, D.MODE_REFERENCE)), (beam, fv.decode_beam(ob, 2, 16, D.MODE_REFERENCE))):
            assert (after[0].tolist(), np.float32(after[1]).view(np.uint32), after[2]) == (before[0].tolist(), np.float32(before[1]).view(np.uint32), before[2])
        grown = fv.stats()["device_bytes"]                 # (the decodes' workspace and the sum-product buffers)
        fv.set_model(A, B, Pi)
        after_set = fv.stats()["device_bytes"]
        assert bytes_model <= after_set <= grown - 2 * table          # both tables went with the model
        fv.loglik(ob[:40])
        assert fv.sumprod_stats()["device_bytes"] == after_set + table    # ... and the next call builds the one it needs
    finally:
        fv.close()
