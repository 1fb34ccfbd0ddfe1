"""GPU: fv_expected_counts against the float64 CPU model (tests/counts_model.py) within guarantee G1 of include/flashvit.h,
the two flush models of G2, the bit equalities of G3, the other input forms, the refusals, and the context left as it was.

Shapes are those of test_gpu_sumprod.py: K = 5 (less than one tile), 37 (pads in every tile), 200 (four 64-wide tiles, the last
one ragged), 1030 (17 tiles each way, more than 1024 states); T in {1, 2, 3, 12, 17, 40}: none, one and several 16-time trips of
the xi kernel, with a ragged last one."""
import ctypes
import math
import os

import numpy as np
import pytest

import counts_model as cm
import modelgen
import sumprod_model as sp
from conftest import golden_model, load_goldens
from flash_viterbi_amd import decoder

pytestmark = pytest.mark.gpu

D = decoder
OUTPUTS = ("trans", "emit", "init", "occ")


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


def check_counts(got, want, A, lengths, tag):
    """G1 for every output the call gave, the exact zeros, and the identities; want: counts_model.fold's dict"""
    K = A.shape[0]
    live = [math.isfinite(c["loglik"]) for c in want["each"]]
    a_max = max(sp.amax(c["run"]) for c in want["each"])
    R = cm.tolerance(max(lengths), K, a_max)
    n = {"trans": sum(lengths) - len(lengths), "emit": sum(lengths), "init": len(lengths), "occ": sum(lengths)}
    for k in OUTPUTS:
        if got[k] is None:
            continue
        ok, worst = cm.within(got[k], want[k], R, max(n[k], 1))
        print(f"{tag} {k}: worst error / bound = {worst:.3e} (R = {R:.3e})")
        assert ok, (tag, k)
    assert (got["trans"][A == 0] == 0).all(), tag
    assert (got["trans"] >= 0).all() and (got["occ"] >= 0).all(), tag
    for s, c in enumerate(want["each"]):
        if live[s]:
            assert abs(got["loglik"][s] - c["loglik"]) <= sp.tol_alpha(lengths[s] - 1, K, sp.amax(c["run"])), tag
    # the identities, each side within G1 of the exact value
    slack = lambda x: 2 * R * np.abs(x) + K * 2.0 ** -150
    assert (np.abs(got["trans"].sum(axis=1) - (got["occ"] - want["last"])) <= slack(got["occ"])).all(), tag
    steps = sum(t - 1 for t, a in zip(lengths, live) if a)
    assert abs(got["trans"].sum() - steps) <= slack(steps), tag
    assert abs(got["init"].sum() - sum(live)) <= slack(sum(live)), tag
    if got["emit"] is not None:
        assert (np.abs(got["emit"].sum(axis=1) - got["occ"]) <= slack(got["occ"])).all(), tag


def ordered_sum(singles):
    """left to right, the first term standing alone"""
    tot = {k: singles[0][k] for k in OUTPUTS}
    for c in singles[1:]:
        for k in OUTPUTS:
            tot[k] = tot[k] + c[k]
    return tot


def same_bits(a, b, tag):
    for k in OUTPUTS:
        assert a[k].tobytes() == b[k].tobytes(), (tag, k)


# ---------------------------------------------------------------- 1. against the model

@pytest.mark.parametrize("name,T", [("ds_K5_T3", 1), ("ds_K5_T3", 2), ("ds_K5_T3", 3), ("plain37", 1), ("plain37", 2), ("plain37", 40),
                                    ("plain200", 40), ("plain1030", 12)])
def test_symbols_against_the_model(ctx, name, T):
    A, B, Pi = model(name)
    fv = ctx(name)
    ob = observations(B.shape[1], T, 100 + T)
    got = fv.expected_counts([ob])
    check_counts(got, cm.batch(A, B, Pi, [ob]), A, [T], f"{name} T={T}")
    st = fv.counts_stats()
    assert (st["sequences"], st["dead_sequences"], st["times"], st["wide_times"]) == (1, 0, T, 0)
    assert st["step_launches"] == 2 * (T - 1) == st["task_steps"] and st["xi_launches"] == (1 if T >= 2 else 0)
    assert got["status"].tolist() == [0] and bits(got["loglik"]) == bits([fv.loglik(ob)])
    if T == 1:
        assert (got["trans"] == 0).all() and bits(got["init"]) == bits(got["occ"])
    same_bits(got, fv.expected_counts([ob]), "twice")
    only = fv.expected_counts([ob], want_trans=False)
    assert only["trans"] is None and fv.counts_stats()["xi_launches"] == 0
    for k in ("emit", "init", "occ"):
        assert only[k].tobytes() == got[k].tobytes()


# ---------------------------------------------------------------- 2. the flush models

@pytest.mark.parametrize("which", ["forward", "backward"])
def test_flush_models_keep_their_transition_mass(which):
    A, B, Pi, e = sp.flush_forward() if which == "forward" else sp.flush_backward()
    fv = D.FlashViterbi(0)
    try:
        fv.set_model(A, B, Pi)
        fv.set_emissions(e)
        got = fv.expected_counts(None, lengths=[sp.FLUSH_T])
        want = cm.one(A, Pi, e)
        assert got["emit"] is None
        check_counts(got, cm.fold([want], sp.FLUSH_K), A, [sp.FLUSH_T], "flush " + which)
        wide = cm.wide_times(want["w"])
        assert wide == ([1, 2] if which == "forward" else [2, 3])
        assert fv.counts_stats()["wide_times"] == len(wide)
        assert abs(got["trans"].sum() - (sp.FLUSH_T - 1)) <= 1e-9          # all five units of transition mass
    finally:
        fv.close()


# ---------------------------------------------------------------- 3. batches (G3)

def dead_symbol_model():
    """plain37 with one more symbol that no state emits: a sequence holding it has probability 0"""
    A, B, Pi = model("plain37")
    return A, np.concatenate([B, np.zeros((B.shape[0], 1), dtype=np.float32)], axis=1), Pi


@pytest.mark.parametrize("name", ["plain37", "plain1030"])
def test_a_ragged_batch_is_the_ordered_sum_of_single_calls(ctx, name):
    A, B, Pi = model(name)
    fv = ctx(name)
    lengths = [1, 2, 17, 40]
    obs = [observations(B.shape[1], n, 40 + i) for i, n in enumerate(lengths)]
    singles = [fv.expected_counts([o]) for o in obs]
    want = ordered_sum(singles)
    for cap in (1, 8):
        fv.set_option(D.OPT_MAX_BATCH, cap)
        got = fv.expected_counts(obs)
        same_bits(got, want, (name, cap))
        assert bits(got["loglik"]) == bits([fv.loglik(o) for o in obs]) == bits([c["loglik"][0] for c in singles])
        st = fv.counts_stats()
        assert (st["sequences"], st["dead_sequences"], st["times"], st["xi_launches"]) == (4, 0, sum(lengths), 3)
        assert st["task_steps"] == 2 * (sum(lengths) - 4)
    fv.set_option(D.OPT_MAX_BATCH, 8)
    if name == "plain37":
        check_counts(got, cm.batch(A, B, Pi, obs), A, lengths, "ragged batch")
    back = fv.expected_counts(obs[::-1])                    # another order: another sum
    same_bits(back, ordered_sum(singles[::-1]), (name, "reversed"))


def test_a_zero_probability_sequence_in_the_middle_adds_nothing():
    A, B, Pi = dead_symbol_model()
    fv = D.FlashViterbi(0)
    try:
        fv.set_model(A, B, Pi)
        M = B.shape[1]
        obs = [observations(M - 1, n, 60 + n) for n in (5, 8, 3)]
        dead = obs[1].copy()
        dead[4] = M - 1
        singles = [fv.expected_counts([o]) for o in (obs[0], obs[2])]
        got = fv.expected_counts([obs[0], dead, obs[2]])
        same_bits(got, ordered_sum(singles), "dead in the middle")
        assert got["status"].tolist() == [0, D.ERR_NO_PRED, 0] and got["loglik"][1] == -math.inf
        assert bits(np.delete(got["loglik"], 1)) == bits([fv.loglik(obs[0]), fv.loglik(obs[2])])
        st = fv.counts_stats()
        assert (st["sequences"], st["dead_sequences"], st["times"]) == (3, 1, 8)
        check_counts(got, cm.batch(A, B, Pi, [obs[0], dead, obs[2]]), A, [5, 8, 3], "dead in the middle")
        alone = fv.expected_counts([dead])
        assert alone["status"].tolist() == [D.ERR_NO_PRED] and all((alone[k] == 0).all() for k in OUTPUTS)
        offsets = np.array([0, 8], dtype=np.int64)
        assert fv._L.fv_expected_counts(fv._h, decoder._p(dead), decoder._p(offsets), 1, None, 0, None, None, None, None, None) == D.ERR_NO_PRED
    finally:
        fv.close()


# ---------------------------------------------------------------- 4. other inputs

def test_staged_emissions_in_a_batch(ctx):
    name, lengths = "plain37", [17, 1, 23]
    A, B, Pi = model(name)
    fv = ctx(name)
    x = scores(sum(lengths), A.shape[0], 9, np.float32)
    starts = np.concatenate([[0], np.cumsum(lengths)])
    x[starts[:-1], 0] = 0.0                       # (a live start, whatever the draw)
    fv.set_emissions(x)
    try:
        got = fv.expected_counts(None, lengths=lengths)
        each = [cm.one(A, Pi, x[a:b].astype(np.float64)) for a, b in zip(starts, starts[1:])]
        check_counts(got, cm.fold(each, A.shape[0]), A, lengths, "staged")
        assert got["emit"] is None and got["status"].tolist() == [0, 0, 0]
    finally:
        fv.clear_emissions()


def test_emission_map(ctx):
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
        got = fv.expected_counts(None, lengths=[T])
        check_counts(got, cm.fold([cm.one(A, Pi, x.astype(np.float64)[:, pdf])], K), A, [T], "plain200 tied")
    finally:
        fv.set_emission_map(None)


def device_read(ptr, nbytes):
    hip = ctypes.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    out = np.empty(nbytes, dtype=np.uint8)
    assert hip.hipMemcpy(decoder._p(out), ctypes.c_void_p(ptr), nbytes, 2) == 0       # hipMemcpyDeviceToHost
    return out


@pytest.mark.parametrize("name", ["plain37", "plain200"])
def test_row_pitch_and_a_device_trans_out(ctx, name):
    A, B, Pi = model(name)
    fv = ctx(name)
    K, ld = A.shape[0], A.shape[0] + 5
    obs = [observations(B.shape[1], n, 70 + n) for n in (17, 3)]
    want = fv.expected_counts(obs)
    ob = np.concatenate(obs)
    offsets = np.array([0, 17, 20], dtype=np.int64)
    host = np.full((K, ld), 9.0)
    assert fv._L.fv_expected_counts(fv._h, decoder._p(ob), decoder._p(offsets), 2, decoder._p(host), ld, None, None, None, None, None) == 0
    assert host[:, :K].tobytes() == want["trans"].tobytes() and (host[:, K:] == 9.0).all()
    dev = fv.test_device_alloc(np.full((K, ld), 9.0))
    try:
        got = fv.expected_counts(obs, trans_out=(dev, ld))
        assert got["trans"] is None
        for k in ("emit", "init", "occ"):
            assert got[k].tobytes() == want[k].tobytes()
        assert device_read(dev, K * ld * 8).tobytes() == host.tobytes()
    finally:
        fv.test_device_free(dev)


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
        assert A.max() > 1 and x.max() > 0
        ob = observations(3, T, 4)
        check_counts(fv.expected_counts([ob]), cm.batch(A, B, Pi, [ob]), A, [T], "entries above 1")
        fv.set_emissions(x)
        check_counts(fv.expected_counts(None, lengths=[T]), cm.fold([cm.one(A, Pi, x)], K), A, [T], "scores above 0")
        assert fv.counts_stats()["wide_times"] == 0
    finally:
        fv.close()


# ---------------------------------------------------------------- 5. refusals

def counts_state(fv):
    st = D.CountsStats()
    got = fv._L.fv_last_counts_stats(fv._h, ctypes.byref(st))
    return (got, st.as_dict() if got == 0 else None)


def refused(fv, call, rc, state_before):
    try:
        got = call()
    except D.FlashVitError as e:
        got = e.rc
    assert got == rc, got
    assert fv._L.fv_last_error_detail(fv._h).decode() != ""
    assert counts_state(fv) == state_before              # no device work: the refused call is not the last call


def live_bytes(fv, ob):
    """the context's device working set as a decode finds it: a refused call that had grown a buffer would show here"""
    fv.decode_full(ob, 1, D.MODE_SINGLE_PASS)
    return fv.stats()["device_bytes"]


def raw(fv, ob, offsets, trans=None, ld=0, emit=None):
    offsets = np.asarray(offsets, dtype=np.int64)
    return fv._L.fv_expected_counts(fv._h, None if ob is None else decoder._p(ob), decoder._p(offsets), offsets.size - 1,
                                    None if trans is None else decoder._p(trans), ld, None if emit is None else decoder._p(emit),
                                    None, None, None, None)


def test_refusals():
    """Every refusal of the header but two.  K > 20192 is not run, as in test_gpu_sumprod.py: a model of that size costs
    fv_set_model ten seconds and more; the rule is the one admission check the sum-product calls share.  FV_ERR_NOMEM has a
    test of its own below."""
    A, B, Pi = model("ds_K9_T7")
    K = A.shape[0]
    ob = np.asarray(golden("ds_K9_T7")["ob"], dtype=np.int32)
    call = lambda f: (lambda: f.expected_counts([ob, ob]))
    sparse, part, group, plain = D.FlashViterbi(0), D.FlashViterbi(0), D.FlashViterbi([0, 0]), D.FlashViterbi(0)
    try:
        none = (D.ERR_STATE, None)
        for f in (plain, sparse, part, group):
            assert counts_state(f) == none
        refused(plain, call(plain), D.ERR_STATE, none)                          # no model
        sparse.set_model_sparse(*D.dense_to_csr(A), B, Pi)
        for f in (part, group, plain):
            f.set_model(A, B, Pi)
        part.set_partition(0, 2)
        for f in (sparse, part, group):
            held = live_bytes(f, ob)
            refused(f, call(f), D.ERR_UNSUPPORTED, none)
            assert live_bytes(f, ob) == held
        sparse.set_sparse_sumprod(1)                                            # ... whether or not the sum-product route is on
        assert math.isfinite(sparse.loglik(ob))
        refused(sparse, call(sparse), D.ERR_UNSUPPORTED, none)
        assert "fv_set_model_sparse" in sparse._L.fv_last_error_detail(sparse._h).decode()
        want = plain.expected_counts([ob])
        before, held = counts_state(plain), live_bytes(plain, ob)
        plain.stream_open()
        refused(plain, call(plain), D.ERR_STATE, before)
        plain.stream_abort()
        plain.streams_open(2)
        refused(plain, call(plain), D.ERR_STATE, before)
        plain.streams_end()
        bad = ob.copy()
        bad[3] = B.shape[1]
        trans, emit = np.zeros((K, K)), np.zeros((K, B.shape[1]))
        for c in (lambda: plain.expected_counts([ob, np.zeros(0, dtype=np.int32)]), lambda: plain.expected_counts([]),
                  lambda: plain.expected_counts([ob, bad]), lambda: plain.expected_counts(None, lengths=[2, 2]),      # nothing staged
                  lambda: raw(plain, ob, [1, 7]), lambda: raw(plain, ob, [0, 5, 3]), lambda: raw(plain, ob, [0, 7], trans, K - 1),
                  lambda: plain.expected_counts([ob], trans_out=(1 << 20, K - 1)),
                  lambda: plain._L.fv_expected_counts(plain._h, decoder._p(ob), None, 1, None, 0, None, None, None, None, None)):
            refused(plain, c, D.ERR_ARG, before)
        plain.set_emissions(np.zeros((3, K), dtype=np.float32))
        refused(plain, lambda: plain.expected_counts(None, lengths=[2, 2]), D.ERR_ARG, before)          # too few staged rows
        refused(plain, lambda: raw(plain, None, [0, 3], emit=emit), D.ERR_ARG, before)                  # emit_out without an alphabet
        assert raw(plain, None, [0, 3], trans, K) == 0
        if D.device_count() >= 2:
            other = D.FlashViterbi(1)
            try:
                there = other.test_device_alloc(np.zeros((K, K)))
                state = counts_state(plain)
                refused(plain, lambda: plain.expected_counts([ob], trans_out=there), D.ERR_ARG, state)
                other.test_device_free(there)
            finally:
                other.close()
        plain.clear_emissions()
        assert live_bytes(plain, ob) >= held
        same_bits(plain.expected_counts([ob]), want, "after the refusals")
    finally:
        for f in (sparse, part, group, plain):
            f.close()


def test_a_working_set_beyond_the_device_is_refused_before_anything_is_allocated(ctx):
    """32 * T * K bytes of alpha, beta, P and Q rows: K = 1030 and T = 30 million are 989 GB, more than the device has"""
    name, T = "plain1030", 30_000_000
    fv = ctx(name)
    small = observations(6, 5, 1)
    fv.expected_counts([small])
    before, held = counts_state(fv), live_bytes(fv, small)
    refused(fv, lambda: fv.expected_counts([np.zeros(T, dtype=np.int32)]), D.ERR_NOMEM, before)
    detail = fv._L.fv_last_error_detail(fv._h).decode()
    assert "fv_expected_counts workspace" in detail and "bytes needed" in detail
    assert int(detail.split(": ")[1].split(" bytes needed")[0]) >= 32 * (T - 1) * 1030
    assert live_bytes(fv, small) == held


# ---------------------------------------------------------------- 6. the context is left as it was

def test_the_context_decodes_and_scores_as_before_and_follows_its_model(ctx):
    name = "plain37"
    A, B, Pi = model(name)
    ob = observations(B.shape[1], 40, 5)
    fv = D.FlashViterbi(0)
    try:
        fv.set_model(A, B, Pi)
        full = fv.decode_full(ob, 3, D.MODE_REFERENCE)
        post = fv.posteriors(ob)
        sp_stats, forms = fv.sumprod_stats(), fv.test_sumprod_forms()
        first = fv.expected_counts([ob, ob[:7]])
        assert fv.sumprod_stats() == sp_stats and fv.test_sumprod_forms() == forms      # their own last call
        after = fv.decode_full(ob, 3, D.MODE_REFERENCE)
        assert (after[0].tolist(), np.float32(after[1]).view(np.uint32), after[2]) == (full[0].tolist(), np.float32(full[1]).view(np.uint32), full[2])
        again = fv.posteriors(ob)
        assert again[0].tobytes() == post[0].tobytes() and again[1].tolist() == post[1].tolist() and bits(again[2]) == bits(post[2])
        A2, B2, Pi2 = modelgen.plain_model(37, 4, 0.7, 99)
        fv.set_model(A2, B2, Pi2)
        got = fv.expected_counts([ob, ob[:7]])
        check_counts(got, cm.batch(A2, B2, Pi2, [ob, ob[:7]]), A2, [40, 7], "replaced model")
        fv.set_model(A, B, Pi)
        same_bits(fv.expected_counts([ob, ob[:7]]), first, "the first model again")
    finally:
        fv.close()


# ---------------------------------------------------------------- 7. end to end

def test_baum_welch_steps_never_lower_the_likelihood():
    A, B, Pi = model("plain37")
    A, B, Pi = (cm.normalise_rows(x).astype(np.float32) for x in (A, B, Pi))
    lengths = [5, 9, 12, 17, 21, 26, 33, 40]
    obs = [observations(B.shape[1], n, 200 + n) for n in lengths]
    margin = sum(lengths) * 2.0 ** -22
    fv = D.FlashViterbi(0)
    try:
        fv.set_model(A, B, Pi)
        seen = [D.baum_welch_step(fv, obs) for _ in range(3)]
        seen.append(float(np.sum(fv.loglik_batch(obs)[0])))
        print("Baum-Welch logliks:", seen)
        assert all(math.isfinite(x) for x in seen)
        assert all(b >= a - margin for a, b in zip(seen, seen[1:]))
        assert seen[-1] > seen[0]
    finally:
        fv.close()
