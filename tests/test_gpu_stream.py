"""GPU: fv_stream_* — the online decode against the one-shot single-pass decode, the oracle and the CPU model of the
commit rule (tests/stream_model.py).

Every case compares, with equality only:
  * the concatenation of the pieces, the score (as uint32) and the return code with decode_full(ob, 1, MODE_SINGLE_PASS) on
    a second context and with the oracle's single pass;
  * every piece, and so the committed count after every push, with the model — an implementation that buffers everything
    and decodes at close fails here;
  * checks, commits, lag_max and bt_restarts of the stream's statistics with the model's.
Shapes are the smallest at which the new code can go wrong: K below one wave, not a multiple of 64, two waves, several
workgroups of the ancestor kernels (K = 2053, 3965); check intervals 1, 4, 16, 64; pushes of 1, 7, 64, T and a ragged list
with a first push of 1 and pushes that end one step after a check."""
import os
import re

import numpy as np
import pytest

import stream_model as sm
from conftest import ROOT, load_goldens
from flash_viterbi_amd import decoder
from test_gpu_emissions import libm_log
from test_gpu_emissions_tied import f32_to_bf16_bits
from test_stream_model import CHECKS, case, model_run, tables

pytestmark = pytest.mark.gpu

D = decoder
DENSE_KERNELS = (D.KERNEL_AUTO, D.KERNEL_F64_STREAM, D.KERNEL_F32_REFINE, D.KERNEL_F16_REFINE, D.KERNEL_Q16_REFINE,
                 D.KERNEL_SPARSE_Q16, D.KERNEL_U16_REFINE)


def default_check_every():
    text = open(os.path.join(ROOT, "flash_viterbi_amd", "csrc", "fv_stream.hip")).read()
    return int(re.search(r"STREAM_CHECK_DEFAULT\s*=\s*(\d+)", text).group(1))


def bits(x):
    return int(np.float32(x).view(np.uint32))


def refused(call, rc):
    with pytest.raises(D.FlashVitError) as e:
        call()
    assert e.value.rc == rc, (e.value.rc, str(e.value))
    return str(e.value)


@pytest.fixture(scope="module")
def ctx():
    made = {}

    def get(name, sparse=False):
        """(the context that streams, the context of the one-shot decodes) on the case's model"""
        key = (name, sparse)
        if key not in made:
            A, B, Pi, _ = case(name)
            pair = (D.FlashViterbi(0), D.FlashViterbi(0))
            for fv in pair:
                if sparse:
                    fv.set_model_sparse(*D.dense_to_csr(A), B, Pi)
                else:
                    fv.set_model(A, B, Pi)
            made[key] = pair
        for fv in made[key]:
            if fv.stream_pending() >= 0:
                fv.stream_abort()
            fv.set_option(D.OPT_KERNEL, D.KERNEL_AUTO)
        return made[key]
    yield get
    for pair in made.values():
        for fv in pair:
            fv.close()


def run_stream(fv, chunks, check_every, ob=None, feed=None, hint=0):
    """The sequence through one stream: pushes of the lengths `chunks` (symbols ob, or the score rows feed(pos, n) returns)
    and a close.  The shape of stream_model.run's result, with score, rc and the stream's statistics."""
    fv.stream_open(hint, check_every)
    out = dict(pieces=[], committed=[], dead=None, score=None, rc=None)
    pos = done = 0
    try:
        for q, n in enumerate(chunks):
            try:
                piece = fv.stream_push(ob=ob[pos:pos + n]) if feed is None else fv.stream_push(scores=feed(pos, n))
            except D.FlashVitError as e:
                if e.rc != D.ERR_NO_PRED:
                    raise
                out["dead"] = q
                out["committed"].append(done)
                break
            pos += n
            done += piece.size
            out["pieces"].append(piece.tolist())
            out["committed"].append(done)
            assert fv.stream_pending() == pos - done
        if out["dead"] is None:
            piece, out["score"], out["rc"] = fv.stream_close()
            out["pieces"].append(piece.tolist())
    finally:
        if fv.stream_pending() >= 0:
            fv.stream_abort()
    out["stats"] = fv.stream_stats()
    return out


def check_run(got, want, ref, tag):
    """got: run_stream's result; want: the model's; ref: (path list, score bits, rc) of the one-shot decode"""
    assert got["dead"] is None and want["dead"] is None, tag
    assert got["committed"] == want["committed"], tag
    assert got["pieces"] == want["pieces"], tag
    assert ([x for p in got["pieces"] for x in p], bits(got["score"]), got["rc"]) == ref, tag
    st = got["stats"]
    assert (st["checks"], st["commits"]) == (want["checks"], want["commits"]), tag
    assert (st["lag_max"], st["bt_restarts"]) == (want["lag_max"], want["bt_restarts"]), tag
    T = len(ref[0])
    assert (st["times"], st["committed"], st["pushes"]) == (T, T, len(got["committed"])), tag


def one_shot(name, ref_fv):
    """the second context's decode, first checked against the oracle's single pass"""
    _, _, _, ob = case(name)
    row, args, path = tables(name)
    res = ref_fv.decode_full(ob, 1, D.MODE_SINGLE_PASS)
    ref = (res[0].tolist(), bits(res[1]), res[2])
    assert ref == (path, bits(row[path[-1]]), 0), name
    return ref


# ---------------------------------------------------------------- 1. every chunking, every check interval

SMALL = ["ds_K5_T3", "ds_K9_T7", "ds_K77_M7_T33", "cfg1_K128_T256", "ds_K200_T100", "ties_all_K64_T64", "cfg1_deadA", "cfg1_deadB",
         "rotor_noise", "wideAB"]


@pytest.mark.parametrize("check_every", CHECKS)
@pytest.mark.parametrize("name", SMALL)
def test_every_chunking_matches_model_and_one_shot(ctx, name, check_every):
    fv, ref_fv = ctx(name)
    _, _, _, ob = case(name)
    ref = one_shot(name, ref_fv)
    closes = set()
    for cn, chunks in sm.chunkings(len(ob)).items():
        got = run_stream(fv, chunks, check_every, ob=ob)
        check_run(got, model_run(name, check_every, cn), ref, (name, check_every, cn))
        closes.add(len(got["pieces"][-1]))
    if name.startswith("cfg1"):
        assert 0 < max(closes) < 128          # the close's pending range: the serial walk of one lane


def test_default_interval_and_capacity(ctx):
    fv, ref_fv = ctx("cfg1_K128_T256")
    _, _, _, ob = case("cfg1_K128_T256")
    got = run_stream(fv, sm.chunkings(256)["7"], 0, ob=ob)
    check_run(got, model_run("cfg1_K128_T256", default_check_every(), "7"), one_shot("cfg1_K128_T256", ref_fv), "default")
    assert got["stats"]["regrows"] == 0 and got["stats"]["arg_rows_capacity"] >= 64
    assert got["stats"]["kernel"] == ref_fv.stats()["kernel"] and got["stats"]["push_ms_total"] > 0


def test_several_workgroups_all_ties(ctx):
    """K = 2053: nine workgroups of the ancestor kernels, every score tied, nothing ever commits"""
    name = "circulant2053"
    fv, ref_fv = ctx(name)
    _, _, _, ob = case(name)
    ref = one_shot(name, ref_fv)
    for ce, cn in ((16, "7"), (1, "T"), (4, "ragged")):
        got = run_stream(fv, sm.chunkings(len(ob))[cn], ce, ob=ob)
        check_run(got, model_run(name, ce, cn), ref, (ce, cn))
        assert got["stats"]["commits"] == 0 and len(got["pieces"][-1]) == len(ob)


def test_cfg2_in_pushes_of_64(ctx):
    """K = 3965, sixteen workgroups.  (The oracle's pass over this model takes the CPU long: the path is the golden's — the
    reference binary's, N = 1 — and the arg table for the model comes from the second context's own pass.)"""
    name = "cfg2_K3965_T256"
    fv, ref_fv = ctx(name)
    _, _, _, ob = case(name)
    g = next(g for g in load_goldens(True) if g["name"] == name)
    stored = next(r for r in g["runs"] if r["algo"] == "flash" and r["N"] == 1)
    res = ref_fv.decode_full(ob, 1, D.MODE_SINGLE_PASS)
    ref = (res[0].tolist(), bits(res[1]), res[2])
    assert ref[0] == stored["path"] and ref[2] == 0
    rows, bp, _ = ref_fv.test_forward(ob, [(0, len(ob) - 1, -1)])
    chunks = sm.chunkings(256)["64"]
    got = run_stream(fv, chunks, 16, ob=ob)
    check_run(got, sm.run(bp[1:], rows[0], 16, chunks), ref, name)
    assert got["stats"]["commits"] > 0


def test_close_after_one_time_and_after_none(ctx):
    fv, ref_fv = ctx("ds_K77_M7_T33")
    A, B, Pi, ob = case("ds_K77_M7_T33")
    fv.stream_open()
    assert fv.stream_push(ob=ob[:1]).size == 0 and fv.stream_pending() == 1
    piece, score, rc = fv.stream_close()
    # the oracle's init row: (float)(log Pi + log B[.][ob[0]]) in double, lowest index among its maxima
    init = (libm_log(Pi) + libm_log(B[:, ob[0]])).astype(np.float32)
    assert (piece.tolist(), bits(score), rc) == ([int(np.argmax(init))], bits(init.max()), 0)
    assert fv.stream_stats()["checks"] == 0
    fv.stream_open()
    piece, score, rc = fv.stream_close()
    assert piece.size == 0 and rc == 0 and fv.stream_pending() == -1


# ---------------------------------------------------------------- 2. dead streams, growth

def test_dead_verdict(ctx):
    name = "no_emitter"
    fv, ref_fv = ctx(name)
    A, B, Pi, ob = case(name)
    row, args, _ = tables(name)
    refused(lambda: ref_fv.decode_full(ob, 1, D.MODE_SINGLE_PASS), D.ERR_NO_PRED)
    refused(lambda: ref_fv.decode_full(ob[:21], 1, D.MODE_SINGLE_PASS), D.ERR_NO_PRED)
    for ce in CHECKS:
        for cn, chunks in sm.chunkings(len(ob)).items():
            want = sm.run(args, row, ce, chunks)
            got = run_stream(fv, chunks, ce, ob=ob)
            assert got["dead"] == want["dead"] is not None, (ce, cn)
            assert got["pieces"] == want["pieces"] and got["committed"] == want["committed"], (ce, cn)
            assert (got["stats"]["checks"], got["stats"]["commits"]) == (want["checks"], want["commits"]), (ce, cn)
    # a dead stream takes no push, its close delivers nothing, and the context is free again afterwards
    fv.stream_open(0, 4)
    refused(lambda: fv.stream_push(ob=ob[:24]), D.ERR_NO_PRED)
    refused(lambda: fv.stream_push(ob=ob[24:]), D.ERR_STATE)
    piece, score, rc = fv.stream_close()
    assert piece.size == 0 and rc == D.ERR_NO_PRED and fv.stream_pending() == -1
    fv.stream_open(0, 4)
    refused(lambda: fv.stream_push(ob=ob[:24]), D.ERR_NO_PRED)
    fv.stream_abort()
    assert fv.stream_pending() == -1


def test_lag_growth_and_the_long_walk(ctx):
    """a rotor without noise: chains never merge, nothing commits, the arg rows grow from 8, the close walks 299 steps"""
    name = "rotor"
    fv, ref_fv = ctx(name)
    _, _, _, ob = case(name)
    ref = one_shot(name, ref_fv)
    want = model_run(name, 16, "7")
    got = run_stream(fv, sm.chunkings(300)["7"], 16, ob=ob, hint=8)
    check_run(got, want, ref, name)
    st = got["stats"]
    assert st["regrows"] >= 3 and st["arg_rows_capacity"] >= 300 and st["commits"] == 0 and set(got["committed"]) == {0}
    assert st["bt_restarts"] == want["bt_restarts"] == ref_fv.stats()["bt_restarts"] > 0
    # the buffer is compacted, not grown, when commits free its front: pushes of 7 through 256 default rows
    fv2, ref2 = ctx("cfg1_K128_T256")
    got = run_stream(fv2, sm.chunkings(256)["7"], 4, ob=case("cfg1_K128_T256")[3], hint=48)
    check_run(got, model_run("cfg1_K128_T256", 4, "7"), one_shot("cfg1_K128_T256", ref2), "compaction")
    assert got["stats"]["arg_rows_capacity"] < 256


# ---------------------------------------------------------------- 3. kernels, sparse-set models, entries above 1

@pytest.mark.parametrize("kernel", DENSE_KERNELS)
def test_every_kernel_the_model_admits(ctx, kernel):
    name = "ds_K200_T100"
    fv, ref_fv = ctx(name)
    _, _, _, ob = case(name)
    for f in (fv, ref_fv):
        f.set_option(D.OPT_KERNEL, kernel)
    ref = one_shot(name, ref_fv)
    got = run_stream(fv, sm.chunkings(100)["ragged"], 4, ob=ob)
    check_run(got, model_run(name, 4, "ragged"), ref, kernel)
    assert got["stats"]["kernel"] == ref_fv.stats()["kernel"]
    if kernel not in (D.KERNEL_AUTO, D.KERNEL_SPARSE_Q16):
        assert got["stats"]["kernel"] == kernel


@pytest.mark.parametrize("kernel", [D.KERNEL_AUTO, D.KERNEL_CSR_F64])
@pytest.mark.parametrize("name", ["ds_K200_T100", "cfg1_deadA"])
def test_sparse_set_models(ctx, name, kernel):
    fv, ref_fv = ctx(name, sparse=True)
    _, _, _, ob = case(name)
    for f in (fv, ref_fv):
        f.set_option(D.OPT_KERNEL, kernel)
    ref = one_shot(name, ref_fv)
    for cn in ("7", "ragged"):
        got = run_stream(fv, sm.chunkings(len(ob))[cn], 16, ob=ob)
        check_run(got, model_run(name, 16, cn), ref, (name, kernel, cn))
    assert got["stats"]["kernel"] == (D.KERNEL_CSR_F64 if kernel == D.KERNEL_CSR_F64 else D.KERNEL_SPARSE_CSR)
    # a kernel that streams a dense table is refused at open, as the one-shot decode refuses it
    fv.set_option(D.OPT_KERNEL, D.KERNEL_F64_STREAM)
    assert "no dense table" in refused(lambda: fv.stream_open(), D.ERR_UNSUPPORTED)
    assert fv.stream_pending() == -1


def test_entries_above_one(ctx):
    """the float64 kernels, the only ones without a condition on the values: dense under F64_STREAM (AUTO's choice too),
    sparse-set under CSR_F64; the filter walk of the sparse-set model refuses at open"""
    import oracle
    A, B, Pi, ob = case("ds_K77_M7_T33")
    A = (A * np.float32(32.0)).astype(np.float32)
    assert (A > 1).sum() > 100 and ((A > 0) & (A < 1)).sum() > 100
    om = oracle.OracleModel(A, B, Pi)
    row, args = om.full_forward(ob, 0, len(ob) - 1, -1)
    path = sm.single_pass_path(row, args)
    chunks = sm.chunkings(len(ob))["ragged"]
    want = sm.run(args, row, 4, chunks)
    for sparse, kernel in ((False, D.KERNEL_F64_STREAM), (False, D.KERNEL_AUTO), (True, D.KERNEL_CSR_F64)):
        pair = (D.FlashViterbi(0), D.FlashViterbi(0))
        try:
            for f in pair:
                if sparse:
                    f.set_model_sparse(*D.dense_to_csr(A), B, Pi)
                else:
                    f.set_model(A, B, Pi)
                f.set_option(D.OPT_KERNEL, kernel)
            res = pair[1].decode_full(ob, 1, D.MODE_SINGLE_PASS)
            ref = (res[0].tolist(), bits(res[1]), res[2])
            assert ref == (path, bits(row[path[-1]]), 0)
            check_run(run_stream(pair[0], chunks, 4, ob=ob), want, ref, (sparse, kernel))
            if sparse:
                pair[0].set_option(D.OPT_KERNEL, D.KERNEL_AUTO)
                assert "FV_KERNEL_CSR_F64" in refused(lambda: pair[0].stream_open(), D.ERR_UNSUPPORTED)
            else:
                pair[0].set_option(D.OPT_KERNEL, D.KERNEL_U16_REFINE)
                refused(lambda: pair[0].stream_open(), D.ERR_UNSUPPORTED)
        finally:
            for f in pair:
                f.close()


# ---------------------------------------------------------------- 4. score rows

class Scores:
    """A and Pi of a golden, T rows of log scores in one of the input forms, and what the second context makes of the
    whole block: set_emissions + decode_full(None, 1, MODE_SINGLE_PASS), and the arg table of that pass (test_forward) for
    the model."""

    def __init__(self, name, form, sparse=False, positive=False, kernel=D.KERNEL_AUTO):
        A, _, Pi, ob = case(name)
        self.K, self.T = A.shape[0], len(ob)
        W = self.K
        rs = np.random.RandomState(11)
        E = rs.uniform(0.05, 1.0, (self.T, W))
        E[rs.uniform(size=E.shape) < 0.05] = 0
        logs = libm_log(E.astype(np.float32))
        if positive:
            logs = logs + 0.75
        self.ld = W + 3 if form in ("f32_ld", "f32_device") else W
        if form == "f64":
            block, self.code = logs, D.EMIS_LOG_F64
        elif form == "f16":
            block, self.code = logs.astype(np.float16), D.EMIS_LOG_F16
        elif form == "bf16":
            block, self.code = f32_to_bf16_bits(logs.astype(np.float32)), D.EMIS_LOG_BF16
        else:
            block, self.code = logs.astype(np.float32), D.EMIS_LOG_F32
        if self.ld > W:
            padded = np.full((self.T, self.ld), np.nan, dtype=block.dtype)
            padded[:, :W] = block
            block = padded
        self.block = np.ascontiguousarray(block)
        self.device = form == "f32_device"
        self.pair = (D.FlashViterbi(0), D.FlashViterbi(0))
        for f in self.pair:
            if sparse:
                f.set_model_sparse(*D.dense_to_csr(A), np.full((self.K, 2), 0.5, np.float32), Pi)
            else:
                f.set_model(A, np.full((self.K, 2), 0.5, np.float32), Pi)
            f.set_option(D.OPT_KERNEL, kernel)
        self.dptr = self.pair[0].test_device_alloc(self.block) if self.device else None

    def feed(self, pos, n):
        if self.device:
            return (self.dptr + pos * self.ld * self.block.itemsize, self.code, n, self.ld)
        return (self.block[pos:pos + n].ctypes.data, self.code, n, self.ld)

    def reference(self):
        ref_fv = self.pair[1]
        ref_fv.set_emissions((self.block.ctypes.data, self.code, self.T, self.ld))
        res = ref_fv.decode_full(None, 1, D.MODE_SINGLE_PASS, T=self.T)
        rows, bp, _ = ref_fv.test_forward(None, [(0, self.T - 1, -1)], T=self.T)
        assert int(np.argmax(rows[0])) == int(res[0][-1])
        return (res[0].tolist(), bits(res[1]), res[2]), rows[0], bp[1:]

    def close(self):
        if self.dptr:
            self.pair[0].test_device_free(self.dptr)
        for f in self.pair:
            f.close()


@pytest.mark.parametrize("form", ["f32", "f64", "f16", "bf16", "f32_ld", "f32_device"])
def test_score_rows(form):
    s = Scores("ds_K200_T100", form)
    try:
        ref, row, args = s.reference()
        assert ref[2] == 0
        for ce, cn in ((4, "ragged"), (16, "7")):
            chunks = sm.chunkings(s.T)[cn]
            check_run(run_stream(s.pair[0], chunks, ce, feed=s.feed), sm.run(args, row, ce, chunks), ref, (form, ce, cn))
        # the context's own staged rows are left alone by a stream of score rows
        assert s.pair[0].stats()["emission_rows"] == 0
    finally:
        s.close()


def test_score_rows_through_an_emission_map():
    A, _, Pi, ob = case("ds_K200_T100")
    K, T, P = A.shape[0], len(ob), 37
    pdf = np.random.RandomState(3).randint(0, P, K).astype(np.int32)
    logs = libm_log(np.random.RandomState(4).uniform(0.05, 1.0, (T, P)).astype(np.float32)).astype(np.float32)
    pair = (D.FlashViterbi(0), D.FlashViterbi(0))
    try:
        for f in pair:
            f.set_model(A, np.full((K, 2), 0.5, np.float32), Pi)
            f.set_emission_map(pdf, P)
        pair[1].set_emissions(logs)
        res = pair[1].decode_full(None, 1, D.MODE_SINGLE_PASS, T=T)
        rows, bp, _ = pair[1].test_forward(None, [(0, T - 1, -1)], T=T)
        ref = (res[0].tolist(), bits(res[1]), res[2])
        chunks = sm.chunkings(T)["ragged"]
        got = run_stream(pair[0], chunks, 4, feed=lambda pos, n: logs[pos:pos + n])
        check_run(got, sm.run(bp[1:], rows[0], 4, chunks), ref, "map")
        pair[0].stream_open()
        assert "ld >= P" in refused(lambda: pair[0].stream_push(scores=logs[:4], ld=P - 1), D.ERR_ARG)
        pair[0].stream_abort()
    finally:
        for f in pair:
            f.close()


@pytest.mark.parametrize("sparse", [False, True])
def test_refused_score_pushes_leave_the_stream_usable(sparse):
    s = Scores("ds_K77_M7_T33", "f32", sparse=sparse)
    try:
        ref, row, args = s.reference()
        fv, K = s.pair[0], s.K
        chunks = [5, 9, s.T - 14]
        want = sm.run(args, row, 4, chunks)
        fv.stream_open(0, 4)
        pieces = [fv.stream_push(scores=s.feed(0, 5)).tolist()]
        for bad, text in ((np.nan, "(t = 7, state = 3)"), (np.inf, "(t = 7, state = 3)")):
            rows = s.block[5:14].copy()
            rows[2, 3] = bad
            assert text in refused(lambda: fv.stream_push(scores=rows), D.ERR_ARG)
            assert fv.stream_pending() == 5 - len(pieces[0]) and fv.stream_stats()["times"] == 5
        rows = s.block[5:14].copy()
        rows[4, 1] = 0.5                      # a density above 1 under a filter kernel
        assert ("FV_KERNEL_CSR_F64" if sparse else "filter+refine") in refused(lambda: fv.stream_push(scores=rows), D.ERR_UNSUPPORTED)
        assert fv.stream_stats()["times"] == 5 and fv.stream_stats()["pushes"] == 1
        refused(lambda: fv.stream_push(ob=np.zeros(3, np.int32)), D.ERR_ARG)       # the other kind
        refused(lambda: fv.stream_push(scores=(s.block.ctypes.data, 7, 3, s.ld)), D.ERR_ARG)
        refused(lambda: fv.stream_push(scores=(s.block.ctypes.data, s.code, 3, K - 1)), D.ERR_ARG)
        refused(lambda: fv.stream_push(scores=(s.block.ctypes.data, s.code, 0, s.ld)), D.ERR_ARG)
        pieces.append(fv.stream_push(scores=s.feed(5, 9)).tolist())
        pieces.append(fv.stream_push(scores=s.feed(14, s.T - 14)).tolist())
        last, score, rc = fv.stream_close()
        pieces.append(last.tolist())
        assert pieces == want["pieces"] and ([x for p in pieces for x in p], bits(score), rc) == ref
    finally:
        s.close()


@pytest.mark.parametrize("sparse", [False, True])
def test_scores_above_zero_under_the_float64_kernels(sparse):
    s = Scores("ds_K77_M7_T33", "f64", sparse=sparse, positive=True,
               kernel=D.KERNEL_CSR_F64 if sparse else D.KERNEL_F64_STREAM)
    try:
        ref, row, args = s.reference()
        chunks = sm.chunkings(s.T)["7"]
        check_run(run_stream(s.pair[0], chunks, 4, feed=s.feed), sm.run(args, row, 4, chunks), ref, sparse)
    finally:
        s.close()


# ---------------------------------------------------------------- 5. life cycle and refusals

def test_life_cycle_and_refusals(ctx):
    fresh = D.FlashViterbi(0)
    try:
        assert fresh.stream_pending() == -1
        refused(lambda: fresh.stream_open(), D.ERR_STATE)                      # no model
        refused(lambda: fresh.stream_stats(), D.ERR_STATE)                     # there never was a stream
        refused(lambda: fresh.stream_push(ob=[0]), D.ERR_STATE)
        refused(lambda: fresh.stream_abort(), D.ERR_STATE)
        refused(lambda: fresh.stream_close(), D.ERR_STATE)
    finally:
        fresh.close()
    name = "ds_K77_M7_T33"
    fv, ref_fv = ctx(name)
    A, B, Pi, ob = case(name)
    ref = one_shot(name, ref_fv)
    before = fv.decode_full(ob, 2, D.MODE_REFERENCE)
    bytes_before = fv.stats()["device_bytes"]
    refused(lambda: fv.stream_open(-1, 0), D.ERR_ARG)
    refused(lambda: fv.stream_open(0, 65), D.ERR_ARG)
    refused(lambda: fv.stream_open(0, -1), D.ERR_ARG)
    fv.stream_open(0, 4)
    refused(lambda: fv.stream_open(0, 4), D.ERR_STATE)                         # one stream per context
    pieces = [fv.stream_push(ob=ob[:10]).tolist()]
    refused(lambda: fv.stream_push(ob=np.zeros(0, np.int32)), D.ERR_ARG)       # n < 1
    bad = ob[10:20].copy()
    bad[4] = B.shape[1]
    assert "ob[4]" in refused(lambda: fv.stream_push(ob=bad), D.ERR_ARG)
    bad[4] = -1
    refused(lambda: fv.stream_push(ob=bad), D.ERR_ARG)
    refused(lambda: fv.stream_push(scores=np.zeros((2, A.shape[0]), np.float32)), D.ERR_ARG)      # the other kind
    assert fv.stream_stats()["times"] == 10 and fv.stream_stats()["pushes"] == 1
    # everything else on the context waits for the stream to end
    for call in (lambda: fv.decode_full(ob, 1, D.MODE_SINGLE_PASS), lambda: fv.decode_full_batch([ob, ob]),
                 lambda: fv.decode_beam(ob, 1, 8), lambda: fv.decode_beam_batch([ob, ob], 1, 8), lambda: fv.decode_vanilla(ob),
                 lambda: fv.decode_checkpoint(ob), lambda: fv.set_model(A, B, Pi),
                 lambda: fv.set_model_sparse(*D.dense_to_csr(A), B, Pi), lambda: fv.set_option(D.OPT_KERNEL, D.KERNEL_F64_STREAM),
                 lambda: fv.set_emissions(np.zeros((3, A.shape[0]), np.float32)), lambda: fv.clear_emissions(),
                 lambda: fv.set_emission_map(np.zeros(A.shape[0], np.int32), 1), lambda: fv.test_forward(ob, [(0, 5, -1)]),
                 lambda: fv.test_flat_poison(3), lambda: fv.set_partition(0, 2)):
        assert "stream is open" in refused(call, D.ERR_STATE)
    pieces.append(fv.stream_push(ob=ob[10:]).tolist())
    last, score, rc = fv.stream_close()
    want = sm.run(tables(name)[1], tables(name)[0], 4, [10, len(ob) - 10])
    assert pieces + [last.tolist()] == want["pieces"] and ([x for p in pieces for x in p] + last.tolist(), bits(score), rc) == ref
    refused(lambda: fv.stream_push(ob=ob[:3]), D.ERR_STATE)                    # closed
    assert fv.stream_stats()["committed"] == len(ob)                           # the last stream's statistics stay
    # after the stream the context decodes what it decoded before, in the memory it had before
    after = fv.decode_full(ob, 2, D.MODE_REFERENCE)
    assert (after[0].tolist(), bits(after[1]), after[2]) == (before[0].tolist(), bits(before[1]), before[2])
    assert fv.stats()["device_bytes"] == bytes_before


def test_contexts_that_cannot_stream_and_destroy_with_a_stream_open():
    A, B, Pi, ob = case("ds_K9_T7")
    part = D.FlashViterbi(0)
    group = D.FlashViterbi([0, 0])
    gone = D.FlashViterbi(0)
    try:
        for f in (part, group, gone):
            f.set_model(A, B, Pi)
        part.set_partition(0, 2)
        for f in (part, group):
            refused(lambda: f.stream_open(), D.ERR_UNSUPPORTED)
            assert f.stream_pending() == -1
        gone.stream_open()
        gone.stream_push(ob=ob[:4])
    finally:
        for f in (part, group, gone):
            f.close()                          # fv_destroy frees the open stream
