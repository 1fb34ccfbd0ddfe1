"""CPU: the stream's commit rule (tests/stream_model.py) judged on the oracle's tables alone.

Every piece the rule hands out is the next stretch of the single-pass path (lowest index among the maxima of the last row,
serial walk), for every chunking and every check interval; all of them give the same concatenation; and the models the GPU
test uses are what they claim: the cfg1 golden commits often and early, so do its two variants with dead back-pointers, a
rotor without noise and the all-ties golden never commit, and a symbol no state emits makes the first check after it find
no live state.  Also home of the cases tests/test_gpu_stream.py runs on the device."""
import functools

import numpy as np
import pytest

import modelgen
import oracle
import stream_model as sm
from conftest import golden_model, load_goldens

CHECKS = (1, 4, 16, 64)


@functools.lru_cache(maxsize=None)
def golden(name):
    g = next(g for g in load_goldens(True) if g["name"] == name)
    return golden_model(g)


@functools.lru_cache(maxsize=None)
def case(name):
    """(A, B, Pi, ob) float32 / int32 of a named case"""
    if name == "cfg1_deadA":                  # five states no transition leads to: their back-pointer is -1 at every time
        A, B, Pi, ob = golden("cfg1_K128_T256")
        A = A.copy()
        A[:, [3, 40, 41, 90, 127]] = 0
        return A, B, Pi, ob
    if name == "cfg1_deadB":                  # 42 states cannot emit symbol 0: dead at the times that observe it
        A, B, Pi, ob = golden("cfg1_K128_T256")
        B = B.copy()
        B[:42, 0] = 0
        return A, B, Pi, ob
    if name in ("rotor_noise", "rotor"):      # chains merge slowly / never
        A, B, Pi = modelgen.rotor(61, 7, 0.2 if name == "rotor_noise" else 0, 100 + 61)
        return A, B, Pi, np.random.RandomState(5).randint(0, 7, 300).astype(np.int32)
    if name.startswith("circulant"):          # all ties, K = 257 / 2053: never commits
        K = int(name[len("circulant"):])
        A, B, Pi = modelgen.circulant_ties(K)
        return A, B, Pi, modelgen.circulant_observations(41, 3, 41)
    if name.startswith("wide"):
        return modelgen.wide_model(name, 300, 10, 200, 77)
    if name == "no_emitter":                  # nobody emits symbol 2, observed at time 20
        A, B, Pi, ob = golden("ds_K77_M7_T33")
        B, ob = B.copy(), ob.copy()
        B[:, 2] = 0
        ob[ob == 2] = 3
        ob[20] = 2
        return A, B, Pi, ob
    return golden(name)


@functools.lru_cache(maxsize=None)
def tables(name):
    """(last row, arg table, single-pass path) of the case from the oracle"""
    A, B, Pi, ob = case(name)
    om = oracle.OracleModel(A, B, Pi)
    row, args = om.full_forward(ob, 0, len(ob) - 1, -1)
    return row, args, sm.single_pass_path(row, args)


@functools.lru_cache(maxsize=None)
def model_run(name, check_every, chunking):
    row, args, _ = tables(name)
    return sm.run(args, row, check_every, sm.chunkings(len(args) + 1)[chunking])


def all_runs(name):
    T = len(tables(name)[1]) + 1
    return {(ce, cn): model_run(name, ce, cn) for ce in CHECKS for cn in sm.chunkings(T)}


LIVE = ["cfg1_K128_T256", "cfg1_deadA", "cfg1_deadB", "ds_K200_T100", "ds_K77_M7_T33", "ds_K5_T3", "ds_K9_T7", "ties_all_K64_T64",
        "ties_semi_K96_T80", "rotor_noise", "rotor", "circulant257", "wideA", "wideB", "wideAB"]


@pytest.mark.parametrize("name", LIVE)
def test_pieces_are_the_single_pass_path(name):
    row, args, ref = tables(name)
    assert min(ref) >= 0
    for key, r in all_runs(name).items():
        assert r["dead"] is None, key
        done = 0
        for piece, count in zip(r["pieces"], r["committed"] + [len(ref)]):
            assert piece == ref[done:done + len(piece)], key          # the next stretch of the path, final once handed out
            done += len(piece)
            assert done == count, key
        assert done == len(ref), key
        # a check per check_every steps and one at the end of every push that ran a step since the last
        assert r["checks"] >= (len(ref) - 1 + key[0] - 1) // key[0] and r["commits"] <= r["checks"], key


def test_chunkings_have_the_shapes_the_cases_need():
    c = sm.chunkings(256)
    assert all(sum(v) == 256 for v in c.values())
    assert c["ragged"][0] == 1 and 17 in c["ragged"] and c["T"] == [256] and set(c["7"]) == {7, 4}


def test_cfg1_commits_often_and_early():
    runs = all_runs("cfg1_K128_T256")
    for key, r in runs.items():
        if key[0] <= 16:
            assert 10 <= r["commits"] <= 20 and 200 < r["committed"][-1] < 256, (key, r["commits"], r["committed"][-1])
        else:                                 # a check every 64 steps (sooner only where a push ends): as few as four in 255 steps
            assert 3 <= r["commits"] <= 20 and r["committed"][-1] >= 128, (key, r["commits"], r["committed"][-1])
    got = {key: (runs[key]["commits"], runs[key]["checks"], runs[key]["committed"][-1]) for key in ((1, "7"), (16, "7"), (16, "ragged"))}
    assert got == {(1, "7"): (20, 255, 221), (16, "7"): (18, 37, 231), (16, "ragged"): (13, 28, 222)}


@pytest.mark.parametrize("name", ["cfg1_deadA", "cfg1_deadB"])
def test_dead_back_pointers_do_not_stop_the_commits(name):
    row, args, ref = tables(name)
    assert (args < 0).sum() > 0               # the variant has states without a predecessor
    for key, r in all_runs(name).items():
        assert (r["commits"] >= 10 and r["committed"][-1] > 200) if key[0] <= 16 else r["commits"] >= 3, key
    if name == "cfg1_deadA":
        assert (args < 0).sum() == 5 * 255
        r = model_run(name, 16, "ragged")
        assert (r["commits"], r["committed"][-1]) == (15, 240)


@pytest.mark.parametrize("name", ["rotor", "ties_all_K64_T64", "circulant257"])
def test_some_models_never_commit(name):
    row, args, ref = tables(name)
    for key, r in all_runs(name).items():
        assert r["commits"] == 0 and set(r["committed"]) == {0} and r["lag_max"] == len(ref), key
        assert len(r["pieces"][-1]) == len(ref)
    if name == "rotor":
        assert model_run(name, 16, "7")["bt_restarts"] == 8        # the close walks 299 steps in 64 lanes


def test_a_symbol_nobody_emits_kills_the_stream_at_the_next_check():
    A, B, Pi, ob = case("no_emitter")
    row, args, _ = tables("no_emitter")
    assert (args[19] < 0).all() and (args[18] >= 0).any()
    om = oracle.OracleModel(A, B, Pi)
    assert om.full_decode(ob, 1, check=False)[3] == -3 and om.full_decode(ob[:21], 1, check=False)[3] == -3
    T = len(ob)
    for ce in CHECKS:
        for cn, chunks in sm.chunkings(T).items():
            r = sm.run(args, row, ce, chunks)
            ends = np.cumsum(chunks)
            q = int(np.searchsorted(ends, 21))                      # the push that consumes time 20
            assert r["dead"] == q, (ce, cn)
            # the pieces before it stand: they are the one-shot path of the prefix that was still alive
            live_row, live_args = om.full_forward(ob[:20], 0, 19, -1)
            ref = sm.single_pass_path(live_row, live_args)
            cat = [x for p in r["pieces"] for x in p]
            assert cat == ref[:len(cat)] and r["committed"][-1] == len(cat), (ce, cn)
