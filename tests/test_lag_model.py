"""CPU: the lag-bounded commit rule (tests/lag_model.py) judged on the oracle's tables alone.

The counts the rule gives on the stream cases, the bound 2 L + C - 2 on the pending times after every push of every
chunking, equality with tests/stream_model.py when the lag is never reached, connected paths that run through every recorded
commit, and commits on the models that never commit without a bound.  Also home of the cached model runs
tests/test_gpu_stream_lag.py compares the device with."""
import functools

import numpy as np
import pytest

import lag_model as lm
import stream_model as sm
from test_stream_model import case, model_run, tables

GRID = ((1, 1), (4, 4), (8, 16), (64, 16))            # (max_lag, check_every)


@functools.lru_cache(maxsize=None)
def lag_run(name, max_lag, check_every, chunking):
    A, B, Pi, ob = case(name)
    return lm.run(A, B, Pi, ob, check_every, max_lag, sm.chunkings(len(ob))[chunking])


def check_path(name, r, tag):
    """the pieces are one connected path through every recorded commit, with the counts the pushes reported"""
    A, _, _, ob = case(name)
    assert r["dead"] is None, tag
    path = r["path"]
    assert len(path) == len(ob) and lm.connected(A, path), tag
    done = 0
    for piece, count in zip(r["pieces"], r["committed"] + [len(ob)]):
        done += len(piece)
        assert done == count, tag
    for a, v, _ in r["records"]:
        assert path[a] == v, tag
    for t, a, v, best, _ in r["forced"]:
        assert path[a] == v and r["pruned"][t].any() and not r["pruned"][t, path[t]], tag
    assert r["commits"] == len(r["records"]) and r["lag"]["forced_commits"] == len(r["forced"]) <= r["commits"], tag


FIGURES = [("cfg1_K128_T256", 4, 4, 31, 38), ("cfg1_K128_T256", 64, 16, 0, 18), ("rotor_noise", 8, 16, 21, 21), ("rotor", 4, 4, 1, 86),
           ("circulant257", 4, 4, 6, 6), ("ties_all_K64_T64", 4, 4, 10, 10), ("wideAB", 4, 4, 29, 29), ("ds_K9_T7", 4, 4, 1, 1)]


@pytest.mark.parametrize("name,L,C,forced,commits", FIGURES)
def test_counts_in_pushes_of_seven(name, L, C, forced, commits):
    r = lag_run(name, L, C, "7")
    check_path(name, r, (name, L, C))
    assert (r["lag"]["forced_commits"], r["commits"]) == (forced, commits)
    assert max(r["pending"]) <= lm.bound(L, C)
    if (name, L) == ("cfg1_K128_T256", 4):
        assert max(r["pending"]) == 10 == lm.bound(4, 4)           # the bound is attained
    if name == "rotor_noise":
        assert max(r["pending"]) == 21 and lm.bound(8, 16) == 30
    if name == "rotor":                                            # one forced commit leaves a single chain: the rest merge by themselves
        assert r["lag"]["first_forced_time"] == r["lag"]["last_forced_time"] == r["forced"][0][0]
        assert r["lag"]["pruned_states"] == 60


@pytest.mark.parametrize("name", ["cfg1_K128_T256", "cfg1_deadA", "rotor_noise", "rotor", "circulant257", "ties_all_K64_T64", "ds_K77_M7_T33"])
def test_the_bound_holds_after_every_push_of_every_chunking(name):
    T = len(case(name)[3])
    for L, C in ((4, 4), (8, 16)):
        for cn in sm.chunkings(T):
            r = lag_run(name, L, C, cn)
            check_path(name, r, (name, L, C, cn))
            assert max(r["pending"]) <= lm.bound(L, C) and r["lag_max"] == max(r["pending"]), (name, L, C, cn)


@pytest.mark.parametrize("name", ["ds_K9_T7", "ds_K77_M7_T33", "ties_all_K64_T64", "circulant257", "rotor"])
def test_a_lag_of_one_checked_every_step_commits_at_every_check(name):
    T = len(case(name)[3])
    runs = {cn: lag_run(name, 1, 1, cn) for cn in ("1", "7", "T", "ragged")}
    for cn, r in runs.items():
        check_path(name, r, (name, cn))
        assert r["commits"] == r["checks"] == T - 1 and set(r["pending"]) <= {1}, (name, cn)
    # check_every = 1: the checks fall at every time whatever the chunking, and so does the result
    assert len({tuple(r["path"]) for r in runs.values()}) == 1
    assert len({(tuple(r["forced"]), r["score"].tobytes()) for r in runs.values()}) == 1


@pytest.mark.parametrize("name", ["cfg1_K128_T256", "cfg1_deadA", "ds_K77_M7_T33", "rotor_noise", "circulant257", "ties_all_K64_T64"])
def test_a_lag_never_reached_is_the_unbounded_stream(name):
    T = len(case(name)[3])
    row = tables(name)[0]
    for C in (4, 16):
        for cn in sm.chunkings(T):
            want = model_run(name, C, cn)
            for L in (T, T + 5, 0):
                r = lag_run(name, L, C, cn)
                assert r["lag"]["forced_commits"] == 0 and r["lag"]["first_forced_time"] == -1 and not r["pruned"].any()
                for key in ("pieces", "committed", "dead", "checks", "commits", "bt_restarts", "lag_max"):
                    assert r[key] == want[key], (name, C, cn, L, key)
                assert r["score"] == row.max()
    # (64, 16) on cfg1: the natural commits come first
    r = lag_run("cfg1_K128_T256", 64, 16, "7")
    assert r["lag"]["forced_commits"] == 0 and r["pieces"] == model_run("cfg1_K128_T256", 16, "7")["pieces"]


@pytest.mark.parametrize("name", ["rotor", "ties_all_K64_T64", "circulant257"])
def test_the_models_that_never_commit_now_commit(name):
    T = len(case(name)[3])
    for cn in ("7", "ragged"):
        assert model_run(name, 4, cn)["commits"] == 0 and model_run(name, 4, cn)["lag_max"] == T
        r = lag_run(name, 4, 4, cn)
        assert r["commits"] > 0 and r["lag"]["forced_commits"] > 0 and r["lag_max"] <= lm.bound(4, 4) < T
        assert r["committed"][-1] >= T - lm.bound(4, 4)


def test_the_pruned_model_is_what_the_rule_decodes():
    """path and score are the single pass over the model with the pruned cells' emissions at zero probability"""
    import oracle
    for name, L, C in (("rotor_noise", 8, 16), ("circulant257", 4, 4), ("ds_K77_M7_T33", 4, 4)):
        A, B, Pi, ob = case(name)
        r = lag_run(name, L, C, "7")
        assert r["pruned"].any()
        Bt, obt = lm.column_model(A, B, Pi, ob)
        Bt[r["pruned"].T] = 0
        om = oracle.OracleModel(A, Bt, Pi)
        path, score, _, rc = om.full_decode(obt, 1, check=False)
        assert (path.tolist(), np.float32(score).tobytes(), rc) == (r["path"], r["score"].tobytes(), 0), name
