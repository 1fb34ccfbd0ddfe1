"""GPU: fv_set_max_lag — lag-bounded online decodes against the CPU model of the rule (tests/lag_model.py), against the
one-shot decode of the pruned model, and against the unbounded stream where no commit is forced.  Equalities only.

Per case and per (max_lag, check_every): every piece, the committed and pending counts after every push, the score bits,
the return code, checks / commits / lag_max / bt_restarts and all five fv_lag_stats members equal the model's.  Shapes: K
below one wave, K not a multiple of 64, two workgroups with ties across them (circulant257), nine workgroups (K = 2053);
models that never commit without a bound; pushes of 1, 7, T and the ragged list."""
import numpy as np
import pytest

import lag_model as lm
import stream_model as sm
from flash_viterbi_amd import decoder
from test_gpu_emissions import libm_log
from test_gpu_stream import DENSE_KERNELS, bits, refused, run_stream
from test_gpu_streams import COUNTERS, even, ragged, run_set, schedule, slot_ob
from test_lag_model import GRID, lag_run
from test_stream_model import case

pytestmark = pytest.mark.gpu

D = decoder
CHUNKINGS = ("1", "7", "T", "ragged")
CASES = ["ds_K9_T7", "ds_K77_M7_T33", "cfg1_K128_T256", "cfg1_deadA", "circulant257", "ties_all_K64_T64", "rotor", "rotor_noise", "wideAB"]


@pytest.fixture(scope="module")
def ctx():
    made = {}

    def get(name, sparse=False):
        """(the context that streams, a second context: one-shot decodes and private single streams) on the case's model,
        no stream or set open, the default kernel, no lag bound"""
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
            if fv.streams_pending(0) >= 0:
                fv.streams_end()
            if fv.stream_pending() >= 0:
                fv.stream_abort()
            fv.set_option(D.OPT_KERNEL, D.KERNEL_AUTO)
            fv.set_option(D.OPT_MAX_BATCH, 8)
            fv.set_max_lag(0)
        return made[key]
    yield get
    for pair in made.values():
        for fv in pair:
            fv.close()


def run_lag(fv, max_lag, check_every, chunks, ob=None, feed=None, hint=0):
    """run_stream under fv_set_max_lag(max_lag), with the stream's fv_lag_stats (read after its close)"""
    fv.set_max_lag(max_lag)
    got = run_stream(fv, chunks, check_every, ob=ob, feed=feed, hint=hint)
    got["lag"] = fv.lag_stats()
    return got


def check_lag(got, want, chunks, tag):
    """got: run_lag's result; want: lag_model.run's"""
    assert got["dead"] is None and want["dead"] is None, tag
    assert got["committed"] == want["committed"], tag
    assert got["pieces"] == want["pieces"], tag
    # (run_stream asserted fv_stream_pending == consumed - committed after every push)
    assert [int(e) - c for e, c in zip(np.cumsum(chunks), got["committed"])] == want["pending"], tag
    assert (bits(got["score"]), got["rc"]) == (bits(want["score"]), 0), tag
    st = got["stats"]
    assert (st["checks"], st["commits"]) == (want["checks"], want["commits"]), tag
    assert (st["lag_max"], st["bt_restarts"]) == (want["lag_max"], want["bt_restarts"]), tag
    assert got["lag"] == want["lag"], tag
    T = sum(chunks)
    assert (st["times"], st["committed"], st["pushes"]) == (T, T, len(chunks)), tag


# ---------------------------------------------------------------- 1. the rule: every case, grid and chunking

@pytest.mark.parametrize("grid", GRID, ids=lambda g: "L%d_C%d" % g)
@pytest.mark.parametrize("name", CASES)
def test_every_chunking_matches_the_model(ctx, name, grid):
    L, C = grid
    fv, _ = ctx(name)
    ob = case(name)[3]
    forced = 0
    for cn in CHUNKINGS:
        chunks = sm.chunkings(len(ob))[cn]
        want = lag_run(name, L, C, cn)
        check_lag(run_lag(fv, L, C, chunks, ob=ob), want, chunks, (name, L, C, cn))
        assert max(want["pending"]) <= lm.bound(L, C)
        forced += want["lag"]["forced_commits"]
    if L <= 4:
        assert forced > 0, name               # the case exercises the forced branch


def test_nine_workgroups_all_ties(ctx):
    """K = 2053: nine workgroups fold the best key, every score tied: s* is state 0's column of the tie, on every check"""
    name = "circulant2053"
    fv, _ = ctx(name)
    ob = case(name)[3]
    assert len(ob) <= 64
    for cn in ("T", "7"):
        chunks = sm.chunkings(len(ob))[cn]
        want = lag_run(name, 16, 16, cn)
        if cn == "T":
            assert want["oracle_runs"] <= 4
        assert want["lag"]["forced_commits"] >= 2 and want["lag"]["pruned_states"] >= 2052
        check_lag(run_lag(fv, 16, 16, chunks, ob=ob), want, chunks, (name, cn))


# ---------------------------------------------------------------- 2. exact for the pruned model

@pytest.mark.parametrize("name,L,C", [("rotor_noise", 8, 16), ("circulant257", 4, 4), ("cfg1_K128_T256", 4, 4), ("ds_K77_M7_T33", 1, 1),
                                      ("cfg1_deadA", 8, 16), ("ties_all_K64_T64", 4, 4)])
def test_one_shot_decode_of_the_pruned_emissions(ctx, name, L, C):
    fv, ref_fv = ctx(name)
    A, B, Pi, ob = case(name)
    chunks = sm.chunkings(len(ob))["7"]
    want = lag_run(name, L, C, "7")
    got = run_lag(fv, L, C, chunks, ob=ob)
    check_lag(got, want, chunks, name)
    assert want["pruned"].any()
    E = np.ascontiguousarray(libm_log(B[:, ob]).T)
    E[want["pruned"]] = -np.inf
    ref_fv.set_emissions(E)
    try:
        res = ref_fv.decode_full(None, 1, D.MODE_SINGLE_PASS, T=len(ob))
    finally:
        ref_fv.clear_emissions()
    assert (res[0].tolist(), bits(res[1]), res[2]) == ([x for p in got["pieces"] for x in p], bits(got["score"]), got["rc"])


# ---------------------------------------------------------------- 3. kernels, CSR-set models, score rows; no forced commit

def same_as_unbounded(fv, chunks, check_every, tag, **how):
    """(64, 16)-like runs that force nothing, and max_lag = 0: run_stream's result member for member"""
    fv.set_max_lag(0)
    plain = run_stream(fv, chunks, check_every, **how)
    for L in (0, 64):
        got = run_lag(fv, L, check_every, chunks, **how)
        assert got["lag"] == dict(max_lag=L, forced_commits=0, pruned_states=0, first_forced_time=-1, last_forced_time=-1), tag
        for key in ("pieces", "committed", "dead", "rc"):
            assert got[key] == plain[key], (tag, L, key)
        assert bits(got["score"]) == bits(plain["score"]), (tag, L)
        for key in plain["stats"]:
            if key != "push_ms_total":
                assert got["stats"][key] == plain["stats"][key], (tag, L, key)
    return plain


def kernel_runs(fv, name, tag):
    A, B, Pi, ob = case(name)
    E = np.ascontiguousarray(libm_log(B[:, ob]).T)
    chunks = sm.chunkings(len(ob))["ragged"]
    want = lag_run(name, 4, 4, "ragged")
    assert want["lag"]["forced_commits"] > 0
    for how in (dict(ob=ob), dict(feed=lambda pos, n: E[pos:pos + n])):
        check_lag(run_lag(fv, 4, 4, chunks, **how), want, chunks, (tag, sorted(how)))
    c7 = sm.chunkings(len(ob))["7"]
    assert lag_run(name, 64, 16, "7")["lag"]["forced_commits"] == 0
    plain = same_as_unbounded(fv, c7, 16, tag, ob=ob)
    assert plain["pieces"] == lag_run(name, 64, 16, "7")["pieces"]
    return plain


@pytest.mark.parametrize("kernel", DENSE_KERNELS)
def test_every_dense_kernel(ctx, kernel):
    fv, _ = ctx("cfg1_K128_T256")
    fv.set_option(D.OPT_KERNEL, kernel)
    plain = kernel_runs(fv, "cfg1_K128_T256", kernel)
    if kernel not in (D.KERNEL_AUTO, D.KERNEL_SPARSE_Q16):
        assert plain["stats"]["kernel"] == kernel


@pytest.mark.parametrize("kernel", [D.KERNEL_AUTO, D.KERNEL_CSR_F64])
def test_csr_set_model(ctx, kernel):
    fv, _ = ctx("cfg1_K128_T256", sparse=True)
    fv.set_option(D.OPT_KERNEL, kernel)
    plain = kernel_runs(fv, "cfg1_K128_T256", ("csr", kernel))
    assert plain["stats"]["kernel"] == (D.KERNEL_CSR_F64 if kernel == D.KERNEL_CSR_F64 else D.KERNEL_SPARSE_CSR)


def test_a_bound_never_reached_on_the_other_cases(ctx):
    for name in ("rotor_noise", "ds_K77_M7_T33", "circulant257"):
        fv, _ = ctx(name)
        ob = case(name)[3]
        T = len(ob)
        for cn in ("7", "ragged"):
            chunks = sm.chunkings(T)[cn]
            fv.set_max_lag(0)
            plain = run_stream(fv, chunks, 16, ob=ob)
            got = run_lag(fv, T, 16, chunks, ob=ob)
            assert got["lag"]["forced_commits"] == 0 and got["lag"]["max_lag"] == T
            assert (got["pieces"], got["committed"], bits(got["score"]), got["rc"]) == (plain["pieces"], plain["committed"], bits(plain["score"]), plain["rc"])
            assert [got["stats"][k] for k in COUNTERS] == [plain["stats"][k] for k in COUNTERS]


# ---------------------------------------------------------------- 4. memory

def test_the_arg_rows_stay_within_the_bound(ctx):
    name = "rotor_noise"
    fv, _ = ctx(name)
    ob = case(name)[3]
    assert len(ob) == 300
    chunks = sm.chunkings(300)["7"]
    want = lag_run(name, 8, 16, "7")
    got = run_lag(fv, 8, 16, chunks, ob=ob, hint=1)
    check_lag(got, want, chunks, name)
    assert lm.bound(8, 16) == 30 and max(want["pending"]) <= 30
    assert got["stats"]["arg_rows_capacity"] <= 2 * (30 + 7)
    # the same pushes without a bound on a model that never merges in time: everything stays pending
    fv2, _ = ctx("rotor")
    got = run_lag(fv2, 0, 16, chunks, ob=case("rotor")[3], hint=1)
    assert got["stats"]["lag_max"] == 300 and got["stats"]["arg_rows_capacity"] >= 300
    got = run_lag(fv2, 8, 16, chunks, ob=case("rotor")[3], hint=1)
    assert got["stats"]["lag_max"] <= 30 and got["stats"]["arg_rows_capacity"] <= 2 * (30 + 7)
    got = run_lag(fv, 0, 16, chunks, ob=ob, hint=1)
    assert got["stats"]["lag_max"] > 30


# ---------------------------------------------------------------- 5. sets

def expected_check_launches(calls, check_every, per_check):
    """(check_launches, check_slots) of the calls of a set: the slots that come due in one lock-step share launches of up to
    eight slots, per_check launches each"""
    times, since, launches, slots = {}, {}, 0, 0
    for call in calls:
        for i in range(max(n for _, n in call)):
            due = 0
            for s, n in call:
                if i >= n:
                    continue
                if times.get(s, 0) + i > 0:
                    since[s] = since.get(s, 0) + 1
                if since.get(s, 0) > 0 and (since[s] == check_every or i == n - 1):
                    since[s] = 0
                    due += 1
            launches += per_check * ((due + 7) // 8)
            slots += due
        for s, n in call:
            times[s] = times.get(s, 0) + n
    return launches, slots


@pytest.mark.parametrize("max_lag", [4, 8])
@pytest.mark.parametrize("S", [1, 3, 9])
def test_sets_match_private_single_streams(ctx, S, max_lag):
    name = "rotor_noise" if max_lag == 8 else "cfg1_K128_T256"
    C = 16 if max_lag == 8 else 4
    fv, ref_fv = ctx(name)
    obs = [slot_ob(case(name)[3], s) for s in range(S)]
    forced = 0
    for form in ("ragged", "staggered"):
        chunks = [ragged(len(o), s) for s, o in enumerate(obs)] if form == "ragged" else [even(len(o), 7) for o in obs]
        calls = schedule(chunks, list(range(S)) if form == "staggered" else None)
        fv.set_max_lag(max_lag)
        got = run_set(fv, S, calls, C, obs=obs)
        assert (got["set"]["check_launches"], got["set"]["check_slots"]) == expected_check_launches(calls, C, 3), (S, form)
        for s in range(S):
            single = run_lag(ref_fv, max_lag, C, chunks[s], ob=obs[s])
            tag = (S, max_lag, form, s)
            assert got[s]["pieces"] == single["pieces"] and got[s]["committed"] == single["committed"], tag
            assert (bits(got[s]["score"]), got[s]["rc"]) == (bits(single["score"]), single["rc"]), tag
            assert [got[s]["stats"][k] for k in COUNTERS] == [single["stats"][k] for k in COUNTERS], tag
            assert fv.lag_stats(s) == single["lag"] and single["lag"]["max_lag"] == max_lag, tag       # (the last set ended)
            assert max(e - c for e, c in zip(np.cumsum(chunks[s]), got[s]["committed"])) <= lm.bound(max_lag, C), tag
            forced += single["lag"]["forced_commits"]
        if S == 1:                            # slot 0 decodes the case's own sequence: the model's run
            cn = "ragged" if form == "ragged" else "7"
            want = lag_run(name, max_lag, C, cn)
            assert got[0]["pieces"] == want["pieces"] and fv.lag_stats(0) == want["lag"]
    assert forced > 0
    # an unbounded set on the same calls: two launches per check
    fv.set_max_lag(0)
    got = run_set(fv, S, calls, C, obs=obs)
    assert (got["set"]["check_launches"], got["set"]["check_slots"]) == expected_check_launches(calls, C, 2)
    assert fv.lag_stats(0)["forced_commits"] == 0 and fv.lag_stats(0)["max_lag"] == 0


def test_a_slot_closed_and_restarted_in_mid_run(ctx):
    name, L, C, T1 = "rotor_noise", 4, 4, 40
    fv, ref_fv = ctx(name)
    obs = [slot_ob(case(name)[3], s) for s in range(3)]
    fv.set_max_lag(L)
    fv.streams_open(3, 0, C)
    try:
        first, _ = fv.streams_push([0, 1, 2], obs=[o[:T1] for o in obs])
        piece, score, rc = fv.streams_close(1)
        single = run_lag(ref_fv, L, C, [T1], ob=obs[1][:T1])
        assert [first[1].tolist(), piece.tolist()] == single["pieces"] and (bits(score), rc) == (bits(single["score"]), single["rc"])
        assert fv.lag_stats(1) == single["lag"] and single["lag"]["forced_commits"] > 0       # the sequence that left the slot
        # slot 1 starts over on slot 2's observations while the others go on
        second, _ = fv.streams_push([0, 1, 2], obs=[obs[0][T1:T1 + 33], obs[2][:33], obs[2][T1:T1 + 33]])
        rest = [obs[0][T1 + 33:], obs[2][33:], obs[2][T1 + 33:]]
        third, _ = fv.streams_push([2, 0, 1], obs=[rest[2], rest[0], rest[1]])
        third = [third[1], third[2], third[0]]
        for s, seq, pushes in ((0, obs[0], [T1, 33, len(rest[0])]), (1, obs[2], [33, len(rest[1])]), (2, obs[2], [T1, 33, len(rest[2])])):
            piece, score, rc = fv.streams_close(s)
            single = run_lag(ref_fv, L, C, pushes, ob=seq)
            mine = ([first[s].tolist()] if s != 1 else []) + [second[s].tolist(), third[s].tolist(), piece.tolist()]
            assert mine == single["pieces"] and (bits(score), rc) == (bits(single["score"]), single["rc"]), s
            assert fv.lag_stats(s) == single["lag"], s
            st = fv.streams_slot_stats(s)
            assert [st[k] for k in COUNTERS] == [single["stats"][k] for k in COUNTERS], s
    finally:
        if fv.streams_pending(0) >= 0:
            fv.streams_end()


# ---------------------------------------------------------------- 6. the setter

def test_setter_refusals_and_life_cycle(ctx):
    fresh = D.FlashViterbi(0)
    try:
        refused(lambda: fresh.lag_stats(), D.ERR_STATE)                        # there never was a stream
        refused(lambda: fresh.lag_stats(0), D.ERR_STATE)                       # ... nor a set
        refused(lambda: fresh.set_max_lag(-1), D.ERR_ARG)
        fresh.set_max_lag(5)                                                   # no model needed; kept across fv_set_model*
        A, B, Pi, ob = case("ds_K9_T7")
        fresh.set_model(A, B, Pi)
        fresh.stream_open(0, 4)
        assert fresh.lag_stats() == dict(max_lag=5, forced_commits=0, pruned_states=0, first_forced_time=-1, last_forced_time=-1)
        fresh.stream_abort()
        fresh.set_model_sparse(*D.dense_to_csr(A), B, Pi)
        fresh.streams_open(2, 0, 4)
        assert fresh.lag_stats(1)["max_lag"] == 5
        refused(lambda: fresh.lag_stats(2), D.ERR_ARG)
        fresh.streams_end()
        assert fresh.lag_stats(1)["max_lag"] == 5
        refused(lambda: fresh.lag_stats(2), D.ERR_ARG)
    finally:
        fresh.close()
    fv, _ = ctx("ds_K77_M7_T33")
    ob = case("ds_K77_M7_T33")[3]
    fv.set_max_lag(4)
    fv.stream_open(0, 4)
    assert "stream is open" in refused(lambda: fv.set_max_lag(8), D.ERR_STATE)
    refused(lambda: fv.set_max_lag(-1), D.ERR_ARG)
    fv.stream_push(ob=ob[:20])
    assert fv.lag_stats()["max_lag"] == 4                                      # the open stream's
    fv.stream_abort()
    assert fv.lag_stats()["max_lag"] == 4                                      # the last one aborted
    fv.streams_open(2, 0, 4)
    assert "set of streams is open" in refused(lambda: fv.set_max_lag(8), D.ERR_STATE)
    fv.streams_end()
    fv.set_max_lag(8)
    fv.stream_open(0, 4)
    assert fv.lag_stats()["max_lag"] == 8
    fv.stream_abort()
