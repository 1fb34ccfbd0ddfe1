"""GPU: fv_streams_* — a set of online streams on one context, the slots of a push call stepped together — against the CPU
model of the commit rule (tests/stream_model.py, one sm.Stream per slot), against the same pushes through fv_stream_* on a
second context, and against that context's one-shot single-pass decode.

Every comparison is an equality.  Per slot: every piece and so the committed count after every call the slot took part in;
checks, commits, lag_max and bt_restarts of the slot's statistics; the concatenation, the score (as uint32) and the return
code.  The set's own counters (step launches, task steps, check launches, slot-checks, meetings with the device) tell a set
from a loop over single streams.  Slots of one set share a model: slot s decodes a rotated, shortened copy of the case's
observations (slot_ob), so no two slots carry the same sequence or the same length."""
import functools

import numpy as np
import pytest

import stream_model as sm
from conftest import load_goldens
from flash_viterbi_amd import decoder
from test_gpu_emissions import libm_log
from test_gpu_stream import DENSE_KERNELS, Scores, bits, refused, run_stream
from test_stream_model import CHECKS, case, tables

pytestmark = pytest.mark.gpu

D = decoder


def slot_ob(ob, s):
    """slot s's sequence: np.roll(ob, 37 * s)[:T - 13 * s]; a case too short for that: rolled by s, one time shorter per slot"""
    T = len(ob)
    if T > 13 * 9:
        return np.ascontiguousarray(np.roll(ob, 37 * s)[:T - 13 * s])
    return np.ascontiguousarray(np.roll(ob, s)[:max(2, T - s % T)])


@functools.lru_cache(maxsize=None)
def slot_tables(name, s):
    """(last row, arg table, single-pass path) of slot s's sequence from the oracle (slot 0: the case's own)"""
    if s == 0:
        return tables(name)
    import oracle
    A, B, Pi, ob = case(name)
    o = slot_ob(ob, s)
    row, args = oracle.OracleModel(A, B, Pi).full_forward(o, 0, len(o) - 1, -1)
    return row, args, sm.single_pass_path(row, args)


@functools.lru_cache(maxsize=None)
def slot_model(name, s, check_every, chunks):
    row, args, _ = slot_tables(name, s)
    return sm.run(args, row, check_every, list(chunks))


def even(T, n):
    return [n] * (T // n) + ([T % n] if T % n else [])


def ragged(T, s):
    """sm.chunkings' ragged list, rotated by the slot index (the lengths still add up to T)"""
    c = sm.chunkings(T)["ragged"]
    return c[s % len(c):] + c[:s % len(c)]


def schedule(chunks, delay=None):
    """The calls of a set: call c names every slot s that has a chunk number c - delay[s], in slot order."""
    delay = delay or [0] * len(chunks)
    ncalls = max(d + len(c) for d, c in zip(delay, chunks))
    calls = [[(s, chunks[s][c - delay[s]]) for s in range(len(chunks)) if 0 <= c - delay[s] < len(chunks[s])] for c in range(ncalls)]
    return [c for c in calls if c]


@pytest.fixture(scope="module")
def ctx():
    made = {}

    def get(name, sparse=False):
        """(the context that holds the set, the context of the single streams and the one-shot decodes) on the case's model"""
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
        return made[key]
    yield get
    for pair in made.values():
        for fv in pair:
            fv.close()


def run_set(fv, nslots, calls, check_every, obs=None, feed=None, hint=0, keep_open=False):
    """The calls through one set, then a close of every slot that took part.  Per slot the shape of run_stream's result;
    also the set's statistics.  feed(call): the scores argument of streams_push for that call."""
    fv.streams_open(nslots, hint, check_every)
    out = {}
    pos, done = {}, {}
    try:
        for call in calls:
            ids = [s for s, _ in call]
            for s in ids:
                if s not in out:
                    out[s] = dict(pieces=[], committed=[], dead=None, score=None, rc=None)
                    pos[s] = done[s] = 0
            if feed is None:
                pieces, status = fv.streams_push(ids, obs=[obs[s][pos[s]:pos[s] + n] for s, n in call])
            else:
                pieces, status = fv.streams_push(ids, scores=feed(call, pos))
            assert status == [0] * len(ids)
            for (s, n), piece in zip(call, pieces):
                pos[s] += n
                done[s] += piece.size
                out[s]["pieces"].append(piece.tolist())
                out[s]["committed"].append(done[s])
                assert fv.streams_pending(s) == pos[s] - done[s]
        for s in out:
            piece, out[s]["score"], out[s]["rc"] = fv.streams_close(s)
            out[s]["pieces"].append(piece.tolist())
            out[s]["stats"] = fv.streams_slot_stats(s)
            assert fv.streams_pending(s) == 0
        out["set"] = fv.streams_stats()
    finally:
        if not keep_open and fv.streams_pending(0) >= 0:
            fv.streams_end()
    return out


COUNTERS = ("times", "committed", "pushes", "checks", "commits", "lag_max", "bt_restarts")


def check_slot(got, want, single, ref, tag):
    """got: a slot of run_set's result; want: the model's run; single: run_stream's result for the same pushes on a context
    of its own; ref: (path list, score bits, rc) of the one-shot decode"""
    assert got["committed"] == want["committed"] == single["committed"], tag
    assert got["pieces"] == want["pieces"] == single["pieces"], tag
    assert ([x for p in got["pieces"] for x in p], bits(got["score"]), got["rc"]) == ref, tag
    assert (bits(got["score"]), got["rc"]) == (bits(single["score"]), single["rc"]), tag
    st = got["stats"]
    assert (st["checks"], st["commits"], st["lag_max"], st["bt_restarts"]) == (want["checks"], want["commits"], want["lag_max"], want["bt_restarts"]), tag
    assert [st[k] for k in COUNTERS] == [single["stats"][k] for k in COUNTERS], tag
    assert st["kernel"] == single["stats"]["kernel"] and st["push_ms_total"] > 0, tag


class Expect:
    """what the second context makes of slot s's sequence: the single stream over given pushes and the one-shot decode, each
    computed once per (case, slot, kernel, ...) and shared"""

    def __init__(self, name, ref_fv, kernel=D.KERNEL_AUTO, oracle_tables=True):
        self.name, self.fv, self.kernel, self.oracle = name, ref_fv, kernel, oracle_tables
        self.singles, self.shots = {}, {}
        self.ob = case(name)[3]

    def seq(self, s):
        return slot_ob(self.ob, s)

    def single(self, s, check_every, chunks, hint=0):
        key = (s, check_every, tuple(chunks), hint)
        if key not in self.singles:
            self.singles[key] = run_stream(self.fv, chunks, check_every, ob=self.seq(s), hint=hint)
        return self.singles[key]

    def one_shot(self, s):
        if s not in self.shots:
            res = self.fv.decode_full(self.seq(s), 1, D.MODE_SINGLE_PASS)
            self.shots[s] = (res[0].tolist(), bits(res[1]), res[2])
            if self.oracle:
                row, _, path = slot_tables(self.name, s)
                assert self.shots[s] == (path, bits(row[path[-1]]), 0), (self.name, s)
        return self.shots[s]


def run_and_check(fv, ex, chunks, check_every, delay=None, hint=0, tag=None):
    """S = len(chunks) slots, slot s pushed in the lengths chunks[s]; every slot checked against model, single stream, one shot"""
    S = len(chunks)
    obs = [ex.seq(s) for s in range(S)]
    got = run_set(fv, S, schedule(chunks, delay), check_every, obs=obs, hint=hint)
    for s in range(S):
        check_slot(got[s], slot_model(ex.name, s, check_every, tuple(chunks[s])), ex.single(s, check_every, chunks[s], hint),
                   ex.one_shot(s), (tag, s))
    return got


# ---------------------------------------------------------------- 1. grouping: slot counts, call schedules, check intervals

GROUPING = ["cfg1_K128_T256", "ds_K77_M7_T33", "ds_K5_T3", "ties_all_K64_T64", "cfg1_deadB"]
_expect = {}


def expect(name, ref_fv, kernel=D.KERNEL_AUTO, sparse=False):
    key = (name, kernel, sparse)
    if key not in _expect or _expect[key].fv is not ref_fv:
        _expect[key] = Expect(name, ref_fv, kernel)
    return _expect[key]


@pytest.mark.parametrize("check_every", CHECKS)
@pytest.mark.parametrize("name", GROUPING)
def test_grouping_matches_model_single_stream_and_one_shot(ctx, name, check_every):
    fv, ref_fv = ctx(name)
    ex = expect(name, ref_fv)
    for S in (1, 3, 8, 9):                    # 3: an idle task in the NB = 4 launch; 9: a second launch of one task
        lens = [len(ex.seq(s)) for s in range(S)]
        for n in (1, 7, 64):                  # (a) every slot in every call, the same length (but for the last chunks)
            run_and_check(fv, ex, [even(T, n) for T in lens], check_every, tag=(name, check_every, S, "a", n))
        # (b) per-slot ragged lengths: the calls name different subsets, the slots come due at different lock-steps
        got = run_and_check(fv, ex, [ragged(T, s) for s, T in enumerate(lens)], check_every, tag=(name, check_every, S, "b"))
        assert got["set"]["nslots"] == S and got["set"]["batch_cap"] == 8
        # (c) staggered starts: slot s gets its first push in call s, so time parities and check phases differ
        run_and_check(fv, ex, [even(T, 7) for T in lens], check_every, delay=list(range(S)), tag=(name, check_every, S, "c"))


# ---------------------------------------------------------------- 2. the sharing is real

def test_slots_share_step_launches_checks_and_meetings(ctx):
    name = "cfg1_K128_T256"
    fv, ref_fv = ctx(name)
    ex = expect(name, ref_fv)
    S = 8
    obs = [ex.seq(s) for s in range(S)]
    results = {}
    for cap, launches in ((8, 64), (2, 256), (1, 512)):
        fv.set_option(D.OPT_MAX_BATCH, cap)
        fv.streams_open(S, 0, 16)
        try:
            first, _ = fv.streams_push(list(range(S)), obs=[o[:16] for o in obs])
            before = fv.streams_stats()
            pieces, status = fv.streams_push(list(range(S)), obs=[o[16:80] for o in obs])
            after = fv.streams_stats()
            slot = [fv.streams_slot_stats(s) for s in range(S)]
        finally:
            fv.streams_end()
        d = {k: after[k] - before[k] for k in ("calls", "step_launches", "task_steps", "check_launches", "check_slots", "syncs")}
        assert (d["calls"], d["step_launches"], d["task_steps"]) == (1, launches, 512), (cap, d)
        assert (d["check_launches"], d["check_slots"]) == (8, 32), (cap, d)
        assert d["syncs"] <= 2, (cap, d)
        assert after["batch_cap"] == cap and status == [0] * S
        results[cap] = ([p.tolist() for p in first], [p.tolist() for p in pieces], [(x["checks"], x["commits"]) for x in slot])
    fv.set_option(D.OPT_MAX_BATCH, 8)
    assert results[8] == results[2] == results[1]
    # ... and what all three delivered is the rule's: the first two pieces of every slot
    streams = []
    for s in range(S):
        row, args, _ = slot_tables(name, s)
        m = sm.Stream(args, row, 16)
        streams.append(([m.push(16)], [m.push(64)], (m.checks, m.commits)))
    assert results[8] == ([a[0] for a, _, _ in streams], [b[0] for _, b, _ in streams], [c for _, _, c in streams])
    assert sum(len(p) for p in results[8][1]) > 0


# ---------------------------------------------------------------- 3. slot life cycle

def test_slots_close_abort_and_start_over_while_others_run(ctx):
    name = "cfg1_K128_T256"
    fv, ref_fv = ctx(name)
    ex = expect(name, ref_fv)
    obs = [ex.seq(s) for s in range(3)]
    T1 = 40                                   # slot 1's first sequence: the first 40 times of its observations
    fv.streams_open(3, 0, 4)
    try:
        models = []
        for s in range(3):
            row, args, _ = slot_tables(name, s)
            models.append(sm.Stream(args, row, 4))
        got = [[], [], []]
        pieces, _ = fv.streams_push([0, 1, 2], obs=[o[:T1] for o in obs])
        for s in range(3):
            got[s].append(pieces[s].tolist())
            assert got[s][-1] == models[s].push(T1)
        # close slot 1 in mid-run of the others: the one-shot decode of its first 40 times
        piece, score, rc = fv.streams_close(1)
        res = ref_fv.decode_full(obs[1][:T1], 1, D.MODE_SINGLE_PASS)
        assert (got[1][0] + piece.tolist(), bits(score), rc) == (res[0].tolist(), bits(res[1]), res[2])
        assert fv.streams_pending(1) == 0 and fv.streams_slot_stats(1)["committed"] == T1
        # closing the empty slot delivers nothing
        piece, score, rc = fv.streams_close(1)
        assert piece.size == 0 and rc == 0
        # the others go on; slot 1 starts a new sequence (slot 2's observations from time 0: another parity than its neighbours)
        row, args, _ = slot_tables(name, 2)
        models[1] = sm.Stream(args, row, 4)
        pieces, _ = fv.streams_push([0, 1, 2], obs=[obs[0][T1:T1 + 33], obs[2][:33], obs[2][T1:T1 + 33]])
        assert [p.tolist() for p in pieces] == [models[0].push(33), models[1].push(33), models[2].push(33)]
        assert fv.streams_slot_stats(1)["times"] == 33 and fv.streams_slot_stats(1)["pushes"] == 1
        # abort slot 0: it is empty again, the others are where they were
        fv.streams_abort(0)
        assert [fv.streams_pending(s) for s in range(3)] == [0, models[1].pending(), models[2].pending()]
        fv.streams_abort(0)                   # (an empty slot: nothing to drop)
        rest = len(obs[2]) - (T1 + 33)
        pieces, _ = fv.streams_push([2, 0, 1], obs=[obs[2][T1 + 33:], obs[0][:rest], obs[2][33:33 + rest]])
        row0, args0, _ = slot_tables(name, 0)
        models[0] = sm.Stream(args0, row0, 4)
        assert [p.tolist() for p in pieces] == [models[2].push(rest), models[0].push(rest), models[1].push(rest)]
        # slot 2 has consumed its whole sequence: its close completes the one-shot path
        piece, score, rc = fv.streams_close(2)
        assert piece.tolist() == models[2].close()
        assert (bits(score), rc) == ex.one_shot(2)[1:]
        assert fv.streams_slot_stats(2)["bt_restarts"] == models[2].bt_restarts
        # the set ends with sequences pending in slots 0 and 1
        assert fv.streams_pending(0) > 0 and fv.streams_pending(1) > 0
        fv.streams_end()
        assert fv.streams_pending(0) == -1
        refused(lambda: fv.streams_end(), D.ERR_STATE)
        assert fv.streams_stats()["calls"] == 3          # the last set's statistics stay
        # the context is free again
        res = fv.decode_full(obs[0], 1, D.MODE_SINGLE_PASS)
        assert (res[0].tolist(), bits(res[1]), res[2]) == ex.one_shot(0)
    finally:
        if fv.streams_pending(0) >= 0:
            fv.streams_end()


def test_destroy_with_a_set_open():
    A, B, Pi, ob = case("ds_K9_T7")
    gone = D.FlashViterbi(0)
    try:
        gone.set_model(A, B, Pi)
        gone.streams_open(4)
        gone.streams_push([0, 3], obs=[ob[:4], ob[:5]])
    finally:
        gone.close()                          # fv_destroy frees the open set
    fresh = D.FlashViterbi(0)
    try:
        fresh.set_model(A, B, Pi)
        fresh.streams_open(1)
        pieces, _ = fresh.streams_push([0], obs=[ob])
        piece, score, rc = fresh.streams_close(0)
        fresh.streams_end()
        res = fresh.decode_full(ob, 1, D.MODE_SINGLE_PASS)
        assert (pieces[0].tolist() + piece.tolist(), bits(score), rc) == (res[0].tolist(), bits(res[1]), res[2])
    finally:
        fresh.close()


# ---------------------------------------------------------------- 4. one dead slot among three

def test_one_dead_slot_does_not_disturb_the_others(ctx):
    name = "no_emitter"                       # nobody emits symbol 2
    fv, ref_fv = ctx(name)
    A, B, Pi, ob = case(name)
    import oracle
    om = oracle.OracleModel(A, B, Pi)
    live = ob.copy()
    live[live == 2] = 3                       # the case's sequence without its one symbol 2: decodable
    seqs = [live, ob, np.ascontiguousarray(np.roll(live, 5)[:30])]         # slot 1 observes symbol 2 at time 20
    refused(lambda: ref_fv.decode_full(seqs[1], 1, D.MODE_SINGLE_PASS), D.ERR_NO_PRED)
    models, shots = {}, {}
    for s in (0, 2):
        row, args = om.full_forward(seqs[s], 0, len(seqs[s]) - 1, -1)
        models[s] = sm.Stream(args, row, 4)
        res = ref_fv.decode_full(seqs[s], 1, D.MODE_SINGLE_PASS)
        shots[s] = (res[0].tolist(), bits(res[1]), res[2])
    row1, args1, _ = tables(name)
    models[1] = sm.Stream(args1, row1, 4)
    fv.streams_open(3, 0, 4)
    try:
        got = {0: [], 1: [], 2: []}
        pieces, status = fv.streams_push([0, 1, 2], obs=[q[:12] for q in seqs])
        assert status == [0, 0, 0]
        for s in range(3):
            got[s] += pieces[s].tolist()
            assert pieces[s].tolist() == models[s].push(12)
        # the call that consumes slot 1's time 20: that slot dies, the call reports it, the others get their pieces
        ids = np.array([0, 1, 2], np.int32)
        cat = np.concatenate([q[12:24] for q in seqs]).astype(np.int32)
        offsets = np.array([0, 12, 24, 36], np.int64)
        room = np.zeros(4, np.int64)
        for q in range(3):
            room[q + 1] = room[q] + fv.streams_pending(q) + 12
        path = np.empty(int(room[-1]), np.int32)
        done, stat = np.zeros(3, np.int64), np.zeros(3, np.int32)
        P = lambda a: a.ctypes.data_as(D.ctypes.c_void_p)
        rc = fv._L.fv_streams_push(fv._h, P(ids), 3, P(cat), P(offsets), P(path), P(room), P(done), P(stat))
        assert rc == D.ERR_NO_PRED and stat.tolist() == [0, D.ERR_NO_PRED, 0] and done[1] == 0
        assert models[1].push(12) is None
        for s in (0, 2):
            piece = path[room[s]:room[s] + done[s]].tolist()
            got[s] += piece
            assert piece == models[s].push(12)
        st1 = fv.streams_slot_stats(1)
        assert (st1["checks"], st1["commits"], st1["times"]) == (models[1].checks, models[1].commits, 24)
        # naming the dead slot refuses the call and consumes nothing anywhere
        pend = [fv.streams_pending(s) for s in range(3)]
        assert "slot 1" in refused(lambda: fv.streams_push([0, 1, 2], obs=[seqs[0][24:], seqs[1][24:], seqs[2][24:]]), D.ERR_STATE)
        assert [fv.streams_pending(s) for s in range(3)] == pend
        assert [fv.streams_slot_stats(s)["times"] for s in range(3)] == [24, 24, 24]
        # the other two are exact to the end
        pieces, status = fv.streams_push([2, 0], obs=[seqs[2][24:], seqs[0][24:]])
        assert status == [0, 0]
        got[2] += pieces[0].tolist()
        got[0] += pieces[1].tolist()
        assert pieces[0].tolist() == models[2].push(len(seqs[2]) - 24) and pieces[1].tolist() == models[0].push(len(seqs[0]) - 24)
        for s in (0, 2):
            piece, score, rc = fv.streams_close(s)
            assert piece.tolist() == models[s].close()
            assert (got[s] + piece.tolist(), bits(score), rc) == shots[s]
        # the dead slot's close delivers nothing; afterwards the slot takes a new sequence
        piece, score, rc = fv.streams_close(1)
        assert piece.size == 0 and rc == D.ERR_NO_PRED and fv.streams_pending(1) == 0
        pieces, status = fv.streams_push([1], obs=[seqs[0]])
        piece, score, rc = fv.streams_close(1)
        assert (pieces[0].tolist() + piece.tolist(), bits(score), rc) == shots[0]
    finally:
        fv.streams_end()


# ---------------------------------------------------------------- 5. several workgroups times several slots

def test_nine_workgroups_two_slots_all_ties(ctx):
    name = "circulant2053"
    fv, ref_fv = ctx(name)
    ex = expect(name, ref_fv)
    lens = [len(ex.seq(s)) for s in range(2)]
    for ce, chunks in ((16, [even(T, 7) for T in lens]), (4, [ragged(T, s) for s, T in enumerate(lens)])):
        got = run_and_check(fv, ex, chunks, ce, tag=(name, ce))
        for s in range(2):
            assert got[s]["stats"]["commits"] == 0 and len(got[s]["pieces"][-1]) == lens[s]


def test_cfg2_eight_slots_in_pushes_of_64(ctx):
    """K = 3965: sixteen workgroups per slot, eight slots per check launch.  (The oracle's pass over this model takes the CPU
    long: the expectation is the second context's single streams and one-shot decodes, and the golden's path for slot 0.)"""
    name = "cfg2_K3965_T256"
    fv, ref_fv = ctx(name)
    ex = Expect(name, ref_fv, oracle_tables=False)
    g = next(g for g in load_goldens(True) if g["name"] == name)
    stored = next(r for r in g["runs"] if r["algo"] == "flash" and r["N"] == 1)
    assert ex.one_shot(0)[0] == stored["path"] and ex.one_shot(0)[2] == 0
    S = 8
    chunks = [even(len(ex.seq(s)), 64) for s in range(S)]
    got = run_set(fv, S, schedule(chunks), 16, obs=[ex.seq(s) for s in range(S)])
    for s in range(S):
        single = ex.single(s, 16, chunks[s])
        assert got[s]["pieces"] == single["pieces"] and got[s]["committed"] == single["committed"], s
        assert ([x for p in got[s]["pieces"] for x in p], bits(got[s]["score"]), got[s]["rc"]) == ex.one_shot(s), s
        assert [got[s]["stats"][k] for k in COUNTERS] == [single["stats"][k] for k in COUNTERS], s
        assert got[s]["stats"]["commits"] > 0
    assert got["set"]["task_steps"] == sum(len(ex.seq(s)) - 1 for s in range(S))
    assert got["set"]["step_launches"] == 255 and got["set"]["batch_cap"] == 8


# ---------------------------------------------------------------- 6. kernels

@pytest.mark.parametrize("kernel", DENSE_KERNELS)
def test_every_dense_kernel(ctx, kernel):
    name = "cfg1_K128_T256"
    fv, ref_fv = ctx(name)
    for f in (fv, ref_fv):
        f.set_option(D.OPT_KERNEL, kernel)
    ex = expect(name, ref_fv, kernel)
    got = run_and_check(fv, ex, [ragged(len(ex.seq(s)), s) for s in range(3)], 4, tag=kernel)
    assert got["set"]["kernel"] == ref_fv.stats()["kernel"] == got[0]["stats"]["kernel"]
    if kernel not in (D.KERNEL_AUTO, D.KERNEL_SPARSE_Q16):
        assert got["set"]["kernel"] == kernel


@pytest.mark.parametrize("kernel", [D.KERNEL_AUTO, D.KERNEL_CSR_F64])
@pytest.mark.parametrize("name", ["ds_K200_T100", "cfg1_deadA"])
def test_sparse_set_models(ctx, name, kernel):
    fv, ref_fv = ctx(name, sparse=True)
    for f in (fv, ref_fv):
        f.set_option(D.OPT_KERNEL, kernel)
    ex = expect(name, ref_fv, kernel, sparse=True)
    got = run_and_check(fv, ex, [ragged(len(ex.seq(s)), s) for s in range(3)], 16, tag=(name, kernel))
    assert got["set"]["kernel"] == (D.KERNEL_CSR_F64 if kernel == D.KERNEL_CSR_F64 else D.KERNEL_SPARSE_CSR)
    # a kernel that streams a dense table is refused at open, as the one-shot decode refuses it
    fv.set_option(D.OPT_KERNEL, D.KERNEL_F64_STREAM)
    assert "no dense table" in refused(lambda: fv.streams_open(3), D.ERR_UNSUPPORTED)
    assert fv.streams_pending(0) == -1


# ---------------------------------------------------------------- 7. score rows

class SlotScores:
    """Three slots of score rows cut from one Scores block (test_gpu_stream.py): slot s's rows are the block's rows rolled by
    37 * s and shortened by 13 * s.  reference(s): what the second context makes of slot s's rows in one block — set_emissions
    + the one-shot decode, and the arg table of that pass for the model — as test_score_rows builds it."""

    def __init__(self, sc):
        self.sc = sc
        self.blocks = [np.ascontiguousarray(np.roll(sc.block, 37 * s, axis=0)[:sc.T - 13 * s]) for s in range(3)]
        self.live = []

    def reference(self, s):
        ref_fv, b = self.sc.pair[1], self.blocks[s]
        ref_fv.set_emissions((b.ctypes.data, self.sc.code, b.shape[0], self.sc.ld))
        res = ref_fv.decode_full(None, 1, D.MODE_SINGLE_PASS, T=b.shape[0])
        rows, bp, _ = ref_fv.test_forward(None, [(0, b.shape[0] - 1, -1)], T=b.shape[0])
        return (res[0].tolist(), bits(res[1]), res[2]), rows[0], bp[1:]

    def feed(self, call, pos):
        """the call's rows packed end to end, as a host pointer or (the device form) a device block of its own"""
        packed = np.ascontiguousarray(np.concatenate([self.blocks[s][pos[s]:pos[s] + n] for s, n in call]))
        self.live.append(packed)
        ptr = packed.ctypes.data
        if self.sc.device:
            ptr = self.sc.pair[0].test_device_alloc(packed)
            self.live.append(("device", ptr))
        return ((ptr, self.sc.code, packed.shape[0], self.sc.ld), [n for _, n in call])

    def close(self):
        for x in self.live:
            if isinstance(x, tuple):
                self.sc.pair[0].test_device_free(x[1])
        self.sc.close()


def check_scores(ss, check_every, tag):
    lens = [b.shape[0] for b in ss.blocks]
    chunks = [ragged(T, s) for s, T in enumerate(lens)]
    got = run_set(ss.sc.pair[0], 3, schedule(chunks), check_every, feed=ss.feed)
    for s in range(3):
        ref, row, args = ss.reference(s)
        assert ref[2] == 0
        want = sm.run(args, row, check_every, chunks[s])
        assert got[s]["pieces"] == want["pieces"] and got[s]["committed"] == want["committed"], (tag, s)
        assert ([x for p in got[s]["pieces"] for x in p], bits(got[s]["score"]), got[s]["rc"]) == ref, (tag, s)
        st = got[s]["stats"]
        assert (st["checks"], st["commits"], st["lag_max"], st["bt_restarts"]) == (want["checks"], want["commits"], want["lag_max"], want["bt_restarts"]), (tag, s)
    return got


@pytest.mark.parametrize("form", ["f32", "f64", "f16", "bf16", "f32_ld", "f32_device"])
def test_score_rows(form):
    ss = SlotScores(Scores("ds_K200_T100", form))
    try:
        got = check_scores(ss, 4, form)
        ncalls = got["set"]["calls"]
        assert got["set"]["syncs"] <= 3 * ncalls + 3 + sum(got[s]["stats"]["regrows"] for s in range(3))      # flags, records, pieces; three closes
        assert ss.sc.pair[0].stats()["emission_rows"] == 0          # the context's own staged rows are left alone
    finally:
        ss.close()


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
        blocks = [np.ascontiguousarray(np.roll(logs, 37 * s, axis=0)[:T - 13 * s]) for s in range(3)]
        chunks = [ragged(b.shape[0], s) for s, b in enumerate(blocks)]
        # (the list form of the wrapper: one 2-D array per named slot)
        got = run_set(pair[0], 3, schedule(chunks), 4, feed=lambda call, pos: [blocks[s][pos[s]:pos[s] + n] for s, n in call])
        for s in range(3):
            pair[1].set_emissions(blocks[s])
            res = pair[1].decode_full(None, 1, D.MODE_SINGLE_PASS, T=blocks[s].shape[0])
            rows, bp, _ = pair[1].test_forward(None, [(0, blocks[s].shape[0] - 1, -1)], T=blocks[s].shape[0])
            want = sm.run(bp[1:], rows[0], 4, chunks[s])
            assert got[s]["pieces"] == want["pieces"], s
            assert ([x for p in got[s]["pieces"] for x in p], bits(got[s]["score"]), got[s]["rc"]) == (res[0].tolist(), bits(res[1]), res[2]), s
        pair[0].streams_open(2)
        assert "ld >= P" in refused(lambda: pair[0].streams_push([0, 1], scores=([logs[:4], logs[:3]]), ld=P - 1), D.ERR_ARG)
        pair[0].streams_end()
    finally:
        for f in pair:
            f.close()


@pytest.mark.parametrize("sparse", [False, True])
def test_refused_score_calls_leave_every_slot_as_it_was(sparse):
    sc = Scores("ds_K77_M7_T33", "f32", sparse=sparse)
    try:
        fv, K = sc.pair[0], sc.K
        blocks = [np.ascontiguousarray(np.roll(sc.block, s, axis=0)[:sc.T - s]) for s in range(3)]
        refs = []
        for s in range(3):
            sc.pair[1].set_emissions(blocks[s])
            res = sc.pair[1].decode_full(None, 1, D.MODE_SINGLE_PASS, T=blocks[s].shape[0])
            rows, bp, _ = sc.pair[1].test_forward(None, [(0, blocks[s].shape[0] - 1, -1)], T=blocks[s].shape[0])
            refs.append(((res[0].tolist(), bits(res[1]), res[2]), sm.Stream(bp[1:], rows[0], 4)))
        fv.streams_open(3, 0, 4)
        got = [[], [], []]
        first = (5, 6, 7)                     # the slots stand at different times
        pieces, _ = fv.streams_push([0, 1, 2], scores=[blocks[s][:first[s]] for s in range(3)])
        for s in range(3):
            got[s] += pieces[s].tolist()
            assert pieces[s].tolist() == refs[s][1].push(first[s])
        pend = [fv.streams_pending(s) for s in range(3)]

        def untouched():
            assert [fv.streams_pending(s) for s in range(3)] == pend
            assert [fv.streams_slot_stats(s)["times"] for s in range(3)] == list(first)
            assert [fv.streams_slot_stats(s)["pushes"] for s in range(3)] == [1, 1, 1]

        nxt = [blocks[s][first[s]:first[s] + 9].copy() for s in range(3)]
        for bad in (np.nan, np.inf):
            rows = [b.copy() for b in nxt]
            rows[2][1, 3] = bad               # slot 2's second row: its time 7 + 1
            text = refused(lambda: fv.streams_push([0, 1, 2], scores=rows), D.ERR_ARG)
            assert "slot 2" in text and "(t = 8, state = 3)" in text, text
            untouched()
        rows = [b.copy() for b in nxt]
        rows[1][4, 1] = 0.5                   # a density above 1 under a filter kernel
        assert ("FV_KERNEL_CSR_F64" if sparse else "filter+refine") in refused(lambda: fv.streams_push([0, 1, 2], scores=rows), D.ERR_UNSUPPORTED)
        untouched()
        refused(lambda: fv.streams_push([0, 1], obs=[[0, 0, 0], [0]]), D.ERR_ARG)       # the other kind
        refused(lambda: fv.streams_push([0], scores=((sc.block.ctypes.data, 7, 3, sc.ld), [3])), D.ERR_ARG)
        refused(lambda: fv.streams_push([0], scores=((sc.block.ctypes.data, sc.code, 3, K - 1), [3])), D.ERR_ARG)
        untouched()
        pieces, _ = fv.streams_push([0, 1, 2], scores=nxt)
        for s in range(3):
            got[s] += pieces[s].tolist()
            assert pieces[s].tolist() == refs[s][1].push(9)
        pieces, _ = fv.streams_push([2, 1, 0], scores=[blocks[s][first[s] + 9:] for s in (2, 1, 0)])
        for q, s in enumerate((2, 1, 0)):
            got[s] += pieces[q].tolist()
            assert pieces[q].tolist() == refs[s][1].push(blocks[s].shape[0] - first[s] - 9)
        for s in range(3):
            piece, score, rc = fv.streams_close(s)
            assert (got[s] + piece.tolist(), bits(score), rc) == refs[s][0], s
        fv.streams_end()
    finally:
        sc.close()


@pytest.mark.parametrize("sparse", [False, True])
def test_scores_above_zero_under_the_float64_kernels(sparse):
    ss = SlotScores(Scores("ds_K77_M7_T33", "f64", sparse=sparse, positive=True,
                           kernel=D.KERNEL_CSR_F64 if sparse else D.KERNEL_F64_STREAM))
    try:
        ss.blocks = [np.ascontiguousarray(np.roll(ss.sc.block, s, axis=0)[:ss.sc.T - s]) for s in range(3)]
        check_scores(ss, 4, sparse)
    finally:
        ss.close()


# ---------------------------------------------------------------- 8. refusals

def test_refusals_consume_nothing(ctx):
    fresh = D.FlashViterbi(0)
    try:
        assert fresh.streams_pending(0) == -1
        refused(lambda: fresh.streams_open(2), D.ERR_STATE)                    # no model
        refused(lambda: fresh.streams_stats(), D.ERR_STATE)                    # there never was a set
        refused(lambda: fresh.streams_push([0], obs=[[0]]), D.ERR_STATE)
        refused(lambda: fresh.streams_close(0), D.ERR_STATE)
        refused(lambda: fresh.streams_abort(0), D.ERR_STATE)
        refused(lambda: fresh.streams_end(), D.ERR_STATE)
        refused(lambda: fresh.streams_slot_stats(0), D.ERR_STATE)
    finally:
        fresh.close()
    name = "ds_K77_M7_T33"
    fv, ref_fv = ctx(name)
    A, B, Pi, ob = case(name)
    ex = expect(name, ref_fv)
    before = fv.decode_full(ob, 2, D.MODE_REFERENCE)
    bytes_before = fv.stats()["device_bytes"]
    for bad in ((0, 0, 0), (65, 0, 0), (2, -1, 0), (2, 0, 65), (2, 0, -1)):
        refused(lambda: fv.streams_open(*bad), D.ERR_ARG)
    # a set and the single stream exclude each other
    fv.stream_open()
    assert "stream is already open" in refused(lambda: fv.streams_open(2), D.ERR_STATE)
    fv.stream_abort()
    fv.streams_open(3, 0, 4)
    refused(lambda: fv.streams_open(3, 0, 4), D.ERR_STATE)
    assert "set of streams is already open" in refused(lambda: fv.stream_open(), D.ERR_STATE)
    obs = [ex.seq(s) for s in range(3)]
    models = []
    for s in range(3):
        row, args, _ = slot_tables(name, s)
        models.append(sm.Stream(args, row, 4))
    pieces, _ = fv.streams_push([0, 1, 2], obs=[o[:10] for o in obs])
    got = [p.tolist() for p in pieces]
    assert got == [m.push(10) for m in models]
    pend = [fv.streams_pending(s) for s in range(3)]
    nxt = [o[10:20] for o in obs]

    def untouched():
        assert [fv.streams_pending(s) for s in range(3)] == pend
        assert [(fv.streams_slot_stats(s)["times"], fv.streams_slot_stats(s)["pushes"]) for s in range(3)] == [(10, 1)] * 3

    calls = fv.streams_stats()["calls"]
    refused(lambda: fv.streams_push([], obs=[]), D.ERR_ARG)                                        # nids < 1
    assert "ids[1] = 3" in refused(lambda: fv.streams_push([0, 3], obs=nxt[:2]), D.ERR_ARG)        # outside the set
    refused(lambda: fv.streams_push([0, -1], obs=nxt[:2]), D.ERR_ARG)
    assert "slot 1 is named twice" in refused(lambda: fv.streams_push([1, 0, 1], obs=nxt), D.ERR_ARG)
    assert "slot 2" in refused(lambda: fv.streams_push([0, 2], obs=[nxt[0], nxt[2][:0]]), D.ERR_ARG)   # a length below 1
    bad = nxt[1].copy()
    bad[4] = B.shape[1]
    text = refused(lambda: fv.streams_push([0, 1, 2], obs=[nxt[0], bad, nxt[2]]), D.ERR_ARG)
    assert "slot 1" in text and "time 14" in text, text
    bad[4] = -1
    refused(lambda: fv.streams_push([0, 1, 2], obs=[nxt[0], bad, nxt[2]]), D.ERR_ARG)
    refused(lambda: fv.streams_push([0, 1], scores=[np.zeros((2, A.shape[0]), np.float32)] * 2), D.ERR_ARG)    # the other kind
    # too little room for slot 1, and NULL pointers: through the C interface
    P = lambda a: a.ctypes.data_as(D.ctypes.c_void_p)
    ids = np.array([0, 1], np.int32)
    cat = np.concatenate(nxt[:2]).astype(np.int32)
    offsets = np.array([0, 10, 20], np.int64)
    room = np.array([0, pend[0] + 10, pend[0] + 10 + pend[1] + 9], np.int64)
    path, done = np.empty(int(room[-1]) + 1, np.int32), np.zeros(2, np.int64)
    L, h = fv._L, fv._h
    assert L.fv_streams_push(h, P(ids), 2, P(cat), P(offsets), P(path), P(room), P(done), None) == D.ERR_ARG
    assert "slot 1 needs room" in L.fv_last_error_detail(h).decode()
    room[2] += 1
    for hole in range(6):
        args = [P(ids), 2, P(cat), P(offsets), P(path), P(room), P(done), None]
        args[hole if hole < 1 else hole + 1] = None
        assert L.fv_streams_push(h, *args) == D.ERR_ARG, hole
    assert L.fv_streams_push(h, P(ids), 2, P(cat), P(np.array([1, 10, 20], np.int64)), P(path), P(room), P(done), None) == D.ERR_ARG
    assert L.fv_streams_close(h, 0, None, None, None) == D.ERR_ARG and L.fv_streams_close(h, 3, P(path), D.ctypes.byref(D.ctypes.c_longlong(0)), None) == D.ERR_ARG
    assert L.fv_streams_abort(h, 3) == D.ERR_ARG and L.fv_streams_pending(h, 3) == -1 and L.fv_streams_pending(h, -1) == -1
    refused(lambda: fv.streams_slot_stats(3), D.ERR_ARG)
    untouched()
    assert fv.streams_stats()["calls"] == calls
    # everything else on the context waits for the set to end
    for call in (lambda: fv.decode_full(ob, 1, D.MODE_SINGLE_PASS), lambda: fv.decode_full_batch([ob, ob]),
                 lambda: fv.decode_beam(ob, 1, 8), lambda: fv.decode_beam_batch([ob, ob], 1, 8), lambda: fv.decode_vanilla(ob),
                 lambda: fv.decode_checkpoint(ob), lambda: fv.set_model(A, B, Pi),
                 lambda: fv.set_model_sparse(*D.dense_to_csr(A), B, Pi), lambda: fv.set_option(D.OPT_KERNEL, D.KERNEL_F64_STREAM),
                 lambda: fv.set_emissions(np.zeros((3, A.shape[0]), np.float32)), lambda: fv.clear_emissions(),
                 lambda: fv.set_emission_map(np.zeros(A.shape[0], np.int32), 1), lambda: fv.test_forward(ob, [(0, 5, -1)]),
                 lambda: fv.test_flat_poison(3), lambda: fv.set_partition(0, 2)):
        assert "set of streams is open" in refused(call, D.ERR_STATE)
    refused(lambda: fv.stream_push(ob=ob[:3]), D.ERR_STATE)                    # the single stream's calls find no stream
    untouched()
    # ... and the pushes that follow show that nothing was consumed
    pieces, _ = fv.streams_push([0, 1, 2], obs=[o[10:] for o in obs])
    for s in range(3):
        assert pieces[s].tolist() == models[s].push(len(obs[s]) - 10)
        piece, score, rc = fv.streams_close(s)
        assert (got[s] + pieces[s].tolist() + piece.tolist(), bits(score), rc) == ex.one_shot(s)
    fv.streams_end()
    # after the set the context decodes what it decoded before, in the memory it had before
    after = fv.decode_full(ob, 2, D.MODE_REFERENCE)
    assert (after[0].tolist(), bits(after[1]), after[2]) == (before[0].tolist(), bits(before[1]), before[2])
    assert fv.stats()["device_bytes"] == bytes_before


def test_contexts_that_cannot_hold_a_set():
    A, B, Pi, ob = case("ds_K9_T7")
    part = D.FlashViterbi(0)
    group = D.FlashViterbi([0, 0])
    try:
        for f in (part, group):
            f.set_model(A, B, Pi)
        part.set_partition(0, 2)
        for f in (part, group):
            refused(lambda: f.streams_open(2), D.ERR_UNSUPPORTED)
            assert f.streams_pending(0) == -1
    finally:
        for f in (part, group):
            f.close()


# ---------------------------------------------------------------- 9. growth

def room_model(hint, pushes):
    """make_room's policy on the host: pushes = [(pending before, n, committed by the push)]; returns (capacity, regrows)"""
    cap, off, regrows = max(2, hint), 0, 0
    for live, n, count in pushes:
        need = live + n
        if off + need > cap:
            if cap >= 2 * need:
                off = 0
            else:
                cap, off, regrows = max(2 * cap, 2 * need), 0, regrows + 1
        off += count
    return cap, regrows


@pytest.mark.parametrize("name", ["ties_all_K64_T64", "cfg1_K128_T256"])
def test_arg_rows_grow_per_slot(ctx, name):
    """lag_rows_hint = 2, two slots pushed in different lengths.  ties_all: nothing ever commits, the lag grows to T and both
    slots' rows regrow, each by its own pushes; cfg1: both slots commit and their rows are compacted in between.  (Slots of
    one set share a model, so a slot that never commits and one that does cannot sit in one set.)"""
    fv, ref_fv = ctx(name)
    ex = expect(name, ref_fv)
    lens = [len(ex.seq(s)) for s in range(2)]
    chunks = [even(lens[0], 7), ragged(lens[1], 1)]
    got = run_and_check(fv, ex, chunks, 4, hint=2, tag=name)
    for s in range(2):
        pushes, before = [], 0
        for n, done in zip(chunks[s], got[s]["committed"]):
            start = sum(chunks[s][:len(pushes)])
            pushes.append((start - before, n, done - before))
            before = done
        cap, regrows = room_model(2, pushes)
        st = got[s]["stats"]
        assert (st["arg_rows_capacity"], st["regrows"]) == (cap, regrows), (name, s)
        assert st["regrows"] > 0
        if name.startswith("ties"):
            assert st["commits"] == 0 and st["lag_max"] == lens[s] and st["arg_rows_capacity"] >= lens[s]
        else:
            assert st["commits"] > 0 and st["arg_rows_capacity"] < lens[s]
