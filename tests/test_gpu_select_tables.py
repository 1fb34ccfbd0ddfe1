"""GPU: the top-B selection and the heap layouts of a FLASH-BS lock-step against the oracle's generate_state_heap.

A beam decode reads one path entry of each step's heap, so a select that drops or duplicates a member whose columns
never win, or a replay that leaves a wrong slot order where no tie is met, changes no decoded path.  Here
fv_test_beam_select (include/flashvit_testing.h) makes single select launches — through the launch rule fv_decode_beam
uses — over caller-given score rows of any K (a selection reads no model), and returns every row's cut record, member
list, exact heap layout (heap_build_all) and the select counters.  The reference of a row is H = oracle.state_heap(row, B)
(pinned against a second restatement by tests/test_oracle_heap_probe.py) plus numpy: theta = the B-th largest score,
G = #{> theta}, E = #{== theta}, d = B - G.  All values are compared as uint32 bit patterns:

  d == E                         cut state 0, N = B, members as a set exactly {scores >= theta} = set(H)
  d < E, E - d <= 32             cut state 1 (speculative), N = G + E, members exactly {scores >= theta}; counter 9 +1
  d < E, E - d > 32 or bit 20    cut state 2 (replayed), N = B, members equal H slot for slot; counter 2 +1
  fewer than B real scores       theta = -FLT_MAX, state 0, N = B: every real score + the first d junk states in state order
  layouts                        equal H slot for slot for every row of every case

Rows are built for their case (G, E and the remainder chosen, placed by a seeded permutation) and the case is asserted
from the numpy side.  K and B lie on both sides of every boundary of the code: the register instantiations (4096, 16384,
65536), one round of keys (1024), one wave (64), the list kernels (K > 16384, capacity above 8192 from B = 1025), the
memory-resident form beyond 65536 (131073: three compaction blocks of 64 + 64 + 1 rounds), B == K and the largest
admitted B; 1 / 24 / 25 / 64 rows per launch (more than 24: jobs derived on the device); lock-steps 0, 1, 2; FV_OPT_DEBUG
0 and bits 7, 10, 15, 20, 22; candidate lists of B - 1, B, 2048 / 2049 (four-wave limit), capacity and capacity + 1 entries.
Every call is made twice with identical results; the last test asserts that every FV_TS_* instantiation launched."""
import os
import re

import numpy as np
import pytest

import oracle
from conftest import ROOT
from flash_viterbi_amd import decoder

pytestmark = pytest.mark.gpu

D = decoder
FLT_MAX = np.float32(np.finfo(np.float32).max)
EAGER, MANY, NO_LIST, NO_WAVE, OWN_PRED = 1 << 20, 1 << 22, 1 << 10, 1 << 15, 1 << 7
PREV_MARGIN = 0.3

_reached = {"selects": 0, "tests": set(), "cases": set(), "lists": set()}
_fv = {}


def fv():
    """One context without a model for the whole module."""
    if "h" not in _fv:
        _fv["h"] = decoder.FlashViterbi(0)
    return _fv["h"]


def header_selects():
    text = open(os.path.join(ROOT, "include", "flashvit_testing.h")).read()
    return {int(bit): (name, what) for name, bit, what in
            re.findall(r"#define\s+(FV_TS_\w+)\s+\(1ull << (\d+)\)\s*/\*\s*(.*?)\s*\*/", text)}


# ---------------------------------------------------------------- rows built for their case

def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def b1(x):
    """bit pattern of one float32"""
    return int(np.array([x], dtype=np.float32).view(np.uint32)[0])


def key2f(k):
    """float32 of the select's order-preserving uint32 key"""
    k = np.asarray(k, dtype=np.uint64).astype(np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7fffffff), ~k).astype(np.uint32).view(np.float32)


def f2key(f):
    u = bits(f)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


class Row:
    """A score row with G scores above theta, E equal to it and the rest below (or junk), and its reference heap."""

    def __init__(self, kind, row, B, want):
        self.kind, self.row, self.B = kind, np.ascontiguousarray(row, dtype=np.float32), B
        row = self.row
        self.K = row.size
        self.real = row > -FLT_MAX
        self.nreal = int(self.real.sum())
        self.hval, self.hstate = oracle.state_heap(row, B)
        self.srt = np.sort(row[self.real])[::-1]
        if self.nreal < B:
            self.case, self.d = "junk", B - self.nreal
            self.G, self.E = self.nreal, self.K - self.nreal
            self.theta = -FLT_MAX
        else:
            self.theta = self.srt[B - 1]
            assert b1(self.hval[0]) == b1(self.theta), "the root of the reference heap is the B-th largest score"
            self.G, self.E = int((row > self.theta).sum()), int((row == self.theta).sum())
            self.d = B - self.G
            assert 1 <= self.d <= self.E
            self.case = "exact" if self.d == self.E else "spec" if self.E - self.d <= D.BEAM_EXTRA else "replay"
        assert self.case == want, f"row {kind} K={self.K} B={B}: built for case {want}, is {self.case}"

    def case_under(self, debug):
        return "replay" if self.case == "spec" and (debug & EAGER) else self.case

    def members(self):
        """(states, value bits) of {scores >= theta}, ascending state"""
        idx = np.nonzero(self.row >= self.theta)[0]
        return idx, bits(self.row[idx])

    def cand_list(self, target, cap, rs):
        """(count, values, states) of the list beam_step's epilogue leaves for a bound at the target-th largest real score:
        every real score >= that bound, shuffled; min(count, cap) entries are given.  A target below B stands for a bound
        that came out above the cut: the G scores above theta (B - 1 of them where the scores are distinct)."""
        if self.nreal == 0 or target <= 0:
            return 0, np.zeros(0, np.float32), np.zeros(0, np.int32)
        if target < self.B:
            idx = np.nonzero(self.real & (self.row > self.theta))[0]
        else:
            idx = np.nonzero(self.real & (self.row >= self.srt[min(target, self.nreal) - 1]))[0]
        idx = idx[rs.permutation(idx.size)]
        C = int(idx.size)
        idx = idx[:cap]
        return C, self.row[idx], idx.astype(np.int32)


def place(rs, K, B, above, theta, E, below, spread=True):
    """above + E copies of theta + below, placed by a seeded permutation; spread: one duplicate of theta inside the
    initial build (states < B) and one among the last states, so that the duplicates span every compaction block."""
    vals = np.concatenate([np.asarray(above, np.float32), np.full(E, theta, np.float32), np.asarray(below, np.float32)])
    assert vals.size == K
    row = vals[rs.permutation(K)]
    if spread and E >= 2 and K > B:
        dup = np.nonzero(row == np.float32(theta))[0]
        for src, dst in ((dup[0], int(rs.randint(0, B))), (dup[-1], K - 1 - int(rs.randint(0, min(64, K - B))))):
            if row[dst] != np.float32(theta):
                row[src], row[dst] = row[dst], row[src]
                dup = np.nonzero(row == np.float32(theta))[0]
    return row


def junk(rs, n):
    return np.where(rs.randint(0, 2, n) == 0, -FLT_MAX, np.float32(-np.inf)).astype(np.float32)


def wide_keys(rs, K, B, nbits, G, E):
    """Rows whose rebased keys use nbits bits, both ends of the key range present: a run of keys upwards from -11700, or
    (32 bits) mixed-sign scores between -3e4 and 3e4 with the cut at 0.5."""
    if nbits == 32:
        lo, hi, tk = int(f2key(np.float32(-3e4))[0]), int(f2key(np.float32(3e4))[0]), int(f2key(np.float32(0.5))[0])
        span = hi - lo + 1
    else:
        span = int(rs.randint(1 << (nbits - 1), 1 << nbits))
        lo = int(f2key(np.float32(-11700.0))[0])
        hi, tk = lo + span - 1, lo + span // 2
    nb = K - G - E
    tk = hi if G == 0 else lo if nb == 0 else tk
    assert (G == 0 or tk < hi) and (nb == 0 or tk > lo)
    ab = rs.randint(tk + 1, hi + 1, G, dtype=np.int64) if G else np.zeros(0, np.int64)
    be = rs.randint(lo, tk, nb, dtype=np.int64) if nb else np.zeros(0, np.int64)
    # (no zeros or denormals: -0.0 compares equal to +0.0 while its key does not)
    ab[np.abs(ab - 0x80000000) <= 0x00800000] = int(f2key(np.float32(1.0))[0])
    be[np.abs(be - 0x80000000) <= 0x00800000] = int(f2key(np.float32(-1.0))[0])
    if G:
        ab[0] = hi
    if nb:
        be[0] = lo
    row = place(rs, K, B, key2f(ab), key2f([tk])[0], E, key2f(be))
    keys = f2key(row).astype(np.int64)
    assert int(keys.max() - keys.min() + 1).bit_length() == nbits, f"wide row: {nbits} key bits intended"
    assert np.isfinite(row).all() and (nbits < 32 or ((row < 0).any() and (row > 0).any()))
    return row


def history_row(rs, K, B, d, E):
    """The case no simple rule gets right: some duplicates of theta inside the initial build and some after
    it, and larger scores arriving after the B-th score >= theta."""
    G, x = B - d, E - d
    theta = np.float32(-52.0)
    tail_above = min(G, x)
    assert G >= 1 and x >= 1 and tail_above >= 1 and K - B >= x
    e_in = min(max(1, E // 2), B - 1, E - 1)
    if K - G - E < B - e_in - min(G - tail_above, B - e_in):
        return None
    above = theta + 0.25 * (1 + rs.permutation(G)).astype(np.float32)
    below = theta - 0.25 * (1 + rs.permutation(K - G - E)).astype(np.float32)
    a_head = min(G - tail_above, B - e_in)
    head = np.concatenate([np.full(e_in, theta, np.float32), above[:a_head], below[:B - e_in - a_head]])
    used_b = B - e_in - a_head
    tail = np.concatenate([above[G - tail_above:], below[used_b:used_b + min(3, below.size - used_b)]])
    used_b2 = used_b + tail.size - tail_above
    mid = np.concatenate([np.full(E - e_in, theta, np.float32), above[a_head:G - tail_above], below[used_b2:]])
    row = np.concatenate([head[rs.permutation(head.size)], mid[rs.permutation(mid.size)], tail[rs.permutation(tail.size)]])
    assert row.size == K
    dup, ge = np.nonzero(row == theta)[0], np.nonzero(row >= theta)[0]
    assert dup[0] < B <= dup[-1], "duplicates on both sides of the initial build"
    assert (np.nonzero(row > theta)[0] > ge[B - 1]).any(), "a larger score arrives after the B-th score >= theta"
    return row


KINDS = ["distinct", "equal", "levels", "bunched", "wide8", "wide9", "wide16", "wide17", "wide24", "wide25", "wide32",
         "junkB", "junkB-1", "junk0", "junkhalf", "history", "history-replay", "ed1", "ed31", "ed32", "ed33"]


def build_row(kind, K, B, rs):
    """None where (K, B) has no such row."""
    free = K - B
    if kind == "distinct":
        return Row(kind, place(rs, K, B, -40.0 + 0.25 * np.arange(1, B), -40.0, 1, -40.0 - 0.25 * np.arange(1, free + 1)), B, "exact")
    if kind == "equal":                                # one key bit
        return Row(kind, np.full(K, -7.5, np.float32), B, "exact" if free == 0 else "spec" if free <= 32 else "replay")
    if kind == "levels":
        d = max(1, B // 3)
        x = min(free, 40)
        above = rs.choice(np.array([-3.0, -3.5, -4.0], np.float32), B - d)
        below = rs.choice(np.array([-6.0, -7.25, -9.0], np.float32), free - x)
        return Row(kind, place(rs, K, B, above, -5.0, d + x, below), B, "exact" if x == 0 else "replay" if x > 32 else "spec")
    if kind == "bunched":                              # a real step: around -11700, one float spacing (2^-10) apart
        d = min(B, 2)
        x = min(free, 5)
        theta = np.float32(-11700.0)
        above = theta + rs.randint(1, 64, B - d).astype(np.float32) / 1024
        below = theta - rs.randint(1, 64, free - x).astype(np.float32) / 1024
        return Row(kind, place(rs, K, B, above, theta, d + x, below), B, "exact" if x == 0 else "spec")
    if kind.startswith("wide"):
        nbits = int(kind[4:])
        if K < 3:
            return None
        d = 1 if nbits % 2 == 0 else min(B, 2)
        x = 0 if nbits % 2 == 0 else min(free, 3)
        if B - d == 0 and free - x == 0:
            return None
        return Row(kind, wide_keys(rs, K, B, nbits, B - d, d + x), B, "exact" if x == 0 else "spec")
    if kind.startswith("junk"):
        nreal = {"junkB": B, "junkB-1": B - 1, "junk0": 0, "junkhalf": B // 2}[kind]
        if K - nreal == 0 or (kind == "junkhalf" and nreal < 2):
            return None
        if kind == "junkhalf":                         # real scores with duplicates
            reals = rs.choice(np.array([-3.0, -4.5, -6.0], np.float32), nreal)
        else:
            reals = -40.0 - 0.25 * np.arange(nreal)
        row = np.concatenate([reals.astype(np.float32), junk(rs, K - nreal)])[rs.permutation(K)]
        return Row(kind, row, B, "exact" if kind == "junkB" else "junk")
    if kind.startswith("history"):
        x = 5 if kind == "history" else 40
        d = max(1, B // 2)
        if free < x or B - d < 1:
            return None
        row = history_row(rs, K, B, d, d + x)
        return None if row is None else Row(kind, row, B, "spec" if x <= 32 else "replay")
    x = int(kind[2:])                                  # ed<x>: E - d = x
    if free < x:
        return None
    d = 1 + (B - 1) // 2
    theta = np.float32(-52.0)
    above = theta + 0.25 * np.arange(1, B - d + 1)
    below = theta - 0.25 * np.arange(1, free - x + 1)
    return Row(kind, place(rs, K, B, above, theta, d + x, below), B, "spec" if x <= 32 else "replay")


def pool_for(K, B, seed):
    rs = np.random.RandomState(seed)
    pool = [r for r in (build_row(kind, K, B, rs) for kind in KINDS) if r is not None]
    assert pool
    return pool


# ---------------------------------------------------------------- one launch, twice, against the reference

LIST_TARGETS = ["fit", None, "B-1", "2048", "B", "2049", "cap", "cap+1"]


def list_for(r, what, cap, rs):
    """None (no list given: the select sees an empty one), or the row's list for a named length."""
    if what is None:
        return None
    B = r.B
    target = {"fit": min(cap, 2 * B), "B-1": B - 1, "B": B, "2048": 2048, "2049": 2049, "cap": cap, "cap+1": cap + 1}[what]
    return r.cand_list(target, cap, rs)


def check_launch(rows, s, debug, lists=None, seed=None, where=""):
    h = fv()
    h.set_option(D.OPT_DEBUG, debug)
    B, K, n = rows[0].B, rows[0].K, len(rows)
    where = f"select K={K} B={B} s={s} rows={n} debug={debug:#x} {where}"
    mat = np.stack([r.row for r in rows])
    theta_prev = float(np.float32(-11690.0))
    args = dict(s=s, lists=lists, prev_theta=theta_prev, prev_margin=PREV_MARGIN, seed=seed)
    got = h.test_beam_select(B, mat, **args)
    again = h.test_beam_select(B, mat, **args)
    cap = got["cand_cap"]
    _reached["selects"] |= got["selects"]
    assert got["selects"] == again["selects"] and got["counters"] == again["counters"], where
    assert np.array_equal(bits(got["cut"]), bits(again["cut"])), f"{where}: cut records differ between two calls"
    assert np.array_equal(bits(got["slot_val"]), bits(again["slot_val"])) and np.array_equal(got["slot_state"], again["slot_state"]), where
    want = {c: 0 for c in D.SELECT_COUNTERS}
    for q, r in enumerate(rows):
        at = f"{where} row {q} ({r.kind}: G={r.G} E={r.E} d={r.d})"
        cut = got["cut"][q]
        case = r.case_under(debug)
        _reached["cases"].add(case)
        C = 0
        if lists is not None and lists[q] is not None:
            C = lists[q][0]
        used = C >= B and C <= cap and s >= 1 and cap > 0
        if used:
            want[7] += 1
            want[13] += C
            _reached["lists"].add("quad" if C <= 2048 and not (debug & NO_WAVE) else "block")
        elif s >= 2 and cap > 0:
            want[11 if C < B else 12] += 1
        assert cut[D.CUT_LIST] == C, f"{at}: CUT_LIST {cut[D.CUT_LIST]}, list of {C}"
        assert b1(cut[D.CUT_THETA]) == b1(r.theta), f"{at}: theta {cut[D.CUT_THETA]!r}, want {r.theta!r}"
        assert not np.isnan(cut[D.CUT_NEXT]), f"{at}: CUT_NEXT is NaN"
        if s == 0 and seed is None:
            assert cut[D.CUT_NEXT] == np.inf, f"{at}: CUT_NEXT {cut[D.CUT_NEXT]} without a previous cut or a seed"
        state, N = {"exact": (0, B), "junk": (0, B), "spec": (1, r.G + r.E), "replay": (2, B)}[case]
        assert cut[D.CUT_STATE] == state and cut[D.CUT_N] == N, f"{at}: case {case}: state {cut[D.CUT_STATE]} N {cut[D.CUT_N]}, want {state} / {N}"
        want[9] += case == "spec"
        want[2] += case == "replay"
        mv, ms = got["members"][q]
        av, as_ = again["members"][q]
        assert (got["raw_state"][q, N:] == -1).all() and np.isnan(got["raw_val"][q, N:]).all(), f"{at}: entries written beyond the {N} members"
        assert ((ms >= 0) & (ms < K)).all(), f"{at}: member states outside [0, K)"
        assert np.array_equal(bits(mv), bits(r.row[ms])), f"{at}: a member's value is not its state's score"
        if case == "replay":
            assert np.array_equal(ms, r.hstate) and np.array_equal(bits(mv), bits(r.hval)), f"{at}: replayed members differ from the reference heap"
            assert np.array_equal(ms, as_) and np.array_equal(bits(mv), bits(av)), f"{at}: two calls differ"
        else:
            order = np.sort(ms)
            assert np.array_equal(order, np.sort(as_)), f"{at}: two calls differ"
            assert (np.diff(order) > 0).all(), f"{at}: a state is listed twice"
            if case == "junk":
                real = r.real[ms]
                assert np.array_equal(np.sort(ms[real]), np.nonzero(r.real)[0]), f"{at}: real members"
                assert np.array_equal(np.sort(ms[real]), np.sort(r.hstate[r.hval > -FLT_MAX])), f"{at}: real members differ from the heap's"
                assert np.array_equal(np.sort(ms[~real]), np.nonzero(~r.real)[0][:r.d]), f"{at}: junk members are not the first {r.d} junk states"
            else:
                idx, vb = r.members()
                assert np.array_equal(order, idx), f"{at}: members differ from {{scores >= theta}}"
                if case == "exact":
                    assert np.array_equal(order, np.sort(r.hstate)), f"{at}: members differ from the reference heap's"
        assert np.array_equal(got["slot_state"][q], r.hstate) and np.array_equal(bits(got["slot_val"][q]), bits(r.hval)), \
            f"{at}: heap_build_all layout differs from the reference heap"
    assert got["counters"] == want, f"{where}: counters {got['counters']}, want {want}"
    assert got["counters"][10] == 0 and got["counters"][5] == 0
    return got


# (s, FV_OPT_DEBUG, rows per launch, lists?): every debug form with every lock-step it changes, both job forms
CONFIGS = [(0, 0, 1, False), (1, 0, 24, False), (2, 0, 25, True), (2, 0, 24, True), (1, 0, 3, True), (2, OWN_PRED, 3, True),
           (2, NO_LIST, 24, False), (0, NO_LIST, 25, False), (1, NO_WAVE, 64, True), (2, NO_WAVE, 5, True), (2, EAGER, 3, True),
           (0, EAGER, 25, False), (0, MANY, 25, False), (1, MANY, 1, True), (2, MANY, 24, True), (2, EAGER | MANY, 24, True),
           (0, EAGER | MANY, 64, False), (2, NO_WAVE | EAGER, 64, True)]

SHAPES = [(2, 2), (63, 2), (63, 63), (64, 3), (64, 64), (65, 63), (65, 64), (65, 65), (1023, 64), (1023, 1023),
          (1024, 65), (1024, 256), (1024, 1024), (1025, 3), (1025, 1024), (1025, 1025), (4096, 2), (4096, 256),
          (4096, 1025), (4096, 4096), (4097, 63), (4097, 1024), (4097, 4097), (16384, 64), (16384, 256), (16384, 1025),
          (16385, 65), (16385, 1024), (16385, 1025), (65536, 256), (65536, 1025), (65537, 3), (65537, 1024),
          (65537, 1025), (131073, 2), (131073, 256), (131073, 1025)]


def run_shape(K, B, configs):
    pool = pool_for(K, B, 31 * K + B)
    rs = np.random.RandomState(K + 7 * B)
    for ci, (s, debug, n, with_lists) in enumerate(configs):
        if K * n > (1 << 21):                           # big rows: few per launch, both job forms kept
            n = 25 if n > 24 else min(n, 2)
        fv().set_option(D.OPT_DEBUG, debug)
        cap = fv().select_cand_cap(K, B)
        assert cap == (0 if debug & NO_LIST else cap) and (cap == 0 or 3 * cap <= 2 * K)
        rows = [pool[(ci * 5 + q) % len(pool)] for q in range(n)]
        lists = None
        if with_lists and cap > 0 and s >= 1:
            lists = [list_for(r, LIST_TARGETS[(ci + q) % len(LIST_TARGETS)], cap, rs) for q, r in enumerate(rows)]
        check_launch(rows, s, debug, lists, where=f"config {ci}")


@pytest.mark.parametrize("K,B", SHAPES, ids=[f"K{k}-B{b}" for k, b in SHAPES])
def test_select_matrix(K, B):
    _reached["tests"].add(f"matrix-{K}-{B}")
    run_shape(K, B, CONFIGS)


def largest_admitted(K):
    lo, hi = 2, K
    while lo < hi:                                      # (nsets = 0: admission only, no device work)
        mid = (lo + hi + 1) // 2
        try:
            fv().select_cand_cap(K, mid)
            lo = mid
        except decoder.FlashVitError as e:
            assert e.rc == D.ERR_UNSUPPORTED
            hi = mid - 1
    return lo


@pytest.mark.parametrize("K", [16384, 65537])
def test_select_largest_admitted_beam(K):
    """The largest B the beam path admits (heap_lds(B) <= 150 KiB: 9085), on the register and the memory-resident form."""
    _reached["tests"].add(f"largest-{K}")
    fv().set_option(D.OPT_DEBUG, 0)
    B = largest_admitted(K)
    assert B == 9085
    run_shape(K, B, [(0, 0, 2, False), (2, 0, 3, False), (2, EAGER, 25, False), (1, MANY, 2, False)])


@pytest.mark.parametrize("K,B", [(16384, 1024), (16385, 1025), (65537, 1024), (4608, 257)])
def test_select_list_lengths(K, B):
    """Every named list length on rows where it is exact (distinct scores below the cut): B - 1 and capacity + 1 are not
    used, B .. capacity are; 2048 entries take the four-wave form, 2049 the whole workgroup."""
    _reached["tests"].add(f"lists-{K}-{B}")
    rs = np.random.RandomState(K + B)
    pool = {r.kind: r for r in pool_for(K, B, 77 * K + B)}
    for s, debug in ((2, 0), (1, 0), (2, NO_WAVE), (2, EAGER), (2, MANY)):
        fv().set_option(D.OPT_DEBUG, debug)
        cap = fv().select_cand_cap(K, B)
        assert cap == min(16384, -(-8 * B // 1024) * 1024)
        for kind in ("distinct", "ed1", "ed32", "ed33", "history"):
            r = pool[kind]
            names = ["B-1", "B", "2048", "2049", "cap", "cap+1"]
            lists = [list_for(r, w, cap, rs) for w in names]
            for w, (C, _, _) in zip(names, lists):
                want = {"B-1": r.G, "B": max(B, r.G + r.E), "2048": max(2048, r.G + r.E), "2049": max(2049, r.G + r.E),
                        "cap": cap, "cap+1": cap + 1}[w]
                assert C == want, f"list {w} of row {kind}: {C} entries"
            got = check_launch([r] * len(names), s, debug, lists, where=f"lists of {kind}")
            assert got["counters"][7] == 4 and got["counters"][11] == (s >= 2) and got["counters"][12] == (s >= 2)


def test_select_seeded_predictor():
    """A pass of a later generation: the slot holds the cut an earlier pass left, and so does the next one."""
    _reached["tests"].add("seeded")
    K, B = 4097, 64
    pool = pool_for(K, B, 5)
    for s in (0, 1, 2):
        for debug in (0, OWN_PRED):
            got = check_launch(pool[:8], s, debug, seed=(-50.0, -53.5), where="seeded")
            if s == 0 and not debug:
                for q, r in enumerate(pool[:8]):
                    if r.case != "junk":
                        assert got["cut"][q, D.CUT_NEXT] < r.theta - 3.0


def test_select_refusals():
    """Host-side: every refusal comes before any device work."""
    _reached["tests"].add("refusals")
    h = fv()
    h.set_option(D.OPT_DEBUG, 0)
    rows = np.zeros((1, 4096), np.float32)

    def refused(rc, beam, mat, **kw):
        with pytest.raises(decoder.FlashVitError) as e:
            h.test_beam_select(beam, mat, **kw)
        assert e.value.rc == rc

    refused(D.ERR_ARG, 1, rows)
    refused(D.ERR_ARG, 4097, rows)
    refused(D.ERR_ARG, 3, np.zeros((1, 2), np.float32))
    refused(D.ERR_UNSUPPORTED, 9086, np.zeros((1, 16384), np.float32))
    refused(D.ERR_ARG, 64, rows, s=3)
    refused(D.ERR_ARG, 64, rows, s=-1)
    refused(D.ERR_ARG, 64, np.zeros((65, 4096), np.float32))
    ok = (3, np.zeros(3, np.float32), np.array([0, 5, 4095], np.int32))
    assert h.select_cand_cap(4096, 64) == 1024
    refused(D.ERR_ARG, 64, rows, s=2, lists=[(3, ok[1], np.array([0, 5, 4096], np.int32))])
    refused(D.ERR_ARG, 64, rows, s=2, lists=[(3, ok[1], np.array([0, -1, 7], np.int32))])
    refused(D.ERR_ARG, 64, rows, s=2, lists=[(-1, ok[1], ok[2])])
    refused(D.ERR_ARG, 64, rows, s=0, lists=[ok])                               # no list at the first step
    assert h.select_cand_cap(4096, 1024) == 0
    refused(D.ERR_ARG, 1024, rows, s=2, lists=[ok])                             # no list at this (K, B)
    h.set_option(D.OPT_DEBUG, NO_LIST)
    assert h.select_cand_cap(4096, 64) == 0
    refused(D.ERR_ARG, 64, rows, s=2, lists=[ok])                               # bit 10: no lists
    h.set_option(D.OPT_DEBUG, 0)
    multi = decoder.FlashViterbi([0, 0])
    try:
        with pytest.raises(decoder.FlashVitError) as e:
            multi.test_beam_select(64, rows)
        assert e.value.rc == D.ERR_ARG
    finally:
        multi.close()
    # and the hook still works after them
    check_launch(pool_for(4096, 64, 1)[:2], 2, 0, [ok, None], where="after refusals")


# ---------------------------------------------------------------- coverage

def test_zz_every_select_instantiation_ran():
    """Runs last: the union of selects_out over the module is every FV_TS_* bit of include/flashvit_testing.h, every case
    of the table was met and lists were selected by four waves and by the whole workgroup."""
    expected = {f"matrix-{k}-{b}" for k, b in SHAPES} | {"largest-16384", "largest-65537", "seeded", "refusals"} | \
               {f"lists-{k}-{b}" for k, b in [(16384, 1024), (16385, 1025), (65537, 1024), (4608, 257)]}
    if not expected <= _reached["tests"]:
        pytest.skip("needs the whole module")
    names = header_selects()
    assert sorted(names) == list(range(11)) and D.TS_ALL == (1 << 11) - 1
    assert {names[b][0] for b in names} == {"FV_TS_" + n for n in (
        "SEL4_LISTED", "SEL4_DERIVED", "SEL16_LISTED", "SEL16_DERIVED", "SEL64_LISTED", "SEL64_DERIVED", "CAND8_LISTED",
        "CAND8_DERIVED", "CAND16_LISTED", "CAND16_DERIVED", "HEAP_BUILD_ALL")}
    missing = [f"{names[b][0]} = {names[b][1]}" for b in sorted(names) if not (_reached["selects"] >> b) & 1]
    assert not missing, "select-kernel instantiations no test launched: " + "; ".join(missing)
    assert _reached["selects"] >> 11 == 0
    assert _reached["cases"] == {"exact", "spec", "replay", "junk"} and _reached["lists"] == {"quad", "block"}
    if "h" in _fv:
        _fv.pop("h").close()
