"""GPU: whole FLASH-BS passes against the oracle, cell by cell.

fv_test_beam_forward (include/flashvit_testing.h) runs caller-chosen passes as one generation of the decode's own beam
driver and copies out what the context then holds for every time of every pass: the K scores, the K back-pointers, the cut
record, the member list, the doubtful-column list and the heap layout.  The oracle side is fvo_beam_forward per pass —
score rows S*, winning states arg* and heaps H* in slot order — pinned to the reference by
tests/test_oracle_beam_forward.py.  Every comparison is an equality, or '>=' where the device holds an upper bound.

What must hold per pass [L, R] and time t (the lazy-replay contract of DESIGN.md 5.4a):
  * cut[t].theta == min(H*[t]): the cut is exact even where scores are not (what doubtful_reach is there to keep);
  * a step t is DIRTY when cut[t-1] is speculative and doubt_count[t] > 0; its listed columns hold upper bounds
    (>= S*, and below theta: a listed column inside the beam would have been a reach event), every other column is exact;
  * an exact column has score == S*, and back-pointer == arg* unless the cell is tagged; a tagged cell's provisional
    state is a member of H*[t-1] whose cell value (the reference expression, restated here) attains the maximum;
  * member lists: CUT_STATE 0 — H*[t] as a multiset; 2 — H*[t] in slot order; 1 — the entries above theta are H*[t]'s,
    the theta-valued entries are ALL states with S*[t] == theta, at most 32 more than the beam;
  * the pass end: whole-sequence pass — end pick and score of the last heap's layout, path = back-track over arg*; any
    other pass — the back-track from its end state if that is a member of H*[R], else -1 everywhere;
  * gate up or FV_OPT_DEBUG bit 19: no dirty step, no tag, scores == S*, back-pointers == arg*, layouts == H* in slot
    order at every time.  A CUT_STATE of 1 may remain where it is unobservable (no theta-valued entry won a column of the
    next step, or the step is the last): the resolve code decides SCORES, and replays a step only for a dirty successor.
Every case asserts the counters that prove its regime ran."""
import math

import numpy as np
import pytest

import modelgen
import oracle
from flash_viterbi_amd import decoder

pytestmark = pytest.mark.gpu

D = decoder
TAG = D.TIE_TAG
EAGER, ALL, NOCUT, MANY, NOLISTS, NOWAVE, QUAD = 1 << 20, 1 << 19, 1 << 23, 1 << 22, 1 << 10, 1 << 15, 1 << 24
ONE_STREAM, GROUPS = 1 << 16, 1 << 17
F64, Q16, Q16_W8 = 256, 512, 512 | (1 << 26)
DEBUGS = (0, EAGER, ALL, ALL | EAGER, ALL | NOCUT, NOCUT, Q16, F64, Q16_W8, MANY, MANY | NOLISTS, NOWAVE)
TV_BEAM_Q16 = (1 << 48) | (1 << 49)      # FV_TV_BEAM_Q16_W8 | FV_TV_BEAM_Q16_W16
FLT_MAX = np.finfo(np.float32).max
# what every case prints (pytest -s) and DESIGN.md 2d tabulates
COUNTERS = ("beam_spec_steps", "beam_reach_events", "beam_exact_sets", "beam_ties", "beam_cand_selects", "beam_list_short",
            "beam_chain_cuts", "step_launches", "task_steps")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def libm_log(x):
    """float64 log of every float32 entry of x through math.log (the libm the library and the oracle call); log 0 = -inf"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    vals, inv = np.unique(x.reshape(-1), return_inverse=True)
    table = np.array([math.log(float(v)) if v > 0 else -math.inf for v in vals], dtype=np.float64)
    return table[inv.reshape(-1)].reshape(x.shape)


class Model:
    """One model: its float32 tables, the oracle, the dense-set context and the oracle's tables per pass (computed once)."""

    def __init__(self, spec, beam):
        self.spec, self.beam = spec, beam
        self.A, self.B, self.Pi, self.ob = modelgen.model32(spec)
        self.K, self.T = spec["K"], spec["T"]
        self.om = oracle.OracleModel(self.A, self.B, self.Pi)
        self.fv = D.FlashViterbi(0)
        self.fv.set_model(self.A, self.B, self.Pi)
        self.tmp = libm_log(self.B).astype(np.float32)          # [K][M]: (float)log B[i][o]
        self._tables, self._sparse, self._emis = {}, None, False

    def tables(self, L, R, init):
        key = (L, R, init)
        if key not in self._tables:
            self._tables[key] = self.om.beam_forward(self.ob, L, R, init, self.beam)
        return self._tables[key]

    def sparse(self):
        if self._sparse is None:
            self._sparse = D.FlashViterbi(0)
            self._sparse.set_model_sparse(*D.dense_to_csr(self.A), self.B, self.Pi)
            self._sparse.set_option(D.OPT_SPARSE_BEAM, 1)
        return self._sparse

    def stage_emissions(self):
        """the M = T restatement: logE[t][i] = log B[i][ob[t]]"""
        if not self._emis:
            self.fv.set_emissions(np.ascontiguousarray(libm_log(self.B)[:, self.ob].T))
            self._emis = True

    def close(self):
        self.fv.close()
        self.om.close()
        if self._sparse is not None:
            self._sparse.close()


SPECS = {
    "semi100": (dict(kind="ties_semi", K=100, M=4, T=300, seed=431, prob=0.5), 30),
    "all96": (dict(kind="ties_all", K=96, M=4, T=200, seed=432, prob=0.5), 17),
    "ds300": (dict(kind="data_script", K=300, M=20, T=400, seed=433, prob=0.2), 50),
    "semi1200": (dict(kind="ties_semi", K=1200, M=4, T=60, seed=221, prob=0.5), 50),
    "fast7000": (dict(kind="sparse_fast", K=7000, M=8, T=300, seed=77, prob=0.05), 100),
    "semi7000": (dict(kind="ties_semi", K=7000, M=4, T=48, seed=242, prob=0.5), 64),
    "ds16500": (dict(kind="data_script", K=16500, M=10, T=24, seed=208, prob=0.02), 300),
    "chain": (dict(kind="ties_semi", K=100, M=4, T=2500, seed=431, prob=0.5), 30),
}


@pytest.fixture(scope="module")
def models():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Model(*SPECS[name])
        return cache[name]
    yield get
    for m in cache.values():
        m.close()


def run(m, passes, dbg, fv=None, emissions=False):
    fv = fv or m.fv
    fv.set_option(D.OPT_DEBUG, dbg)
    try:
        out = fv.test_beam_forward(None if emissions else m.ob, m.beam, passes, T=m.T if emissions else None)
        out["stats"] = fv.stats()
    finally:
        fv.set_option(D.OPT_DEBUG, 0)
    return out


def backtrack(arg, L, R, end):
    """states at L .. R-1 of the walk from `end` at R over arg* (row t - L - 1 is step t); -1 once a cell has no predecessor"""
    path = np.full(R - L, -1, np.int32)
    st = end
    for t in range(R, L, -1):
        st = int(arg[t - L - 1][st]) if st >= 0 else -1
        path[t - 1 - L] = st
    return path


def check_pass(m, out, p, dbg, whole):
    """every invariant of the module docstring for one pass of one hook call; returns the number of dirty steps"""
    L, R, init, end = p
    K, B = m.K, m.beam
    S, arg, Hv, Hs, fstate, fscore = m.tables(L, R, init)
    cut, dcount = out["cut"], out["doubt_count"]
    decided = bool(dbg & ALL) or out["gate"] != 0
    where = f"{m.spec['kind']} K={K} pass={p} debug={dbg:#x}"
    ndirty = 0
    for t in range(L, R + 1):
        r = t - L
        at = f"{where} t={t}"
        real = S[r] > -FLT_MAX
        few = int(real.sum()) < B
        # fewer than B real scores: the cut is the select's "no real score" value and the list is filled up with junk states
        theta = np.float32(-FLT_MAX) if few else Hv[r].min()
        assert bits(cut[t, D.CUT_THETA]) == bits(theta), at
        state, n = int(cut[t, D.CUT_STATE]), int(cut[t, D.CUT_N])
        dirty = t > L and cut[t - 1, D.CUT_STATE] == 1 and dcount[t] > 0
        ndirty += bool(dirty)
        assert not (dirty and (decided or dbg & EAGER)), at
        exact = np.ones(K, bool)
        if dirty:
            assert dcount[t] <= D.DOUBT_CAP, at              # (more: treated as reaching the beam, resolved at once)
            cols = out["doubt"][t, :dcount[t]]
            assert cols.min() >= 0 and cols.max() < K, at
            exact[cols] = False
            assert np.all(out["scores"][t, cols] >= S[r, cols]), at
            assert np.all(out["scores"][t, cols] < theta), at
        assert np.array_equal(bits(out["scores"][t])[exact], bits(S[r])[exact]), at
        if t > L:
            bp = out["bp"][t]
            tagged = (bp >= 0) & ((bp & TAG) != 0)
            assert not (decided and tagged.any()), at
            plain = exact & ~tagged
            assert np.array_equal(bp[plain], arg[r - 1][plain]), at
            c = np.nonzero(tagged & exact)[0]
            if c.size:
                prov = bp[c] & ~TAG
                slot = np.full(K, -1, np.int64)
                slot[Hs[r - 1]] = np.arange(B)
                assert np.all(slot[prov] >= 0), at
                tmp = m.tmp[c, m.ob[t]]
                s = (tmp + Hv[r - 1][slot[prov]]).astype(np.float32)                       # float add
                cell = (s.astype(np.float64) + libm_log(m.A[prov, c])).astype(np.float32)  # double add, one rounding
                assert np.array_equal(bits(cell), bits(S[r, c])), at
        mv, ms = out["member_val"][t, :max(n, 0)], out["member_state"][t, :max(n, 0)]
        if few and state == 0:
            # (the select's contract, tests/test_gpu_select_tables.py: every real score, then the first junk states in state
            # order; -FLT_MAX and -inf can never win a cell, so which junk states the reference's heap holds is unobservable)
            want = np.concatenate([np.nonzero(real)[0], np.nonzero(~real)[0][:B - int(real.sum())]])
            o = np.argsort(ms, kind="stable")
            assert n == B and np.array_equal(ms[o], np.sort(want)) and np.array_equal(bits(mv[o]), bits(S[r][np.sort(want)])), at
        elif state == 2:
            assert n == B and np.array_equal(bits(mv), bits(Hv[r])) and np.array_equal(ms, Hs[r]), at
        elif state == 0:
            o, w = np.argsort(ms, kind="stable"), np.argsort(Hs[r], kind="stable")
            assert n == B and np.array_equal(ms[o], Hs[r][w]) and np.array_equal(bits(mv[o]), bits(Hv[r][w])), at
        else:
            assert state == 1 and B < n <= B + D.BEAM_EXTRA and not dbg & EAGER, at
            assert decided <= (t == R or dcount[t + 1] == 0), at
            above, wabove = mv > theta, Hv[r] > theta
            o, w = np.argsort(ms[above], kind="stable"), np.argsort(Hs[r][wabove], kind="stable")
            assert np.array_equal(ms[above][o], Hs[r][wabove][w]), at
            assert np.array_equal(bits(mv[above][o]), bits(Hv[r][wabove][w])), at
            assert np.all(mv[~above] == theta), at
            assert sorted(ms[~above].tolist()) == np.nonzero(S[r] == theta)[0].tolist(), at
        if decided or (whole and t == R):
            assert np.array_equal(bits(out["slot_val"][t]), bits(Hv[r])) and np.array_equal(out["slot_state"][t], Hs[r]), at
    path = out["path"]
    if whole:
        assert path[R] == fstate and bits(out["score"]) == bits(fscore), where
        assert np.array_equal(path[L:R], backtrack(arg, L, R, fstate)), where
    else:
        assert path[R] == end, where
        member = end >= 0 and end in Hs[R - L].tolist()
        want = backtrack(arg, L, R, end) if member else np.full(R - L, -1, np.int32)
        assert np.array_equal(path[L:R], want), where
    return ndirty


def check(m, out, passes, dbg):
    whole = len(passes) == 1 and passes[0] == (0, m.T - 1, -1, -1)
    st = out["stats"]
    if dbg & EAGER:
        assert st["beam_spec_steps"] == 0
    return sum(check_pass(m, out, p, dbg, whole) for p in passes)


def whole_pass(m):
    return [(0, m.T - 1, -1, -1)]


def straddle(S, Hv, extra_max=None):
    """does the cut of this row fall on a duplicated value (more scores equal to it than the heap keeps)?"""
    theta = Hv.min()
    E, kept = int(np.count_nonzero(S == theta)), int(np.count_nonzero(Hv == theta))
    return theta > -FLT_MAX and E > kept and (extra_max is None or E - kept <= extra_max)


# ---------------------------------------------------------------- whole-sequence passes (cases 1, 2, 3, 4, 5, 6)

@pytest.mark.parametrize("dbg", DEBUGS, ids=lambda d: f"{d:#x}")
def test_semi100_whole_pass(models, dbg):
    """case 1: B = 30 is no multiple of 16; speculative steps, reach events and exact replays all occur"""
    m = models("semi100")
    out = run(m, whole_pass(m), dbg)
    ndirty = check(m, out, whole_pass(m), dbg)
    st = out["stats"]
    print("semi100", hex(dbg), {k: st[k] for k in COUNTERS}, "gate", out["gate"], "dirty", ndirty)
    if not dbg & EAGER:
        assert st["beam_spec_steps"] > 0 and st["beam_reach_events"] > 0 and st["beam_exact_sets"] > 0
    assert bool(out["variants"] & TV_BEAM_Q16) == bool(dbg & Q16)


@pytest.mark.parametrize("dbg", DEBUGS, ids=lambda d: f"{d:#x}")
def test_all96_whole_pass(models, dbg):
    """case 2: every cut has more than 32 duplicates beyond the beam (immediate replays) and the walk meets tied cells"""
    m = models("all96")
    out = run(m, whole_pass(m), dbg)
    ndirty = check(m, out, whole_pass(m), dbg)
    st = out["stats"]
    print("all96", hex(dbg), {k: st[k] for k in COUNTERS}, "gate", out["gate"], "dirty", ndirty)
    S, _, Hv, _, _, _ = m.tables(0, m.T - 1, -1)
    assert all(straddle(S[r], Hv[r]) and not straddle(S[r], Hv[r], D.BEAM_EXTRA) for r in range(1, m.T))
    assert st["beam_exact_sets"] >= m.T - 1 and st["beam_spec_steps"] == 0
    assert out["gate"] != 0 and st["beam_ties"] > 0


@pytest.mark.parametrize("dbg", DEBUGS, ids=lambda d: f"{d:#x}")
def test_ds300_whole_pass(models, dbg):
    """case 3: an ordinary model — a few duplicated cuts, no tied cell on the path: the gate stays down"""
    m = models("ds300")
    out = run(m, whole_pass(m), dbg)
    ndirty = check(m, out, whole_pass(m), dbg)
    st = out["stats"]
    print("ds300", hex(dbg), {k: st[k] for k in COUNTERS}, "gate", out["gate"], "dirty", ndirty)
    assert st["beam_spec_steps"] + st["beam_exact_sets"] > 0
    if not dbg & ALL:
        assert out["gate"] == 0 and st["beam_ties"] == 0
        assert (ndirty > 0) == (not dbg & EAGER)         # steps stay dirty to the end: their invariants are not vacuous


def plan_generation(m, g, opath):
    """the passes of generation g of the N = 8 plan, conditioned on the oracle's decoded path"""
    return [(L, R, -1 if L == 0 else int(opath[L - 1]), int(opath[R]))
            for L, R, gen, _ in D.plan_passes(m.T, 8) if gen == g]


@pytest.mark.parametrize("dbg", DEBUGS, ids=lambda d: f"{d:#x}")
def test_semi1200_whole_pass_and_plan_generations(models, dbg):
    """case 4: the whole pass, then generations 1 and 2 of the N = 8 plan in batched lock-step launches"""
    m = models("semi1200")
    out = run(m, whole_pass(m), dbg)
    check(m, out, whole_pass(m), dbg)
    opath = m.om.beam_decode(m.ob, 8, m.beam, check=False)[0]
    for g in (1, 2):
        passes = plan_generation(m, g, opath)
        assert len(passes) >= 2
        out = run(m, passes, dbg)
        ndirty = check(m, out, passes, dbg)
        st = out["stats"]
        print("semi1200 gen", g, hex(dbg), {k: st[k] for k in COUNTERS}, "gate", out["gate"], "dirty", ndirty)
        assert st["passes"] == len(passes) and st["task_steps"] == sum(R - L for L, R, _, _ in passes)
        assert st["step_launches"] == max(R - L for L, R, _, _ in passes) < st["task_steps"]
        if not dbg & (ALL | EAGER):
            # a ties model whose gate stays down: undecided steps survive the generation, reach events happened on the way
            assert out["gate"] == 0 and ndirty > 0 and st["beam_spec_steps"] > 0
            assert g != 1 or (st["beam_reach_events"] > 0 and st["beam_exact_sets"] > 0)


BIG_DEBUGS = DEBUGS + (QUAD, NOCUT | Q16)


@pytest.mark.parametrize("dbg", BIG_DEBUGS, ids=lambda d: f"{d:#x}")
def test_fast7000_whole_pass(models, dbg):
    """case 5a: K >= 3 * 2048, the selects read candidate lists"""
    m = models("fast7000")
    out = run(m, whole_pass(m), dbg)
    ndirty = check(m, out, whole_pass(m), dbg)
    st = out["stats"]
    print("fast7000", hex(dbg), {k: st[k] for k in COUNTERS}, "gate", out["gate"], "dirty", ndirty)
    assert (st["beam_cand_selects"] > 0) == (not dbg & NOLISTS)
    if not dbg & (ALL | EAGER):
        assert out["gate"] == 0 and ndirty > 0 and st["beam_reach_events"] > 0


@pytest.mark.parametrize("dbg", BIG_DEBUGS, ids=lambda d: f"{d:#x}")
def test_semi7000_whole_pass(models, dbg):
    """case 5b: candidate lists under ties — lists that turn out too short are ignored"""
    m = models("semi7000")
    out = run(m, whole_pass(m), dbg)
    ndirty = check(m, out, whole_pass(m), dbg)
    st = out["stats"]
    print("semi7000", hex(dbg), {k: st[k] for k in COUNTERS}, "gate", out["gate"], "dirty", ndirty)
    if not dbg & NOLISTS:
        assert st["beam_list_short"] > 0


@pytest.mark.parametrize("dbg", BIG_DEBUGS, ids=lambda d: f"{d:#x}")
def test_ds16500_whole_pass(models, dbg):
    """case 6: K > 16384 — the 64-round select for the first two steps, topb_select_cand on the lists, beam_step_q16"""
    m = models("ds16500")
    out = run(m, whole_pass(m), dbg)
    ndirty = check(m, out, whole_pass(m), dbg)
    st = out["stats"]
    print("ds16500", hex(dbg), {k: st[k] for k in COUNTERS}, "gate", out["gate"], "dirty", ndirty)
    sel = out["selects"]
    if dbg & MANY:
        assert sel & D.TS_BITS["topb_select_cand<8,listed>"] and not sel & D.TS_BITS["topb_select<64,listed>"]
    else:
        assert sel & D.TS_BITS["topb_select<64,listed>"]
        assert bool(sel & D.TS_BITS["topb_select_cand<8,listed>"]) == (not dbg & NOLISTS)
    assert bool(out["variants"] & TV_BEAM_Q16) == bool(dbg & Q16)


# ---------------------------------------------------------------- chain cuts

@pytest.mark.parametrize("dbg", (0, NOCUT, ALL, Q16))
def test_chain_cuts_leave_exact_tables(models, dbg):
    """runs of undecided steps cut short by replay_safe (beam_chain_cuts > 0), and decided in full under bit 23: the
    dirty-step invariants hold both ways"""
    m = models("chain")
    out = run(m, whole_pass(m), dbg)
    ndirty = check(m, out, whole_pass(m), dbg)
    st = out["stats"]
    print("chain", hex(dbg), {k: st[k] for k in COUNTERS}, "gate", out["gate"], "dirty", ndirty)
    assert (st["beam_chain_cuts"] > 0) == (not dbg & NOCUT)
    assert st["beam_reach_events"] > 0 and out["gate"] != 0


# ---------------------------------------------------------------- case 7: more passes than one launch carries

def thirty_passes(m):
    """30 passes of 1 .. 12 steps laid along the sequence, some touching, conditioned on the oracle's decoded path"""
    opath = m.om.beam_decode(m.ob, 1, m.beam, check=False)[0]
    rs = np.random.RandomState(7)
    lens = rs.permutation(np.arange(30) % 12 + 1)
    passes, L = [], 0
    for i, n in enumerate(lens):
        R = L + int(n)
        passes.append((L, R, -1 if L == 0 else int(opath[L - 1]), int(opath[R])))
        L = R + 1 + (i % 3 == 2)                   # every third pass is followed by a gap
    assert L <= m.T
    return passes


@pytest.mark.parametrize("dbg", (ONE_STREAM, GROUPS, ONE_STREAM | ALL, GROUPS | ALL, ONE_STREAM | EAGER, GROUPS | NOCUT))
def test_thirty_passes_split_launches_and_derived_jobs(models, dbg):
    m = models("semi100")
    passes = thirty_passes(m)
    out = run(m, passes, dbg)
    ndirty = check(m, out, passes, dbg)
    st = out["stats"]
    print("thirty", hex(dbg), {k: st[k] for k in COUNTERS}, "gate", out["gate"], "dirty", ndirty, hex(out["selects"]))
    lens = sorted((R - L for L, R, _, _ in passes), reverse=True)
    ng = 1 if dbg & ONE_STREAM else 4
    launches = sum(-(-sum(1 for n in lens[g::ng] if n >= s) // 24) for g in range(ng) for s in range(1, 13))
    assert st["task_steps"] == sum(lens) and st["step_launches"] == launches
    derived, listed = D.TS_BITS["topb_select<4,derived>"], D.TS_BITS["topb_select<4,listed>"]
    assert bool(out["selects"] & derived) == (ng == 1) and out["selects"] & listed
    if not dbg & EAGER:
        assert st["beam_reach_events"] > 0 and (st["beam_chain_cuts"] > 0) == (not dbg & NOCUT)
    # rows outside every pass were left as the wrapper filled them
    covered = np.zeros(m.T, bool)
    for L, R, _, _ in passes:
        covered[L:R + 1] = True
    assert np.all(np.isnan(out["scores"][~covered])) and np.all(out["path"][~covered] == -2)


# ---------------------------------------------------------------- case 8: end states

def end_state_pass(m):
    """A right-hand pass whose last step is speculative for certain: its cut falls on duplicates a list can carry (at most
    32 beyond the beam) and the step before it has no duplicated cut (so it is not dirty and cannot be a reach event).
    Returns (L, R, init, S*[R], H*[R])."""
    opath = m.om.beam_decode(m.ob, 1, m.beam, check=False)[0]
    L = 40
    init = int(opath[L - 1])
    S, _, Hv, Hs, _, _ = m.tables(L, m.T - 1, init)
    for r in range(2, m.T - L):
        if not straddle(S[r - 1], Hv[r - 1]) and straddle(S[r], Hv[r], D.BEAM_EXTRA):
            return L, L + r, init, S[r], Hv[r], Hs[r]
    raise AssertionError("no step with a carried duplicate cut after a clean one")


@pytest.mark.parametrize("dbg", (0, NOCUT, ALL, EAGER))
def test_fixed_end_states_at_a_speculative_last_step(models, dbg):
    m = models("semi100")
    L, R, init, S, Hv, Hs = end_state_pass(m)
    theta = Hv.min()
    dup = np.nonzero(S == theta)[0]
    kept = [int(s) for s in dup if s in Hs.tolist()]
    lost = [int(s) for s in dup if s not in Hs.tolist()]
    assert kept and lost
    below = int(np.argmin(S))
    assert S[below] < theta
    for name, end in (("miss", below), ("kept", kept[0]), ("lost", lost[-1]), ("kept", kept[-1]), ("lost", lost[0])):
        p = (L, R, init, end)
        out = run(m, [p], dbg)
        check(m, out, [p], dbg)
        st = int(out["cut"][R, D.CUT_STATE])
        print("end", name, hex(dbg), "state", st, "exact_sets", out["stats"]["beam_exact_sets"], out["path"][L:R + 1].tolist()[-3:])
        assert (out["rc"] == D.WARN_BEAM_MISS) == (name != "kept")
        if dbg & EAGER:
            assert st == 2
        else:
            # the membership branch of beam_resolve mode 0: only an end state that is a cut duplicate decides the step
            assert st == (1 if name == "miss" else 2)


# ---------------------------------------------------------------- case 9: the CSR instantiations

def same_tables(a, b, passes, whole):
    for k in ("scores", "bp", "cut", "doubt_count", "path"):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
    n = np.nan_to_num(a["cut"][:, D.CUT_N]).astype(np.int64)                 # entries of every row's member list
    live = np.arange(a["member_val"].shape[1])[None, :] < n[:, None]
    for k in ("member_val", "member_state"):
        assert np.array_equal(a[k].view(np.uint32)[live], b[k].view(np.uint32)[live]), k
    assert a["gate"] == b["gate"] and a["rc"] == b["rc"] and bits(a["score"]) == bits(b["score"])
    for L, R, _, _ in passes:
        for t in range(L, R + 1):           # the lists are appended with atomics: equal as sets
            n = min(int(a["doubt_count"][t]), D.DOUBT_CAP)
            assert sorted(a["doubt"][t, :n].tolist()) == sorted(b["doubt"][t, :n].tolist()), t
        rows = range(L, R + 1) if a["gate"] else ([R] if whole else [])
        for t in rows:
            assert np.array_equal(bits(a["slot_val"][t]), bits(b["slot_val"][t])), t
            assert np.array_equal(a["slot_state"][t], b["slot_state"][t]), t


@pytest.mark.parametrize("name", ["semi100", "all96", "semi1200"])
def test_sparse_set_model_gives_the_same_tables(models, name):
    """FV_OPT_SPARSE_BEAM: the CSR forms of patch_doubtful, tie_fixup and beam_resolve leave the dense forms' bytes"""
    m = models(name)
    sp = m.sparse()
    jobs = [whole_pass(m)]
    if name == "semi1200":
        opath = m.om.beam_decode(m.ob, 8, m.beam, check=False)[0]
        jobs += [plan_generation(m, 1, opath), plan_generation(m, 2, opath)]
    seen = dict(beam_reach_events=0, beam_exact_sets=0, beam_ties=0)
    for passes in jobs:
        for dbg in (0, ALL, NOCUT, EAGER):
            dense = run(m, passes, dbg)
            got = run(m, passes, dbg, fv=sp)
            assert got["variants"] == D.TV_BEAM_CSR and got["stats"]["kernel"] == D.KERNEL_CSR_F64
            same_tables(got, dense, passes, passes == whole_pass(m))
            check(m, got, passes, dbg)
            for k in seen:
                assert got["stats"][k] == dense["stats"][k], (k, dbg)
                seen[k] += got["stats"][k]
    print("sparse", name, seen)
    assert seen["beam_exact_sets"] > 0 and seen["beam_ties"] > 0
    assert name == "all96" or seen["beam_reach_events"] > 0


# ---------------------------------------------------------------- case 10: staged emission rows

def test_emission_rows_give_the_symbol_routes_tables(models):
    m = models("ds300")
    m.stage_emissions()
    for dbg in (0, ALL, Q16):
        want = run(m, whole_pass(m), dbg)
        got = run(m, whole_pass(m), dbg, emissions=True)
        same_tables(got, want, whole_pass(m), True)
        check(m, got, whole_pass(m), dbg)
        assert got["variants"] == want["variants"] and got["stats"]["emission_rows"] == m.T


# ---------------------------------------------------------------- refusals

def test_refusals(models):
    m = models("semi100")
    T, K = m.T, m.K

    def refused(passes, beam=None, rc=D.ERR_ARG):
        with pytest.raises(D.FlashVitError) as e:
            m.fv.test_beam_forward(m.ob, beam or m.beam, passes)
        assert e.value.rc == rc, str(e.value)

    refused([(5, 5, 1, 1)])                                  # R <= L
    refused([(0, T, -1, -1)])                                # R >= T
    refused([(0, 9, 3, 1)])                                  # a state in front of time 0
    refused([(1, 9, K, 1)])
    refused([(1, 9, 1, -2)])
    refused([(1, 9, 1, 1), (9, 12, 1, 1)])                   # overlap
    refused([(1, 9, 1, 1), (10, 12, 2, 1)])                  # touching passes that disagree
    refused([(2 * i, 2 * i + 1, -1, 0) for i in range(65)])  # more than 64
    refused([(1, 9, 1, 1)], beam=K + 1)
    bad = m.ob.copy()
    bad[7] = m.spec["M"]
    with pytest.raises(D.FlashVitError):
        m.fv.test_beam_forward(bad, m.beam, [(0, T - 1, -1, -1)])
    out = m.fv.test_beam_forward(m.ob, m.beam, [(1, 9, 1, 1), (10, 12, 1, 1)])      # touching passes that agree
    assert out["path"][9] == 1 and out["path"][12] == 1
