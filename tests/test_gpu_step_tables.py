"""GPU: whole step tables of the full-state and beam step kernels against the oracle.

Every other full-state test checks what a decode returns: T path entries and one score.  A step computes K scores and
K back-pointers, and a decode reads one back-pointer of each step, so a kernel can be wrong in a column the optimum
does not pass through, or in a batch slot, slab or tile the fixtures do not reach, and those tests stay green.  Here
fv_test_forward (include/flashvit_testing.h) runs caller-chosen passes as one generation of the full-state driver and
returns every back-pointer row and each pass's final score row; the oracle's full_forward computes the same tables
cell by cell.  Scores must be bit-equal, back-pointers equal (-1 where a column has no finite predecessor), in every
column, for every kernel, forced form, batch limit, and K on both sides of each launch-regime boundary:

   4096 / 4097     more 16-column tiles than CUs: the 16-bit tables and the packed kernel leave their whole-tile forms
   4320 / 4321     batched launches of 8 tasks -> 4 (score rows in LDS)
   9440 / 9441     4 -> 2
  19680 / 19681    2 -> 1
  40160 / 40161    a float32 score row no longer fits LDS: no f32 / f16 / sparse table, float64 and Q16 in slabs

The beam half makes single launches of the beam step kernel through fv_test_beam_step over given slot sets and compares
scores, back-pointers, tie tags and list, doubt list and candidate list with the oracle's beam_step_probe (slots in order
and reversed).  Every hook call is made twice (the tables must be identical), and the union of the step-kernel
instantiations that ran over the module must be every FV_TV_* bit of the header."""
import math
import os
import re
import time

import numpy as np
import pytest

import modelgen
import oracle
from conftest import ROOT
from flash_viterbi_amd import decoder, hostio

pytestmark = pytest.mark.gpu

D = decoder
KERNELS = {"auto": D.KERNEL_AUTO, "f64": D.KERNEL_F64_STREAM, "f32": D.KERNEL_F32_REFINE, "f16": D.KERNEL_F16_REFINE,
           "q16": D.KERNEL_Q16_REFINE, "sparse": D.KERNEL_SPARSE_Q16, "u16": D.KERNEL_U16_REFINE}
SLABS = 1 << 21
# FV_OPT_DEBUG forms per kernel: 2 no reverse sweep, 4 alternate load schedule, 8192 packed kernel in 16-wave workgroups,
# 16384 packed kernel for batched launches, 262144 no forked streams, 1 << 21 three slabs of source rows
FORMS = {"auto": (0,), "f64": (0, 2, SLABS), "f32": (0, 2, 4, SLABS), "f16": (0, 2, 4, SLABS), "q16": (0, 2, 4, SLABS),
         "sparse": (0, 262144),
         "u16": (0, 2, 4, 8192, 8192 | 4, 16384, 16384 | 8192, 16384 | 8192 | 4, 16384 | 4, 262144 | 16384,
                 262144 | 16384 | 4)}
BATCHES = (1, 2, 3, 8)
BP_FILL = -2

_reached = {"variants": 0, "tests": set()}


def header_variants():
    """{bit: (macro, instantiation)} of include/flashvit_testing.h"""
    text = open(os.path.join(ROOT, "include", "flashvit_testing.h")).read()
    out = {}
    for name, bit, what in re.findall(r"#define\s+(FV_TV_\w+)\s+\(1ull << (\d+)\)\s*/\*\s*(.*?)\s*\*/", text):
        out[int(bit)] = (name, what)
    return out


# ---------------------------------------------------------------- models and pass sets

def one_state_model(M, T, seed):
    rs = np.random.RandomState(seed)
    Bm = rs.uniform(0.1, 1.0, (1, M))
    Bm /= Bm.sum()
    return (np.ones((1, 1), np.float32), hostio.quantize_text16(Bm), np.ones(1, np.float32),
            rs.randint(0, M, T).astype(np.int32))


def build_model(kind, K, T, seed, prob=0.112, M=8):
    if K == 1:
        return one_state_model(M, T, seed)
    if kind in ("wideA", "wideB"):
        return modelgen.wide_model(kind, K, M, T, seed)
    if kind == "unreachable":
        # every 7th column of A zero, a third of Pi zero (the golden unreachable_K300_T40 is this model)
        return modelgen.unreachable_model(K, M, T, seed)
    if kind == "data_script" and K < 64:
        # (the generator leaves a row without out-edges unnormalised, NaN, which small K draws often; the vectorised
        # builder of the same distributions gives such a row one edge)
        kind = "sparse_fast"
    return modelgen.model32(dict(kind=kind, K=K, M=M, T=T, prob=prob, seed=seed))


def lowest_live_predecessors(A, init_state, steps):
    """Per step, for every column the lowest state that has a finite score and an edge into it (-1: none)."""
    E = A > 0
    live = np.ones(A.shape[0], dtype=bool) if init_state < 0 else E[init_state].copy()
    out = []
    for _ in range(steps):
        cand = E & live[:, None]
        has = cand.any(axis=0)
        out.append(np.where(has, np.argmax(cand, axis=0), -1))
        live = has
    return np.array(out, dtype=np.int32)


def pass_set(lengths, K, seed):
    """Passes of the given lengths, one after another with gaps of 0 or 1 time steps; the first starts from Pi at
    L = 0, the others from a random state.  Returned in a shuffled order (the hook maps its rows back by L) with the
    sequence length they need."""
    rs = np.random.RandomState(seed)
    passes, L = [], 0
    for n in lengths:
        passes.append((L, L + n, -1 if L == 0 else int(rs.randint(0, K))))
        L += n + 1 + int(rs.randint(0, 2))
    order = rs.permutation(len(passes))
    return [passes[i] for i in order], L


# unequal lengths: with a batch limit of 8 the launches carry 8, 7, ... 1 tasks; with 3: 3, 3, 2 ...
BATCH_SET = (9, 8, 6, 5, 4, 3, 2, 1)
# five or more passes of 64+ steps: the forked-stream generation of the packed 16-bit kernel and the sparse walk
FORK_SET = (70, 64, 66, 80, 64, 65)


class Case:
    """One model on the device and in the oracle; the oracle's tables per pass set are computed once."""

    def __init__(self, A, Bm, Pi, ob):
        self.A, self.Bm, self.Pi, self.ob = A, Bm, Pi, ob
        self.K = A.shape[0]
        self.om = oracle.OracleModel(A, Bm, Pi)
        self.fv = decoder.FlashViterbi(0)
        self.fv.set_model(A, Bm, Pi)
        self._want = {}

    def close(self):
        self.fv.close()
        self.om.close()

    def want(self, passes):
        key = tuple(passes)
        if key not in self._want:
            self._want[key] = [self.om.full_forward(self.ob, L, R, s) for L, R, s in passes]
        return self._want[key]

    def run(self, passes, kernel, debug=0, batch=8):
        fv = self.fv
        fv.set_option(D.OPT_KERNEL, KERNELS[kernel])
        fv.set_option(D.OPT_DEBUG, debug)
        fv.set_option(D.OPT_MAX_BATCH, batch)
        rows, bp, var = fv.test_forward(self.ob, passes, BP_FILL)
        rows2, bp2, var2 = fv.test_forward(self.ob, passes, BP_FILL)
        where = f"K={self.K} kernel={kernel} debug={debug} batch={batch}"
        assert np.array_equal(rows.view(np.uint32), rows2.view(np.uint32)) and np.array_equal(bp, bp2) and var == var2, \
            f"{where}: two calls gave different tables"
        _reached["variants"] |= var
        self.check(passes, rows, bp, where)
        return var

    def check(self, passes, rows, bp, where):
        covered = np.zeros(bp.shape[0], dtype=bool)
        for q, (L, R, s) in enumerate(passes):
            row, args = self.want(passes)[q]
            bad = np.nonzero(rows[q].view(np.uint32) != row.view(np.uint32))[0]
            assert bad.size == 0, (f"{where} pass ({L},{R},{s}): final score row differs in {bad.size} columns, "
                                   f"first {bad[:8].tolist()}: got {rows[q][bad[:4]].tolist()} want {row[bad[:4]].tolist()}")
            got = bp[L + 1:R + 1]
            diff = np.argwhere(got != args)
            if diff.size:
                j, c = diff[0]
                pytest.fail(f"{where} pass ({L},{R},{s}): {len(diff)} back-pointers differ; first at time {L + 1 + j} "
                            f"column {c}: got {got[j, c]} want {args[j, c]}; columns of that row: "
                            f"{np.nonzero(got[j] != args[j])[0][:12].tolist()}")
            covered[L + 1:R + 1] = True
        assert (bp[~covered] == BP_FILL).all(), f"{where}: the hook wrote back-pointer rows outside its passes"


def record(name):
    _reached["tests"].add(name)


def sweep(case, passes, kernels=KERNELS, batches=BATCHES):
    for kernel in kernels:
        for debug in FORMS[kernel]:
            for batch in batches:
                case.run(passes, kernel, debug, batch)


# ---------------------------------------------------------------- argument checks

def test_hook_refuses_bad_pass_sets():
    record("refuses")
    A, Bm, Pi, ob = build_model("data_script", 64, 40, 5)
    fv = decoder.FlashViterbi(0)
    try:
        fv.set_model(A, Bm, Pi)
        for passes in ([(3, 3, 1)], [(5, 2, 1)], [(0, 10, -1), (10, 20, 3)], [(0, 10, -1), (4, 8, 3)], [(5, 9, -1)],
                       [(0, 5, 3)], [(2, 6, 64)], [(0, 40, -1)], [(-1, 4, -1)]):
            with pytest.raises(decoder.FlashVitError) as e:
                fv.test_forward(ob, passes)
            assert e.value.rc == -1, passes
        bad_ob = ob.copy()
        bad_ob[7] = 8
        with pytest.raises(decoder.FlashVitError):
            fv.test_forward(bad_ob, [(0, 10, -1)])
        # adjacent passes are fine: [0, 10] and [11, 20] (the second starts from a state at time 10)
        fv.test_forward(ob, [(0, 10, -1), (11, 20, 3)])
    finally:
        fv.close()
    group = decoder.FlashViterbi([0, 0])          # a multi-device context (one device listed twice)
    try:
        group.set_model(A, Bm, Pi)
        with pytest.raises(decoder.FlashVitError) as e:
            group.test_forward(ob, [(0, 10, -1)])
        assert e.value.rc == -1
    finally:
        group.close()


# ---------------------------------------------------------------- small K: every kernel, form and batch limit

@pytest.mark.parametrize("K", [1, 2, 17, 31, 32, 33, 257, 1000])
def test_small_k_every_kernel_form_and_batch(K):
    record(f"small{K}")
    passes, T = pass_set(BATCH_SET, K, 100 + K)
    case = Case(*build_model("data_script", K, T + 3, 200 + K, prob=0.112 if K < 1000 else 0.02))
    try:
        sweep(case, passes)
        single, _ = pass_set((T - 2,), K, 7)                 # one pass over (nearly) everything
        three = [(5, 12, int(case.ob[0]) % K), (14, 30, 0), (31, 33, K - 1)]
        for kernel in KERNELS:
            case.run(single, kernel)
            case.run(three, kernel, batch=3)
    finally:
        case.close()


MODELS = [("data_script", 1000, 0.02), ("data_script", 700, 0.112), ("data_script", 600, 0.9), ("ties_all", 512, 0.5),
          ("wideA", 600, None), ("wideB", 600, None), ("unreachable", 300, None)]


@pytest.mark.parametrize("kind,K,prob", MODELS, ids=[f"{m[0]}-K{m[1]}" + (f"-p{m[2]}" if m[2] else "") for m in MODELS])
def test_models_every_kernel_form_and_batch(kind, K, prob):
    record(f"model-{kind}-{K}")
    passes, T = pass_set(BATCH_SET, K, 300 + K)
    case = Case(*build_model(kind, K, T + 2, 400 + K, prob=prob))
    try:
        want = case.want(passes)
        if kind == "unreachable":
            # the case is what it claims: columns without a finite predecessor, -inf entries in the Pi row
            assert all((args == -1).any() for _, args in want)
            assert any((row == -np.finfo(np.float32).max).any() for row, _ in want)
            assert (case.Pi == 0).any()
        if kind == "ties_all":
            # every finite candidate of a column is the same float: each back-pointer is the lowest finite predecessor
            for (L, R, st), (_, args) in zip(passes, want):
                assert np.array_equal(args, lowest_live_predecessors(case.A, st, R - L)), (L, R, st)
        sweep(case, passes, batches=(1, 3, 8))
    finally:
        case.close()


@pytest.mark.parametrize("K", [257, 1000])
def test_forked_generation_long_passes(K):
    """Six passes of 64+ steps: the packed 16-bit kernel and the sparse walk deal batches of four to three streams."""
    record(f"fork{K}")
    passes, T = pass_set(FORK_SET, K, 500 + K)
    case = Case(*build_model("data_script", K, T + 1, 600 + K, prob=0.02))
    try:
        for kernel, debug in (("u16", 0), ("u16", 16384), ("u16", 16384 | 4), ("sparse", 0), ("sparse", 262144), ("auto", 0),
                              ("q16", 0), ("f64", 0)):
            case.run(passes, kernel, debug, 8)
        # the same model through the sparse walk's dense-model path: p = 0.9, forced
        case.close()
        case = Case(*build_model("data_script", K, T + 1, 700 + K, prob=0.9))
        case.run(passes, "sparse", 0, 8)
        case.run(passes, "u16", 0, 8)
    finally:
        case.close()


# ---------------------------------------------------------------- launch-regime boundaries

# (K, pass lengths): a few steps per pass; enough passes for the largest batch the regime allows
BOUNDARIES = [(4096, (4, 4, 3, 3, 2, 2, 1, 1)), (4097, (4, 4, 3, 3, 2, 2, 1, 1)), (4320, (4, 3, 3, 2, 2, 2, 1, 1)),
              (4321, (4, 3, 3, 2, 2, 2, 1, 1)), (9440, (4, 3, 2, 2, 1)), (9441, (4, 3, 2, 2, 1)), (19680, (3, 2, 1)),
              (19681, (3, 2, 1)), (40160, (2, 2, 1)), (40161, (2, 2, 1, 1))]


@pytest.mark.parametrize("K,lengths", BOUNDARIES, ids=[f"K{b[0]}" for b in BOUNDARIES])
def test_launch_regime_boundaries(K, lengths):
    record(f"boundary{K}")
    t0 = time.time()
    passes, T = pass_set(lengths, K, 800 + K)
    A, Bm, Pi, ob = modelgen.model32(dict(kind="sparse_fast", K=K, M=8, T=T + 1, prob=0.02, seed=900 + K))
    case = Case(A, Bm, Pi, ob)
    try:
        case.want(passes)
        big = K > 40160
        batches = (8, 3) if K <= 9441 else (8,)
        for kernel in KERNELS:
            if big and kernel in ("f32", "f16", "sparse"):
                # like fv_decode_full: no float32 score row fits LDS, so these kernels cannot take the model
                case.fv.set_option(D.OPT_KERNEL, KERNELS[kernel])
                case.fv.set_option(D.OPT_DEBUG, 0)
                with pytest.raises(decoder.FlashVitError) as e:
                    case.fv.test_forward(ob, passes)
                assert e.value.rc == -6
                with pytest.raises(decoder.FlashVitError):
                    case.fv.decode_full(ob, 1)
                continue
            forms = (0,)
            if kernel == "u16" and K <= 4321:
                forms = (0, 16384 | 262144, 8192 | 16384 | 262144)
            for debug in forms:
                for batch in batches:
                    case.run(passes, kernel, debug, batch)
    finally:
        case.close()
    print(f"K={K}: {time.time() - t0:.1f} s")


# ---------------------------------------------------------------- beam step

# FV_OPT_DEBUG of the beam step: library's choice, float64 rows (16- / 4-wave by B), 16-bit filter (16-wave, 8-wave)
BEAM_DEBUG = (0, 256, 256 | (1 << 25), 512, 512 | (1 << 25), 512 | (1 << 26))
FLT_MAX = float(np.finfo(np.float32).max)


def uniform_model(K, M, seed):
    """Every transition weight 1/K except column 0 (unreachable for K >= 3): all cells of a column tie wherever the
    entries' values do."""
    rs = np.random.RandomState(seed)
    A = np.full((K, K), 1.0 / K)
    if K >= 3:
        A[:, 0] = 0.0
    Bm = np.full((K, M), 1.0 / M)
    ob = rs.randint(0, M, 4).astype(np.int32)
    return hostio.quantize_text16(A), hostio.quantize_text16(Bm), hostio.quantize_text16(np.full(K, 1.0 / K)), ob


def beam_model(kind, K, seed):
    if kind == "uniform":
        return uniform_model(K, 4, seed)
    if kind == "wide":
        return modelgen.wide_model("wideA", K, 6, 4, seed)
    if kind == "sparse":
        return modelgen.model32(dict(kind="sparse_fast", K=K, M=6, T=4, prob=0.01, seed=seed))
    return modelgen.model32(dict(kind="ties_all", K=K, M=4, T=4, prob=0.5, seed=seed))


def slot_values(rs, n, tie_heavy):
    if tie_heavy:
        return rs.choice(np.array([-3.0, -3.5, -4.0, -7.25], np.float32), n).astype(np.float32)
    return (-(rs.uniform(0, 1, n) * 10.0 ** rs.uniform(-2, 2.5, n))).astype(np.float32)


class BeamCase:
    def __init__(self, A, Bm, Pi, ob):
        self.A, self.Bm = A, Bm
        self.K, self.M = A.shape[0], Bm.shape[1]
        self.om = oracle.OracleModel(A, Bm, Pi)
        self.fv = decoder.FlashViterbi(0)
        self.fv.set_model(A, Bm, Pi)

    def close(self):
        self.fv.close()
        self.om.close()

    def make_sets(self, rs, nsets, B, extra=0, tie_heavy=True):
        """nsets slot sets of B + extra entries on distinct states; with extra > 0 the last 1 + extra entries hold the
        cut value theta (a speculative list: B - 1 members above the cut, every duplicate at it)."""
        sets, syms = [], rs.randint(0, self.M, nsets)
        theta = np.float32(-5.0) if tie_heavy else np.float32(-rs.uniform(1.0, 50.0))
        for _ in range(nsets):
            n = B + extra
            vals = slot_values(rs, n, tie_heavy)
            states = rs.choice(self.K, n, replace=False).astype(np.int32)
            if extra:
                above = (rs.choice(np.array([-3.0, -3.5, -4.0], np.float32), B - 1) if tie_heavy else
                         np.maximum(theta + np.abs(slot_values(rs, B - 1, False)), np.nextafter(theta, np.float32(0))))
                vals = np.concatenate([above.astype(np.float32), np.full(1 + extra, theta, np.float32)])
                order = rs.permutation(n)
                vals, states = vals[order], states[order]
            sets.append((vals, states))
        return sets, syms, theta

    def expect(self, vals, states, o):
        fs, fa = self.om.beam_step_probe(vals, states, o, blocked=False)
        rs_, ra = self.om.beam_step_probe(vals[::-1], states[::-1], o, blocked=False)
        assert np.array_equal(fs.view(np.uint32), rs_.view(np.uint32))
        n = vals.size
        rev = np.where(ra >= 0, n - 1 - ra, -1)
        return fs, fa, (fa >= 0) & (fa != rev)

    def cell(self, v, s, col, o):
        tmp = np.float32(math.log(float(self.Bm[col, o])))
        return np.float32(float(np.float32(tmp + np.float32(v))) + math.log(float(self.A[s, col])))

    def run(self, B, sets, syms, debug, speculative=False, theta=0.0, bound=float("inf"), cand_cap=0):
        fv = self.fv
        fv.set_option(D.OPT_DEBUG, debug)
        where = f"beam K={self.K} B={B} n={sets[0][0].size} sets={len(sets)} debug={debug} spec={speculative}"
        got = fv.test_beam_step(B, sets, syms, speculative, theta, bound, cand_cap)
        again = fv.test_beam_step(B, sets, syms, speculative, theta, bound, cand_cap)
        assert np.array_equal(got["scores"].view(np.uint32), again["scores"].view(np.uint32)), where
        assert np.array_equal(got["bp"], again["bp"]) and got["ties"] == again["ties"], where
        # lists as sets; a list whose count exceeds its capacity holds whichever entries came first: the count only
        lists = lambda r, key, cap: [(c, set(x) if c <= cap else None) for c, x in r[key]]
        assert lists(got, "doubt", 1024) == lists(again, "doubt", 1024), where
        assert lists(got, "cand", cand_cap) == lists(again, "cand", cand_cap), where
        _reached["variants"] |= got["variants"]
        want_ties = set()
        for q, ((vals, states), o) in enumerate(zip(sets, syms)):
            fs, fa, tied = self.expect(vals, states, o)
            sc, bp = got["scores"][q], got["bp"][q]
            bad = np.nonzero(sc.view(np.uint32) != fs.view(np.uint32))[0]
            assert bad.size == 0, f"{where} set {q}: scores differ in {bad.size} columns, first {bad[:8].tolist()}"
            none = fa < 0
            assert (bp[none] == -1).all() and (sc[none] == -FLT_MAX).all(), f"{where} set {q}: unreachable columns"
            tag = (bp >= 0) & ((bp & D.TIE_TAG) != 0)
            wrong = np.nonzero(tag != tied)[0]
            assert wrong.size == 0, (f"{where} set {q}: TIE_TAG differs from the tied cells in columns {wrong[:8].tolist()} "
                                     f"(tagged {tag[wrong[:4]].tolist()})")
            plain = ~none & ~tied
            diff = np.nonzero(bp[plain] != states[fa[plain]])[0]
            assert diff.size == 0, f"{where} set {q}: back-pointers differ in columns {np.nonzero(plain)[0][diff[:8]].tolist()}"
            slot_of = {int(st): e for e, st in enumerate(states)}
            for col in np.nonzero(tied)[0]:
                st = int(bp[col] & ~D.TIE_TAG)
                assert st in slot_of and self.cell(vals[slot_of[st]], st, col, o) == fs[col], f"{where} set {q} column {col}"
                want_ties.add((q, int(col)))
            # doubt list: speculative sets only; columns whose maximum only theta-valued entries attain must be listed,
            # columns whose maximum no theta-valued entry attains must not
            count, listed = got["doubt"][q]
            if not speculative:
                assert count == 0, where
            else:
                th = vals == theta
                mt = self.om.beam_step_probe(vals[th], states[th], o, blocked=False)[0]
                mo = self.om.beam_step_probe(vals[~th], states[~th], o, blocked=False)[0] if (~th).any() else np.full(self.K, -np.inf, np.float32)
                by_t, by_o = ~none & (mt == fs), ~none & (mo == fs)
                must, never = set(np.nonzero(by_t & ~by_o)[0].tolist()), set(np.nonzero(~by_t)[0].tolist())
                assert len(listed) == len(set(listed)) and not (set(listed) & never), f"{where} set {q}: doubt lists a column no duplicate wins"
                assert count >= len(must), where
                if count <= 1024:
                    assert len(listed) == count and must <= set(listed), f"{where} set {q}: doubt misses {sorted(must - set(listed))[:8]}"
            if cand_cap:
                fin = np.nonzero((fs > -FLT_MAX) & (fs >= np.float32(bound)))[0]
                count, lst = got["cand"][q]
                assert count == fin.size, f"{where} set {q}: {count} candidates, want {fin.size}"
                if count <= cand_cap:
                    assert {(float(v), c) for v, c in lst} == {(float(fs[c]), int(c)) for c in fin}, f"{where} set {q}: candidate list"
        assert got["ties"] == want_ties, f"{where}: tie list differs from the tied cells"
        return got


BEAM_CASES = [("uniform", 2, 2), ("uniform", 64, 2), ("uniform", 64, 16), ("uniform", 64, 63), ("uniform", 64, 64),
              ("uniform", 65, 65), ("uniform", 127, 64), ("uniform", 128, 65), ("uniform", 129, 127), ("wide", 600, 63),
              ("wide", 600, 255), ("ties_all", 3965, 64), ("ties_all", 3965, 255), ("ties_all", 3965, 1024),
              ("sparse", 16500, 1024)]


@pytest.mark.parametrize("kind,K,B", BEAM_CASES, ids=[f"{c[0]}-K{c[1]}-B{c[2]}" for c in BEAM_CASES])
def test_beam_step_matrix(kind, K, B):
    record(f"beam-{kind}-{K}-{B}")
    rs = np.random.RandomState(K * 7 + B)
    case = BeamCase(*beam_model(kind, K, 1000 + K))
    try:
        for nsets in ((1, 3) if K * B > 4e6 else (1, 3, 24)):
            sets, syms, _ = case.make_sets(rs, nsets, B, tie_heavy=kind != "wide")
            fs0 = case.expect(*sets[0], syms[0])[0]
            fin = np.sort(fs0[fs0 > -FLT_MAX])
            bound = float(fin[-min(fin.size, B + B // 2)]) if fin.size else float("inf")
            for i, debug in enumerate(BEAM_DEBUG):
                cap = 0 if i == 1 else 2 * B + 7
                case.run(B, sets, syms, debug, bound=bound if i % 2 == 0 else float("inf"), cand_cap=cap)
    finally:
        case.close()


@pytest.mark.parametrize("kind", ["ties_all", "wide"])
@pytest.mark.parametrize("B", [30, 64, 100, 257])
def test_beam_step_speculative_lists(kind, B):
    """Speculative lists of B + E entries (E = 1, 15, 16, 17, 32), every duplicate at the cut value theta: the extra
    entries are swept separately, with the residue of B modulo the waves (the class of DESIGN.md's
    "The bug the adversarial tests found")."""
    record(f"spec-{kind}-{B}")
    rs = np.random.RandomState(B + (0 if kind == "wide" else 5000))
    case = BeamCase(*beam_model(kind, 600, 1100 + B))
    try:
        for E in (1, 15, 16, 17, 32):
            sets, syms, theta = case.make_sets(rs, 3, B, extra=E, tie_heavy=kind != "wide")
            for debug in BEAM_DEBUG:
                case.run(B, sets, syms, debug, speculative=True, theta=float(theta), cand_cap=2 * B)
        sets, syms, theta = case.make_sets(rs, 2, B, extra=16, tie_heavy=kind != "wide")
        case.run(B, sets, syms, 512, speculative=False, theta=float(theta))        # the same list, not speculative: no doubt
    finally:
        case.close()


def test_beam_step_largest_accepted_width():
    """The largest B fv_decode_beam accepts (the admission is shared with the hook) at K = 16500."""
    record("beam-largest")
    case = BeamCase(*beam_model("sparse", 16500, 1200))
    rs = np.random.RandomState(12)
    try:
        lo, hi = 1024, 16500
        while lo < hi:                                   # largest B the hook admits
            mid = (lo + hi + 1) // 2
            try:
                case.fv.test_beam_step(mid, [(np.zeros(mid, np.float32), np.arange(mid, dtype=np.int32))], [0])
                lo = mid
            except decoder.FlashVitError as e:
                assert e.rc == -6
                hi = mid - 1
        B = lo
        assert B < 16500
        ob = np.zeros(2, np.int32)
        with pytest.raises(decoder.FlashVitError) as e:
            case.fv.decode_beam(ob, 1, B + 1)
        assert e.value.rc == -6
        sets, syms, _ = case.make_sets(rs, 1, B, tie_heavy=False)
        for debug in (0, 256, 512):
            case.run(B, sets, syms, debug)
    finally:
        case.close()


# ---------------------------------------------------------------- coverage

def test_zz_every_step_instantiation_ran():
    """Runs last: the union of variants_out over the module is every FV_TV_* bit of include/flashvit_testing.h."""
    expected = {"refuses"} | {f"small{K}" for K in (1, 2, 17, 31, 32, 33, 257, 1000)} | \
               {f"model-{m[0]}-{m[1]}" for m in MODELS} | {"fork257", "fork1000"} | {f"boundary{b[0]}" for b in BOUNDARIES} | \
               {f"beam-{c[0]}-{c[1]}-{c[2]}" for c in BEAM_CASES} | {f"spec-{k}-{B}" for k in ("ties_all", "wide") for B in (30, 64, 100, 257)} | \
               {"beam-largest"}
    if not expected <= _reached["tests"]:
        pytest.skip("needs the whole module")
    bits = header_variants()
    assert len(bits) == 50 and sorted(bits) == list(range(50))
    missing = [f"{bits[b][0]} = {bits[b][1]}" for b in sorted(bits) if not (_reached["variants"] >> b) & 1]
    assert not missing, "step-kernel instantiations no test launched: " + "; ".join(missing)
    assert _reached["variants"] >> 50 == 0
