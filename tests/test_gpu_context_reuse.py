"""GPU: one context kept alive across models, shapes and entry points, judged call by call.

A context owns its workspace for life: buffers grow and never shrink, every entry point draws on them, and a model setter
keeps them while it changes K and with it the pitch of every score row.  What a call finds there is whatever the calls
before it left.  Three parts, every comparison an equality:

1. Every entry point in a seeded shuffled order on one long-lived context, across model changes in both directions and
   between the dense and the CSR setter.  Two judges per call: the CPU oracle (path, float32 score by bits, return code;
   tests/stream_model.py and tests/lag_model.py for streams and sets) and a FRESH context that runs the same call alone —
   its results, and the statistics that must describe this call and nothing before it (STAT_KEYS, the stream, set and lag
   counters).  The same on a [0, 0] multi-device context with every call it admits: it refuses the batch decodes, the
   test hooks, streams and sets, and never takes the flat route (asserted), so those closures and the flat-route ones
   stay on the single device; a batch decode on staged rows is asserted refused there.
2. Stale pads, set up on purpose: a model without row pads fills every column of every score row, code row and checkpoint
   row; a model of another K then decodes far lower scores in the same memory, and device_bytes proves that nothing grew
   (so nothing was cleared) in between.
3. Streams and sets through the launch forms of FV_OPT_DEBUG (bit 21, the slab route, among them) and after a decode that
   took the FV_OPT_ROW_CODES route.

A route a case names is asserted as taken: stats()["kernel"], flat_passes, the FV_TV_* bits of fv_test_forward.
"""
import functools

import numpy as np
import pytest

import lag_model as lm
import modelgen
import oracle
import stream_model as sm
from conftest import golden_model, load_goldens
from flash_viterbi_amd import decoder
from test_gpu_beam_tables import check_pass
from test_gpu_emissions import libm_log
from test_gpu_emissions_tied import bf16_to_f32, f32_to_bf16_bits
from test_gpu_step_tables import pass_set
from test_gpu_stream import run_stream
from test_gpu_streams import run_set, schedule, slot_ob

pytestmark = pytest.mark.gpu

D = decoder
REF, SINGLE = D.MODE_REFERENCE, D.MODE_SINGLE_PASS
AUTO, F64, F32, F16, Q16, SPQ, U16 = (D.KERNEL_AUTO, D.KERNEL_F64_STREAM, D.KERNEL_F32_REFINE, D.KERNEL_F16_REFINE,
                                       D.KERNEL_Q16_REFINE, D.KERNEL_SPARSE_Q16, D.KERNEL_U16_REFINE)
ALT, W16, PACKED, SLABS, CSR_MEM = 1 << 2, 1 << 13, 1 << 14, 1 << 21, D.DEBUG_CSR_ROWS_IN_MEMORY
TV_SLAB = {F64: 1 << 22, F32: 1 << 23, F16: 1 << 24, Q16: 1 << 25}       # FV_TV_SLAB_*
TV_SLAB_ANY = 0xF << 22
TV_CSR_LDS, TV_CSR_MEM = 0xF << 50, 0xF << 54                             # FV_TV_CSR_LDS_NB* / FV_TV_CSR_MEM_NB*
# what fv_last_stats must report of the call before it and of nothing else: the tuple tests/test_gpu_batch.py treats as
# deterministic, COUNTERS of tests/test_gpu_beam_launch_counts.py, and the plan, route and staging members
STAT_KEYS = ("cells", "task_steps", "column_steps", "alg_bytes", "passes", "refine_near", "refine_rescan", "refine_saturated",
             "beam_spec_steps", "beam_reach_events", "beam_exact_sets", "beam_cand_selects", "beam_list_short", "beam_list_long",
             "beam_ties", "beam_chain_cuts", "bt_restarts", "generations", "kernel", "flat_passes", "flat_missed",
             "flat_first_miss", "emission_rows")
M = 8
CHECK = 4                  # check interval of every stream and set here
PUSH = 16


def bits(x):
    return int(np.float32(x).view(np.uint32))


def tri(res):
    path, score, rc = res
    return (np.asarray(path).tolist(), bits(score), int(rc))


def det(fv):
    s = fv.stats()
    return tuple((k, s[k]) for k in STAT_KEYS)


def attempt(call):
    """a decode through the wrapper; a negative return code is reported, not raised (its path is the reference's 'undefined')"""
    try:
        return tri(call())
    except D.FlashVitError as e:
        return ([], 0, e.rc)


def refused(call):
    with pytest.raises(D.FlashVitError) as e:
        call()
    return e.value.rc


def even(T, n):
    return [n] * (T // n) + ([T % n] if T % n else [])


def members(fv):
    """members of the context (the runner marks a multi-device context; anything else is one device)"""
    return getattr(fv, "members", 1)


def strip(stats):
    return tuple(sorted((k, v) for k, v in stats.items() if k != "push_ms_total"))


# ---------------------------------------------------------------- models, observations, the oracle's statements

DENSE = {"d544": (544, 511), "d513": (513, 512), "d530": (530, 513), "d600": (600, 514), "d200": (200, 515), "d77": (77, 516)}


@functools.lru_cache(maxsize=None)
def model(name):
    """(A, B, Pi, set through fv_set_model_sparse?)"""
    if name in DENSE:
        K, seed = DENSE[name]
        return modelgen.model32(dict(kind="data_script", K=K, M=M, T=8, prob=0.2, seed=seed))[:3] + (False,)
    if name == "e520":                         # density 0.5: FV_KERNEL_AUTO is the packed 16-bit kernel, so plain defaults reach the flat route
        return modelgen.model32(dict(kind="data_script", K=520, M=M, T=8, prob=0.5, seed=518))[:3] + (False,)
    if name == "s1600":                        # 3 * 1024 <= 2 * K: the smallest size class at which FLASH-BS selects keep candidate lists
        return modelgen.model32(dict(kind="sparse_fast", K=1600, M=M, T=8, prob=0.05, seed=517))[:3] + (False,)
    if name == "c530":                         # the matrix of d530 through the CSR setter
        return model("d530")[:3] + (True,)
    if name == "g200":                         # the K = 200 golden (part 3)
        g = next(g for g in load_goldens() if g["name"] == "ds_K200_T100")
        return golden_model(g)[:3] + (False,)
    if name == "gc200":
        return model("g200")[:3] + (True,)
    if name == "wideA":                        # sixteen decades of weights, scaled by 4: entries above 1, so AUTO is the float64 kernel
        A, B, Pi, _ = modelgen.wide_model("wideA", 150, M, 8, 401)
        A = (A * np.float32(4)).astype(np.float32)
        assert (A > 1).sum() > 1000
        return A, B, Pi, False
    if name == "unreach":                      # states no path reaches, and a symbol (M - 1) no state emits: FV_ERR_NO_PRED
        A, B, Pi, _ = modelgen.unreachable_model(160, M, 8, 700, prob=0.2)
        B = B.copy()
        B[:, M - 1] = 0
        return A, B, Pi, False
    raise KeyError(name)


def size(name):
    return model(name)[0].shape[0]


@functools.lru_cache(maxsize=None)
def OB(name):
    """300 symbols every state set of the model can emit (unreach: without the dead symbol)"""
    if name in ("c530", "gc200"):
        return OB({"c530": "d530", "gc200": "g200"}[name])
    nsym = model(name)[1].shape[1] - (1 if name == "unreach" else 0)
    return np.random.RandomState(sum(map(ord, name))).randint(0, nsym, 300).astype(np.int32)


@functools.lru_cache(maxsize=None)
def om(name):
    A, B, Pi, _ = model(name)
    return oracle.OracleModel(A, B, Pi)


def put_model(fv, name):
    A, B, Pi, csr = model(name)
    if csr:
        fv.set_model_sparse(*D.dense_to_csr(A), B, Pi)
    else:
        fv.set_model(A, B, Pi)


def o_full(o, ob, N):
    p, s, _, rc = o.full_decode(ob, N, check=False)
    return tri((p, s, rc))


def o_beam(o, ob, N, B):
    p, s, _, rc = o.beam_decode(ob, N, B, check=False)
    return tri((p, s, rc))


def o_single(o, ob):
    """FV_MODE_SINGLE_PASS: one pass, the lowest index among the maxima of the last row, the serial walk"""
    row, args = o.full_forward(ob, 0, len(ob) - 1, -1)
    path = sm.single_pass_path(row, args)
    return (path, bits(row[path[-1]]), 0)


def o_vanilla(o, ob):
    return tri(o.vanilla_decode(ob, check=False))


def o_ckpt(o, ob, step):
    return tri(o.checkpoint_decode(ob, step, check=False))


def agrees(got, want):
    """a triple against the oracle's: below zero only the return code is a statement"""
    return got[2] == want[2] if want[2] < 0 else got == want


def defaults(fv):
    """every documented setting back to what a fresh context has; the workspace stays as the calls before left it"""
    for key, v in ((D.OPT_KERNEL, AUTO), (D.OPT_MAX_BATCH, 8), (D.OPT_FLAT_GENERATIONS, D.FLAT_AUTO), (D.OPT_ROW_CODES, 1),
                   (D.OPT_SPARSE_BEAM, 0), (D.OPT_DEBUG, 0)):
        fv.set_option(key, v)
    fv.set_max_lag(0)
    fv.test_flat_poison(-1)
    if fv.P:
        fv.set_emission_map(None)
    if fv.stats()["emission_rows"]:
        fv.clear_emissions()


def plain(fv, name, T=70, N=3):
    """an ordinary decode after something unusual: the oracle's path, and statistics that describe it alone"""
    ob = OB(name)[:T]
    got = tri(fv.decode_full(ob, N))
    assert got == o_full(om(name), ob, N), (name, "ordinary decode")
    return got, det(fv)


def kernel_reported(name, kernel):
    if name in ("c530", "gc200"):
        return D.KERNEL_SPARSE_CSR
    if name == "wideA":
        return F64
    if name == "e520":
        return U16 if kernel in (AUTO, SPQ) else kernel   # (density 0.5: AUTO takes the packed kernel)
    return SPQ if kernel == AUTO else kernel          # (density 0.2: AUTO takes the sparse walk)


# ---------------------------------------------------------------- part 1: the table of calls

class Call:
    def __init__(self, name, mdl, run, multi=False):
        self.name, self.model, self.run, self.multi = name, mdl, run, multi


def c_full(name, kernel):
    """decode_full: N in 1, 3, 8, both modes, one kernel"""
    T = 130
    ob = OB(name)[:T]
    want = {N: o_full(om(name), ob, N) for N in (1, 3, 8)}
    single = o_single(om(name), ob)
    rep = kernel_reported(name, kernel)

    def run(fv):
        fv.set_option(D.OPT_KERNEL, kernel)
        out = []
        for N in (1, 3, 8):
            for mode in (REF, SINGLE):
                got = tri(fv.decode_full(ob, N, mode))
                assert got == (want[N] if mode == REF else single), (name, kernel, N, mode)
                assert fv.stats()["kernel"] == rep, (name, kernel)
                out.append((got, det(fv)))
        return out
    return Call(f"full {name} kernel {kernel}", name, run, multi=True)


def c_options(name):
    """decode_full under FV_OPT_ROW_CODES 2, then FV_OPT_FLAT_GENERATIONS 0 and 2 (the packed kernel: the one the two serve)"""
    T, N = 130, 8
    ob = OB(name)[:T]
    want = o_full(om(name), ob, N)
    nright = len(D.plan_passes(T, N)) - 1

    def run(fv):
        fv.set_option(D.OPT_KERNEL, U16)
        out = []
        for key, v in ((D.OPT_ROW_CODES, 2), (D.OPT_FLAT_GENERATIONS, 0), (D.OPT_FLAT_GENERATIONS, 2)):
            fv.set_option(key, v)
            got = tri(fv.decode_full(ob, N))
            st = fv.stats()
            assert got == want and st["kernel"] == U16, (name, key, v)
            if key == D.OPT_FLAT_GENERATIONS:
                # (a multi-device context never takes the flat route: the option is accepted and changes nothing)
                assert st["flat_passes"] == (nright if v == 2 and members(fv) == 1 else 0), (name, v, st["flat_passes"])
            out.append((got, det(fv)))
        return out
    return Call(f"row codes and flat options {name}", name, run, multi=True)


def c_flat(name):
    """K >= 512, N = 8, T = 256 with FV_OPT_FLAT_GENERATIONS at its default: the flat route is taken (by the packed kernel —
    at this density FV_KERNEL_AUTO is the sparse walk, which auto leaves generation by generation: asserted too); the same
    decode with a poisoned snapshot entry, and again with the poison cleared.  Not run on the multi-device context: it never
    takes the flat route (c_options asserts that there), and fv_test_flat_poison acts on nothing else"""
    T, N = 256, 8
    ob = OB(name)[:T]
    want = o_full(om(name), ob, N)
    plan = D.plan_passes(T, N)
    t_poison = next(p[0] - 1 for p in plan if p[2] == 1 and p[0] > 0)       # a generation-1 pass starts from it

    def run(fv):
        out = []
        got = tri(fv.decode_full(ob, N))
        assert got == want and fv.stats()["kernel"] == SPQ and fv.stats()["flat_passes"] == 0, name
        out.append((got, det(fv)))
        fv.set_option(D.OPT_KERNEL, U16)
        for poison in (-1, t_poison, -1):
            fv.test_flat_poison(poison)
            got = tri(fv.decode_full(ob, N))
            st = fv.stats()
            assert got == want and st["kernel"] == U16, (name, poison)
            assert st["flat_passes"] > 0, (name, poison)
            assert st["flat_passes"] == len(plan) - 1
            assert (st["flat_first_miss"], st["flat_missed"] > 0) == ((1, True) if poison >= 0 else (-1, False)), (name, poison)
            out.append((got, det(fv)))
        return out
    return Call(f"flat route {name}", name, run)


RAGGED = (40, 2, 77, 33, 9)


def c_batches(name):
    """decode_full_batch and decode_beam_batch on ragged lengths"""
    N, beam = 4, 24
    seqs = [np.ascontiguousarray(np.roll(OB(name), 31 * s)[:n]) for s, n in enumerate(RAGGED)]
    want_full = [o_full(om(name), o, N) for o in seqs]
    want_beam = [o_beam(om(name), o, N, beam) for o in seqs]
    csr = model(name)[3]

    def run(fv):
        fv.set_option(D.OPT_SPARSE_BEAM, 1 if csr else 0)
        out = []
        for which, want in (("full", want_full), ("beam", want_beam)):
            if which == "full":
                paths, scores, statuses = fv.decode_full_batch(seqs, N)
            else:
                paths, scores, statuses = fv.decode_beam_batch(seqs, N, beam)
            got = [tri((paths[s], scores[s], statuses[s])) for s in range(len(seqs))]
            assert all(agrees(g, w) for g, w in zip(got, want)), (name, which)
            out.append((got, det(fv)))
        return out
    return Call(f"batches {name}", name, run)


def c_beam(name, beam, multi=True):
    T, N = 120, 3
    ob = OB(name)[:T]
    want = o_beam(om(name), ob, N, beam)
    csr = model(name)[3]

    def run(fv):
        fv.set_option(D.OPT_SPARSE_BEAM, 1 if csr else 0)
        got = tri(fv.decode_beam(ob, N, beam))
        assert got == want, (name, beam)
        return got, det(fv)
    return Call(f"beam {name} B {beam}", name, run, multi=multi)


def c_baselines(name):
    """decode_vanilla, decode_checkpoint with step 0 and step 7"""
    T = 110
    ob = OB(name)[:T]
    want = [o_vanilla(om(name), ob), o_ckpt(om(name), ob, 0), o_ckpt(om(name), ob, 7)]

    def run(fv):
        out = []
        for q, call in enumerate((lambda: fv.decode_vanilla(ob), lambda: fv.decode_checkpoint(ob, 0), lambda: fv.decode_checkpoint(ob, 7))):
            got = tri(call())
            assert got == want[q] and fv.stats()["kernel"] == F64, (name, q)
            out.append((got, det(fv)))
        return out
    return Call(f"vanilla and checkpoint {name}", name, run, multi=True)


@functools.lru_cache(maxsize=None)
def emissions(name, T, seed=7):
    """(E float32 probabilities [T, K] with five percent zeros, their float64 logs, the oracle of the M = T model)"""
    A, _, Pi, _ = model(name)
    K = A.shape[0]
    rs = np.random.RandomState(seed + K)
    E = rs.uniform(0.05, 1.0, (T, K)).astype(np.float32)
    E[rs.uniform(size=(T, K)) < 0.05] = 0
    return E, libm_log(E), oracle.OracleModel(A, np.ascontiguousarray(E.T), Pi)


def emission_decodes(fv, T, lengths, csr):
    """ob = None decodes of each family on the staged rows: [(triple(s), statistics)]"""
    out = []
    calls = [lambda: fv.decode_full(None, 3, T=T), lambda: fv.decode_full(None, 1, SINGLE, T=T)]
    if not csr:
        calls += [lambda: fv.decode_beam(None, 3, 24, T=T), lambda: fv.decode_vanilla(None, T=T), lambda: fv.decode_checkpoint(None, 0, T=T)]
    for call in calls:
        out.append((attempt(call), det(fv)))
    if members(fv) > 1:                        # sequences are not dealt to members: refused, and nothing of it stays
        assert refused(lambda: fv.decode_full_batch(None, 3, lengths=lengths)) == D.ERR_UNSUPPORTED
        out.append(([], ()))
    else:
        paths, scores, statuses = fv.decode_full_batch(None, 3, lengths=lengths)
        out.append(([tri((paths[s], scores[s], statuses[s])) for s in range(len(lengths))], det(fv)))
    return out


def c_emissions(name, dtype):
    """set_emissions in one of the four dtypes, then ob = None decodes of each family.  float64 rows of libm logs are the
    oracle's M = T model; the narrower types are no model's logs: each is defined by its widening, so the same decodes on the
    staged float64 widening of the block judge them (as tests/test_gpu_emissions_tied.py does), with no return code below 0"""
    T, lengths = 60, [25, 2, 33]
    E, logE, eo = emissions(name, T)
    csr = model(name)[3]
    t = np.arange(T, dtype=np.int32)
    want = None
    if dtype == "f64":
        want = [o_full(eo, t, 3), o_single(eo, t)]
        if not csr:
            want += [o_beam(eo, t, 3, 24), o_vanilla(eo, t), o_ckpt(eo, t, 0)]
        offs = np.concatenate([[0], np.cumsum(lengths)])
        per = []
        for s, n in enumerate(lengths):
            so = oracle.OracleModel(model(name)[0], np.ascontiguousarray(E[offs[s]:offs[s + 1]].T), model(name)[2])
            per.append(o_full(so, np.arange(n, dtype=np.int32), 3))
            so.close()
        want.append(per)
    block = {"f64": logE, "f32": logE.astype(np.float32), "f16": logE.astype(np.float16),
             "bf16": f32_to_bf16_bits(logE.astype(np.float32))}[dtype]
    block = np.ascontiguousarray(block)
    wide = None if dtype == "f64" else np.ascontiguousarray((bf16_to_f32(block) if dtype == "bf16" else block).astype(np.float64))

    def run(fv):
        if dtype == "bf16":
            fv.set_emissions((block.ctypes.data, D.EMIS_LOG_BF16, T, block.shape[1]))
        else:
            fv.set_emissions(block)
        assert fv.stats()["emission_rows"] == T
        out = emission_decodes(fv, T, lengths, csr)
        if want is not None:
            for q, w in enumerate(want[:-1]):
                assert agrees(out[q][0], w), (name, dtype, q)
            assert all(agrees(g, w) for g, w in zip(out[-1][0], want[-1])), (name, dtype, "batch")
        if wide is not None:
            fv.set_emissions(wide)
            widened = emission_decodes(fv, T, lengths, csr)
            assert [o[0] for o in out] == [o[0] for o in widened], (name, dtype, "differs from its float64 widening")
            assert all(o[0][2] >= 0 for o in out[:-1]) and all(g[2] >= 0 for g in out[-1][0]), (name, dtype)
            out += widened
        return out
    return Call(f"emissions {name} {dtype}", name, run, multi=True)


def c_map(name):
    """set_emission_map with P < K, set_emissions through the map, then clear_emissions, then a symbol decode"""
    T, P = 50, 37
    A, _, Pi, _ = model(name)
    K = A.shape[0]
    rs = np.random.RandomState(3 + K)
    pdf = rs.randint(0, P, K).astype(np.int32)
    Ep = rs.uniform(0.05, 1.0, (T, P)).astype(np.float32)
    logs = libm_log(Ep)
    eo = oracle.OracleModel(A, np.ascontiguousarray(Ep[:, pdf].T), Pi)
    t = np.arange(T, dtype=np.int32)
    want = [o_full(eo, t, 3), o_beam(eo, t, 3, 24)]
    eo.close()

    def run(fv):
        fv.set_emission_map(pdf, P)
        fv.set_emissions(logs)
        out = [(attempt(lambda: fv.decode_full(None, 3, T=T)), det(fv)), (attempt(lambda: fv.decode_beam(None, 3, 24, T=T)), det(fv))]
        assert agrees(out[0][0], want[0]) and agrees(out[1][0], want[1]), name
        fv.clear_emissions()
        assert fv.stats()["emission_rows"] == 0 and refused(lambda: fv.decode_full(None, 3, T=T)) == D.ERR_ARG
        out.append(plain(fv, name))
        return out
    return Call(f"emission map {name}", name, run, multi=True)


def c_symbols_over_staged_rows(name, with_map):
    """emission rows (through a map or not) stay staged while symbol decodes of every family run: the emission view is chosen
    call by call, and a symbol decode is what it is without them"""
    T, P = 45, 29
    A, _, Pi, csr = model(name)
    K = A.shape[0]
    rs = np.random.RandomState(11 + K)
    pdf = rs.randint(0, P, K).astype(np.int32)
    W = P if with_map else K
    Ep = rs.uniform(0.05, 1.0, (T, W)).astype(np.float32)
    logs = libm_log(Ep)
    eo = oracle.OracleModel(A, np.ascontiguousarray((Ep[:, pdf] if with_map else Ep).T), Pi)
    want_rows = o_full(eo, np.arange(T, dtype=np.int32), 3)
    eo.close()
    ob = OB(name)[:80]
    o = om(name)
    want = [o_full(o, ob, 3), o_single(o, ob), o_beam(o, ob, 3, 24), o_vanilla(o, ob), o_ckpt(o, ob, 0)]

    def run(fv):
        if with_map:
            fv.set_emission_map(pdf, P)
        fv.set_emissions(logs)
        out = []
        for turn in range(2):                  # rows, symbols, rows again, symbols again
            got = attempt(lambda: fv.decode_full(None, 3, T=T))
            assert agrees(got, want_rows), (name, with_map, turn)
            out.append((got, det(fv)))
            calls = (lambda: fv.decode_full(ob, 3), lambda: fv.decode_full(ob, 1, SINGLE), lambda: fv.decode_beam(ob, 3, 24),
                     lambda: fv.decode_vanilla(ob), lambda: fv.decode_checkpoint(ob, 0))
            for q, call in enumerate(calls):
                got = tri(call())
                assert got == want[q] and fv.stats()["emission_rows"] == T, (name, with_map, turn, q)
                out.append((got, det(fv)))
        return out
    return Call(f"symbols over staged rows {name} map {with_map}", name, run, multi=True)


def c_flat_auto(name):
    """a denser model, every option at its default: FV_KERNEL_AUTO is the packed kernel and the decode takes the flat route"""
    T, N = 256, 8
    ob = OB(name)[:T]
    want = o_full(om(name), ob, N)
    nright = len(D.plan_passes(T, N)) - 1

    def run(fv):
        got = tri(fv.decode_full(ob, N))
        st = fv.stats()
        assert got == want and st["kernel"] == U16, name
        assert st["flat_passes"] > 0 and st["flat_passes"] == nright and st["flat_first_miss"] == -1, (name, st["flat_passes"])
        return got, det(fv)
    return Call(f"flat route under plain defaults {name}", name, run)


def c_forward(name):
    """fv_test_forward: right-hand passes under FV_OPT_ROW_CODES 2 against full_forward, then an ordinary decode in which
    neither the hook's debug bit 3 nor the rows and answers it overwrote show"""
    K = size(name)
    ob = OB(name)
    sets = [pass_set(lengths, K, 60 + K)[0] for lengths in ((8, 4, 2), (13, 9, 8, 6, 5, 4, 2, 1))]
    want = [[om(name).full_forward(ob, L, R, s) for L, R, s in passes] for passes in sets]

    def run(fv):
        fv.set_option(D.OPT_KERNEL, U16)
        fv.set_option(D.OPT_ROW_CODES, 2)
        out = []
        for passes, tabs in zip(sets, want):
            rows, bp, var = fv.test_forward(ob, passes, -2)
            assert var & D.TV_ROW_CODES, (name, hex(var))
            for q, (L, R, s) in enumerate(passes):
                assert np.array_equal(rows[q].view(np.uint32), tabs[q][0].view(np.uint32)), (name, L, R)
                assert np.array_equal(bp[L + 1:R + 1], tabs[q][1]), (name, L, R)
            out.append((rows.tobytes(), bp.tobytes(), var, det(fv)))
        fv.set_option(D.OPT_ROW_CODES, 1)
        fv.set_option(D.OPT_KERNEL, AUTO)
        out.append(plain(fv, name, T=90, N=8))            # (under bit 3 a decode's column_steps would be 0)
        assert dict(out[-1][1])["column_steps"] > 0
        return out
    return Call(f"test_forward {name}", name, run)


class BeamView:
    """what tests/test_gpu_beam_tables.py's check_pass reads of a model"""

    def __init__(self, name, beam, T):
        A, B, _, _ = model(name)
        self.name, self.A, self.K, self.beam, self.T = name, A, A.shape[0], beam, T
        self.ob = OB(name)[:T]
        self.spec = dict(kind=name)
        self.tmp = libm_log(B).astype(np.float32)
        self._tables = {}

    def tables(self, L, R, init):
        if (L, R, init) not in self._tables:
            self._tables[(L, R, init)] = om(self.name).beam_forward(self.ob, L, R, init, self.beam)
        return self._tables[(L, R, init)]


def c_beam_forward(name):
    """fv_test_beam_forward in whole and right-hand form against beam_forward, cell by cell; then an ordinary beam decode and
    an ordinary full decode on the buffers and counters the hook overwrote"""
    T, beam, N = 60, 40, 4
    m = BeamView(name, beam, T)
    opath = om(name).beam_decode(m.ob, N, beam, check=False)[0]
    assert opath.min() >= 0
    whole = [(0, T - 1, -1, -1)]
    right = [(L, R, -1 if L == 0 else int(opath[L - 1]), int(opath[R])) for L, R, g, _ in D.plan_passes(T, N) if g == 1]
    want_beam = o_beam(om(name), m.ob, N, beam)
    csr = model(name)[3]

    def run(fv):
        fv.set_option(D.OPT_SPARSE_BEAM, 1 if csr else 0)
        out = []
        for passes in (whole, right):
            o = fv.test_beam_forward(m.ob, beam, passes)
            for p in passes:
                check_pass(m, o, p, 0, passes is whole)
            out.append((o["path"].tolist(), bits(o["score"]) if passes is whole else 0, o["rc"], o["gate"], o["variants"], o["selects"], det(fv)))
        got = tri(fv.decode_beam(m.ob, N, beam))
        assert got == want_beam, name
        out.append((got, det(fv)))
        if not csr:
            out.append(plain(fv, name))
        return out
    return Call(f"test_beam_forward {name}", name, run)


@functools.lru_cache(maxsize=None)
def lag_want(name, key, T, max_lag, chunks):
    """tests/lag_model.py on a sequence cut from the model's observations (max_lag 0: tests/stream_model.py's rule)"""
    A, B, Pi, _ = model(name)
    r = lm.run(A, B, Pi, sequence(name, key, T), CHECK, max_lag, list(chunks))
    assert r["dead"] is None
    return dict(pieces=r["pieces"], committed=r["committed"], score=bits(r["score"]), checks=r["checks"], commits=r["commits"],
                lag_max=r["lag_max"], bt_restarts=r["bt_restarts"], lag=r["lag"])


def sequence(name, key, T):
    return np.ascontiguousarray(np.roll(OB(name), 37 * key)[:T])


def stream_result(got, lag):
    return (got["pieces"], got["committed"], bits(got["score"]), got["rc"], strip(got["stats"]), tuple(sorted(lag.items())))


def check_stream(got, lag, want, tag):
    assert got["dead"] is None, tag
    assert (got["pieces"], got["committed"], bits(got["score"]), got["rc"]) == (want["pieces"], want["committed"], want["score"], 0), tag
    st = got["stats"]
    assert (st["checks"], st["commits"], st["lag_max"], st["bt_restarts"]) == (want["checks"], want["commits"], want["lag_max"], want["bt_restarts"]), tag
    assert lag == want["lag"], tag


def c_stream(name, max_lag):
    """a single stream in pushes of 16, by symbols and by score rows; a decode right after its close and right before the
    next open; under a lag bound, then with the bound back at 0: the unbounded stream bit for bit"""
    T = 100
    ob = sequence(name, 0, T)
    chunks = tuple(even(T, PUSH))
    want = lag_want(name, 0, T, max_lag, chunks)
    free = lag_want(name, 0, T, 0, chunks)
    rows = np.ascontiguousarray(libm_log(model(name)[1])[:, ob].T)          # logE[t][i] = log B[i][ob[t]]: the same stream
    rep = kernel_reported(name, AUTO)

    def run(fv):
        out = []
        fv.set_max_lag(max_lag)
        for how in (dict(ob=ob), dict(feed=lambda pos, n: rows[pos:pos + n])):
            got = run_stream(fv, list(chunks), CHECK, **how)
            lag = fv.lag_stats()
            check_stream(got, lag, want, (name, max_lag, sorted(how)))
            assert got["stats"]["kernel"] == rep
            out.append(stream_result(got, lag))
            out.append(plain(fv, name))                   # close, then at once a decode; then at once the next stream
        if max_lag:
            fv.set_max_lag(0)
            got = run_stream(fv, list(chunks), CHECK, ob=ob)
            lag = fv.lag_stats()
            check_stream(got, lag, free, (name, "bound cleared"))
            assert lag == dict(max_lag=0, forced_commits=0, pruned_states=0, first_forced_time=-1, last_forced_time=-1)
            out.append(stream_result(got, lag))
        return out
    return Call(f"stream {name} lag {max_lag}", name, run)


def c_set(name, max_lag):
    """a set of three slots; slot 1 is closed in mid-run and starts another sequence while the others go on"""
    T1 = 40
    seqs = {"s0": sequence(name, 0, 100), "s1a": sequence(name, 1, T1), "s1b": sequence(name, 3, 60), "s2": sequence(name, 2, 87)}
    pushes = {"s0": (T1, 60), "s1a": (T1,), "s1b": (30, 30), "s2": (T1, 47)}
    keys = {"s0": 0, "s1a": 1, "s1b": 3, "s2": 2}
    want = {k: lag_want(name, keys[k], len(seqs[k]), max_lag, pushes[k]) for k in seqs}

    def run(fv):
        fv.set_max_lag(max_lag)
        fv.streams_open(3, 0, CHECK)
        got = {k: dict(pieces=[]) for k in seqs}
        try:
            def push(ids, parts):
                pieces, status = fv.streams_push(ids, obs=[seqs[k][a:b] for k, a, b in parts])
                assert status == [0] * len(ids)
                for (k, _, _), p in zip(parts, pieces):
                    got[k]["pieces"].append(p.tolist())

            def close(slot, k):
                piece, score, rc = fv.streams_close(slot)
                got[k]["pieces"].append(piece.tolist())
                got[k].update(score=bits(score), rc=rc, stats=fv.streams_slot_stats(slot), lag=fv.lag_stats(slot))

            push([0, 1, 2], [("s0", 0, T1), ("s1a", 0, T1), ("s2", 0, T1)])
            close(1, "s1a")
            push([0, 1, 2], [("s0", T1, 100), ("s1b", 0, 30), ("s2", T1, 87)])
            push([1], [("s1b", 30, 60)])
            for slot, k in ((2, "s2"), (0, "s0"), (1, "s1b")):
                close(slot, k)
            set_stats = fv.streams_stats()
        finally:
            fv.streams_end()
        for k, g in got.items():
            w, st = want[k], g["stats"]
            assert (g["pieces"], g["score"], g["rc"]) == (w["pieces"], w["score"], 0), (name, max_lag, k)
            assert (st["checks"], st["commits"], st["lag_max"], st["bt_restarts"]) == (w["checks"], w["commits"], w["lag_max"], w["bt_restarts"]), (name, k)
            assert (st["times"], st["committed"], st["pushes"]) == (len(seqs[k]), len(seqs[k]), len(pushes[k])), (name, k)
            assert g["lag"] == w["lag"], (name, max_lag, k)
        out = [(k, g["pieces"], g["score"], g["rc"], strip(g["stats"]), tuple(sorted(g["lag"].items()))) for k, g in sorted(got.items())]
        out.append(strip(set_stats))
        out.append(plain(fv, name))
        return out
    return Call(f"set {name} lag {max_lag}", name, run)


def c_refusals(name):
    """refused calls, each with its documented code, each followed by an ordinary decode"""
    ob = OB(name)[:64]
    csr = model(name)[3]

    def run(fv):
        out = []
        bad = ob.copy()
        bad[17] = model(name)[1].shape[1]
        assert refused(lambda: fv.decode_full(bad, 3)) == D.ERR_ARG                 # a symbol >= M
        out.append(plain(fv, name))
        assert refused(lambda: fv.decode_full(ob[:16], 8)) == D.ERR_ARG             # T == 2 * n_split, n_split > 2
        out.append(plain(fv, name))
        if name == "wideA":
            for kernel in (U16, Q16, SPQ):                                          # a filter kernel on entries above 1
                fv.set_option(D.OPT_KERNEL, kernel)
                assert refused(lambda: fv.decode_full(ob, 3)) == D.ERR_UNSUPPORTED
            fv.set_option(D.OPT_KERNEL, AUTO)
            out.append(plain(fv, name))
        if csr:
            assert refused(lambda: fv.decode_beam(ob, 3, 16)) == D.ERR_UNSUPPORTED   # FV_OPT_SPARSE_BEAM is 0
            assert refused(lambda: fv.decode_beam_batch([ob, ob[:9]], 3, 16)) == D.ERR_UNSUPPORTED
            out.append(plain(fv, name))
        return out
    return Call(f"refusals {name}", name, run, multi=True)


def c_no_pred():
    """the dead symbol at time 20: FV_ERR_NO_PRED from every full-state entry point, each followed by an ordinary decode"""
    name = "unreach"
    ob = OB(name)[:64].copy()
    ob[20] = M - 1
    assert o_full(om(name), ob, 3)[2] == D.ERR_NO_PRED and o_full(om(name), ob, 1)[2] == D.ERR_NO_PRED
    assert o_vanilla(om(name), ob)[2] == D.ERR_NO_PRED

    def run(fv):
        out = []
        for call in (lambda: fv.decode_full(ob, 3), lambda: fv.decode_full(ob, 1, SINGLE), lambda: fv.decode_vanilla(ob)):
            got = attempt(call)
            assert got[2] == D.ERR_NO_PRED
            out.append((got[2], det(fv)))
            out.append(plain(fv, name))
        return out
    return Call("no predecessor", name, run, multi=True)


def c_beam_miss():
    """a beam too narrow for the model with unreachable states: FV_WARN_BEAM_MISS and -1 entries, then an ordinary decode"""
    name = "unreach"
    ob = OB(name)[:64]
    N, beam = next((N, B) for N in (3, 4, 1) for B in (2, 3, 4, 6, 8) if o_beam(om(name), ob, N, B)[2] == D.WARN_BEAM_MISS)
    want = o_beam(om(name), ob, N, beam)
    assert min(want[0]) == -1

    def run(fv):
        got = tri(fv.decode_beam(ob, N, beam))
        assert got == want
        return [(got, det(fv)), plain(fv, name)]
    return Call("beam miss", name, run, multi=True)


@functools.lru_cache(maxsize=None)
def table():
    calls = []
    for name in DENSE:
        calls += [c_full(name, k) for k in (AUTO, U16, Q16, F64, SPQ)]
        calls += [c_options(name), c_batches(name), c_baselines(name), c_refusals(name)]
        calls += [c_beam(name, b) for b in (11, 40, 64)]
    calls += [c_flat(name) for name in ("d544", "d513", "d530", "d600")]
    calls += [c_full("c530", k) for k in (AUTO, SPQ)] + [c_batches("c530"), c_refusals("c530")] + [c_beam("c530", b) for b in (11, 40, 64)]
    calls += [c_full("wideA", k) for k in (AUTO, F64)] + [c_refusals("wideA"), c_beam("wideA", 40), c_baselines("wideA")]
    calls += [c_full("unreach", AUTO), c_no_pred(), c_beam_miss()]
    # K = 1600: the selects of a beam decode read the cut records an earlier pass left at the same times to predict their
    # candidate lists (the records are reset per decode), and the list counters tell when they read another decode's
    calls += [c_beam("s1600", b) for b in (40, 64, 100)]
    calls += [c_emissions(name, dt) for name in ("d513", "d200") for dt in ("f64", "f32", "f16", "bf16")] + [c_emissions("c530", "f64")]
    calls += [c_map("d530"), c_map("d200")]
    calls += [c_symbols_over_staged_rows("d513", True), c_symbols_over_staged_rows("d200", False)]
    calls += [c_flat_auto("e520"), c_full("e520", AUTO)]
    calls += [c_forward(name) for name in ("d513", "d530", "d600", "d77")]
    calls += [c_beam_forward(name) for name in ("d200", "d530", "c530")]
    for name in ("d530", "c530", "d77"):
        calls += [c_stream(name, 0), c_stream(name, 16), c_set(name, 0), c_set(name, 16)]
    return calls


def differing(got, want, where=""):
    """the first place two nested results differ at"""
    if type(got) is not type(want):
        return f"{where}: {type(got).__name__} / {type(want).__name__}"
    if isinstance(got, (list, tuple)):
        if len(got) != len(want):
            return f"{where}: lengths {len(got)} / {len(want)}"
        for i, (g, w) in enumerate(zip(got, want)):
            if g != w:
                return differing(g, w, f"{where}[{i}]")
        return None
    return None if got == want else f"{where}: {str(got)[:200]} / {str(want)[:200]}"


def assert_both_directions(names):
    """the order has model changes larger K -> smaller, smaller -> larger, dense -> CSR and CSR -> dense"""
    seen = set()
    for a, b in zip(names, names[1:]):
        if a == b:
            continue
        seen.add("down" if size(b) < size(a) else "up" if size(b) > size(a) else "same")
        seen.add(("csr" if model(a)[3] else "dense") + ">" + ("csr" if model(b)[3] else "dense"))
    assert {"down", "up", "dense>csr", "csr>dense"} <= seen, seen


@pytest.mark.parametrize("devices", [0, [0, 0]], ids=["one_device", "two_members"])
@pytest.mark.parametrize("seed", [101, 202, 303])
def test_every_entry_point_in_shuffled_order_across_model_changes(seed, devices):
    multi = isinstance(devices, list)
    calls = [c for c in table() if c.multi or not multi]
    order = np.random.RandomState(seed).permutation(len(calls))
    assert_both_directions([calls[i].model for i in order])
    fv = D.FlashViterbi(devices)
    fv.members = len(devices) if multi else 1
    current, before = None, "nothing"
    try:
        for i in order:
            c = calls[i]
            if c.model != current:
                put_model(fv, c.model)
                current = c.model
            defaults(fv)
            got = c.run(fv)
            fresh = D.FlashViterbi(devices)
            fresh.members = fv.members
            try:
                put_model(fresh, c.model)
                want = c.run(fresh)
            finally:
                fresh.close()
            assert got == want, f"seed {seed}: '{c.name}' after '{before}' differs from a fresh context (reused / fresh) at {differing(got, want)}"
            before = c.name
    finally:
        fv.close()


# ---------------------------------------------------------------- part 2: stale pads, directed

# (model that fills the workspace, model that then decodes in it, rows of the first decode).  513 -> 544: the arg rows of
# 300 x 513 cells hold the 256 x 544 of the second decode, and the flat plan of T = 300 is no smaller than that of T = 256.
PAIRS = {"544_513": ("d544", "d513", 256), "513_544": ("d513", "d544", 300), "600_530": ("d600", "d530", 256),
         "530_csr": ("d530", "c530", 256)}
T2, N2 = 256, 8


@functools.lru_cache(maxsize=None)
def near_zero_emissions(name, T):
    """log of values in [0.9, 1): every score row the decode leaves is finite in every column"""
    A, _, Pi, _ = model(name)
    K = A.shape[0]
    E = np.random.RandomState(90 + K).uniform(0.9, 1.0, (T, K)).astype(np.float32)
    eo = oracle.OracleModel(A, np.ascontiguousarray(E.T), Pi)
    t = np.arange(T, dtype=np.int32)
    want = (o_full(eo, t, N2), o_ckpt(eo, t, 0))
    eo.close()
    return libm_log(E), want


@functools.lru_cache(maxsize=None)
def second_model_wants(name):
    ob = OB(name)[:T2]
    o = om(name)
    row, _ = o.full_forward(ob, 0, 60, -1)
    assert row.max() < -300                                # far below anything the first decode left
    passes = pass_set((9, 5, 3, 1), size(name), 20 + size(name))[0]
    return ob, o_full(o, ob, N2), o_ckpt(o, ob, 0), passes, [o.full_forward(ob, L, R, s) for L, R, s in passes]


@pytest.mark.parametrize("kernel,codes", [(U16, 0), (U16, 2), (Q16, 0), (Q16, 2), (F64, 0)], ids=["u16", "u16_codes", "q16", "q16_codes", "f64"])
@pytest.mark.parametrize("pair", list(PAIRS))
def test_stale_pads_after_a_model_change(pair, kernel, codes):
    first, second, T1 = PAIRS[pair]
    logE, want1 = near_zero_emissions(first, T1)
    ob, want_full, want_ckpt, passes, tabs = second_model_wants(second)
    csr = model(second)[3]
    fv = D.FlashViterbi(0)
    try:
        for batch in (1, 8):
            where = (pair, kernel, codes, batch)
            # 1. no pads (or other pads): every real column of every row slot, code tile and checkpoint row is written
            put_model(fv, first)
            fv.set_option(D.OPT_DEBUG, 0)
            fv.set_option(D.OPT_KERNEL, kernel)
            fv.set_option(D.OPT_ROW_CODES, codes)
            fv.set_option(D.OPT_MAX_BATCH, batch)
            fv.set_emissions(logE)
            assert tri(fv.decode_full(None, N2, T=T1)) == want1[0], where
            assert fv.stats()["kernel"] == kernel
            assert tri(fv.decode_checkpoint(None, 0, T=T1)) == want1[1], where
            # 2. the second model: same memory, other K
            put_model(fv, second)
            held = fv.stats()["device_bytes"]
            forms = (0, CSR_MEM) if csr else (0,)
            for debug in forms:
                if csr:
                    fv.set_option(D.OPT_KERNEL, AUTO)
                    fv.set_option(D.OPT_DEBUG, debug)
                # 3. scores far below what the pads hold
                got = tri(fv.decode_full(ob, N2))
                st = fv.stats()
                # 4. nothing grew, so no buffer was cleared: the pads are what step 1 left
                assert st["device_bytes"] == held, (where, debug, st["device_bytes"], held)
                assert st["kernel"] == (D.KERNEL_SPARSE_CSR if csr else kernel)
                # 5.
                assert got == want_full, (where, debug)
                if not csr:
                    assert tri(fv.decode_checkpoint(ob, 0)) == want_ckpt, where
                    assert fv.stats()["device_bytes"] == held, (where, "the checkpoint decode grew a buffer")
                rows, bp, var = fv.test_forward(ob, passes, -2)
                # (the hook's statistics carry no device_bytes; a four-step decode, which needs less of every buffer than
                # the decode above and so grows none, reads the sum after the hook)
                fv.decode_full(ob[:4], 1)
                assert fv.stats()["device_bytes"] == held, (where, debug, "the hook grew a buffer")
                for q, (L, R, s) in enumerate(passes):
                    bad = np.nonzero(rows[q].view(np.uint32) != tabs[q][0].view(np.uint32))[0]
                    assert bad.size == 0, (where, debug, (L, R), bad[:8].tolist())
                    assert np.array_equal(bp[L + 1:R + 1], tabs[q][1]), (where, debug, (L, R))
                if csr:
                    assert bool(var & TV_CSR_MEM) == bool(debug) and bool(var & TV_CSR_LDS) == (not debug), hex(var)
                else:
                    assert bool(var & D.TV_ROW_CODES) == (kernel == U16 and codes == 2), hex(var)
            fv.set_option(D.OPT_DEBUG, 0)
    finally:
        fv.close()


# ---------------------------------------------------------------- part 3: streams and sets through the launch forms

FORMS = (0, ALT, W16, PACKED, SLABS, SLABS | ALT)
T3 = 100


@functools.lru_cache(maxsize=None)
def slot_want(name, s):
    """the oracle's single pass over slot s's sequence and the commit rule's run over it in pushes of 16"""
    ob = slot_ob(OB(name)[:T3], s)
    row, args = om(name).full_forward(ob, 0, len(ob) - 1, -1)
    path = sm.single_pass_path(row, args)
    return ob, (path, bits(row[path[-1]]), 0), sm.run(args, row, CHECK, even(len(ob), PUSH))


def check_against_rule(got, name, s, tag):
    _, ref, want = slot_want(name, s)
    assert got["committed"] == want["committed"] and got["pieces"] == want["pieces"], tag
    assert ([x for p in got["pieces"] for x in p], bits(got["score"]), got["rc"]) == ref, tag
    st = got["stats"]
    assert (st["checks"], st["commits"], st["lag_max"], st["bt_restarts"]) == (want["checks"], want["commits"], want["lag_max"], want["bt_restarts"]), tag


def stream_and_set(fv, name, kernel, tag):
    """the single stream, then a set of three slots, every slot against the rule; what a fresh context must repeat"""
    ob = slot_want(name, 0)[0]
    got = run_stream(fv, even(len(ob), PUSH), CHECK, ob=ob)
    check_against_rule(got, name, 0, (tag, "stream"))
    assert got["stats"]["kernel"] == kernel_reported(name, kernel), tag
    one = (got["pieces"], got["committed"], bits(got["score"]), got["rc"], strip(got["stats"]))
    obs = [slot_want(name, s)[0] for s in range(3)]
    res = run_set(fv, 3, schedule([even(len(o), PUSH) for o in obs]), CHECK, obs=obs)
    for s in range(3):
        check_against_rule(res[s], name, s, (tag, "slot", s))
    assert res["set"]["kernel"] == kernel_reported(name, kernel), tag
    three = [(res[s]["pieces"], res[s]["committed"], bits(res[s]["score"]), res[s]["rc"], strip(res[s]["stats"])) for s in range(3)]
    return one, three, strip(res["set"])


def prove_forms(fv, name, kernel, debug):
    """fv_test_forward under the same options tells which step kernels a stream's single-task launches (one pass) and a
    set's batched launches (three passes in lock-step) are: the slab route is asserted where bit 21 is set"""
    K, ob = size(name), OB(name)[:T3]
    o = om(name)
    csr = model(name)[3]
    for passes in ([(0, 12, -1)], [(0, 12, -1), (14, 26, 5 % K), (28, 40, 70 % K)]):
        rows, bp, var = fv.test_forward(ob, passes, -2)
        for q, (L, R, s) in enumerate(passes):
            row, args = o.full_forward(ob, L, R, s)
            assert np.array_equal(rows[q].view(np.uint32), row.view(np.uint32)) and np.array_equal(bp[L + 1:R + 1], args), (name, kernel, debug, L)
        if csr:
            assert bool(var & TV_CSR_MEM) == bool(debug & CSR_MEM), hex(var)
            continue
        # the tables' kernels sweep slabs; the packed kernel and the sparse walk have no slab form — but FV_KERNEL_U16_REFINE
        # runs its batched launches on the f32 filter of the 16-bit table unless bit 14 keeps them packed
        slab = TV_SLAB.get(kernel, 0)
        if kernel == U16 and len(passes) > 1 and not debug & PACKED:
            slab = TV_SLAB[Q16]
        assert (var & TV_SLAB_ANY) == (slab if debug & SLABS else 0), (name, kernel, debug, len(passes), hex(var))


def take_the_code_route(fv, name):
    """a packed-kernel decode under FV_OPT_ROW_CODES 2 (proven by the hook's variants): code rows written, row_coded set"""
    ob = OB(name)[:T3]
    fv.set_option(D.OPT_KERNEL, U16)
    fv.set_option(D.OPT_ROW_CODES, 2)
    _, _, var = fv.test_forward(ob, [(0, 12, -1), (14, 22, 3), (24, 28, 9)], -2)          # (the longest ends alone: packed launches on coded rows)
    assert var & D.TV_ROW_CODES
    assert tri(fv.decode_full(ob, 8)) == o_full(om(name), ob, 8)


def forms_case(name, kernel, forms):
    fv = D.FlashViterbi(0)
    try:
        put_model(fv, name)
        for codes in (1, 2):
            for debug in forms:
                tag = (name, kernel, debug, codes)
                fv.set_option(D.OPT_DEBUG, 0)
                if codes == 2 and not model(name)[3]:
                    take_the_code_route(fv, name)
                fv.set_option(D.OPT_KERNEL, kernel)
                fv.set_option(D.OPT_ROW_CODES, codes)
                fv.set_option(D.OPT_DEBUG, debug)
                prove_forms(fv, name, kernel, debug)
                got = stream_and_set(fv, name, kernel, tag)
                fresh = D.FlashViterbi(0)
                try:
                    put_model(fresh, name)
                    fresh.set_option(D.OPT_KERNEL, kernel)
                    fresh.set_option(D.OPT_ROW_CODES, codes)
                    fresh.set_option(D.OPT_DEBUG, debug)
                    want = stream_and_set(fresh, name, kernel, (tag, "fresh"))
                finally:
                    fresh.close()
                assert got == want, f"{tag}: reused / fresh context differ at {differing(got, want)}"
    finally:
        fv.close()


@pytest.mark.parametrize("kernel", [AUTO, F64, F32, F16, Q16, SPQ, U16], ids=["auto", "f64", "f32", "f16", "q16", "sparse", "u16"])
@pytest.mark.parametrize("name", ["g200", "d530"])
def test_streams_and_sets_through_the_launch_forms(name, kernel):
    forms_case(name, kernel, FORMS)


@pytest.mark.parametrize("name", ["gc200", "c530"])
def test_streams_and_sets_on_the_csr_set_model_in_both_row_forms(name):
    forms_case(name, AUTO, (0, CSR_MEM))
