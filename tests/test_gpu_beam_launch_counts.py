"""GPU: the launch geometry of the FLASH-BS driver, pinned decode by decode.

The companion of test_gpu_launch_counts.py for fv_decode_beam, fv_decode_beam_batch and fv_test_beam_forward.  How the
driver queues a decode — the stream groups a generation is dealt to, the chunks of 24 passes a lock-step is launched
in, the step kernel a launch size selects — can change without moving one decoded bit.  So each decode below is made
once and compared with a table:

    (rc, step_launches, task_steps, passes, generations, crc32 of the path, bits of the score)
    + the device counters of COUNTERS, + (variants, selects) for fv_test_beam_forward

The table was recorded from the commit before the driver took its launch arguments from one builder each and its
stream groups from one policy function.  It was recorded there twice, in two processes; a field the two runs disagreed
on holds None and is not compared (beam_dup_cols / beam_dup_steps vary between identical runs and are never pinned).
The table asserts equality: it pins what that commit did, never what the code under test does."""
import functools
import math
import zlib

import numpy as np
import pytest

import modelgen
from flash_viterbi_amd import decoder

pytestmark = pytest.mark.gpu

D = decoder
FIELDS = ("rc", "step_launches", "task_steps", "passes", "generations", "path_crc", "score_bits")
COUNTERS = ("beam_spec_steps", "beam_reach_events", "beam_exact_sets", "beam_cand_selects", "beam_list_short", "beam_list_long",
            "beam_ties", "beam_chain_cuts", "bt_restarts")
ALL_FIELDS = FIELDS + COUNTERS
ONE_STREAM, GROUPS, ALL_LAYOUTS, EAGER, F64, Q16, W16, W8, GEN0 = 1 << 16, 1 << 17, 1 << 19, 1 << 20, 1 << 8, 1 << 9, 1 << 25, 1 << 26, 1 << 29
DEBUGS = (0, ONE_STREAM, GROUPS, ALL_LAYOUTS, EAGER, F64, Q16, W16, W8, ALL_LAYOUTS | GROUPS)
TV_W4, TV_W16, TV_Q16_W8, TV_Q16_W16 = 1 << 46, 1 << 47, 1 << 48, 1 << 49
TS = D.TS_BITS
TS_LISTED = TS["topb_select<4,listed>"] | TS["topb_select<16,listed>"] | TS["topb_select<64,listed>"] | \
    TS["topb_select_cand<8,listed>"] | TS["topb_select_cand<16,listed>"]
TS_DERIVED = TS_LISTED << 1
K0, BEAM0 = 600, 50
BEAM_CHUNK, PASS_CHUNK, HEAP_CHUNK = 24, 64, 440
# (T, n_split) -> passes per generation (fv::build_plan), asserted before the decodes
SHAPES = {
    "T130 n8": (130, 8, (1, 10, 24, 22, 7)),            # 24 passes: exactly one chunk, the listed select
    "T330 n4": (330, 4, (1, 8, 25, 40, 35, 16, 3)),     # 25 passes: one more than a chunk, two launches, the derived select
    "T330 n16": (330, 16, (1, 18, 48, 46, 15)),            # 48 passes: two full chunks
    "T530 n16": (530, 16, (1, 19, 66, 94, 61, 15)),        # 66 and 94 passes: two init-row launches; 94 deal out as 24, 24, 23, 23
}


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes())


def bits(x):
    return int(np.asarray(x, dtype=np.float32).reshape(1).view(np.uint32)[0])


def record(fv, rc, path, score_bits, extra=()):
    s = fv.stats()
    return (int(rc),) + tuple(int(s[f]) for f in FIELDS[1:5]) + (crc(path), int(score_bits)) + tuple(int(s[f]) for f in COUNTERS) + tuple(extra)


def libm_log(x):
    """float64 log of every float32 entry of x through math.log (the libm the library calls); log 0 = -inf"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    vals, inv = np.unique(x.reshape(-1), return_inverse=True)
    table = np.array([math.log(float(v)) if v > 0 else -math.inf for v in vals], dtype=np.float64)
    return table[inv.reshape(-1)].reshape(x.shape)


@functools.lru_cache(maxsize=None)
def data_model():
    return modelgen.model32(dict(kind="data_script", K=K0, M=8, T=530, prob=0.112, seed=41))


def open_model(A, Bm, Pi, csr=False):
    fv = decoder.FlashViterbi(0)
    if csr:
        fv.set_model_sparse(*decoder.dense_to_csr(A), Bm, Pi)
        fv.set_option(D.OPT_SPARSE_BEAM, 1)
    else:
        fv.set_model(A, Bm, Pi)
    return fv


def generations(T, n_split):
    """the plan's passes (L, R) generation by generation"""
    plan = decoder.plan_passes(T, n_split)
    return [[(L, R) for L, R, g, _ in plan if g == gen] for gen in range(1 + max(g for _, _, g, _ in plan))]


def decode(fv, ob, n_split, beam, debug, T=None):
    fv.set_option(D.OPT_DEBUG, debug)
    try:
        path, score, rc = fv.decode_beam(ob, n_split, beam, T=T)
    finally:
        fv.set_option(D.OPT_DEBUG, 0)
    return record(fv, rc, path, bits(score)), path


def forward(fv, ob, beam, passes, path, debug):
    """the passes (L, R) as one generation of fv_test_beam_forward, between the states of `path` (a decode's; -1 -> 0)"""
    state = lambda t: max(int(path[t]), 0)
    whole = len(passes) == 1 and passes[0] == (0, len(ob) - 1)
    tp = [(L, R, -1 if L == 0 else state(L - 1), -1 if whole else state(R)) for L, R in passes]
    fv.set_option(D.OPT_DEBUG, debug)
    try:
        out = fv.test_beam_forward(ob, beam, tp)
    finally:
        fv.set_option(D.OPT_DEBUG, 0)
    return record(fv, out["rc"], out["path"], bits(out["score"]), (out["variants"], out["selects"]))


# ---------------------------------------------------------------- the decodes

def measure_shape(name):
    """K = 600, B = 50: one plan under every FV_OPT_DEBUG of DEBUGS; its largest generation of at most 64 passes through
    fv_test_beam_forward under 0 and bit 17.  The first shape also on a CSR-set model under FV_OPT_SPARSE_BEAM and with
    ob == NULL on staged emission rows."""
    T, n_split, want = SHAPES[name]
    gens = generations(T, n_split)
    if want is not None:
        assert tuple(len(g) for g in gens) == want, name
    A, Bm, Pi, ob = data_model()
    ob = ob[:T]
    out = {}
    fv = open_model(A, Bm, Pi)
    try:
        path = None
        for debug in DEBUGS:
            out[f"dense dbg{debug}"], p = decode(fv, ob, n_split, BEAM0, debug)
            path = p if path is None else path
        hook = max((g for g in gens if len(g) <= 64 and (name != "T330 n4" or len(g) == BEAM_CHUNK + 1)), key=len)
        for debug in (0, GROUPS):
            out[f"forward{len(hook)} dbg{debug}"] = forward(fv, ob, BEAM0, hook, path, debug)
        if name == "T130 n8":
            fv.set_emissions(np.ascontiguousarray(libm_log(Bm)[:, ob].T))
            for debug in DEBUGS:
                out[f"emis dbg{debug}"], _ = decode(fv, None, n_split, BEAM0, debug, T=T)
            fv.clear_emissions()
    finally:
        fv.close()
    if name == "T130 n8":
        fv = open_model(A, Bm, Pi, csr=True)
        try:
            for debug in DEBUGS:
                out[f"csr dbg{debug}"], _ = decode(fv, ob, n_split, BEAM0, debug)
        finally:
            fv.close()
    return out


BATCH_LENGTHS = (40, 129, 2, 77, 33, 58)
BATCH_DEBUGS = (0, GEN0, ONE_STREAM, GROUPS)


def decode_batch(fv, seqs, n_split, beam, debug):
    fv.set_option(D.OPT_DEBUG, debug)
    try:
        paths, scores, statuses = fv.decode_beam_batch(seqs, n_split, beam)
    finally:
        fv.set_option(D.OPT_DEBUG, 0)
    return record(fv, statuses.max(), np.concatenate(paths), crc(scores))


def measure_batch():
    """fv_decode_beam_batch: six sequences at n_split 4 (generations of 6, 29, 56, 45, 16, 3 passes); then 450 short
    sequences at K = 100, whose generation 0 exceeds HEAP_CHUNK passes"""
    A, Bm, Pi, _ = data_model()
    rs = np.random.RandomState(5)
    seqs = [rs.randint(0, 8, n).astype(np.int32) for n in BATCH_LENGTHS]
    plan = decoder.plan_passes_batch(BATCH_LENGTHS, 4)
    assert [sum(1 for p in plan if p[2] == g) for g in range(6)] == [6, 29, 56, 45, 16, 3]
    out = {}
    fv = open_model(A, Bm, Pi)
    try:
        for debug in BATCH_DEBUGS:
            out[f"batch6 dbg{debug}"] = decode_batch(fv, seqs, 4, BEAM0, debug)
    finally:
        fv.close()
    lengths = [2 + i % 4 for i in range(450)]
    plan = decoder.plan_passes_batch(lengths, 2)
    assert max(sum(1 for p in plan if p[2] == g) for g in range(1 + max(p[2] for p in plan))) > HEAP_CHUNK
    A, Bm, Pi, _ = modelgen.model32(dict(kind="data_script", K=100, M=8, T=4, prob=0.3, seed=43))
    seqs = [rs.randint(0, 8, n).astype(np.int32) for n in lengths]
    fv = open_model(A, Bm, Pi)
    try:
        for debug in (0, ONE_STREAM):
            out[f"heap450 dbg{debug}"] = decode_batch(fv, seqs, 2, 10, debug)
    finally:
        fv.close()
    return out


def measure_thresholds():
    """K = 16000, T = 34, n_split 8 (generation 1: 8 passes of 2-3 steps).  beam * K = 16e6 at B = 1000: the generations
    fork; B = 999: they do not.  One whole-sequence pass moves 76.8 MB of float64 rows at B = 600 (below 80 MB: the float64
    kernel) and 128 MB at B = 1000 (the 16-bit kernel, 125 panels: 16 waves); the 8 passes of generation 1 in one launch
    are 1000 workgroups, more than 2 x 256 CUs: 8 waves."""
    K, T = 16000, 34
    A, Bm, Pi, ob = modelgen.model32(dict(kind="sparse_fast", K=K, M=8, T=T, prob=0.02, seed=16000))
    gens = generations(T, 8)
    assert len(gens[1]) == 8 and all(2 <= R - L <= 3 for L, R in gens[1])
    out = {}
    fv = open_model(A, Bm, Pi)
    try:
        for beam in (999, 1000):
            out[f"decode B{beam}"], path = decode(fv, ob, 8, beam, 0)
        for beam in (600, 1000):
            out[f"forward whole B{beam}"] = forward(fv, ob, beam, [(0, T - 1)], path, 0)
        out["forward gen1 B999"] = forward(fv, ob, 999, gens[1], path, 0)
        out["forward gen1 B1000"] = forward(fv, ob, 1000, gens[1], path, 0)
    finally:
        fv.close()
    return out


# ---------------------------------------------------------------- the table (recorded from the parent commit)

EXPECTED = {
    "T130 n8": {
        "dense dbg0": (0, 155, 371, 64, 5, 4170943097, 3290582559, 2, 0, 0, 0, 0, 0, 0, 0, 0),
        "dense dbg65536": (0, 155, 371, 64, 5, 4170943097, 3290582559, 2, 0, 0, 0, 0, 0, 0, 0, 0),
        "dense dbg131072": (0, 233, 371, 64, 5, 4170943097, 3290582559, 2, 0, 0, 0, 0, 0, 0, 0, 0),
        "dense dbg524288": (0, 155, 371, 64, 5, 4170943097, 3290582559, 2, 0, 2, 0, 0, 0, 4, 0, 0),
        "dense dbg1048576": (0, 155, 371, 64, 5, 4170943097, 3290582559, 0, 0, 2, 0, 0, 0, 0, 0, 0),
        "dense dbg256": (0, 155, 371, 64, 5, 4170943097, 3290582559, 2, 0, 0, 0, 0, 0, 0, 0, 0),
        "dense dbg512": (0, 155, 371, 64, 5, 4170943097, 3290582559, 2, 0, 0, 0, 0, 0, 0, 0, 0),
        "dense dbg33554432": (0, 155, 371, 64, 5, 4170943097, 3290582559, 2, 0, 0, 0, 0, 0, 0, 0, 0),
        "dense dbg67108864": (0, 155, 371, 64, 5, 4170943097, 3290582559, 2, 0, 0, 0, 0, 0, 0, 0, 0),
        "dense dbg655360": (0, 233, 371, 64, 5, 4170943097, 3290582559, 2, 0, 2, 0, 0, 0, 4, 0, 0),
        "forward24 dbg0": (0, 7, 82, 24, 1, 1699084204, 2143289344, 0, 0, 0, 0, 0, 0, 0, 0, 0, 70368744177664, 1),
        "forward24 dbg131072": (0, 28, 82, 24, 1, 1699084204, 2143289344, 0, 0, 0, 0, 0, 0, 0, 0, 0, 70368744177664, 1),
        "emis dbg0": (0, 155, 371, 64, 5, 4170943097, 3290582559, 2, 0, 0, 0, 0, 0, 0, 0, 0),
        "emis dbg65536": (0, 155, 371, 64, 5, 4170943097, 3290582559, 2, 0, 0, 0, 0, 0, 0, 0, 0),
        "emis dbg131072": (0, 233, 371, 64, 5, 4170943097, 3290582559, 2, 0, 0, 0, 0, 0, 0, 0, 0),
        "emis dbg524288": (0, 155, 371, 64, 5, 4170943097, 3290582559, 2, 0, 2, 0, 0, 0, 4, 0, 0),
        "emis dbg1048576": (0, 155, 371, 64, 5, 4170943097, 3290582559, 0, 0, 2, 0, 0, 0, 0, 0, 0),
        "emis dbg256": (0, 155, 371, 64, 5, 4170943097, 3290582559, 2, 0, 0, 0, 0, 0, 0, 0, 0),
        "emis dbg512": (0, 155, 371, 64, 5, 4170943097, 3290582559, 2, 0, 0, 0, 0, 0, 0, 0, 0),
        "emis dbg33554432": (0, 155, 371, 64, 5, 4170943097, 3290582559, 2, 0, 0, 0, 0, 0, 0, 0, 0),
        "emis dbg67108864": (0, 155, 371, 64, 5, 4170943097, 3290582559, 2, 0, 0, 0, 0, 0, 0, 0, 0),
        "emis dbg655360": (0, 233, 371, 64, 5, 4170943097, 3290582559, 2, 0, 2, 0, 0, 0, 4, 0, 0),
        "csr dbg0": (0, 155, 371, 64, 5, 4170943097, 3290582559, 2, 0, 0, 0, 0, 0, 0, 0, 0),
        "csr dbg65536": (0, 155, 371, 64, 5, 4170943097, 3290582559, 2, 0, 0, 0, 0, 0, 0, 0, 0),
        "csr dbg131072": (0, 233, 371, 64, 5, 4170943097, 3290582559, 2, 0, 0, 0, 0, 0, 0, 0, 0),
        "csr dbg524288": (0, 155, 371, 64, 5, 4170943097, 3290582559, 2, 0, 2, 0, 0, 0, 4, 0, 0),
        "csr dbg1048576": (0, 155, 371, 64, 5, 4170943097, 3290582559, 0, 0, 2, 0, 0, 0, 0, 0, 0),
        "csr dbg256": (0, 155, 371, 64, 5, 4170943097, 3290582559, 2, 0, 0, 0, 0, 0, 0, 0, 0),
        "csr dbg512": (0, 155, 371, 64, 5, 4170943097, 3290582559, 2, 0, 0, 0, 0, 0, 0, 0, 0),
        "csr dbg33554432": (0, 155, 371, 64, 5, 4170943097, 3290582559, 2, 0, 0, 0, 0, 0, 0, 0, 0),
        "csr dbg67108864": (0, 155, 371, 64, 5, 4170943097, 3290582559, 2, 0, 0, 0, 0, 0, 0, 0, 0),
        "csr dbg655360": (0, 233, 371, 64, 5, 4170943097, 3290582559, 2, 0, 2, 0, 0, 0, 4, 0, 0),
    },
    "T330 n4": {
        "dense dbg0": (0, 487, 1233, 128, 7, 1141897149, 3301790041, 5, 0, 0, 0, 0, 0, 0, 0, 1),
        "dense dbg65536": (0, 487, 1233, 128, 7, 1141897149, 3301790041, 5, 0, 0, 0, 0, 0, 0, 0, 1),
        "dense dbg131072": (0, 866, 1233, 128, 7, 1141897149, 3301790041, 5, 0, 0, 0, 0, 0, 0, 0, 1),
        "dense dbg524288": (0, 487, 1233, 128, 7, 1141897149, 3301790041, 5, 0, 5, 0, 0, 0, 19, 0, 1),
        "dense dbg1048576": (0, 487, 1233, 128, 7, 1141897149, 3301790041, 0, 0, 5, 0, 0, 0, 0, 0, 1),
        "dense dbg256": (0, 487, 1233, 128, 7, 1141897149, 3301790041, 5, 0, 0, 0, 0, 0, 0, 0, 1),
        "dense dbg512": (0, 487, 1233, 128, 7, 1141897149, 3301790041, 5, 0, 0, 0, 0, 0, 0, 0, 1),
        "dense dbg33554432": (0, 487, 1233, 128, 7, 1141897149, 3301790041, 5, 0, 0, 0, 0, 0, 0, 0, 1),
        "dense dbg67108864": (0, 487, 1233, 128, 7, 1141897149, 3301790041, 5, 0, 0, 0, 0, 0, 0, 0, 1),
        "dense dbg655360": (0, 866, 1233, 128, 7, 1141897149, 3301790041, 5, 0, 5, 0, 0, 0, 19, 0, 1),
        "forward25 dbg0": (0, 41, 278, 25, 1, 3501083387, 2143289344, 0, 0, 0, 0, 0, 0, 0, 0, 0, 70368744177664, 3),
        "forward25 dbg131072": (0, 140, 278, 25, 1, 3501083387, 2143289344, 0, 0, 0, 0, 0, 0, 0, 0, 0, 70368744177664, 1),
    },
    "T330 n16": {
        "dense dbg0": (0, 368, 969, 128, 5, 2500745765, 3301790041, 4, 0, 0, 0, 0, 0, 0, 0, 1),
        "dense dbg65536": (0, 368, 969, 128, 5, 2500745765, 3301790041, 4, 0, 0, 0, 0, 0, 0, 0, 1),
        "dense dbg131072": (0, 465, 969, 128, 5, 2500745765, 3301790041, 4, 0, 0, 0, 0, 0, 0, 0, 1),
        "dense dbg524288": (0, 368, 969, 128, 5, 2500745765, 3301790041, 4, 0, 4, 0, 0, 0, 20, 0, 1),
        "dense dbg1048576": (0, 368, 969, 128, 5, 2500745765, 3301790041, 0, 0, 4, 0, 0, 0, 0, 0, 1),
        "dense dbg256": (0, 368, 969, 128, 5, 2500745765, 3301790041, 4, 0, 0, 0, 0, 0, 0, 0, 1),
        "dense dbg512": (0, 368, 969, 128, 5, 2500745765, 3301790041, 4, 0, 0, 0, 0, 0, 0, 0, 1),
        "dense dbg33554432": (0, 368, 969, 128, 5, 2500745765, 3301790041, 4, 0, 0, 0, 0, 0, 0, 0, 1),
        "dense dbg67108864": (0, 368, 969, 128, 5, 2500745765, 3301790041, 4, 0, 0, 0, 0, 0, 0, 0, 1),
        "dense dbg655360": (0, 465, 969, 128, 5, 2500745765, 3301790041, 4, 0, 4, 0, 0, 0, 20, 0, 1),
        "forward48 dbg0": (0, 13, 225, 48, 1, 2407706833, 2143289344, 0, 0, 0, 0, 0, 0, 0, 0, 0, 70368744177664, 3),
        "forward48 dbg131072": (0, 36, 225, 48, 1, 2407706833, 2143289344, 0, 0, 0, 0, 0, 0, 0, 0, 0, 70368744177664, 1),
    },
    "T530 n16": {
        "dense dbg0": (0, 602, 1795, 256, 6, 2383228665, 3307521154, 6, 0, 0, 0, 0, 0, 0, 0, 2),
        "dense dbg65536": (0, 602, 1795, 256, 6, 2383228665, 3307521154, 6, 0, 0, 0, 0, 0, 0, 0, 2),
        "dense dbg131072": (0, 761, 1795, 256, 6, 2383228665, 3307521154, 6, 0, 0, 0, 0, 0, 0, 0, 2),
        "dense dbg524288": (0, 602, 1795, 256, 6, 2383228665, 3307521154, 6, 0, 6, 0, 0, 0, 68, 0, 2),
        "dense dbg1048576": (0, 602, 1795, 256, 6, 2383228665, 3307521154, 0, 0, 6, 0, 0, 0, 0, 0, 2),
        "dense dbg256": (0, 602, 1795, 256, 6, 2383228665, 3307521154, 6, 0, 0, 0, 0, 0, 0, 0, 2),
        "dense dbg512": (0, 602, 1795, 256, 6, 2383228665, 3307521154, 6, 0, 0, 0, 0, 0, 0, 0, 2),
        "dense dbg33554432": (0, 602, 1795, 256, 6, 2383228665, 3307521154, 6, 0, 0, 0, 0, 0, 0, 0, 2),
        "dense dbg67108864": (0, 602, 1795, 256, 6, 2383228665, 3307521154, 6, 0, 0, 0, 0, 0, 0, 0, 2),
        "dense dbg655360": (0, 761, 1795, 256, 6, 2383228665, 3307521154, 6, 0, 6, 0, 0, 0, 68, 0, 2),
        "forward61 dbg0": (0, 5, 91, 61, 1, 2600655140, 2143289344, 0, 0, 0, 0, 0, 0, 0, 0, 0, 70368744177664, 3),
        "forward61 dbg131072": (0, 12, 91, 61, 1, 2600655140, 2143289344, 0, 0, 0, 0, 0, 0, 0, 0, 0, 70368744177664, 1),
    },
    "batch": {
        "batch6 dbg0": (0, 364, 937, 155, 6, 3860265841, 741661088, 1, 0, 0, 0, 0, 0, 0, 0, 1),
        "batch6 dbg536870912": (0, 192, 937, 155, 6, 3860265841, 741661088, 1, 0, 0, 0, 0, 0, 0, 0, 1),
        "batch6 dbg65536": (0, 192, 937, 155, 6, 3860265841, 741661088, 1, 0, 0, 0, 0, 0, 0, 0, 1),
        "batch6 dbg131072": (0, 501, 937, 155, 6, 3860265841, 741661088, 1, 0, 0, 0, 0, 0, 0, 0, 1),
        "heap450 dbg0": (0, 66, 1347, 674, 2, 1867714071, 711593310, 0, 0, 0, 0, 0, 0, 0, 0, 0),
        "heap450 dbg65536": (0, 59, 1347, 674, 2, 1867714071, 711593310, 0, 0, 0, 0, 0, 0, 0, 0, 0),
    },
    "thresholds": {
        "decode B999": (0, 37, 63, 16, 3, 742597126, 3277736258, 0, 0, 0, 46, 0, 1, 0, 0, 0),
        "decode B1000": (0, 49, 63, 16, 3, 742597126, 3277736258, 3, 0, 1, 46, 0, 1, 0, 0, 0),
        "forward whole B600": (0, 33, 33, 1, 1, 742597126, 3277736258, 0, 0, 0, 32, 0, 0, 0, 0, 0, 140737488355328, 4),
        "forward whole B1000": (0, 33, 33, 1, 1, 742597126, 3277736258, 3, 0, 1, 32, 0, 0, 0, 0, 0, 562949953421312, 4),
        "forward gen1 B999": (0, 3, 23, 8, 1, 22428731, 2143289344, 0, 0, 0, 6, 8, 1, 0, 0, 0, 281474976710656, 4),
        "forward gen1 B1000": (0, 12, 23, 8, 1, 22428731, 2143289344, 0, 0, 0, 6, 8, 1, 0, 0, 0, 562949953421312, 4),
    },
}


def check(name, got):
    want = EXPECTED[name]
    for key in sorted(got):
        print(f"{name}: {key}: {got[key]}")
    assert sorted(got) == sorted(want), f"{name}: the cases differ from the table's"
    wrong = {k: (got[k], want[k]) for k in got
             if len(got[k]) != len(want[k]) or any(w is not None and g != w for g, w in zip(got[k], want[k]))}
    assert not wrong, f"{name}: (got, recorded) {ALL_FIELDS} differ for {len(wrong)} decodes: {wrong}"


LAUNCHES = FIELDS.index("step_launches")


@pytest.mark.parametrize("name", list(SHAPES))
def test_plan_under_every_switch(name):
    got = measure_shape(name)
    check(name, got)
    # the shape reaches what it is here for: bit 17 deals the generations out (more launches), bit 16 changes nothing at
    # this beam * K, no switch moves the work
    assert got[f"dense dbg{GROUPS}"][LAUNCHES] > got["dense dbg0"][LAUNCHES]
    assert got[f"dense dbg{ONE_STREAM}"] == got["dense dbg0"]
    assert len({r[2:5] for r in got.values() if len(r) == len(ALL_FIELDS)}) == 1
    hook = [k for k in got if k.startswith("forward")]
    selects = {k: got[k][-1] for k in hook}
    if name == "T330 n4":       # 25 passes: the second chunk makes the select derive its jobs; dealt to four groups it lists them
        assert selects["forward25 dbg0"] & TS_DERIVED and not selects[f"forward25 dbg{GROUPS}"] & TS_DERIVED
        assert got["forward25 dbg0"][LAUNCHES] > max(R - L for L, R in next(g for g in generations(330, 4) if len(g) == 25))
    if name == "T130 n8":       # 24 passes: one chunk, listed
        assert selects["forward24 dbg0"] & TS_LISTED and not selects["forward24 dbg0"] & TS_DERIVED
        assert got[f"csr dbg0"][:5] == got["dense dbg0"][:5] == got["emis dbg0"][:5]


def test_batch_and_heap_chunk():
    got = measure_batch()
    check("batch", got)
    # generation 0 of the forest changes form under bit 29; the default deals it out, as bit 17 does the later ones too
    assert got[f"batch6 dbg{GEN0}"][LAUNCHES] < got["batch6 dbg0"][LAUNCHES] < got[f"batch6 dbg{GROUPS}"][LAUNCHES]
    assert got[f"batch6 dbg{GEN0}"][LAUNCHES] == got[f"batch6 dbg{ONE_STREAM}"][LAUNCHES]
    assert got["heap450 dbg0"][LAUNCHES] > got[f"heap450 dbg{ONE_STREAM}"][LAUNCHES]


def test_size_thresholds():
    got = measure_thresholds()
    check("thresholds", got)
    assert got["decode B999"][LAUNCHES] != got["decode B1000"][LAUNCHES]
    variants = {k: got[k][-2] for k in got if k.startswith("forward")}
    assert variants["forward whole B600"] == TV_W16
    assert variants["forward whole B1000"] == TV_Q16_W16
    assert variants["forward gen1 B999"] == TV_Q16_W8
