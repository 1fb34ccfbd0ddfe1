"""GPU: the launch geometry of the full-state driver, pinned decode by decode.

Every other test compares what a decode returns.  How the driver queues it can change without moving one decoded bit:
a batch limit of 4 where it was 8, a generation that no longer forks, last columns run as full steps, a stream's steps
counted as a decode's.  So each decode below is made once and five fields of fv_last_stats are compared with a table:

    (step_launches, task_steps, column_steps, passes, flat_passes)

The table was recorded from the commit before the launch layer took its arguments explicitly (launch description,
one generation policy) and asserts equality: it pins what that commit did, never what the code under test does.  For
fv_test_forward the FV_TV_* variant bits are pinned as well."""
import numpy as np
import pytest

import modelgen
from flash_viterbi_amd import decoder

pytestmark = pytest.mark.gpu

D = decoder
FIELDS = ("step_launches", "task_steps", "column_steps", "passes", "flat_passes")
KERNELS = {"auto": D.KERNEL_AUTO, "f64": D.KERNEL_F64_STREAM, "f32": D.KERNEL_F32_REFINE, "f16": D.KERNEL_F16_REFINE,
           "q16": D.KERNEL_Q16_REFINE, "sparse": D.KERNEL_SPARSE_Q16, "u16": D.KERNEL_U16_REFINE, "csr64": D.KERNEL_CSR_F64}
# FV_OPT_DEBUG: bit 3 every last step a full step, bit 14 the packed kernel for batched launches, bit 18 no forked streams
DEBUGS = (0, 1 << 3, 1 << 14, 1 << 18)
K0, T0 = 600, 130


def counts(fv):
    s = fv.stats()
    return tuple(int(s[f]) for f in FIELDS)


def data_model(T):
    return modelgen.model32(dict(kind="data_script", K=K0, M=8, T=T, prob=0.112, seed=41))


def open_model(A, Bm, Pi, csr):
    fv = decoder.FlashViterbi(0)
    if csr:
        fv.set_model_sparse(*decoder.dense_to_csr(A), Bm, Pi)
    else:
        fv.set_model(A, Bm, Pi)
    return fv


def decode(fv, ob, n_split, kernel="auto", batch=8, flat=1, debug=0, mode=D.MODE_REFERENCE):
    fv.set_option(D.OPT_KERNEL, KERNELS[kernel])
    fv.set_option(D.OPT_MAX_BATCH, batch)
    fv.set_option(D.OPT_FLAT_GENERATIONS, flat)
    fv.set_option(D.OPT_DEBUG, debug)
    fv.decode_full(ob, n_split, mode)
    return counts(fv)


# ---------------------------------------------------------------- the decodes

def measure_matrix(csr):
    """K = 600, T = 130, n_split = 8: every kernel choice x FV_OPT_MAX_BATCH x FV_OPT_FLAT_GENERATIONS x FV_OPT_DEBUG"""
    A, Bm, Pi, ob = data_model(T0)
    fv = open_model(A, Bm, Pi, csr)
    out = {}
    try:
        for kernel in (("auto", "sparse", "csr64") if csr else ("auto", "f64", "f32", "f16", "q16", "sparse", "u16")):
            for batch in (1, 3, 8):
                for flat in (0, 2):
                    for debug in DEBUGS:
                        out[f"{kernel} b{batch} flat{flat} dbg{debug}"] = decode(fv, ob, 8, kernel, batch, flat, debug)
    finally:
        fv.close()
    return out


def measure_fork_threshold():
    """T = 330, n_split = 4: generation 1 has 8 passes of up to 81 steps, two batches of four — the generation driver
    deals them to two streams, the flat form asks for three (n_split = 16 at this T has generations of 18, 48, 46 and
    15 passes, none between 5 and 8; it is measured as well).  T = 530, n_split = 4 on the CSR-set model: passes of 64+
    steps, the walk kernels' fork rule; n_split = 16 there: no pass of 64 steps, no fork."""
    A, Bm, Pi, ob = data_model(530)
    out = {}
    fv = open_model(A, Bm, Pi, False)
    try:
        for kernel in ("u16", "sparse", "q16"):
            for n_split in (4, 16):
                for flat in (0, 2):
                    for debug in (0, 1 << 18):
                        out[f"dense {kernel} T330 n{n_split} flat{flat} dbg{debug}"] = decode(fv, ob[:330], n_split, kernel, 8, flat, debug)
    finally:
        fv.close()
    fv = open_model(A, Bm, Pi, True)
    try:
        for kernel in ("auto", "csr64"):
            for T, n_split in ((330, 4), (530, 4), (530, 16)):
                for flat in (0, 2):
                    for debug in (0, 1 << 18):
                        out[f"csr {kernel} T{T} n{n_split} flat{flat} dbg{debug}"] = decode(fv, ob[:T], n_split, kernel, 8, flat, debug)
    finally:
        fv.close()
    return out


LDS_KS = (4320, 4321, 9440, 9441)


def measure_lds_boundary(K):
    """The K at which the batched launches' score rows stop fitting LDS (8 -> 4 tasks after 4320, 4 -> 2 after 9440);
    the models of test_gpu_step_tables.py's boundary cases.  T = 12, n_split = 4 has generations of at most 4 passes,
    which no limit above 4 shows; T = 34, n_split = 8 is the smallest plan with a generation of 8 passes of more than
    one step (3 each), and a checkpoint decode of step 4 there has 9 segments."""
    A, Bm, Pi, ob = modelgen.model32(dict(kind="sparse_fast", K=K, M=8, T=34, prob=0.02, seed=900 + K))
    fv = open_model(A, Bm, Pi, False)
    out = {}
    try:
        for kernel in ("q16", "f64", "u16"):
            for debug in (0, 1 << 18):
                out[f"{kernel} T12 n4 dbg{debug}"] = decode(fv, ob[:12], 4, kernel, 8, 0, debug)
                out[f"{kernel} T34 n8 dbg{debug}"] = decode(fv, ob, 8, kernel, 8, 0, debug)
        fv.set_option(D.OPT_DEBUG, 0)
        fv.decode_checkpoint(ob, 4)
        out["checkpoint T34 step4"] = counts(fv)
    finally:
        fv.close()
    return out


def measure_entry_points():
    """single pass, vanilla, checkpoint, the batch decode, a stream push after a decode, fv_test_forward"""
    A, Bm, Pi, ob = data_model(T0)
    fv = open_model(A, Bm, Pi, False)
    out = {}
    try:
        for kernel in ("auto", "u16", "f64"):
            out[f"single_pass {kernel}"] = decode(fv, ob, 1, kernel, mode=D.MODE_SINGLE_PASS)
        fv.set_option(D.OPT_KERNEL, D.KERNEL_AUTO)
        fv.decode_vanilla(ob)
        out["vanilla"] = counts(fv)
        for step in (0, 7):
            for batch in (3, 8):
                fv.set_option(D.OPT_MAX_BATCH, batch)
                fv.decode_checkpoint(ob, step)
                out[f"checkpoint step{step} b{batch}"] = counts(fv)
        rs = np.random.RandomState(5)
        # (four sequences: generation 0 has four passes, too few to fork under either setting of bit 28; six: it forks)
        seqs = [rs.randint(0, 8, n).astype(np.int32) for n in (40, 129, 2, 77, 33, 58)]
        for kernel in ("auto", "u16", "q16"):
            for debug in (0, 1 << 28):
                for nseq in (4, 6):
                    fv.set_option(D.OPT_KERNEL, KERNELS[kernel])
                    fv.set_option(D.OPT_DEBUG, debug)
                    fv.decode_full_batch(seqs[:nseq], 4)
                    out[f"batch{nseq} {kernel} dbg{debug}"] = counts(fv)
        # a stream's launches are not a decode's: fv_last_stats keeps the decode's figures across a push
        for kernel in ("auto", "u16"):
            before = decode(fv, ob, 8, kernel)
            fv.stream_open()
            try:
                fv.stream_push(ob[:40])
                out[f"stream {kernel} after push"] = counts(fv)
                assert counts(fv) == before, "fv_stream_push changed fv_last_stats"
            finally:
                fv.stream_abort()
        # six passes of 64+ steps, one after the other with a gap of one step: the forked form of the hook
        passes, L = [], 0
        for n in (70, 64, 66, 80, 64, 65):
            passes.append((L, L + n, -1 if L == 0 else (7 * L) % K0))
            L += n + 1
        obf = np.random.RandomState(6).randint(0, 8, L + 1).astype(np.int32)
        for kernel in ("auto", "u16", "q16"):
            for debug in (0, 1 << 18):
                fv.set_option(D.OPT_KERNEL, KERNELS[kernel])
                fv.set_option(D.OPT_DEBUG, debug)
                fv.set_option(D.OPT_MAX_BATCH, 8)
                _, _, variants = fv.test_forward(obf, passes)
                out[f"test_forward {kernel} dbg{debug}"] = counts(fv) + (variants,)
    finally:
        fv.close()
    return out


# ---------------------------------------------------------------- the table (recorded from the parent commit)

# K = 600, T = 130, n_split = 8: per (FV_OPT_MAX_BATCH, FV_OPT_FLAT_GENERATIONS) the figures under FV_OPT_DEBUG 0, bit 3,
# bit 14, bit 18.  Every kernel choice of both model forms recorded these rows (the walks' passes are shorter than 64
# steps: no fork) but the packed kernel at a batch limit of 8, which forks.
_MATRIX = {
    "b1 flat0": ((308, 308, 63, 64, 0), (371, 371, 0, 64, 0), (308, 308, 63, 64, 0), (308, 308, 63, 64, 0)),
    "b1 flat2": ((308, 308, 63, 64, 63), (371, 371, 0, 64, 63), (308, 308, 63, 64, 63), (308, 308, 63, 64, 63)),
    "b3 flat0": ((199, 308, 63, 64, 0), (222, 371, 0, 64, 0), (199, 308, 63, 64, 0), (199, 308, 63, 64, 0)),
    "b3 flat2": ((195, 308, 63, 64, 63), (217, 371, 0, 64, 63), (195, 308, 63, 64, 63), (195, 308, 63, 64, 63)),
    "b8 flat0": ((155, 308, 63, 64, 0), (164, 371, 0, 64, 0), (155, 308, 63, 64, 0), (155, 308, 63, 64, 0)),
    "b8 flat2": ((153, 308, 63, 64, 63), (161, 371, 0, 64, 63), (153, 308, 63, 64, 63), (153, 308, 63, 64, 63)),
}
_MATRIX_U16 = {
    "b8 flat0": ((179, 308, 63, 64, 0), (196, 371, 0, 64, 0), (179, 308, 63, 64, 0), (155, 308, 63, 64, 0)),
    "b8 flat2": ((177, 308, 63, 64, 63), (193, 371, 0, 64, 63), (177, 308, 63, 64, 63), (153, 308, 63, 64, 63)),
}


def _matrix(kernels):
    return {f"{kernel} {row} dbg{debug}": (_MATRIX_U16 if kernel == "u16" and row in _MATRIX_U16 else _MATRIX)[row][i]
            for kernel in kernels for row in _MATRIX for i, debug in enumerate(DEBUGS)}


EXPECTED = {
    "matrix-dense": _matrix(("auto", "f64", "f32", "f16", "q16", "sparse", "u16")),
    "matrix-csr": _matrix(("auto", "sparse", "csr64")),
    "fork": {
        "csr auto T330 n4 flat0 dbg0": (522, 1106, 127, 128, 0), "csr auto T330 n4 flat0 dbg262144": (503, 1106, 127, 128, 0),
        "csr auto T330 n4 flat2 dbg0": (544, 1106, 127, 128, 127), "csr auto T330 n4 flat2 dbg262144": (458, 1106, 127, 128, 127),
        "csr auto T530 n16 flat0 dbg0": (666, 1540, 255, 256, 0), "csr auto T530 n16 flat0 dbg262144": (666, 1540, 255, 256, 0),
        "csr auto T530 n16 flat2 dbg0": (659, 1540, 255, 256, 255), "csr auto T530 n16 flat2 dbg262144": (659, 1540, 255, 256, 255),
        "csr auto T530 n4 flat0 dbg0": (906, 1970, 255, 256, 0), "csr auto T530 n4 flat0 dbg262144": (836, 1970, 255, 256, 0),
        "csr auto T530 n4 flat2 dbg0": (922, 1970, 255, 256, 255), "csr auto T530 n4 flat2 dbg262144": (759, 1970, 255, 256, 255),
        "csr csr64 T330 n4 flat0 dbg0": (522, 1106, 127, 128, 0), "csr csr64 T330 n4 flat0 dbg262144": (503, 1106, 127, 128, 0),
        "csr csr64 T330 n4 flat2 dbg0": (544, 1106, 127, 128, 127), "csr csr64 T330 n4 flat2 dbg262144": (458, 1106, 127, 128, 127),
        "csr csr64 T530 n16 flat0 dbg0": (666, 1540, 255, 256, 0), "csr csr64 T530 n16 flat0 dbg262144": (666, 1540, 255, 256, 0),
        "csr csr64 T530 n16 flat2 dbg0": (659, 1540, 255, 256, 255), "csr csr64 T530 n16 flat2 dbg262144": (659, 1540, 255, 256, 255),
        "csr csr64 T530 n4 flat0 dbg0": (906, 1970, 255, 256, 0), "csr csr64 T530 n4 flat0 dbg262144": (836, 1970, 255, 256, 0),
        "csr csr64 T530 n4 flat2 dbg0": (922, 1970, 255, 256, 255), "csr csr64 T530 n4 flat2 dbg262144": (759, 1970, 255, 256, 255),
        "dense q16 T330 n16 flat0 dbg0": (398, 842, 127, 128, 0), "dense q16 T330 n16 flat0 dbg262144": (398, 842, 127, 128, 0),
        "dense q16 T330 n16 flat2 dbg0": (396, 842, 127, 128, 127), "dense q16 T330 n16 flat2 dbg262144": (396, 842, 127, 128, 127),
        "dense q16 T330 n4 flat0 dbg0": (503, 1106, 127, 128, 0), "dense q16 T330 n4 flat0 dbg262144": (503, 1106, 127, 128, 0),
        "dense q16 T330 n4 flat2 dbg0": (458, 1106, 127, 128, 127), "dense q16 T330 n4 flat2 dbg262144": (458, 1106, 127, 128, 127),
        "dense sparse T330 n16 flat0 dbg0": (398, 842, 127, 128, 0), "dense sparse T330 n16 flat0 dbg262144": (398, 842, 127, 128, 0),
        "dense sparse T330 n16 flat2 dbg0": (396, 842, 127, 128, 127), "dense sparse T330 n16 flat2 dbg262144": (396, 842, 127, 128, 127),
        "dense sparse T330 n4 flat0 dbg0": (522, 1106, 127, 128, 0), "dense sparse T330 n4 flat0 dbg262144": (503, 1106, 127, 128, 0),
        "dense sparse T330 n4 flat2 dbg0": (544, 1106, 127, 128, 127), "dense sparse T330 n4 flat2 dbg262144": (458, 1106, 127, 128, 127),
        "dense u16 T330 n16 flat0 dbg0": (464, 842, 127, 128, 0), "dense u16 T330 n16 flat0 dbg262144": (398, 842, 127, 128, 0),
        "dense u16 T330 n16 flat2 dbg0": (462, 842, 127, 128, 127), "dense u16 T330 n16 flat2 dbg262144": (396, 842, 127, 128, 127),
        "dense u16 T330 n4 flat0 dbg0": (564, 1106, 127, 128, 0), "dense u16 T330 n4 flat0 dbg262144": (503, 1106, 127, 128, 0),
        "dense u16 T330 n4 flat2 dbg0": (544, 1106, 127, 128, 127), "dense u16 T330 n4 flat2 dbg262144": (458, 1106, 127, 128, 127),
    },
    "lds-4320": {
        "checkpoint T34 step4": (38, 66, 0, 10, 0), "f64 T12 n4 dbg0": (12, 13, 4, 5, 0), "f64 T12 n4 dbg262144": (12, 13, 4, 5, 0),
        "f64 T34 n8 dbg0": (35, 48, 15, 16, 0), "f64 T34 n8 dbg262144": (35, 48, 15, 16, 0), "q16 T12 n4 dbg0": (12, 13, 4, 5, 0),
        "q16 T12 n4 dbg262144": (12, 13, 4, 5, 0), "q16 T34 n8 dbg0": (35, 48, 15, 16, 0), "q16 T34 n8 dbg262144": (35, 48, 15, 16, 0),
        "u16 T12 n4 dbg0": (12, 13, 4, 5, 0), "u16 T12 n4 dbg262144": (12, 13, 4, 5, 0), "u16 T34 n8 dbg0": (37, 48, 15, 16, 0),
        "u16 T34 n8 dbg262144": (35, 48, 15, 16, 0),
    },
    "lds-4321": {
        "checkpoint T34 step4": (42, 66, 0, 10, 0), "f64 T12 n4 dbg0": (12, 13, 4, 5, 0), "f64 T12 n4 dbg262144": (12, 13, 4, 5, 0),
        "f64 T34 n8 dbg0": (37, 48, 15, 16, 0), "f64 T34 n8 dbg262144": (37, 48, 15, 16, 0), "q16 T12 n4 dbg0": (12, 13, 4, 5, 0),
        "q16 T12 n4 dbg262144": (12, 13, 4, 5, 0), "q16 T34 n8 dbg0": (37, 48, 15, 16, 0), "q16 T34 n8 dbg262144": (37, 48, 15, 16, 0),
        "u16 T12 n4 dbg0": (12, 13, 4, 5, 0), "u16 T12 n4 dbg262144": (12, 13, 4, 5, 0), "u16 T34 n8 dbg0": (37, 48, 15, 16, 0),
        "u16 T34 n8 dbg262144": (37, 48, 15, 16, 0),
    },
    "lds-9440": {
        "checkpoint T34 step4": (42, 66, 0, 10, 0), "f64 T12 n4 dbg0": (12, 13, 4, 5, 0), "f64 T12 n4 dbg262144": (12, 13, 4, 5, 0),
        "f64 T34 n8 dbg0": (37, 48, 15, 16, 0), "f64 T34 n8 dbg262144": (37, 48, 15, 16, 0), "q16 T12 n4 dbg0": (12, 13, 4, 5, 0),
        "q16 T12 n4 dbg262144": (12, 13, 4, 5, 0), "q16 T34 n8 dbg0": (37, 48, 15, 16, 0), "q16 T34 n8 dbg262144": (37, 48, 15, 16, 0),
        "u16 T12 n4 dbg0": (12, 13, 4, 5, 0), "u16 T12 n4 dbg262144": (12, 13, 4, 5, 0), "u16 T34 n8 dbg0": (37, 48, 15, 16, 0),
        "u16 T34 n8 dbg262144": (37, 48, 15, 16, 0),
    },
    "lds-9441": {
        "checkpoint T34 step4": (50, 66, 0, 10, 0), "f64 T12 n4 dbg0": (12, 13, 4, 5, 0), "f64 T12 n4 dbg262144": (12, 13, 4, 5, 0),
        "f64 T34 n8 dbg0": (41, 48, 15, 16, 0), "f64 T34 n8 dbg262144": (41, 48, 15, 16, 0), "q16 T12 n4 dbg0": (12, 13, 4, 5, 0),
        "q16 T12 n4 dbg262144": (12, 13, 4, 5, 0), "q16 T34 n8 dbg0": (41, 48, 15, 16, 0), "q16 T34 n8 dbg262144": (41, 48, 15, 16, 0),
        "u16 T12 n4 dbg0": (12, 13, 4, 5, 0), "u16 T12 n4 dbg262144": (12, 13, 4, 5, 0), "u16 T34 n8 dbg0": (41, 48, 15, 16, 0),
        "u16 T34 n8 dbg262144": (41, 48, 15, 16, 0),
    },
    # (test_forward: the sixth figure is the FV_TV_* variant bits the hook returned)
    "entry": {
        "batch4 auto dbg0": (198, 606, 109, 113, 0), "batch4 auto dbg268435456": (198, 606, 109, 113, 0), "batch4 q16 dbg0": (198, 606, 109, 113, 0),
        "batch4 q16 dbg268435456": (198, 606, 109, 113, 0), "batch4 u16 dbg0": (234, 606, 109, 113, 0),
        "batch4 u16 dbg268435456": (234, 606, 109, 113, 0), "batch6 auto dbg0": (244, 788, 149, 155, 0),
        "batch6 auto dbg268435456": (212, 788, 149, 155, 0), "batch6 q16 dbg0": (212, 788, 149, 155, 0),
        "batch6 q16 dbg268435456": (212, 788, 149, 155, 0), "batch6 u16 dbg0": (292, 788, 149, 155, 0),
        "batch6 u16 dbg268435456": (260, 788, 149, 155, 0), "checkpoint step0 b3": (173, 258, 0, 13, 0), "checkpoint step0 b8": (151, 258, 0, 13, 0),
        "checkpoint step7 b3": (174, 258, 0, 20, 0), "checkpoint step7 b8": (150, 258, 0, 20, 0), "single_pass auto": (129, 129, 0, 1, 0),
        "single_pass f64": (129, 129, 0, 1, 0), "single_pass u16": (129, 129, 0, 1, 0), "stream auto after push": (155, 308, 63, 64, 0),
        "stream u16 after push": (177, 308, 63, 64, 63), "test_forward auto dbg0": (144, 409, 0, 6, 0, 30786325577728),
        "test_forward auto dbg262144": (80, 409, 0, 6, 0, 65970697666560), "test_forward q16 dbg0": (80, 409, 0, 6, 0, 3932160),
        "test_forward q16 dbg262144": (80, 409, 0, 6, 0, 3932160), "test_forward u16 dbg0": (144, 409, 0, 6, 0, 1924145348608),
        "test_forward u16 dbg262144": (80, 409, 0, 6, 0, 17182752768), "vanilla": (129, 129, 0, 1, 0),
    },
}


def check(name, got):
    want = EXPECTED[name]
    for key in sorted(got):
        print(f"{name}: {key}: {got[key]}")
    assert sorted(got) == sorted(want), f"{name}: the cases differ from the table's"
    wrong = {k: (got[k], want[k]) for k in got if tuple(got[k]) != tuple(want[k])}
    assert not wrong, f"{name}: (got, recorded) {FIELDS} differ for {len(wrong)} decodes: {wrong}"


@pytest.mark.parametrize("csr", [False, True], ids=["dense", "csr"])
def test_every_kernel_forked_and_serial(csr):
    name = "matrix-csr" if csr else "matrix-dense"
    got = measure_matrix(csr)
    check(name, got)
    # the shape reaches what it is here for: last columns (bit 3 moves them into full steps), the batch limit, the flat
    # form and, for the packed kernel, a forked generation (bit 18 changes the launches)
    any_kernel = "auto" if csr else "q16"
    assert got[f"{any_kernel} b8 flat0 dbg0"][2] > 0 and got[f"{any_kernel} b8 flat0 dbg{1 << 3}"][2] == 0
    assert got[f"{any_kernel} b8 flat0 dbg0"][0] < got[f"{any_kernel} b3 flat0 dbg0"][0] < got[f"{any_kernel} b1 flat0 dbg0"][0]
    assert got[f"{any_kernel} b8 flat2 dbg0"][4] > 0 and got[f"{any_kernel} b8 flat0 dbg0"][4] == 0
    if not csr:
        assert got["u16 b8 flat0 dbg0"][0] != got[f"u16 b8 flat0 dbg{1 << 18}"][0]


def test_fork_threshold():
    got = measure_fork_threshold()
    check("fork", got)
    for case in ("dense u16 T330 n4", "dense u16 T330 n16", "dense sparse T330 n4", "csr auto T330 n4", "csr auto T530 n4",
                 "csr csr64 T530 n4"):
        assert got[f"{case} flat0 dbg0"][0] != got[f"{case} flat0 dbg{1 << 18}"][0], case
    # passes shorter than 64 steps: the walks stay on one stream
    assert got["csr auto T530 n16 flat0 dbg0"] == got[f"csr auto T530 n16 flat0 dbg{1 << 18}"]


@pytest.mark.parametrize("K", LDS_KS)
def test_lds_batch_limit_boundaries(K):
    check(f"lds-{K}", measure_lds_boundary(K))


def test_entry_points():
    got = measure_entry_points()
    check("entry", got)
    assert got["batch6 u16 dbg0"][0] != got[f"batch6 u16 dbg{1 << 28}"][0]
    assert got["test_forward u16 dbg0"] != got[f"test_forward u16 dbg{1 << 18}"]
