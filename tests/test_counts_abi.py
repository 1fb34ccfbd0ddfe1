"""fv_expected_counts / fv_last_counts_stats without a GPU: both are exported and listed, the prototypes of the header are the
documented ones and stand after fv_set_sparse_sumprod, decoder.CountsStats mirrors fv_counts_stats member for member, the
wrappers have the documented signatures, a NULL context answers FV_ERR_ARG, and the header states G1 - G3 and the refusals."""
import ctypes
import inspect
import os
import re

import numpy as np

from conftest import ROOT
from flash_viterbi_amd import decoder

NAMES = ("fv_expected_counts", "fv_last_counts_stats")


def header():
    return open(os.path.join(ROOT, "include", "flashvit.h")).read()


def test_library_exports_the_functions():
    lib = decoder.load_library()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in decoder.EXPORTS and name not in decoder.TEST_EXPORTS
    assert lib.fv_expected_counts(None, None, None, 1, None, 0, None, None, None, None, None) == decoder.ERR_ARG
    st = decoder.CountsStats()
    assert lib.fv_last_counts_stats(None, ctypes.byref(st)) == decoder.ERR_ARG


def test_prototypes_match_the_header():
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    protos = {m.group(2): (m.group(1), re.sub(r"\s+", " ", m.group(3)).strip())
              for m in re.finditer(r"(\w[\w ]*?)\s+(" + "|".join(NAMES) + r")\s*\(([^)]*)\)\s*;", text)}
    assert protos == {
        "fv_expected_counts": ("int", "fv_ctx *ctx, const int *ob, const long long *offsets, int nseq, double *trans_out, long long ld, "
                                      "double *emit_out, double *init_out, double *occ_out, double *loglik_out, int *status_out"),
        "fv_last_counts_stats": ("int", "const fv_ctx *ctx, fv_counts_stats *out")}
    assert text.index("fv_set_sparse_sumprod") < text.index("fv_expected_counts") < text.index("fv_counts_stats;") \
        < text.index("fv_last_counts_stats") < text.index("fv_last_stats")
    lib = decoder.load_library()
    assert [len(getattr(lib, n).argtypes) for n in NAMES] == [11, 2]
    assert lib.fv_expected_counts.argtypes[5] is ctypes.c_longlong


def test_counts_stats_mirrors_the_header():
    m = re.search(r"typedef struct \{([^}]*)\} fv_counts_stats;", header())
    assert m
    members = re.findall(r"\b(double|long long|int)\s+(\w+)\s*;", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    ctype = {"double": ctypes.c_double, "long long": ctypes.c_longlong, "int": ctypes.c_int}
    assert [(n, ctype[t]) for t, n in members] == list(decoder.CountsStats._fields_)
    assert [n for _, n in members] == ["call_ms", "gpu_ms", "sequences", "dead_sequences", "times", "step_launches", "task_steps",
                                       "xi_launches", "wide_times", "device_bytes"]
    assert ctypes.sizeof(decoder.CountsStats) == 10 * 8
    # the two pinned structs are left alone
    for other in ("fv_stats", "fv_sumprod_stats"):
        body = re.search(r"typedef struct \{([^}]*)\} " + other + ";", header()).group(1)
        assert "xi_launches" not in body and "wide_times" not in body


def test_wrapper_signatures():
    F = decoder.FlashViterbi
    p = inspect.signature(F.expected_counts).parameters
    assert list(p)[1:] == ["obs", "lengths", "want_trans", "trans_out"]
    assert (p["obs"].default, p["lengths"].default, p["want_trans"].default, p["trans_out"].default) == (None, None, True, None)
    assert list(inspect.signature(F.counts_stats).parameters) == ["self"]
    assert list(inspect.signature(decoder.baum_welch_step).parameters) == ["fv", "obs"]


def test_the_m_step_leaves_all_zero_rows_at_zero():
    got = decoder.normalise_rows(np.array([[1.0, 3.0], [0.0, 0.0]]))
    assert got.dtype == np.float64 and got.tolist() == [[0.25, 0.75], [0.0, 0.0]]


def test_the_header_says_the_guarantees_and_the_refusals():
    text = re.sub(r"\s*\n \*\s*", " ", header())
    for phrase in ("G1. Accuracy", "R = 3 * tol(T - 1)", "within R * exact + n * 2^-160", "exactly 0 where A[i][j] == 0",
                   "G2. No flush", "w_t above 500", "e^(-708 + 500) * 2^128 < 2^-171", "Ordinary models have wide_times == 0",
                   "G3. Reproducible bits", "left-to-right float64 sum of the single-sequence calls' outputs", "the first term stands alone",
                   "whatever FV_OPT_MAX_BATCH is", "loglik_out[s] has the bits of fv_loglik", "No floating-point atomics anywhere",
                   "Any output pointer may be NULL", "Outputs are overwritten, not added to", "emit_out must then be NULL",
                   "a sequence of length 1 contributes to init, occ and emit only", "contributes nothing", "ld < K",
                   "a trans_out on another device", "whether or not fv_set_sparse_sumprod is on", "is a follow-up", "K > 20192",
                   "FV_ERR_NOMEM, with the byte count, before anything is allocated",
                   "Model entries above 1 and emission scores above 0 are accepted",
                   "fv_last_sumprod_stats and fv_last_stats keep reporting their own last calls",
                   "sum_ij trans = sum_s (T_s - 1)",
                   # the sentence the earlier block keeps
                   "streaming likelihoods and Baum-Welch accumulators (xi) are not offered either"):
        assert phrase in text, phrase
