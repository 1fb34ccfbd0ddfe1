"""fv_loglik / fv_loglik_batch / fv_posteriors / fv_last_sumprod_stats and the hook fv_test_sumprod_rows without a GPU: all
are exported and listed, the prototypes of the headers are the documented ones and stand after fv_last_lag_stats,
decoder.SumprodStats mirrors fv_sumprod_stats member for member, the wrappers have the documented signatures, a NULL
context answers FV_ERR_ARG, and the header states the three guarantees and the refusals."""
import ctypes
import inspect
import os
import re

from conftest import ROOT
from flash_viterbi_amd import decoder

NAMES = ("fv_loglik", "fv_loglik_batch", "fv_posteriors", "fv_last_sumprod_stats")
HOOK = "fv_test_sumprod_rows"


def header(name="flashvit.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def test_library_exports_the_functions():
    lib = decoder.load_library()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in decoder.EXPORTS and name not in decoder.TEST_EXPORTS
    assert hasattr(lib, HOOK) and HOOK in decoder.TEST_EXPORTS and HOOK not in decoder.EXPORTS
    out = ctypes.c_double(0)
    assert lib.fv_loglik(None, None, 4, ctypes.byref(out)) == decoder.ERR_ARG
    assert lib.fv_loglik_batch(None, None, None, 1, None, None) == decoder.ERR_ARG
    assert lib.fv_posteriors(None, None, 4, None, 0, None, ctypes.byref(out)) == decoder.ERR_ARG
    st = decoder.SumprodStats()
    assert lib.fv_last_sumprod_stats(None, ctypes.byref(st)) == decoder.ERR_ARG
    assert lib.fv_test_sumprod_rows(None, None, 4, None, None) == decoder.ERR_ARG


def test_prototypes_match_the_headers():
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    protos = {m.group(2): (m.group(1), re.sub(r"\s+", " ", m.group(3)).strip())
              for m in re.finditer(r"(\w[\w ]*?)\s+(" + "|".join(NAMES) + r")\s*\(([^)]*)\)\s*;", text)}
    assert protos == {
        "fv_loglik": ("int", "fv_ctx *ctx, const int *ob, int T, double *loglik_out"),
        "fv_loglik_batch": ("int", "fv_ctx *ctx, const int *ob, const long long *offsets, int nseq, double *loglik_out, int *status_out"),
        "fv_posteriors": ("int", "fv_ctx *ctx, const int *ob, int T, float *gamma_out, long long ld, int *path_out, double *loglik_out"),
        "fv_last_sumprod_stats": ("int", "const fv_ctx *ctx, fv_sumprod_stats *out")}
    assert text.index("fv_last_lag_stats") < text.index("fv_loglik") < text.index("fv_sumprod_stats;") < text.index("fv_last_sumprod_stats")
    hook = re.sub(r"/\*.*?\*/", "", header("flashvit_testing.h"), flags=re.S)
    m = re.search(r"int\s+fv_test_sumprod_rows\s*\(([^)]*)\)\s*;", hook)
    assert m and re.sub(r"\s+", " ", m.group(1)).strip() == "fv_ctx *ctx, const int *ob, int T, double *alpha_out, double *beta_out"
    lib = decoder.load_library()
    assert [len(getattr(lib, n).argtypes) for n in NAMES + (HOOK,)] == [4, 6, 7, 2, 5]
    assert lib.fv_posteriors.argtypes[4] is ctypes.c_longlong


def test_sumprod_stats_mirrors_the_header():
    m = re.search(r"typedef struct \{([^}]*)\} fv_sumprod_stats;", header())
    assert m
    members = re.findall(r"\b(double|long long|int)\s+(\w+)\s*;", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    ctype = {"double": ctypes.c_double, "long long": ctypes.c_longlong, "int": ctypes.c_int}
    assert [(n, ctype[t]) for t, n in members] == list(decoder.SumprodStats._fields_)
    assert [n for _, n in members] == ["call_ms", "gpu_ms", "step_launches", "task_steps", "table_bytes_per_step", "device_bytes",
                                       "refine_columns", "refine_finite", "passes", "batch_cap"]
    assert ctypes.sizeof(decoder.SumprodStats) == 9 * 8
    # fv_stats is left alone: its layout is pinned elsewhere, and no member of the new struct went there
    stats = re.search(r"typedef struct \{([^}]*)\} fv_stats;", header()).group(1)
    assert "refine_columns" not in stats and "refine_finite" not in stats


def test_wrapper_signatures():
    F = decoder.FlashViterbi
    p = inspect.signature(F.loglik).parameters
    assert list(p)[1:] == ["ob", "T"] and p["ob"].default is None and p["T"].default is None
    p = inspect.signature(F.loglik_batch).parameters
    assert list(p)[1:] == ["obs", "lengths"] and p["lengths"].default is None
    p = inspect.signature(F.posteriors).parameters
    assert list(p)[1:] == ["ob", "T", "want_gamma", "out"]
    assert (p["ob"].default, p["T"].default, p["want_gamma"].default, p["out"].default) == (None, None, True, None)
    assert list(inspect.signature(F.sumprod_stats).parameters) == ["self"]


def test_the_header_says_the_guarantees_and_the_refusals():
    text = re.sub(r"\s*\n \*\s*", " ", header())
    for phrase in ("1. Accuracy", "2 * (t + 1) * (K + 1024) * u * max(1, Amax)", "derived, not measured",
                   "-inf comes out where, and only where, the exact value is -inf",
                   "2. No flush", "falls below 2^-800", "every float32 model entry", "3. Reproducible bits", "whatever FV_OPT_MAX_BATCH",
                   "has the bits of fv_loglik", "no reduction uses floating-point atomics",
                   "FV_ERR_NO_PRED when loglik is -inf", "path_out is filled with -1", "gamma_out is not written",
                   "a symbol outside [0, M)", "multi-device, partitioned and communicator contexts",
                   "Models set by fv_set_model_sparse are refused", "K > 20192", "FV_ERR_NOMEM, with the byte count",
                   "4 * K^2 bytes each", "Model entries above 1 and emission scores above 0 are accepted",
                   "streaming likelihoods and Baum-Welch accumulators (xi)"):
        assert phrase in text, phrase
