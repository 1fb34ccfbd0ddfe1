"""fv_stream_* without a GPU: the seven functions are exported and listed, decoder.StreamStats mirrors fv_stream_stats of
include/flashvit.h member for member, the wrappers have the documented signatures, and what the stream must not touch —
fv_stats, the option / error / kernel enumerators — is as it was."""
import ctypes
import inspect
import os
import re

from conftest import ROOT
from flash_viterbi_amd import decoder

NAMES = ("fv_stream_open", "fv_stream_push", "fv_stream_push_emissions", "fv_stream_pending", "fv_stream_close",
         "fv_stream_abort", "fv_stream_last_stats")


def header():
    return open(os.path.join(ROOT, "include", "flashvit.h")).read()


def test_library_exports_the_stream_functions():
    lib = decoder.load_library()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in decoder.EXPORTS and name not in decoder.TEST_EXPORTS
    assert lib.fv_stream_pending.restype is ctypes.c_longlong
    # without a context every one of them answers, none crashes
    assert lib.fv_stream_pending(None) == -1
    assert lib.fv_stream_open(None, 0, 0) == decoder.ERR_ARG and lib.fv_stream_abort(None) == decoder.ERR_ARG
    assert lib.fv_stream_close(None, None, None, None) == decoder.ERR_ARG
    assert lib.fv_stream_push(None, None, 1, None, None) == decoder.ERR_ARG
    assert lib.fv_stream_push_emissions(None, None, 0, 1, 1, None, None) == decoder.ERR_ARG
    assert lib.fv_stream_last_stats(None, None) == decoder.ERR_ARG


def test_stream_stats_mirrors_the_header():
    text = header()
    body = re.sub(r"/\*.*?\*/", "", text[text.index("typedef struct {\n    long long times;"):text.index("} fv_stream_stats;")], flags=re.S)
    members = re.findall(r"\b(double|long long|int)\s+(\w+)\s*;", body)
    ctype = {"double": ctypes.c_double, "long long": ctypes.c_longlong, "int": ctypes.c_int}
    assert [(n, ctype[t]) for t, n in members] == list(decoder.StreamStats._fields_)
    assert [n for _, n in members] == ["times", "committed", "pushes", "checks", "commits", "lag_max", "arg_rows_capacity",
                                       "regrows", "bt_restarts", "push_ms_total", "kernel"]


def test_prototypes_match_the_header():
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    protos = {m.group(1): re.sub(r"\s+", " ", m.group(2)).strip() for m in re.finditer(r"\b(fv_stream_\w+)\s*\(([^)]*)\)\s*;", text)}
    assert protos == {
        "fv_stream_open": "fv_ctx *ctx, long long lag_rows_hint, int check_every",
        "fv_stream_push": "fv_ctx *ctx, const int *ob, int n, int *path_out, long long *committed_out",
        "fv_stream_push_emissions": "fv_ctx *ctx, const void *scores, int dtype, int n, long long ld, int *path_out, long long *committed_out",
        "fv_stream_pending": "const fv_ctx *ctx",
        "fv_stream_close": "fv_ctx *ctx, int *path_out, long long *n_out, float *score_out",
        "fv_stream_abort": "fv_ctx *ctx",
        "fv_stream_last_stats": "const fv_ctx *ctx, fv_stream_stats *out"}
    lib = decoder.load_library()
    assert [len(getattr(lib, n).argtypes) for n in NAMES] == [3, 5, 7, 1, 4, 1, 2]


def test_wrapper_signatures():
    sig = {n: list(inspect.signature(getattr(decoder.FlashViterbi, n)).parameters)[1:] for n in
           ("stream_open", "stream_push", "stream_pending", "stream_close", "stream_abort", "stream_stats")}
    assert sig == {"stream_open": ["lag_rows_hint", "check_every"], "stream_push": ["ob", "scores", "ld"], "stream_pending": [],
                   "stream_close": [], "stream_abort": [], "stream_stats": []}
    defaults = inspect.signature(decoder.FlashViterbi.stream_open).parameters
    assert defaults["lag_rows_hint"].default == 0 and defaults["check_every"].default == 0


def test_the_stream_adds_no_option_error_or_kernel_and_leaves_fv_stats_alone():
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    assert sorted(set(re.findall(r"\bFV_OPT_[A-Z0-9_]+", text))) == sorted(
        ["FV_OPT_KERNEL", "FV_OPT_MAX_BATCH", "FV_OPT_PROFILE", "FV_OPT_SEL_MARGIN", "FV_OPT_FLAT_GENERATIONS", "FV_OPT_ROW_CODES",
         "FV_OPT_SPARSE_BEAM", "FV_OPT_DEBUG"])
    assert sorted(set(re.findall(r"\bFV_ERR_[A-Z_]+", text))) == sorted(
        ["FV_ERR_ARG", "FV_ERR_NOMEM", "FV_ERR_NO_PRED", "FV_ERR_DEVICE", "FV_ERR_STATE", "FV_ERR_UNSUPPORTED", "FV_ERR_COMM"])
    assert len(set(re.findall(r"\bFV_KERNEL_[A-Z0-9_]+", text))) == 9
    assert [n for n, _ in decoder.Stats._fields_][-1] == "bt_restarts"
    assert "enum { FV_EMIS_LOG_F32 = 0, FV_EMIS_LOG_F64 = 1 };" in header() and "enum { FV_EMIS_LOG_F16 = 2, FV_EMIS_LOG_BF16 = 3 };" in header()
