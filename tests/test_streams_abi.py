"""fv_streams_* without a GPU: the functions are exported and listed, the prototypes of include/flashvit.h are the documented
ones, decoder.StreamsStats mirrors fv_streams_stats member for member, the wrappers have the documented signatures, every
function answers a NULL context without crashing, and what the set must not touch — the option / error / kernel
enumerators, fv_stats, fv_stream_stats — is as it was."""
import ctypes
import inspect
import os
import re

from conftest import ROOT
from flash_viterbi_amd import decoder

NAMES = ("fv_streams_open", "fv_streams_push", "fv_streams_push_emissions", "fv_streams_pending", "fv_streams_close",
         "fv_streams_abort", "fv_streams_end", "fv_streams_slot_stats", "fv_streams_last_stats")


def header():
    return open(os.path.join(ROOT, "include", "flashvit.h")).read()


def test_library_exports_the_set_functions():
    lib = decoder.load_library()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in decoder.EXPORTS and name not in decoder.TEST_EXPORTS
    assert lib.fv_streams_pending.restype is ctypes.c_longlong
    # without a context every one of them answers, none crashes
    assert lib.fv_streams_pending(None, 0) == -1
    assert lib.fv_streams_open(None, 1, 0, 0) == decoder.ERR_ARG
    assert lib.fv_streams_push(None, None, 1, None, None, None, None, None, None) == decoder.ERR_ARG
    assert lib.fv_streams_push_emissions(None, None, 1, None, 0, None, 1, None, None, None, None) == decoder.ERR_ARG
    assert lib.fv_streams_close(None, 0, None, None, None) == decoder.ERR_ARG
    assert lib.fv_streams_abort(None, 0) == decoder.ERR_ARG and lib.fv_streams_end(None) == decoder.ERR_ARG
    assert lib.fv_streams_slot_stats(None, 0, None) == decoder.ERR_ARG
    assert lib.fv_streams_last_stats(None, None) == decoder.ERR_ARG


def test_prototypes_match_the_header():
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    protos = {m.group(1): re.sub(r"\s+", " ", m.group(2)).strip() for m in re.finditer(r"\b(fv_streams_\w+)\s*\(([^)]*)\)\s*;", text)}
    assert protos == {
        "fv_streams_open": "fv_ctx *ctx, int nslots, long long lag_rows_hint, int check_every",
        "fv_streams_push": "fv_ctx *ctx, const int *ids, int nids, const int *ob, const long long *offsets, "
                           "int *path_out, const long long *path_offsets, long long *committed_out, int *status_out",
        "fv_streams_push_emissions": "fv_ctx *ctx, const int *ids, int nids, const void *scores, int dtype, "
                                     "const long long *offsets, long long ld, "
                                     "int *path_out, const long long *path_offsets, long long *committed_out, int *status_out",
        "fv_streams_pending": "const fv_ctx *ctx, int id",
        "fv_streams_close": "fv_ctx *ctx, int id, int *path_out, long long *n_out, float *score_out",
        "fv_streams_abort": "fv_ctx *ctx, int id",
        "fv_streams_end": "fv_ctx *ctx",
        "fv_streams_slot_stats": "const fv_ctx *ctx, int id, fv_stream_stats *out",
        "fv_streams_last_stats": "const fv_ctx *ctx, fv_streams_stats *out"}
    for name in NAMES:                        # every one returns int, but the pending count
        ret = re.search(r"(\w[\w ]*?)\s+" + name + r"\s*\(", text).group(1)
        assert ret == ("long long" if name == "fv_streams_pending" else "int"), name
    lib = decoder.load_library()
    assert [len(getattr(lib, n).argtypes) for n in NAMES] == [4, 9, 11, 2, 5, 2, 1, 3, 2]


def test_streams_stats_mirrors_the_header():
    text = header()
    m = re.search(r"typedef struct \{([^}]*)\} fv_streams_stats;", text)
    assert m
    ctype = {"double": ctypes.c_double, "long long": ctypes.c_longlong, "int": ctypes.c_int}
    members = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if decl:
            t = re.match(r"(double|long long|int)\s+(.*)", decl)
            members += [(n.strip(), ctype[t.group(1)]) for n in t.group(2).split(",")]
    assert members == list(decoder.StreamsStats._fields_)
    assert [n for n, _ in members] == ["calls", "step_launches", "task_steps", "check_launches", "check_slots", "syncs", "nslots",
                                       "batch_cap", "kernel", "push_ms_total"]
    assert ctypes.sizeof(decoder.StreamsStats) == 6 * 8 + 3 * 4 + 4 + 8          # (one int of padding before the double)


def test_wrapper_signatures():
    names = ("streams_open", "streams_push", "streams_pending", "streams_close", "streams_abort", "streams_end",
             "streams_slot_stats", "streams_stats")
    sig = {n: list(inspect.signature(getattr(decoder.FlashViterbi, n)).parameters)[1:] for n in names}
    assert sig == {"streams_open": ["nslots", "lag_rows_hint", "check_every"], "streams_push": ["ids", "obs", "scores", "ld"],
                   "streams_pending": ["id"], "streams_close": ["id"], "streams_abort": ["id"], "streams_end": [],
                   "streams_slot_stats": ["id"], "streams_stats": []}
    p = inspect.signature(decoder.FlashViterbi.streams_open).parameters
    assert p["lag_rows_hint"].default == 0 and p["check_every"].default == 0 and p["nslots"].default is inspect.Parameter.empty
    p = inspect.signature(decoder.FlashViterbi.streams_push).parameters
    assert p["obs"].default is None and p["scores"].default is None and p["ld"].default is None


def test_the_set_adds_no_option_error_or_kernel_and_leaves_the_statistics_structs_alone():
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    assert sorted(set(re.findall(r"\bFV_OPT_[A-Z0-9_]+", text))) == sorted(
        ["FV_OPT_KERNEL", "FV_OPT_MAX_BATCH", "FV_OPT_PROFILE", "FV_OPT_SEL_MARGIN", "FV_OPT_FLAT_GENERATIONS", "FV_OPT_ROW_CODES",
         "FV_OPT_SPARSE_BEAM", "FV_OPT_DEBUG"])
    assert sorted(set(re.findall(r"\bFV_ERR_[A-Z_]+", text))) == sorted(
        ["FV_ERR_ARG", "FV_ERR_NOMEM", "FV_ERR_NO_PRED", "FV_ERR_DEVICE", "FV_ERR_STATE", "FV_ERR_UNSUPPORTED", "FV_ERR_COMM"])
    assert len(set(re.findall(r"\bFV_KERNEL_[A-Z0-9_]+", text))) == 9
    assert [n for n, _ in decoder.Stats._fields_][-1] == "bt_restarts"
    full = header()
    body = re.sub(r"/\*.*?\*/", "", full[full.index("typedef struct {\n    long long times;"):full.index("} fv_stream_stats;")], flags=re.S)
    assert [n for _, n in re.findall(r"\b(double|long long|int)\s+(\w+)\s*;", body)] == [
        "times", "committed", "pushes", "checks", "commits", "lag_max", "arg_rows_capacity", "regrows", "bt_restarts",
        "push_ms_total", "kernel"] == [n for n, _ in decoder.StreamStats._fields_]
