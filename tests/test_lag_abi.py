"""fv_set_max_lag / fv_last_lag_stats without a GPU: both are exported and listed, the prototypes of include/flashvit.h are the
documented ones and stand after fv_streams_last_stats, decoder.LagStats mirrors fv_lag_stats member for member, the wrappers
have the documented signatures, and both answer a NULL context (and fv_set_max_lag a negative bound) with FV_ERR_ARG."""
import ctypes
import inspect
import os
import re

from conftest import ROOT
from flash_viterbi_amd import decoder

NAMES = ("fv_set_max_lag", "fv_last_lag_stats")


def header():
    return open(os.path.join(ROOT, "include", "flashvit.h")).read()


def test_library_exports_the_two_functions():
    lib = decoder.load_library()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in decoder.EXPORTS and name not in decoder.TEST_EXPORTS
    assert lib.fv_set_max_lag(None, 4) == decoder.ERR_ARG and lib.fv_set_max_lag(None, 0) == decoder.ERR_ARG
    assert lib.fv_set_max_lag(None, -1) == decoder.ERR_ARG
    out = decoder.LagStats()
    assert lib.fv_last_lag_stats(None, -1, ctypes.byref(out)) == decoder.ERR_ARG
    assert lib.fv_last_lag_stats(None, 0, None) == decoder.ERR_ARG


def test_prototypes_match_the_header():
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    protos = {m.group(2): (m.group(1), re.sub(r"\s+", " ", m.group(3)).strip())
              for m in re.finditer(r"(\w[\w ]*?)\s+(fv_set_max_lag|fv_last_lag_stats)\s*\(([^)]*)\)\s*;", text)}
    assert protos == {"fv_set_max_lag": ("int", "fv_ctx *ctx, long long max_lag"),
                      "fv_last_lag_stats": ("int", "const fv_ctx *ctx, int slot, fv_lag_stats *out")}
    assert text.index("fv_streams_last_stats") < text.index("fv_set_max_lag") < text.index("fv_lag_stats;") < text.index("fv_last_lag_stats")
    lib = decoder.load_library()
    assert [len(getattr(lib, n).argtypes) for n in NAMES] == [2, 3]
    assert lib.fv_set_max_lag.argtypes[1] is ctypes.c_longlong


def test_lag_stats_mirrors_the_header():
    text = header()
    m = re.search(r"typedef struct \{([^}]*)\} fv_lag_stats;", text)
    assert m and m.group(1).lstrip().startswith("long long max_lag;")
    members = re.findall(r"\b(double|long long|int)\s+(\w+)\s*;", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    ctype = {"double": ctypes.c_double, "long long": ctypes.c_longlong, "int": ctypes.c_int}
    assert [(n, ctype[t]) for t, n in members] == list(decoder.LagStats._fields_)
    assert [n for _, n in members] == ["max_lag", "forced_commits", "pruned_states", "first_forced_time", "last_forced_time"]
    assert ctypes.sizeof(decoder.LagStats) == 5 * 8


def test_wrapper_signatures():
    p = inspect.signature(decoder.FlashViterbi.set_max_lag).parameters
    assert list(p)[1:] == ["max_lag"] and p["max_lag"].default is inspect.Parameter.empty
    p = inspect.signature(decoder.FlashViterbi.lag_stats).parameters
    assert list(p)[1:] == ["slot"] and p["slot"].default is None


def test_the_header_says_what_the_mode_guarantees_and_gives_up():
    text = re.sub(r"\s*\n \*\s*", " ", header())
    for phrase in ("Connected path", "Exact for the pruned model", "Bounded lag", "2 L + C - 2", "What it costs",
                   "no longer the Viterbi path of the whole input", "FV_ERR_NO_PRED where the exact decode finds a path",
                   "No forced commit, nothing changes", "the pair becomes three launches"):
        assert phrase in text, phrase
