"""fv_set_emission_map and the 16-bit score types without a GPU: the function is exported and listed in the drop-in
ABI, the two constants equal the header's (a separate enum: the original two-member line stays as it was), and fv_stats
gained no member with them (its one later member, bt_restarts, is listed)."""
import ctypes
import inspect
import os
import re

from conftest import ROOT
from flash_viterbi_amd import decoder


def header():
    return open(os.path.join(ROOT, "include", "flashvit.h")).read()


def test_library_exports_the_map_function():
    lib = decoder.load_library()
    assert hasattr(lib, "fv_set_emission_map")
    assert "fv_set_emission_map" in decoder.EXPORTS and "fv_set_emission_map" not in decoder.TEST_EXPORTS
    assert re.search(r"\bint\s+fv_set_emission_map\s*\(\s*fv_ctx\s*\*\s*ctx\s*,\s*const\s+int\s*\*\s*pdf_of_state\s*,\s*int\s+P\s*\)\s*;", header())


def test_constants_match_the_header():
    assert (decoder.EMIS_LOG_F16, decoder.EMIS_LOG_BF16) == (2, 3)
    m = re.search(r"enum\s*\{\s*FV_EMIS_LOG_F16\s*=\s*(\d+)\s*,\s*FV_EMIS_LOG_BF16\s*=\s*(\d+)\s*\}", header())
    assert m and (int(m.group(1)), int(m.group(2))) == (decoder.EMIS_LOG_F16, decoder.EMIS_LOG_BF16)
    # the enum of the first two types is untouched, character for character
    assert "\nenum { FV_EMIS_LOG_F32 = 0, FV_EMIS_LOG_F64 = 1 };\n" in header()
    assert (decoder.EMIS_LOG_F32, decoder.EMIS_LOG_F64) == (0, 1)


def test_stats_gained_no_member():
    names = [n for n, _ in decoder.Stats._fields_]
    assert names[-3:] == ["set_emissions_ms", "emission_rows", "bt_restarts"]      # (bt_restarts: appended later, for the back-tracks)
    assert dict(decoder.Stats._fields_)["bt_restarts"] is ctypes.c_longlong
    text = header()
    body = re.sub(r"/\*.*?\*/", "", text[text.index("typedef struct {\n    double set_model_ms"):text.index("} fv_stats;")], flags=re.S)
    assert re.findall(r"\b(?:double|long long|int)\s+(\w+)\s*;", body) == names


def test_wrapper_has_the_map_method():
    assert hasattr(decoder.FlashViterbi, "set_emission_map")
    params = inspect.signature(decoder.FlashViterbi.set_emission_map).parameters
    assert list(params) == ["self", "pdf_of_state", "P"] and params["P"].default is None
