"""fv_set_emissions without a GPU: the two functions and the three test hooks (device alloc, device free, the staging kernel timed by device events) are exported and listed, the constants exist,
and decoder.Stats holds the two fields include/flashvit.h appends to fv_stats (only bt_restarts, appended later, follows them)."""
import ctypes
import os
import re

from conftest import ROOT
from flash_viterbi_amd import decoder


def test_library_exports_emission_functions_and_hooks():
    lib = decoder.load_library()
    for name in ("fv_set_emissions", "fv_clear_emissions"):
        assert hasattr(lib, name), name
        assert name in decoder.EXPORTS and name not in decoder.TEST_EXPORTS
    for name in ("fv_test_device_alloc", "fv_test_device_free", "fv_test_stage_emissions_ms"):
        assert hasattr(lib, name), name
        assert name in decoder.TEST_EXPORTS and name not in decoder.EXPORTS
    for method in ("set_emissions", "clear_emissions", "test_device_alloc", "test_device_free", "test_stage_emissions_ms"):
        assert hasattr(decoder.FlashViterbi, method), method


def test_constants_match_the_header():
    assert decoder.EMIS_LOG_F32 == 0 and decoder.EMIS_LOG_F64 == 1
    text = open(os.path.join(ROOT, "include", "flashvit.h")).read()
    m = re.search(r"enum\s*\{\s*FV_EMIS_LOG_F32\s*=\s*(\d+)\s*,\s*FV_EMIS_LOG_F64\s*=\s*(\d+)\s*\}", text)
    assert m and (int(m.group(1)), int(m.group(2))) == (decoder.EMIS_LOG_F32, decoder.EMIS_LOG_F64)


def test_stats_ends_with_the_emission_fields():
    names = [n for n, _ in decoder.Stats._fields_]
    assert names[-3:-1] == ["set_emissions_ms", "emission_rows"]      # (bt_restarts was appended behind them later)
    assert dict(decoder.Stats._fields_)["set_emissions_ms"] is ctypes.c_double
    assert dict(decoder.Stats._fields_)["emission_rows"] is ctypes.c_longlong
    # the same order as the struct of the header: its last two members
    text = open(os.path.join(ROOT, "include", "flashvit.h")).read()
    body = re.sub(r"/\*.*?\*/", "", text[text.index("typedef struct {\n    double set_model_ms"):text.index("} fv_stats;")], flags=re.S)
    members = re.findall(r"\b(?:double|long long|int)\s+(\w+)\s*;", body)
    assert members == names


def test_decodes_take_ob_none_with_a_length():
    import inspect
    for name in ("decode_full", "decode_beam", "decode_vanilla", "decode_checkpoint", "test_forward"):
        assert "T" in inspect.signature(getattr(decoder.FlashViterbi, name)).parameters, name
    for name in ("decode_full_batch", "decode_beam_batch"):
        assert "lengths" in inspect.signature(getattr(decoder.FlashViterbi, name)).parameters, name
