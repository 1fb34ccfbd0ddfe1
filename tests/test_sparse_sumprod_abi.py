"""fv_set_sparse_sumprod / fv_test_sumprod_forms without a GPU: both are exported and listed, the prototypes of the headers are
the ones the wrappers call, a NULL context answers FV_ERR_ARG, the Python mirrors of the FV_SPF_* bits equal the header, and the
header states the default, the K rule and the order rule."""
import ctypes
import inspect
import os
import re

from flash_viterbi_amd import decoder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header(name="flashvit.h"):
    with open(os.path.join(ROOT, "include", name)) as f:
        return f.read()


def test_library_exports_the_functions():
    lib = decoder.load_library()
    assert hasattr(lib, "fv_set_sparse_sumprod")
    assert "fv_set_sparse_sumprod" in decoder.EXPORTS and "fv_set_sparse_sumprod" not in decoder.TEST_EXPORTS
    assert hasattr(lib, "fv_test_sumprod_forms")
    assert "fv_test_sumprod_forms" in decoder.TEST_EXPORTS and "fv_test_sumprod_forms" not in decoder.EXPORTS
    for on in (0, 1, 2):
        assert lib.fv_set_sparse_sumprod(None, on) == decoder.ERR_ARG
    mask = ctypes.c_ulonglong(0)
    assert lib.fv_test_sumprod_forms(None, ctypes.byref(mask)) == decoder.ERR_ARG


def test_prototypes_match_the_headers():
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    m = re.search(r"(\w[\w ]*?)\s+fv_set_sparse_sumprod\s*\(([^)]*)\)\s*;", text)
    assert m and (m.group(1), re.sub(r"\s+", " ", m.group(2)).strip()) == ("int", "fv_ctx *ctx, int on")
    assert text.index("fv_last_sumprod_stats") < text.index("fv_set_sparse_sumprod") < text.index("fv_last_stats")
    hook = re.sub(r"/\*.*?\*/", "", header("flashvit_testing.h"), flags=re.S)
    m = re.search(r"int\s+fv_test_sumprod_forms\s*\(([^)]*)\)\s*;", hook)
    assert m and re.sub(r"\s+", " ", m.group(1)).strip() == "const fv_ctx *ctx, unsigned long long *mask_out"
    lib = decoder.load_library()
    assert lib.fv_set_sparse_sumprod.argtypes == [ctypes.c_void_p, ctypes.c_int]
    assert len(lib.fv_test_sumprod_forms.argtypes) == 2


def test_wrapper_signatures():
    F = decoder.FlashViterbi
    assert list(inspect.signature(F.set_sparse_sumprod).parameters) == ["self", "on"]
    assert list(inspect.signature(F.test_sumprod_forms).parameters) == ["self"]


def test_form_bits_mirror_the_header():
    hook = header("flashvit_testing.h")
    shifts = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+FV_SPF_(\w+)_SHIFT\s+(\d+)", hook)}
    assert shifts == {"DENSE": decoder.SPF_DENSE_SHIFT, "CSR_FWD_LDS": decoder.SPF_CSR_FWD_LDS_SHIFT,
                      "CSR_FWD_MEM": decoder.SPF_CSR_FWD_MEM_SHIFT, "CSR_BACK_LDS": decoder.SPF_CSR_BACK_LDS_SHIFT,
                      "CSR_BACK_MEM": decoder.SPF_CSR_BACK_MEM_SHIFT}
    assert re.search(r"#define\s+FV_SPF_FAMILY\(shift\)\s+\(7ull << \(shift\)\)", hook)
    families = [decoder.spf_family(s) for s in sorted(shifts.values())]
    assert sum(families) == (1 << 15) - 1                 # three bits each (NB = 1, 2, 4), no two families share one
    for a in families:
        assert sum(1 for b in families if a & b) == 1


def test_the_header_says_the_default_the_k_rule_and_the_order_rule():
    text = re.sub(r"\s*\n \*\s*", " ", header())
    for phrase in ("on = 0 (the default): such a model is refused",
                   "Any other value: FV_ERR_ARG", "FV_ERR_STATE, as fv_set_option",
                   "kept across fv_set_model and fv_set_model_sparse", "on a model set by fv_set_model it changes nothing",
                   "Multi-device, partitioned and communicator contexts stay refused",
                   "The K <= 20192 limit does not apply to this route: K is bounded by memory",
                   "holds for any K < 2^31", "less than 2^-863",
                   "a task's summation order is a function of the stored table alone",
                   "on whether the score rows were staged in LDS or read from memory",
                   "stored entries equal to 0 change no bit of any result",
                   "refused unless fv_set_sparse_sumprod"):
        assert phrase in text, phrase
