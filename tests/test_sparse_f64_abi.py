"""FV_KERNEL_CSR_F64 without a GPU: the Python mirrors of the kernel value and of the FV_TV_CSR64_* instantiation bits
equal the header text, and the neighbouring values are what the headers say they are."""
import os
import re

from conftest import ROOT
from flash_viterbi_amd import decoder

INCLUDE = os.path.join(ROOT, "include")


def header(name):
    return open(os.path.join(INCLUDE, name)).read()


def test_kernel_value_mirrors_the_header():
    text = header("flashvit.h")
    values = {n: int(v) for n, v in re.findall(r"\b(FV_KERNEL_[A-Z0-9_]+)\s*=\s*(\d+)", text)}
    assert values["FV_KERNEL_CSR_F64"] == decoder.KERNEL_CSR_F64 == 8
    assert values["FV_KERNEL_SPARSE_CSR"] == decoder.KERNEL_SPARSE_CSR == 7
    assert sorted(values.values()) == list(range(9))              # no value twice, none left out
    assert max(values.values()) == decoder.KERNEL_CSR_F64


def test_instantiation_bits_mirror_the_header():
    text = header("flashvit_testing.h")
    shift64 = int(re.search(r"#define\s+FV_TV_CSR64_SHIFT\s+(\d+)", text).group(1))
    bits = {n: shift64 + int(q) for n, q in re.findall(r"#define\s+(FV_TV_CSR64_[A-Z0-9]+)\s+\(1ull\s*<<\s*\(FV_TV_CSR64_SHIFT\s*\+\s*(\d+)\)\)", text)}
    assert bits == {"FV_TV_CSR64_NB1": 58, "FV_TV_CSR64_NB2": 59, "FV_TV_CSR64_NB4": 60, "FV_TV_CSR64_NB8": 61, "FV_TV_CSR64_MEM": 62}
    assert decoder.TV_CSR64_NB == tuple(1 << bits[f"FV_TV_CSR64_NB{nb}"] for nb in (1, 2, 4, 8))
    assert decoder.TV_CSR64_MEM == 1 << bits["FV_TV_CSR64_MEM"]
    # no other FV_TV_* bit of the header shares a position with them
    shift = int(re.search(r"#define\s+FV_TV_CSR_SHIFT\s+(\d+)", text).group(1))
    others = [int(b) for n, b in re.findall(r"#define\s+(FV_TV_[A-Z0-9_]+)\s+\(1ull\s*<<\s*(\d+)\)", text) if not n.startswith("FV_TV_CSR64_")]
    others += [shift + int(q) for q in re.findall(r"\(1ull\s*<<\s*\(FV_TV_CSR_SHIFT\s*\+\s*(\d+)\)\)", text)]
    assert len(others) == 58 and sorted(others) == list(range(58))
