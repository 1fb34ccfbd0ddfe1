"""FV_OPT_SPARSE_BEAM without a GPU: the Python mirrors of the option key and of FV_TV_BEAM_CSR equal the header text, the
option keys stay distinct, and the host-only entry points do not depend on the option."""
import os
import re

from conftest import ROOT
from flash_viterbi_amd import decoder

INCLUDE = os.path.join(ROOT, "include")


def header(name):
    return open(os.path.join(INCLUDE, name)).read()


def test_option_key_mirrors_the_header():
    values = {n: int(v) for n, v in re.findall(r"^\s+(FV_OPT_[A-Z0-9_]+)\s*=\s*(\d+),", header("flashvit.h"), re.M)}      # the enumerators
    assert values["FV_OPT_SPARSE_BEAM"] == decoder.OPT_SPARSE_BEAM == 7
    assert len(set(values.values())) == len(values)               # no key twice
    mirrors = {"FV_OPT_KERNEL": decoder.OPT_KERNEL, "FV_OPT_MAX_BATCH": decoder.OPT_MAX_BATCH, "FV_OPT_PROFILE": decoder.OPT_PROFILE,
               "FV_OPT_SEL_MARGIN": decoder.OPT_SEL_MARGIN, "FV_OPT_FLAT_GENERATIONS": decoder.OPT_FLAT_GENERATIONS,
               "FV_OPT_ROW_CODES": decoder.OPT_ROW_CODES, "FV_OPT_SPARSE_BEAM": decoder.OPT_SPARSE_BEAM, "FV_OPT_DEBUG": decoder.OPT_DEBUG}
    assert values == mirrors


def test_step_variant_mirrors_the_header():
    text = header("flashvit_testing.h")
    bit = {n: int(b) for n, b in re.findall(r"#define\s+(FV_TV_BEAM_[A-Z0-9_]+)\s+\(1ull\s*<<\s*(\d+)\)", text)}
    pair = re.search(r"#define\s+FV_TV_BEAM_CSR\s+\((FV_TV_BEAM_\w+)\s*\|\s*(FV_TV_BEAM_\w+)\)", text)
    assert pair and set(pair.groups()) == {"FV_TV_BEAM_W4", "FV_TV_BEAM_W16"}
    assert decoder.TV_BEAM_CSR == (1 << bit["FV_TV_BEAM_W4"]) | (1 << bit["FV_TV_BEAM_W16"])
    # two bits: no single dense instantiation reports it
    assert bin(decoder.TV_BEAM_CSR).count("1") == 2 and all(decoder.TV_BEAM_CSR != 1 << b for b in bit.values())


def test_host_only_entry_points_are_unaffected():
    """The schedules, the memory formulas and the CSR helper take no context: what they return is what they returned."""
    plan = decoder.plan_passes(24, 3)
    assert plan[0][:2] == (0, 23) and len({(p[0], p[1]) for p in plan}) == len(plan)
    assert decoder.plan_passes(24, 3, decoder.MODE_SINGLE_PASS) == [plan[0]]
    batch = decoder.plan_passes_batch([2, 7, 23], 3)
    assert sorted({p[3] for p in batch}) == [0, 1, 2]
    assert decoder.reference_memory_bytes(300, 40, 4, 128) > 0 and decoder.checkpoint_memory_bytes(300, 40) > 0
    import numpy as np
    A = np.array([[0, 0.5, 0.5], [0, 0, 0], [1, 0, 0]], np.float32)
    ip, ix, dt = decoder.dense_to_csr(A)
    assert ip.tolist() == [0, 2, 2, 3] and ix.tolist() == [1, 2, 0] and dt.tolist() == [0.5, 0.5, 1.0]
