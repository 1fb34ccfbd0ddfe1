"""GPU: FV_OPT_FLAT_GENERATIONS — all right-hand generations at once from the whole-sequence chain, a resolver, and the
generation-by-generation decode from the first generation that cannot be committed.

Bar: path and score bit-equal to the goldens and to the same decode with the option off, for every full-state kernel;
the statistics (speculative passes, missed passes, first-miss generation) equal to what the CPU model of the scheme
(tests/flat_model.py, on the oracle's single-pass primitive) computes — on the goldens, where only ties_semi_K96_T80
misses, and under fv_test_flat_poison, which makes any chosen position miss."""
import numpy as np
import pytest

import oracle
from conftest import golden_model, load_goldens
from flash_viterbi_amd import decoder
from flat_model import flat_decode_cpu

pytestmark = pytest.mark.gpu

FLAT = decoder.OPT_FLAT_GENERATIONS
# (how the model is set, FV_OPT_KERNEL, kernel reported): 1 .. 6 on the dense table, 7 and 8 through fv_set_model_sparse
FORMS = [("dense", k, k) for k in (decoder.KERNEL_F64_STREAM, decoder.KERNEL_F32_REFINE, decoder.KERNEL_F16_REFINE,
                                   decoder.KERNEL_Q16_REFINE, decoder.KERNEL_SPARSE_Q16, decoder.KERNEL_U16_REFINE)]
FORMS += [("sparse", decoder.KERNEL_AUTO, decoder.KERNEL_SPARSE_CSR), ("sparse", decoder.KERNEL_CSR_F64, decoder.KERNEL_CSR_F64)]
CASES = [(g, n) for g in load_goldens() for n in sorted({r["N"] for r in g["runs"] if r["algo"] == "flash"})]
CASE_IDS = [f"{g['name']}-N{n}" for g, n in CASES]


@pytest.fixture(scope="module")
def ctxs():
    cache = {}

    def get(g, how="dense"):
        key = (g["name"], how)
        if key not in cache:
            A, B, Pi, ob = golden_model(g)
            fv = decoder.FlashViterbi(0)
            if how == "dense":
                fv.set_model(A, B, Pi)
            else:
                fv.set_model_sparse(*decoder.dense_to_csr(A), B, Pi)
            cache[key] = (fv, ob)
        return cache[key]
    yield get
    for fv, _ in cache.values():
        fv.close()


@pytest.fixture(scope="module")
def model():
    """CPU model of the scheme per (golden, n_split, poisoned position): computed once, shared."""
    cache = {}

    def get(g, n, poison=None):
        key = (g["name"], n, poison)
        if key not in cache:
            A, B, Pi, ob = golden_model(g)
            cache[key] = flat_decode_cpu(oracle.OracleModel(A, B, Pi), ob, n, A.shape[0], poison)
        return cache[key]
    return get


def decode(fv, ob, n, flat):
    fv.set_option(FLAT, flat)
    try:
        path, score, rc = fv.decode_full(ob, n, decoder.MODE_REFERENCE)
    finally:
        fv.set_option(FLAT, decoder.FLAT_AUTO)
    return path.tolist(), score, rc, fv.stats()


@pytest.mark.parametrize("g,n", CASES, ids=CASE_IDS)
def test_every_kernel_matches_golden_and_the_option_off(ctxs, model, g, n):
    ref = next(r for r in g["runs"] if r["algo"] == "flash" and r["N"] == n)
    cpu_path, right_hand, cpu_missed, cpu_first = model(g, n)
    assert cpu_path.tolist() == ref["path"]
    for how, kernel, reported in FORMS:
        fv, ob = ctxs(g, how)
        fv.set_option(decoder.OPT_KERNEL, kernel)
        path, score, rc, st = decode(fv, ob, n, decoder.FLAT_ON)
        print(f"{g['name']} N={n} kernel {reported}: flat passes {st['flat_passes']} missed {st['flat_missed']} first miss {st['flat_first_miss']}")
        assert rc == 0 and path == ref["path"] and score == np.float32(ref["score"]), (how, kernel)
        assert st["kernel"] == reported or (kernel == decoder.KERNEL_SPARSE_Q16 and st["kernel"] == decoder.KERNEL_U16_REFINE)
        assert st["flat_passes"] == right_hand
        assert (st["flat_missed"], st["flat_first_miss"]) == (cpu_missed, cpu_first)
        if g["name"] != "ties_semi_K96_T80":
            assert st["flat_missed"] == 0 and st["flat_first_miss"] == -1 and st["passes"] == right_hand + 1
        elif n in (1, 3, 8):
            assert st["flat_missed"] >= 1 and st["flat_first_miss"] >= 2
        opath, oscore, orc, ost = decode(fv, ob, n, decoder.FLAT_OFF)
        assert (opath, oscore, orc) == (path, score, rc)
        assert (ost["flat_passes"], ost["flat_missed"], ost["flat_first_miss"]) == (0, 0, -1)


def reads(plan):
    """position -> lowest generation of a right-hand pass that is conditioned on it (its L-1 or its R)"""
    first = {}
    for L, R, gen, _ in plan:
        if gen >= 1:
            for t in (L - 1, R):
                first[t] = min(first.get(t, gen), gen)
    return first


@pytest.mark.parametrize("name,n", [("ds_K77_M7_T33", 4), ("ds_K512_T64", 8)])
def test_poisoned_snapshot_misses_where_it_is_read_and_changes_nothing(ctxs, model, name, n):
    """Poison at a generation-1 pass's L-1, at a position only a deepest-generation pass reads, and at one nobody reads:
    first miss in generation 1, in the deepest generation, none.  (At both shapes the R of every deepest-generation pass
    is also the R of its generation-1 ancestor — a right child keeps its parent's R — so the position only the deepest
    generation reads is such a pass's L-1; the deepest pass's R is poisoned as a fourth case and must miss in the lowest
    generation that reads it.)  The expected figures come from the plan and from the CPU model, never from the device."""
    g = next(x for x in load_goldens() if x["name"] == name)
    ref = next(r for r in g["runs"] if r["algo"] == "flash" and r["N"] == n)
    plan = decoder.plan_passes(len(g["ob"]), n)
    first = reads(plan)
    deepest = max(p[2] for p in plan)
    assert deepest >= 2
    t_first = next(p[0] - 1 for p in plan if p[2] == 1)
    t_deep = next(t for p in plan if p[2] == deepest for t in (p[1], p[0] - 1) if first[t] == deepest)
    t_deep_R = next(p[1] for p in plan if p[2] == deepest)
    t_none = next(t for t in range(len(g["ob"])) if t not in first)
    for how, kernel in (("dense", decoder.KERNEL_U16_REFINE), ("dense", decoder.KERNEL_F64_STREAM), ("sparse", decoder.KERNEL_AUTO)):
        fv, ob = ctxs(g, how)
        fv.set_option(decoder.OPT_KERNEL, kernel)
        clean = decode(fv, ob, n, decoder.FLAT_ON)
        assert clean[0] == ref["path"] and clean[3]["flat_first_miss"] == -1
        for t, want in ((t_first, 1), (t_deep, deepest), (t_none, -1), (t_deep_R, first[t_deep_R])):
            fv.test_flat_poison(t)
            try:
                path, score, rc, st = decode(fv, ob, n, decoder.FLAT_ON)
            finally:
                fv.test_flat_poison(-1)
            _, _, cpu_missed, cpu_first = model(g, n, t)
            print(f"{name} poison {t}: first miss {st['flat_first_miss']} missed {st['flat_missed']} passes {st['passes']}")
            assert (path, score, rc) == clean[:3]
            assert st["flat_first_miss"] == want == cpu_first and st["flat_missed"] == cpu_missed
            assert (st["flat_missed"] >= 1) == (want >= 1)
            # the generations from the miss on ran twice
            again = sum(1 for p in plan if want >= 1 and p[2] >= want)
            assert st["passes"] == len(plan) + again
        assert decode(fv, ob, n, decoder.FLAT_ON)[3]["flat_first_miss"] == -1      # cleared


def test_auto_is_off_for_a_small_model_and_on_for_the_bench_model():
    import modelgen
    A, B, Pi, ob = modelgen.model32(dict(kind="data_script", K=64, M=8, T=16, prob=0.3, seed=5))
    fv = decoder.FlashViterbi(0)
    try:
        fv.set_model(A, B, Pi)
        fv.decode_full(ob, 2)
        st = fv.stats()
        assert st["flat_passes"] == 0 and st["device_bytes"] == 86592 + 16      # (the figure tests/test_gpu_device_bytes.py pins: its 86592 + BT_WORD)
        fv.set_option(FLAT, decoder.FLAT_OFF)
        fv.decode_full(ob, 2)
        assert fv.stats()["device_bytes"] == st["device_bytes"]
    finally:
        fv.close()
    g = next(x for x in load_goldens(include_big=True) if x["name"] == "cfg2_K3965_T256")
    ref = next(r for r in g["runs"] if r["algo"] == "flash" and r["N"] == 8)
    A, B, Pi, ob = golden_model(g)
    fv = decoder.FlashViterbi(0)
    try:
        fv.set_model(A, B, Pi)
        fv.set_option(decoder.OPT_KERNEL, decoder.KERNEL_U16_REFINE)
        path, score, rc = fv.decode_full(ob, 8)
        st = fv.stats()
        assert rc == 0 and path.tolist() == ref["path"] and score == np.float32(ref["score"])
        assert st["flat_passes"] == 126 and st["flat_missed"] == 0 and st["flat_first_miss"] == -1
    finally:
        fv.close()


def test_back_to_back_decodes_of_different_length(ctxs):
    """One context, the option on, T = 100 and then T = 33: the workspace grows for the first and is reused (larger than
    needed, holding the first decode's snapshot, chains and pass table) by the second."""
    g = next(x for x in load_goldens() if x["name"] == "ds_K200_T100")
    A, B, Pi, ob = golden_model(g)
    om = oracle.OracleModel(A, B, Pi)
    fv = decoder.FlashViterbi(0)
    try:
        fv.set_model(A, B, Pi)
        for kernel in (decoder.KERNEL_U16_REFINE, decoder.KERNEL_F64_STREAM):
            fv.set_option(decoder.OPT_KERNEL, kernel)
            for T in (100, 33, 100):
                want_path, want_score, _, want_rc = om.full_decode(ob[:T], 5)
                path, score, rc, st = decode(fv, ob[:T], 5, decoder.FLAT_ON)
                assert (path, score, rc) == (want_path.tolist(), want_score, want_rc), (kernel, T)
                assert st["flat_passes"] == len(decoder.plan_passes(T, 5)) - 1 and st["flat_first_miss"] == -1
    finally:
        fv.close()
