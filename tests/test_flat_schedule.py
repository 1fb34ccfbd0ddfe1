"""CPU: the flat schedule of FV_OPT_FLAT_GENERATIONS (fv_plan_flat, flash_viterbi_amd/csrc/fv_schedule.cpp) and the
speculate / resolve / fall back scheme on the oracle's single-pass primitive.

The scheme must reproduce the golden path of every small golden at every n_split, with no mis-speculated pass anywhere
except on ties_semi_K96_T80, where at least one pass of a generation >= 2 must miss for every n_split: that golden is
what keeps the fall-back from going untested."""
import pytest

import oracle
from conftest import golden_model, load_goldens
from flash_viterbi_amd import decoder
from flat_model import flat_decode_cpu

SHAPES = [(2, 1), (7, 1), (33, 4), (100, 7), (256, 8), (4096, 8)]


@pytest.mark.parametrize("T,N", SHAPES)
@pytest.mark.parametrize("cap,nstreams", [(4, 3), (8, 1), (1, 2)])
def test_flat_plan_shape(T, N, cap, nstreams):
    plan = decoder.plan_passes(T, N)
    flat = decoder.plan_flat(T, N, cap, nstreams)
    # every pass of a generation >= 1 exactly once, in the plan's order
    assert [(f["L"], f["R"], f["generation"]) for f in flat] == [p[:3] for p in plan if p[2] >= 1]
    # chain slots: R - L entries each, disjoint (a prefix sum)
    spans = sorted((f["chain"], f["chain"] + f["R"] - f["L"]) for f in flat)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and (not spans or spans[0][0] == 0)
    # arg rows: generation 1 keeps the rows of its own times (disjoint in time), the others own R - L private rows
    first = sorted((f["L"] + 1, f["R"] + 1) for f in flat if f["generation"] == 1)
    assert all(f["arg_row"] == -1 for f in flat if f["generation"] == 1)
    assert all(a[1] <= b[0] for a, b in zip(first, first[1:]))
    rows = sorted((f["arg_row"], f["arg_row"] + f["R"] - f["L"]) for f in flat if f["generation"] > 1)
    assert all(a[0] >= 0 for a in rows) and all(a[1] <= b[0] for a, b in zip(rows, rows[1:]))
    assert sum(b - a for a, b in rows) == sum(f["R"] - f["L"] for f in flat if f["generation"] > 1)
    # batches: passes of one stream, at most `cap`; one-step passes are column jobs only
    batches = {}
    for f in flat:
        assert 0 <= f["stream"] < nstreams
        assert (f["batch"] < 0) == (f["R"] - f["L"] == 1)
        if f["batch"] >= 0:
            batches.setdefault(f["batch"], []).append(f)
    for members in batches.values():
        assert 1 <= len(members) <= cap
        assert len({m["stream"] for m in members}) == 1
    # the streams carry equal sums of length: they differ by less than the longest batch
    if batches:
        load = [0] * nstreams
        for members in batches.values():
            load[members[0]["stream"]] += max(m["R"] - m["L"] for m in members) - 1
        assert max(load) - min(load) <= max(max(m["R"] - m["L"] for m in ms) - 1 for ms in batches.values())


def test_flat_plan_of_the_bench_shape():
    """T = 256, n_split = 8: 126 right-hand passes, 63 of them one-step; 128 step launches of at most four tasks, the
    longest pass 31 steps; 362 private arg rows."""
    flat = decoder.plan_flat(256, 8, 4, 3)
    lens = [f["R"] - f["L"] for f in flat]
    assert len(flat) == 126 and lens.count(1) == 63 and max(lens) == 31
    batches = {}
    for f in flat:
        if f["batch"] >= 0:
            batches[f["batch"]] = max(batches.get(f["batch"], 0), f["R"] - f["L"])
    assert sum(n - 1 for n in batches.values()) == 128
    assert sum(f["R"] - f["L"] for f in flat if f["generation"] > 1) == 362


def test_flat_plan_rejects_bad_arguments():
    for args in ((1, 1, 4, 3), (16, 8, 4, 3), (64, 2, 0, 3), (64, 2, 4, 0)):
        with pytest.raises(decoder.FlashVitError):
            decoder.plan_flat(*args)


CASES = [(g, n) for g in load_goldens() for n in sorted({r["N"] for r in g["runs"] if r["algo"] == "flash"})]


@pytest.mark.parametrize("g,n", CASES, ids=[f"{g['name']}-N{n}" for g, n in CASES])
def test_speculate_resolve_fall_back_reproduces_the_golden(g, n):
    A, B, Pi, ob = golden_model(g)
    m = oracle.OracleModel(A, B, Pi)
    ans, npasses, missed, first_miss = flat_decode_cpu(m, ob, n, A.shape[0])
    ref = next(r for r in g["runs"] if r["algo"] == "flash" and r["N"] == n)
    assert ans.tolist() == ref["path"]
    assert npasses == len(decoder.plan_passes(len(ob), n)) - 1
    print(f"{g['name']} N={n}: {npasses} passes, first miss in generation {first_miss}, {missed} passes")
    if g["name"] == "ties_semi_K96_T80":
        assert n not in (1, 3, 8) or (missed >= 1 and first_miss >= 2)
    else:
        assert missed == 0 and first_miss == -1


def test_the_fall_back_golden_covers_its_three_splits():
    assert {n for g, n in CASES if g["name"] == "ties_semi_K96_T80"} >= {1, 3, 8}
