"""CPU: the host-side schedule of a batch decode (fv_plan_passes_batch, flash_viterbi_amd/csrc/fv_schedule.cpp).

A batch lays its sequences end to end on one time axis; its plan is the forest of the per-sequence plans, each shifted
to its sequence's offset, generation g of the batch being the union of generation g of every sequence.  Here the
forest is compared pass by pass with fv_plan_passes of every sequence, and executed on the CPU with the oracle's
single-pass primitive (as tests/test_schedule.py does for one sequence): it must reproduce the oracle's decode of every
sequence — which is itself pinned to the reference binaries."""
import ctypes

import numpy as np
import pytest

import oracle
from conftest import golden_model, load_goldens
from flash_viterbi_amd import decoder

LENGTHS = [[256, 64, 17, 2, 300], [5], [33, 33, 33], [2, 2], [7, 100, 3]]


def offsets_of(lengths):
    return [0] + [int(x) for x in np.cumsum(lengths)]


@pytest.mark.parametrize("lengths", LENGTHS, ids=lambda v: "-".join(map(str, v)))
@pytest.mark.parametrize("n_split", [1, 2, 3, 8])
@pytest.mark.parametrize("mode", [decoder.MODE_REFERENCE, decoder.MODE_SINGLE_PASS])
def test_forest_is_the_shifted_plans(lengths, n_split, mode):
    assert not any(T == 2 * n_split and n_split > 2 for T in lengths)
    off = offsets_of(lengths)
    forest = decoder.plan_passes_batch(lengths, n_split, mode)
    gens = [p[2] for p in forest]
    assert gens == sorted(gens), "launch order: sorted by generation"
    for s, T in enumerate(lengths):
        mine = [p for p in forest if p[3] == s]
        single = decoder.plan_passes(T, n_split, mode)
        assert [(L - off[s], R - off[s], g) for L, R, g, _ in mine] == [(L, R, g) for L, R, g, _ in single], (s, T)
        for L, R, g, _ in mine:
            assert off[s] <= L < R <= off[s + 1] - 1
        assert mine[0][:3] == (off[s], off[s + 1] - 1, 0), "pass 0 of a sequence: its whole-sequence pass, generation 0"
        assert all(p[2] > 0 for p in mine[1:])
    assert sorted(set(p[3] for p in forest)) == list(range(len(lengths)))
    # generation 0 holds exactly the whole-sequence passes, in sequence order
    assert [p[3] for p in forest if p[2] == 0] == list(range(len(lengths)))


def run_forest_on_cpu(m, obs, n_split, mode=0):
    """Executes the batch plan generation by generation on the concatenated time axis, with the product's rules: the
    whole-sequence pass of a sequence starts from Pi, every other pass from the answer at L - 1."""
    lengths = [len(o) for o in obs]
    off = offsets_of(lengths)
    ob = np.concatenate([np.asarray(o, dtype=np.int32) for o in obs])
    ans = np.zeros(ob.size, dtype=np.int64)
    forest = decoder.plan_passes_batch(lengths, n_split, mode)
    for g in sorted(set(p[2] for p in forest)):
        for (L, R, gen, s) in [p for p in forest if p[2] == g]:
            seq = ob[off[s]:off[s + 1]]
            whole = g == 0
            if whole:
                assert L == off[s] and R == off[s + 1] - 1
            init = -1 if whole else int(ans[L - 1])
            row, args = m.full_forward(seq, L - off[s], R - off[s], init)
            if whole:
                ans[R] = int(np.argmax(row))          # first maximum = lowest index
            st = int(ans[R])
            for j in range(R, L, -1):
                st = int(args[j - L - 1][st]) if st >= 0 else -1
                ans[j - 1] = st
    return [ans[off[s]:off[s + 1]] for s in range(len(obs))]


GOLDENS = [g for g in load_goldens() if g["name"] in ("ds_K77_M7_T33", "ds_K200_T100", "ds_K9_T7")]


@pytest.mark.parametrize("g", GOLDENS, ids=[g["name"] for g in GOLDENS])
@pytest.mark.parametrize("n_split", [1, 2, 3, 8])
def test_forest_executed_on_cpu_equals_full_decode_of_every_sequence(g, n_split):
    A, B, Pi, ob = golden_model(g)
    M = B.shape[1]
    T = len(ob)
    rs = np.random.RandomState(1000 + n_split)

    def legal(t):
        return t + 1 if (t == 2 * n_split and n_split > 2) else t
    assert legal(T) == T, "no golden has T == 2 * n_split with n_split > 2"
    obs = [rs.randint(0, M, legal(T // 2 + 1)).astype(np.int32), np.asarray(ob, dtype=np.int32),
           rs.randint(0, M, legal(2 * T + 1)).astype(np.int32)]
    m = oracle.OracleModel(A, B, Pi)
    got = run_forest_on_cpu(m, obs, n_split)
    for s, o in enumerate(obs):
        want, _, _, rc = m.full_decode(o, n_split, check=False)
        assert got[s].tolist() == want.tolist(), (s, len(o), rc)
    ref = [r for r in g["runs"] if r["algo"] == "flash" and r["N"] == n_split]
    if ref:
        assert got[1].tolist() == ref[0]["path"]
    m.close()


def test_batch_plan_refusals():
    with pytest.raises(decoder.FlashVitError):
        decoder.plan_passes_batch([10, 1, 10], 1)           # a length of 1
    with pytest.raises(decoder.FlashVitError):
        decoder.plan_passes_batch([10, 8, 10], 4)           # T == 2N, N > 2
    lib = decoder.load_library()
    assert lib.fv_plan_passes_batch(None, 0, 1, 0, None, 0) < 0          # nseq = 0
    lens = np.array([4, 4], dtype=np.int32)
    assert lib.fv_plan_passes_batch(lens.ctypes.data_as(ctypes.c_void_p), 0, 1, 0, None, 0) < 0
    assert lib.fv_plan_passes_batch(lens.ctypes.data_as(ctypes.c_void_p), 2, 0, 0, None, 0) < 0   # n_split = 0
    assert decoder.plan_passes_batch([8], 4, decoder.MODE_SINGLE_PASS) == [(0, 7, 0, 0)]
