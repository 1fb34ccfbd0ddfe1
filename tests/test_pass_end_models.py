"""CPU: the two models of tests/test_gpu_pass_ends.py are what they claim, judged on the oracle's tables alone.

rotor            the 64-lane back-track (tests/backtrack_model.py) retries on the oracle's arg table of one pass over the
                 whole sequence: never at T = 128 (127 steps: one lane walks), at every longer T, and without noise
                 exactly as often as the scheme's arithmetic predicts on a table whose chains never merge.
circulant_ties   every finite score of a row is the same float, the end pick is the lowest live state (after symbol 8 / 9
                 the model's two cuts, after another symbol state 0), every back-pointer on the path the lowest live
                 predecessor, and the tied live predecessors of most path cells lie in more than one block of 64, 256 and
                 1024 states — other waves, other gathers of a thread, other trips of the loop in the kernels that pick."""
import functools

import numpy as np
import pytest

import backtrack_model as btm
import modelgen
import oracle

ROTOR_T = (128, 129, 130, 192, 193, 194, 2049, 2050, 4161)


@functools.lru_cache(maxsize=None)
def rotor_model(K, noise):
    A, Bm, Pi = modelgen.rotor(K, 7, noise, 100 + K)
    return A, Bm, Pi, oracle.OracleModel(A, Bm, Pi)


@functools.lru_cache(maxsize=None)
def circulant_model(K):
    A, Bm, Pi = modelgen.circulant_ties(K)
    return A, Bm, Pi, oracle.OracleModel(A, Bm, Pi)


def observations(M, T, seed):
    return np.random.RandomState(seed).randint(0, M, T).astype(np.int32)


def rotor_formula(n):
    """retries on a table without merges (tests/test_backtrack_model.py derives it)"""
    if n < btm.BT_MIN_PARALLEL:
        return 0
    cs = (n + 63) // 64
    return ((n + cs - 1) // cs - 1) // (btm.BT_WARMUP // cs + 1)


@pytest.mark.parametrize("noise", [0, 0.02, 0.2])
@pytest.mark.parametrize("K", [61, 257])
def test_rotor_makes_the_walk_retry(K, noise):
    A, Bm, Pi, om = rotor_model(K, noise)
    if noise == 0:
        assert ((A > 0).sum(axis=0) == 1).all() and ((A > 0).sum(axis=1) == 1).all()      # one predecessor, one successor
    else:
        assert ((A > 0).sum(axis=1) == 3).all()
    counts = {}
    for T in ROTOR_T:
        ob = observations(7, T, 1000 + T)
        row, args = om.full_forward(ob, 0, T - 1, -1)
        end = int(np.argmax(row))
        table = args.tolist()
        chain, counts[T] = btm.chunk_walk(table, 0, T - 1, end)
        assert chain == btm.serial_walk(table, 0, T - 1, end)
    print(f"rotor K={K} noise={noise}: retries by T {counts}")
    assert counts[128] == 0 and all(counts[T] > 0 for T in ROTOR_T if T > 128)
    if noise == 0:
        assert counts == {T: rotor_formula(T - 1) for T in ROTOR_T}
        assert (counts[129], counts[194], counts[2049], counts[2050], counts[4161]) == (3, 5, 31, 62, 63)


def live_sets(K, Bm, ob):
    """live[t][k]: state k has a finite score at time t of the whole-sequence pass"""
    off = modelgen.CIRCULANT_OFF[K]
    live = np.zeros((len(ob), K), dtype=bool)
    live[0] = Bm[:, ob[0]] > 0
    for t in range(1, len(ob)):
        idx = np.nonzero(live[t - 1])[0]
        nxt = np.zeros(K, dtype=bool)
        for o in off:
            nxt[(idx + o) % K] = True
        live[t] = nxt & (Bm[:, ob[t]] > 0)
    return live


def circulant_facts(K, T, last):
    """The whole pass from the oracle's tables; returns (end state, {block: path cells whose live predecessors lie in more
    than one block of that many states})."""
    A, Bm, Pi, om = circulant_model(K)
    ob = modelgen.circulant_observations(T, last, T)
    live = live_sets(K, Bm, ob)
    row, args = om.full_forward(ob, 0, T - 1, -1)
    finite = row > -np.finfo(np.float32).max
    assert np.array_equal(finite, live[T - 1]) and np.unique(row[finite]).size == 1
    end = int(np.argmax(row))
    assert end == int(np.nonzero(live[T - 1])[0][0])
    path = btm.serial_walk(args.tolist(), 0, T - 1, end) + [end]
    straddle = {64: 0, 256: 0, 1024: 0}
    for t in range(1, T):
        preds = sorted(k for k in ((path[t] - o) % K for o in modelgen.CIRCULANT_OFF[K]) if live[t - 1][k])
        assert preds and path[t - 1] == preds[0], t
        for blk in straddle:
            straddle[blk] += len({k // blk for k in preds}) > 1
    return end, straddle


def check_circulant(K, T, last):
    """Of the T - 1 path cells at least 3/4 have tied live predecessors in more than one 64-block (another wave of
    last_column), at K >= 1025 in more than one 256-block (another of a thread's four gathers) and at K = 2053 in more than
    one 1024-block (another trip of the loop).  K = 257 and K = 1025 have a single state beyond 256 / 1024: there one path
    cell whose predecessors include it is what can be had — the end column after symbol 8, for which the models' offset
    lists hold cut - 256 and cut - 1024 (mod K)."""
    end, straddle = circulant_facts(K, T, last)
    print(f"circulant K={K} T={T} last symbol {last}: end {end}, path cells with predecessors in more than one block {straddle} of {T - 1}")
    if last in (8, 9):
        assert end == modelgen.CIRCULANT_CUT[K][last - 8]
    else:
        assert end == 0
    need = -(-3 * (T - 1) // 4)
    assert straddle[64] >= need
    if K >= 1025:
        assert straddle[256] >= need
    if K == 2053:
        assert straddle[1024] >= need
        assert (end >= 1024) if last == 8 else (256 <= end < 1024) if last == 9 else True
    if last == 8:
        assert straddle[256] >= 1 and (K == 257 or straddle[1024] >= 1)
    return end


@pytest.mark.parametrize("T", [41, 130])
@pytest.mark.parametrize("K", [257, 1025, 2053])
def test_circulant_model_is_what_it_claims(K, T):
    A, Bm, Pi, _ = circulant_model(K)
    assert ((A == 0.125).sum(axis=1) == 8).all() and ((A == 0.125).sum(axis=0) == 8).all() and ((A == 0) | (A == 0.125)).all()
    for last in (8, 9, 3):
        check_circulant(K, T, last)
