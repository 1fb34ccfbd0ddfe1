"""CPU: tests/backtrack_model.py — the restatement of the 64-lane back-track (backtrack_walk, beam_end_backtrack) — gives
the serial walk's chain on tables built to make it retry, and its retry count on the pure rotor is the one the scheme's
arithmetic predicts.

Tables: a rotor (every state has one predecessor, no two chains ever merge: every guess that did not start from the truth
is wrong), a rotor with 3 % random jumps into three states (chains merge slowly: some chunks stand, some do not), and
both with rows of -1 (a dead chain stays dead).  Lengths on both sides of BT_MIN_PARALLEL, of a change of chunk size
(191 .. 193: 3 -> 4 times per chunk; 2047 .. 2049: 32 -> 33, the warm-up's length) and the longest the GPU tests use."""
import numpy as np
import pytest

import backtrack_model as btm

LENGTHS = (127, 128, 129, 191, 192, 193, 2047, 2048, 2049, 4160)
# pure rotor: retries by length (derived in rotor_restarts below, not measured)
ROTOR_RESTARTS = {127: 0, 128: 3, 129: 3, 193: 5, 2048: 31, 2049: 62, 4160: 63}


def rotor(K, n):
    """bp[j][i] = (i - 1) mod K for n times"""
    return [[(i - 1) % K for i in range(K)]] * n


def rotor_restarts(n):
    """Retries of the scheme on a table without merges.  A lane is right only if its walk started at top(base), from the
    true state: chunks base .. base + BT_WARMUP // cs.  The next one fails and becomes the base, so every retry moves the
    base by BT_WARMUP // cs + 1 chunks until the last non-empty chunk is within reach.  (A guess could also be right by
    accident, if the distance it is off by were a multiple of K: the first failing lane is off by at most cs <= 65 states
    after its BT_WARMUP steps, never by a multiple of 61 or 257 other than 0.)"""
    if n < btm.BT_MIN_PARALLEL:
        return 0
    cs = (n + 63) // 64
    chunks = (n + cs - 1) // cs
    return (chunks - 1) // (btm.BT_WARMUP // cs + 1)


def test_constants_are_the_headers():
    assert (btm.BT_WARMUP, btm.BT_MIN_PARALLEL) == (32, 128) and btm.LANES == 64


@pytest.mark.parametrize("K", [61, 257])
@pytest.mark.parametrize("n", LENGTHS)
def test_chunk_walk_equals_serial_walk(K, n):
    rs = np.random.RandomState(1000 * K + n)
    rot = rotor(K, n)
    # 3 % of the cells jump into states 0 .. 2
    slow = np.asarray(rot)
    jump = rs.rand(n, K) < 0.03
    slow = np.where(jump, rs.randint(0, 3, (n, K)), slow)
    # a row of -1 in the middle: everything below it is dead; and scattered -1 cells
    dead_row = np.asarray(rot).copy()
    dead_row[n // 2, :] = -1
    dead_cells = np.where(rs.rand(n, K) < 0.002, -1, slow)
    seen = {}
    for name, table in (("rotor", rot), ("slow", slow.tolist()), ("dead_row", dead_row.tolist()), ("dead_cells", dead_cells.tolist())):
        for L, end in ((0, 5), (7, K - 1)):
            # (L > 0: the table's first row is the arg row of time L + 1, as the kernels pass it)
            want = btm.serial_walk(table, L, L + n, end)
            got, restarts = btm.chunk_walk(table, L, L + n, end)
            assert got == want, (name, L, end)
            assert (restarts == 0) == (n < btm.BT_MIN_PARALLEL) or name != "rotor"
            seen[name, L] = restarts
    print(f"K {K} len {n}: restarts {seen}")
    assert seen["rotor", 0] == seen["rotor", 7] == rotor_restarts(n)
    if n in ROTOR_RESTARTS:
        assert seen["rotor", 0] == ROTOR_RESTARTS[n]
    if n >= btm.BT_MIN_PARALLEL:
        assert -1 in btm.serial_walk(dead_row.tolist(), 0, n, 5)          # the walk did meet the dead row


def test_rotor_restarts_table_is_the_formula():
    assert {n: rotor_restarts(n) for n in ROTOR_RESTARTS} == ROTOR_RESTARTS


def test_tags_count_on_verified_chunks_only():
    """the beam form of the walk: same chain, same retries; a tagged cell on the true chain counts, one that only a wrong
    guess runs through does not"""
    K, n = 61, 193
    table = rotor(K, n)
    want, restarts = btm.chunk_walk(table, 0, n, 5)
    true_cells = [(j, st) for j, st in zip(range(1, n + 1), want[1:] + [5])]          # (time j, state at time j): the hop reads bp[j][state]
    for tagged, on_path in (({true_cells[40]}, True), ({(true_cells[40][0], (true_cells[40][1] + 1) % K)}, False), (set(), False)):
        got, r, met, anywhere = btm.chunk_walk_tags(table, 0, n, 5, tagged)
        assert (got, r, met) == (want, restarts, on_path) and anywhere >= met
    # every state of every time tagged: wrong guesses meet tags too
    everywhere = {(j, k) for j in range(1, n + 1) for k in range(K)}
    assert btm.chunk_walk_tags(table, 0, n, 5, everywhere)[2:] == (True, True)
    # short chains: one lane, the true chain only
    short = rotor(K, 100)
    chain = btm.serial_walk(short, 0, 100, 7)
    assert btm.chunk_walk_tags(short, 0, 100, 7, {(100, 7)}) == (chain, 0, True, True)
    assert btm.chunk_walk_tags(short, 0, 100, 7, {(100, 8)}) == (chain, 0, False, False)


def test_merged_chains_need_no_retry():
    """every column's predecessor is state 3: all guesses are right after one step"""
    table = [[3] * 17] * 1000
    got, restarts = btm.chunk_walk(table, 0, 1000, 9)
    assert got == [3] * 1000 and restarts == 0
