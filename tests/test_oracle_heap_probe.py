"""CPU: oracle.state_heap (fvo_state_heap_probe: the oracle's heap_reset / heap_offer / heap_build / heap_replace_min)
against the pure-Python state_heap of tests/test_replay_safe_lemma.py.

Two independent restatements of generate_state_heap (reference src/FLASH_BS_Viterbi_multithread.c:96-211); the C one is
the reference of tests/test_gpu_select_tables.py.  The heaps must agree slot for slot, values as bit patterns: rows with
few distinct values (which duplicate of the cut survives, and where, depends on the whole push history) and rows holding
the two "never chosen" values -FLT_MAX and -inf."""
import numpy as np
import pytest

import oracle
from test_replay_safe_lemma import state_heap

FLT_MAX = np.finfo(np.float32).max


def same(row, beam):
    row = np.ascontiguousarray(row, dtype=np.float32)
    want = state_heap([np.float32(v) for v in row], beam)
    hval, hstate = oracle.state_heap(row, beam)
    assert hval.dtype == np.float32 and hval.shape == (beam,) and hstate.shape == (beam,)
    wv = np.array([w[0] for w in want], dtype=np.float32)
    ws = [w[1] for w in want]
    assert hstate.tolist() == ws, f"K={row.size} beam={beam}: states differ"
    assert np.array_equal(hval.view(np.uint32), wv.view(np.uint32)), f"K={row.size} beam={beam}: values differ"


@pytest.mark.parametrize("seed", range(20))
def test_rows_with_few_distinct_values(seed):
    rs = np.random.RandomState(seed)
    for K in sorted({2, 3, 400} | set(rs.randint(2, 401, 12).tolist())):
        levels = int(rs.randint(1, 9))
        row = (-11700.0 + rs.randint(0, levels, K)).astype(np.float32)
        for beam in sorted({2, K} | set(rs.randint(2, K + 1, 4).tolist())):
            same(row, beam)


@pytest.mark.parametrize("seed", range(10))
def test_rows_holding_the_never_chosen_values(seed):
    rs = np.random.RandomState(100 + seed)
    for K in (2, 5, 64, 65, 257, 400):
        kinds = rs.randint(0, 4, K)              # real, -FLT_MAX, -inf, real
        row = np.where(kinds == 1, -FLT_MAX, np.where(kinds == 2, -np.inf, -rs.randint(1, 6, K))).astype(np.float32)
        nreal = int(np.count_nonzero(row > -FLT_MAX))
        for beam in sorted({2, K, max(2, min(K, nreal)), max(2, min(K, nreal + 1)), max(2, nreal - 1)}):
            same(row, beam)
    same(np.full(9, -np.inf, np.float32), 4)
    same(np.full(9, -FLT_MAX, np.float32), 9)
    same(np.array([-np.inf, -FLT_MAX] * 8, np.float32), 5)


def test_refusals():
    with pytest.raises(oracle.OracleError):
        oracle.state_heap(np.zeros(4, np.float32), 5)
    with pytest.raises(oracle.OracleError):
        oracle.state_heap(np.zeros(4, np.float32), 0)
