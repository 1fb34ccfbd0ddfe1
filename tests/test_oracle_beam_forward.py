"""CPU: oracle.beam_forward (fvo_beam_forward), the table-keeping FLASH-BS pass that tests/test_gpu_beam_tables.py
compares the device's per-step buffers with.

Two pins.  (1) Row by row it equals the chain composed from the two probes tests/test_oracle_heap_probe.py and
tests/test_oracle_blocked.py already hold to the reference: state_heap of a row, beam_step_probe over that heap in both
forms (cell-at-a-time and blocked), state_heap again.  (2) For n_split = 1, back-tracking arg_state from final_state gives
the entries fvo_beam_decode takes from its whole-sequence pass: path[T-1], path[(T-1) >> 1] and the score."""
import numpy as np
import pytest

import modelgen
import oracle

MODELS = [dict(kind="ties_semi", K=100, M=4, T=300, seed=431, prob=0.5, beam=30),
          dict(kind="ties_all", K=96, M=4, T=200, seed=432, prob=0.5, beam=17),
          dict(kind="data_script", K=300, M=20, T=400, seed=433, prob=0.2, beam=50)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def init_row(A, Bm, Pi, o, st):
    """(float)(log X + log B[i][o]) in double, as the oracle's arithmetic contract states it"""
    x = np.log(Pi.astype(np.float64)) if st < 0 else np.log(A[st].astype(np.float64))
    with np.errstate(divide="ignore"):
        return (x + np.log(Bm[:, o].astype(np.float64))).astype(np.float32)


def composed(om, A, Bm, Pi, ob, L, R, st, beam):
    """the same tables from the two probes"""
    K = om.K
    with np.errstate(divide="ignore"):
        row = init_row(A, Bm, Pi, ob[L], st)
    scores, args, hv, hs = [row], [], [], []
    v, s = oracle.state_heap(row, beam)
    hv.append(v); hs.append(s)
    for j in range(L + 1, R + 1):
        scr, arg = om.beam_step_probe(v, s, ob[j], blocked=True)
        scr0, arg0 = om.beam_step_probe(v, s, ob[j], blocked=False)
        assert np.array_equal(bits(scr), bits(scr0)) and np.array_equal(arg, arg0), j
        scores.append(scr)
        args.append(np.where(arg < 0, -1, s[np.maximum(arg, 0)]).astype(np.int32))
        v, s = oracle.state_heap(scr, beam)
        hv.append(v); hs.append(s)
    return np.stack(scores), np.stack(args) if args else np.empty((0, K), np.int32), np.stack(hv), np.stack(hs)


@pytest.fixture(scope="module", params=MODELS, ids=lambda m: m["kind"])
def case(request):
    spec = request.param
    A, Bm, Pi, ob = modelgen.model32(spec)
    om = oracle.OracleModel(A, Bm, Pi)
    yield spec, A, Bm, Pi, ob, om
    om.close()


def test_beam_forward_equals_the_composed_probe_chain(case):
    spec, A, Bm, Pi, ob, om = case
    T, beam, K = spec["T"], spec["beam"], spec["K"]
    # the whole sequence from Pi; a middle pass from a state; a middle pass from Pi (the row after a beam miss); one row
    for L, R, st in ((0, T - 1, -1), (T // 3, T // 3 + 40, 7), (T // 2, T // 2 + 25, -1), (5, 5, K - 1)):
        scores, arg, hval, hstate, fstate, fscore = om.beam_forward(ob, L, R, st, beam)
        ws, wa, wv, wh = composed(om, A, Bm, Pi, ob, L, R, st, beam)
        n = R - L + 1
        assert scores.shape == (n, K) and arg.shape == (n - 1, K) and hval.shape == (n, beam) and hstate.shape == (n, beam)
        for r in range(n):
            assert np.array_equal(bits(scores[r]), bits(ws[r])), (L, R, st, r)
            assert np.array_equal(bits(hval[r]), bits(wv[r])) and np.array_equal(hstate[r], wh[r]), (L, R, st, r)
            if r:
                assert np.array_equal(arg[r - 1], wa[r - 1]), (L, R, st, r)
        # the end pick: slot 1, then slots beam/2+2 .. beam, strict '>'
        pick, best = 0, hval[-1][0]
        for i in range(beam // 2 + 1, beam):
            if hval[-1][i] > best:
                pick, best = i, hval[-1][i]
        assert fstate == hstate[-1][pick] and bits(fscore) == bits(best)


def test_backtrack_of_the_whole_pass_reproduces_beam_decode(case):
    spec, A, Bm, Pi, ob, om = case
    T, beam = spec["T"], spec["beam"]
    path, score, _, rc = om.beam_decode(ob, 1, beam, check=False)
    _, arg, _, _, fstate, fscore = om.beam_forward(ob, 0, T - 1, -1, beam)
    walk = np.empty(T, np.int32)
    walk[T - 1] = fstate
    for t in range(T - 1, 0, -1):
        walk[t - 1] = arg[t - 1][walk[t]]
        assert walk[t - 1] >= 0
    assert rc >= 0
    assert walk[T - 1] == path[T - 1] and walk[(T - 1) >> 1] == path[(T - 1) >> 1]
    assert bits(fscore) == bits(score)


def test_refusals(case):
    spec, A, Bm, Pi, ob, om = case
    for L, R, st, beam in ((3, 2, -1, 4), (-1, 2, -1, 4), (0, spec["T"], -1, 4), (0, 3, spec["K"], 4), (0, 3, -1, 1),
                           (0, 3, -1, spec["K"] + 1)):
        with pytest.raises(oracle.OracleError):
            om.beam_forward(ob, L, R, st, beam)
