"""CPU: the arithmetic of FV_OPT_ROW_CODES (flash_viterbi_amd/csrc/fv_kernels.hip.inc, the comment block above pk_adds).

The packed 16-bit kernel stages the incoming score row as codes c(k) = rne((Mx - v_k) / step), Mx the row maximum.  On the
row-codes route the producer of a 16-column tile w leaves p(k) = rne((tmax_w - v_k) / step) and tmax_w, and the consumer
stages c'(k) = p(k) (+sat) d_w with d_w = rne((Mx - tmax_w) / step), Mx = max_w tmax_w.  This file restates the three
functions in numpy float32 and checks what the derivation states and the refine window relies on:

  * Mx from the tile maxima is the row maximum, bit for bit;
  * where c'(k) < 65535: |step c'(k) - (Mx - v_k)| <= 1.024 step (two roundings of at most 0.5 + 0.012 each; one rounding,
    today's route, 0.512 step);
  * c'(k) = 65535 only for an unreachable v_k or where (Mx - v_k) / step >= 65534 - 1.024: the unclamped code is >= 65534,
    which is what the saturation guard (thr >= 65535, two units of slack) covers;
  * the two routes never differ by more than two code units.

Rows are drawn over the score magnitudes of T = 16 ... 4200 steps, with unreachable entries, wholly unreachable tiles, pad
columns in the last tile and tiles further below the row maximum than the code range.  The counterpart of
tests/test_slab_merge.py for this change."""
import numpy as np
import pytest

F32 = np.float32
FLT_MAX = np.finfo(np.float32).max
TILE = 16


def score_code(mx, v, inv_step):
    """fv_kernels.hip.inc, score_code: float32 throughout, round to nearest even, 65535 beyond the range or unreachable"""
    mx, v = np.asarray(mx, F32), np.asarray(v, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        q = ((mx - v).astype(F32) * F32(inv_step)).astype(F32)
        ok = (v > F32(-0.5) * FLT_MAX) & (q < F32(65534.5))
        return np.where(ok, np.rint(np.where(ok, q, 0)), 65535).astype(np.int64)


def producer(v, K, inv_step):
    """tile maxima over the real columns (-FLT_MAX: none reachable) and codes relative to them; pads count as unreachable"""
    n = (K + TILE - 1) // TILE * TILE
    x = np.full(n, -FLT_MAX, F32)
    x[:K] = np.where(v[:K] > -FLT_MAX, v[:K], -FLT_MAX)
    tmax = x.reshape(-1, TILE).max(axis=1)
    return score_code(np.repeat(tmax, TILE), x, inv_step), tmax


def consumer(p, tmax, inv_step):
    mx = tmax.max()
    d = score_code(mx, tmax, inv_step)
    return np.minimum(p + np.repeat(d, TILE), 65535), mx, d


def rows(T, K, spread, rs):
    """a score row after about T steps: magnitudes T * (2 .. 6), entries spread over `spread` below the best"""
    base = -T * rs.uniform(2.0, 6.0)
    v = (base - spread * rs.rand(K) ** 2).astype(F32)
    v[rs.rand(K) < 0.1] = -FLT_MAX                                   # unreachable states
    t = rs.randint(0, K // TILE)
    v[t * TILE:(t + 1) * TILE] = -FLT_MAX                            # a wholly unreachable tile
    return v


STEPS = [10.5 / 65534, 36.8 / 65534, 2.0 / 65534]


@pytest.mark.parametrize("T", [16, 64, 256, 1024, 4200])
@pytest.mark.parametrize("step", STEPS)
def test_two_rounding_codes_stay_within_the_stated_bound(T, step):
    rs = np.random.RandomState(T)
    step = F32(step)
    inv = F32(1.0) / step
    K = 777                                                          # the last tile has 7 pad columns
    for spread in (0.5, 8.0, 60.0):
        for _ in range(20):
            v = rows(T, K, spread, rs)
            if spread == 60.0:                                       # a tile further below the maximum than the code range
                t = rs.randint(0, K // TILE)
                v[t * TILE:(t + 1) * TILE] = (v[v > -FLT_MAX].max() - F32(70000.0) * step - rs.rand(TILE)).astype(F32)
            p, tmax = producer(v, K, inv)
            c2, mx, d = consumer(p, tmax, inv)
            live = v > -FLT_MAX
            assert mx == v[live].max() and mx.dtype == np.float32
            c1 = score_code(mx, v, inv)
            c2 = c2[:K]
            assert (p[K:] == 65535).all()
            dist = (np.float64(mx) - v.astype(np.float64)) / np.float64(step)          # exact distance in steps
            assert (c1[~live] == 65535).all() and (c2[~live] == 65535).all()
            in1, in2 = live & (c1 < 65535), live & (c2 < 65535)
            assert np.abs(c1[in1] - dist[in1]).max() <= 0.512
            assert np.abs(c2[in2] - dist[in2]).max() <= 1.024
            sat = live & (c2 == 65535)
            assert (dist[sat] >= 65534 - 1.024).all()
            both = in1 & in2
            assert np.abs(c1[both] - c2[both]).max() <= 2
            if spread == 60.0:
                assert (d == 65535).any() and sat.any()                                # d_w itself saturated


def test_empty_row_and_single_tile():
    inv = F32(1.0) / F32(STEPS[0])
    v = np.full(9, -FLT_MAX, F32)
    p, tmax = producer(v, 9, inv)
    c, mx, d = consumer(p, tmax, inv)
    assert mx == -FLT_MAX and (c == 65535).all() and (d == 65535).all()
    v[3] = F32(-7.25)
    v[5] = F32(-7.5)
    p, tmax = producer(v, 9, inv)
    c, mx, d = consumer(p, tmax, inv)
    assert mx == F32(-7.25) and d.tolist() == [0] and c[3] == 0 and c[5] == int(np.rint(F32(0.25) * inv))
    assert (np.delete(c, [3, 5]) == 65535).all()
