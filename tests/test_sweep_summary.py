"""CPU: the lane summary of the packed step kernel (trellis_step_u16), restated both ways.

A lane of the kernel sees its share of one column as row blocks of 8 rows, four (even, odd) pairs each, and 16-bit sums
z = score code + table code (saturating at 65535).  The refine needs of it: the smallest z (m1), where it is (block a1, row
parity par, then the row inside the block), and whether a SECOND cell has z <= thr — then the lane's rows are re-walked
(kind 2), otherwise the one cell is evaluated (kind 1), or nothing is (kind 0).

  old_summary   what the sweep used to keep: the exact smallest and second smallest z per parity half, every cell visited;
  new_summary   what it keeps now: per half the smallest and second smallest BLOCK MINIMUM (m2'), and the second smallest of
                the located block's own half from `locate`, which decodes that block anyway.

Both give the same (kind, located row) for every threshold: in the form that folds locate's value into m2 before the kinds
are decided (the kernel's SPEC path) and in the form that decides from m2' first and turns a candidate lane into kind 2
behind locate (the other path).  The derivation stands above pk_adds in fv_kernels.hip.inc; this file is the check of it."""
import itertools

import numpy as np

SAT = 65535


def halves(z):
    """z: [blocks, 8] -> [blocks, 2, 4]: per block the four even rows, then the four odd rows"""
    return np.stack([z[:, 0::2], z[:, 1::2]], axis=1)


def first_block_of_min(bm):
    """per half: the block at which the running minimum last improved strictly (-1: never left 65535)"""
    out = []
    for h in range(2):
        m, a = SAT, -1
        for j, v in enumerate(bm[:, h]):
            if v < m:
                m, a = int(v), j
        out.append(a)
    return out


def two_smallest(v):
    s = np.sort(np.concatenate([np.asarray(v, dtype=np.int64).ravel(), [SAT, SAT]]))
    return int(s[0]), int(s[1])


def locate(z, blk, par, m1):
    """the kernel's locate: lowest pair of block blk whose z of half par equals m1 (the block's first row of that parity if none
    does), and the second smallest of that half's four z, equal sums counted twice"""
    zh = halves(z)[blk, par]
    hit = np.nonzero(zh == m1)[0]
    row = blk * 8 + 2 * (int(hit[0]) if hit.size else 0) + par
    return row, two_smallest(zh)[1]


def head(z, m1p, m2p):
    lo, hi = m1p
    par = 1 if hi < lo else 0
    a = first_block_of_min(halves(z).min(axis=2))
    return par, (hi if par else lo), a[par], min(max(lo, hi), m2p[0], m2p[1])


def old_summary(z):
    zh = halves(z)
    pairs = [two_smallest(zh[:, h]) for h in range(2)]
    par, m1, a1, m2 = head(z, [p[0] for p in pairs], [p[1] for p in pairs])
    return par, m1, a1, m2


def old_kind(s, thr):
    par, m1, a1, m2, row = s
    if thr >= SAT or m2 <= thr:
        return 2, None
    if m1 <= thr and a1 >= 0:
        return 1, row
    return 0, None


def new_summary(z):
    bm = halves(z).min(axis=2)                                   # [blocks, 2] block minima
    pairs = [two_smallest(bm[:, h]) for h in range(2)]
    return head(z, [p[0] for p in pairs], [p[1] for p in pairs])   # m2 here is m2'


def new_kind_folded(s, thr):
    """locate before the kinds are decided: its second smallest goes into m2 (only where the lane has a block)"""
    par, m1, a1, m2, row, second = s
    if a1 >= 0:
        m2 = min(m2, second)
    if thr >= SAT or m2 <= thr:
        return 2, None
    if m1 <= thr and a1 >= 0:
        return 1, row
    return 0, None


def new_kind_behind(s, thr):
    """kinds from m2' first; a candidate lane becomes kind 2 behind locate"""
    par, m1, a1, m2, row, second = s
    if thr >= SAT or m2 <= thr:
        return 2, None
    if m1 <= thr and a1 >= 0:
        return (2, None) if second <= thr else (1, row)
    return 0, None


def summaries(z):
    """(old, new) with what locate gives for the lane's block (None where the lane has none: a1 = -1)"""
    z = np.asarray(z, dtype=np.int64).reshape(-1, 8)
    o, n = old_summary(z), new_summary(z)
    row_o = locate(z, o[2], o[0], o[1])[0] if o[2] >= 0 else None
    row_n, second = locate(z, n[2], n[0], n[1]) if n[2] >= 0 else (None, None)
    return o + (row_o,), n + (row_n, second)


def thresholds(z, m1):
    """every value of the lane near its smallest (further up every kind is 2 long since), and the ends of the code range"""
    v = np.unique(z).astype(np.int64)[:6]
    return sorted({int(t) for t in np.concatenate([v - 1, v, v + 1, [0, m1 + 3, SAT - 1, SAT, SAT + 5]]) if t >= 0})


def check(z):
    o, n = summaries(z)
    ts = thresholds(z, o[1])
    for thr in ts:
        want = old_kind(o, thr)
        assert new_kind_folded(n, thr) == want, (np.asarray(z).tolist(), thr, want, n)
        assert new_kind_behind(n, thr) == want, (np.asarray(z).tolist(), thr, want, n)
    return len(ts)


def test_old_summary_is_the_two_smallest_cells():
    """the restatement of the old sweep against the definition: m1, m2 = the two smallest z of the lane, a tie counted twice"""
    rs = np.random.RandomState(1)
    for _ in range(300):
        z = rs.randint(0, 40, (rs.randint(1, 5), 8))
        par, m1, a1, m2 = old_summary(z)
        assert (m1, m2) == two_smallest(z)
        assert z[a1, par::2].min() == m1 and (a1 == 0 or halves(z)[:a1, par].min() > m1)


def test_random_lanes():
    rs = np.random.RandomState(2)
    cases = 0
    for i in range(1500):
        blocks = rs.randint(1, 7)
        spread = (3, 12, 200, 60000)[i % 4]              # narrow ranges: ties everywhere
        z = rs.randint(0, spread, (blocks, 8)) + rs.randint(0, SAT - spread)
        if i % 5 == 0:
            z[rs.rand(blocks, 8) < 0.3] = SAT            # saturated sums among them
        cases += check(np.minimum(z, SAT))
    assert cases > 5000


def test_two_small_cells_at_every_relative_position():
    """Four blocks (two trips of a double-buffered sweep): the two smallest cells at every pair of positions — same pair,
    same block-half (rows k and k + 2 / 4 / 6), other parity, next block, other trip — tied, and 1 and 5 apart; the rest
    of the lane far above, or just above the window."""
    rs = np.random.RandomState(3)
    seen = set()
    for (p, q), (gap, rest) in itertools.product(itertools.combinations(range(32), 2), ((0, 1000), (0, 4), (1, 1000), (5, 4))):
        for first, second in ((p, q), (q, p)):
            z = rs.randint(100 + rest, 100 + rest + 50, 32)
            z[first], z[second] = 100, 100 + gap
            check(z)
            b0, k0, b1, k1 = first // 8, first % 8, second // 8, second % 8
            seen.add("pair" if b0 == b1 and k0 // 2 == k1 // 2 else
                     f"half+{abs(k1 - k0)}" if b0 == b1 and (k0 - k1) % 2 == 0 else
                     "parity" if b0 == b1 else "trip" if b0 // 2 == b1 // 2 else "other trip")
    assert seen == {"pair", "half+2", "half+4", "half+6", "parity", "trip", "other trip"}


def test_three_way_ties_and_whole_lane_ties():
    for blocks in (1, 2, 3):
        check(np.full((blocks, 8), 7))                     # everything ties (uniform models)
        for p, q, r in itertools.combinations(range(blocks * 8), 3):
            if (p + q + r) % 3:
                continue
            z = np.full(blocks * 8, 900)
            z[[p, q, r]] = 5
            check(z)


def test_saturated_lanes():
    """a lane of saturated sums only has no block (a1 = -1): never a candidate, kind 2 only through the guard; one or two live
    cells among saturated ones; the smallest cell at 65534"""
    check(np.full((3, 8), SAT))
    for p in range(16):
        z = np.full(16, SAT)
        z[p] = 65534
        check(z)
        for q in range(16):
            if q != p:
                y = z.copy()
                y[q] = 65530
                check(y)
                y[q] = 65534
                check(y)
    assert new_summary(np.full((2, 8), SAT))[2] == -1 and old_summary(np.full((2, 8), SAT))[2] == -1


def test_lo_equals_hi_rewalks():
    """the even and the odd half tie: parity 0 is taken, m2' = max(lo, hi) = m1, and whenever the smallest is inside the window
    the lane is kind 2 — whatever the blocks hold"""
    rs = np.random.RandomState(5)
    for _ in range(200):
        z = rs.randint(50, 90, (3, 8))
        e, o = rs.randint(0, 12, 2)
        z.reshape(-1)[2 * e], z.reshape(-1)[2 * o + 1] = 20, 20
        par, m1, a1, m2 = new_summary(z)
        assert (par, m1, m2) == (0, 20, 20) and a1 == (2 * e) // 8
        n = summaries(z)[1]
        assert new_kind_behind(n, 20) == (2, None) and new_kind_folded(n, 20) == (2, None) and new_kind_folded(n, 19) == (0, None)
        check(z)
