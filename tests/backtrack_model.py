"""CPU model of the speculative back-track (flash_viterbi_amd/csrc/fv_kernels.hip.inc, backtrack_walk; the same walk
stands in beam_end_backtrack): a chain of at least BT_MIN_PARALLEL steps is cut into 64 chunks of the time axis, lane c
walks chunk c after BT_WARMUP steps above it from a guessed state, a chunk stands only if it entered with the state the
verified chunk above it left with, and the first chunk that fails restarts everything from it down.

Plain Python on an arg table; shared by the CPU test (against the serial walk) and the GPU tests, which compare
fv_stats.bt_restarts with the number of retries counted here on the oracle's arg tables."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LANES = 64


def layout_constants():
    """(BT_WARMUP, BT_MIN_PARALLEL) of csrc/fv_layout.h"""
    text = open(os.path.join(ROOT, "flash_viterbi_amd", "csrc", "fv_layout.h")).read()
    m = re.search(r"constexpr\s+int\s+BT_WARMUP\s*=\s*(\d+)\s*,\s*BT_MIN_PARALLEL\s*=\s*(\d+)\s*;", text)
    assert m, "fv_layout.h: BT_WARMUP / BT_MIN_PARALLEL not found"
    return int(m.group(1)), int(m.group(2))


BT_WARMUP, BT_MIN_PARALLEL = layout_constants()


def hop(bp, L, st, j):
    """state at time j -> state at time j - 1; bp[j - L - 1] is the arg row of time j.  A dead state stays dead."""
    return int(bp[j - L - 1][st]) if st >= 0 else -1


def serial_walk(bp, L, R, end):
    """c[L .. R-1] of the chain that ends in `end` at time R: c[j - 1] = bp[j][c[j]]."""
    out, st = [0] * (R - L), int(end)
    for j in range(R, L, -1):
        st = hop(bp, L, st, j)
        out[j - 1 - L] = st
    return out


def chunk_walk(bp, L, R, end):
    """(chain c[L .. R-1], restarts): the walk as the 64 lanes do it.  restarts = passes through the retry branch; chains
    shorter than BT_MIN_PARALLEL are walked serially by one lane (0 restarts)."""
    n = R - L
    if n < BT_MIN_PARALLEL:
        return serial_walk(bp, L, R, end), 0
    cs = (n + LANES - 1) // LANES                  # times per chunk; chunk c: from time top(c) down to top(c + 1)

    def top(c):
        return max(R - c * cs, L)

    out = [None] * n
    base, exact, restarts = 0, int(end), 0         # chunks below `base` are final; `exact` = state at time top(base)
    while base < LANES and top(base) > L:
        x, y = [-2] * LANES, [-2] * LANES          # state a lane entered its chunk with / left it with
        for lane in range(base, LANES):
            if top(lane) <= L:
                continue                           # an empty trailing chunk
            t_hi, t_lo = top(lane), top(lane + 1)
            t, st = min(top(base), t_hi + BT_WARMUP), exact
            while t > t_hi:
                st = hop(bp, L, st, t)
                t -= 1
            x[lane] = st
            while t > t_lo:
                st = hop(bp, L, st, t)
                out[t - 1 - L] = st
                t -= 1
            y[lane] = st
        bad = [lane for lane in range(LANES)
               if not (lane <= base or top(lane) <= L                          # final already, or empty
                       or min(top(base), top(lane) + BT_WARMUP) == top(base)   # started from the truth
                       or x[lane] == y[lane - 1])]
        if not bad:
            break
        f = bad[0]                                 # everything above chunk f is final
        exact, base, restarts = y[f - 1], f, restarts + 1
    return out, restarts


def chunk_walk_tags(bp, L, R, end, tagged):
    """The walk of beam_end_backtrack: `tagged` holds the cells (time j, state) whose back-pointer is provisional (two beam
    entries attained the cell's maximum).  Returns (chain, restarts, on_path, anywhere): whether a hop inside a VERIFIED
    chunk read a tagged cell — the only ones that count: they are the cells of the true chain — and whether any hop
    inside any chunk did, verified or not (hops of the warm-up above a chunk belong to the chunk above)."""
    n = R - L
    if n < BT_MIN_PARALLEL:
        chain = serial_walk(bp, L, R, end)
        met = any((j, st) in tagged for j, st in zip(range(L + 1, R + 1), chain[1:] + [int(end)]))
        return chain, 0, met, met
    cs = (n + LANES - 1) // LANES

    def top(c):
        return max(R - c * cs, L)

    out = [None] * n
    base, exact, restarts, on_path, anywhere = 0, int(end), 0, False, False
    while base < LANES and top(base) > L:
        x, y, tag = [-2] * LANES, [-2] * LANES, [False] * LANES
        for lane in range(base, LANES):
            if top(lane) <= L:
                continue
            t_hi, t_lo = top(lane), top(lane + 1)
            t, st = min(top(base), t_hi + BT_WARMUP), exact
            while t > t_hi:
                st = hop(bp, L, st, t)
                t -= 1
            x[lane] = st
            while t > t_lo:
                tag[lane] |= (t, st) in tagged
                st = hop(bp, L, st, t)
                out[t - 1 - L] = st
                t -= 1
            y[lane] = st
        bad = [lane for lane in range(LANES)
               if not (lane <= base or top(lane) <= L or min(top(base), top(lane) + BT_WARMUP) == top(base) or x[lane] == y[lane - 1])]
        f = bad[0] if bad else LANES                # chunks base .. f - 1 are final
        on_path |= any(tag[base:f])
        anywhere |= any(tag[base:])
        if not bad:
            break
        exact, base, restarts = y[f - 1], f, restarts + 1
    return out, restarts, on_path, anywhere
