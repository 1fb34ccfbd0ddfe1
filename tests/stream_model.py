"""CPU model of the stream's commit rule (include/flashvit.h, fv_stream_*), on an arg table of the
oracle's full_forward: args[j - 1] is the arg row of time j of one pass over the whole sequence from Pi.

Kept besides the arg rows of the uncommitted times: anc[K], the state at the anchor time a on the survivor path of every
state of the current time (a = 0 and anc[s] = s at first; after a step with arg row bp, anc'[s] = anc[bp[s]] where
bp[s] >= 0, else -1).  A check — every check_every steps counted from the check before, and after the last step of every
push — looks at the set V of non-negative anc values:
  one element v   every path that can still be decoded runs through (a, v): the times up to a are committed by a back-track
                  from (a, v), and the anchor moves to the current time t: a = t, anc[s] = s where bp[s] >= 0, else -1;
  none            no state has a predecessor: the stream is dead;
  otherwise       nothing.
A push hands out what its LAST commit committed (that survivor path runs through the earlier ones); a push that ends dead
hands out nothing, and every check of it is still run and counted.  Plain numpy; shared by the CPU test (against the
single-pass path) and the GPU tests, which compare committed counts, pieces, checks and commits with the library's."""
import numpy as np

import backtrack_model as btm


def single_pass_path(row, args):
    """the path of one pass over the sequence: lowest index among the maxima of the last row, serial walk"""
    end = int(np.argmax(row))
    return btm.serial_walk(args.tolist(), 0, len(args), end) + [end]


class Stream:
    """The rule, push by push.  args: int array [T - 1, K]; row: the last score row (for close)."""

    def __init__(self, args, row, check_every):
        self.args = np.asarray(args)
        self.table = self.args.tolist()
        self.row = np.asarray(row)
        self.K = self.row.size
        self.check_every = int(check_every)
        self.anc = np.arange(self.K)
        self.anchor = 0
        self.times = self.committed = 0
        self.since = 0
        self.checks = self.commits = self.bt_restarts = 0
        self.dead = False
        self.lag_max = 0

    def pending(self):
        return self.times - self.committed

    def _walk(self, L, R, end):
        """states of times L .. R of the chain through (R, end), and the retries of the 64-lane walk over it"""
        if R == L:
            return [int(end)]
        chain, restarts = btm.chunk_walk(self.table[L:], 0, R - L, int(end))
        assert chain == btm.serial_walk(self.table[L:], 0, R - L, int(end))
        self.bt_restarts += restarts
        return chain + [int(end)]

    def push(self, n):
        """consumes the next n times; returns the committed piece (a list), or None when the push ends dead"""
        assert not self.dead and n >= 1 and self.times + n <= len(self.args) + 1
        record = None
        for i in range(n):
            j = self.times + i
            if j > 0:
                bp = self.args[j - 1]
                self.anc = np.where(bp >= 0, self.anc[np.maximum(bp, 0)], -1)
                self.since += 1
            if self.since > 0 and (self.since == self.check_every or i == n - 1):
                self.checks += 1
                self.since = 0
                V = np.unique(self.anc[self.anc >= 0])
                if V.size == 0:
                    self.dead = True
                elif V.size == 1:
                    assert self.anchor >= self.committed         # the anchor always lies beyond the last committed time
                    record = (self.anchor, int(V[0]))
                    self.commits += 1
                    self.anchor = j
                    self.anc = np.where(bp >= 0, np.arange(self.K), -1)
        self.times += n
        if self.dead:
            return None
        piece = []
        if record is not None:
            piece = self._walk(self.committed, record[0], record[1])
            self.committed = record[0] + 1
        self.lag_max = max(self.lag_max, self.pending())
        return piece

    def close(self):
        """the end pick on the last row and the back-track of everything pending (the sequence must have been consumed whole)"""
        assert not self.dead and self.times == len(self.args) + 1
        piece = self._walk(self.committed, self.times - 1, int(np.argmax(self.row)))
        self.committed = self.times
        return piece


def run(args, row, check_every, chunks):
    """The whole sequence in pushes of the lengths `chunks` (they add up to T) and a close.  Returns a dict: pieces (one
    list per push, then the close's), committed (the count after every push), checks, commits, bt_restarts, lag_max, and
    dead = the index of the push that ended dead (None: none; nothing is pushed or closed after it)."""
    s = Stream(args, row, check_every)
    out = dict(pieces=[], committed=[], dead=None)
    for q, n in enumerate(chunks):
        piece = s.push(n)
        if piece is None:
            out["dead"] = q
            out["committed"].append(s.committed)
            break
        out["pieces"].append(piece)
        out["committed"].append(s.committed)
    if out["dead"] is None:
        out["pieces"].append(s.close())
    out.update(checks=s.checks, commits=s.commits, bt_restarts=s.bt_restarts, lag_max=s.lag_max)
    return out


def chunkings(T):
    """the chunkings every case is run through: pushes of 1, 7, 64 and T, and a ragged list that has a first push of
    exactly 1 and a push of 17 — one step beyond a check for check_every = 4 and 16"""
    def even(n):
        return [n] * (T // n) + ([T % n] if T % n else [])
    ragged, left, k = [1], T - 1, 0
    for n in (17, 3, 1, 30, 2, 65, 9):
        if left <= 0:
            break
        ragged.append(min(n, left))
        left -= ragged[-1]
    while left > 0:
        ragged.append(min((17, 5, 33, 1)[k % 4], left))
        left -= ragged[-1]
        k += 1
    return {"1": even(1), "7": even(7), "64": even(64), "T": [T], "ragged": ragged}
