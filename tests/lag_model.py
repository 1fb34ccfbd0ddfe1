"""CPU model of the lag-bounded stream (include/flashvit.h, fv_set_max_lag): tests/stream_model.py's loop
with the forced branch, on the oracle's tables.

A symbol stream on (A, B, Pi, ob) is the oracle model (A, B', Pi) with B'[:, t] = B[:, ob[t]], M = T and the observations
0 .. T-1, and pruning the cell (t, s) is B'[s, t] = 0.  At a check at time t that finds more than one ancestor with
t - anchor >= max_lag the model
  * takes the score row of time t from full_forward(ob', 0, t); s* = the lowest index among its maxima, v* = anc[s*];
  * prunes every state whose ancestor is not v* (zeroes those cells of B'), rebuilds the OracleModel and goes on with the
    new arg table, after asserting that the arg rows before t and the survivors' entries of row t did not move (the pruned
    entries of row t keep their old values, as on the device, where the row is never recomputed);
  * records (anchor, v*) like any commit, moves the anchor to t and re-anchors the survivors.
max_lag = 0 is stream_model.Stream.  Plain numpy; shared by the CPU test and tests/test_gpu_stream_lag.py."""
import numpy as np

import backtrack_model as btm
import oracle


def column_model(A, B, Pi, ob):
    """(B', ob'): one emission column per time"""
    ob = np.asarray(ob)
    return np.ascontiguousarray(np.asarray(B, dtype=np.float32)[:, ob]), np.arange(ob.size, dtype=np.int32)


class Stream:
    def __init__(self, A, B, Pi, ob, check_every, max_lag):
        self.A, self.Pi = A, Pi
        self.Bt, self.obt = column_model(A, B, Pi, ob)
        self.T, self.K = self.obt.size, self.Bt.shape[0]
        self.check_every, self.max_lag = int(check_every), int(max_lag)
        # the tables are computed as far as the next check: a forced commit there changes everything behind it.
        # args[j - 1], table[j - 1]: the arg row of time j, valid for j <= upto; row: the score row of time row_time
        self.args = np.full((self.T - 1, self.K), -2, dtype=np.int32)
        self.table = [None] * (self.T - 1)
        self.upto, self.row, self.row_time = 0, None, -1
        self.anc = np.arange(self.K)
        self.anchor = 0
        self.times = self.committed = self.since = 0
        self.checks = self.commits = self.bt_restarts = self.lag_max = 0
        self.dead = False
        self.pruned = np.zeros((self.T, self.K), dtype=bool)       # the cells set to -inf
        self.records = []                                          # every commit: (anchor, state, forced)
        self.forced = []                                           # every forced commit: (t, anchor, v*, s*, states counted)
        self.oracle_runs = 0

    def _extend(self, R):
        """one pass of the oracle over times 0 .. R of the model as pruned so far"""
        om = oracle.OracleModel(self.A, self.Bt, self.Pi)
        try:
            row, args = om.full_forward(self.obt, 0, R, -1)
        finally:
            om.close()
        self.oracle_runs += 1
        gone = self.pruned[1:R + 1]                                # (row j - 1 of the table is time j; no check at time 0)
        assert (args[gone] == -1).all()
        args[gone] = self.args[:R][gone]                           # the device never recomputes a row: the old entries stay
        # the arg rows before the last forced commit, and the survivors' entries of its row, did not move
        assert (args[:self.upto] == self.args[:self.upto]).all()
        self.args[self.upto:R] = args[self.upto:]
        self.table[self.upto:R] = args[self.upto:].tolist()
        self.upto, self.row, self.row_time = max(self.upto, R), row, R

    def pending(self):
        return self.times - self.committed

    def _walk(self, L, R, end):
        if R == L:
            return [int(end)]
        chain, restarts = btm.chunk_walk(self.table[L:R], 0, R - L, int(end))
        assert chain == btm.serial_walk(self.table[L:R], 0, R - L, int(end))
        self.bt_restarts += restarts
        return chain + [int(end)]

    def _force(self, t):
        if self.row_time != t:
            self._extend(t)
        best = int(np.argmax(self.row))
        v = int(self.anc[best])
        assert v >= 0 and self.row[best] > -np.finfo(np.float32).max      # more than one ancestor: a finite maximum
        out = self.anc != v
        self.forced.append((t, self.anchor, v, best, int(((self.anc >= 0) & out).sum())))
        self.pruned[t, out] = True
        self.Bt[out, t] = 0
        self.upto, self.row_time = t, -1                           # what lies behind time t is to be computed again
        return v, np.where(~out, np.arange(self.K), -1)

    def push(self, n):
        """consumes the next n times; returns the committed piece (a list), or None when the push ends dead"""
        assert not self.dead and n >= 1 and self.times + n <= self.T
        record = None
        for i in range(n):
            j = self.times + i
            if j > 0:
                if j > self.upto:
                    # as far as the next check, or the first time a commit can be forced at (the anchor only moves
                    # forward) where that is later; unbounded: the whole sequence
                    first = max(j + min(self.check_every - self.since - 1, n - 1 - i), self.anchor + self.max_lag)
                    self._extend(min(first, self.T - 1) if self.max_lag > 0 else self.T - 1)
                bp = self.args[j - 1]
                self.anc = np.where(bp >= 0, self.anc[np.maximum(bp, 0)], -1)
                self.since += 1
            if self.since > 0 and (self.since == self.check_every or i == n - 1):
                self.checks += 1
                self.since = 0
                V = np.unique(self.anc[self.anc >= 0])
                if V.size == 0:
                    self.dead = True
                elif V.size == 1 or (self.max_lag > 0 and j - self.anchor >= self.max_lag):
                    assert self.anchor >= self.committed
                    if V.size == 1:
                        v, anc = int(V[0]), np.where(bp >= 0, np.arange(self.K), -1)
                    else:
                        v, anc = self._force(j)
                    record = (self.anchor, v)
                    self.records.append((self.anchor, v, V.size > 1))
                    self.commits += 1
                    self.anchor, self.anc = j, anc
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
        assert not self.dead and self.times == self.T
        if self.row_time != self.T - 1:
            self._extend(self.T - 1)
        piece = self._walk(self.committed, self.times - 1, int(np.argmax(self.row)))
        self.committed = self.times
        return piece

    def lag_stats(self):
        t = [f[0] for f in self.forced]
        return dict(max_lag=self.max_lag, forced_commits=len(t), pruned_states=sum(f[4] for f in self.forced),
                    first_forced_time=t[0] if t else -1, last_forced_time=t[-1] if t else -1)


def run(A, B, Pi, ob, check_every, max_lag, chunks):
    """stream_model.run's result, and: pending (after every push), score (float32, the close's), records, forced, pruned
    (bool [T, K]), lag (the fv_lag_stats members), path (the concatenation; None for a dead run), oracle_runs."""
    s = Stream(A, B, Pi, ob, check_every, max_lag)
    out = dict(pieces=[], committed=[], pending=[], dead=None, score=None, path=None)
    for q, n in enumerate(chunks):
        piece = s.push(n)
        out["committed"].append(s.committed)
        out["pending"].append(s.pending())
        if piece is None:
            out["dead"] = q
            break
        out["pieces"].append(piece)
    if out["dead"] is None:
        out["pieces"].append(s.close())
        out["score"] = np.float32(s.row.max())
        out["path"] = [x for p in out["pieces"] for x in p]
    out.update(checks=s.checks, commits=s.commits, bt_restarts=s.bt_restarts, lag_max=s.lag_max, records=s.records,
               forced=s.forced, pruned=s.pruned, lag=s.lag_stats(), oracle_runs=s.oracle_runs, args=s.args, row=s.row)
    return out


def bound(max_lag, check_every):
    """the largest pending count after an accepted push of a lag-bounded stream"""
    return 2 * max_lag + check_every - 2


def connected(A, path):
    """every transition of the path has a finite log"""
    p = np.asarray(path)
    return bool((p >= 0).all() and (np.asarray(A)[p[:-1], p[1:]] > 0).all())
