"""The float64 CPU model of fv_expected_counts (include/flashvit.h) on top of sumprod_model: the expected
counts by the per-cell log form, the scale w_t that decides the wide times, a brute-force enumerator for tiny K and T, and
the tolerance of guarantee G1.

Nothing here scales by a row maximum: every xi cell is exp(alpha + LA + e + beta - loglik) on its own, so nothing is
flushed that the exact value keeps."""
import itertools
import math

import numpy as np

import sumprod_model as sp

WIDE_ABOVE = 500.0
FLOOR = 2.0 ** -160


def one(A, Pi, e, ob=None, M=0):
    """One sequence.  e: T x K float64 emission terms; ob, M: its symbols and the alphabet (emit is None without them).
    Returns a dict: trans (K x K), init, occ, last (g_{T-1}) (K), emit (K x M or None), loglik, w (the T - 1 values of w_t),
    run (sumprod_model.run's dict).  A sequence of probability 0 has zero counts."""
    r = sp.run(A, Pi, e)
    e = np.asarray(e, dtype=np.float64)
    T, K = e.shape
    out = dict(trans=np.zeros((K, K)), init=np.zeros(K), occ=np.zeros(K), last=np.zeros(K),
               emit=None if ob is None else np.zeros((K, M)), loglik=r["loglik"], w=np.zeros(max(T - 1, 0)), run=r)
    if not math.isfinite(r["loglik"]):
        return out
    LA = sp.libm_log(A)
    alpha, beta, ll = r["alpha"], r["beta"], r["loglik"]
    with np.errstate(invalid="ignore"):
        for t in range(T - 1):
            eb = e[t + 1] + beta[t + 1]
            out["trans"] += np.exp(alpha[t][:, None] + LA + eb[None, :] - ll)
            out["w"][t] = alpha[t].max() + eb.max() - ll
    g = r["gamma"]
    out["init"], out["occ"], out["last"] = g[0].copy(), g.sum(axis=0), g[T - 1].copy()
    if ob is not None:
        for t in range(T):
            out["emit"][:, ob[t]] += g[t]
    return out


def wide_times(w):
    """the times the device adds in the exact form"""
    return [t for t, x in enumerate(w) if x > WIDE_ABOVE]


def batch(A, B, Pi, obs):
    """Symbol sequences: the sums over the live sequences in order, beside per-sequence results (`each`)."""
    K, M = B.shape
    each = [one(A, Pi, sp.emission_rows(B, o), o, M) for o in obs]
    return fold(each, K, M)


def fold(each, K, M=0):
    tot = dict(trans=np.zeros((K, K)), init=np.zeros(K), occ=np.zeros(K), last=np.zeros(K),
               emit=np.zeros((K, M)) if M else None, each=each, loglik=np.array([c["loglik"] for c in each]))
    for c in each:
        for k in ("trans", "init", "occ", "last") + (("emit",) if M else ()):
            tot[k] = tot[k] + c[k]
    return tot


def tolerance(T_longest, K, a_max):
    """R of guarantee G1: three shares of tol_alpha(T - 1)"""
    return 3.0 * sp.tol_alpha(T_longest - 1, K, a_max)


def within(got, exact, R, n):
    """(ok, worst error over bound) of |got - exact| <= R * exact + n * 2^-160, cell by cell"""
    got, exact = np.asarray(got, dtype=np.float64), np.asarray(exact, dtype=np.float64)
    bound = R * exact + n * FLOOR
    err = np.abs(got - exact)
    return bool((err <= bound).all() and np.isfinite(got).all()), float((err / bound).max())


def brute(A, Pi, e, ob=None, M=0):
    """The counts by enumerating all K^T paths, every sum by math.fsum: for tiny K, T only."""
    A = np.asarray(A, dtype=np.float32).astype(np.float64)
    Pi = np.asarray(Pi, dtype=np.float32).astype(np.float64)
    T, K = e.shape
    E = np.exp(e)
    terms = []
    tr = [[[] for _ in range(K)] for _ in range(K)]
    by = [[[] for _ in range(K)] for _ in range(T)]
    for path in itertools.product(range(K), repeat=T):
        p = Pi[path[0]] * E[0][path[0]]
        for t in range(1, T):
            p *= A[path[t - 1]][path[t]] * E[t][path[t]]
        terms.append(p)
        for t in range(T):
            by[t][path[t]].append(p)
        for t in range(T - 1):
            tr[path[t]][path[t + 1]].append(p)
    total = math.fsum(terms)
    g = np.array([[math.fsum(by[t][j]) / total for j in range(K)] for t in range(T)])
    out = dict(trans=np.array([[math.fsum(tr[i][j]) / total for j in range(K)] for i in range(K)]),
               init=g[0].copy(), occ=np.array([math.fsum(g[:, j]) for j in range(K)]), last=g[T - 1].copy(), loglik=math.log(total),
               emit=None)
    if ob is not None:
        out["emit"] = np.array([[math.fsum(g[t, j] for t in range(T) if ob[t] == m) for m in range(M)] for j in range(K)])
    return out


def normalise_rows(counts):
    """the M-step of one table in float64; an all-zero row stays zero"""
    counts = np.asarray(counts, dtype=np.float64)
    total = counts.sum(axis=-1, keepdims=True)
    return np.divide(counts, total, out=np.zeros_like(counts), where=total > 0)


def em_step(A, B, Pi, obs):
    """One EM iteration of the model on the CPU: (float32 A, B, Pi of the M-step, the summed loglik of the model given)"""
    c = batch(A, B, Pi, obs)
    new = tuple(normalise_rows(c[k]).astype(np.float32) for k in ("trans", "emit", "init"))
    return new, float(np.sum(c["loglik"]))
