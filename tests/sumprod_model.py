"""The float64 CPU model of fv_loglik / fv_posteriors (include/flashvit.h): forward, backward, gamma and
the posterior path by per-column-maximum log-sum-exp, and the tolerance functions of guarantee 1.

The model never scales by a row maximum: every column is max_i + log sum_i exp(. - max_i), so nothing is flushed that
the exact value keeps."""
import math

import numpy as np

U = 2.0 ** -53


def libm_log(x):
    """float64 log of every float32 entry of x through math.log (the host libm of fv_set_model); log 0 = -inf"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    vals, inv = np.unique(x.reshape(-1), return_inverse=True)
    table = np.array([math.log(float(v)) if v > 0 else -math.inf for v in vals], dtype=np.float64)
    return table[inv].reshape(x.shape)


def lse_columns(v, LA):
    """out[j] = log sum_i exp(v[i] + LA[i][j]), each column scaled by its own maximum; -inf where no term is finite"""
    with np.errstate(invalid="ignore", divide="ignore"):
        X = v[:, None] + LA
        m = X.max(axis=0)
        safe = np.where(np.isfinite(m), m, 0.0)
        s = np.exp(X - safe[None, :]).sum(axis=0)
        return np.where(np.isfinite(m), safe + np.log(s), -np.inf)


def lse(v):
    m = v.max()
    if not np.isfinite(m):
        return -math.inf
    return float(m + math.log(np.exp(v - m).sum()))


def emission_rows(B, ob):
    """e[t][j] = log((double)B[j][ob[t]])"""
    return np.ascontiguousarray(libm_log(B)[:, np.asarray(ob, dtype=np.int64)].T)


def forward(A, Pi, e):
    """the alpha rows alone (T x K float64)"""
    LA, LPi = libm_log(A), libm_log(Pi)
    e = np.asarray(e, dtype=np.float64)
    alpha = np.empty(e.shape)
    with np.errstate(invalid="ignore"):
        alpha[0] = LPi + e[0]
        for t in range(1, e.shape[0]):
            alpha[t] = e[t] + lse_columns(alpha[t - 1], LA)
    return alpha


def run(A, Pi, e):
    """A, Pi: the float32 model; e: T x K float64 emission terms.  Returns a dict: alpha, beta (T x K float64), loglik,
    gamma (T x K float64, None when loglik is -inf), path (int32; -1 when loglik is -inf), ab = alpha + beta."""
    LA, LPi = libm_log(A), libm_log(Pi)
    e = np.asarray(e, dtype=np.float64)
    T, K = e.shape
    alpha = np.empty((T, K))
    beta = np.zeros((T, K))
    with np.errstate(invalid="ignore"):
        alpha[0] = LPi + e[0]
        for t in range(1, T):
            alpha[t] = e[t] + lse_columns(alpha[t - 1], LA)
        LAT = np.ascontiguousarray(LA.T)
        for t in range(T - 2, -1, -1):
            beta[t] = lse_columns(e[t + 1] + beta[t + 1], LAT)
        ab = alpha + beta
    loglik = lse(alpha[T - 1])
    if not math.isfinite(loglik):
        return dict(alpha=alpha, beta=beta, loglik=loglik, gamma=None, path=np.full(T, -1, dtype=np.int32), ab=ab)
    gamma = np.exp(ab - loglik)              # (exp(-inf) = 0 where either term is -inf)
    return dict(alpha=alpha, beta=beta, loglik=loglik, gamma=gamma, path=ab.argmax(axis=1).astype(np.int32), ab=ab)


def amax(r):
    """the largest finite |alpha| or |beta| of a run"""
    both = np.concatenate([r["alpha"].reshape(-1), r["beta"].reshape(-1)])
    both = both[np.isfinite(both)]
    return float(np.abs(both).max()) if both.size else 0.0


def tol_alpha(t, K, a_max):
    """guarantee 1 for alpha[t][*]; tol_alpha(T - 1, ...) is loglik's"""
    return 2.0 * (t + 1) * (K + 1024) * U * max(1.0, a_max)


def tol_beta(t, T, K, a_max):
    return 2.0 * (T - t) * (K + 1024) * U * max(1.0, a_max)


def tol_rows(T, K, a_max):
    """(T x 1 tolerances of the alpha rows, of the beta rows)"""
    t = np.arange(T, dtype=np.float64)[:, None]
    scale = 2.0 * (K + 1024) * U * max(1.0, a_max)
    return (t + 1) * scale, (T - t) * scale


def brute(A, Pi, e):
    """loglik and gamma by enumerating all K^T paths, summed with math.fsum: for tiny K, T only"""
    import itertools
    A = np.asarray(A, dtype=np.float32).astype(np.float64)
    Pi = np.asarray(Pi, dtype=np.float32).astype(np.float64)
    T, K = e.shape
    E = np.exp(e)
    terms, by = [], [[[] for _ in range(K)] for _ in range(T)]
    for path in itertools.product(range(K), repeat=T):
        p = Pi[path[0]] * E[0][path[0]]
        for t in range(1, T):
            p *= A[path[t - 1]][path[t]] * E[t][path[t]]
        terms.append(p)
        for t in range(T):
            by[t][path[t]].append(p)
    total = math.fsum(terms)
    gamma = np.array([[math.fsum(by[t][j]) / total if total > 0 else 0.0 for j in range(K)] for t in range(T)])
    return (math.log(total) if total > 0 else -math.inf), gamma


# ---- the two flush models (guarantee 2): K = 37, T = 6, transitions 0 or 1/2, staged emission scores

FLUSH_K, FLUSH_T = 37, 6


def flush_forward():
    """(A, B, Pi, e): states 0..15 score -800 at time 1; state 36 has in-edges from 0..15 only; state 35 has its only
    in-edge from 36; at time 3 only state 35 has a finite score.  Every path of non-zero probability runs through
    (1, one of 0..15), (2, 36), (3, 35): alpha[1][0..15] and alpha[2][36] lie about 800 below their rows' maxima, and a
    step that scales by the row maximum alone flushes both to 0."""
    K, T = FLUSH_K, FLUSH_T
    A = np.zeros((K, K), dtype=np.float32)
    A[:36, :35] = 0.5              # 0..35 -> 0..34
    A[:16, 36] = 0.5               # 0..15 -> 36
    A[36, 35] = 0.5                # 36 -> 35, its only successor and 35's only predecessor
    B = np.full((K, 2), 0.5, dtype=np.float32)
    Pi = np.full(K, np.float32(1.0 / K))
    e = np.zeros((T, K))
    e[1, :16] = -800.0
    e[3, :] = -np.inf
    e[3, 35] = 0.0
    return A, B, Pi, e


def flush_backward():
    """the time-reversed twin: transposed transitions and reversed score rows, so the backward pass meets the two
    flushed columns"""
    A, B, Pi, e = flush_forward()
    return np.ascontiguousarray(A.T), B, Pi, np.ascontiguousarray(e[::-1])
