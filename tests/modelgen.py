"""Test-side model builders: every golden case is described by a small spec dict
from which the float64 model the generator would have saved is rebuilt, then
pushed through the text quantisation the reference loader applies."""
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from flash_viterbi_amd import hostio  # noqa: E402
from flash_viterbi_amd.generate_data import data_script  # noqa: E402


def _ties_all(K, M, seed, degree=8):
    """Every row has `degree` out-edges of weight 1/degree, B and Pi uniform: every finite
    score at a step is the same float, so the decoded path is decided by tie-breaking only."""
    rs = np.random.RandomState(seed)
    A = np.zeros((K, K))
    for k in range(K):
        A[k, rs.choice(K, size=degree, replace=False)] = 1.0 / degree
    return A, np.full((K, M), 1.0 / M), np.full(K, 1.0 / K)


def _ties_semi(K, M, seed):
    """Dyadic weights (row sums exactly 1): many, but not all, candidates tie."""
    rs = np.random.RandomState(seed)
    A = np.zeros((K, K))
    w = np.array([0.25, 0.25, 0.125, 0.125, 0.125, 0.125])
    for k in range(K):
        A[k, rs.choice(K, size=w.size, replace=False)] = rs.permutation(w)
    base = np.array([0.5, 0.25, 0.125, 0.125] + [0.0] * (M - 4)) if M >= 4 else np.full(M, 1.0 / M)
    if M > 4:  # keep every symbol possible: split the last weight
        base = np.array([0.5, 0.25, 0.125] + [0.125 / (M - 3)] * (M - 3))
    B = np.stack([rs.permutation(base) for _ in range(K)])
    return A, B, np.full(K, 1.0 / K)


def _classes(rs, shape, probs=(0.25, 0.25, 0.25, 0.25)):
    """entries of {1e-16, 1e-8, 1e-3, U(0.1, 1)}"""
    cls = rs.choice(4, size=shape, p=probs)
    u = rs.uniform(0.1, 1.0, size=shape)
    return np.where(cls == 0, 1e-16, np.where(cls == 1, 1e-8, np.where(cls == 2, 1e-3, u)))


def _wide64(kind, K, M, seed):
    """float64 (A, B, Pi) of a wide-range model and the generator after them (wide_model draws its observations from it)."""
    rs = np.random.RandomState(seed)
    if kind == "wideA":
        # every transition present, weights over 16 decades: the table's step is large (36.8 / 65534), the filter's
        # window wide, the score rows stay inside the code range
        A = _classes(rs, (K, K))
        Bm = _classes(rs, (K, M), (0.1, 0.2, 0.3, 0.4))
        Pi = _classes(rs, (K,), (0.1, 0.2, 0.3, 0.4))
    elif kind == "wideB":
        # sparse transitions of ordinary weights (code range = |log 0.1| = 2.3), emissions over 16 decades: most score
        # rows lie further below the row maximum than the code range reaches; columns all of whose in-edges come from
        # such rows have only saturated sums
        p = min(1.0, 6.0 / K)
        A = rs.uniform(0.1, 1.0, (K, K)) * (rs.uniform(0, 1, (K, K)) < p)
        A[np.arange(K), rs.randint(0, K, K)] = rs.uniform(0.1, 1.0, K)        # every state has a successor
        Bm = _classes(rs, (K, M))
        Pi = _classes(rs, (K,), (0.1, 0.2, 0.3, 0.4))
    elif kind == "wideAB":
        # both: sparse transitions over 16 decades (a third of the graph), emissions likewise
        A = _classes(rs, (K, K)) * (rs.uniform(0, 1, (K, K)) < 0.3)
        A[np.arange(K), rs.randint(0, K, K)] = 0.5
        Bm = _classes(rs, (K, M))
        Pi = _classes(rs, (K,))
    else:
        raise ValueError(kind)
    return A, Bm, Pi, rs


def _rotor64(K, M, noise, seed):
    rs = np.random.RandomState(seed)
    A = np.zeros((K, K))
    A[np.arange(K), (np.arange(K) + 1) % K] = 1.0
    if noise:
        for k in range(K):
            others = np.delete(np.arange(K), (k + 1) % K)
            A[k, rs.choice(others, size=2, replace=False)] = noise
        A /= A.sum(axis=1, keepdims=True)
    Bm = rs.uniform(0.1, 1.0, (K, M))
    Bm /= Bm.sum(axis=1, keepdims=True)
    Pi = rs.uniform(0.1, 1.0, K)
    Pi /= Pi.sum()
    return A, Bm, Pi


def _rotor_tied_column64(K, g):
    A = np.zeros((K, K))
    A[np.arange(K), (np.arange(K) + 1) % K] = 1.0
    A[g - 1, g + 1] = 1.0
    Bm = np.full((K, 2), 0.5)
    Bm[g - 1, 1] = 0.25
    return A, Bm, np.full(K, 1.0 / K)


CIRCULANT_OFF = {2053: (255, 256, 257, 1023, 1024, 1025, 1500, 2000),
                 1025: (100, 255, 256, 257, 500, 700, 900, 1001),
                 257: (50, 100, 128, 150, 200, 230, 251, 255)}
CIRCULANT_CUT = {2053: (1030, 300), 1025: (1000, 300), 257: (250, 60)}      # states below it cannot emit symbol 8 / symbol 9


def _circulant32(K, OFF, cuts):
    """float32 directly: every entry is 0, 1/8 or float32(1/K), and the '%.16f' text of the widened values reads back as
    the same float32 (tests/test_modelgen_builders.py)."""
    A = np.zeros((K, K), dtype=np.float32)
    for o in OFF:
        A[np.arange(K), (np.arange(K) + o) % K] = 0.125
    Bm = np.full((K, 10), 0.125, dtype=np.float32)
    Bm[:cuts[0], 8] = 0
    Bm[:cuts[1], 9] = 0
    return A, Bm, np.full(K, np.float32(1.0 / K))


def _knock_out(A, Pi, seed):
    """Copies with every 7th column of A zero (those states have no predecessor: -FLT_MAX / -1 in every step row) and a
    third of Pi zero (-inf entries of a Pi-initialised row)."""
    A = A.copy()
    A[:, ::7] = 0.0
    Pi = Pi.copy()
    Pi[np.random.RandomState(seed).rand(A.shape[0]) < 0.33] = 0.0
    return A, Pi


def _unreachable64(K, M, seed, prob):
    A, Bm, Pi = data_script.make_model64(K, M, seed, prob)
    A, Pi = _knock_out(A, Pi, seed)
    return A, Bm, Pi


def model64(spec):
    """The float64 (A, B, Pi) whose '%.16f' text the reference loader reads: the one construction of every kind."""
    kind = spec["kind"]
    K, M = spec["K"], spec["M"]
    if kind == "data_script":
        return data_script.make_model64(K, M, spec["seed"], spec["prob"])
    if kind == "ties_all":
        return _ties_all(K, M, spec["seed"])
    if kind == "ties_semi":
        return _ties_semi(K, M, spec["seed"])
    if kind in ("wideA", "wideB", "wideAB"):
        return _wide64(kind, K, M, spec["seed"])[:3]
    if kind == "rotor":
        return _rotor64(K, M, spec["noise"], spec["seed"])
    if kind == "rotor_tied_column":
        assert M == 2
        return _rotor_tied_column64(K, spec["g"])
    if kind == "circulant_ties":
        assert M == 10
        return tuple(x.astype(np.float64) for x in _circulant32(K, CIRCULANT_OFF[K], CIRCULANT_CUT[K]))
    if kind == "unreachable":
        return _unreachable64(K, M, spec["seed"], spec["prob"])
    raise ValueError(kind)


def observations(spec):
    if "ob" in spec:
        return np.asarray(spec["ob"], dtype=np.int32)
    rng = random.Random(spec.get("ob_seed", spec["seed"]))
    return np.asarray([rng.randint(0, spec["M"] - 1) for _ in range(spec["T"])], dtype=np.int32)


def model32(spec):
    """(A, B, Pi, ob) in the float32 the reference loader reads from the generator's text."""
    if spec["kind"] == "sparse_fast":
        A, B, Pi = data_script.make_model32_fast(spec["K"], spec["M"], spec["seed"], spec["prob"])
        return A, B, Pi, observations(spec)
    A, B, Pi = model64(spec)
    return (hostio.quantize_text16(A), hostio.quantize_text16(B), hostio.quantize_text16(Pi),
            observations(spec))


def write_text(spec, out_dir):
    """Writes the four text files the reference programs open (prob is part of the name)."""
    A, B, Pi = model64(spec)
    data_script.write_files(out_dir, spec["K"], spec["T"], spec["prob"], A, B, Pi,
                            observations(spec), text=True, binary=False)


def _model32(**spec):
    return model32(dict(spec, ob=()))[:3]


def wide_model(kind, K, M, T, seed):
    """Wide-range models (float32 A, B, Pi and the observations): the inputs where the filter kernels' error bracket is
    thinnest (tests/test_gpu_adversarial.py).  The observations continue the model's random stream."""
    A, Bm, Pi, rs = _wide64(kind, K, M, seed)
    ob = rs.randint(0, M, T).astype(np.int32)
    return hostio.quantize_text16(A), hostio.quantize_text16(Bm), hostio.quantize_text16(Pi), ob


def wide_spec(kind, K, M, T, seed):
    """The spec of wide_model(kind, K, M, T, seed), its observations written out (no random.Random(seed) draws them)."""
    ob = wide_model(kind, K, M, T, seed)[3]
    return dict(kind=kind, K=K, M=M, T=T, prob=0.5, seed=seed, ob=[int(x) for x in ob])


def rotor(K, M, noise, seed):
    """State k moves to k + 1 (mod K).  noise = 0: every column has exactly one predecessor, so no two back-track chains
    ever merge — a guessed start is wrong for good (tests/test_gpu_pass_ends.py).  noise > 0: two more edges of that
    weight per row (rows renormalised): chains merge, slowly.  B and Pi ~ U(0.1, 1), normalised.  float32 (A, B, Pi)."""
    return _model32(kind="rotor", K=K, M=M, noise=noise, seed=seed)


def rotor_tied_column(K=131, g=30):
    """The rotor with weight 1 on every edge, one more edge g-1 -> g+1, uniform Pi, and two symbols every state emits with
    1/2 — but state g-1 emits symbol 1 with 1/4 (rows not normalised).  Every state has the same score unless its chain
    passed state g-1 under symbol 1, so column g+1 — the only one with two predecessors — is tied at every time except
    the two after a symbol 1: a FLASH-BS decode tags that cell at almost every time, and only there.  float32 (A, B, Pi)."""
    return _model32(kind="rotor_tied_column", K=K, M=2, g=g)


def circulant_ties(K=2053, OFF=None, cuts=None):
    """State k moves to k + o (mod K) for the eight o of OFF, weight 1/8 each; Pi uniform; ten symbols: 0 .. 7 are emitted
    by every state with 1/8, symbol 8 only by the states from cuts[0] on, symbol 9 only by those from cuts[1] on (the rows
    of B are deliberately not normalised).  Every finite score of a step is the same float, so every back-pointer is the
    lowest live predecessor and every end pick the lowest live state: after symbol 8 / 9 that is cuts[0] / cuts[1].  The
    predecessors of a column lie up to 2000 states apart: tied candidates in different waves, workgroup trips and
    1024-blocks of the kernels that pick among them.  float32 (A, B, Pi); the spec kind `circulant_ties` is the
    widening of these arrays for the K of CIRCULANT_OFF."""
    return _circulant32(K, CIRCULANT_OFF[K] if OFF is None else OFF, CIRCULANT_CUT[K] if cuts is None else cuts)


def circulant_observations(T, last, seed):
    """symbols 0 .. 7 at random, `last` (8 or 9: a cut; anything else: none) at the last time and at T/3 and 2T/3"""
    ob = np.random.RandomState(seed).randint(0, 8, T).astype(np.int32)
    if last in (8, 9):
        ob[T // 3] = ob[2 * T // 3] = last
    ob[T - 1] = last
    return ob


def unreachable_model(K, M, T, seed, prob=0.112):
    """A generate_data model with states no path reaches (_knock_out), observations from RandomState(seed + 1)."""
    ob = np.random.RandomState(seed + 1).randint(0, M, T).astype(np.int32)
    return _model32(kind="unreachable", K=K, M=M, seed=seed, prob=prob) + (ob,)


def unreachable_fast(K, M, T, seed):
    """The same knock-out on the vectorised builder's float32 model (prob 0.1) — not the spec kind `unreachable`."""
    A, Bm, Pi, _ = model32(dict(kind="sparse_fast", K=K, M=M, T=T, prob=0.1, seed=seed, ob=()))
    A, Pi = _knock_out(A, Pi, seed)
    return A, Bm, Pi, np.random.RandomState(seed + 1).randint(0, M, T).astype(np.int32)


def sha(a):
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def plain_model(K, M, density, seed, scale=1.0, zero_a=False):
    """Unnormalised float32 (A, B, Pi) with entries in [0, scale), a fraction `density` of A kept, from numpy's PCG64 alone (no arithmetic a numpy build could round differently)."""
    rng = np.random.default_rng(seed)
    A = rng.random((K, K), dtype=np.float32)
    keep = rng.random((K, K), dtype=np.float32) < np.float32(density)
    A = np.where(keep, A, np.float32(0)).astype(np.float32)
    B = rng.random((K, M), dtype=np.float32)
    Pi = rng.random(K, dtype=np.float32)
    if scale != 1.0:
        A = (A * np.float32(scale)).astype(np.float32)      # (exact: a power of two)
    if zero_a:
        A[:] = 0
    return A, B, Pi
