"""The CPU model of fv_expected_counts (tests/counts_model.py) against a brute-force enumeration, the identities of the
counts, the wide times of the two flush models, and EM's monotone likelihood on a small normalised model."""
import math

import numpy as np
import pytest

import counts_model as cm
import modelgen
import sumprod_model as sp


def small_model(K, M, seed, zeros=True):
    rng = np.random.default_rng(seed)
    A = rng.random((K, K)).astype(np.float32)
    if zeros:
        A[rng.random((K, K)) < 0.25] = 0
        A[np.arange(K), np.arange(K)] = 0.5           # (no dead row)
    return A, rng.random((K, M)).astype(np.float32) + np.float32(0.05), rng.random(K).astype(np.float32) + np.float32(0.05)


@pytest.mark.parametrize("K,T", [(3, 4), (2, 1), (2, 2), (2, 3)])
def test_model_against_brute_force(K, T):
    A, B, Pi = small_model(K, 3, 10 * K + T)
    ob = np.random.default_rng(T).integers(0, 3, T)
    e = sp.emission_rows(B, ob)
    got, want = cm.one(A, Pi, e, ob, 3), cm.brute(A, Pi, e, ob, 3)
    R = cm.tolerance(T, K, sp.amax(got["run"]))
    assert abs(got["loglik"] - want["loglik"]) <= sp.tol_alpha(T - 1, K, sp.amax(got["run"]))
    for k, n in (("trans", T - 1), ("init", 1), ("occ", T), ("last", 1), ("emit", T)):
        ok, worst = cm.within(got[k], want[k], R, max(n, 1))
        print(f"K={K} T={T} {k}: worst error / bound = {worst:.3e}")
        assert ok, k
    assert (got["trans"][A == 0] == 0).all()
    if T == 1:
        assert (got["trans"] == 0).all() and got["w"].size == 0


def check_identities(c, lengths, live, R, K):
    """the four identities of the header, each side within R of the other (sums of up to K cells)"""
    slack = lambda x: 2 * R * np.abs(x) + K * 2.0 ** -150
    assert (np.abs(c["trans"].sum(axis=1) - (c["occ"] - c["last"])) <= slack(c["occ"])).all()
    steps = sum(n - 1 for n, a in zip(lengths, live) if a)
    assert abs(c["trans"].sum() - steps) <= slack(steps)
    assert abs(c["init"].sum() - sum(live)) <= slack(sum(live))
    if c["emit"] is not None:
        assert (np.abs(c["emit"].sum(axis=1) - c["occ"]) <= slack(c["occ"])).all()


def test_identities_on_a_ragged_batch():
    A, B, Pi = modelgen.plain_model(37, 4, 0.5, 11)
    lengths = [1, 2, 17, 40]
    obs = [np.random.default_rng(40 + i).integers(0, 4, n) for i, n in enumerate(lengths)]
    c = cm.batch(A, B, Pi, obs)
    R = cm.tolerance(40, 37, max(sp.amax(x["run"]) for x in c["each"]))
    check_identities(c, lengths, [True] * 4, R, 37)
    assert (c["trans"][A == 0] == 0).all()


def test_a_dead_sequence_adds_nothing():
    A, B, Pi = modelgen.plain_model(37, 4, 0.5, 11)
    B = np.concatenate([B, np.zeros((37, 1), dtype=np.float32)], axis=1)
    good = np.random.default_rng(1).integers(0, 4, 9)
    dead = good.copy()
    dead[4] = 4
    both, alone = cm.batch(A, B, Pi, [good, dead, good]), cm.batch(A, B, Pi, [good, good])
    assert both["loglik"][1] == -math.inf
    for k in ("trans", "init", "occ", "emit"):
        assert (both[k] == alone[k]).all()


def test_wide_times_of_the_flush_models_and_of_an_ordinary_one():
    A, B, Pi, e = sp.flush_forward()
    c = cm.one(A, Pi, e)
    print("flush forward w_t:", c["w"])
    assert cm.wide_times(c["w"]) == [1, 2]
    R = cm.tolerance(sp.FLUSH_T, sp.FLUSH_K, sp.amax(c["run"]))
    check_identities(c, [sp.FLUSH_T], [True], R, sp.FLUSH_K)
    assert abs(c["trans"].sum() - 5) <= 1e-9 and c["trans"][36, 35] == pytest.approx(1.0)
    A, B, Pi, e = sp.flush_backward()
    c = cm.one(A, Pi, e)
    print("flush backward w_t:", c["w"])
    assert cm.wide_times(c["w"]) == [2, 3]
    check_identities(c, [sp.FLUSH_T], [True], R, sp.FLUSH_K)
    A, B, Pi = modelgen.plain_model(37, 4, 0.5, 11)
    ob = np.random.default_rng(140).integers(0, 4, 40)
    c = cm.one(A, Pi, sp.emission_rows(B, ob), ob, 4)
    print("plain37 w_t in", c["w"].min(), c["w"].max())
    assert (c["w"] <= 0).all()


def test_row_maximum_scaling_alone_loses_the_flush_models_mass():
    """why the wide times exist: the plain scaled outer product P Q^T A loses transition mass on both flush models"""
    for make in (sp.flush_forward, sp.flush_backward):
        A, B, Pi, e = make()
        c = cm.one(A, Pi, e)
        r = c["run"]
        lin = np.zeros_like(c["trans"])
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            for t in range(sp.FLUSH_T - 1):
                eb = e[t + 1] + r["beta"][t + 1]
                P = np.exp(r["alpha"][t] - r["alpha"][t].max())
                Q = np.exp(eb - eb.max() + min(c["w"][t], 700.0))
                lin += np.outer(P, Q) * A.astype(np.float64)
        assert lin.sum() < c["trans"].sum() - 1.5


def test_em_never_lowers_the_likelihood():
    K, M, lengths = 6, 3, (1, 7, 12, 20)
    rng = np.random.default_rng(5)
    A, B, Pi = (cm.normalise_rows(rng.random(s) + 0.1).astype(np.float32) for s in ((K, K), (K, M), (K,)))
    obs = [rng.integers(0, M, n) for n in lengths]
    margin = sum(lengths) * 2.0 ** -22
    seen = []
    for _ in range(5):                       # four iterations: five likelihoods
        (A, B, Pi), ll = cm.em_step(A, B, Pi, obs)
        seen.append(ll)
    print("EM logliks:", seen)
    assert all(b >= a - margin for a, b in zip(seen, seen[1:]))
    assert seen[-1] > seen[0]
