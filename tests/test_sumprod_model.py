"""CPU: tests/sumprod_model.py, the float64 model the GPU tests of fv_loglik / fv_posteriors compare with, pinned to brute
force (all K^T paths summed with math.fsum), its -inf rules, and the two flush models: each must have a finite loglik
and a column that lies more than 745 below its row's maximum, or the GPU tests on them would exercise nothing."""
import math

import numpy as np
import pytest

import sumprod_model as sp


def small_model(K, T, seed, zero=0.0):
    rng = np.random.default_rng(seed)
    A = rng.random((K, K), dtype=np.float32)
    A[rng.random((K, K)) < zero] = 0
    Pi = rng.random(K, dtype=np.float32)
    e = np.log(rng.random((T, K)))
    return A, Pi, e


@pytest.mark.parametrize("K,T,seed", [(3, 5, 1), (2, 8, 2), (3, 5, 3)])
def test_model_equals_brute_force(K, T, seed):
    A, Pi, e = small_model(K, T, seed, zero=0.3 if seed == 3 else 0.0)
    r = sp.run(A, Pi, e)
    ll, gamma = sp.brute(A, Pi, e)
    assert math.isfinite(ll)
    assert abs(r["loglik"] - ll) <= 1e-14 * max(1.0, abs(ll))
    assert np.abs(r["gamma"] - gamma).max() <= 1e-14
    assert np.abs(r["gamma"].sum(axis=1) - 1.0).max() <= 1e-14
    assert (r["path"] == gamma.argmax(axis=1)).all()       # (random scores: the best two of a row lie far apart)


def test_unreachable_state_is_minus_inf_and_gamma_zero():
    A, Pi, e = small_model(4, 5, 7)
    A[:, 2] = 0            # no predecessor
    Pi[2] = 0              # and no start
    r = sp.run(A, Pi, e)
    assert math.isfinite(r["loglik"])
    assert np.isneginf(r["alpha"][:, 2]).all()
    assert (r["gamma"][:, 2] == 0).all() and (r["path"] != 2).all()
    assert np.isfinite(np.delete(r["alpha"], 2, axis=1)).all()


def test_zero_probability_sequence():
    A, Pi, e = small_model(3, 4, 9)
    e[2, :] = -np.inf
    r = sp.run(A, Pi, e)
    assert r["loglik"] == -math.inf and r["gamma"] is None and (r["path"] == -1).all()
    assert np.isfinite(r["alpha"][:2]).all() and np.isneginf(r["alpha"][2:]).all()


def test_tolerances_are_the_header_formula():
    assert sp.tol_alpha(0, 200, 0.5) == 2 * 1 * 1224 * 2.0 ** -53
    assert sp.tol_alpha(63, 200, 100.0) == 2 * 64 * 1224 * 2.0 ** -53 * 100.0
    assert sp.tol_beta(63, 64, 200, 100.0) == sp.tol_alpha(0, 200, 100.0)
    ta, tb = sp.tol_rows(64, 200, 100.0)
    assert ta[63, 0] == sp.tol_alpha(63, 200, 100.0) and tb[0, 0] == sp.tol_beta(0, 64, 200, 100.0)


def test_forward_flush_model_exercises_the_flush():
    A, B, Pi, e = sp.flush_forward()
    r = sp.run(A, Pi, e)
    assert math.isfinite(r["loglik"]) and -830 < r["loglik"] < -780
    al = r["alpha"]
    # the only predecessors of (2, 36) and of (3, 35) lie more than 745 below their rows' maxima
    assert (np.nonzero(A[:, 36])[0] == np.arange(16)).all() and (np.nonzero(A[:, 35])[0] == [36]).all()
    assert al[1, :16].max() < al[1].max() - 745
    assert al[2, 36] < al[2].max() - 745 and math.isfinite(al[2, 36])
    assert np.isfinite(al[3]).sum() == 1 and math.isfinite(al[3, 35])
    assert abs(r["gamma"][2, 36] - 1) < 1e-12 and abs(r["gamma"][3, 35] - 1) < 1e-12


def test_backward_flush_model_exercises_the_flush():
    A, B, Pi, e = sp.flush_backward()
    r = sp.run(A, Pi, e)
    T = sp.FLUSH_T
    assert math.isfinite(r["loglik"]) and -830 < r["loglik"] < -780
    v = e + r["beta"]              # what the backward step takes in: v[t + 1] gives beta[t]
    # beta[T - 3][36] comes from v[T - 2][0..15] only, beta[T - 4][35] from v[T - 3][36] only
    assert (np.nonzero(A[36])[0] == np.arange(16)).all() and (np.nonzero(A[35])[0] == [36]).all()
    assert v[T - 2, :16].max() < v[T - 2].max() - 745
    assert v[T - 3, 36] < v[T - 3].max() - 745 and math.isfinite(r["beta"][T - 3, 36])
    assert math.isfinite(r["beta"][T - 4, 35])
    assert abs(r["gamma"][T - 3, 36] - 1) < 1e-12 and abs(r["gamma"][T - 4, 35] - 1) < 1e-12
