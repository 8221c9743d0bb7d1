"""CPU: the oracle's dP/dtheta (po.parameter_matrix) against a formula that has no eigen system in it, at repeated and nearly
repeated eigenvalues.

The yardstick is the upper right block of exp([[Q t, dQ t], [0, Q t]]) from scipy.linalg.expm (degenerate_eigen_util).  The bound
is 1e-12 * max |dP/dtheta|: the expm1 form of the divided difference measured at most 2.4e-15 on these models and expm itself is
good to about 1e-15, so the bound leaves a factor of 400; the quotient (e^{l_a t} - e^{l_b t}) / (l_a - l_b) with an exact l_a != l_b
test, which the oracle restated from the reference until this file existed, misses it by nine to twelve orders of magnitude at
K80, F81 and near JC69 (0.43, 0.99 and 1.9e-3 of max |dP| at t = 1e-6).
"""
import numpy as np
import pytest

import degenerate_eigen_util as du
from oracle import phyoracle as po

TIMES = (0.0, 1e-6, 0.05, 1.0, 30.0)


@pytest.mark.parametrize("name", du.MODELS)
def test_the_models_are_the_cases_they_are_named_for(name):
    ev, U, Ui = du.eigen(name)
    gap = du.smallest_gap(ev)
    print(f"{name}: eigenvalues {ev!r}, smallest gap {gap:.3e}")
    lo, hi = du.GAPS[name]
    assert lo <= gap <= hi
    np.testing.assert_allclose(U @ Ui, np.eye(4), atol=1e-14)
    Q = du.rate_matrix(ev, U, Ui)
    np.testing.assert_allclose(Q.sum(axis=1), 0.0, atol=1e-14)


@pytest.mark.parametrize("t", TIMES)
@pytest.mark.parametrize("name", du.MODELS)
def test_parameter_matrix_against_block_expm(name, t):
    ev, U, Ui = du.eigen(name)
    Q = du.rate_matrix(ev, U, Ui)
    worst = 0.0
    for dQ in du.random_dq(4, 3, seed=5):
        want = du.block_expm_derivative(Q, dQ, t)
        got = po.parameter_matrix(ev, U, Ui, dQ, t)
        scale = np.abs(want).max()
        err = np.abs(got - want).max()
        worst = max(worst, err / scale if scale > 0 else err)
        assert err <= 1e-12 * scale, (name, t, err, scale)
    print(f"{name} t = {t:g}: max error {worst:.3e} of max |dP| (bound 1e-12)")


def test_parameter_matrix_on_a_saturated_branch_is_finite():
    """(l_a - l_b) t beyond 709, the range of exp: with the larger eigenvalue in front no factor overflows (the other order is
    0 * inf there).  expm's scaling and squaring is no yardstick at such t; it is one at t = 60, where the form is held to it"""
    ev, U, Ui = du.eigen("gtr_random")
    dQ = du.random_dq(4, 1, seed=6)[0]
    for t in (400.0, 2000.0):
        got = po.parameter_matrix(ev, U, Ui, dQ, t)
        assert np.all(np.isfinite(got))
    t = 60.0
    want = du.block_expm_derivative(du.rate_matrix(ev, U, Ui), dQ, t)
    assert np.abs(po.parameter_matrix(ev, U, Ui, dQ, t) - want).max() <= 1e-12 * np.abs(want).max()
