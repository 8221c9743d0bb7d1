"""CPU-only: the NumPy restatement of phyamd_nni_optimize's rule (tests/nni_optimize_util.py) on the oracle alone, on the 4- and
8-taxon cases of tests/test_nni_gpu.py.  The one-row evaluator agrees with the definition; the rule ends at a stationary point or
at a bound; the bound on d1 at t* that tests/test_nni_optimize_gpu.py relies on holds for the restatement itself; and at least
90 % of each case's entries qualify for the comparison of lengths there."""
import numpy as np
import pytest

import nni_optimize_util as u
from test_nni_gpu import CASES, _problem

SMALL = sorted(c for c in CASES if c.startswith(("t4", "t8")))
ALL = sorted(CASES)


def interior(t):
    """not pinned to a bound: further than two steps of the final size from either"""
    return u.LOWER + 2 * u.TOLERANCE < t < u.UPPER - 2 * u.TOLERANCE


@pytest.mark.parametrize("case", SMALL)
def test_the_one_row_evaluator_is_the_definition(case):
    pb, _ = _problem(case)
    rng = np.random.default_rng(1)
    for k, v in u.entries(pb):
        f = u.EdgeEvaluator(pb, v, k)
        for t in (1e-8, pb.branch_lengths[v] * rng.uniform(0.5, 2.0), 1.0):
            got, want = f(t), u.evaluate(pb, v, k, t)
            assert abs(got[0] - want[0]) <= 1e-12 * abs(want[0]), (k, v, t, got, want)
            assert abs(got[1] - want[1]) <= 1e-10 * max(1.0, abs(want[1])), (k, v, t, got, want)
            assert abs(got[2] - want[2]) <= 1e-10 * max(1.0, abs(want[2])), (k, v, t, got, want)


@pytest.mark.parametrize("case", SMALL)
def test_the_rule_ends_at_a_stationary_point_or_a_bound(case):
    pb, _ = _problem(case)
    solved = u.solve_case(pb)
    inside = 0
    for (k, v), (t, n, _, _) in solved.items():
        assert 0 < n <= u.MAX_ITERATIONS and u.LOWER <= t <= u.UPPER, (k, v, t, n)
        lnl, d1, d2 = u.evaluate(pb, v, k, t)
        if interior(t):
            inside += 1
            # a central difference of the oracle's lnL changes sign around t*: lnL falls off to both sides
            h = 1e-3 * t
            up, down = u.evaluate(pb, v, k, t + h)[0], u.evaluate(pb, v, k, t - h)[0]
            assert (up - lnl) < 0 and (lnl - down) > 0, (k, v, t, down, lnl, up)
            # what the GPU test asks of the engine: one step from t* is no longer than the tolerance, with room for the curvature's
            # change over that step
            print(f"{case} ({k}, {v}): t* {t!r} after {n}, |d1| {abs(d1):.3e} <= 2 |d2| tol {2 * abs(d2) * u.TOLERANCE:.3e}")
            assert d2 < 0 and abs(d1) <= 2 * abs(d2) * u.TOLERANCE, (k, v, t, d1, d2)
        else:  # pinned to the lower bound (no entry of these cases grows to 10): lnL still rises towards it
            assert t - u.LOWER <= 2 * u.TOLERANCE and d1 < 0, (k, v, t, d1)
    assert inside >= 1, "no interior optimum in this case"


@pytest.mark.parametrize("case", ALL)
def test_nine_entries_in_ten_qualify(case):
    pb, _ = _problem(case)
    solved = u.solve_case(pb)
    good = sum(1 for x in solved.values() if x[2])
    print(f"{case}: {good} of {len(solved)} entries qualify")
    assert len(solved) == 3 * (pb.T - 2) and good >= 0.9 * len(solved)


def test_the_iteration_cap_and_a_lnl_that_is_not_finite():
    def f(t):  # 0.3 log t - t: its maximum is at 0.3
        return 0.3 * np.log(t) - t, 0.3 / t - 1.0, -0.3 / (t * t)
    t, n = u.optimise(f, 0.2)
    assert 0 < n < 10 and abs(t - 0.3) <= u.TOLERANCE
    t, n = u.optimise(f, 0.2, max_iterations=1)
    assert n == -1 and t == 0.2 - (0.3 / 0.2 - 1.0) / (-0.3 / (0.2 * 0.2))  # the first proposal
    t, n = u.optimise(lambda t: (-np.inf, np.nan, np.nan), 0.2)
    assert (t, n) == (0.2, -1)
    # a function that rises up to the upper bound is followed there by halving
    t, n = u.optimise(lambda t: (t, 1.0, -1e-9), 0.5, upper=1.0)
    assert n > 0 and 1.0 - t <= u.TOLERANCE
