"""CPU-only: the NumPy restatement of the NNI optimisation rule (tests/nni_optimize_util.py, which knows no state count) on the oracle
alone, on the seven 20-state cases of tests/test_nni_general_gpu.py that tests/test_nni_optimize_general_gpu.py compares the engine
with.  The one-row evaluator agrees with the definition at the tolerances of tests/test_nni_optimize_util.py -- also at 17 taxa,
where the GPU test takes d2 from it --; every entry ends inside the bounds after a positive count; every case has interior optima;
and at least 90 % of each case's entries qualify for the comparison of lengths there."""
import numpy as np
import pytest

import nni_optimize_util as u
from test_nni_general_gpu import CASES
from test_nni_optimize_general_gpu import _interior, _solved

ALL = sorted(CASES)


@pytest.mark.parametrize("case", ALL)
def test_the_one_row_evaluator_is_the_definition(case):
    pb, _, solved = _solved(case)
    rng = np.random.default_rng(1)
    entries = u.entries(pb)
    if pb.T >= 17:  # every fourth entry, which takes the arrangements in turn (the definition is three passes over the tree)
        entries = entries[::4]
    for k, v in entries:
        f = solved[(k, v)][3]
        for t in (1e-8, pb.branch_lengths[v] * rng.uniform(0.5, 2.0), 1.0):
            got, want = f(t), u.evaluate(pb, v, k, t)
            assert abs(got[0] - want[0]) <= 1e-12 * abs(want[0]), (k, v, t, got, want)
            assert abs(got[1] - want[1]) <= 1e-10 * max(1.0, abs(want[1])), (k, v, t, got, want)
            assert abs(got[2] - want[2]) <= 1e-10 * max(1.0, abs(want[2])), (k, v, t, got, want)


@pytest.mark.parametrize("case", ALL)
def test_nine_entries_in_ten_qualify(case):
    pb, _, solved = _solved(case)
    good = sum(1 for x in solved.values() if x[2])
    inside = sum(1 for x in solved.values() if _interior(x[0]))
    counts = [x[1] for x in solved.values()]
    print(f"{case}: {good} of {len(solved)} entries qualify, {inside} interior, iterations {min(counts)}..{max(counts)}")
    assert len(solved) == 3 * (pb.T - 2) and good >= 0.9 * len(solved)
    assert all(0 < n <= u.MAX_ITERATIONS and u.LOWER <= x[0] <= u.UPPER for x, n in zip(solved.values(), counts))
    assert inside >= 1, "no interior optimum in this case"
