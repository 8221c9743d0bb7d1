"""CPU-only: the NumPy restatement of phyamd_optimize_branch_lengths' rule (tests/branch_optimize_util.py) on the oracle alone.  The
edge evaluator agrees with the definition at every node, tips included; lnL never falls from visit to visit; a converged run leaves
every interior branch at a maximum (d2 < 0 by the oracle); and on every case tests/test_branch_optimize_gpu.py compares lengths on,
at least nine visits, or branches of a pass, in ten are stable under relative errors of 1e-9 on d1 and d2."""
import numpy as np
import pytest

import branch_optimize_util as b
from hessian_util import branch_hessian_diagonal
from oracle.phyoracle import branch_gradient_from_cat


def interior(t):
    return b.LOWER + 2 * b.TOLERANCE < t < b.UPPER - 2 * b.TOLERANCE


@pytest.mark.parametrize("case", ["t2", "t3", "t8_relabelled_p65", "t8_caterpillar_p64"])
def test_the_edge_evaluator_is_the_definition(case):
    pb = b.problem(case)
    rng = np.random.default_rng(1)
    for n in b.post_order(pb):
        f = b.Edge(pb, n)
        for t in (1e-8, pb.branch_lengths[n] * rng.uniform(0.5, 2.0), 1.0):
            q = b.with_lengths(pb, pb.branch_lengths)
            q.branch_lengths[n] = t
            r = q.gradient()
            want = (r["lnl"], branch_gradient_from_cat(r["cat_grad"], pb.cat_rates, pb.cat_props)[n], branch_hessian_diagonal(q)[2][n])
            got = f(t)
            assert abs(got[0] - want[0]) <= 1e-12 * abs(want[0]), (n, t, got, want)
            assert abs(got[1] - want[1]) <= 1e-10 * max(1.0, abs(want[1])), (n, t, got, want)
            assert abs(got[2] - want[2]) <= 1e-10 * max(1.0, abs(want[2])), (n, t, got, want)


def test_the_visits_are_the_post_order():
    pb = b.problem("t8_relabelled_p65")
    order = b.post_order(pb)
    assert sorted(order) == [n for n in range(pb.N) if n != pb.root]
    at = {n: i for i, n in enumerate(order)}
    for n in range(pb.T, pb.N):
        if n != pb.root:
            assert at[pb.left[n]] < at[pb.right[n]] < at[n]
    mask = np.zeros(pb.N, dtype=bool)
    mask[[0, pb.root, order[-1]]] = True
    assert b.post_order(pb, mask) == [0, order[-1]]


@pytest.mark.parametrize("case", ["t8_balanced_p65", "t8_relabelled_p64"])
def test_lnl_never_falls_and_a_converged_run_is_at_a_maximum(case):
    pb = b.problem(case)
    q = b.with_lengths(pb, b.start_lengths(pb))
    trace = [q.log_likelihood()["lnl"]]
    b.one_pass(q, trace=trace)
    assert len(trace) == pb.N and all(y >= x - 1e-12 * abs(x) for x, y in zip(trace, trace[1:])), trace
    assert trace[-1] > trace[0] + 1.0
    lengths, lnl, initial, passes = b.run(b.with_lengths(pb, b.start_lengths(pb)))
    assert 1 < passes <= b.MAX_PASSES and lnl >= trace[-1] and initial == trace[0]
    done = b.with_lengths(pb, lengths)
    assert abs(done.log_likelihood()["lnl"] - lnl) <= 1e-12 * abs(lnl)
    d2 = branch_hessian_diagonal(done)[2]
    inside = [n for n in b.post_order(pb) if interior(lengths[n])]
    assert len(inside) >= pb.T and all(d2[n] < 0 for n in inside), (lengths, d2)
    # a further pass gains no more than the tolerance the run stopped on
    again = b.with_lengths(pb, lengths)
    assert b.one_pass(again)[1] - lnl <= b.LNL_TOLERANCE


def test_the_caps_and_an_empty_mask():
    pb = b.with_lengths(b.problem("t8_random_p65"), b.start_lengths(b.problem("t8_random_p65")))
    lengths, lnl, initial, passes = b.run(pb, max_passes=1)
    assert passes == -1 and lnl > initial
    lengths, lnl, initial, passes = b.run(pb, max_passes=3, max_iterations=1)
    assert lnl >= initial
    lengths, lnl, initial, passes = b.run(pb, mask=np.zeros(pb.N, dtype=bool))
    assert passes == 0 and lnl == initial and np.array_equal(lengths, pb.branch_lengths)


@pytest.mark.parametrize("case", b.T8)
def test_nine_visits_in_ten_qualify(case):
    visits = b.one_visit(case)
    good = sum(1 for _, ok in visits.values() if ok)
    print(f"{case}: {good} of {len(visits)} visits qualify")
    assert len(visits) == 14 and good >= 0.9 * len(visits)


@pytest.mark.parametrize("case", b.PASS_CASES)
def test_nine_branches_of_a_pass_in_ten_qualify(case):
    pb = b.problem(case)
    lengths, good = b.one_pass_thrice(case)
    print(f"{case}: {int(good.sum())} of {pb.N - 1} branches qualify")
    assert good.sum() >= 0.9 * (pb.N - 1)
    assert all(b.LOWER <= lengths[n] <= b.UPPER for n in b.post_order(pb))
