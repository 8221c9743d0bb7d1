"""CPU-only: the restatement of phyamd_spr_optimize's rule (tests/spr_optimize_util.py) by itself.  A pass over the rearranged tree
with p, w and u marked visits (left[u], right[u], u), with p in the slot it had and w in the one the sibling had; the samples of the
37-taxon cases hold every class of move; and at least nine in ten entries of every case are qualified -- their three lengths after one
pass move by less than tolerance / 10 when every d1 and d2 of the pass is off by a relative 1e-9 either way -- so the GPU test compares
lengths on most of what it runs."""
import numpy as np
import pytest

import branch_optimize_util as b
import spr_optimize_util as t
import test_spr_gpu as s
from test_nni_gpu import _parents


@pytest.mark.parametrize("case", t.CASES)
def test_the_visit_order_is_left_right_then_u(case):
    pb, _ = t.problem(case)
    parent = _parents(pb)
    for p, w in t.entries(case):
        u = int(parent[p])
        q = t.rearranged(pb, parent, p, w)
        order = b.post_order(q, t.mask(pb, parent, p, w))
        assert order == [int(q.left[u]), int(q.right[u]), u], (p, w, order)
        assert {int(q.left[u]), int(q.right[u])} == {p, w}
        assert (q.left[u] == p) == (pb.left[u] == p)  # p keeps its slot; w has the slot s had


@pytest.mark.parametrize("case", t.CASES)
def test_the_entries_of_a_case(case):
    pb, _ = t.problem(case)
    parent, mask = _parents(pb), s._candidate_mask(pb)
    entries = t.entries(case)
    assert len(set(entries)) == len(entries) and all(mask[p, w] for p, w in entries)
    if pb.T <= 8:
        assert len(entries) == mask.sum()
    else:
        assert len(entries) == t.SAMPLE
        assert set().union(*(s._classes(pb, parent, p, w) for p, w in entries)) == set(s.CLASSES)


@pytest.mark.parametrize("case", t.CASES)
def test_nine_entries_in_ten_qualify(case):
    ref = t.one_pass_thrice(case)
    good = sum(1 for _, ok in ref.values() if ok)
    print(f"{case}: {good} of {len(ref)} entries qualify")
    assert good >= 0.9 * len(ref)
    for three, _ in ref.values():
        assert np.all((three >= t.LOWER) & (three <= t.UPPER))


def test_the_restatement_is_the_batch_optimisers_on_the_rearranged_tree():
    """run() returns the three marked lengths of branch_optimize_util.run, which leaves every other length alone"""
    pb, _ = t.problem("t8_random_p65")
    parent = _parents(pb)
    p, w = t.entries("t8_random_p65")[3]
    q = t.rearranged(pb, parent, p, w)
    lengths, lnl, initial, passes = b.run(q, t.mask(pb, parent, p, w))
    three, lnl2, initial2, passes2 = t.run(pb, parent, p, w)
    other = [n for n in range(pb.N) if n not in t.nodes(parent, p, w)]
    assert np.array_equal(lengths[other], q.branch_lengths[other]) and np.array_equal(three, lengths[t.nodes(parent, p, w)])
    assert (lnl, initial, passes) == (lnl2, initial2, passes2) and passes > 0 and lnl >= initial
    assert abs(initial - s._reference(pb, parent, p, w)) <= 1e-12 * abs(initial)
    assert abs(t.at_lengths(pb, parent, p, w, three).log_likelihood()["lnl"] - lnl) <= 1e-12 * abs(lnl)
