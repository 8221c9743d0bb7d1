"""CPU-only: the restatement of phyamd_spr_optimize_general's rule (tests/spr_optimize_general_util.py) by itself, on the seven 20-state
cases of tests/test_spr_general_gpu.py.  A pass over the rearranged tree with p, w and u marked visits (left[u], right[u], u), with p in
the slot it had and w in the one the sibling had; the two sampled cases hold every class of move; at least nine in ten entries of every
case are qualified -- their three lengths after one pass move by less than tolerance / 10 when every d1 and d2 of the pass is off by a
relative 1e-9 either way -- so the GPU test compares lengths on most of what it runs; and at least half of all entries stop by the
rule (passes > 0), so the GPU test's check of a further pass runs on most of them."""
import numpy as np
import pytest

import branch_optimize_util as b
import spr_optimize_general_util as t
import test_spr_general_gpu as g
import test_spr_gpu as s
from invalidation_util import parents as _parents


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
    if case in t.SAMPLED:
        assert len(entries) == t.SAMPLE
        assert set().union(*(g._all_classes(pb, parent, p, w) for p, w in entries)) == set(s.CLASSES) | set(g.MORE_CLASSES)
    else:
        assert len(entries) == mask.sum()


@pytest.mark.parametrize("case", t.CASES)
def test_nine_entries_in_ten_qualify(case):
    ref = t.one_pass_thrice(case)
    good = sum(1 for _, ok in ref.values() if ok)
    print(f"{case}: {good} of {len(ref)} entries qualify")
    assert good >= 0.9 * len(ref)
    for three, _ in ref.values():
        assert np.all((three >= t.LOWER) & (three <= t.UPPER))


def test_at_least_half_of_all_entries_stop_by_the_rule():
    stopped = total = 0
    for case in t.CASES:
        full = t.run_all(case)
        passes = [x[3] for x in full.values()]
        print(f"{case}: {len(full)} entries, passes {min(passes)}..{max(passes)}")
        stopped, total = stopped + sum(1 for k in passes if k > 0), total + len(passes)
        for three, lnl, initial, k in full.values():
            assert k != 0 and abs(k) <= t.MAX_PASSES and lnl >= initial and np.all((three >= t.LOWER) & (three <= t.UPPER))
    assert 2 * stopped >= total, (stopped, total)
