"""CPU-only: the restatement of phyamd_placement_optimize's rule (tests/placement_optimize_util.py) by itself.  A pass over the placed
tree with n, x and z marked visits (n, x, z); the lnL of the start is placement_util.oracle_lnl's; a subset of the branches leaves
the other lengths alone; and at least nine in ten candidates of every case are qualified -- their three lengths after one pass move
by less than tolerance / 10 when every d1 and d2 of the pass is off by a relative 1e-9 either way -- so the GPU test compares
lengths on most of what it runs."""
import numpy as np
import pytest

import branch_optimize_util as b
import placement_optimize_util as t
import placement_util as u


@pytest.mark.parametrize("name", sorted(t.CASES))
def test_the_visit_order_is_n_x_z(name):
    pb, _, masks, split, cands = t.case(name)
    for q, n in cands:
        p = t.placed(pb, n, masks[q], t.start(pb, n, split))
        three = t.nodes(pb, n)
        assert [int(p.left[three[2]]), int(p.right[three[2]])] == three[:2]
        assert b.post_order(p, t.mask(pb, n)) == three, (q, n)
        assert b.post_order(p, t.mask(pb, n, 5)) == [three[0], three[2]] and b.post_order(p, t.mask(pb, n, 2)) == [three[1]]


def test_the_cases_are_the_tabled_ones():
    assert [t.CASES[c][:6] for c in t.TABLED] == [(2, "random", 5, 1, 3, 0.5), (3, "random", 64, 4, 5, 0.25), (9, "random", 130, 8, 4, 0.5),
                                                  (9, "caterpillar", 70, 4, 4, 0.3), (9, "random", 65, 2, 4, 0.7)]
    for name in t.CASES:
        pb, _, masks, _, cands = t.case(name)
        distinct = set(map(tuple, cands.tolist()))
        assert distinct == {(q, n) for q in range(len(masks)) for n in u.edges(pb)}  # every (query, edge)
        assert len(cands) - len(distinct) == t.CASES[name][7]
    assert any(t.CASES[c][6] for c in t.CASES) and any(t.CASES[c][7] for c in t.CASES)
    assert t.case("t5_p70_c2_ambiguous")[0].tip_states is None


@pytest.mark.parametrize("name", ["t3_p64_c4", "t9_caterpillar_p70_c4", "t5_p70_c2_ambiguous"])
def test_initial_is_the_placement_calls_entry(name):
    pb, _, masks, split, cands = t.case(name)
    for q, n in cands[::3]:
        _, lnl, initial, passes = t.run(pb, n, masks[q], split, max_passes=1)
        ref = u.oracle_lnl(pb, n, masks[q], split, t.PENDANT)
        assert abs(initial - ref) <= 1e-12 * abs(ref) and lnl >= initial and abs(passes) == 1


def test_a_subset_of_the_branches_leaves_the_others_alone():
    pb, _, masks, split, cands = t.case("t9_p65_c2")
    q, n = cands[7]
    s = t.start(pb, n, split)
    full, lnl7, initial7, _ = t.run(pb, n, masks[q], split)
    for branches in (1, 2, 4, 5, 3, 6):
        three, lnl, initial, passes = t.run(pb, n, masks[q], split, branches)
        marked = np.array([bool(branches >> k & 1) for k in range(3)])
        assert np.array_equal(three[~marked], s[~marked]) and np.all(three[marked] != s[marked]), (branches, three, s)
        assert initial == initial7 and initial <= lnl <= lnl7 + 1e-6 and passes > 0
        assert abs(t.placed(pb, n, masks[q], three).log_likelihood()["lnl"] - lnl) <= 1e-12 * abs(lnl)
    assert np.all(full != s)


@pytest.mark.parametrize("name", sorted(t.CASES))
def test_nine_entries_in_ten_qualify(name):
    ref = t.one_pass_thrice(name)
    good = sum(1 for _, ok in ref.values() if ok)
    print(f"{name}: {good} of {len(ref)} entries qualify")
    assert good >= 0.9 * len(ref)
    for three, _ in ref.values():
        assert np.all((three >= t.LOWER) & (three <= t.UPPER))


@pytest.mark.parametrize("branches", [2, 5])
def test_nine_entries_in_ten_qualify_with_a_subset(branches):
    ref = t.one_pass_thrice("t9_p65_c2", branches)
    good = sum(1 for _, ok in ref.values() if ok)
    print(f"t9_p65_c2, branches {branches}: {good} of {len(ref)} entries qualify")
    assert good >= 0.9 * len(ref)


def test_the_whole_rule_ends_with_a_pass_count():
    """passes > 0: the stop test held after that pass; -MAX_PASSES: the cap (slow climbs along the distal / proximal ridge exist)"""
    pb, _, masks, split, cands = t.case("t3_p64_c4")
    results = [t.run(pb, n, masks[q], split) for q, n in cands]
    print("passes:", [r[3] for r in results])
    assert all(0 < r[3] <= t.MAX_PASSES or r[3] == -t.MAX_PASSES for r in results)
    assert all(r[1] >= r[2] for r in results) and any(0 < r[3] < t.MAX_PASSES for r in results)
