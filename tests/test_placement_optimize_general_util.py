"""CPU-only: the restatement of phyamd_placement_optimize_general's rule (tests/placement_optimize_general_util.py) by itself.  A pass
over the placed tree with n, x and z marked visits (n, x, z); the lnL of the start is placement_general_util.oracle_lnl's; the
whole rule is monotone and ends with a pass count; and the conditions the GPU test relies on hold for the cases' seeds: at least
nine in ten entries of every case are qualified -- their three lengths after one pass move by less than tolerance / 10 when every d1
and d2 of the pass is off by a relative 1e-9 either way --, at least one entry of every case is stopped by the rule and not by the
cap of max_passes, and so is at least half of all entries.  The counts are printed per case."""
import numpy as np
import pytest

import branch_optimize_util as b
import placement_general_util as u
import placement_optimize_general_util as t


@pytest.mark.parametrize("name", sorted(t.CASES))
def test_the_visit_order_is_n_x_z(name):
    pb, _, codes, sets, split, cands = t.case(name)
    for q, n in cands:
        p = t.placed(pb, n, codes[q], sets, t.start(pb, n, split), t.reference(name))
        three = t.nodes(pb, n)
        assert [int(p.left[three[2]]), int(p.right[three[2]])] == three[:2]
        assert b.post_order(p, t.mask(pb, n)) == three, (q, n)
        assert b.post_order(p, t.mask(pb, n, 5)) == [three[0], three[2]] and b.post_order(p, t.mask(pb, n, 2)) == [three[1]]


def test_the_cases_are_the_tabled_ones():
    shapes = {c: t.CASES[c][:4] for c in t.CASES}
    assert shapes == {"t2_p5_c1": (2, "random", 5, 1), "t3_p16_c4": (3, "random", 16, 4), "t3_p17_c2": (3, "random", 17, 2), "t9_p130_c8": (9, "random", 130, 8),
                      "t9_caterpillar_p70_c4": (9, "caterpillar", 70, 4), "t5_p300_c2": (5, "random", 300, 2), "t4_p66_c1_twice": (4, "random", 66, 1)}
    assert t.CASES["t3_p16_c4"][7] == 3 and t.CASES["t9_p130_c8"][4:] == (1, 0.5, 3, 11, 0) and t.CASES["t9_caterpillar_p70_c4"][5] == 0.3
    assert t.CASES["t5_p300_c2"][6:8] == (2, 4) and t.CASES["t4_p66_c1_twice"][8] == 5
    for name in t.CASES:
        pb, tip_mode, codes, sets, _, cands = t.case(name)
        assert pb.S == 20 and codes.shape == (t.CASES[name][4], pb.P) and len(sets) == t.CASES[name][7] and codes.max() <= 20 + len(sets)
        assert set(t.distinct(name)) == {(q, n) for q in range(len(codes)) for n in u.edges(pb)}  # every (query, edge)
        assert len(cands) - len(t.distinct(name)) == t.CASES[name][8]
        assert (tip_mode == "partials") == bool(t.CASES[name][6])
    codes = t.case("t9_p130_c8")[2]
    assert set(range(21, 32)) <= set(codes[0].tolist())  # one row with the highest classes
    name, row = t.ALL_UNKNOWN
    assert np.all(t.case(name)[2][row] == u.UNKNOWN)


@pytest.mark.parametrize("name", ["t3_p16_c4", "t9_caterpillar_p70_c4", "t5_p300_c2"])
def test_initial_is_the_placement_calls_entry(name):
    pb, _, codes, sets, split, cands = t.case(name)
    for q, n in cands[::3]:
        _, lnl, initial, passes = t.run(pb, n, codes[q], sets, split, reference=t.reference(name), max_passes=1)
        ref = u.oracle_lnl(pb, n, codes[q], sets, split, t.PENDANT, t.reference(name))
        assert abs(initial - ref) <= 1e-12 * abs(ref) and lnl >= initial and abs(passes) == 1


@pytest.mark.parametrize("name", ["t2_p5_c1", "t3_p16_c4"])
def test_the_whole_rule_is_monotone_and_ends_with_a_pass_count(name):
    """passes > 0: the stop test held after that pass; -MAX_PASSES: the cap (slow climbs along the distal / proximal ridge exist)"""
    pb, _, codes, sets, split, _ = t.case(name)
    for (q, n), (three, lnl, initial, passes) in t.full_runs(name).items():
        assert 0 < passes <= t.MAX_PASSES or passes == -t.MAX_PASSES, (q, n, passes)
        assert lnl >= initial and np.all((three >= t.LOWER) & (three <= t.UPPER))
        trace, p = [], t.placed(pb, n, codes[q], sets, t.start(pb, n, split), t.reference(name))
        assert b.one_pass(p, t.mask(pb, n), trace=trace)[0] is None
        assert len(trace) == 3 and trace[0] >= initial and trace[1] >= trace[0] and trace[2] >= trace[1], (q, n, initial, trace)


@pytest.mark.parametrize("name", sorted(t.CASES))
def test_the_conditions_on_the_case_hold(name):
    ref, runs = t.one_pass_thrice(name), t.full_runs(name)
    good = sum(1 for _, ok in ref.values() if ok)
    by_rule = sum(1 for r in runs.values() if r[3] > 0)
    capped = sum(1 for r in runs.values() if r[3] == -t.MAX_PASSES)
    print(f"{name}: {good} of {len(ref)} entries qualify; {by_rule} stop by the rule, {capped} reach the cap of {t.MAX_PASSES} passes")
    assert by_rule + capped == len(runs)
    assert good >= 0.9 * len(ref)
    assert by_rule >= 1
    for three, _ in ref.values():
        assert np.all((three >= t.LOWER) & (three <= t.UPPER))


def test_half_of_all_entries_stop_by_the_rule():
    runs = [r for name in sorted(t.CASES) for r in t.full_runs(name).values()]  # (computed once: shared with the per-case test)
    stopped = sum(1 for r in runs if r[3] > 0)
    print(f"all cases: {stopped} of {len(runs)} entries stop by the rule")
    assert 2 * stopped >= len(runs)


@pytest.mark.parametrize("case,branches", [("t9_caterpillar_p70_c4", 2), ("t9_caterpillar_p70_c4", 5), ("t5_p300_c2", 2)])
def test_nine_entries_in_ten_qualify_with_a_subset(case, branches):
    ref = t.one_pass_thrice(case, branches)
    good = sum(1 for _, ok in ref.values() if ok)
    print(f"{case}, branches {branches}: {good} of {len(ref)} entries qualify")
    assert good >= 0.9 * len(ref)
