"""CPU-only: the NumPy restatement of phyamd_placement_log_likelihoods_general's table route (tests/placement_general_util.py)
against the CPU oracle's tree with T + 1 tips built from the definition, at 1e-10 relative on two small cases -- the restatement
is pinned before the kernel is -- and physher_amd.placement's helpers on 20-state results."""
import numpy as np
import pytest

import pair_distance_general_util as gu
import placement_general_util as u
from gpu_util import random_problem
from physher_amd import placement


def _states_case():
    pb = random_problem(5, 7, 2, seed=57, S=20, gaps=0.1)
    pb.weights = np.array([1.0, 3.0, 2.5, 1.0, 4.0, 0.5, 2.0])  # not uniform
    return pb


def _sets_case():
    """reference tips from ambiguous partials (three engine sets), one category"""
    return gu.with_sets(random_problem(4, 9, 1, seed=58, S=20, gaps=0.1), 3, 0.2, 158)


@pytest.mark.parametrize("make, set_count", [(_states_case, 2), (_sets_case, 11)], ids=["states_two_sets", "partials_eleven_sets"])
def test_the_table_route_matches_the_oracle(make, set_count):
    pb = make()
    rng = np.random.default_rng(5)
    sets = u.random_sets(rng, set_count)
    codes = u.random_codes(rng, 4, pb.P, set_count, unknown=0.15, in_sets=0.3)
    codes[3] = u.UNKNOWN  # an all-unknown query: the base tree's own lnL on every edge
    if set_count == u.MAX_SETS:
        codes[2, :] = (21 + np.arange(pb.P)) % 32  # the highest classes
        codes[2] = np.where(codes[2] < 21, 31, codes[2])
    pendants = [0.07, 0.9]
    worst = 0.0
    for sigma in (0.5, 0.25, 0.0, 1.0):
        got, ref = u.table_route(pb, codes, sets, pendants, sigma), u.oracle_all(pb, codes, sets, pendants, sigma)
        assert got.shape == ref.shape == (2, 4, pb.N)
        assert np.all(np.isnan(got[:, :, pb.root])) and np.isfinite(np.delete(got, pb.root, axis=2)).all()
        err = np.nanmax(np.abs(got - ref) / np.abs(ref))
        worst = max(worst, err)
        assert err <= 1e-10, (sigma, err)
    base = pb.log_likelihood()["lnl"]
    assert np.nanmax(np.abs(got[:, 3] - base)) <= 1e-10 * abs(base)
    print(f"worst relative lnL error {worst:.3e}")


def test_the_augmented_problem_is_the_definition():
    pb = _sets_case()
    parent = u.parents(pb)
    n = next(v for v in u.edges(pb) if v >= pb.T)  # an internal edge
    sets = u.random_sets(np.random.default_rng(1), 2)
    row = np.array([0, 19, 20, 21, 22, 5, 20, 21, 3], dtype=np.uint8)
    q = u.augmented_problem(pb, n, row, sets, 0.25, 0.3)
    T = pb.T
    new = lambda i: i if i < T else i + 1
    z = 2 * T
    assert q.T == T + 1 and q.N == pb.N + 2 and q.root == new(pb.root)
    assert {int(q.left[z]), int(q.right[z])} == {new(n), T}
    assert z in (int(q.left[new(parent[n])]), int(q.right[new(parent[n])]))
    assert abs(q.branch_lengths[new(n)] + q.branch_lengths[z] - pb.branch_lengths[n]) <= 1e-17
    assert q.branch_lengths[T] == 0.3 and q.branch_lengths[new(n)] == 0.25 * pb.branch_lengths[n]
    part = np.asarray(q.tip_partials)
    assert part.shape == (T + 1, pb.P, 20) and np.array_equal(part[:T], np.asarray(pb.tip_partials))
    assert part[T, 0].sum() == 1 and part[T, 0, 0] == 1 and part[T, 1, 19] == 1 and np.all(part[T, 2] == 1)
    members = lambda w: [(int(w) >> s) & 1 for s in range(20)]
    assert list(part[T, 3]) == members(sets[0]) and list(part[T, 4]) == members(sets[1])


def test_the_tables_hold_zero_for_dead_classes_and_weightless_patterns():
    pb = _states_case()
    pb.weights[2] = 0.0
    sets = u.random_sets(np.random.default_rng(2), 1)
    tab = u.tables(pb, sets, [0.1], 0.5)
    assert tab.shape == (1, pb.N, pb.P, 32)
    assert np.all(tab[:, :, :, 22:] == 0) and np.all(tab[:, :, 2] == 0) and np.all(tab[:, pb.root] == 0)
    live = np.delete(np.delete(tab, pb.root, axis=1), 2, axis=2)[..., :22]
    assert np.all(np.isfinite(live)) and np.all(live < 0)


def test_codes_from_protein():
    codes, sets = placement.codes_from_protein(["ACDY", "bzjx", "-?*w"])
    assert codes.dtype == np.uint8 and codes.shape == (3, 4) and sets.dtype == np.uint64 and sets.shape == (3,)
    assert codes.tolist() == [[0, 1, 2, 19], [21, 22, 23, 20], [20, 20, 20, 18]]
    aa = placement.AMINO_ACIDS
    word = lambda letters: sum(1 << aa.index(x) for x in letters)
    assert sets.tolist() == [word("DN"), word("EQ"), word("IL")]
    assert codes.max() <= 20 + len(sets)
    with pytest.raises(ValueError):
        placement.codes_from_protein(["AC", "A"])


def test_the_result_helpers_work_on_twenty_state_scores():
    """likelihood_weight_ratios and top_candidates take the call's [Q][N] scores unchanged: here the restatement's"""
    pb = _states_case()
    rng = np.random.default_rng(3)
    codes = u.random_codes(rng, 3, pb.P)
    lnl = u.table_route(pb, codes, [], [0.2], 0.5)[0]
    lwr = placement.likelihood_weight_ratios(lnl)
    assert lwr.shape == lnl.shape and np.all(lwr[:, pb.root] == 0) and np.allclose(lwr.sum(axis=1), 1.0)
    cand = placement.top_candidates(lnl, 2)
    assert cand.shape == (6, 2) and np.all(cand[:, 1] != pb.root)
    assert np.array_equal(cand[::2, 1], np.nanargmax(lnl, axis=1))
