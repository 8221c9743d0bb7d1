"""CPU-only: the NumPy restatement of phyamd_placement_log_likelihoods' table route (tests/placement_util.py) against the CPU
oracle's tree with T + 1 tips built from the definition, and physher_amd.placement's two helpers."""
import numpy as np
import pytest

import pair_distance_util as pu
import placement_util as u
from gpu_util import random_problem
from physher_amd import placement


def _small():
    pb = random_problem(5, 7, 2, seed=57, gaps=0.1)
    pb.weights = np.array([1.0, 3.0, 2.5, 1.0, 4.0, 0.5, 2.0])  # not uniform
    return pb


def test_the_table_route_matches_the_oracle_on_five_taxa():
    """5 taxa, 7 patterns, 2 categories: every (length, query, edge) at 1e-12 relative, for an inner split and both ends"""
    pb = _small()
    rng = np.random.default_rng(5)
    masks = u.random_masks(rng, 4, pb.P, gaps=0.15, ambiguous=0.2)
    masks[3] = 15  # an all-gap query: the base tree's own lnL on every edge
    pendants = [0.07, 0.9]
    worst = 0.0
    for sigma in (0.5, 0.25, 0.0, 1.0):
        got, ref = u.table_route(pb, masks, pendants, sigma), u.oracle_all(pb, masks, pendants, sigma)
        assert got.shape == ref.shape == (2, 4, pb.N)
        assert np.all(np.isnan(got[:, :, pb.root])) and np.isfinite(np.delete(got, pb.root, axis=2)).all()
        err = np.nanmax(np.abs(got - ref) / np.abs(ref))
        worst = max(worst, err)
        assert err <= 1e-12, (sigma, err)
    base = pb.log_likelihood()["lnl"]
    assert np.nanmax(np.abs(got[:, 3] - base)) <= 1e-12 * abs(base)
    print(f"worst relative lnL error {worst:.3e}")


def test_the_augmented_problem_is_the_definition():
    pb = _small()
    parent = u.parents(pb)
    n = next(v for v in u.edges(pb) if v >= pb.T)  # an internal edge
    row = np.full(pb.P, 4, dtype=np.uint8)
    q = u.augmented_problem(pb, n, row, 0.25, 0.3)
    T = pb.T
    new = lambda i: i if i < T else i + 1
    z = 2 * T
    assert q.T == T + 1 and q.N == pb.N + 2 and q.root == new(pb.root)
    assert {int(q.left[z]), int(q.right[z])} == {new(n), T}
    assert z in (int(q.left[new(parent[n])]), int(q.right[new(parent[n])]))
    assert abs(q.branch_lengths[new(n)] + q.branch_lengths[z] - pb.branch_lengths[n]) <= 1e-17
    assert q.branch_lengths[new(n)] == 0.25 * pb.branch_lengths[n] and q.branch_lengths[T] == 0.3
    assert np.array_equal(q.tip_partials[T], np.tile([0.0, 0.0, 1.0, 0.0], (pb.P, 1)))
    others = [v for v in range(pb.N) if v not in (n, pb.root)]
    assert np.array_equal(q.branch_lengths[[new(v) for v in others]], pb.branch_lengths[others])


def test_pruned_base_keeps_the_rest_of_the_tree():
    pb = random_problem(6, 9, 1, seed=3)
    parent = u.parents(pb)
    x = next(t for t in range(pb.T) if parent[t] != pb.root)
    base, new_id, row, tx = u.pruned_base(pb, x)
    assert base.T == pb.T - 1 and tx == pb.branch_lengths[x] and np.array_equal(row, pu.problem_masks(pb)[x])
    assert new_id[x] == -1 and new_id[parent[x]] == -1 and sorted(new_id[new_id >= 0]) == list(range(base.N))
    # the query back in its old place with the old lengths: the split that gives t_s back, and the original tree's lnL
    s = pb.right[parent[x]] if pb.left[parent[x]] == x else pb.left[parent[x]]
    sigma = pb.branch_lengths[s] / (pb.branch_lengths[s] + pb.branch_lengths[parent[x]])
    back = u.oracle_lnl(base, int(new_id[s]), row, sigma, tx)
    ref = pb.log_likelihood()["lnl"]
    assert abs(back - ref) <= 1e-12 * abs(ref)


def test_masks_from_states_is_the_engines_tip_encoding():
    codes = np.array([[0, 1, 2, 3, 4, 17, 255]], dtype=np.uint8)
    assert np.array_equal(placement.masks_from_states(codes), [[1, 2, 4, 8, 15, 15, 15]])
    assert placement.masks_from_states(codes).dtype == np.uint8
    assert np.array_equal(placement.masks_from_states(codes), pu.masks_from_states(codes))
    assert np.array_equal(placement.masks_from_states(np.array([-1, 3])), [15, 8])
    with pytest.raises(ValueError):
        placement.masks_from_states(np.array([0.5]))
    with pytest.raises(ValueError):
        placement.masks_from_states(codes, state_count=20)


def test_likelihood_weight_ratios():
    lnl = np.array([[-1000.0, np.nan, -1001.0, -np.inf, -1000.0],
                    [-np.inf, np.nan, -np.inf, -np.inf, -np.inf],
                    [-3.0e5, np.nan, -3.0e5 - 800.0, -2.0, -2.0]])
    w = placement.likelihood_weight_ratios(lnl)
    assert w.shape == lnl.shape and np.all(np.isfinite(w)) and np.all(w[:, 1] == 0.0) and w[0, 3] == 0.0
    e = np.exp(-1.0)
    assert np.allclose(w[0], np.array([1.0, 0.0, e, 0.0, 1.0]) / (2.0 + e), rtol=1e-15, atol=0.0)
    assert np.all(w[1] == 0.0)  # nothing finite: no weight anywhere
    assert np.array_equal(w[2], [0.0, 0.0, 0.0, 0.5, 0.5])
    assert abs(w[0].sum() - 1.0) <= 1e-15
    stacked = placement.likelihood_weight_ratios(np.stack([lnl, lnl]))
    assert np.array_equal(stacked[1], w)
    with pytest.raises(ValueError):
        placement.likelihood_weight_ratios(np.array([0.0, np.inf]))
