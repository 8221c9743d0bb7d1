"""CPU: the helpers of tests/invalidation_util.py pinned on the oracle alone, before tests/test_invalidation_gpu.py uses them as
yardsticks.  The problems are that file's three (4 states unscaled and rescaled, 20 states), built here without an engine."""
import functools

import numpy as np
import pytest

import invalidation_util as iu
from gpu_util import random_problem
from oracle import phyoracle as po

# name: (S, T, P, C, oracle rescale) -- the shapes of tests/test_invalidation_gpu.py
SHAPES = {"4s": (4, 9, 65, 2, 0), "4s_rescaled": (4, 9, 65, 2, 1), "20s": (20, 6, 17, 2, 0)}


@functools.lru_cache(maxsize=None)
def _problem(name):
    S, T, P, C, rescale = SHAPES[name]
    return random_problem(T, P, C, seed=500 + S + T, S=S, gaps=0.03, bl=(0.3, 0.9) if rescale else (0.01, 0.1), rescale=rescale)


def _perm(pb, seed=7):
    """a permutation of the internal ids that moves the root off the last id"""
    rng = np.random.default_rng(seed)
    while True:
        perm = np.concatenate([np.arange(pb.T), pb.T + rng.permutation(pb.T - 1)])
        if perm[pb.root] != pb.N - 1:
            return perm


@pytest.mark.parametrize("name", list(SHAPES))
def test_relabel_permutes_rows_and_nothing_else(name):
    pb = _problem(name)
    perm = _perm(pb)
    q = iu.relabel(pb, perm)
    assert q.root != q.N - 1 and q.root == perm[pb.root]
    assert np.all(q.left[:q.T] == -1) and np.all(q.right[:q.T] == -1)
    a, b = pb.gradient(), q.gradient()
    assert abs(a["lnl"] - b["lnl"]) <= 1e-13 * abs(a["lnl"])
    assert np.array_equal(a["pattern_lk"], b["pattern_lk"])  # (the same products in the same order: bit-equal)
    assert np.array_equal(a["cat_grad"], b["cat_grad"][perm])
    assert np.array_equal(pb.branch_lengths, q.branch_lengths[perm])


@pytest.mark.parametrize("name", list(SHAPES))
def test_neighbour_is_the_exchange_of_two_subtrees(name):
    """the neighbour has the same nodes, two of them with exchanged parents, and exchanging them again gives the tree back; its
    likelihood is the one of the rearranged arrays that tests/test_nni_gpu.py scores entry by entry"""
    pb = _problem(name)
    par = iu.parents(pb)
    v = next(n for n in range(pb.T, pb.N) if n != pb.root)
    u = par[v]
    s = pb.right[u] if pb.left[u] == v else pb.left[u]
    for which, moved in ((1, pb.left[v]), (2, pb.right[v])):
        q = iu.neighbour(pb, v, which)
        qpar = iu.parents(q)
        assert qpar[moved] == u and qpar[s] == v
        assert np.array_equal(np.delete(qpar, [moved, s]), np.delete(par, [moved, s]))
        assert np.array_equal(q.branch_lengths, pb.branch_lengths) and q.root == pb.root
        back = iu.neighbour(q, v, which)
        assert np.array_equal(iu.parents(back), par)
        assert q.log_likelihood()["lnl"] != pb.log_likelihood()["lnl"]
        left, right, bl = iu.rearranged(pb, v, which, pb.branch_lengths[v])
        assert np.array_equal(left, q.left) and np.array_equal(right, q.right) and np.array_equal(bl, q.branch_lengths)


@pytest.mark.parametrize("name", list(SHAPES))
def test_other_tree_changes_the_shape_in_both_directions(name):
    pb = _problem(name)
    cat, bal = iu.other_tree(pb, "caterpillar", 3), iu.other_tree(pb, "balanced", 4)
    for q in (cat, bal):
        par = iu.parents(q)
        assert np.sum(par < 0) == 1 and par[q.root] < 0 and np.all(par[np.arange(q.N) != q.root] >= q.T)
        assert q.tip_states is pb.tip_states and q.T == pb.T
        assert np.isfinite(q.log_likelihood()["lnl"])
    assert iu.levels(cat) == pb.T - 1 and iu.levels(bal) < iu.levels(cat)


@pytest.mark.parametrize("name", list(SHAPES))
def test_matrices_at_are_the_oracles(name):
    """the oracle forms P = p_t(lengths[n] * rate) itself (fill_matrices): prune on matrices_at equals the oracle (below), and the
    matrices are stochastic and those of the eigen system"""
    pb = _problem(name)
    m = iu.matrices_at(pb, pb.branch_lengths)
    assert m.shape == (pb.N, pb.C, pb.S, pb.S)
    np.testing.assert_allclose(m.sum(axis=3), 1.0, rtol=0, atol=1e-12)
    Q = iu.rate_matrix(pb)
    n, c = 1, pb.C - 1
    t = pb.branch_lengths[n] * pb.cat_rates[c]
    np.testing.assert_allclose(po.p_t(pb.S, pb.eval, pb.evec, pb.ivec, t, derivative=True), Q @ m[n, c], rtol=0, atol=1e-12)


@pytest.mark.parametrize("name", list(SHAPES))
def test_prune_is_the_oracle_on_the_oracles_matrices(name):
    """pins the convention: g[node][c] without w_c r_c"""
    pb = _problem(name)
    ref = pb.gradient()
    got = iu.prune(pb, iu.matrices_at(pb, pb.branch_lengths), iu.rate_matrix(pb))
    gmax = np.abs(ref["cat_grad"]).max()
    print(f"lnL {got['lnl']!r} oracle {ref['lnl']!r}; gradient {np.abs(got['cat_grad'] - ref['cat_grad']).max():.3e} of {gmax:.3e}")
    assert abs(got["lnl"] - ref["lnl"]) <= 1e-12 * abs(ref["lnl"])
    assert np.abs(got["pattern_lk"] - ref["pattern_lk"]).max() <= 1e-11
    assert np.abs(got["cat_grad"] - ref["cat_grad"]).max() <= 1e-11 * max(1.0, gmax)
    assert np.all(got["cat_grad"][pb.root] == 0.0)


@pytest.mark.parametrize("name", ["4s", "20s"])
def test_prune_follows_a_change_of_some_nodes_lengths(name):
    """matrices_at at other lengths for two nodes = the oracle with those two lengths replaced"""
    pb = _problem(name)
    other = pb.branch_lengths.copy()
    nodes = [0, next(n for n in range(pb.T, pb.N) if n != pb.root)]
    other[nodes] *= 1.7
    ref = iu.replace(pb, branch_lengths=other).gradient()
    mats = iu.matrices_at(pb, pb.branch_lengths)
    mats[nodes] = iu.matrices_at(pb, other)[nodes]
    got = iu.prune(pb, mats, iu.rate_matrix(pb))
    assert abs(got["lnl"] - ref["lnl"]) <= 1e-12 * abs(ref["lnl"])
    assert np.abs(got["cat_grad"] - ref["cat_grad"]).max() <= 1e-11 * max(1.0, np.abs(ref["cat_grad"]).max())
