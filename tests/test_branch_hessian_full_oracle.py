"""The two restatements of the full branch-length Hessian (tests/full_hessian_util.py, what phyamd_branch_hessian is checked against
on the GPU), pinned on the CPU: against each other, against the restatement of the diagonal (tests/hessian_util.py), and -- the
brute-force one -- against five-point differences of the oracle's analytic branch gradient in every branch length.

Worst differences seen over the four cases: (a) against (b) 3.5e-15 of max(1, max|H|); diagonal and gradient against hessian_util
9.0e-15 (relative, per entry); (a) against the differences 2.2e-7 of max(1, max|H|) (bound 1e-6, the bound of
test_branch_hessian_oracle.py for the same kind of difference)."""
import copy

import numpy as np
import pytest

from full_hessian_util import brute_force, message_form
from gpu_util import random_problem
from hessian_util import branch_hessian_diagonal
from oracle import phyoracle as po

CASES = [  # T, P, C, shape, gaps, pinv, seed
    (7, 50, 1, "random", 0.0, None, 1),
    (8, 60, 2, "caterpillar", 0.05, None, 2),
    (9, 70, 4, "random", 0.05, None, 3),
    (10, 64, 4, "caterpillar", 0.03, 0.2, 4),
]
_cache = {}


def _case(i):
    """the problem and both restatements, computed once per case"""
    if i not in _cache:
        T, P, C, shape, gaps, pinv, seed = CASES[i]
        pb = random_problem(T, P, C, seed=seed, shape=shape, gaps=gaps, pinv=pinv)
        _cache[i] = (pb, brute_force(pb), message_form(pb))
    return _cache[i]


@pytest.mark.parametrize("i", range(len(CASES)))
def test_the_two_restatements_agree(i):
    pb, (la, ga, Ha), (lb, gb, Hb) = _case(i)
    scale = max(1.0, np.abs(Ha).max())
    assert la == pytest.approx(lb, rel=1e-12)
    print("a-b", np.abs(Ha - Hb).max() / scale, np.abs(ga - gb).max() / max(1.0, np.abs(ga).max()))
    assert np.abs(Ha - Hb).max() <= 1e-12 * scale
    assert np.abs(ga - gb).max() <= 1e-12 * max(1.0, np.abs(ga).max())


@pytest.mark.parametrize("i", range(len(CASES)))
def test_diagonal_gradient_symmetry_and_root(i):
    pb, a, b = _case(i)
    lnl, d1, d2 = branch_hessian_diagonal(pb)
    for l, g, H in (a, b):
        assert l == pytest.approx(lnl, rel=1e-12)
        print("diag", (np.abs(np.diag(H) - d2) / np.maximum(1.0, np.abs(d2))).max(), (np.abs(g - d1) / np.maximum(1.0, np.abs(d1))).max())
        assert np.all(np.abs(np.diag(H) - d2) <= 1e-12 * np.maximum(1.0, np.abs(d2)))
        assert np.all(np.abs(g - d1) <= 1e-12 * np.maximum(1.0, np.abs(d1)))
        assert np.array_equal(H, H.T)
        assert not H[pb.root].any() and not H[:, pb.root].any() and g[pb.root] == 0.0


def _branch_gradient(pb, b, dt):
    q = copy.copy(pb)
    q.branch_lengths = pb.branch_lengths.copy()
    q.branch_lengths[b] += dt
    return po.branch_gradient_from_cat(q.gradient()["cat_grad"], q.cat_rates, q.cat_props, zero_node=q.root)


@pytest.mark.parametrize("i", range(len(CASES)))
def test_brute_force_matches_differences_of_the_analytic_gradient(i):
    pb, (_, g, H), _ = _case(i)
    scale = max(1.0, np.abs(H).max())
    assert np.abs(g - _branch_gradient(pb, 0, 0.0)).max() <= 1e-10 * max(1.0, np.abs(g).max())
    worst = 0.0
    for b in range(pb.N):
        if b == pb.root:
            continue
        h = min(3e-4, 0.1 * pb.branch_lengths[b])
        f = [_branch_gradient(pb, b, dt) for dt in (-2 * h, -h, h, 2 * h)]
        column = (f[0] - 8 * f[1] + 8 * f[2] - f[3]) / (12 * h)
        worst = max(worst, np.abs(column - H[:, b]).max())
    print("differences", worst / scale)
    assert worst <= 1e-6 * scale
