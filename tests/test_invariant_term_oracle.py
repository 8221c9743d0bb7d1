"""CPU: pin the oracle's +I root term (oracle/phyoracle.py, root_invariant_term) before GPU tests are measured against it.

The term is d lnL / d pinv at fixed category rates, where pinv is the proportion of the invariant class (category 0, rate 0)
and the other C - 1 categories share 1 - pinv equally.  It is checked against a central difference of the oracle's lnL and
against the same sum formed pattern by pattern from the oracle's root partial, its scale factors and its per-pattern lnL.
"""
import numpy as np
import pytest

from gpu_util import random_problem
from oracle import phyoracle as po


def _with_pinv(pb, pinv):
    props = np.concatenate([[pinv], np.full(pb.C - 1, (1.0 - pinv) / (pb.C - 1))])
    return po.Problem(pb.left, pb.right, pb.root, pb.weights, pb.eval, pb.evec, pb.ivec, pb.freqs, pb.cat_rates, props, pb.branch_lengths,
                      tip_states=pb.tip_states, rescale=pb.rescale)


@pytest.mark.parametrize("C", [2, 4, 5])
@pytest.mark.parametrize("rescale", [0, 1])
def test_root_invariant_term_is_the_pinv_derivative(C, rescale):
    pinv = 0.3
    deep = rescale == 1  # long branches on a deeper tree: the oracle's scale factors are really used
    pb = random_problem(120 if deep else 16, 61, C, seed=500 + 10 * C + rescale, gaps=0.05, bl=(0.3, 0.9) if deep else (0.02, 0.2),
                        rescale=rescale, pinv=pinv)
    assert pb.cat_rates[0] == 0.0 and abs(pb.cat_props[0] - pinv) <= 1e-15 and abs(pb.cat_props.sum() - 1.0) <= 1e-15
    assert abs(pb.cat_rates @ pb.cat_props - 1.0) <= 1e-14
    r = pb.log_likelihood(want_lower=True)
    if deep:
        assert r["rescaled"] and np.any(r["scaling"][pb.root] != 0.0)
    got = po.root_invariant_term(pb)
    h = 1e-6
    fd = (_with_pinv(pb, pinv + h).log_likelihood()["lnl"] - _with_pinv(pb, pinv - h).log_likelihood()["lnl"]) / (2 * h)
    assert abs(got - fd) <= 1e-6 * abs(fd), (got, fd)
    # the same sum, pattern by pattern: 1 / L_k = exp(log scale factor of the root - lnL_k) in the units of the stored root partial
    root = r["lower"][pb.root]
    direct = 0.0
    for k in range(pb.P):
        s = sum(pb.freqs[i] * (root[0, k, i] - np.mean(root[1:, k, i])) for i in range(pb.S))
        direct += pb.weights[k] * s * np.exp(r["scaling"][pb.root, k] - r["pattern_lk"][k])
    assert abs(got - direct) <= 1e-10 * max(1.0, abs(direct)), (got, direct)


def test_random_problem_without_pinv_is_unchanged():
    """pinv=None consumes the generator as before: every existing seed gives the same problem."""
    a = random_problem(20, 50, 4, seed=3)
    rng = np.random.default_rng(3)
    from physher_amd import synth
    tree = synth.random_tree(20, rng, shape="random", bl_low=0.01, bl_high=0.1)
    synth.evolve(tree, 50, 4, rng)
    rng.integers(1, 5, size=50)
    rng.dirichlet(np.full(4, 5.0))
    rng.uniform(0.5, 3.0, size=(4, 4))
    rates = np.sort(rng.gamma(0.5, 2.0, size=4)) + 0.05
    rates = rates / (rates * 0.25).sum()
    np.testing.assert_array_equal(a.cat_rates, rates)
    np.testing.assert_array_equal(a.cat_props, np.full(4, 0.25))
    b = random_problem(20, 50, 4, seed=3, pinv=0.2)
    np.testing.assert_array_equal(a.tip_states, b.tip_states)  # (the rates are drawn last)
    assert b.cat_rates[0] == 0.0 and b.cat_props[0] == 0.2
