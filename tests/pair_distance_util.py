"""NumPy restatement of phyamd_pairwise_distances on the CPU.  No engine, no GPU.

A pair (i, j) is the two-tip tree with one branch of length t: L_k(t) = sum_c w_c sum_a (V^T (pi o m_i))_a (V^-1 m_j)_a exp(lambda_a r_c t),
m_i and m_j the two 0/1 state masks of pattern k.  L_k depends on k only through the pair of 4-bit masks, so the weighted 16 x 16
table of mask pairs (table, by np.add.at) is a sufficient statistic and f(t) = (lnL, d1, d2) is a sum over its bins (PairEvaluator).
oracle_problem is the same pair as a problem of the CPU oracle, which tests/test_pair_distance_util.py pins f against.  The rule is
nni_optimize_util.optimise, the stability of an answer nni_optimize_util.qualified."""
import numpy as np

import nni_optimize_util as nu
from oracle import phyoracle as po

START = 0.1


def masks_from_states(states):
    """[T][P] state codes -> 4-bit masks (bit s = state s; a code >= 4: every state)"""
    states = np.asarray(states)
    return np.where(states < 4, np.left_shift(1, np.minimum(states, 3)), 15).astype(np.uint8)


def masks_from_partials(partials):
    """[T][P][4] 0/1 partials -> 4-bit masks"""
    partials = np.asarray(partials)
    assert np.all((partials == 0) | (partials == 1))
    return (partials.astype(np.int64) @ np.array([1, 2, 4, 8])).astype(np.uint8)


def partials_from_masks(masks):
    return ((np.asarray(masks)[..., None] >> np.arange(4)) & 1).astype(np.float64)


def problem_masks(pb):
    return masks_from_partials(pb.tip_partials) if pb.tip_partials is not None else masks_from_states(pb.tip_states)


def all_pairs(T):
    return np.array([(i, j) for i in range(T) for j in range(i + 1, T)], dtype=np.int32)


def table(mask_i, mask_j, weights):
    """N[mi][mj] = sum_k w_k [mask_i[k] = mi][mask_j[k] = mj], the patterns added in pattern order"""
    n = np.zeros((16, 16))
    np.add.at(n, (mask_i, mask_j), weights)
    return n


def tables(masks, weights, pairs):
    return np.stack([table(masks[i], masks[j], weights) for i, j in pairs])


def coefficients(pb):
    """G[mi][mj][a] = (V^T (pi o mi))_a (V^-1 mj)_a"""
    m = partials_from_masks(np.arange(16))              # [16][4]
    g = (m * pb.freqs) @ pb.evec                         # [mi][a]
    q = m @ pb.ivec.T                                    # [mj][a]
    return g[:, None, :] * q[None, :, :]


class PairEvaluator:
    """t -> (lnl, d1, d2) of a pair from its table: the sums over the bins with N > 0 in bin order 16 mi + mj"""

    def __init__(self, pb, counts, G=None):
        G = coefficients(pb) if G is None else G
        keep = counts.reshape(256) > 0
        self.N, self.G, self.pb = counts.reshape(256)[keep], G.reshape(256, 4)[keep], pb

    def __call__(self, t):
        pb = self.pb
        x = np.outer(pb.cat_rates, pb.eval)              # [c][a] = lambda_a r_c
        e = pb.cat_props[:, None] * np.exp(x * t)
        S = np.stack([e.sum(0), (x * e).sum(0), (x * x * e).sum(0)])  # [n][a]
        F = self.G @ S.T                                 # [bin][n]
        with np.errstate(divide="ignore", invalid="ignore"):
            r1, r2 = F[:, 1] / F[:, 0], F[:, 2] / F[:, 0]
            return float(np.sum(self.N * np.log(F[:, 0]))), float(np.sum(self.N * r1)), float(np.sum(self.N * (r2 - r1 * r1)))


def oracle_problem(pb, i, j, t):
    """the pair as the oracle's two-tip tree: the root's children are taxon j on a branch of length t and taxon i on one of length 0,
    so that pi meets taxon i's mask: sum_s pi_s m_i[s] (P(t) m_j)_s"""
    part = partials_from_masks(problem_masks(pb)[[j, i]])
    return po.Problem([-1, -1, 0], [-1, -1, 1], 2, pb.weights, pb.eval, pb.evec, pb.ivec, pb.freqs, pb.cat_rates, pb.cat_props, [t, 0.0, 0.0], tip_partials=part)


def oracle_evaluate(pb, i, j, t):
    """(lnl, d1) of the pair at t by the oracle"""
    r = oracle_problem(pb, i, j, t).gradient()
    return r["lnl"], po.branch_gradient_from_cat(r["cat_grad"], pb.cat_rates, pb.cat_props)[0]


def solve_case(pb, pairs=None, start=None, weights=None, **kw):
    """every pair of pb by the rule on PairEvaluator: [(t*, iterations, qualified, the evaluator)] in the order of pairs (None: all
    i < j); start [count] or None: 0.1"""
    pairs = all_pairs(pb.T) if pairs is None else pairs
    masks, G = problem_masks(pb), coefficients(pb)
    out = []
    for p, (i, j) in enumerate(pairs):
        f = PairEvaluator(pb, table(masks[i], masks[j], pb.weights if weights is None else weights), G)
        s = START if start is None else start[p]
        t, n = nu.optimise(f, s, **kw)
        out.append((t, n, nu.qualified(f, s, t, **kw), f))
    return out
