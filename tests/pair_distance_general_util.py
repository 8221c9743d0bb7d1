"""NumPy restatement of phyamd_pairwise_distances_general on the CPU.  No engine, no GPU.

pair_distance_util.py with tip CLASSES in the place of 4-bit masks: a tip cell's class is a state (0..19), unknown (20: every state)
or 21 + q for ambiguity set q, the sets numbered in the order in which the engine meets them (tip by tip, pattern by pattern:
codes_from_problem).  With m_c the 0/1 vector of class c, a pair (i, j) is the two-tip tree with one branch of length t:
L_k(t) = sum_c w_c sum_a (V^T (pi o m_ci))_a (V^-1 m_cj)_a exp(lambda_a r_c t).  L_k depends on k only through the pair of classes, so
the weighted 32 x 32 table of class pairs (table, by np.add.at) is a sufficient statistic and f(t) = (lnL, d1, d2) is a sum over its
bins (PairEvaluator).  oracle_problem is the same pair as a problem of the CPU oracle with 20-state tip partials, which
tests/test_pair_distance_general_util.py pins f against.  The rule is nni_optimize_util.optimise, the stability of an answer
nni_optimize_util.qualified.  The cases of the GPU test are built here (CASES), so that the CPU pin runs on the same problems."""
import numpy as np

import nni_optimize_util as nu
from gpu_util import random_problem
from oracle import phyoracle as po
from pair_distance_util import all_pairs

START = 0.1
S, CLASSES, UNKNOWN = 20, 32, 20
SEGMENT = 4096


def class_members(sets):
    """uint64 [32]: bit s of entry c = state s is a member of class c; `sets` holds the ambiguity sets' member words in class order"""
    m = np.zeros(CLASSES, dtype=np.uint64)
    m[:S] = np.uint64(1) << np.arange(S, dtype=np.uint64)
    m[UNKNOWN] = (1 << S) - 1
    assert len(sets) <= CLASSES - S - 1
    m[S + 1:S + 1 + len(sets)] = np.array(sets, dtype=np.uint64)
    return m


def member_matrix(members):
    """[32][20] 0/1: the vectors m_c"""
    return ((np.asarray(members, dtype=np.uint64)[:, None] >> np.arange(S, dtype=np.uint64)) & np.uint64(1)).astype(np.float64)


def codes_from_problem(pb):
    """(codes uint8 [T][P], class_members uint64 [32]) as the engine forms them: from tip states a code >= 20 is unknown; from 0/1
    tip partials one member is that state, twenty members are unknown, and any other set gets the next free class the first time it
    is met, tip by tip and pattern by pattern"""
    if pb.tip_partials is None:
        return np.where(pb.tip_states < S, pb.tip_states, UNKNOWN).astype(np.uint8), class_members([])
    part = np.asarray(pb.tip_partials)
    assert np.all((part == 0) | (part == 1))
    words = part.astype(np.int64) @ (1 << np.arange(S, dtype=np.int64))
    ones = part.sum(axis=-1).astype(int)
    codes = np.zeros(words.shape, dtype=np.uint8)
    sets = []
    for t in range(pb.T):
        for k in range(pb.P):
            if ones[t, k] == 1:
                codes[t, k] = int(np.argmax(part[t, k]))
            elif ones[t, k] == S:
                codes[t, k] = UNKNOWN
            else:
                w = int(words[t, k])
                if w not in sets:
                    sets.append(w)
                codes[t, k] = S + 1 + sets.index(w)
    return codes, class_members(sets)


def table(code_i, code_j, weights):
    """N[ci][cj] = sum_k w_k [class_i[k] = ci][class_j[k] = cj], the patterns added in pattern order"""
    n = np.zeros((CLASSES, CLASSES))
    np.add.at(n, (code_i, code_j), weights)
    return n


def tables(codes, weights, pairs):
    return np.stack([table(codes[i], codes[j], weights) for i, j in pairs])


def coefficients(pb, members):
    """G[ci][cj][a] = (V^T (pi o m_ci))_a (V^-1 m_cj)_a"""
    m = member_matrix(members)                           # [32][20]
    g = (m * pb.freqs) @ pb.evec                         # [ci][a]
    q = m @ pb.ivec.T                                    # [cj][a]
    return g[:, None, :] * q[None, :, :]


class PairEvaluator:
    """t -> (lnl, d1, d2) of a pair from its table: the sums over the bins with N > 0 in bin order 32 ci + cj"""

    def __init__(self, pb, counts, G):
        keep = counts.reshape(-1) > 0
        self.N, self.G, self.pb = counts.reshape(-1)[keep], G.reshape(CLASSES * CLASSES, S)[keep], pb

    def __call__(self, t):
        pb = self.pb
        x = np.outer(pb.cat_rates, pb.eval)              # [c][a] = lambda_a r_c
        e = pb.cat_props[:, None] * np.exp(x * t)
        Sn = np.stack([e.sum(0), (x * e).sum(0), (x * x * e).sum(0)])  # [n][a]
        F = self.G @ Sn.T                                # [bin][n]
        with np.errstate(divide="ignore", invalid="ignore"):
            r1, r2 = F[:, 1] / F[:, 0], F[:, 2] / F[:, 0]
            return float(np.sum(self.N * np.log(F[:, 0]))), float(np.sum(self.N * r1)), float(np.sum(self.N * (r2 - r1 * r1)))


def oracle_problem(pb, i, j, t):
    """the pair as the oracle's two-tip tree (pair_distance_util.oracle_problem): the root's children are taxon j on a branch of
    length t and taxon i on one of length 0, so that pi meets taxon i's vector"""
    codes, members = codes_from_problem(pb)
    part = member_matrix(members)[codes[[j, i]]]
    return po.Problem([-1, -1, 0], [-1, -1, 1], 2, pb.weights, pb.eval, pb.evec, pb.ivec, pb.freqs, pb.cat_rates, pb.cat_props, [t, 0.0, 0.0], tip_partials=part)


def oracle_evaluate(pb, i, j, t):
    """(lnl, d1) of the pair at t by the oracle"""
    r = oracle_problem(pb, i, j, t).gradient()
    return r["lnl"], po.branch_gradient_from_cat(r["cat_grad"], pb.cat_rates, pb.cat_props)[0]


def solve_case(pb, pairs=None, start=None, weights=None, **kw):
    """every pair of pb by the rule on PairEvaluator: [(t*, iterations, qualified, the evaluator)] in the order of pairs (None: all
    i < j); start [count] or None: 0.1"""
    pairs = all_pairs(pb.T) if pairs is None else pairs
    codes, members = codes_from_problem(pb)
    G = coefficients(pb, members)
    out = []
    for p, (i, j) in enumerate(pairs):
        f = PairEvaluator(pb, table(codes[i], codes[j], pb.weights if weights is None else weights), G)
        s = START if start is None else start[p]
        t, n = nu.optimise(f, s, **kw)
        out.append((t, n, nu.qualified(f, s, t, **kw), f))
    return out


# --- the cases ---------------------------------------------------------------------------------------------------------------------

def partials_from_states(states):
    """[T][P] state codes -> [T][P][20] 0/1 partials (a code >= 20: every state)"""
    states = np.asarray(states)
    return np.where((states < S)[..., None], np.arange(S) == states[..., None], True).astype(np.float64)


def with_sets(pb, count, fraction, seed):
    """pb with `fraction` of its cells replaced by one of `count` random ambiguity sets (each state a member with probability 0.3,
    redrawn until the set has 2..19 members and differs from the others), as 0/1 tip partials"""
    rng = np.random.default_rng(seed)
    sets = []
    while len(sets) < count:
        m = rng.random(S) < 0.3
        if 2 <= m.sum() <= S - 1 and not any(np.array_equal(m, x) for x in sets):
            sets.append(m)
    part = partials_from_states(pb.tip_states)
    pick = rng.random(pb.tip_states.shape) < fraction
    which = rng.integers(0, count, size=pb.tip_states.shape)
    part[pick] = np.array(sets, dtype=np.float64)[which[pick]]
    pb.tip_partials = part
    return pb


def _case_b():
    pb = with_sets(random_problem(9, 130, 4, 21, S=S, gaps=0.05, bl=(0.05, 0.3)), 11, 0.1, 121)
    assert set(codes_from_problem(pb)[0].ravel().tolist()) == set(range(CLASSES))  # every row and column of the table
    return pb


def wag_problem():
    """six taxa x fifty patterns under the project's own WAG + Gamma(4): the zero eigenvalue and the real model's eigenvalue spread"""
    from physher_amd import _phycpp_amd as pc
    pb = random_problem(6, 50, 4, 27, S=S, gaps=0.1, bl=(0.05, 0.3))
    m = pc.substitution_model("WAG")
    site = pc.GammaSiteModelInterface(0.5, 4, None, None)
    return po.Problem(pb.left, pb.right, pb.root, pb.weights, m["eval"], m["evec"], m["ivec"], m["frequencies"], site.rates(), site.proportions(), pb.branch_lengths,
                      tip_states=pb.tip_states)


CASES = {
    "A_t6_p50_c1": lambda: random_problem(6, 50, 1, 20, S=S, gaps=0.1, bl=(0.05, 0.3)),                    # one category
    "B_t9_p130_sets": _case_b,                                            # eight rounds + 2 patterns, every class: both hi tiles
    "C_t7_p70_few_sets": lambda: with_sets(random_problem(7, 70, 2, 22, S=S), 3, 0.05, 122),
    "D_t8_p100_saturated": lambda: random_problem(8, 100, 2, 23, S=S, gaps=0.1, bl=(1.0, 5.0)),
    "E_t8_p40_identical": lambda: random_problem(8, 40, 4, 24, S=S, bl=(1e-5, 1e-4)),
    "F_t4_two_segments": lambda: with_sets(random_problem(4, SEGMENT + 70, 4, 25, S=S, gaps=0.05), 2, 0.02, 125),
    "G_t6_p50_c12": lambda: random_problem(6, 50, 12, 26, S=S, gaps=0.1),
    "W_t6_p50_wag": wag_problem,
}
