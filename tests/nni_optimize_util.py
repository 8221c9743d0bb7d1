"""NumPy restatement of phyamd_nni_optimize's rule on the CPU oracle.  No engine, no GPU.

An entry (k, v) is NNI arrangement k of the internal node v (invalidation_util.rearranged); its lnL, d1 and d2 at a central length t
are, by definition (evaluate): the oracle's lnL of the rearranged tree, the oracle's per-category gradient through
branch_gradient_from_cat at row v, and hessian_util.branch_hessian_diagonal's d2 at row v.  EdgeEvaluator gives the same three
numbers from the oracle's partials of the rearranged tree at v alone -- hessian_util's formulas for the one row, the partials taken
once because they do not depend on t_v -- so that an iteration costs one small product instead of three passes over the tree; it
is pinned against evaluate in tests/test_nni_optimize_util.py.  optimise is the rule itself, in the words of the header."""
import copy

import numpy as np

from hessian_util import branch_hessian_diagonal
from invalidation_util import rearranged
from oracle.phyoracle import branch_gradient_from_cat

TOLERANCE, LOWER, UPPER, MAX_ITERATIONS = 1e-8, 1e-8, 10.0, 100


def candidates(pb):
    return [v for v in range(pb.T, pb.N) if v != pb.root]


def entries(pb):
    return [(k, v) for v in candidates(pb) for k in range(3)]


def rearranged_problem(pb, v, k, t):
    q = copy.copy(pb)
    q.left, q.right, q.branch_lengths = rearranged(pb, v, k, t)
    return q


def evaluate(pb, v, k, t):
    """(lnl, d1, d2) of entry (k, v) at central length t: the definition"""
    q = rearranged_problem(pb, v, k, t)
    r = q.gradient()
    d1 = branch_gradient_from_cat(r["cat_grad"], pb.cat_rates, pb.cat_props)[v]
    return r["lnl"], d1, branch_hessian_diagonal(q)[2][v]


class EdgeEvaluator:
    """t -> (lnl, d1, d2) of entry (k, v), from the oracle's lower and upper partial of the rearranged tree at v"""

    def __init__(self, pb, v, k):
        q = rearranged_problem(pb, v, k, pb.branch_lengths[v])
        r = q.gradient(want_partials=True)
        assert not r["rescaled"]
        self.pb, self.lower = pb, r["lower"][v]
        self.fu = r["upper"][v] * pb.freqs  # [C][P][S]
        self.Q = pb.evec @ np.diag(pb.eval) @ pb.ivec

    def __call__(self, t):
        pb = self.pb
        # P_c = |V exp(lambda t r_c) V^-1| (substmodel.c:552), every category at once
        Pm = np.abs(np.einsum("ia,ca,aj->cij", pb.evec, np.exp(np.outer(t * pb.cat_rates, pb.eval)), pb.ivec))
        b = np.einsum("cij,ckj->cki", Pm, self.lower)
        qb = b @ self.Q.T
        w, wr = pb.cat_props, pb.cat_props * pb.cat_rates
        L = np.einsum("c,cki,cki->k", w, self.fu, b)
        A = np.einsum("c,cki,cki->k", wr, self.fu, qb)
        B = np.einsum("c,cki,cki->k", wr * pb.cat_rates, self.fu, qb @ self.Q.T)
        with np.errstate(divide="ignore", invalid="ignore"):
            return float(np.sum(pb.weights * np.log(L))), float(np.sum(pb.weights * A / L)), float(np.sum(pb.weights * (B / L - (A / L) ** 2)))


def optimise(f, start, lower=LOWER, upper=UPPER, tolerance=TOLERANCE, max_iterations=MAX_ITERATIONS, perturb=(0.0, 0.0)):
    """The rule.  f: t -> (lnl, d1, d2).  Returns (t*, iterations): iterations is the number of proposals, negated when
    max_iterations ran out or lnL was not finite at an iterate (t* is then that iterate).  perturb: relative errors put on d1 and d2"""
    t, a, b = min(max(start, lower), upper), lower, upper
    for n in range(1, max_iterations + 1):
        lnl, d1, d2 = f(t)
        if not np.isfinite(lnl):
            return t, -n
        d1, d2 = d1 * (1.0 + perturb[0]), d2 * (1.0 + perturb[1])
        if d1 > 0:
            a = t
        else:
            b = t
        nxt = t - d1 / d2 if d2 != 0 else np.nan
        if not (d2 < 0 and a < nxt < b):
            nxt = 0.5 * (a + b)
        done = abs(nxt - t) <= tolerance
        t = nxt
        if done:
            return t, n
    return t, -max_iterations


def qualified(f, start, t_star, eps=1e-9, **kw):
    """the entry's t* is stable: with d1 and d2 off by a relative eps either way, the rule ends less than tolerance / 10 away"""
    tol = kw.get("tolerance", TOLERANCE)
    return all(abs(optimise(f, start, perturb=p, **kw)[0] - t_star) < tol / 10 for p in ((eps, -eps), (-eps, eps)))


def solve_case(pb, start=None, **kw):
    """every entry of pb by the rule on EdgeEvaluator: {(k, v): (t*, iterations, qualified, the evaluator)}; start [3][N] or None:
    pb's own lengths"""
    out = {}
    for k, v in entries(pb):
        f = EdgeEvaluator(pb, v, k)
        s = pb.branch_lengths[v] if start is None else start[k, v]
        t, n = optimise(f, s, **kw)
        out[(k, v)] = (t, n, qualified(f, s, t, **kw), f)
    return out
