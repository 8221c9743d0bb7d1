"""NumPy restatement of phyamd_optimize_branch_lengths' rule on the CPU oracle.  No engine, no GPU.

The one-dimensional rule is nni_optimize_util.optimise, imported.  A visit of node n evaluates f(t) = (lnL, d1, d2) of the tree with
t_n = t from the oracle's lower and upper partial at n, taken from a fresh gradient(want_partials=True) at the lengths as they stand
at that visit (Edge): nothing is carried from visit to visit, so the restatement cannot be stale by construction.  Edge is pinned
against the definition -- the oracle's lnL, branch_gradient_from_cat, hessian_util.branch_hessian_diagonal -- in
tests/test_branch_optimize_util.py.  CASES are the problems tests/test_branch_optimize_gpu.py runs; one_visit and one_pass_thrice
are computed once per case and shared by the CPU and the GPU test."""
import copy
import functools

import numpy as np

import nni_optimize_util as u
from gpu_util import random_problem
from test_nni_gpu import _relabelled

TOLERANCE, LOWER, UPPER, MAX_ITERATIONS = u.TOLERANCE, u.LOWER, u.UPPER, u.MAX_ITERATIONS
LNL_TOLERANCE, MAX_PASSES = 1e-6, 50
EPS = 1e-9  # the relative error on d1 and d2 a result has to be stable under to be compared (nni_optimize_util.qualified)
PERTURBATIONS = ((0.0, 0.0), (EPS, -EPS), (-EPS, EPS))

# (T, P, C, shape, relabel, gaps, pinv)
CASES = {
    "t2": (2, 65, 2, "random", False, 0.0, None),
    "t3": (3, 64, 1, "random", False, 0.0, None),
    "t37_gaps_pinv": (37, 238, 4, "random", False, 0.05, 0.25),
    "t37_c8": (37, 700, 8, "random", False, 0.0, None),
}
for _shape in ("caterpillar", "balanced", "random", "relabelled"):
    for _P in (64, 65):
        CASES[f"t8_{_shape}_p{_P}"] = (8, _P, 2, "random" if _shape == "relabelled" else _shape, _shape == "relabelled", 0.02, None)
T8 = sorted(c for c in CASES if c.startswith("t8"))
PASS_CASES = ["t2", "t3"] + T8 + ["t37_gaps_pinv"]  # the cases whose whole pass is restated three times


@functools.lru_cache(maxsize=None)
def _problem(case):
    T, P, C, shape, rel, gaps, pinv = CASES[case]
    pb = random_problem(T, P, C, seed=13 * T + P + C, shape=shape, gaps=gaps, pinv=pinv)
    return _relabelled(pb, 7) if rel else pb  # (internal ids permuted, the root not last)


def problem(case):
    """a copy of the case's problem that the caller may change (its lengths are its own)"""
    return with_lengths(_problem(case), _problem(case).branch_lengths)


def with_lengths(pb, lengths):
    q = copy.copy(pb)
    q.branch_lengths = np.array(lengths, dtype=np.float64)
    return q


def post_order(pb, mask=None):
    """the nodes a pass visits, in its order: left subtree, right subtree, node; never the root"""
    out, stack = [], [(pb.root, False)]
    while stack:
        n, done = stack.pop()
        if done or n < pb.T:
            if n != pb.root and (mask is None or mask[n]):
                out.append(n)
            continue
        stack.extend([(n, True), (int(pb.right[n]), False), (int(pb.left[n]), False)])
    return out


class Edge(u.EdgeEvaluator):
    """t -> (lnl, d1, d2) of pb with t_n = t, from the oracle's lower and upper partial at n at pb's lengths as they stand now"""

    def __init__(self, pb, n):
        r = pb.gradient(want_partials=True)
        assert not r["rescaled"]
        self.pb, self.lower = pb, r["lower"][n]
        self.fu = r["upper"][n] * pb.freqs
        self.Q = pb.evec @ np.diag(pb.eval) @ pb.ivec


def visit(pb, n, perturb=(0.0, 0.0), lower=LOWER, upper=UPPER, tolerance=TOLERANCE, max_iterations=MAX_ITERATIONS):
    """One visit of node n on pb's lengths, which it changes.  Returns (lnl now, None), or (the lnL that is not finite, n) where an
    iterate's lnL is not finite: the lengths are then untouched"""
    f, seen = Edge(pb, n), []

    def recorded(t):
        r = f(t)
        seen.append(r[0])
        return r
    t0 = min(max(pb.branch_lengths[n], lower), upper)
    t1, _ = u.optimise(recorded, t0, lower=lower, upper=upper, tolerance=tolerance, max_iterations=max_iterations, perturb=perturb)
    if not np.isfinite(seen[-1]):
        return seen[-1], n
    l0, l1 = seen[0], f(t1)[0]
    accept = np.isfinite(l1) and l1 >= l0
    pb.branch_lengths[n] = t1 if accept else t0
    return (l1 if accept else l0), None


def one_pass(pb, mask=None, perturb=(0.0, 0.0), trace=None, **kw):
    """a pass over pb's lengths, which it changes; trace: lnL after each visit is appended.  Returns the node whose visit ended
    the item with a lnL that is not finite (and that lnL), or (None, lnL after the pass by the oracle)"""
    for n in post_order(pb, mask):
        lnl, ended = visit(pb, n, perturb, **kw)
        if ended is not None:
            return ended, lnl
        if trace is not None:
            trace.append(lnl)
    return None, pb.log_likelihood()["lnl"]


def run(pb, mask=None, lnl_tolerance=LNL_TOLERANCE, max_passes=MAX_PASSES, **kw):
    """the whole rule from pb's lengths: (lengths, lnl, initial_lnl, passes); pb is not changed"""
    q = with_lengths(pb, pb.branch_lengths)
    initial = previous = q.log_likelihood()["lnl"]
    if not post_order(q, mask):
        return q.branch_lengths, initial, initial, 0
    for p in range(1, max_passes + 1):
        ended, lnl = one_pass(q, mask, **kw)
        if ended is not None:
            return q.branch_lengths, lnl, initial, -p
        if lnl - previous <= lnl_tolerance:
            return q.branch_lengths, lnl, initial, p
        previous = lnl
    return q.branch_lengths, previous, initial, -max_passes


def start_lengths(pb, seed=5):
    """a start away from the optimum: the problem's lengths times factors in [0.3, 3]"""
    return pb.branch_lengths * np.random.default_rng(seed).uniform(0.3, 3.0, size=pb.N)


@functools.lru_cache(maxsize=None)
def one_visit(case):
    """every node of the case visited alone from start_lengths: {n: (t, qualified)}"""
    pb = problem(case)
    start, out = start_lengths(pb), {}
    for n in post_order(pb):
        ts = []
        for p in PERTURBATIONS:
            q = with_lengths(pb, start)
            visit(q, n, p)
            ts.append(q.branch_lengths[n])
        out[n] = (ts[0], all(abs(t - ts[0]) < TOLERANCE / 10 for t in ts[1:]))
    return out


@functools.lru_cache(maxsize=None)
def one_pass_thrice(case):
    """one pass from start_lengths, unperturbed and under both perturbations at every visit: (lengths, qualified [N])"""
    pb = problem(case)
    runs = []
    for p in PERTURBATIONS:
        q = with_lengths(pb, start_lengths(pb))
        one_pass(q, None, p)
        runs.append(q.branch_lengths)
    good = np.all([np.abs(r - runs[0]) < TOLERANCE / 10 for r in runs[1:]], axis=0)
    good[pb.root] = False
    return runs[0], good
