"""NumPy restatement of phyamd_spr_optimize_general's rule on the CPU oracle.  No engine, no GPU.

The restatement is tests/spr_optimize_util.py's, which knows no state count: entry (p, w) is branch_optimize_util.run / one_pass on the
rearranged problem of the entry (test_spr_gpu._moved: the move's definition, with its lengths) with p, w and u = parent(p) marked.
CASES are test_spr_general_gpu.CASES, built as its _case builds them but without that test's oracle table; entries(case) are the
(p, w) a case is checked on -- every candidate of the five cases of at most nine taxa whose candidates are few, and in
t9_random_p130_c8_sets and t17_random_p200_c4 the seeded sample test_spr_general_gpu._sample(pb, 48), which holds every class of
CLASSES and MORE_CLASSES (the assert inside _sample).  one_pass_thrice and run_all are computed once per case and shared by the CPU
and the GPU test."""
import functools

import numpy as np

import branch_optimize_util as b
import pair_distance_general_util as gu
import spr_optimize_util as t
import test_spr_general_gpu as g
import test_spr_gpu as s
from gpu_util import random_problem
from invalidation_util import parents as _parents
from test_tree_batch_gpu import _relabel

TOLERANCE, LOWER, UPPER, MAX_ITERATIONS = t.TOLERANCE, t.LOWER, t.UPPER, t.MAX_ITERATIONS
LNL_TOLERANCE, MAX_PASSES = t.LNL_TOLERANCE, t.MAX_PASSES
CASES = sorted(g.CASES)
SAMPLED = ("t9_random_p130_c8_sets", "t17_random_p200_c4")
SAMPLE = 48
nodes, rearranged, mask, at_lengths, run = t.nodes, t.rearranged, t.mask, t.at_lengths, t.run


@functools.lru_cache(maxsize=None)
def problem(case):
    """(problem, tip mode) of the case, as test_spr_general_gpu._case builds it: not to be changed"""
    T, shape, P, C, gaps, pinv, tip_sets, relabel = g.CASES[case]
    pb = random_problem(T, P, C, seed=7 * T + P + C, S=20, shape=shape, gaps=gaps, pinv=pinv)
    if relabel:
        tree, _ = _relabel((pb.left, pb.right, pb.root, pb.branch_lengths), np.random.default_rng(3), pb.T)
        pb.left, pb.right, pb.root, pb.branch_lengths = tree[0], tree[1], tree[2], tree[3]
    if tip_sets:
        gu.with_sets(pb, tip_sets, 0.1, 7 * T + P + C + 1)
    return pb, ("partials" if tip_sets else "states")


@functools.lru_cache(maxsize=None)
def entries(case):
    pb, _ = problem(case)
    if case in SAMPLED:
        return [(int(p), int(w)) for p, w in g._sample(pb, SAMPLE)]
    return s._pairs(s._candidate_mask(pb))


@functools.lru_cache(maxsize=None)
def one_pass_thrice(case):
    """one pass of every entry of the case, unperturbed and under both perturbations at every visit:
    {(p, w): ((t_p, t_w, t_u), qualified)}"""
    pb, _ = problem(case)
    parent, out = _parents(pb), {}
    for p, w in entries(case):
        three, m, runs = nodes(parent, p, w), mask(pb, parent, p, w), []
        for perturb in b.PERTURBATIONS:
            q = rearranged(pb, parent, p, w)
            ended, _ = b.one_pass(q, m, perturb)
            assert ended is None, (case, p, w)
            runs.append(q.branch_lengths[three])
        out[(p, w)] = (runs[0], bool(np.all([np.abs(r - runs[0]) < TOLERANCE / 10 for r in runs[1:]])))
    return out


@functools.lru_cache(maxsize=None)
def run_all(case):
    """the whole rule of every entry of the case: {(p, w): ((t_p, t_w, t_u), lnl, initial_lnl, passes)}"""
    pb, _ = problem(case)
    parent = _parents(pb)
    return {(p, w): run(pb, parent, p, w) for p, w in entries(case)}
