"""NumPy restatement of phyamd_spr_optimize's rule on the CPU oracle.  No engine, no GPU.

Entry (p, w) is, by definition, phyamd_optimize_branch_lengths' result for one item: the rearranged tree of the entry
(test_spr_gpu._moved: the move's definition, with its lengths), only p, w and u = parent(p) marked.  So the restatement is
branch_optimize_util.run / one_pass on that problem with that mask, nothing else: the visit order is its post_order, which the CPU
test pins to (left[u], right[u], u).  CASES are test_spr_gpu.CASES; entries(case) are the (p, w) a case is checked on -- every
candidate up to eight taxa, a fixed seeded sample of SAMPLE candidates that holds every class of test_spr_gpu.CLASSES at 37 --
and one_pass_thrice is computed once per case and shared by the CPU and the GPU test."""
import copy
import functools

import numpy as np

import branch_optimize_util as b
import test_spr_gpu as s
from test_nni_gpu import _parents

TOLERANCE, LOWER, UPPER, MAX_ITERATIONS = b.TOLERANCE, b.LOWER, b.UPPER, b.MAX_ITERATIONS
LNL_TOLERANCE, MAX_PASSES = b.LNL_TOLERANCE, b.MAX_PASSES
CASES = sorted(s.CASES)
SAMPLE = 200
SEEDS = {}  # case -> the seed of its sample, where the default (SAMPLE) leaves fewer than nine entries in ten qualified


def problem(case):
    """(problem, tip mode) of the case: test_spr_gpu's own, not to be changed"""
    return s._problem(case)


def nodes(parent, p, w):
    """the three nodes of entry (p, w), in `lengths`' order"""
    return [p, w, int(parent[p])]


def rearranged(pb, parent, p, w):
    q = copy.copy(pb)
    q.left, q.right, q.branch_lengths = s._moved(pb, parent, p, w)
    return q


def mask(pb, parent, p, w):
    m = np.zeros(pb.N, dtype=bool)
    m[nodes(parent, p, w)] = True
    return m


def at_lengths(pb, parent, p, w, three):
    """the rearranged problem of the entry with (t_p, t_w, t_u) = three"""
    q = rearranged(pb, parent, p, w)
    q.branch_lengths[nodes(parent, p, w)] = three
    return q


def run(pb, parent, p, w, **kw):
    """the whole rule for entry (p, w): ((t_p, t_w, t_u), lnl, initial_lnl, passes)"""
    lengths, lnl, initial, passes = b.run(rearranged(pb, parent, p, w), mask(pb, parent, p, w), **kw)
    return lengths[nodes(parent, p, w)], lnl, initial, passes


@functools.lru_cache(maxsize=None)
def entries(case):
    pb, _ = problem(case)
    parent = _parents(pb)
    pairs = s._pairs(s._candidate_mask(pb))
    if pb.T <= 8:
        return pairs
    order = np.random.default_rng(SEEDS.get(case, SAMPLE)).permutation(len(pairs))
    sample, missing = [], set(s.CLASSES)
    for i in order:  # first one pair per class still missing, then whatever comes (test_spr_gpu.test_two_hundred_taxa's way)
        got = s._classes(pb, parent, *pairs[i])
        if got & missing:
            sample.append(pairs[i])
            missing -= got
    assert not missing, missing
    chosen = set(sample)
    for i in order:
        if len(sample) == SAMPLE:
            break
        if pairs[i] not in chosen:
            sample.append(pairs[i])
            chosen.add(pairs[i])
    return sample


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
