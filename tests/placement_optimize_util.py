"""NumPy restatement of phyamd_placement_optimize's rule on the CPU oracle.  No engine, no GPU.

Candidate (q, n) is, by definition, phyamd_optimize_branch_lengths' result for one item: the placed tree of
phyamd_placement_log_likelihoods' definition (placement_util.augmented_problem: T + 1 tips, the new node z with the left child n and
the right child x, the query) with the three lengths around z independent -- distal t_n, pendant t_x, proximal t_z -- and only the
nodes `branches` chooses marked.  So the restatement is branch_optimize_util.run / one_pass on that problem with that mask, nothing
else: the visit order is its post_order, which the CPU test pins to (n, x, z).  CASES are the problems both tests run; every
(query, edge) of a case is a candidate, and one_pass_thrice is computed once per (case, branches) and shared by the CPU and the GPU
test."""
import functools

import numpy as np

import branch_optimize_util as b
import placement_util as u
from gpu_util import random_problem
from test_batch_gpu import _ambiguous_partials

TOLERANCE, LOWER, UPPER, MAX_ITERATIONS = b.TOLERANCE, b.LOWER, b.UPPER, b.MAX_ITERATIONS
LNL_TOLERANCE, MAX_PASSES = b.LNL_TOLERANCE, b.MAX_PASSES
PENDANT = 0.1  # the start pendant length of every candidate

# (T, shape, P, C, Q, split, ambiguity codes in the tips, candidates that appear twice): no internal edge (T = 2), one (T = 3), a
# root child that is a tip (caterpillar); less than a block of patterns, exactly one, one and a bit, two with a ragged end; 1, 2, 4
# and 8 category waves; and past k_qopt_solve4's 256 threads (CBOPT_THREADS), where a thread builds the coefficients of a second
# and a third pattern: 257 patterns (a second trip with one live thread), 300 over tip-partial masks (a ragged second trip), 600
# (three trips, the last ragged)
CASES = {
    "t2_p5_c1": (2, "random", 5, 1, 3, 0.5, False, 0),
    "t3_p64_c4": (3, "random", 64, 4, 5, 0.25, False, 0),
    "t9_p130_c8": (9, "random", 130, 8, 4, 0.5, False, 0),
    "t9_caterpillar_p70_c4": (9, "caterpillar", 70, 4, 4, 0.3, False, 0),
    "t9_p65_c2": (9, "random", 65, 2, 4, 0.7, False, 0),
    "t5_p70_c2_ambiguous": (5, "random", 70, 2, 3, 0.4, True, 0),
    "t4_p66_c1_twice": (4, "random", 66, 1, 2, 0.5, False, 5),
    "t6_p257_c8": (6, "random", 257, 8, 2, 0.3, False, 0),
    "t5_p300_c2_ambiguous": (5, "random", 300, 2, 3, 0.4, True, 0),
    "t4_p600_c4": (4, "random", 600, 4, 3, 0.5, False, 0),
}
TABLED = ["t2_p5_c1", "t3_p64_c4", "t9_p130_c8", "t9_caterpillar_p70_c4", "t9_p65_c2"]
SEEDS = {}  # case -> the seed of its problem, where the default (7 T + P + C) leaves fewer than nine entries in ten qualified


@functools.lru_cache(maxsize=None)
def case(name):
    """(problem, tip mode, query masks [Q][P], split, candidates [count][2] int32), computed once and not to be changed"""
    T, shape, P, C, Q, split, ambig, twice = CASES[name]
    pb = random_problem(T, P, C, seed=SEEDS.get(name, 7 * T + P + C), shape=shape, gaps=0.08)
    if ambig:
        _ambiguous_partials(pb, 3)
    masks = u.random_masks(np.random.default_rng(P + Q), Q, P, 0.1, 0.15)
    cands = [(q, n) for q in range(Q) for n in u.edges(pb)]
    cands += cands[1:1 + twice]  # the same query and edge again, away from their first appearance
    cands = np.array(cands, dtype=np.int32)
    masks.setflags(write=False), cands.setflags(write=False)
    return pb, ("partials" if ambig else "states"), masks, split, cands


def nodes(pb, n):
    """the three node ids of a candidate on edge n in the placed problem, in `lengths`' order: n, the query x, the new node z"""
    return [int(n) if n < pb.T else int(n) + 1, pb.T, 2 * pb.T]


def start(pb, n, split, pendant=PENDANT):
    """(distal, pendant, proximal) at the start, in the call's own arithmetic"""
    return np.array([split * pb.branch_lengths[n], pendant, (1.0 - split) * pb.branch_lengths[n]])


def placed(pb, n, mask_row, three):
    """the placed problem with (t_n, t_x, t_z) = three: placement_util.augmented_problem, then the two edge halves overwritten"""
    q = u.augmented_problem(pb, n, mask_row, 0.5, three[1])
    q.branch_lengths[nodes(pb, n)] = three
    return q


def mask(pb, n, branches=7):
    """the placed problem's optimise row: bit 0 of branches marks n, bit 1 x, bit 2 z"""
    m = np.zeros(pb.N + 2, dtype=bool)
    for bit, node in enumerate(nodes(pb, n)):
        m[node] = bool(branches >> bit & 1)
    return m


def run(pb, n, mask_row, split, branches=7, pendant=PENDANT, **kw):
    """the whole rule for a candidate: ((t_n, t_x, t_z), lnl, initial_lnl, passes)"""
    lengths, lnl, initial, passes = b.run(placed(pb, n, mask_row, start(pb, n, split, pendant)), mask(pb, n, branches), **kw)
    return lengths[nodes(pb, n)], lnl, initial, passes


@functools.lru_cache(maxsize=None)
def one_pass_thrice(name, branches=7):
    """one pass of every distinct candidate of the case, unperturbed and under both perturbations at every visit:
    {(q, n): ((t_n, t_x, t_z), qualified)}"""
    pb, _, masks, split, cands = case(name)
    out = {}
    for q, n in sorted(set(map(tuple, cands.tolist()))):
        three, m, runs = nodes(pb, n), mask(pb, n, branches), []
        for perturb in b.PERTURBATIONS:
            p = placed(pb, n, masks[q], start(pb, n, split))
            ended, _ = b.one_pass(p, m, perturb)
            assert ended is None, (name, q, n)
            runs.append(p.branch_lengths[three])
        out[(q, n)] = (runs[0], bool(np.all([np.abs(r - runs[0]) < TOLERANCE / 10 for r in runs[1:]])))
    return out
