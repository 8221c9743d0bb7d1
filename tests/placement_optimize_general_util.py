"""NumPy restatement of phyamd_placement_optimize_general's rule on the CPU oracle.  No engine, no GPU.

placement_optimize_util.py for 20 states, with class codes in the place of 4-bit masks.  Candidate (q, n) is the placed tree of
phyamd_placement_log_likelihoods_general's definition (placement_general_util.augmented_problem: T + 1 tips, the new node z with the
left child n and the right child x, the query, whose partials are the 0/1 member vectors of its class codes) with the three lengths
around z independent -- distal t_n, pendant t_x, proximal t_z -- and only the nodes `branches` chooses marked.  The restatement is
branch_optimize_util.run / one_pass on that problem with that mask, nothing else: the visit order is its post_order, which the CPU
test pins to (n, x, z), and Edge / EdgeEvaluator are generic in the state count.  CASES are the problems both tests run; every
(query, edge) of a case is a candidate, and one_pass_thrice and full_runs are computed once per case and shared by the CPU and the
GPU test."""
import functools

import numpy as np

import branch_optimize_util as b
import pair_distance_general_util as gu
import placement_general_util as u
from gpu_util import random_problem

TOLERANCE, LOWER, UPPER, MAX_ITERATIONS = b.TOLERANCE, b.LOWER, b.UPPER, b.MAX_ITERATIONS
LNL_TOLERANCE, MAX_PASSES = b.LNL_TOLERANCE, b.MAX_PASSES
PENDANT = 0.1  # the start pendant length of every candidate

# (T, shape, P, C, Q, split, engine sets in the reference tips, sets of the call, candidates that appear twice): the smallest shapes
# where the kernel can go wrong -- no internal edge (T = 2), one (T = 3), a root child that is a tip (caterpillar); less than one
# 16-pattern tile, exactly one, one and a ragged second, more tiles (9) than the workgroup has waves (4), and past 256 patterns; 1,
# 2, 4 and 8 categories; reference tips from states and from ambiguous partials; queries without sets, with a few and with all eleven
CASES = {
    "t2_p5_c1": (2, "random", 5, 1, 3, 0.5, 0, 0, 0),
    "t3_p16_c4": (3, "random", 16, 4, 3, 0.25, 0, 3, 0),
    "t3_p17_c2": (3, "random", 17, 2, 12, 0.6, 0, 0, 0),
    "t9_p130_c8": (9, "random", 130, 8, 1, 0.5, 3, 11, 0),
    "t9_caterpillar_p70_c4": (9, "caterpillar", 70, 4, 2, 0.3, 0, 2, 0),
    "t5_p300_c2": (5, "random", 300, 2, 2, 0.4, 2, 4, 0),
    "t4_p66_c1_twice": (4, "random", 66, 1, 2, 0.5, 0, 0, 5),
}
ALL_UNKNOWN = ("t3_p17_c2", 1)  # the case and the query row that is unknown at every pattern
SEEDS = {}  # case -> the seed of its problem, where the default (7 T + P + C) misses a condition of tests/test_placement_optimize_general_util.py


@functools.lru_cache(maxsize=None)
def case(name):
    """(problem, tip mode, query codes [Q][P], the call's sets, split, candidates [count][2] int32), computed once and not to be
    changed"""
    T, shape, P, C, Q, split, tip_sets, set_count, twice = CASES[name]
    seed = SEEDS.get(name, 7 * T + P + C)
    pb = random_problem(T, P, C, seed=seed, S=20, shape=shape, gaps=0.08)  # (gaps: unknown cells in the tips)
    if tip_sets:
        gu.with_sets(pb, tip_sets, 0.1, seed + 1)
    rng = np.random.default_rng(P + Q)
    sets = u.random_sets(rng, set_count)
    codes = u.random_codes(rng, Q, P, set_count, unknown=0.1, in_sets=0.2)
    if set_count == u.MAX_SETS:
        codes[0, :set_count] = u.S + 1 + np.arange(set_count)  # the highest classes, 21..31, in one row
    if name == ALL_UNKNOWN[0]:
        codes[ALL_UNKNOWN[1]] = u.UNKNOWN
    cands = [(q, n) for q in range(Q) for n in u.edges(pb)]
    cands += cands[1:1 + twice]  # the same query and edge again, away from their first appearance
    cands = np.array(cands, dtype=np.int32)
    for a in (codes, sets, cands):
        a.setflags(write=False)
    return pb, ("partials" if tip_sets else "states"), codes, sets, split, cands


@functools.lru_cache(maxsize=None)
def reference(name):
    """the 0/1 vectors of the case's reference tips (placement_general_util.reference_partials), once"""
    return u.reference_partials(case(name)[0])


def distinct(name):
    return sorted(set(map(tuple, case(name)[5].tolist())))


def nodes(pb, n):
    """the three node ids of a candidate on edge n in the placed problem, in `lengths`' order: n, the query x, the new node z"""
    return [int(n) if n < pb.T else int(n) + 1, pb.T, 2 * pb.T]


def start(pb, n, split, pendant=PENDANT):
    """(distal, pendant, proximal) at the start, in the call's own arithmetic"""
    return np.array([split * pb.branch_lengths[n], pendant, (1.0 - split) * pb.branch_lengths[n]])


def placed(pb, n, code_row, sets, three, reference=None):
    """the placed problem with (t_n, t_x, t_z) = three: placement_general_util.augmented_problem, then the two edge halves
    overwritten"""
    q = u.augmented_problem(pb, n, code_row, sets, 0.5, three[1], reference)
    q.branch_lengths[nodes(pb, n)] = three
    return q


def mask(pb, n, branches=7):
    """the placed problem's optimise row: bit 0 of branches marks n, bit 1 x, bit 2 z"""
    m = np.zeros(pb.N + 2, dtype=bool)
    for bit, node in enumerate(nodes(pb, n)):
        m[node] = bool(branches >> bit & 1)
    return m


def run(pb, n, code_row, sets, split, branches=7, pendant=PENDANT, reference=None, **kw):
    """the whole rule for a candidate: ((t_n, t_x, t_z), lnl, initial_lnl, passes)"""
    lengths, lnl, initial, passes = b.run(placed(pb, n, code_row, sets, start(pb, n, split, pendant), reference), mask(pb, n, branches), **kw)
    return lengths[nodes(pb, n)], lnl, initial, passes


@functools.lru_cache(maxsize=None)
def one_pass_thrice(name, branches=7):
    """one pass of every distinct candidate of the case, unperturbed and under both perturbations at every visit:
    {(q, n): ((t_n, t_x, t_z), qualified)}"""
    pb, _, codes, sets, split, _ = case(name)
    out = {}
    for q, n in distinct(name):
        three, m, runs = nodes(pb, n), mask(pb, n, branches), []
        for perturb in b.PERTURBATIONS:
            p = placed(pb, n, codes[q], sets, start(pb, n, split), reference(name))
            ended, _ = b.one_pass(p, m, perturb)
            assert ended is None, (name, q, n)
            runs.append(p.branch_lengths[three])
        out[(q, n)] = (runs[0], bool(np.all([np.abs(r - runs[0]) < TOLERANCE / 10 for r in runs[1:]])))
    return out


@functools.lru_cache(maxsize=None)
def full_runs(name):
    """the whole rule of every distinct candidate of the case: {(q, n): ((t_n, t_x, t_z), lnl, initial_lnl, passes)}"""
    pb, _, codes, sets, split, _ = case(name)
    return {(q, n): run(pb, n, codes[q], sets, split, reference=reference(name)) for q, n in distinct(name)}
