#!/usr/bin/env python3
"""Wall time of optimising the three branches around chosen placements of protein queries by phyamd_placement_optimize_general, next
to the route a 20-state engine had before it, in the same process on the same data: 200 taxa x 512 patterns under the project's own
WAG + Gamma(4), 1024 random protein queries (5 % ambiguity letters) x their 5 best edges, taken from a preceding
placement_log_likelihoods_general(codes, [0.1], 0.5, sets) call -- timed separately as `score` -- by
physher_amd.placement.top_candidates.

  call          placement_optimize_general(codes, candidates, sets, split=0.5, branches=b) for b = 7 (all three branches) and 2 (the
                pendant length alone), the call's default bounds, tolerances and pass cap
  engine_route  a second engine of T + 1 tips; per candidate set_topology, set_branch_lengths and set_tip_partials; the rule on the
                host (nni_optimize_util.optimise per visit, the acceptance and stop test of the call), every iterate a
                set_branch_length and a branch_hessian_diagonal: a tree walk and a host round trip each.  Timed on
                `--route-candidates` candidates and scaled to the call's count

Each timing is a host clock around whole calls that end with their results on the host.  Before anything is timed the two routes are
compared on the route's candidates: lnL of the start at 1e-10 relative, and the largest relative difference of the final lnL is
recorded (an entry on which rounding tips an accept, a bisection or the stop test differently is no error of either route).  One
warm-up call, then `--reps` calls.  Prints one JSON line and writes it to profiles/placement_optimize_general_timing.json.

usage: placement_optimize_general_timing.py [--reps K] [--route-candidates M] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from gpu_util import engine_from_problem  # noqa: E402
from nni_timing import stats  # noqa: E402
from physher_amd import placement  # noqa: E402
from physher_amd.engine import RESCALE_NEVER  # noqa: E402
from placement_general_timing import wag_problem  # noqa: E402
from placement_optimize_timing import timed  # noqa: E402

SHAPE = (200, 512, 4)
QUERIES, TOP = 1024, 5
BRANCHES = (7, 2)
SPLIT, PENDANT = 0.5, 0.1
LOWER, UPPER, TOLERANCE, MAX_ITERATIONS, LNL_TOLERANCE, MAX_PASSES = 1e-8, 10.0, 1e-8, 100, 1e-6, 50  # the call's defaults


def main():
    import nni_optimize_util as rule
    import placement_general_util as u
    import placement_optimize_general_util as t
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--route-candidates", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "placement_optimize_general_timing.json"))
    args = ap.parse_args()
    T, P, C = SHAPE
    pb = wag_problem(T, P, C)
    rng = np.random.default_rng(11)
    letters = np.array(list(placement.AMINO_ACIDS + "BZJX-"))
    pick = np.where(rng.random((QUERIES, P)) < 0.05, rng.integers(20, 25, size=(QUERIES, P)), rng.integers(0, 20, size=(QUERIES, P)))
    codes, sets = placement.codes_from_protein(["".join(row) for row in letters[pick]])
    R = args.route_candidates
    rows = []
    with engine_from_problem(pb, rescale=RESCALE_NEVER, device=0) as e:
        score = timed(lambda: e.placement_log_likelihoods_general(codes, [PENDANT], SPLIT, sets), args.reps)
        cands = placement.top_candidates(e.placement_log_likelihoods_general(codes, [PENDANT], SPLIT, sets)[0][0], TOP)
        assert cands.shape == (QUERIES * TOP, 2)
        some = cands[:: max(1, len(cands) // R)][:R]  # the route's candidates: spread over the queries
        # the T + 1 tip trees of the route's candidates, built before anything is timed
        augmented = [t.placed(pb, n, codes[q], sets, t.start(pb, n, SPLIT, PENDANT)) for q, n in some]
        partials = [u.query_partials(codes[q], sets) for q, _ in some]
        with engine_from_problem(augmented[0], rescale=RESCALE_NEVER, tip_mode="partials", device=0) as other:

            def engine_route(branches):
                out = []
                for a, part, (_, n) in zip(augmented, partials, some):
                    other.set_topology(a.left, a.right, a.root)
                    other.set_branch_lengths(a.branch_lengths)
                    other.set_tip_partials(T, part)
                    three = [v for bit, v in enumerate(t.nodes(pb, n)) if branches >> bit & 1]
                    lengths = a.branch_lengths.copy()
                    initial = previous = lnl = other.log_likelihood()
                    passes = evaluations = 0
                    for k in range(1, MAX_PASSES + 1):
                        for v in three:
                            def f(x, v=v):
                                other.set_branch_length(v, x)
                                value, d1, d2 = other.branch_hessian_diagonal()
                                return value, d1[v], d2[v]
                            t0 = min(max(lengths[v], LOWER), UPPER)
                            l0 = f(t0)[0]
                            t1, n_it = rule.optimise(f, t0, lower=LOWER, upper=UPPER, tolerance=TOLERANCE, max_iterations=MAX_ITERATIONS)
                            l1 = f(t1)[0]
                            evaluations += abs(n_it) + 2
                            keep = np.isfinite(l1) and l1 >= l0
                            lengths[v], lnl = (t1, l1) if keep else (t0, l0)
                            other.set_branch_length(v, lengths[v])
                        if lnl - previous <= LNL_TOLERANCE:
                            passes = k
                            break
                        previous = lnl
                    out.append((lnl, initial, passes if passes else -MAX_PASSES, evaluations))
                return out

            for br in BRANCHES:
                got = e.placement_optimize_general(codes, some, sets, split=SPLIT, branches=br)
                ref = engine_route(br)
                start_worst = float(max(abs(got[2][i] - r[1]) / abs(r[1]) for i, r in enumerate(ref)))
                assert start_worst <= 1e-10, start_worst
                final_worst = float(max(abs(got[1][i] - r[0]) / abs(r[0]) for i, r in enumerate(ref)))
                route = timed(lambda: engine_route(br), 1)
                ms = timed(lambda: e.placement_optimize_general(codes, cands, sets, split=SPLIT, branches=br), args.reps)
                prof = e.placement_optimize_profile()
                passes = e.placement_optimize_general(codes, cands, sets, split=SPLIT, branches=br)[3]
                scaled = [x * len(cands) / R for x in route]
                rows.append({"taxa": T, "patterns": P, "categories": C, "queries": QUERIES, "candidates": len(cands), "sets": int(len(sets)), "branches": br,
                             "score": stats(score), "call": stats(ms), "calls_timed": args.reps, "us_per_candidate": float(1e3 * np.median(ms) / len(cands)),
                             "chunks": prof["chunks"], "distinct_edges": prof["edges"], "visits_per_candidate": prof["visits"] / len(cands),
                             "iterations_per_candidate": prof["iterations"] / len(cands), "scratch_bytes": prof["scratch_bytes"],
                             "candidates_at_the_pass_cap": int((passes < 0).sum()), "engine_route_scaled": stats(scaled), "engine_route_candidates_timed": R,
                             "engine_route_ms_per_candidate": float(np.median(route) / R), "engine_route_evaluations_per_candidate": float(np.mean([r[3] for r in ref])),
                             "engine_route_over_call": float(np.median(scaled) / np.median(ms)), "start_max_rel_lnl_difference_to_engine_route": start_worst,
                             "final_max_rel_lnl_difference_to_engine_route": final_worst,
                             "passes_call_vs_route": [[int(got[3][i]), int(r[2])] for i, r in enumerate(ref)]})
                print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    line = json.dumps({"shapes": rows})
    print(line, flush=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
