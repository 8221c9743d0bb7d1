#!/usr/bin/env python3
"""Wall time of phyamd_spr_optimize_general -- the three graft branches of every SPR regraft of chosen subtrees of a protein engine's
tree, optimised in one call -- next to the walk it shares with the scoring call and to the loop it replaces, in the same process on
the same data (synthetic sequences under the project's WAG + Gamma(4), 2 % unknown cells):

  optimize      spr_optimize_general(prune): lengths, lnL, initial lnL and passes of every candidate, on the host
  spr           spr_log_likelihoods_general(prune) for the same rows: the shared walk and one score per candidate -- what the
                optimisation adds is the difference
  engine_route  a second engine given the rearranged tree (set_topology + set_branch_lengths), then the rule on the host: per visit
                a keep-partials gradient and one branch_log_likelihood(node, t) -- a host round trip -- per iterate, a
                set_branch_length to accept; timed on `--route-entries` candidates and SCALED to the call's candidates (labelled as
                such in the output)

Shapes: 200 taxa, 4 categories, a list of 16 prune nodes, at 512 and at 50 000 patterns.  Each timing is a host clock around whole
calls that end with their results on the host (every call ends in a stream synchronise).  The first call also makes the engine a
keep-partials engine and runs its gradient; it is reported separately (`first_call_ms`).  Before anything is timed the routes are
compared on the route's candidates: lnL at the result 1e-8 relative (the two stop after the same rule on values that differ in
rounding, so a pass more or less is possible).  Two warm-up calls, then repetitions until at least `--seconds` of calls have been timed
(at least `--reps`).  Prints one JSON line and writes it to profiles/spr_optimize_general_timing.json.

usage: spr_optimize_general_timing.py [--reps K] [--seconds S] [--route-entries M] [--out FILE]"""
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
from invalidation_util import parents  # noqa: E402
from nni_timing import stats  # noqa: E402
from physher_amd.engine import RESCALE_NEVER  # noqa: E402
from placement_general_timing import wag_problem  # noqa: E402
from placement_timing import timed  # noqa: E402
from spr_general_timing import moved  # noqa: E402

SHAPES = ((200, 512, 4, 16), (200, 50000, 4, 16))  # (taxa, patterns, categories, prune nodes)
LOWER, UPPER, TOLERANCE, MAX_ITERATIONS, LNL_TOLERANCE, MAX_PASSES = 1e-8, 10.0, 1e-8, 100, 1e-6, 50


def host_visit(e, n, tn):
    """the rule of one visit over branch_log_likelihood: (the length the visit leaves, lnL there, trials)"""
    e.gradient()  # the resident partials of the lengths as they stand
    t0 = min(max(tn, LOWER), UPPER)
    t, a, b, l0, trials = t0, LOWER, UPPER, None, 0
    for _ in range(MAX_ITERATIONS):
        lnl, d1, d2 = e.branch_log_likelihood(n, t)
        trials += 1
        if l0 is None:
            l0 = lnl
        if d1 > 0:
            a = t
        else:
            b = t
        nxt = t - d1 / d2 if d2 != 0 else np.nan
        if not (d2 < 0 and a < nxt < b):
            nxt = 0.5 * (a + b)
        done = abs(nxt - t) <= TOLERANCE
        t = nxt
        if done:
            break
    l1 = e.branch_log_likelihood(n, t)[0]
    return (t, l1, trials + 1) if np.isfinite(l1) and l1 >= l0 else (t0, l0, trials + 1)


def host_rule(e, root, tree, three):
    """one rearranged tree through the host loop: (lnl, passes, trials); three: the nodes a pass visits, in its order"""
    left, right, bl = tree
    e.set_topology(left, right, root)
    e.set_branch_lengths(bl)
    lengths = np.array(bl, dtype=np.float64)
    previous, trials = e.log_likelihood(), 0
    for k in range(1, MAX_PASSES + 1):
        lnl = previous
        for n in three:
            t, lnl, used = host_visit(e, n, lengths[n])
            trials += used
            lengths[n] = t
            e.set_branch_length(n, t)
        if lnl - previous <= LNL_TOLERANCE:
            return lnl, k, trials
        previous = lnl
    return previous, -MAX_PASSES, trials


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--route-entries", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spr_optimize_general_timing.json"))
    args = ap.parse_args()
    rows = []
    for T, P, C, count in SHAPES:
        pb = wag_problem(T, P, C)
        parent = parents(pb)
        rng = np.random.default_rng(5)
        live = [n for n in range(pb.N) if n != pb.root and parent[n] != pb.root]
        prune = np.array(sorted(rng.choice(live, size=count, replace=False)), dtype=np.int32)
        with engine_from_problem(pb, rescale=RESCALE_NEVER, device=0) as e, engine_from_problem(pb, rescale=RESCALE_NEVER, device=0) as other:
            other.set_keep_partials(True)
            t0 = time.perf_counter()
            lengths, lnl, lnl0, passes = e.spr_optimize_general(prune)
            first_call_ms = 1e3 * (time.perf_counter() - t0)
            prof = e.spr_optimize_profile()
            entries = [(i, int(w)) for i in range(len(prune)) for w in np.nonzero(np.isfinite(lnl[i]))[0]]
            assert prof["candidates"] == len(entries)
            picked = [entries[i] for i in sorted(rng.choice(len(entries), size=min(args.route_entries, len(entries)), replace=False))]
            trees, visits = [], []
            for i, w in picked:  # built before anything is timed
                p = int(prune[i])
                u = int(parent[p])
                trees.append(moved(pb, parent, p, w))
                visits.append([p, w, u] if pb.left[u] == p else [w, p, u])  # u's left child, its right child, u

            def engine_route():
                return [host_rule(other, pb.root, tree, three) for tree, three in zip(trees, visits)]

            ref = engine_route()
            err = max(abs(r[0] - lnl[i, w]) / abs(r[0]) for (i, w), r in zip(picked, ref))
            assert err <= 1e-8, err
            spr_first = e.spr_log_likelihoods_general(prune)
            err0 = float(np.nanmax(np.abs(spr_first - lnl0) / np.abs(spr_first)))
            assert err0 <= 1e-10, err0
            opt = timed(lambda: e.spr_optimize_general(prune), args.reps, args.seconds)
            prof = e.spr_optimize_profile()
            spr = timed(lambda: e.spr_log_likelihoods_general(prune), args.reps, args.seconds)
            route = timed(engine_route, 2, 0.0)
            scaled = [x * len(entries) / len(picked) for x in route]
            live_passes = passes[np.isfinite(lnl)]
            rows.append({"taxa": T, "patterns": P, "categories": C, "prunes": int(prof["prunes"]), "candidates": int(prof["candidates"]), "chunks": int(prof["chunks"]),
                         "visits": int(prof["visits"]), "iterations": int(prof["iterations"]), "scratch_bytes": int(prof["scratch_bytes"]),
                         "passes_min": int(live_passes.min()), "passes_max": int(live_passes.max()), "optimize": stats(opt), "optimize_calls_timed": len(opt),
                         "spr": stats(spr), "spr_calls_timed": len(spr), "optimize_over_spr": float(np.median(opt) / np.median(spr)),
                         "engine_route_scaled": stats(scaled), "engine_route_entries_timed": len(picked), "engine_route_trials": int(sum(r[2] for r in ref)),
                         "engine_route_ms_per_entry": float(np.median(route) / len(picked)),
                         "engine_route_scaled_over_optimize": float(np.median(scaled) / np.median(opt)), "first_call_ms": first_call_ms,
                         "max_rel_lnl_difference_to_engine_route": float(err), "max_rel_initial_lnl_difference_to_spr": err0})
            print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    line = json.dumps({"shapes": rows})
    print(line, flush=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
