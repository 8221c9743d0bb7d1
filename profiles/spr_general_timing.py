#!/usr/bin/env python3
"""Wall time of SPR scoring on a protein engine's tree by phyamd_spr_log_likelihoods_general next to the loop it replaces, in the
same process on the same data (synthetic sequences under the project's WAG + Gamma(4), 2 % unknown cells):

  spr          spr_log_likelihoods_general(prune): lnL of every regraft of the prune nodes' subtrees, on the host
  engine_route a second engine; per candidate (p, w) set_topology + set_branch_lengths + log_likelihood -- a full tree pass and
               several host round trips each; timed on `--route-entries` candidates and SCALED to the call's candidates (labelled
               as such in the output)

Shapes: 200 taxa x 512 patterns with every node a prune node, and 200 taxa x 50 000 patterns with a list of 16 prune nodes, 4
categories.  Each timing is a host clock around whole calls that end with their results on the host (every call ends in a stream
synchronise).  The first call also makes the engine a keep-partials engine and runs its gradient; it is reported separately
(`first_call_ms`).  Before anything is timed the two routes are compared on the route's candidates: lnL at 1e-10 relative.  Two
warm-up calls, then repetitions until at least `--seconds` of calls have been timed (at least `--reps`).  Prints one JSON line and
writes it to profiles/spr_general_timing.json.

usage: spr_general_timing.py [--reps K] [--seconds S] [--route-entries M] [--out FILE]"""
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

SHAPES = ((200, 512, 4, None), (200, 50000, 4, 16))  # (taxa, patterns, categories, prune nodes or None: all)


def moved(pb, parent, p, w):
    """(left, right, branch_lengths) after pruning p and regrafting it onto the edge above w: the move's definition"""
    left, right, bl = pb.left.copy(), pb.right.copy(), pb.branch_lengths.copy()
    sib = lambda n: pb.right[parent[n]] if pb.left[parent[n]] == n else pb.left[parent[n]]
    u = parent[p]
    s, g, x = sib(p), parent[u], parent[w]
    (left if pb.left[g] == u else right)[g] = s
    bl[s] = pb.branch_lengths[s] + pb.branch_lengths[u]
    (left if pb.left[x] == w else right)[x] = u
    (left if pb.left[u] == s else right)[u] = w
    bl[u] = bl[w] = 0.5 * pb.branch_lengths[w]
    return left, right, bl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--route-entries", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spr_general_timing.json"))
    args = ap.parse_args()
    rows = []
    for T, P, C, count in SHAPES:
        pb = wag_problem(T, P, C)
        parent = parents(pb)
        rng = np.random.default_rng(5)
        live = [n for n in range(pb.N) if n != pb.root and parent[n] != pb.root]
        prune = None if count is None else np.array(sorted(rng.choice(live, size=count, replace=False)), dtype=np.int32)
        with engine_from_problem(pb, rescale=RESCALE_NEVER, device=0) as e, engine_from_problem(pb, rescale=RESCALE_NEVER, device=0) as other:
            t0 = time.perf_counter()
            got = e.spr_log_likelihoods_general(prune)
            first_call_ms = 1e3 * (time.perf_counter() - t0)
            row_nodes = np.arange(pb.N) if prune is None else prune
            entries = [(i, int(w)) for i in range(len(row_nodes)) for w in np.nonzero(np.isfinite(got[i]))[0]]
            picked = [entries[i] for i in sorted(rng.choice(len(entries), size=min(args.route_entries, len(entries)), replace=False))]
            trees = [moved(pb, parent, int(row_nodes[i]), w) for i, w in picked]  # built before anything is timed

            def engine_route():
                out = np.empty(len(picked))
                for j, (left, right, bl) in enumerate(trees):
                    other.set_topology(left, right, pb.root)
                    other.set_branch_lengths(bl)
                    out[j] = other.log_likelihood()
                return out

            ref = engine_route()
            mine = np.array([got[i, w] for i, w in picked])
            err = np.abs(mine - ref) / np.abs(ref)
            assert err.max() <= 1e-10, err
            call = timed(lambda: e.spr_log_likelihoods_general(prune), args.reps, args.seconds)
            prof = e.spr_profile()
            assert prof["candidates"] == len(entries)
            route = timed(engine_route, 3, 0.0)
            scaled = [x * len(entries) / len(picked) for x in route]
            rows.append({"taxa": T, "patterns": P, "categories": C, "prunes": int(prof["prunes"]), "candidates": int(prof["candidates"]), "chunks": int(prof["chunks"]),
                         "scratch_bytes": int(prof["scratch_bytes"]), "spr": stats(call), "spr_calls_timed": len(call), "engine_route_scaled": stats(scaled),
                         "engine_route_entries_timed": len(picked), "engine_route_ms_per_entry": float(np.median(route) / len(picked)),
                         "engine_route_scaled_over_spr": float(np.median(scaled) / np.median(call)), "first_call_ms": first_call_ms,
                         "max_rel_lnl_difference_to_engine_route": float(err.max())})
            print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    line = json.dumps({"shapes": rows})
    print(line, flush=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
