#!/usr/bin/env python3
"""Wall time of scoring query sequences on every edge of a tree by phyamd_placement_log_likelihoods next to the route a caller had
before it, in the same process on the same data (synthetic, GTR-like model, Gamma categories):

  full        placement_log_likelihoods(masks, [pendant], 0.5): lnl [1, Q, N] and the best edges, on the host
  best_only   placement_log_likelihoods(..., want_lnl=False): the best edge and its lnL per query, on the host
  spr_route   a second engine of T + 1 taxa that holds a query tip; per query set_tip_states(T, query) and
              spr_log_likelihoods(prune=[T]); timed on 64 queries and scaled to Q

Shapes: 69 taxa x 238 patterns x 4 categories and 200 x 512 x 4, with 64 / 1024 / 16384 queries, one pendant length, split 0.5.  Each
timing is a host clock around whole calls that end with their results on the host (every call ends in a stream synchronise).
Before anything is timed the two routes are compared on the 64 queries, on every edge the SPR row has a candidate for, at 1e-10
relative.  Two warm-up calls per form and query count, then repetitions until at least `--seconds` of calls have been timed (at
least `--reps`).  `gather_adds` is Q x edges x padded patterns, the table reads the scoring kernel makes; over the best-only call's
time it is a lower bound on that kernel's rate (the walk, the tables, the mask upload and the download are in the time).  Prints one
JSON line and writes it to profiles/placement_timing.json.

usage: placement_timing.py [--reps K] [--seconds S] [--out FILE]"""
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

from gpu_util import engine_from_problem, random_problem  # noqa: E402
from nni_timing import stats  # noqa: E402
from physher_amd import placement  # noqa: E402
from physher_amd.engine import RESCALE_NEVER  # noqa: E402

SHAPES = ((69, 238, 4), (200, 512, 4))
QUERIES = (64, 1024, 16384)
ROUTE_QUERIES = 64
SPLIT = 0.5


def timed(call, reps, seconds):
    for _ in range(2):
        call()
    out, total = [], 0.0
    while len(out) < reps or (total < seconds and len(out) < 400):
        t0 = time.perf_counter()
        call()
        dt = time.perf_counter() - t0
        out.append(1e3 * dt)
        total += dt
    return out


def main():
    import placement_util as u
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "placement_timing.json"))
    args = ap.parse_args()
    rows = []
    for T, P, C in SHAPES:
        pb = random_problem(T, P, C, seed=7, gaps=0.02)
        pb.weights = np.ones(P)
        rng = np.random.default_rng(11)
        states = rng.integers(0, 4, size=(max(QUERIES), P)).astype(np.uint8)
        states[rng.random(states.shape) < 0.02] = 17  # gaps
        masks = placement.masks_from_states(states)
        parent = u.parents(pb)
        home = next(n for n in range(T) if parent[n] != pb.root)  # where the second engine's tree holds the query tip
        pendant = 0.1
        aug = u.augmented_problem(pb, home, masks[0], SPLIT, pendant)
        new = lambda i: i if i < T else i + 1
        targets = [n for n in u.edges(pb) if n != home]
        with engine_from_problem(pb, rescale=RESCALE_NEVER, device=0) as e, engine_from_problem(aug, rescale=RESCALE_NEVER, tip_mode="partials", device=0) as other:

            def spr_route(count=ROUTE_QUERIES):
                out = np.empty((count, aug.N))
                for q in range(count):
                    other.set_tip_states(T, states[q])
                    out[q] = other.spr_log_likelihoods([T])[0]
                return out

            ref = spr_route()
            got = e.placement_log_likelihoods(masks[:ROUTE_QUERIES], [pendant], SPLIT)[0][0]
            a, b = got[:, targets], ref[:, [new(n) for n in targets]]
            assert np.all(np.isfinite(b)), "the SPR row has a candidate for every other edge"
            worst = float(np.max(np.abs(a - b) / np.abs(b)))
            assert worst <= 1e-10, worst
            route = timed(spr_route, 3, 0.0)
            for Q in QUERIES:
                m = masks[:Q]
                full = timed(lambda: e.placement_log_likelihoods(m, [pendant], SPLIT), args.reps, args.seconds)
                prof = e.placement_profile()
                best = timed(lambda: e.placement_log_likelihoods(m, [pendant], SPLIT, want_lnl=False), args.reps, args.seconds)
                scaled = [x * Q / ROUTE_QUERIES for x in route]
                gathers = Q * (pb.N - 1) * ((P + 63) // 64 * 64)
                rows.append({"taxa": T, "patterns": P, "categories": C, "queries": Q, "edges": pb.N - 1, "full": stats(full), "best_only": stats(best),
                             "full_calls_timed": len(full), "best_only_calls_timed": len(best), "spr_route_scaled": stats(scaled),
                             "spr_route_queries_timed": ROUTE_QUERIES, "spr_route_over_full": float(np.median(scaled) / np.median(full)),
                             "spr_route_over_best_only": float(np.median(scaled) / np.median(best)), "edge_chunks": prof["edge_chunks"],
                             "query_chunks": prof["query_chunks"], "scratch_bytes": prof["scratch_bytes"], "lnl_bytes": Q * pb.N * 8, "gather_adds": gathers,
                             "gather_adds_per_s_best_only_call": float(gathers / (1e-3 * np.min(best))), "max_rel_lnl_difference_to_spr_route": worst})
                print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    line = json.dumps({"shapes": rows})
    print(line, flush=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
