#!/usr/bin/env python3
"""Wall time of optimising the three branches around chosen placements by phyamd_placement_optimize, in the same process on the
same data (synthetic, GTR-like model, Gamma categories), in two forms:

  top5        the 5 best edges per query, taken from a preceding placement_log_likelihoods(masks, [0.1], 0.5) call -- timed
              separately as `score` -- by physher_amd.placement.top_candidates
  all_edges   every (query, edge), next to the route it replaces: a second engine of T + 1 taxa that holds a query tip; per query
              set_tip_states(T, query) and spr_optimize(prune=[T]); timed on 64 queries and scaled to Q

Shapes: 69 taxa x 238 patterns x 4 categories and 200 x 512 x 4, with 64 / 1024 / 16384 queries, branches 7 (all three) and 2 (the
pendant length alone), the start pendant 0.1, split 0.5, the call's default bounds, tolerances and pass cap.  Each timing is a host
clock around whole calls that end with their results on the host.  Before anything is timed the two routes are compared on the 64
queries on every edge the SPR row has a candidate for: lnL of the start at 1e-10 relative on every entry, and lnL after one pass,
where the share of entries within 1e-10 relative is recorded (an entry on which rounding tips an accept or a bisection differently
is no error of either route) and has to be nine in ten.  A form with more than
`--max-candidates` candidates is timed on the first queries that stay under it and scaled to Q (`queries_timed` says so): the
candidates run in chunks of at most 65535 anyway, each a launch of its own.  One warm-up call, then `--reps` calls.  Prints one JSON
line and writes it to profiles/placement_optimize_timing.json.

usage: placement_optimize_timing.py [--reps K] [--max-candidates M] [--out FILE]"""
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
BRANCHES = (7, 2)
ROUTE_QUERIES = 64
SPLIT, PENDANT, TOP = 0.5, 0.1, 5


def timed(call, reps):
    call()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        out.append(1e3 * (time.perf_counter() - t0))
    return out


def main():
    import placement_util as u
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-candidates", type=int, default=150000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "placement_optimize_timing.json"))
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
        aug = u.augmented_problem(pb, home, masks[0], SPLIT, PENDANT)
        new = lambda i: i if i < T else i + 1
        targets = [n for n in u.edges(pb) if n != home]
        edges = np.array(u.edges(pb), dtype=np.int32)
        with engine_from_problem(pb, rescale=RESCALE_NEVER, device=0) as e, engine_from_problem(aug, rescale=RESCALE_NEVER, tip_mode="partials", device=0) as other:

            def spr_route(count=ROUTE_QUERIES, **kw):
                out = []
                for q in range(count):
                    other.set_tip_states(T, states[q])
                    out.append([a[0] for a in other.spr_optimize([T], **kw)])
                return out

            def all_edges(queries, nodes=edges):
                return np.stack([np.repeat(np.arange(queries, dtype=np.int32), len(nodes)), np.tile(np.asarray(nodes, dtype=np.int32), queries)], axis=1)

            # (the SPR route has no subset of branches: compared with all three only).  The start is compared on every entry; after
            # one pass the two routes take the same decisions wherever rounding does not tip one (an accept, a bisection), so the
            # share of entries that agree is recorded with the worst difference, and the entries that differ are kept
            ref = spr_route(max_passes=1)
            pairs = all_edges(ROUTE_QUERIES, targets)
            got = e.placement_optimize(masks[:ROUTE_QUERIES], pairs, split=SPLIT, max_passes=1)
            cols = [new(n) for n in targets]
            b = np.array([r[1][cols] for r in ref]).ravel()
            b0 = np.array([r[2][cols] for r in ref]).ravel()
            blen = np.array([r[0][cols][:, [1, 0, 2]] for r in ref]).reshape(-1, 3)  # (t_p, t_w, t_u) -> (distal, pendant, proximal)
            assert np.all(np.isfinite(b)), "the SPR row has a candidate for every other edge"
            start_worst = float(np.max(np.abs(got[2] - b0) / np.abs(b0)))
            assert start_worst <= 1e-10, start_worst
            rel = np.abs(got[1] - b) / np.abs(b)
            differ = np.flatnonzero(rel > 1e-10)
            compared = {"entries": len(rel), "start_max_rel_lnl_difference": start_worst, "one_pass_entries_within_1e-10": int(len(rel) - len(differ)),
                        "one_pass_max_rel_lnl_difference": float(rel.max()),
                        "one_pass_differing": [{"query": int(pairs[i, 0]), "node": int(pairs[i, 1]), "lengths": got[0][i].tolist(), "lnl": float(got[1][i]),
                                                "spr_lengths": blen[i].tolist(), "spr_lnl": float(b[i])} for i in differ[:20]]}
            print(json.dumps(compared), file=sys.stderr, flush=True)
            assert len(differ) <= 0.1 * len(rel), compared
            route = timed(spr_route, 1)
            route_prof = other.spr_optimize_profile()
            for Q in QUERIES:
                m = masks[:Q]
                score = timed(lambda: e.placement_log_likelihoods(m, [PENDANT], SPLIT), args.reps)
                top = placement.top_candidates(e.placement_log_likelihoods(m, [PENDANT], SPLIT)[0][0], TOP)
                assert top.shape == (Q * TOP, 2)
                for br in BRANCHES:
                    row = {"taxa": T, "patterns": P, "categories": C, "queries": Q, "edges": pb.N - 1, "branches": br, "score": stats(score)}
                    for form, cands_of in (("top5", lambda n: top[:n * TOP]), ("all_edges", all_edges)):
                        per_query = TOP if form == "top5" else pb.N - 1
                        n = max(1, min(Q, args.max_candidates // per_query))
                        cands = cands_of(n)
                        reps = args.reps if len(cands) <= 20000 else 1
                        ms = timed(lambda: e.placement_optimize(m[:n], cands, split=SPLIT, branches=br), reps)
                        prof = e.placement_optimize_profile()
                        scaled = [x * Q / n for x in ms]
                        row[form] = {"ms": stats(scaled), "queries_timed": n, "candidates_timed": len(cands), "calls_timed": reps, "chunks": prof["chunks"],
                                     "visits_per_candidate": prof["visits"] / len(cands), "iterations_per_candidate": prof["iterations"] / len(cands),
                                     "scratch_bytes": prof["scratch_bytes"], "us_per_candidate": float(1e3 * np.median(ms) / len(cands))}
                    scaled = [x * Q / ROUTE_QUERIES for x in route]
                    row["spr_route_scaled"] = stats(scaled)
                    row["spr_route_queries_timed"] = ROUTE_QUERIES
                    row["spr_route_visits_per_candidate"] = route_prof["visits"] / max(route_prof["candidates"], 1)
                    row["spr_route_iterations_per_candidate"] = route_prof["iterations"] / max(route_prof["candidates"], 1)
                    row["spr_route_over_all_edges"] = float(np.median(scaled) / row["all_edges"]["ms"]["median_ms"]) if br == 7 else None
                    row["score_plus_top5_over_all_edges"] = float((np.median(score) + row["top5"]["ms"]["median_ms"]) / row["all_edges"]["ms"]["median_ms"])
                    row["compared_with_spr_route"] = compared
                    rows.append(row)
                    print(json.dumps(row), file=sys.stderr, flush=True)
    line = json.dumps({"shapes": rows})
    print(line, flush=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
