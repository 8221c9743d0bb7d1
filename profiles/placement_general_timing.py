#!/usr/bin/env python3
"""Wall time of scoring protein query sequences on every edge of a tree by phyamd_placement_log_likelihoods_general next to the
route a caller had before it, in the same process on the same data (synthetic sequences under the project's WAG + Gamma(4), 2 %
unknown cells; 3 % of the query cells are B / Z / J sets):

  full         placement_log_likelihoods_general(codes, [pendant], 0.5, sets): lnl [1, Q, N] and the best edges, on the host
  best_only    the same with want_lnl=False: the best edge and its lnL per query, on the host
  engine_route a second engine of T + 1 tips; per (query, edge) set_topology + set_branch_lengths + set_tip_partials(T, query) +
               log_likelihood -- a full tree walk and a host round trip each; timed on `--route-queries` queries x all edges and
               scaled to Q

Shape: 200 taxa x 512 patterns x 4 categories with 64 / 1024 / 16384 queries, one pendant length, split 0.5.  Each timing is a host
clock around whole calls that end with their results on the host (every call ends in a stream synchronise).  The first call also
makes the engine a keep-partials engine and runs its gradient; that call is a warm-up and is reported separately (`first_call_ms`).
Before anything is timed the two routes are compared on the route's queries on every edge at 1e-10 relative.  Two warm-up calls per
form and query count, then repetitions until at least `--seconds` of calls have been timed (at least `--reps`).  `gather_adds` is
Q x edges x padded patterns, the table reads the scoring kernel makes; over the best-only call's time it is a lower bound on that
kernel's rate (the images, the tables, the code upload and the download are in the time).  `table_mfma_at_most` is 30 v_mfma_f64
instructions per (edge, 16-pattern tile, category): the table kernel issues 20 on a tip edge.  Prints one JSON line and writes it
to profiles/placement_general_timing.json.

usage: placement_general_timing.py [--reps K] [--seconds S] [--route-queries M] [--out FILE]"""
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
from oracle import phyoracle as po  # noqa: E402
from physher_amd import placement  # noqa: E402
from physher_amd.engine import RESCALE_NEVER  # noqa: E402
from placement_timing import timed  # noqa: E402

SHAPE = (200, 512, 4)
QUERIES = (64, 1024, 16384)
SPLIT, PENDANT = 0.5, 0.1


def wag_problem(T, P, C, seed=7):
    from physher_amd import _phycpp_amd as pc
    pb = random_problem(T, P, C, seed, S=20, gaps=0.02)
    m = pc.substitution_model("WAG")
    site = pc.GammaSiteModelInterface(0.5, C, None, None)
    return po.Problem(pb.left, pb.right, pb.root, np.ones(P), m["eval"], m["evec"], m["ivec"], m["frequencies"], site.rates(), site.proportions(), pb.branch_lengths,
                      tip_states=pb.tip_states)


def main():
    import placement_general_util as u
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--route-queries", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "placement_general_timing.json"))
    args = ap.parse_args()
    T, P, C = SHAPE
    pb = wag_problem(T, P, C)
    rng = np.random.default_rng(11)
    letters = np.array(list(placement.AMINO_ACIDS + "BZJX-"))
    pick = np.where(rng.random((max(QUERIES), P)) < 0.05, rng.integers(20, 25, size=(max(QUERIES), P)), rng.integers(0, 20, size=(max(QUERIES), P)))
    codes, sets = placement.codes_from_protein(["".join(row) for row in letters[pick]])
    edges = u.edges(pb)
    R = args.route_queries
    # the T + 1 tip trees of every edge, built before anything is timed (ids: placement_general_util.augmented_problem)
    augmented = [u.augmented_problem(pb, n, codes[0], sets, SPLIT, PENDANT) for n in edges]
    query_partials = [u.query_partials(codes[q], sets) for q in range(R)]
    rows = []
    with engine_from_problem(pb, rescale=RESCALE_NEVER, device=0) as e, engine_from_problem(augmented[0], rescale=RESCALE_NEVER, tip_mode="partials", device=0) as other:

        def engine_route():
            out = np.full((R, pb.N), np.nan)
            for q in range(R):
                for a, n in zip(augmented, edges):
                    other.set_topology(a.left, a.right, a.root)
                    other.set_branch_lengths(a.branch_lengths)
                    other.set_tip_partials(T, query_partials[q])
                    out[q, n] = other.log_likelihood()
            return out

        t0 = time.perf_counter()
        got = e.placement_log_likelihoods_general(codes[:R], [PENDANT], SPLIT, sets)[0][0]
        first_call_ms = 1e3 * (time.perf_counter() - t0)
        ref = engine_route()
        worst = float(np.nanmax(np.abs(got - ref) / np.abs(ref)))
        assert worst <= 1e-10, worst
        route = timed(engine_route, 3, 0.0)
        Ppad = (P + 127) // 128 * 128
        for Q in QUERIES:
            c = codes[:Q]
            full = timed(lambda: e.placement_log_likelihoods_general(c, [PENDANT], SPLIT, sets), args.reps, args.seconds)
            prof = e.placement_profile()
            best = timed(lambda: e.placement_log_likelihoods_general(c, [PENDANT], SPLIT, sets, want_lnl=False), args.reps, args.seconds)
            scaled = [x * Q / R for x in route]
            gathers = Q * (pb.N - 1) * Ppad
            rows.append({"taxa": T, "patterns": P, "categories": C, "queries": Q, "edges": pb.N - 1, "sets": int(len(sets)), "full": stats(full), "best_only": stats(best),
                         "full_calls_timed": len(full), "best_only_calls_timed": len(best), "engine_route_scaled": stats(scaled), "engine_route_queries_timed": R,
                         "engine_route_ms_per_query_edge": float(np.median(route) / (R * (pb.N - 1))),
                         "engine_route_over_full": float(np.median(scaled) / np.median(full)), "engine_route_over_best_only": float(np.median(scaled) / np.median(best)),
                         "edge_chunks": prof["edge_chunks"], "query_chunks": prof["query_chunks"], "scratch_bytes": prof["scratch_bytes"], "lnl_bytes": Q * pb.N * 8,
                         "gather_adds": gathers, "gather_adds_per_s_best_only_call": float(gathers / (1e-3 * np.min(best))),
                         "table_mfma_at_most": (pb.N - 1) * (Ppad // 16) * C * 30, "first_call_ms": first_call_ms, "max_rel_lnl_difference_to_engine_route": worst})
            print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    line = json.dumps({"shapes": rows})
    print(line, flush=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
