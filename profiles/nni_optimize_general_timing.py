#!/usr/bin/env python3
"""Wall time of the optimised NNI neighbourhood of a protein engine's tree by phyamd_nni_optimize_general next to the two routes it
replaces, in the same process on the same data (synthetic sequences under the project's WAG + Gamma(4), 2 % unknown cells):

  optimize      nni_optimize_general(): the central branch of the three arrangements of every internal edge optimised on the
                device, with lnL, d1, d2 and the counts on the host
  host_rule     the same rule run on the host for all entries at once: one nni_log_likelihoods_general call per round (every entry
                still iterating gets its next trial length), until the last entry has stopped, and one more for the values at t*;
                every round redoes the seven products per tile and a host round trip
  engine_route  a second engine; per entry set_topology, then per iteration set_branch_length + branch_hessian_diagonal -- two full
                tree passes and several host round trips each; timed on `--route-entries` entries and SCALED to the 3 (T - 2) entries
                (labelled as such in the output)

Shapes: 200 taxa x 512 patterns and 200 taxa x 50 000 patterns, 4 categories; the rule's defaults (tolerance 1e-8, bounds
[1e-8, 10], 100 iterations, start at the engine's lengths).  Each timing is a host clock around whole calls that end with their
results on the host.  The first call also makes the engine a keep-partials engine and runs its gradient; it is reported separately
(`first_call_ms`).  Before anything is timed the three routes are compared: lnL at t* at 1e-10 relative, and how far the lengths
lie apart is reported.  `solve_ms` is the call less a nni_log_likelihoods_general call without derivatives on the same engine, which
costs what the coefficient kernel costs or more: what the one-workgroup-per-entry iterations take.  `K_bytes` is the coefficients'
3 C 20 Pp doubles per candidate, read once per iteration.  Prints one JSON line and writes it to
profiles/nni_optimize_general_timing.json.

usage: nni_optimize_general_timing.py [--reps K] [--seconds S] [--route-entries M] [--out FILE]"""
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
from invalidation_util import rearranged  # noqa: E402
from nni_timing import stats  # noqa: E402
from physher_amd.engine import RESCALE_NEVER  # noqa: E402
from placement_general_timing import wag_problem  # noqa: E402
from placement_timing import timed  # noqa: E402

SHAPES = ((200, 512, 4), (200, 50000, 4))
LOWER, UPPER, TOLERANCE, MAX_ITERATIONS = 1e-8, 10.0, 1e-8, 100


def propose(t, d1, d2, a, b):
    """the rule's step on arrays: the bracket's new ends and the next iterate"""
    up = d1 > 0
    a, b = np.where(up, t, a), np.where(up, b, t)
    with np.errstate(divide="ignore", invalid="ignore"):
        nxt = t - d1 / d2
    nxt = np.where((d2 < 0) & (a < nxt) & (nxt < b), nxt, 0.5 * (a + b))
    return a, b, nxt


def host_rule(e, pb, cand):
    """(lengths, lnl, rounds): every entry by the rule, a nni_log_likelihoods_general call per round"""
    t = np.clip(np.tile(pb.branch_lengths, (3, 1)), LOWER, UPPER)
    a, b = np.full_like(t, LOWER), np.full_like(t, UPPER)
    active = np.zeros(t.shape, dtype=bool)
    active[:, cand] = True
    rounds = 0
    while active.any() and rounds < MAX_ITERATIONS:
        _, d1, d2 = e.nni_log_likelihoods_general(t)
        rounds += 1
        na, nb, nxt = propose(t, d1, d2, a, b)
        done = np.abs(nxt - t) <= TOLERANCE
        a, b, t = np.where(active, na, a), np.where(active, nb, b), np.where(active, nxt, t)
        active &= ~done
    lnl, _, _ = e.nni_log_likelihoods_general(t)
    return t, lnl, rounds


def engine_rule(other, pb, v, tree):
    """(t*, lnl, iterations) of one entry on a second engine that holds the rearranged tree"""
    left, right, bl = tree
    other.set_topology(left, right, pb.root)
    other.set_branch_lengths(bl)
    t, a, b = min(max(float(bl[v]), LOWER), UPPER), LOWER, UPPER
    for n in range(1, MAX_ITERATIONS + 1):
        other.set_branch_length(v, t)
        _, d1, d2 = other.branch_hessian_diagonal()
        a, b, nxt = (float(x) for x in propose(t, d1[v], d2[v], a, b))
        done = abs(nxt - t) <= TOLERANCE
        t = nxt
        if done:
            break
    other.set_branch_length(v, t)
    return t, other.log_likelihood(), n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--route-entries", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nni_optimize_general_timing.json"))
    args = ap.parse_args()
    rows = []
    for T, P, C in SHAPES:
        pb = wag_problem(T, P, C)
        cand = [v for v in range(pb.T, pb.N) if v != pb.root]
        entries = [(k, v) for v in cand for k in range(3)]
        rng = np.random.default_rng(5)
        picked = [entries[i] for i in sorted(rng.choice(len(entries), size=min(args.route_entries, len(entries)), replace=False))]
        trees = [rearranged(pb, v, k, pb.branch_lengths[v]) for k, v in picked]  # built before anything is timed
        with engine_from_problem(pb, rescale=RESCALE_NEVER, device=0) as e, engine_from_problem(pb, rescale=RESCALE_NEVER, device=0) as other:

            def engine_route():
                return [engine_rule(other, pb, v, tree) for (k, v), tree in zip(picked, trees)]

            t0 = time.perf_counter()
            lengths, lnl, d1, d2, it = e.nni_optimize_general()
            first_call_ms = 1e3 * (time.perf_counter() - t0)
            prof = e.nni_optimize_profile()
            ht, hl, rounds = host_rule(e, pb, cand)
            ref = engine_route()
            host_dt = float(np.abs(ht[:, cand] - lengths[:, cand]).max())
            host_dl = float((np.abs(hl[:, cand] - lnl[:, cand]) / np.abs(lnl[:, cand])).max())
            route_dt = max(abs(r[0] - lengths[k, v]) for (k, v), r in zip(picked, ref))
            route_dl = max(abs(r[1] - lnl[k, v]) / abs(r[1]) for (k, v), r in zip(picked, ref))
            assert np.all(it[:, cand] > 0) and host_dl <= 1e-10 and route_dl <= 1e-10, (host_dl, route_dl)
            opt = timed(lambda: e.nni_optimize_general(), args.reps, args.seconds)
            score = timed(lambda: e.nni_log_likelihoods_general(want_derivatives=False), args.reps, args.seconds)
            host = timed(lambda: host_rule(e, pb, cand), 3, 0.0)
            route = timed(engine_route, 2, 0.0)
            scaled = [x * len(entries) / len(picked) for x in route]
            rows.append({"taxa": T, "patterns": P, "categories": C, "entries": len(entries), "optimize": stats(opt), "optimize_calls_timed": len(opt),
                         "iterations": int(prof["iterations"]), "iterations_per_entry_max": int(np.abs(it).max()), "chunks": int(prof["chunks"]),
                         "scratch_bytes": int(prof["scratch_bytes"]), "K_bytes": int(len(cand) * 3 * C * 20 * ((P + 15) // 16 * 16) * 8),
                         "score_lnl_call": stats(score), "solve_ms": float(np.median(opt) - np.median(score)),
                         "host_rule": stats(host), "host_rule_rounds": rounds, "host_rule_over_optimize": float(np.median(host) / np.median(opt)),
                         "engine_route_scaled": stats(scaled), "engine_route_entries_timed": len(picked),
                         "engine_route_iterations_timed": int(sum(r[2] for r in ref)), "engine_route_ms_per_entry": float(np.median(route) / len(picked)),
                         "engine_route_scaled_over_optimize": float(np.median(scaled) / np.median(opt)), "first_call_ms": first_call_ms,
                         "max_length_difference_to_host_rule": host_dt, "max_rel_lnl_difference_to_host_rule": host_dl,
                         "max_length_difference_to_engine_route": float(route_dt), "max_rel_lnl_difference_to_engine_route": float(route_dl)})
            print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    line = json.dumps({"shapes": rows})
    print(line, flush=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
