#!/usr/bin/env python3
"""Wall time of the whole NNI neighbourhood of a protein engine's tree by phyamd_nni_log_likelihoods_general next to the loop it
replaces, in the same process on the same data (synthetic sequences under the project's WAG + Gamma(4), 2 % unknown cells):

  nni          nni_log_likelihoods_general(want_derivatives=False): lnL of the three arrangements of every internal edge, on the host
  nni_d        the same with d1 and d2
  engine_route a second engine; per entry (k, v) set_topology + set_branch_length + branch_hessian_diagonal -- two full tree passes
               and several host round trips each; timed on `--route-entries` entries and SCALED to the 3 (T - 2) entries of a round
               (labelled as such in the output)

Shapes: 200 taxa x 512 patterns and 200 taxa x 50 000 patterns, 4 categories.  Each timing is a host clock around whole calls that
end with their results on the host (every call ends in a stream synchronise).  The first call also makes the engine a keep-partials
engine and runs its gradient; it is reported separately (`first_call_ms`).  Before anything is timed the two routes are compared on
the route's entries: lnL at 1e-10 relative, d1 and d2 at 1e-9 * max(1, |ref|).  Two warm-up calls per form, then repetitions until at
least `--seconds` of calls have been timed (at least `--reps`).  `mfma_products` is 7 twenty-wide products per (candidate, category,
16-pattern tile) less the one of a candidate under the root.  Prints one JSON line and writes it to profiles/nni_general_timing.json.

usage: nni_general_timing.py [--reps K] [--seconds S] [--route-entries M] [--out FILE]"""
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
from invalidation_util import parents, rearranged  # noqa: E402
from nni_timing import stats  # noqa: E402
from physher_amd.engine import RESCALE_NEVER  # noqa: E402
from placement_general_timing import wag_problem  # noqa: E402
from placement_timing import timed  # noqa: E402

SHAPES = ((200, 512, 4), (200, 50000, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--route-entries", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nni_general_timing.json"))
    args = ap.parse_args()
    rows = []
    for T, P, C in SHAPES:
        pb = wag_problem(T, P, C)
        cand = [v for v in range(pb.T, pb.N) if v != pb.root]
        entries = [(k, v) for v in cand for k in range(3)]
        rng = np.random.default_rng(5)
        picked = [entries[i] for i in sorted(rng.choice(len(entries), size=min(args.route_entries, len(entries)), replace=False))]
        trees = [rearranged(pb, v, k, pb.branch_lengths[v]) for k, v in picked]  # built before anything is timed
        under_root = sum(1 for v in cand if parents(pb)[v] == pb.root)
        with engine_from_problem(pb, rescale=RESCALE_NEVER, device=0) as e, engine_from_problem(pb, rescale=RESCALE_NEVER, device=0) as other:

            def engine_route():
                out = np.empty((len(picked), 3))
                for i, ((k, v), (left, right, bl)) in enumerate(zip(picked, trees)):
                    other.set_topology(left, right, pb.root)
                    other.set_branch_length(v, float(bl[v]))
                    lnl, d1, d2 = other.branch_hessian_diagonal()
                    out[i] = lnl, d1[v], d2[v]
                return out

            t0 = time.perf_counter()
            got = e.nni_log_likelihoods_general()
            first_call_ms = 1e3 * (time.perf_counter() - t0)
            ref = engine_route()
            mine = np.array([[a[k, v] for a in got] for k, v in picked])
            err = np.abs(mine - ref) / np.concatenate([np.abs(ref[:, :1]), np.maximum(1.0, np.abs(ref[:, 1:]))], axis=1)
            assert err[:, 0].max() <= 1e-10 and err[:, 1:].max() <= 1e-9, err.max(axis=0)
            lo = timed(lambda: e.nni_log_likelihoods_general(want_derivatives=False), args.reps, args.seconds)
            full = timed(lambda: e.nni_log_likelihoods_general(), args.reps, args.seconds)
            prof = e.nni_profile()
            route = timed(engine_route, 3, 0.0)
            scaled = [x * len(entries) / len(picked) for x in route]
            tiles = (P + 127) // 128 * 8
            rows.append({"taxa": T, "patterns": P, "categories": C, "entries": len(entries), "nni_lnl": stats(lo), "nni_lnl_d1_d2": stats(full),
                         "nni_lnl_calls_timed": len(lo), "nni_lnl_d1_d2_calls_timed": len(full), "engine_route_scaled": stats(scaled),
                         "engine_route_entries_timed": len(picked), "engine_route_ms_per_entry": float(np.median(route) / len(picked)),
                         "engine_route_scaled_over_nni_lnl_d1_d2": float(np.median(scaled) / np.median(full)), "scratch_bytes": prof["scratch_bytes"],
                         "mfma_products": (7 * len(cand) - under_root) * C * tiles, "first_call_ms": first_call_ms,
                         "max_rel_lnl_difference_to_engine_route": float(err[:, 0].max()), "max_d1_d2_difference_to_engine_route": float(err[:, 1:].max())})
            print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    line = json.dumps({"shapes": rows})
    print(line, flush=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
