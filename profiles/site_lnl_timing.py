#!/usr/bin/env python3
"""Wall time of phyamd_pattern_log_likelihoods_trees -- the per-pattern log-likelihoods of B trees and R RELL replicates of them in
one call -- next to the only other way to get the same numbers, in the same process on the same data (synthetic, GTR-like model,
4 Gamma categories; 69 taxa x 238 patterns and 200 taxa x 5000 patterns; 16 and 128 random trees; 0 and 1024 bootstrap rows):

  call  Engine.pattern_log_likelihoods_trees: lnl [B], pattern_lnl [B, P] and, with replicates, replicate_lnl [R, B], on the host
  loop  per tree phyamd_set_topology + phyamd_set_branch_lengths + phyamd_log_likelihood + phyamd_get_pattern_log_likelihoods on ONE
        other engine (phyamd_set_topology on the call's engine would take its scratch with it), then NumPy W @ ell.T

Both forms end with their results on the host, so each timing ends device-synchronised.  The scratch per item of the call and of
phyamd_gradient_batch_trees in its lnL-only form on the same trees is read from an engine that has made no other call.  Two warm-up rounds of each form, then
`reps` repetitions (at least 10), the two forms alternating.  Prints one JSON line (committed as profiles/site_lnl_timing.json).

usage: site_lnl_timing.py [--reps K]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))

from batch_timing import engine  # noqa: E402
from physher_amd import resampling, synth  # noqa: E402

SHAPES = ((69, 238, 4), (200, 5000, 4))
COUNTS = (16, 128)
REPLICATES = (0, 1024)


def stats(x):
    x = np.asarray(x)
    return {"min_ms": float(x.min()), "median_ms": float(np.median(x)), "p10_ms": float(np.percentile(x, 10)), "p90_ms": float(np.percentile(x, 90))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    reps = max(args.reps, 10)
    rows = []
    for T, P, C in SHAPES:
        e, tree, rng = engine(T, P, C)
        other, _, _ = engine(T, P, C)
        with e, other:
            for B in COUNTS:
                trees = [synth.random_tree(T, rng) for _ in range(B)]
                left = np.ascontiguousarray([t.left for t in trees], dtype=np.int32)
                right = np.ascontiguousarray([t.right for t in trees], dtype=np.int32)
                roots = np.ascontiguousarray([t.root for t in trees], dtype=np.int32)
                bl = np.ascontiguousarray([t.length for t in trees], dtype=np.float64)
                for R in REPLICATES:
                    W = resampling.bootstrap_weights(np.ones(P), R, rng) if R else None

                    def call():
                        return e.pattern_log_likelihoods_trees(left, right, roots, bl, replicate_weights=W)

                    def loop():
                        lnl, ell = np.empty(B), np.empty((B, P))
                        for b in range(B):
                            other.set_topology(left[b], right[b], int(roots[b]))
                            other.set_branch_lengths(bl[b])
                            lnl[b] = other.log_likelihood()
                            ell[b] = other.pattern_log_likelihoods()
                        return lnl, ell, (W @ ell.T if R else None)

                    for _ in range(2):
                        got, ref = call(), loop()
                    prof = e.site_lnl_profile()
                    assert prof["items"] == B, prof
                    err = float(np.abs(got[1] - ref[1]).max())
                    rerr = float(np.abs(got[2] - ref[2]).max() / np.abs(ref[2]).max()) if R else None
                    tc, tl = [], []
                    for _ in range(reps):
                        t0 = time.perf_counter()
                        call()
                        t1 = time.perf_counter()
                        loop()
                        t2 = time.perf_counter()
                        tc.append(1e3 * (t1 - t0))
                        tl.append(1e3 * (t2 - t1))
                    # the scratch of either call on an engine that has made no other (without a cap the scratch keeps what earlier calls needed)
                    with engine(T, P, C)[0] as fresh:
                        fresh.pattern_log_likelihoods_trees(left, right, roots, bl, replicate_weights=W)
                        scratch = fresh.site_lnl_profile()["scratch_bytes"]
                    with engine(T, P, C)[0] as fresh:
                        fresh.gradient_batch_trees(left, right, roots, bl, want_gradient=False)
                        tree_scratch = fresh.batch_profile()["scratch_bytes"]
                    rows.append({"taxa": T, "patterns": P, "categories": C, "items": B, "replicates": R, "call": stats(tc), "loop": stats(tl),
                                 "loop_over_call": float(np.median(tl) / np.median(tc)), "chunks": prof["chunks"], "replicate_chunks": prof["replicate_chunks"],
                                 "lower_slots": prof["lower_slots"], "scratch_bytes": scratch, "scratch_bytes_per_item": scratch / B,
                                 "lnl_only_tree_batch_scratch_bytes_per_item": tree_scratch / B, "max_pattern_lnl_difference_to_loop": err,
                                 "max_rel_replicate_difference_to_loop": rerr})
                    print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    print(json.dumps({"shapes": rows}), flush=True)


if __name__ == "__main__":
    main()
