#!/usr/bin/env python3
"""Wall time of B replicates by phyamd_gradient_batch_weights next to the loop it replaces on the same engine, in the same process
(synthetic data, GTR-like model, Gamma-4): phyamd_set_pattern_weights + phyamd_gradient per replicate on the shared-lengths path,
and with phyamd_set_branch_lengths per replicate on the path with a length vector per item.  The weight rows are bootstrap draws
of the alignment's sites.  Both forms return their results to the host, so each timing ends device-synchronised.  Two warm-up
calls of each form, then alternating repetitions: at least `reps` (at least 10) and as many as bring each form's timed window to
half a second.  Prints one JSON line: per (shape, B, path) min / median of both forms in ms and the ratio loop median / call
median (committed as profiles/weight_batch_timing.json).

usage: weight_batch_timing.py [--reps K]"""
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
from physher_amd import resampling  # noqa: E402

# (taxa, patterns, categories, replicate counts)
SHAPES = [(69, 238, 4, (16, 128, 1024)), (200, 512, 4, (16, 128, 1024))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    rows = []
    for T, P, C, batches in SHAPES:
        e, tree, rng = engine(T, P, C)
        with e:
            own = rng.integers(1, 5, size=P).astype(np.float64)
            e.set_pattern_weights(own)
            for B in batches:
                W = resampling.bootstrap_weights(own, B, rng)
                bl = np.ascontiguousarray(tree.length[None, :] * rng.uniform(0.5, 1.8, size=(B, e.N)))
                for path, lengths in (("shared_lengths", None), ("per_item_lengths", bl)):

                    def call():
                        return e.gradient_batch_weights(W, lengths)

                    def loop():
                        out = []
                        for b in range(B):
                            e.set_pattern_weights(W[b])
                            if lengths is not None:
                                e.set_branch_lengths(lengths[b])
                            out.append(e.gradient())
                        e.set_pattern_weights(own)
                        if lengths is not None:
                            e.set_branch_lengths(tree.length)
                        return out

                    for _ in range(2):
                        t0 = time.perf_counter()
                        got = call()
                        t1 = time.perf_counter()
                        ref = loop()
                        t2 = time.perf_counter()
                    prof = e.weight_batch_profile()
                    err = max(abs(got[0][b] - ref[b][0]) / abs(ref[b][0]) for b in range(B))
                    gerr = max(float(np.abs(got[1][b] - ref[b][1]).max() / max(1.0, np.abs(ref[b][1]).max())) for b in range(B))
                    reps = max(args.reps, 10, int(np.ceil(0.5 / max(min(t1 - t0, t2 - t1), 1e-6))))
                    reps = min(reps, 2000)
                    tc, tl = [], []
                    for _ in range(reps):
                        t0 = time.perf_counter()
                        call()
                        t1 = time.perf_counter()
                        loop()
                        t2 = time.perf_counter()
                        tc.append(1e3 * (t1 - t0))
                        tl.append(1e3 * (t2 - t1))
                    rows.append({"taxa": T, "patterns": P, "categories": C, "replicates": B, "path": path, "repetitions": reps,
                                 "call_min_ms": min(tc), "call_median_ms": float(np.median(tc)), "loop_min_ms": min(tl),
                                 "loop_median_ms": float(np.median(tl)), "ratio": float(np.median(tl) / np.median(tc)),
                                 "call_median_below_loop_min": bool(np.median(tc) < min(tl)), "items_fast": prof["items_fast"],
                                 "item_chunks": prof["item_chunks"], "pattern_chunks": prof["pattern_chunks"], "walks": prof["walks"],
                                 "scratch_bytes": prof["scratch_bytes"], "max_rel_lnl_difference": err, "max_rel_gradient_difference": gerr})
                    print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    print(json.dumps({"shapes": rows}), flush=True)


if __name__ == "__main__":
    main()
