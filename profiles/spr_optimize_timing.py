#!/usr/bin/env python3
"""Wall time of the three graft branches of every SPR regraft optimised by phyamd_spr_optimize next to the way a caller got the same
numbers before it: the rearranged trees built on the host, then phyamd_optimize_branch_lengths over them with only p, w and u
marked -- every tree walked from the tips, two launches per visit slot in lockstep -- in the same process on the same data
(synthetic, GTR-like model, Gamma categories):

  spr_optimize   every candidate (p, w) of the prune nodes, one call
  tree_batch     optimize_branch_lengths(trees, lengths, optimise=mask) over the same trees in calls of at most `--batch` trees;
                 their arrays are built once, outside the timing

Shapes: 69 taxa x 238 patterns x 4 categories, the full neighbourhood (prune=None), and 200 taxa x 512 patterns x 4 categories with a
fixed list of 16 prune nodes.  Bounds [1e-8, 10], tolerance 1e-8, at most 100 iterations, lnl_tolerance 1e-6, at most 50 passes.
Both forms return their results to the host, so each timing ends device-synchronised.  Before anything is timed the two forms are
compared entry by entry with max_passes = 1, where both make the same three visits: lnL 1e-10 relative on every entry, the three
lengths within the tolerance on at least nine entries in ten (an entry whose Newton iteration ends within rounding of the tolerance
may take one side a step further).  Run to convergence the two may stop a pass apart on an entry whose last gain is within rounding
of lnl_tolerance; the largest lnL difference and the share of entries with the same pass count are reported, not asserted.  Two
warm-up rounds of each form, then `reps` repetitions of the call (at least 10) and `batch_reps` of the tree batch (at least 3), the
forms alternating.  Prints one JSON line and writes it to `--out` (committed as profiles/spr_optimize_timing.json when it was run on
an MI355X).

usage: spr_optimize_timing.py [--reps K] [--batch-reps K] [--batch B] [--out FILE]"""
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
from spr_timing import candidates, stats  # noqa: E402

# (taxa, patterns, categories, prune nodes: None = every node)
SHAPES = ((69, 238, 4, None), (200, 512, 4, 16))
TOLERANCE = 1e-8


def prune_list(tree, count):
    """`count` prune nodes with candidates, fixed: spread evenly over the node ids, tips and internal nodes alike"""
    T, N, root = tree.tip_count, tree.node_count, tree.root
    live = [n for n in range(N) if n != root and n not in (tree.left[root], tree.right[root])]
    return [live[i * len(live) // count] for i in range(count)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batch-reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spr_optimize_timing.json"))
    args = ap.parse_args()
    reps, batch_reps = max(args.reps, 10), max(args.batch_reps, 3)
    rows = []
    for T, P, C, count in SHAPES:
        e, tree, _ = engine(T, P, C)
        N = tree.node_count
        prune = None if count is None else np.array(prune_list(tree, count), dtype=np.int32)
        row_of = {int(p): i for i, p in enumerate(range(N) if prune is None else prune)}
        cands = [c for c in candidates(tree) if c[0] in row_of]
        parent = -np.ones(N, dtype=np.int64)
        for n in range(T, N):
            parent[tree.left[n]] = parent[tree.right[n]] = n
        three = np.array([[c[0], c[1], parent[c[0]]] for c in cands])  # p, w, u
        calls = []  # the tree batch's arrays, per call
        for first in range(0, len(cands), args.batch):
            part = cands[first:first + args.batch]
            mask = np.zeros((len(part), N), dtype=np.uint8)
            mask[np.arange(len(part))[:, None], three[first:first + len(part)]] = 1
            calls.append(((np.ascontiguousarray([x[2] for x in part], dtype=np.int32), np.ascontiguousarray([x[3] for x in part], dtype=np.int32),
                           np.full(len(part), tree.root, dtype=np.int32)), np.ascontiguousarray([x[4] for x in part]), mask))
        at = (np.array([row_of[int(c[0])] for c in cands]), np.array([c[1] for c in cands]))
        del cands
        with e:

            def device(**kw):
                return e.spr_optimize(prune, tolerance=TOLERANCE, **kw)

            def batch(**kw):
                out = [e.optimize_branch_lengths(trees, bl, mask, tolerance=TOLERANCE, **kw) for trees, bl, mask in calls]
                lengths = np.concatenate([o[0] for o in out])
                return lengths[np.arange(len(lengths))[:, None], three], np.concatenate([o[1] for o in out]), np.concatenate([o[3] for o in out])

            device()
            scratch = e.spr_optimize_profile()["scratch_bytes"]  # (before the tree batch has grown the shared scratch)
            got, ref = device(max_passes=1), batch(max_passes=1)
            assert np.isfinite(got[1]).sum() == len(ref[1]), (np.isfinite(got[1]).sum(), len(ref[1]))
            err1 = float(np.max(np.abs(got[1][at] - ref[1]) / np.abs(ref[1])))
            dt = np.abs(got[0][at] - ref[0]).max(axis=1)
            within = float(np.mean(dt <= TOLERANCE))
            assert err1 <= 1e-10 and within >= 0.9, (err1, within, dt.max())
            for _ in range(2):
                got = device()
                prof = e.spr_optimize_profile()
                ref = batch()
            bprof = e.branch_optimize_profile()
            err = float(np.max(np.abs(got[1][at] - ref[1]) / np.abs(ref[1])))
            same_passes = float(np.mean(got[3][at] == ref[2]))
            ts, tb = [], []
            for i in range(reps):
                t0 = time.perf_counter()
                device()
                t1 = time.perf_counter()
                ts.append(1e3 * (t1 - t0))
                if i < batch_reps:
                    batch()
                    tb.append(1e3 * (time.perf_counter() - t1))
            rows.append({"taxa": T, "patterns": P, "categories": C, "prune_nodes": N if prune is None else len(prune), "candidates": len(ref[1]),
                         "spr_optimize": stats(ts), "tree_batch": stats(tb), "tree_batch_calls": len(calls),
                         "tree_batch_over_spr_optimize": float(np.median(tb) / np.median(ts)), "chunks": prof["chunks"], "visits": prof["visits"],
                         "iterations": prof["iterations"], "most_passes_of_an_entry": int(np.abs(got[3]).max()), "most_passes_of_the_last_tree_batch_call": bprof["passes"],
                         "scratch_bytes": scratch, "one_pass_max_rel_lnl_difference": err1, "one_pass_max_length_difference": float(dt.max()),
                         "one_pass_entries_within_tolerance": within, "converged_max_rel_lnl_difference": err, "converged_entries_with_the_same_passes": same_passes})
    line = json.dumps({"shapes": rows})
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
