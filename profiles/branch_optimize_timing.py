#!/usr/bin/env python3
"""Wall time of all branch lengths of a batch of trees optimised by phyamd_optimize_branch_lengths next to the host loop it
replaces, in the same process on the same data (synthetic, GTR-like model, Gamma categories):

  device   optimize_branch_lengths(trees, lengths): every tree of the batch in one call
  host     per tree set_topology and set_branch_lengths, then pass after pass, per visit, the same rule over
           branch_log_likelihood(node, t) -- one host round trip per trial -- and a set_branch_length to accept; the same stop
           test on the lnL of the pass's last visit

Shapes: 69 taxa x 238 patterns x 4 categories and 200 taxa x 512 patterns x 4 categories, with 1 / 16 / 128 trees -- NNI neighbours
of the tree the alignment was simulated on, what a hill-climb hands over after ranking them -- from that tree's lengths; bounds [1e-8, 10], tolerance 1e-8, at most 100 iterations, lnl_tolerance 1e-6, at
most 50 passes.  Both forms leave their results on the host, so each timing ends device-synchronised.  Before anything is timed
the two forms are compared on the first tree: lnL at the result 1e-8 relative (the two stop after the same rule on values that
differ in rounding, so a pass more or less is possible).  Two warm-up calls of the device form and one of the host loop (on the
first tree), then `reps` repetitions of the device call (at least 10) and `host_reps` (at least 3) of the host loop over the first
min(B, host_trees) trees, scaled to B trees: the loop's cost per tree does not depend on the batch.  Prints one JSON line and
writes it to profiles/branch_optimize_timing.json.

usage: branch_optimize_timing.py [--reps K] [--host-reps K] [--host-trees K]"""
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
from nni_timing import neighbours, stats  # noqa: E402

SHAPES = ((69, 238, 4), (200, 512, 4))
COUNTS = (1, 16, 128)
LOWER, UPPER, TOLERANCE, MAX_ITERATIONS, LNL_TOLERANCE, MAX_PASSES = 1e-8, 10.0, 1e-8, 100, 1e-6, 50


def post_order(left, right, root, T):
    out, stack = [], [(root, False)]
    while stack:
        n, done = stack.pop()
        if done or n < T:
            if n != root:
                out.append(n)
            continue
        stack.extend([(n, True), (int(right[n]), False), (int(left[n]), False)])
    return out


def host_visit(e, n, tn):
    """the rule of one visit over branch_log_likelihood: (the length the visit leaves, lnL there, trials)"""
    t0 = min(max(tn, LOWER), UPPER)
    t, a, b, l0, trials = t0, LOWER, UPPER, None, 0
    for _ in range(MAX_ITERATIONS):
        lnl, d1, d2 = e.branch_log_likelihood(n, t)
        trials += 1
        if l0 is None:
            l0 = lnl
        if not np.isfinite(lnl):
            return None, lnl, trials
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


def host_loop(e, left, right, root, lengths):
    """one tree through the host loop: (lengths, lnl, passes, trials)"""
    e.set_topology(left, right, root)
    e.set_branch_lengths(lengths)
    out = np.array(lengths, dtype=np.float64)
    order = post_order(left, right, root, e.T)
    previous, trials = e.log_likelihood(), 0
    for p in range(1, MAX_PASSES + 1):
        lnl = previous
        for n in order:
            t, lnl, k = host_visit(e, n, out[n])
            trials += k
            if t is None:
                return out, lnl, -p, trials
            out[n] = t
            e.set_branch_length(n, t)
        if lnl - previous <= LNL_TOLERANCE:
            return out, lnl, p, trials
        previous = lnl
    return out, previous, -MAX_PASSES, trials


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--host-trees", type=int, default=1)
    args = ap.parse_args()
    reps, host_reps, host_trees = max(args.reps, 10), max(args.host_reps, 3), max(args.host_trees, 1)
    rows = []
    for T, P, C in SHAPES:
        e, own, _ = engine(T, P, C)
        nb = neighbours(own)
        other, _, _ = engine(T, P, C)  # the host loop's engine: its topology changes tree by tree
        with e, other:
            for B in COUNTS:
                left = np.ascontiguousarray([x[2] for x in nb[:B]], dtype=np.int32)
                right = np.ascontiguousarray([x[3] for x in nb[:B]], dtype=np.int32)
                roots = np.full(B, own.root, dtype=np.int32)
                bl = np.ascontiguousarray(np.repeat(np.asarray(own.length, dtype=np.float64)[None, :], B, axis=0))
                bl[:, own.root] = 0.0

                def device():
                    return e.optimize_branch_lengths((left, right, roots), bl, lower=LOWER, upper=UPPER, tolerance=TOLERANCE, max_iterations=MAX_ITERATIONS,
                                                     lnl_tolerance=LNL_TOLERANCE, max_passes=MAX_PASSES)

                def host(count):
                    return [host_loop(other, left[i], right[i], int(roots[i]), bl[i]) for i in range(count)]

                for _ in range(2):
                    dev = device()
                prof = e.branch_optimize_profile()
                ref = host(1)[0]
                err = float(abs(dev[1][0] - ref[1]) / abs(ref[1]))
                assert err <= 1e-8, (dev[1][0], ref[1])
                nh = min(B, host_trees)
                td, th = [], []
                for _ in range(reps):
                    t0 = time.perf_counter()
                    device()
                    td.append(1e3 * (time.perf_counter() - t0))
                for _ in range(host_reps):
                    t0 = time.perf_counter()
                    host(nh)
                    th.append(1e3 * (time.perf_counter() - t0) * B / nh)
                ratio = float(np.median(th) / np.median(td))
                rows.append({"taxa": T, "patterns": P, "categories": C, "trees": B, "device": stats(td), "host_loop": stats(th), "host_trees_timed": nh,
                             "host_over_device": ratio, "device_is_slower": bool(ratio < 1.0), "device_passes": [int(dev[3].min()), int(dev[3].max())],
                             "host_passes_first_tree": ref[2], "host_trials_first_tree": ref[3], "device_visits": prof["visits"],
                             "device_iterations": prof["iterations"], "device_chunks": prof["chunks"], "scratch_bytes": prof["scratch_bytes"],
                             "rel_lnl_difference_first_tree": err, "max_length_difference_first_tree": float(np.abs(dev[0][0] - ref[0]).max())})
    line = json.dumps({"shapes": rows})
    print(line, flush=True)
    with open(os.path.join(ROOT, "profiles", "branch_optimize_timing.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
