#!/usr/bin/env python3
"""Wall time of the optimised central branch of every NNI neighbour of the engine's tree by phyamd_nni_optimize next to the way a
caller got the same numbers before it: the same rule on the host, every entry at once, over repeated
phyamd_nni_log_likelihoods(central_lengths) calls -- one per round of proposals, each a whole walk of the tree, until every entry
has stopped, and one more at the final lengths -- in the same process on the same data (synthetic, GTR-like model, Gamma
categories):

  device   nni_optimize(): one walk, the coefficient kernel, the iteration of every entry in one launch
  host     host_rule(): rounds of nni_log_likelihoods, the rule in NumPy between them

Shapes: 69 taxa x 238 patterns x 4 categories and 200 taxa x 512 patterns x 4 categories; bounds [1e-8, 10], tolerance 1e-8, at most
100 iterations, from the tree's own lengths.  Both forms return their results to the host, so each timing ends
device-synchronised.  Before anything is timed the two forms are compared entry by entry: lnL 1e-10 relative, d1 and d2
1e-9 * max(1, |ref|) -- each side at its own t* --, the lengths within the tolerance and the iteration counts within one on at
least nine entries in ten (a halving step that lands on the tolerance may take one side a round further).  Two warm-up calls of each form,
then `reps` repetitions (at least 10), the forms alternating.  Prints one JSON line and writes it to
profiles/nni_optimize_timing.json.

usage: nni_optimize_timing.py [--reps K]"""
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
from nni_timing import stats  # noqa: E402

SHAPES = ((69, 238, 4), (200, 512, 4))
LOWER, UPPER, TOLERANCE, MAX_ITERATIONS = 1e-8, 10.0, 1e-8, 100


def host_rule(e, start, cand):
    """phyamd_nni_optimize's rule for every entry at once on nni_log_likelihoods: (lengths, lnl, d1, d2, iterations, rounds)"""
    N = start.shape[1]
    t = np.zeros((3, N))
    t[:, cand] = np.clip(start[:, cand], LOWER, UPPER)
    a, b = np.full((3, N), LOWER), np.full((3, N), UPPER)
    live = np.zeros((3, N), dtype=bool)
    live[:, cand] = True
    it = np.zeros((3, N), dtype=np.int32)
    rounds = 0
    while live.any() and rounds < MAX_ITERATIONS:
        lnl, d1, d2 = e.nni_log_likelihoods(t)
        rounds += 1
        bad = live & ~np.isfinite(lnl)
        it[bad] = -rounds
        live &= ~bad
        up = live & (d1 > 0)
        a[up] = t[up]
        b[live & ~up] = t[live & ~up]
        with np.errstate(divide="ignore", invalid="ignore"):
            nxt = t - d1 / d2
        newton = (d2 < 0) & (a < nxt) & (nxt < b)
        nxt = np.where(newton, nxt, 0.5 * (a + b))
        done = live & (np.abs(nxt - t) <= TOLERANCE)
        t[live] = nxt[live]
        it[done] = rounds
        live &= ~done
    it[live] = -rounds
    lnl, d1, d2 = e.nni_log_likelihoods(t)
    t[:, [n for n in range(N) if n not in set(cand)]] = np.nan
    return t, lnl, d1, d2, it, rounds + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    reps = max(args.reps, 10)
    rows = []
    for T, P, C in SHAPES:
        e, tree, _ = engine(T, P, C)
        cand = [v for v in range(T, 2 * T - 1) if v != tree.root]
        start = np.ascontiguousarray(np.repeat(tree.length[None, :], 3, axis=0))
        with e:

            def device():
                return e.nni_optimize(lower=LOWER, upper=UPPER, tolerance=TOLERANCE, max_iterations=MAX_ITERATIONS)

            def host():
                return host_rule(e, start, cand)

            for _ in range(2):
                dev = device()
                ref = host()
            prof = e.nni_optimize_profile()
            err = [float(np.max(np.abs(dev[1][:, cand] - ref[1][:, cand]) / np.abs(ref[1][:, cand])))]
            for i in (2, 3):
                err.append(float(np.max(np.abs(dev[i][:, cand] - ref[i][:, cand]) / np.maximum(1.0, np.abs(ref[i][:, cand])))))
            assert err[0] <= 1e-10 and err[1] <= 1e-9 and err[2] <= 1e-9, err
            dt, dn = np.abs(dev[0][:, cand] - ref[0][:, cand]), np.abs(dev[4][:, cand] - ref[4][:, cand])
            agree = float(np.mean((dt <= TOLERANCE) & (dn <= 1)))
            assert agree >= 0.9 and dt.max() <= 2 * TOLERANCE, (agree, dt.max())
            td, th = [], []
            for _ in range(reps):
                t0 = time.perf_counter()
                device()
                t1 = time.perf_counter()
                host()
                t2 = time.perf_counter()
                td.append(1e3 * (t1 - t0))
                th.append(1e3 * (t2 - t1))
            rows.append({"taxa": T, "patterns": P, "categories": C, "entries": 3 * len(cand), "device": stats(td), "host_rule": stats(th),
                         "host_over_device": float(np.median(th) / np.median(td)), "host_rounds": ref[5], "device_iterations": prof["iterations"],
                         "device_max_iterations_of_an_entry": int(np.abs(dev[4]).max()), "device_chunks": prof["chunks"],
                         "scratch_bytes": prof["scratch_bytes"], "max_rel_lnl_difference": err[0], "max_d1_difference": err[1], "max_d2_difference": err[2],
                         "max_length_difference": float(dt.max()), "entries_within_tolerance_and_one_iteration": agree})
    line = json.dumps({"shapes": rows})
    print(line, flush=True)
    with open(os.path.join(ROOT, "profiles", "nni_optimize_timing.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
