#!/usr/bin/env python3
"""Wall time of B evaluations by phyamd_gradient_batch next to the loop it replaces -- phyamd_set_branch_lengths +
phyamd_gradient per item -- on the same engine, in the same process (synthetic data, GTR-like model, Gamma categories).  Both
forms return their results to the host, so each timing ends device-synchronised.  Two warm-up calls of each form, then `reps`
repetitions (at least 10) each, alternating.  Prints one JSON line: per (shape, B) min / median of both forms in ms and the ratio
loop median / batch median (committed as profiles/batch_timing.json).

--sweep: the crossover behind the fast path's pattern bound (BATCH_MAX_PATTERNS, phyamd_shard.inc) instead: 64 and 500 taxa,
2 048 .. 65 536 patterns, B = 4 and 32, with the bound lifted for the run (PHYAMD_BATCH_MAX_PATTERNS, read when an engine is
created), so that the batched walk itself is timed on both sides of it (committed as profiles/batch_sweep.json).

usage: batch_timing.py [--reps K] [--skip-large] [--sweep]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from golden_util import reversible_eigen  # noqa: E402
from physher_amd import synth  # noqa: E402
from physher_amd.engine import RESCALE_AUTO, Engine  # noqa: E402

# (taxa, patterns, categories, batch sizes)
SHAPES = [(69, 238, 4, (1, 16, 128)), (64, 512, 4, (1, 16, 128)), (500, 100_000, 4, (4,))]
SWEEP = [(T, P, 4, (4, 32)) for T in (64, 500) for P in (2048, 8192, 32768, 65536)]


def engine(T, P, C, seed=7):
    rng = np.random.default_rng(seed)
    tree = synth.random_tree(T, rng)
    e = Engine(T, P, 4, C, device=0, rescale=RESCALE_AUTO)
    e.set_topology(tree.left, tree.right, tree.root)
    e.set_branch_lengths(tree.length)
    freqs = rng.dirichlet(np.full(4, 5.0))
    r = rng.uniform(0.5, 3.0, size=(4, 4))
    e.set_eigen(*reversible_eigen(0.5 * (r + r.T), freqs))
    e.set_frequencies(freqs)
    rates = np.sort(rng.gamma(0.5, 2.0, size=C)) + 0.05
    props = np.full(C, 1.0 / C)
    e.set_category_rates(rates / (rates * props).sum(), props)
    e.set_pattern_weights(np.ones(P))
    states = synth.evolve(tree, P, 4, rng)
    for t in range(T):
        e.set_tip_states(t, states[t])
    return e, tree, rng


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--skip-large", action="store_true")
    ap.add_argument("--sweep", action="store_true")
    args = ap.parse_args()
    if args.sweep:
        os.environ["PHYAMD_BATCH_MAX_PATTERNS"] = str(1 << 30)
    rows = []
    for T, P, C, batches in SWEEP if args.sweep else SHAPES:
        if args.skip_large and P >= 100_000:
            continue
        e, tree, rng = engine(T, P, C)
        with e:
            for B in batches:
                bl = np.ascontiguousarray(tree.length[None, :] * rng.uniform(0.5, 1.8, size=(B, e.N)))

                def batch():
                    return e.gradient_batch(bl)

                def loop():
                    out = []
                    for b in range(B):
                        e.set_branch_lengths(bl[b])
                        out.append(e.gradient())
                    return out

                for _ in range(2):
                    got = batch()
                    ref = loop()
                prof = e.batch_profile()
                err = max(abs(got[0][b] - ref[b][0]) / abs(ref[b][0]) for b in range(B))
                tb, tl = [], []
                for _ in range(max(args.reps, 10)):
                    t0 = time.perf_counter()
                    batch()
                    t1 = time.perf_counter()
                    loop()
                    t2 = time.perf_counter()
                    tb.append(1e3 * (t1 - t0))
                    tl.append(1e3 * (t2 - t1))
                rows.append({"taxa": T, "patterns": P, "categories": C, "items": B, "batch_min_ms": min(tb), "batch_median_ms": float(np.median(tb)),
                             "loop_min_ms": min(tl), "loop_median_ms": float(np.median(tl)), "ratio": float(np.median(tl) / np.median(tb)),
                             "batch_median_below_loop_min": bool(np.median(tb) < min(tl)), "items_fast": prof["items_fast"], "chunks": prof["chunks"],
                             "scratch_bytes": prof["scratch_bytes"], "max_rel_lnl_difference": err})
    print(json.dumps({"pattern_bound_lifted": bool(args.sweep), "shapes": rows}), flush=True)


if __name__ == "__main__":
    main()
