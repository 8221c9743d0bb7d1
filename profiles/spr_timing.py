#!/usr/bin/env python3
"""Wall time of the whole SPR neighbourhood of the engine's tree by phyamd_spr_log_likelihoods (prune=None: every prune node, every
target edge) next to the only other way to get the same numbers: phyamd_gradient_batch_trees(want_gradient=False) over the same
rearranged trees, in the same process on the same data (synthetic, GTR-like model, Gamma categories):

  spr          lnL of every candidate (p, w), one call
  tree_batch   lnL of the same trees, each walked from the tips, in calls of at most `--batch` trees; their arrays are built once,
               outside the timing

Shapes: 69 taxa x 238 patterns x 4 categories and 200 taxa x 512 patterns x 4 categories.  Both forms return their results to the
host, so each timing ends device-synchronised.  Two warm-up rounds of each form, then `reps` repetitions of the call (at least
10) and `batch_reps` of the tree batch (at least 3: at 200 taxa it walks some 150 000 trees per repetition), the forms
alternating.  The two forms' lnL are compared entry by entry before anything is timed.  Prints one JSON line and writes it to
`--out` (committed as profiles/spr_timing.json when it was run on an MI355X).

usage: spr_timing.py [--reps K] [--batch-reps K] [--batch B] [--out FILE]"""
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

SHAPES = ((69, 238, 4), (200, 512, 4))


def candidates(tree):
    """(p, w, left, right, lengths) of every SPR candidate in phyamd_spr_log_likelihoods' definition: s = sibling(p) takes the place
    of u = parent(p) with both lengths, u goes onto the edge above w, whose halves get half its length"""
    T, N, root = tree.tip_count, tree.node_count, tree.root
    parent = -np.ones(N, dtype=np.int64)
    for n in range(T, N):
        parent[tree.left[n]] = parent[tree.right[n]] = n
    sibling = lambda n: tree.right[parent[n]] if tree.left[parent[n]] == n else tree.left[parent[n]]
    out = []
    for p in range(N):
        if p == root or parent[p] == root:
            continue
        u, s = parent[p], sibling(p)
        g = parent[u]
        below, stack = set(), [p]
        while stack:
            n = stack.pop()
            below.add(n)
            if n >= T:
                stack += [tree.left[n], tree.right[n]]
        for w in range(N):
            if w in (root, u, s) or w in below:
                continue
            x = parent[w]
            left, right, bl = tree.left.copy(), tree.right.copy(), tree.length.copy()
            (left if tree.left[g] == u else right)[g] = s
            bl[s] = tree.length[s] + tree.length[u]
            (left if tree.left[x] == w else right)[x] = u
            (left if tree.left[u] == s else right)[u] = w
            bl[u] = bl[w] = 0.5 * tree.length[w]
            out.append((p, w, left, right, bl))
    return out


def stats(x):
    x = np.asarray(x)
    return {"min_ms": float(x.min()), "median_ms": float(np.median(x)), "p10_ms": float(np.percentile(x, 10)), "p90_ms": float(np.percentile(x, 90))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batch-reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spr_timing.json"))
    args = ap.parse_args()
    reps, batch_reps = max(args.reps, 10), max(args.batch_reps, 3)
    rows = []
    for T, P, C in SHAPES:
        e, tree, _ = engine(T, P, C)
        cands = candidates(tree)
        calls = []  # the tree batch's arrays, per call
        for first in range(0, len(cands), args.batch):
            part = cands[first:first + args.batch]
            calls.append((np.ascontiguousarray([x[2] for x in part], dtype=np.int32), np.ascontiguousarray([x[3] for x in part], dtype=np.int32),
                          np.full(len(part), tree.root, dtype=np.int32), np.ascontiguousarray([x[4] for x in part])))
        at = (np.array([x[0] for x in cands]), np.array([x[1] for x in cands]))
        del cands
        with e:

            def spr():
                return e.spr_log_likelihoods()

            def batch():
                return np.concatenate([e.gradient_batch_trees(*c, want_gradient=False)[0] for c in calls])

            spr()
            prof = e.spr_profile()  # (before a tree batch has grown the shared scratch)
            for _ in range(2):
                got = spr()
                ref = batch()
            assert prof["candidates"] == len(ref) and np.isfinite(got).sum() == len(ref), prof
            err = float(np.max(np.abs(got[at] - ref) / np.abs(ref)))
            assert err <= 1e-10, err
            ts, tb = [], []
            for i in range(reps):
                t0 = time.perf_counter()
                spr()
                t1 = time.perf_counter()
                ts.append(1e3 * (t1 - t0))
                if i < batch_reps:
                    batch()
                    tb.append(1e3 * (time.perf_counter() - t1))
            rows.append({"taxa": T, "patterns": P, "categories": C, "candidates": len(ref), "spr": stats(ts), "tree_batch": stats(tb),
                         "tree_batch_calls": len(calls), "tree_batch_over_spr": float(np.median(tb) / np.median(ts)), "spr_chunks": prof["chunks"],
                         "spr_scratch_bytes": prof["scratch_bytes"], "max_rel_lnl_difference": err})
    line = json.dumps({"shapes": rows})
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
