#!/usr/bin/env python3
"""Wall time of the whole NNI neighbourhood of the engine's tree by phyamd_nni_log_likelihoods next to the only other way to get
the same numbers in one call: phyamd_gradient_batch_trees(want_gradient=False) over all 2 (T - 2) rearranged trees, in the same
process on the same data (synthetic, GTR-like model, Gamma categories):

  nni          lnL of the three arrangements of every internal edge (want_derivatives=False), and the same with d1 and d2
  tree_batch   lnL of the 2 (T - 2) neighbours, each walked from the tips; its arrays are built once, outside the timing

Shapes: 69 taxa x 238 patterns x 4 categories and 200 taxa x 512 patterns x 4 categories.  Both forms return their results to the
host, so each timing ends device-synchronised.  Two warm-up calls of each form, then `reps` repetitions (at least 10), the forms
alternating.  The two forms' lnL are compared entry by entry before anything is timed.  Prints one JSON line (committed as
profiles/nni_timing.json when it was run on an MI355X).

usage: nni_timing.py [--reps K]"""
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


def neighbours(tree):
    """(k, v, left, right) of the 2 (T - 2) rearranged trees in phyamd_nni_log_likelihoods' numbering: k = 1 exchanges left[v],
    k = 2 right[v] with v's sibling"""
    T, N, root = tree.tip_count, tree.node_count, tree.root
    parent = -np.ones(N, dtype=np.int64)
    for n in range(T, N):
        parent[tree.left[n]] = parent[tree.right[n]] = n
    out = []
    for v in range(T, N):
        if v == root:
            continue
        u = parent[v]
        for k in (1, 2):
            left, right = tree.left.copy(), tree.right.copy()
            of_u = left if left[u] != v else right
            of_v = left if k == 1 else right
            of_u[u], of_v[v] = of_v[v], of_u[u]
            out.append((k, v, left, right))
    return out


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
        e, tree, _ = engine(T, P, C)
        nb = neighbours(tree)
        left = np.ascontiguousarray([x[2] for x in nb], dtype=np.int32)
        right = np.ascontiguousarray([x[3] for x in nb], dtype=np.int32)
        roots = np.full(len(nb), tree.root, dtype=np.int32)
        bl = np.ascontiguousarray(np.repeat(tree.length[None, :], len(nb), axis=0))
        with e:

            def nni():
                return e.nni_log_likelihoods(want_derivatives=False)

            def nni_d():
                return e.nni_log_likelihoods()

            def batch():
                return e.gradient_batch_trees(left, right, roots, bl, want_gradient=False)

            nni()
            nni_scratch = e.nni_profile()["scratch_bytes"]  # (before a tree batch has grown the shared scratch)
            for _ in range(2):
                got, _, _ = nni()
                full = nni_d()
                ref, _ = batch()
            prof = e.batch_profile()
            assert prof["items_fast"] == len(nb) and prof["items_sequential"] == 0, prof
            assert np.array_equal(got, full[0], equal_nan=True)
            err = max(abs(got[k, v] - ref[i]) / abs(ref[i]) for i, (k, v, _, _) in enumerate(nb))
            assert err <= 1e-10, err
            tn, td, tb = [], [], []
            for _ in range(reps):
                t0 = time.perf_counter()
                nni()
                t1 = time.perf_counter()
                nni_d()
                t2 = time.perf_counter()
                batch()
                t3 = time.perf_counter()
                tn.append(1e3 * (t1 - t0))
                td.append(1e3 * (t2 - t1))
                tb.append(1e3 * (t3 - t2))
            rows.append({"taxa": T, "patterns": P, "categories": C, "neighbours": len(nb), "nni_lnl": stats(tn), "nni_lnl_d1_d2": stats(td),
                         "tree_batch_lnl": stats(tb), "tree_batch_over_nni_lnl": float(np.median(tb) / np.median(tn)),
                         "tree_batch_over_nni_lnl_d1_d2": float(np.median(tb) / np.median(td)), "tree_batch_chunks": prof["chunks"],
                         "tree_batch_scratch_bytes": prof["scratch_bytes"], "nni_scratch_bytes": nni_scratch,
                         "max_rel_lnl_difference": float(err)})
    print(json.dumps({"shapes": rows}), flush=True)


if __name__ == "__main__":
    main()
