#!/usr/bin/env python3
"""Wall time of B TREES by phyamd_gradient_batch_trees next to the two calls it is to be judged against, in the same process on
the same data (69 taxa x 238 patterns x 4 categories, synthetic, GTR-like model, Gamma categories):

  loop     phyamd_set_topology + phyamd_set_branch_lengths + phyamd_gradient per item on ONE other engine: the only way to
           evaluate another topology without the call
  lengths  phyamd_gradient_batch with the same count on the engine's own tree: what per-item op lists cost on top of shared ones

Two item sets per count (16, 128): the NNI neighbourhood of the engine's tree (2 x 67 rearrangements, cut or cycled to the count,
lengths carried over) and random topologies.  All three forms return their results to the host, so each timing ends
device-synchronised.  Two warm-up calls of each form, then `reps` repetitions (at least 10), the three forms alternating.  The
host time a tree batch spends building and uploading its op lists comes from the engine itself (PHYAMD_BATCH_TRACE=1, read when an
engine is created: one line per chunk on stderr, which this script collects in a file).  Prints one JSON line (committed as
profiles/tree_batch_timing.json).

usage: tree_batch_timing.py [--reps K]"""
import argparse
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))

os.environ["PHYAMD_BATCH_TRACE"] = "1"

from batch_timing import engine  # noqa: E402
from physher_amd import synth  # noqa: E402

T, P, C = 69, 238, 4
COUNTS = (16, 128)


def nni_neighbourhood(tree):
    """all 2 x (internal non-root edges) NNI rearrangements: a child of v changes places with v's sibling"""
    N, root = tree.node_count, tree.root
    parent = -np.ones(N, dtype=np.int64)
    for n in range(tree.tip_count, N):
        parent[tree.left[n]] = parent[tree.right[n]] = n
    out = []
    for v in range(tree.tip_count, N):
        if v == root:
            continue
        p = parent[v]
        for side in (0, 1):
            left, right = tree.left.copy(), tree.right.copy()
            kids = left if side == 0 else right
            if left[p] == v:
                kids[v], right[p] = right[p], kids[v]
            else:
                kids[v], left[p] = left[p], kids[v]
            out.append((left, right, root, tree.length.copy()))
    return out


def stats(x):
    x = np.asarray(x)
    return {"min_ms": float(x.min()), "median_ms": float(np.median(x)), "p10_ms": float(np.percentile(x, 10)), "p90_ms": float(np.percentile(x, 90))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    reps = max(args.reps, 10)
    trace = tempfile.TemporaryFile(mode="w+b")
    sys.stderr.flush()
    stderr = os.dup(2)
    os.dup2(trace.fileno(), 2)  # the engine's per-chunk lines
    try:
        measure(reps, trace)
    finally:
        sys.stderr.flush()
        os.dup2(stderr, 2)


def measure(reps, trace):

    def chunks_traced():
        trace.seek(0)
        text = trace.read().decode()
        trace.seek(0)
        trace.truncate()
        return [(int(m[0]), float(m[1]), float(m[2])) for m in re.findall(r"chunk (\d+) items \d+ slots \d+ build_ms (\S+) upload_ms (\S+)", text)]

    e, tree, rng = engine(T, P, C)
    other, _, _ = engine(T, P, C)  # the loop's engine: phyamd_set_topology on `e` would take the batch's scratch with it
    nni = nni_neighbourhood(tree)
    rows = []
    with e, other:
        for B in COUNTS:
            sets = {"nni": [nni[i % len(nni)] for i in range(B)], "random": []}
            for _ in range(B):
                t = synth.random_tree(T, rng)
                sets["random"].append((t.left, t.right, t.root, t.length))
            shared = np.ascontiguousarray(tree.length[None, :] * rng.uniform(0.5, 1.8, size=(B, e.N)))
            for name, trees in sets.items():
                left = np.ascontiguousarray([t[0] for t in trees], dtype=np.int32)
                right = np.ascontiguousarray([t[1] for t in trees], dtype=np.int32)
                roots = np.ascontiguousarray([t[2] for t in trees], dtype=np.int32)
                bl = np.ascontiguousarray([t[3] for t in trees], dtype=np.float64)

                def batch():
                    return e.gradient_batch_trees(left, right, roots, bl)

                def loop():
                    out = []
                    for b in range(B):
                        other.set_topology(left[b], right[b], int(roots[b]))
                        other.set_branch_lengths(bl[b])
                        out.append(other.gradient())
                    return out

                def lengths():
                    return e.gradient_batch(shared)

                for _ in range(2):
                    got, ref = batch(), loop()
                    lengths()
                    assert e.batch_profile()["items_fast"] == B
                    batch()
                prof = e.batch_profile()
                assert prof["items_fast"] == B and prof["items_sequential"] == 0, prof
                err = max(abs(got[0][b] - ref[b][0]) / abs(ref[b][0]) for b in range(B))
                gerr = max(np.abs(got[1][b] - ref[b][1]).max() / max(1.0, np.abs(ref[b][1]).max()) for b in range(B))
                chunks_traced()
                tb, tl, ts = [], [], []
                for _ in range(reps):
                    t0 = time.perf_counter()
                    batch()
                    t1 = time.perf_counter()
                    loop()
                    t2 = time.perf_counter()
                    lengths()
                    t3 = time.perf_counter()
                    tb.append(1e3 * (t1 - t0))
                    tl.append(1e3 * (t2 - t1))
                    ts.append(1e3 * (t3 - t2))
                traced = chunks_traced()
                per_call = len(traced) // reps
                build = [sum(x[1] for x in traced[r * per_call:(r + 1) * per_call]) for r in range(reps)]
                upload = [sum(x[2] for x in traced[r * per_call:(r + 1) * per_call]) for r in range(reps)]
                rows.append({"taxa": T, "patterns": P, "categories": C, "items": B, "set": name, "tree_batch": stats(tb), "loop": stats(tl),
                             "lengths_batch": stats(ts), "loop_over_tree_batch": float(np.median(tl) / np.median(tb)),
                             "tree_batch_over_lengths_batch": float(np.median(tb) / np.median(ts)), "chunks": prof["chunks"],
                             "op_list_build_median_ms_per_call": float(np.median(build)), "op_list_upload_median_ms_per_call": float(np.median(upload)),
                             "scratch_bytes": prof["scratch_bytes"], "max_rel_lnl_difference_to_loop": err, "max_gradient_difference_to_loop": gerr})
    print(json.dumps({"shapes": rows}), flush=True)


if __name__ == "__main__":
    main()
