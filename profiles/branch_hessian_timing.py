#!/usr/bin/env python3
"""Whole-call wall time of phyamd_branch_hessian next to the fastest route to the same matrix without it: central differences of
the analytic branch gradient through phyamd_gradient_batch over 2 (2T - 2) branch-length vectors (4T tree walks, half the digits).
Synthetic data, GTR-like model, Gamma(4); 69 taxa x 238 patterns and 200 taxa x 512 patterns.  Every call returns its result to the
host, so each timing ends device-synchronised; two warm-up calls first.  branch_hessian_ms includes the evaluation of lnL and the
gradient the call triggers after an input changed (the baseline evaluates everything too); _resident_ms is the matrix alone.  Prints one JSON line per shape and writes them all to
profiles/branch_hessian_timing.json (--out).

usage: branch_hessian_timing.py [--reps K] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))

sys.path.insert(0, os.path.join(ROOT, "tests"))

from golden_util import reversible_eigen  # noqa: E402
from hessian_timing import timed  # noqa: E402
from physher_amd import synth  # noqa: E402
from physher_amd.engine import RESCALE_AUTO, Engine  # noqa: E402

SHAPES = [(69, 238, 4), (200, 512, 4)]


def engine(T, P, C, seed=7):
    """(engine, tree, category rates, proportions)"""
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
    rates = rates / (rates * props).sum()
    e.set_category_rates(rates, props)
    e.set_pattern_weights(np.ones(P))
    states = synth.evolve(tree, P, 4, rng)
    for t in range(T):
        e.set_tip_states(t, states[t])
    return e, tree, rates, props


def difference_hessian(e, tree, rates, props, h=1e-4):
    """central differences of the branch gradient in every branch length, all 2 (N - 1) vectors in one gradient_batch call"""
    branches = [n for n in range(e.N) if n != tree.root]
    lengths = np.tile(np.asarray(tree.length, dtype=np.float64), (2 * len(branches), 1))
    step = np.empty(len(branches))
    for i, b in enumerate(branches):
        step[i] = min(h, 0.1 * tree.length[b])
        lengths[2 * i, b] += step[i]
        lengths[2 * i + 1, b] -= step[i]
    _, cg = e.gradient_batch(lengths)
    g = cg @ (rates * props) if e.C > 1 else cg[:, :, 0]
    H = np.zeros((e.N, e.N))
    for i, b in enumerate(branches):
        H[:, b] = (g[2 * i] - g[2 * i + 1]) / (2 * step[i])
    H[tree.root, :] = 0.0
    return H


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "branch_hessian_timing.json"))
    args = ap.parse_args()
    rows = []
    for T, P, C in SHAPES:
        e, tree, rates, props = engine(T, P, C)
        out = {"taxa": T, "patterns": P, "states": 4, "categories": C}
        with e:
            def fresh():  # as after new branch lengths: the call evaluates lnL and the gradient, then forms the matrix
                e.update_all_nodes()
                e.branch_hessian()

            out["branch_hessian_ms"] = timed(fresh, args.reps)
            out["branch_hessian_resident_ms"] = timed(lambda: e.branch_hessian(), args.reps)  # the partials are resident and current
            prof = e.hessian_profile()
            out.update(pairs=prof["pairs"], chunks=prof["chunks"], scratch_bytes=prof["scratch_bytes"])
            out["hessian_diagonal_ms"] = timed(lambda: e.branch_hessian_diagonal(), args.reps)
            out["difference_baseline_ms"] = timed(lambda: difference_hessian(e, tree, rates, props), max(2, args.reps // 2))
            out["speedup"] = out["difference_baseline_ms"] / out["branch_hessian_ms"]
            H = e.branch_hessian()[2]
            D = difference_hessian(e, tree, rates, props)
            out["difference_baseline_max_rel_error"] = float(np.abs(D - H).max() / max(1.0, np.abs(H).max()))
        rows.append(out)
        print(json.dumps(out), flush=True)
    with open(args.out, "w") as f:
        json.dump({"shapes": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
