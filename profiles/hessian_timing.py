#!/usr/bin/env python3
"""Wall time of phyamd_branch_hessian_diagonal next to phyamd_branch_gradient and the per-branch phyamd_branch_log_likelihood loop
it replaces, at the bench shapes (cfg2..cfg5; synthetic data, GTR-like model, Gamma categories).  Every call returns its result
to the host, so each timing ends device-synchronised; two warm-up calls first.  Prints one JSON line per shape.

usage: hessian_timing.py [cfg2 cfg3 cfg4 cfg5]  [--reps K]"""
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
from physher_amd.engine import RESCALE_AUTO, Engine, EngineError  # noqa: E402

SHAPES = {"cfg2": (500, 100_000, 4, 4), "cfg3": (200, 50_000, 20, 4), "cfg4": (100, 20_000, 61, 1), "cfg5": (1000, 1_000_000, 4, 4)}


def engine(T, P, S, C, seed=7):
    rng = np.random.default_rng(seed)
    tree = synth.random_tree(T, rng)
    e = Engine(T, P, S, C, device=0, rescale=RESCALE_AUTO)
    e.set_topology(tree.left, tree.right, tree.root)
    e.set_branch_lengths(tree.length)
    freqs = rng.dirichlet(np.full(S, 5.0))
    r = rng.uniform(0.5, 3.0, size=(S, S))
    e.set_eigen(*reversible_eigen(0.5 * (r + r.T), freqs))
    e.set_frequencies(freqs)
    rates = np.sort(rng.gamma(0.5, 2.0, size=C)) + 0.05
    props = np.full(C, 1.0 / C)
    e.set_category_rates(rates / (rates * props).sum(), props)
    e.set_pattern_weights(np.ones(P))
    block = 100_000
    states = np.empty((T, P), dtype=np.uint8)
    for b0 in range(0, P, block):
        states[:, b0:b0 + block] = synth.evolve(tree, min(block, P - b0), S, rng)
    for t in range(T):
        e.set_tip_states(t, states[t])
    return e, tree


def timed(fn, reps):
    fn()
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return 1e3 * (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("configs", nargs="*", default=["cfg2", "cfg3", "cfg4", "cfg5"])
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    for cfg in args.configs:
        T, P, S, C = SHAPES[cfg]
        e, tree = engine(T, P, S, C)
        out = {"config": cfg, "taxa": T, "patterns": P, "states": S, "categories": C}
        with e:
            out["branch_gradient_ms"] = timed(lambda: e.branch_gradient(), args.reps)
            try:
                out["hessian_ms"] = timed(lambda: e.branch_hessian_diagonal(), args.reps)
            except EngineError as err:
                out["hessian"] = str(err)
            out["rescaling"] = bool(e.rescaling)
            if S == 4:
                branches = [n for n in range(e.N) if n != tree.root]
                sweep = branches if cfg != "cfg5" else branches[:100]
                e.branch_log_likelihood(sweep[0], tree.length[sweep[0]])
                t0 = time.perf_counter()
                for n in sweep:
                    e.branch_log_likelihood(n, tree.length[n])
                ms = 1e3 * (time.perf_counter() - t0)
                out["branch_loop_ms"] = ms * len(branches) / len(sweep)
                out["branch_loop_measured_branches"] = len(sweep)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
