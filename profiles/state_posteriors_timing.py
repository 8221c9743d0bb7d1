#!/usr/bin/env python3
"""Wall time of the marginal state posteriors and reconstructed states of EVERY node by phyamd_state_posteriors (nodes=None) next
to the only way to get the same numbers without it: phyamd_get_partials for the lower and the upper partial of every node of a
keep-partials engine that has run a gradient, and the contraction in NumPy, in the same process on the same data (synthetic,
GTR-like model, Gamma categories):

  call        Engine.state_posteriors(): posteriors [N, P, 4] and states [N, P], one call
  partials    Engine.partials(n) and Engine.partials(n, upper=True) for every node, Engine.node_matrices(n), then
              J = sum_c w_c p o ((pi o u) P), posterior = J / sum_j J, state = argmax

Shapes: 69 taxa x 238 patterns x 4 categories and 200 taxa x 5000 patterns x 4 categories.  The evaluation itself (the
keep-partials gradient) is outside both timings: it has run before, and neither form changes an input.  Both forms return their
results to the host, so each timing ends device-synchronised.  Two warm-up rounds of each form, then `reps` repetitions (at least
10), the forms alternating.  The two forms are compared before anything is timed: posteriors to 1e-12, states wherever the top-two
gap is at least 1e-9.  Prints one JSON line and writes it to `--out` (committed as profiles/state_posteriors_timing.json only
when it was run on an MI355X).

usage: state_posteriors_timing.py [--reps K] [--out FILE]"""
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

SHAPES = ((69, 238, 4), (200, 5000, 4))


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
    return e, tree, freqs, props


def stats(x):
    x = np.asarray(x)
    return {"min_ms": float(x.min()), "median_ms": float(np.median(x)), "p10_ms": float(np.percentile(x, 10)), "p90_ms": float(np.percentile(x, 90))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "state_posteriors_timing.json"))
    args = ap.parse_args()
    reps = max(args.reps, 10)
    rows = []
    for T, P, C in SHAPES:
        e, tree, freqs, props = engine(T, P, C)
        N, root = tree.node_count, tree.root
        with e:
            e.set_keep_partials(True)
            e.gradient()

            def call():
                return e.state_posteriors()

            def partials():
                post = np.empty((N, P, 4))
                for n in range(N):
                    p = e.partials(n)  # [C][P][4]
                    if n == root:
                        J = np.einsum("c,ckj,j->kj", props, p, freqs)
                    else:
                        J = np.einsum("c,ckj,cki,i,cij->kj", props, p, e.partials(n, upper=True), freqs, e.node_matrices(n), optimize=True)
                    post[n] = J / J.sum(axis=1, keepdims=True)
                return post, post.argmax(axis=2).astype(np.uint8)

            for _ in range(2):
                got = call()
                ref = partials()
            err = float(np.abs(got[0] - ref[0]).max())
            assert err <= 1e-12, err
            top = np.sort(ref[0], axis=2)
            sure = top[:, :, -1] - top[:, :, -2] >= 1e-9
            assert np.array_equal(got[1][sure], ref[1][sure])
            tc, tp = [], []
            for _ in range(reps):
                t0 = time.perf_counter()
                call()
                t1 = time.perf_counter()
                partials()
                t2 = time.perf_counter()
                tc.append(1e3 * (t1 - t0))
                tp.append(1e3 * (t2 - t1))
            rows.append({"taxa": T, "patterns": P, "categories": C, "nodes": N, "call": stats(tc), "partials": stats(tp),
                         "partials_over_call": float(np.median(tp) / np.median(tc)), "max_abs_posterior_difference": err,
                         "cells_compared_for_states": int(sure.sum()), "cells": int(sure.size), "device_bytes": e.profile()["device_bytes"]})
    line = json.dumps({"shapes": rows})
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
