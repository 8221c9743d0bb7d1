#!/usr/bin/env python3
"""Wall time of the ML distance of every pair of taxa of a 20-state engine by phyamd_pairwise_distances_general next to the way a
caller got the same numbers before it: the NumPy restatement of tests/pair_distance_general_util.py on the host -- per pair the
class-pair table by np.add.at over the patterns, then the same rule on the table -- in the same process on the same data (synthetic,
a reversible 20-state model, Gamma categories, 3 % gaps):

  device        pairwise_distances_general(): the tables on the matrix pipe, every pair's iteration in one launch
  counts_only   pairwise_distances_general(counts_only=True): the tables alone, returned to the host
  host          per pair table() + optimise(); on `host_pairs` pairs drawn at random when there are more, scaled to all pairs

Shapes: 200 taxa x 512 patterns x 4 categories and (unless --skip-large) 200 x 50000 x 4, the benchmark's 20-state shape; bounds
[1e-8, 10], tolerance 1e-8, at most 100 iterations, start 0.1.  Each timing ends with its results on the host.  Before anything is
timed the two forms are compared on the host's pairs: lnL 1e-10 relative, d1 and d2 1e-9 * max(1, |ref|) at the device's t*, the
lengths within the tolerance on at least nine pairs in ten.  Two warm-up calls, then `reps` repetitions.  The counting kernel issues,
per run of up to `partners` pairs that share their first taxon, 16 v_mfma_f64_16x16x4_f64 per partner and round of 16 patterns
(`mfma_instructions`).  That count over the counts-only call's time is `mfma_per_s_counts_only_call`; the call ends with the tables on
the host (`counts_bytes`, into a fresh array), so the count over the whole distance call's time, which downloads 36 bytes a pair, is
given as well (`mfma_per_s_whole_call`: a lower bound on the kernel's rate, the iterations are in it).  Prints one JSON line and
writes it to profiles/pair_distance_general_timing.json.

--partners N names the PAIRDIST_GEN_PARTNERS the loaded library was built with (it enters the instruction count and the record
only); with --device-only the host restatement is neither run nor compared: the form in which the alternatives of that constant
were timed.

usage: pair_distance_general_timing.py [--reps K] [--skip-large | --skip-small] [--host-pairs M] [--partners N] [--device-only] [--out FILE]"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from golden_util import reversible_eigen  # noqa: E402
from nni_timing import stats  # noqa: E402
from physher_amd import synth  # noqa: E402
from physher_amd.engine import RESCALE_NEVER, Engine  # noqa: E402

SHAPES = ((200, 512, 4), (200, 50_000, 4))
LOWER, UPPER, TOLERANCE, MAX_ITERATIONS = 1e-8, 10.0, 1e-8, 100
PARTNERS = 4  # PAIRDIST_GEN_PARTNERS of phyamd_pairdist_gen.inc
S = 20


def problem(T, P, C, seed=7):
    """(engine without a tree, the same inputs for the host restatement)"""
    rng = np.random.default_rng(seed)
    tree = synth.random_tree(T, rng)
    freqs = rng.dirichlet(np.full(S, 5.0))
    r = rng.uniform(0.5, 3.0, size=(S, S))
    ev, U, Ui = reversible_eigen(0.5 * (r + r.T), freqs)
    rates = np.sort(rng.gamma(0.5, 2.0, size=C)) + 0.05
    props = np.full(C, 1.0 / C)
    rates = rates / (rates * props).sum()
    states = synth.evolve(tree, P, S, rng)
    states = np.where(rng.random(states.shape) < 0.03, S, states).astype(np.uint8)
    weights = np.ones(P)
    e = Engine(T, P, S, C, device=0, rescale=RESCALE_NEVER)
    e.set_eigen(ev, U, Ui)
    e.set_frequencies(freqs)
    e.set_category_rates(rates, props)
    e.set_pattern_weights(weights)
    for t in range(T):
        e.set_tip_states(t, states[t])
    pb = types.SimpleNamespace(T=T, P=P, C=C, eval=np.asarray(ev), evec=np.asarray(U), ivec=np.asarray(Ui), freqs=freqs, cat_rates=rates, cat_props=props,
                               weights=weights, tip_states=states, tip_partials=None)
    return e, pb


def main():
    import nni_optimize_util as nu
    import pair_distance_general_util as u
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--skip-large", action="store_true")
    ap.add_argument("--skip-small", action="store_true")
    ap.add_argument("--host-pairs", type=int, default=200)
    ap.add_argument("--partners", type=int, default=PARTNERS)
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_distance_general_timing.json"))
    args = ap.parse_args()
    rows = []
    for T, P, C in SHAPES[:1] if args.skip_large else SHAPES[1:] if args.skip_small else SHAPES:
        large = P >= 50_000
        reps = 5 if large else max(args.reps, 10)
        e, pb = problem(T, P, C)
        pairs = u.all_pairs(T)
        sample = np.arange(len(pairs))
        if len(pairs) > args.host_pairs:
            sample = np.sort(np.random.default_rng(1).choice(len(pairs), size=args.host_pairs, replace=False))
        codes, members = u.codes_from_problem(pb)
        G = u.coefficients(pb, members)
        with e:

            def device():
                return e.pairwise_distances_general(lower=LOWER, upper=UPPER, tolerance=TOLERANCE, max_iterations=MAX_ITERATIONS)

            def counts_only():
                return e.pairwise_distances_general(counts_only=True)

            def host():
                out = []
                for i, j in pairs[sample]:
                    f = u.PairEvaluator(pb, u.table(codes[i], codes[j], pb.weights), G)
                    t, n = nu.optimise(f, u.START, lower=LOWER, upper=UPPER, tolerance=TOLERANCE, max_iterations=MAX_ITERATIONS)
                    out.append((t, n) + f(t))
                return np.array(out)

            for _ in range(2):
                counts_only()
                dev = device()
            prof = e.distance_profile()
            row = {"taxa": T, "patterns": P, "categories": C, "pairs": len(pairs), "partners": args.partners}
            if not args.device_only:
                ref = host()
                dist, lnl, d1, d2 = dev[:4]
                at = np.array([u.PairEvaluator(pb, u.table(codes[i], codes[j], pb.weights), G)(dist[p]) for p, (i, j) in zip(sample, pairs[sample])])
                err = [float(np.max(np.abs(lnl[sample] - at[:, 0]) / np.abs(at[:, 0]))), float(np.max(np.abs(d1[sample] - at[:, 1]) / np.maximum(1.0, np.abs(at[:, 1])))),
                       float(np.max(np.abs(d2[sample] - at[:, 2]) / np.maximum(1.0, np.abs(at[:, 2]))))]
                assert err[0] <= 1e-10 and err[1] <= 1e-9 and err[2] <= 1e-9, err
                dt = np.abs(dist[sample] - ref[:, 0])
                agree = float(np.mean(dt <= TOLERANCE))
                assert agree >= 0.9, agree
                row.update({"max_rel_lnl_difference": err[0], "max_d1_difference": err[1], "max_d2_difference": err[2], "max_length_difference": float(dt.max()),
                            "pairs_within_tolerance": agree})
            td, tc, th = [], [], []
            for k in range(reps):
                t0 = time.perf_counter()
                device()
                t1 = time.perf_counter()
                td.append(1e3 * (t1 - t0))
                counts_only()
                tc.append(1e3 * (time.perf_counter() - t1))
                if k < 3 and not args.device_only:
                    t2 = time.perf_counter()
                    host()
                    th.append(1e3 * (time.perf_counter() - t2) * len(pairs) / len(sample))
            groups = sum((T - 1 - i + args.partners - 1) // args.partners for i in range(T - 1))
            mfma = groups * ((P + 15) // 16) * 16 * args.partners
            row.update({"device": stats(td), "counts_only": stats(tc), "device_iterations": prof["iterations"], "device_chunks": prof["chunks"], "segments": prof["segments"],
                        "scratch_bytes": prof["scratch_bytes"], "mfma_instructions": mfma, "mfma_per_s_counts_only_call": float(mfma / (1e-3 * np.min(tc))),
                        "mfma_per_s_whole_call": float(mfma / (1e-3 * np.min(td))), "counts_bytes": len(pairs) * 8192})
            if th:
                row.update({"host_scaled_to_all_pairs": stats(th), "host_pairs_timed": len(sample), "host_over_device": float(np.median(th) / np.median(td))})
            rows.append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
    line = json.dumps({"shapes": rows})
    print(line, flush=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
