"""CPU-only: the NumPy restatement of phyamd_pairwise_distances (tests/pair_distance_util.py) against the CPU oracle's two-tip tree,
and physher_amd.distances' count-based distances against a direct restatement of the reference's loops (distancematrix.c)."""
import numpy as np

import nni_optimize_util as nu
import pair_distance_util as u
from gpu_util import random_problem
from physher_amd import distances


def _case_a():
    return random_problem(6, 50, 4, 1, gaps=0.1)


def test_f_matches_the_oracle_on_every_pair_of_case_a():
    pb = _case_a()
    pairs = u.all_pairs(pb.T)
    solved = u.solve_case(pb)
    worst = np.zeros(2)
    for (i, j), (t, n, good, f) in zip(pairs, solved):
        assert good and n > 0, (i, j, t, n)
        for at in (t, 0.05, 1.3):
            lnl, d1, _ = f(at)
            rl, r1 = u.oracle_evaluate(pb, i, j, at)
            err = np.array([abs(lnl - rl) / abs(rl), abs(d1 - r1) / max(1.0, abs(r1))])
            worst = np.maximum(worst, err)
            assert err[0] <= 1e-12 and err[1] <= 1e-9, (i, j, at, lnl, rl, d1, r1)
    print(f"worst lnL {worst[0]:.3e} d1 {worst[1]:.3e}")


def test_d2_is_the_derivative_of_d1_and_the_optimum_is_interior():
    pb = _case_a()
    for (t, n, good, f) in u.solve_case(pb):
        h = 1e-5
        d2 = f(t)[2]
        fd = (f(t + h)[1] - f(t - h)[1]) / (2 * h)
        assert abs(d2 - fd) <= 1e-6 * max(1.0, abs(d2)), (t, d2, fd)
        assert nu.LOWER + 2 * nu.TOLERANCE < t < nu.UPPER - 2 * nu.TOLERANCE
        assert d2 < 0 and abs(f(t)[1]) <= 2 * abs(d2) * nu.TOLERANCE


def test_the_table_is_a_sufficient_statistic():
    """f from the table equals the sum over the patterns one by one"""
    pb = _case_a()
    masks, G = u.problem_masks(pb), u.coefficients(pb)
    i, j, t = 1, 4, 0.23
    f = u.PairEvaluator(pb, u.table(masks[i], masks[j], pb.weights), G)
    x = np.outer(pb.cat_rates, pb.eval)
    L = np.einsum("ka,ca,c->k", G[masks[i], masks[j]], np.exp(x * t), pb.cat_props)
    assert abs(f(t)[0] - np.sum(pb.weights * np.log(L))) <= 1e-12 * abs(f(t)[0])
    assert u.table(masks[i], masks[j], pb.weights).sum() == pb.weights.sum()


def _reference_counts(si, sj, w):
    """the loops of _distance_raw_patterns / _distance_k2p_patterns: (differences, transitions, compared) over state codes"""
    d = ts = n = 0.0
    for a, b, wk in zip(si, sj, w):
        if a < 4 and b < 4:
            d += wk if a != b else 0.0
            ts += wk if {int(a), int(b)} in ({0, 2}, {1, 3}) else 0.0
            n += wk
    return d, ts, n


def _synthetic_states():
    rng = np.random.default_rng(7)
    P = 60
    s = rng.integers(0, 4, size=(5, P)).astype(np.uint8)
    s[1] = s[0]
    s[1, :6] = (s[0, :6] + 1) % 4                          # close to taxon 0
    s[2] = (s[0] + rng.integers(1, 4, size=P)) % 4          # differs from taxon 0 everywhere: p = 1 >= 0.75
    s[3, ::2] = 17                                          # gaps in the even columns ...
    s[4, 1::2] = 17                                         # ... and in the odd ones: taxa 3 and 4 share no single-state cell
    s[0, 5] = 17
    w = rng.integers(1, 5, size=P).astype(np.float64)
    return s, w


def test_p_distance_and_jc69_follow_the_references_loops():
    s, w = _synthetic_states()
    masks = u.masks_from_states(s)
    pairs = u.all_pairs(5)
    counts = u.tables(masks, w, pairs)
    p, jc = distances.p_distance(counts), distances.jc69(counts)
    seen = set()
    for k, (i, j) in enumerate(pairs):
        d, _, n = _reference_counts(s[i], s[j], w)
        want_p = 1000.0 if n == 0 else d / n
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.float64(d) / np.float64(n)
            want_jc = 1000.0 if q >= 0.75 else -0.75 * np.log(1.0 - (4.0 / 3.0) * q)
        assert p[k] == want_p, (i, j, p[k], want_p)
        assert (np.isnan(jc[k]) and np.isnan(want_jc)) or abs(jc[k] - want_jc) <= 1e-15 * abs(want_jc), (i, j, jc[k], want_jc)
        seen.add("empty" if n == 0 else "saturated" if d / n >= 0.75 else "plain")
    assert seen == {"empty", "saturated", "plain"}
    k = [tuple(x) for x in pairs].index((3, 4))
    assert p[k] == 1000.0 and np.isnan(jc[k])               # nothing compared: 1000 and the reference's 0 / 0
    k = [tuple(x) for x in pairs].index((0, 2))
    assert p[k] == 1.0 and jc[k] == 1000.0


def test_k2p_with_equal_rates_is_jc69_and_counts_transitions():
    n4 = np.full((4, 4), 2.0)                               # every change equally often: transitions are a third of the changes
    np.fill_diagonal(n4, 30.0)
    counts = np.zeros((16, 16))
    counts[np.ix_(distances.SINGLE, distances.SINGLE)] = n4
    counts[15, 15] = 11.0                                   # cells that are not single states do not count
    counts[3, 1] = 5.0
    assert abs(distances.k2p(counts) - distances.jc69(counts)) <= 1e-15
    assert abs(distances.p_distance(counts) - 24.0 / 144.0) <= 1e-16
    s, w = _synthetic_states()
    i, j = 0, 1
    d, ts, n = _reference_counts(s[i], s[j], w)
    P, Q = ts / n, (d - ts) / n
    want = -0.5 * np.log(1 - 2 * P - Q) - 0.25 * np.log(1 - 2 * Q)
    got = distances.k2p(u.table(u.masks_from_states(s)[i], u.masks_from_states(s)[j], w))
    assert abs(got - want) <= 1e-15


def test_square_is_symmetric_with_a_zero_diagonal():
    T = 5
    pairs = u.all_pairs(T)
    v = np.arange(1.0, len(pairs) + 1)
    m = distances.square(v, T)
    assert np.array_equal(m, m.T) and np.all(np.diag(m) == 0)
    for k, (i, j) in enumerate(pairs):
        assert m[i, j] == v[k]
