"""CPU-only: the NumPy restatement of phyamd_pairwise_distances_general (tests/pair_distance_general_util.py) against the CPU oracle's
two-tip tree with 20-state tip partials, and physher_amd.distances' 20-state helpers against a direct restatement of the reference's
loop (distancematrix.c, _distance_aa_kimura_patterns).

The pin's bounds are the 4-state pin's (tests/test_pair_distance_util.py): lnL within 1e-12 relative, d1 within 1e-9 max(1, |ref|);
the restatement gave 9e-15 and 2.5e-12 on these two cases when it was written."""
import numpy as np
import pytest

import nni_optimize_util as nu
import pair_distance_general_util as u
from physher_amd import distances


def _pin(pb, pairs, solved, lengths):
    worst = np.zeros(2)
    for (i, j), (t, n, good, f) in zip(pairs, solved):
        assert good and n > 0, (i, j, t, n)
        for at in lengths(t):
            lnl, d1, _ = f(at)
            rl, r1 = u.oracle_evaluate(pb, i, j, at)
            err = np.array([abs(lnl - rl) / abs(rl), abs(d1 - r1) / max(1.0, abs(r1))])
            worst = np.maximum(worst, err)
            assert err[0] <= 1e-12 and err[1] <= 1e-9, (i, j, at, lnl, rl, d1, r1)
    print(f"worst lnL {worst[0]:.3e} d1 {worst[1]:.3e}")


def test_f_matches_the_oracle_on_every_pair_of_case_a():
    pb = u.CASES["A_t6_p50_c1"]()
    _pin(pb, u.all_pairs(pb.T), u.solve_case(pb), lambda t: (t, 0.05, 1.3))


def test_f_matches_the_oracle_on_every_pair_of_case_b():
    """every class: the sets' vectors reach the oracle as tip partials"""
    pb = u.CASES["B_t9_p130_sets"]()
    _pin(pb, u.all_pairs(pb.T), u.solve_case(pb), lambda t: (t,))


def test_d2_is_the_derivative_of_d1_and_the_optimum_is_interior():
    pb = u.CASES["A_t6_p50_c1"]()
    for (t, n, good, f) in u.solve_case(pb):
        h = 1e-5
        d2 = f(t)[2]
        fd = (f(t + h)[1] - f(t - h)[1]) / (2 * h)
        assert abs(d2 - fd) <= 1e-6 * max(1.0, abs(d2)), (t, d2, fd)
        assert nu.LOWER + 2 * nu.TOLERANCE < t < nu.UPPER - 2 * nu.TOLERANCE
        assert d2 < 0 and abs(f(t)[1]) <= 2 * abs(d2) * nu.TOLERANCE


def test_the_classes_are_numbered_in_the_order_they_are_met():
    pb = u.CASES["C_t7_p70_few_sets"]()
    codes, members = u.codes_from_problem(pb)
    assert members[3] == 1 << 3 and members[u.UNKNOWN] == (1 << 20) - 1 and np.all(members[24:] == 0) and np.all(members[21:24] != 0)
    first = [np.flatnonzero(codes.ravel() == c)[0] for c in (21, 22, 23)]  # (tip by tip, pattern by pattern: the flat order)
    assert first == sorted(first)
    m = u.member_matrix(members)
    assert np.array_equal(m[codes], pb.tip_partials)
    # the table is a sufficient statistic: f from it equals the sum over the patterns one by one
    G = u.coefficients(pb, members)
    i, j, t = 1, 4, 0.23
    f = u.PairEvaluator(pb, u.table(codes[i], codes[j], pb.weights), G)
    x = np.outer(pb.cat_rates, pb.eval)
    L = np.einsum("ka,ca,c->k", G[codes[i], codes[j]], np.exp(x * t), pb.cat_props)
    assert abs(f(t)[0] - np.sum(pb.weights * np.log(L))) <= 1e-12 * abs(f(t)[0])
    assert u.table(codes[i], codes[j], pb.weights).sum() == pb.weights.sum()


def _reference_counts(si, sj, w):
    """the loop of _distance_aa_kimura_patterns: (differences, compared) over state codes"""
    d = n = 0.0
    for a, b, wk in zip(si, sj, w):
        if a < 20 and b < 20:
            d += wk if a != b else 0.0
            n += wk
    return d, n


def _synthetic_problem():
    """five taxa x sixty patterns with gaps and two ambiguity sets; taxa 3 and 4 share no cell where both are states"""
    rng = np.random.default_rng(7)
    P = 60
    s = rng.integers(0, 20, size=(5, P)).astype(np.uint8)
    s[1] = s[0]
    s[1, :6] = (s[0, :6] + 1) % 20                          # close to taxon 0
    s[2] = (s[0] + rng.integers(1, 20, size=P)) % 20        # differs from taxon 0 everywhere: p = 1
    s[3, ::2] = 33                                          # gaps in the even columns ...
    s[4, 1::2] = 33                                         # ... and in the odd ones
    s[0, 5] = 33
    w = rng.integers(1, 5, size=P).astype(np.float64)
    part = u.partials_from_states(s)
    sets = {(0, 7): [2, 5], (1, 9): [2, 5], (2, 11): [0, 1, 19], (3, 1): [4, 6]}
    for (t, k), members in sets.items():
        part[t, k] = 0.0
        part[t, k, members] = 1.0
        s[t, k] = 40                                        # (the reference's pattern array holds a code >= 20 for a set)
    return s, w, part


class _Cells:
    def __init__(self, part):
        self.tip_partials, self.tip_states, self.T, self.P = part, None, part.shape[0], part.shape[1]


def test_kimura_protein_and_p_distance_follow_the_references_loop():
    s, w, part = _synthetic_problem()
    codes, members = u.codes_from_problem(_Cells(part))
    assert set(codes.ravel().tolist()) >= {20, 21, 22, 23} and members[21] == (1 << 2) | (1 << 5)
    pairs = u.all_pairs(5)
    counts = u.tables(codes, w, pairs)
    p, km = distances.p_distance_general(counts), distances.kimura_protein(counts)
    n20 = distances.state_counts_general(counts)
    assert n20.shape == (len(pairs), 20, 20)
    seen = set()
    for k, (i, j) in enumerate(pairs):
        d, n = _reference_counts(s[i], s[j], w)
        assert n20[k].sum() == n and np.trace(n20[k]) == n - d
        want_p = 1000.0 if n == 0 else d / n
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.float64(d) / np.float64(n)
            want_km = -np.log(1.0 - q - 0.2 * q * q)
        assert p[k] == want_p, (i, j, p[k], want_p)
        assert (np.isnan(km[k]) and np.isnan(want_km)) or km[k] == want_km or abs(km[k] - want_km) <= 1e-15 * abs(want_km), (i, j, km[k], want_km)
        seen.add("empty" if n == 0 else "saturated" if d == n else "plain")
    assert seen == {"empty", "saturated", "plain"}
    k = [tuple(x) for x in pairs].index((3, 4))
    assert p[k] == 1000.0 and np.isnan(km[k])               # nothing compared: 1000 and the reference's 0 / 0
    k = [tuple(x) for x in pairs].index((0, 2))
    assert p[k] == 1.0 and np.isnan(km[k])                  # p = 1: the logarithm of -0.2, as in the reference
    k = [tuple(x) for x in pairs].index((0, 1))
    assert 0 < km[k] < 1 and km[k] > p[k]


def test_the_helpers_keep_to_their_own_tables():
    with pytest.raises(ValueError):
        distances.state_counts_general(np.zeros((3, 16, 16)))
    with pytest.raises(ValueError):
        distances.kimura_protein(np.zeros((16, 16)))
    with pytest.raises(ValueError):
        distances.p_distance(np.zeros((32, 32)))            # the 4-state helpers keep rejecting anything but 16 x 16
    with pytest.raises(ValueError):
        distances.state_counts(np.zeros((2, 32, 32)))
