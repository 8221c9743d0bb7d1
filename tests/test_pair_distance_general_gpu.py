"""GPU: phyamd_pairwise_distances_general -- the maximum-likelihood distance of every pair of taxa of a 20-state engine under its own
model, before any topology exists -- pair by pair against the NumPy restatement of the rule on the class-pair tables
(tests/pair_distance_general_util.py, which tests/test_pair_distance_general_util.py pins against the CPU oracle's two-tip tree).

The bounds are those of tests/test_pair_distance_gpu.py.  At the returned t*: lnl within 1e-10 relative, d1 and d2 within
1e-9 * max(1, |ref|) of the restatement.  On the pairs that qualify (their t* moves by less than tolerance / 10 under relative errors
of 1e-9 on d1 and d2: at least nine in ten, and every pair in the CPU prototype), |t* - t_ref| <= tolerance and the iteration counts
differ by at most one.  An interior converged pair has d2 < 0 and |d1| <= 2 |d2| tolerance.  The tables are bit-equal to np.add.at
under whole-number weights and class_members equals the restatement's.  Then the invariants of the contract and every refusal."""
import functools

import numpy as np
import pytest

import nni_optimize_util as nu
import pair_distance_general_util as u
from gpu_util import engine_from_problem, random_problem
from physher_amd.engine import RESCALE_ALWAYS, RESCALE_AUTO, RESCALE_NEVER, Engine, EngineError, _ptr
from test_batch_gpu import _bits

pytestmark = pytest.mark.gpu
EINVAL, EUNSUPPORTED = -1, -4
TOL, LOWER, UPPER = nu.TOLERANCE, nu.LOWER, nu.UPPER
SEGMENT = u.SEGMENT
NAME = "phyamd_pairwise_distances_general"


@functools.lru_cache(maxsize=None)
def _solved(case):
    """the case's problem, its class codes and members, and the restatement's answer for every pair: computed once, shared, never
    changed"""
    pb = u.CASES[case]()
    codes, members = u.codes_from_problem(pb)
    return pb, codes, members, u.solve_case(pb)


def _tip_mode(pb):
    return "partials" if pb.tip_partials is not None else "states"


def _engine(pb, **kw):
    return engine_from_problem(pb, tip_mode=_tip_mode(pb), **kw)


def _engine_without_a_tree(pb, model=True, **kw):
    """tip data and weights -- and the model -- on an engine whose set_topology and set_branch_lengths are never called"""
    e = Engine(pb.T, pb.P, pb.S, pb.C, **kw)
    if model:
        e.set_eigen(pb.eval, pb.evec, pb.ivec)
        e.set_frequencies(pb.freqs)
        e.set_category_rates(pb.cat_rates, pb.cat_props)
    e.set_pattern_weights(pb.weights)
    for t in range(pb.T):
        if pb.tip_partials is not None:
            e.set_tip_partials(t, pb.tip_partials[t])
        else:
            e.set_tip_states(t, pb.tip_states[t])
    return e


def _interior(t):
    return LOWER + 2 * TOL < t < UPPER - 2 * TOL


def _check_against_the_restatement(case, solved, out):
    dist, lnl, d1, d2, it = out[:5]
    worst, qualified = np.zeros(4), 0
    for p, (t_ref, n_ref, good, f) in enumerate(solved):
        t, n = dist[p], int(it[p])
        assert LOWER <= t <= UPPER and 0 < n <= nu.MAX_ITERATIONS, (case, p, t, n)
        rl, r1, r2 = f(t)
        err = np.array([abs(lnl[p] - rl) / abs(rl), abs(d1[p] - r1) / max(1.0, abs(r1)), abs(d2[p] - r2) / max(1.0, abs(r2)), 0.0])
        if good:
            qualified += 1
            err[3] = abs(t - t_ref)
        worst = np.maximum(worst, err)
        assert err[0] <= 1e-10, (case, p, lnl[p], rl)
        assert err[1] <= 1e-9, (case, p, d1[p], r1)
        assert err[2] <= 1e-9, (case, p, d2[p], r2)
        if good:
            assert err[3] <= TOL, (case, p, t, t_ref)
            assert abs(n - n_ref) <= 1, (case, p, n, n_ref)
        if _interior(t):
            assert r2 < 0 and abs(r1) <= 2 * abs(r2) * TOL, (case, p, t, r1, r2)
    print(f"{case}: {len(solved)} pairs ({qualified} qualified), worst lnL {worst[0]:.3e} d1 {worst[1]:.3e} d2 {worst[2]:.3e} |t* - t_ref| {worst[3]:.3e}")
    assert qualified >= 0.9 * len(solved)


@pytest.mark.parametrize("case", sorted(u.CASES))
def test_every_pair_matches_the_restatement(case):
    pb, codes, members, solved = _solved(case)
    pairs = u.all_pairs(pb.T)
    with _engine(pb, rescale=RESCALE_AUTO) as e:
        out = e.pairwise_distances_general(lower=LOWER, upper=UPPER, tolerance=TOL, max_iterations=nu.MAX_ITERATIONS, want_counts=True, want_class_members=True)
        prof = e.distance_profile()
        assert not e.rescaling
    dist, lnl, d1, d2, it, counts, got_members = out
    for a in (dist, lnl, d1, d2):
        assert a.shape == (len(pairs),)
    assert it.shape == (len(pairs),) and it.dtype == np.int32 and counts.shape == (len(pairs), 32, 32)
    assert got_members.shape == (32,) and got_members.dtype == np.uint64 and np.array_equal(got_members, members), (got_members, members)
    assert prof["pairs"] == len(pairs) and prof["chunks"] == 1 and prof["scratch_bytes"] > 0
    assert prof["segments"] == (pb.P + SEGMENT - 1) // SEGMENT
    assert prof["iterations"] == int(np.abs(it).sum())
    # whole-number weights: every partial sum is exact, whatever the order
    assert np.array_equal(counts, u.tables(codes, pb.weights, pairs)), case
    _check_against_the_restatement(case, solved, out)
    at_upper = [p for p in range(len(pairs)) if UPPER - dist[p] <= TOL]
    at_lower = [p for p in range(len(pairs)) if dist[p] - LOWER <= 2 * TOL]
    if case.startswith("B"):
        assert set(codes.ravel().tolist()) == set(range(32))
    if case.startswith("D"):  # saturated pairs end at upper: a result
        assert len(at_upper) >= 1 and all(d1[p] > 0 and it[p] > 0 for p in at_upper), (at_upper, d1[at_upper])
    elif case.startswith("E"):  # identical rows end at lower: a result
        assert len(at_lower) == len(pairs) and all(d1[p] < 0 and it[p] > 0 for p in at_lower), (at_lower, d1[at_lower])
    else:
        assert not at_upper and not at_lower


def test_a_rescaling_engine_is_not_refused():
    pb, _, _, solved = _solved("A_t6_p50_c1")
    with _engine(pb, rescale=RESCALE_ALWAYS) as e:
        assert e.rescaling
        out = e.pairwise_distances_general(want_counts=True)
        assert e.rescaling
    _check_against_the_restatement("A rescaling", solved, out)


def test_counts_with_fractional_weights_and_counts_only_without_a_model():
    pb, codes, members, _ = _solved("B_t9_p130_sets")
    pairs = u.all_pairs(pb.T)
    with _engine_without_a_tree(pb, model=False, rescale=RESCALE_NEVER) as e:
        out = e.pairwise_distances_general(counts_only=True, want_class_members=True, lower=5.0, upper=1.0, tolerance=-1.0, max_iterations=0)  # (the bounds are ignored)
        assert all(x is None for x in out[:5])
        assert np.array_equal(out[5], u.tables(codes, pb.weights, pairs)) and np.array_equal(out[6], members)
        assert e.distance_profile()["iterations"] == 0
        with pytest.raises(EngineError) as err:  # distances need the model
            e.pairwise_distances_general()
        assert err.value.code == EINVAL and "eigen" in str(err.value), err.value
        w = pb.weights * 0.37
        e.set_pattern_weights(w)
        counts = e.pairwise_distances_general(counts_only=True)[5]
        assert np.all(np.abs(counts - u.tables(codes, w, pairs)) <= 1e-13 * w.sum())
        assert np.all(np.abs(counts.sum(axis=(1, 2)) - w.sum()) <= 1e-13 * w.sum())


def test_the_segments_add_up_with_fractional_weights():
    pb, codes, _, _ = _solved("F_t4_two_segments")
    pairs = u.all_pairs(pb.T)
    w = pb.weights * 0.37
    with _engine_without_a_tree(pb, model=False, rescale=RESCALE_NEVER) as e:
        e.set_pattern_weights(w)
        counts = e.pairwise_distances_general(counts_only=True)[5]
        assert e.distance_profile()["segments"] == 2
    assert np.all(np.abs(counts - u.tables(codes, w, pairs)) <= 1e-13 * w.sum())


def _same(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a[:4], b[:4])) and np.array_equal(a[4], b[4])


def test_no_topology_is_needed_and_a_pair_does_not_depend_on_the_list():
    pb, _, _, solved = _solved("B_t9_p130_sets")
    pairs = u.all_pairs(pb.T)
    with _engine(pb, rescale=RESCALE_NEVER) as e:
        want = e.pairwise_distances_general(want_counts=True)
    with _engine_without_a_tree(pb, rescale=RESCALE_NEVER) as e:
        got = e.pairwise_distances_general(want_counts=True)
        assert _same(want, got) and np.array_equal(want[5], got[5])
        assert _same(want, e.pairwise_distances_general())  # two calls
        # the optional outputs do not change the others' bits
        bare = e.pairwise_distances_general(want_derivatives=False, want_iterations=False)
        assert all(bare[k] is None for k in (2, 3, 4, 5, 6))
        assert np.array_equal(_bits(bare[0]), _bits(want[0])) and np.array_equal(_bits(bare[1]), _bits(want[1]))
        # an explicit list in shuffled order, a pair twice, runs of one and of many pairs that share their first taxon: other
        # groupings into waves
        order = np.random.default_rng(11).permutation(len(pairs))
        order = np.concatenate([order, order[:3]])
        got = e.pairwise_distances_general(pairs[order], want_counts=True)
        assert all(np.array_equal(_bits(x), _bits(y[order])) for x, y in zip(got[:4], want[:4]))
        assert np.array_equal(got[4], want[4][order]) and np.array_equal(got[5], want[5][order])
        one = e.pairwise_distances_general(pairs[[17]])
        assert all(_bits(x)[0] == _bits(y)[17] for x, y in zip(one[:4], want[:4]))
        sub = e.pairwise_distances_general(pairs[3:12], want_counts=True)  # a run that starts inside taxon 0's partners
        assert all(np.array_equal(_bits(x), _bits(y[3:12])) for x, y in zip(sub[:4], want[:4])) and np.array_equal(sub[5], want[5][3:12])
        # (j, i): pi on the other side; the model is reversible, so the same function up to rounding
        back = e.pairwise_distances_general(pairs[:, ::-1], want_counts=True)
        assert np.array_equal(back[5], want[5].transpose(0, 2, 1))
        assert np.all(np.abs(back[0] - want[0]) <= TOL), np.abs(back[0] - want[0]).max()
        assert np.all(np.abs(back[1] - want[1]) <= 1e-10 * np.abs(want[1]))
        # the caller's start: the restatement from the same start
        start = np.random.default_rng(5).uniform(0.01, 2.0, size=len(pairs))
        other = u.solve_case(pb, start=start)
        moved = e.pairwise_distances_general(start=start)
        for p, (t_ref, n_ref, good, _) in enumerate(other):
            if good:
                assert abs(moved[0][p] - t_ref) <= TOL and abs(int(moved[4][p]) - n_ref) <= 1, (p, moved[0][p], t_ref)
            if good and solved[p][2]:
                assert abs(moved[0][p] - solved[p][0]) <= 2 * TOL, p


def test_the_engine_is_untouched():
    pb = _solved("D_t8_p100_saturated")[0]
    with _engine(pb, rescale=RESCALE_AUTO) as e, _engine(pb, rescale=RESCALE_AUTO) as fresh:
        before = (e.log_likelihood(), e.gradient())
        fresh.log_likelihood(), fresh.gradient()  # the same history without the call: an incremental update follows on both
        first = e.pairwise_distances_general()
        assert _same(first, e.pairwise_distances_general())
        after = (e.log_likelihood(), e.gradient())
        fresh.log_likelihood(), fresh.gradient()
        assert _bits(before[0]) == _bits(after[0])
        assert _bits(before[1][0]) == _bits(after[1][0]) and np.array_equal(_bits(before[1][1]), _bits(after[1][1]))
        node = 5 if pb.root != 5 else 6
        for eng in (e, fresh):
            eng.set_branch_length(node, 0.37)
        a, b = e.gradient(), fresh.gradient()
        assert _bits(a[0]) == _bits(b[0]) and np.array_equal(_bits(a[1]), _bits(b[1]))


def test_chunks_under_a_memory_cap_change_no_bit():
    pb = _solved("B_t9_p130_sets")[0]
    npairs = pb.T * (pb.T - 1) // 2
    per_pair = 8 + 8 + 8192 + 8192 + 8 + 32 + 4  # the two taxa, the group record, one segment, the table, the start, the results
    with _engine(pb, rescale=RESCALE_NEVER) as e:
        e.log_likelihood()
        held = e.profile()["device_bytes"]
        want = e.pairwise_distances_general(want_counts=True)
        prof = e.distance_profile()
        assert prof["chunks"] == 1 and prof["scratch_bytes"] == npairs * per_pair and e.profile()["device_bytes"] >= held + prof["scratch_bytes"]
    ran = None
    for extra in range(0, 40 * npairs * per_pair, 4 * per_pair):  # room for four more pairs at a time: the first cap the call runs under
        cap = held + extra
        try:
            with _engine(pb, rescale=RESCALE_NEVER, max_device_bytes=cap) as e:
                e.log_likelihood()
                if e.profile()["tiles"] != 1:
                    continue
                try:
                    got = e.pairwise_distances_general(want_counts=True)
                except EngineError as err:
                    assert err.code == EUNSUPPORTED and "scratch" in str(err) and NAME in str(err), err
                    continue
                ran = e.distance_profile()
                print(f"cap = held + {extra}: {ran['chunks']} chunks; device_bytes {e.profile()['device_bytes']}")
                assert e.profile()["device_bytes"] <= cap
                assert _same(want, got) and np.array_equal(want[5], got[5])
                assert _same(want, e.pairwise_distances_general()) and e.profile()["device_bytes"] <= cap
                break
        except EngineError as err:  # (a cap that does not hold the engine itself)
            assert err.code != EUNSUPPORTED, err
            continue
    assert ran is not None and ran["chunks"] >= 2 and ran["pairs"] == npairs, ran


def test_one_iteration_returns_the_first_proposal():
    pb, _, _, solved = _solved("A_t6_p50_c1")
    with _engine(pb, rescale=RESCALE_NEVER) as e:
        dist, lnl, d1, d2, it = e.pairwise_distances_general(max_iterations=1)[:5]
    assert np.all(it == -1)
    assert np.all(np.isfinite(dist)) and np.all(np.isfinite(lnl)) and np.all(np.isfinite(d1)) and np.all(np.isfinite(d2))
    compared = 0
    for p, x in enumerate(solved):
        f, s = x[3], u.START
        t_ref, n_ref = nu.optimise(f, s, max_iterations=1)
        assert n_ref == -1
        # the proposal is the same midpoint, or the Newton step t - d1 / d2 from the same t with d1 and d2 as far off as the suite
        # allows them (1e-9 * max(1, |ref|) each): twice the first-order change of the step, and a rounding of t itself
        _, r1, r2 = f(s)
        bound = 2e-9 * (max(1.0, abs(r1)) + abs(t_ref - s) * max(1.0, abs(r2))) / abs(r2) + 4 * np.spacing(t_ref)
        if not all(abs(nu.optimise(f, s, max_iterations=1, perturb=q)[0] - t_ref) <= bound for q in ((1e-9, -1e-9), (-1e-9, 1e-9))):
            continue  # (such errors change which of the two proposals is made)
        compared += 1
        assert abs(dist[p] - t_ref) <= bound, (p, dist[p], t_ref, bound)
    assert compared >= 0.9 * len(solved)


def test_the_profile_reports_the_last_distance_call_of_either_kind():
    pb = _solved("F_t4_two_segments")[0]
    with _engine(pb, rescale=RESCALE_NEVER) as e:
        _, _, _, _, it, _, _ = e.pairwise_distances_general(u.all_pairs(pb.T)[:4])
        prof = e.distance_profile()
        assert prof["pairs"] == 4 and prof["chunks"] == 1 and prof["segments"] == 2 and prof["iterations"] == int(np.abs(it).sum()) and prof["ms"] > 0
        assert prof["scratch_bytes"] >= 4 * (8 + 8 + 2 * 8192 + 8192 + 8 + 32 + 4)
        e.pairwise_distances_general(counts_only=True)
        prof = e.distance_profile()
        assert prof["pairs"] == 6 and prof["iterations"] == 0
    q = random_problem(5, 30, 2, seed=3)
    with engine_from_problem(q, rescale=RESCALE_NEVER) as e:  # ... and the 4-state call's, as before
        e.pairwise_distances()
        assert e.distance_profile()["pairs"] == 10 and e.distance_profile()["segments"] == 1


def _refused(e, code=EUNSUPPORTED, **kw):
    with pytest.raises(EngineError) as err:
        e.pairwise_distances_general(**kw)
    assert err.value.code == code, err.value
    assert NAME in str(err.value), err.value
    print(err.value)
    return str(err.value)


def _still_usable(e, pb):
    ref = pb.log_likelihood()["lnl"]
    assert abs(e.log_likelihood() - ref) <= 1e-10 * abs(ref)


def test_other_state_counts_are_refused():
    pb = random_problem(8, 100, 2, seed=3)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        msg = _refused(e)
        assert "20 states" in msg and "use phyamd_pairwise_distances" in msg
        assert "use phyamd_pairwise_distances" in _refused(e, counts_only=True)
        e.pairwise_distances()  # the call it points at
        _still_usable(e, pb)
    with Engine(4, 10, 61, 1, rescale=RESCALE_NEVER) as e:
        msg = _refused(e, counts_only=True)
        assert "61" in msg and "not built" in msg


def _with_sets(pb, count):
    """pb's states with `count` different two-member sets in the first cells of tip 0"""
    part = u.partials_from_states(pb.tip_states)
    for q in range(count):
        part[0, q] = 0.0
        part[0, q, [q, q + 1]] = 1.0
    return part


def test_twelve_sets_and_a_set_without_a_member_are_refused():
    pb = random_problem(6, 50, 2, seed=31, S=20)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        e.set_tip_partials(0, _with_sets(pb, 11)[0])
        out = e.pairwise_distances_general(want_class_members=True)
        assert np.all(out[6][21:] == [(1 << q) | (2 << q) for q in range(11)]) and np.all(np.isfinite(out[1]))
        e.set_tip_partials(0, _with_sets(pb, 12)[0])  # a twelfth: class 32
        msg = _refused(e)
        assert "12 ambiguity sets" in msg and "at most 11" in msg
        assert "12 ambiguity sets" in _refused(e, counts_only=True)
        e.log_likelihood()  # the engine itself takes up to 235 sets
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        part = u.partials_from_states(pb.tip_states[2])
        part[7] = 0.0
        e.set_tip_partials(2, part)
        assert "no member" in _refused(e)
        assert "no member" in _refused(e, counts_only=True)


def test_a_tiled_engine_is_refused():
    pb = random_problem(12, 1500, 2, seed=4032, S=20, gaps=0.04)  # (a case of test_pattern_tiling_under_a_memory_cap)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        e.gradient()
        cap = int(0.45 * e.profile()["device_bytes"])
    with engine_from_problem(pb, rescale=RESCALE_NEVER, max_device_bytes=cap) as e:
        assert e.profile()["tiles"] > 1
        assert "tiled" in _refused(e)
        _still_usable(e, pb)


def test_a_sharded_handle_is_refused():
    pb = random_problem(8, 200, 2, seed=3, S=20)
    with engine_from_problem(pb, rescale=RESCALE_NEVER, devices=[0, 0]) as e:
        assert e.shard_count == 2
        assert "shard" in _refused(e)
        _still_usable(e, pb)


def test_invalid_arguments_and_flags():
    pb = random_problem(8, 100, 2, seed=3, S=20)
    npairs = pb.T * (pb.T - 1) // 2
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        assert "flags" in _refused(e, flags=1)
        want = e.pairwise_distances_general()
        for bad in ([[2, 2]], [[0, 1], [5, 5]]):
            assert "different" in _refused(e, code=EINVAL, pairs=np.array(bad))
        for bad in ([[0, 8]], [[-1, 3]], [[0, 1], [9, 2]]):
            assert "outside" in _refused(e, code=EINVAL, pairs=np.array(bad))
        out = np.empty(npairs + 1)
        fn = getattr(e._lib, NAME)
        for count in (npairs - 1, npairs + 1, 0):  # a count that does not match null pairs
            rc = fn(e._h, 0, count, None, None, LOWER, UPPER, TOL, 100, _ptr(out), None, None, None, None, None, None)
            assert rc == EINVAL
            with pytest.raises(EngineError) as err:
                e._check(rc)
            assert "count" in str(err.value) and NAME in str(err.value), err.value
        rc = fn(e._h, 0, npairs, None, None, LOWER, UPPER, TOL, 100, None, None, None, None, None, None, None)  # neither distances nor counts
        assert rc == EINVAL
        rc = fn(e._h, 0, npairs, None, None, LOWER, UPPER, TOL, 100, None, _ptr(out), None, None, None, _ptr(np.empty((npairs, 32, 32))), None)  # lnl without distances
        assert rc == EINVAL
        rc = fn(None, 0, npairs, None, None, LOWER, UPPER, TOL, 100, _ptr(out), None, None, None, None, None, None)  # null engine
        assert rc == EINVAL
        for kw in (dict(lower=-1e-3), dict(lower=0.5, upper=0.5), dict(lower=2.0, upper=1.0), dict(upper=np.inf), dict(lower=np.nan), dict(upper=np.nan)):
            assert "bounds" in _refused(e, code=EINVAL, **kw), kw
        for tol in (0.0, -1e-8, np.inf, np.nan):
            assert "tolerance" in _refused(e, code=EINVAL, tolerance=tol), tol
        for n in (0, -3, 1001):
            assert "max_iterations" in _refused(e, code=EINVAL, max_iterations=n), n
        for bad in (-0.01, np.nan, np.inf):
            start = np.full(npairs, 0.1)
            start[4] = bad
            msg = _refused(e, code=EINVAL, start=start)
            assert "start" in msg and "[4]" in msg, msg
        e.pairwise_distances_general(lower=0.0, max_iterations=1000)  # the ends of what is allowed
        assert _same(want, e.pairwise_distances_general(start=np.full(npairs, 0.1)))
    with Engine(pb.T, pb.P, pb.S, pb.C, rescale=RESCALE_NEVER) as e:  # a tip that was never set, then no weights, then no model
        for t in range(pb.T - 1):
            e.set_tip_states(t, pb.tip_states[t])
        e.set_pattern_weights(pb.weights)
        assert f"tip {pb.T - 1}" in _refused(e, code=EINVAL, counts_only=True)
    with Engine(pb.T, pb.P, pb.S, pb.C, rescale=RESCALE_NEVER) as e:
        for t in range(pb.T):
            e.set_tip_states(t, pb.tip_states[t])
        assert "weights" in _refused(e, code=EINVAL, counts_only=True)
        e.set_pattern_weights(pb.weights)
        e.pairwise_distances_general(counts_only=True)
        assert "eigen" in _refused(e, code=EINVAL)
        e.set_eigen(pb.eval, pb.evec, pb.ivec)
        assert "frequencies" in _refused(e, code=EINVAL)
        e.set_frequencies(pb.freqs)
        assert "rates" in _refused(e, code=EINVAL)
        e.set_category_rates(pb.cat_rates, pb.cat_props)
        e.pairwise_distances_general()
