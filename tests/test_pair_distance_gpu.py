"""GPU: phyamd_pairwise_distances -- the maximum-likelihood distance of every pair of taxa under the engine's own model, before any
topology exists -- pair by pair against the NumPy restatement of the rule on the mask-pair tables (tests/pair_distance_util.py, which
tests/test_pair_distance_util.py pins against the CPU oracle's two-tip tree).

At the returned t*: lnl within 1e-10 relative, d1 and d2 within 1e-9 * max(1, |ref|) of the restatement (the bounds of the
NNI-optimise test).  On the pairs that qualify (their t* moves by less than tolerance / 10 under relative errors of 1e-9 on d1 and
d2: at least nine in ten, and every pair in the CPU prototype), |t* - t_ref| <= tolerance and the iteration counts differ by at most
one.  An interior converged pair has d2 < 0 and |d1| <= 2 |d2| tolerance.  The tables are bit-equal to np.add.at under whole-number
weights.  Then the invariants of the contract and every refusal."""
import functools

import numpy as np
import pytest

import nni_optimize_util as nu
import pair_distance_util as u
from gpu_util import engine_from_problem, random_problem
from physher_amd.engine import RESCALE_ALWAYS, RESCALE_AUTO, RESCALE_NEVER, Engine, EngineError, _ptr
from test_batch_gpu import _bits

pytestmark = pytest.mark.gpu
EINVAL, EUNSUPPORTED = -1, -4
TOL, LOWER, UPPER = nu.TOLERANCE, nu.LOWER, nu.UPPER
SEGMENT = 4096


def _case_b():
    """10 % of the cells replaced by random ambiguity masks 1..15, set through set_tip_partials"""
    pb = random_problem(9, 130, 4, 2, gaps=0.05)
    masks = u.masks_from_states(pb.tip_states)
    rng = np.random.default_rng(3)
    pick = rng.random(masks.shape) < 0.1
    masks = np.where(pick, rng.integers(1, 16, size=masks.shape), masks).astype(np.uint8)
    assert set(masks.ravel().tolist()) == set(range(1, 16))  # every row and column of the table
    pb.tip_partials = u.partials_from_masks(masks)
    return pb


CASES = {
    "A_t6_p50": lambda: random_problem(6, 50, 4, 1, gaps=0.1),                           # one partial block
    "B_t9_p130_masks": _case_b,                                                          # two blocks plus 2 patterns, every mask
    "C_t7_p70_c1": lambda: random_problem(7, 70, 1, 3),                                  # one category
    "D_t8_p100_saturated": lambda: random_problem(8, 100, 2, 4, gaps=0.1, bl=(0.5, 3.0)),
    "E_t8_p40_identical": lambda: random_problem(8, 40, 4, 5, bl=(1e-4, 1e-3)),
    "F_t4_two_segments": lambda: random_problem(4, SEGMENT + 70, 4, 6, gaps=0.05),       # the sum over segments
    "G_t6_p50_c12": lambda: random_problem(6, 50, 12, 1, gaps=0.1),                      # twelve categories
}


@functools.lru_cache(maxsize=None)
def _solved(case):
    """the case's problem and the restatement's answer for every pair: computed once, shared, never changed"""
    pb = CASES[case]()
    return pb, u.solve_case(pb)


def _tip_mode(pb):
    return "partials" if pb.tip_partials is not None else "states"


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


def _check_against_the_restatement(case, pb, solved, out):
    dist, lnl, d1, d2, it, _ = out
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


@pytest.mark.parametrize("case", sorted(CASES))
def test_every_pair_matches_the_restatement(case):
    pb, solved = _solved(case)
    pairs = u.all_pairs(pb.T)
    with engine_from_problem(pb, rescale=RESCALE_AUTO, tip_mode=_tip_mode(pb)) as e:
        out = e.pairwise_distances(lower=LOWER, upper=UPPER, tolerance=TOL, max_iterations=nu.MAX_ITERATIONS, want_counts=True)
        prof = e.distance_profile()
        assert not e.rescaling
    dist, lnl, d1, d2, it, counts = out
    for a in (dist, lnl, d1, d2):
        assert a.shape == (len(pairs),)
    assert it.shape == (len(pairs),) and it.dtype == np.int32 and counts.shape == (len(pairs), 16, 16)
    assert prof["pairs"] == len(pairs) and prof["chunks"] == 1 and prof["scratch_bytes"] > 0
    assert prof["segments"] == (pb.P + SEGMENT - 1) // SEGMENT
    assert prof["iterations"] == int(np.abs(it).sum())
    # whole-number weights: every partial sum is exact, whatever the order
    assert np.array_equal(counts, u.tables(u.problem_masks(pb), pb.weights, pairs)), case
    _check_against_the_restatement(case, pb, solved, out)
    at_upper = [p for p in range(len(pairs)) if UPPER - dist[p] <= TOL]
    at_lower = [p for p in range(len(pairs)) if dist[p] - LOWER <= 2 * TOL]
    if case.startswith("D"):  # saturated pairs end at upper: a result
        assert len(at_upper) >= 1 and all(d1[p] > 0 and it[p] > 0 for p in at_upper), (at_upper, d1[at_upper])
    elif case.startswith("E"):  # identical rows end at lower: a result
        assert len(at_lower) == len(pairs) and all(d1[p] < 0 and it[p] > 0 for p in at_lower), (at_lower, d1[at_lower])
    else:
        assert not at_upper and not at_lower


def test_a_rescaling_engine_is_not_refused():
    pb, solved = _solved("A_t6_p50")
    with engine_from_problem(pb, rescale=RESCALE_ALWAYS) as e:
        assert e.rescaling
        out = e.pairwise_distances(want_counts=True)
        assert e.rescaling
    _check_against_the_restatement("A rescaling", pb, solved, out)


def test_counts_with_fractional_weights_and_counts_only_without_a_model():
    pb, _ = _solved("B_t9_p130_masks")
    pairs = u.all_pairs(pb.T)
    masks = u.problem_masks(pb)
    with _engine_without_a_tree(pb, model=False, rescale=RESCALE_NEVER) as e:
        _, _, _, _, _, counts = e.pairwise_distances(counts_only=True, lower=5.0, upper=1.0, tolerance=-1.0, max_iterations=0)  # (the bounds are ignored)
        assert np.array_equal(counts, u.tables(masks, pb.weights, pairs))
        assert e.distance_profile()["iterations"] == 0
        with pytest.raises(EngineError) as err:  # distances need the model
            e.pairwise_distances()
        assert err.value.code == EINVAL and "eigen" in str(err.value), err.value
        w = pb.weights * 0.37
        e.set_pattern_weights(w)
        _, _, _, _, _, counts = e.pairwise_distances(counts_only=True)
        assert np.all(np.abs(counts - u.tables(masks, w, pairs)) <= 1e-13 * w.sum())
        assert np.all(np.abs(counts.sum(axis=(1, 2)) - w.sum()) <= 1e-13 * w.sum())


def test_the_segments_add_up_with_fractional_weights():
    pb, _ = _solved("F_t4_two_segments")
    pairs = u.all_pairs(pb.T)
    w = pb.weights * 0.37
    with _engine_without_a_tree(pb, model=False, rescale=RESCALE_NEVER) as e:
        e.set_pattern_weights(w)
        _, _, _, _, _, counts = e.pairwise_distances(counts_only=True)
        assert e.distance_profile()["segments"] == 2
    assert np.all(np.abs(counts - u.tables(u.problem_masks(pb), w, pairs)) <= 1e-13 * w.sum())


def _same(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a[:4], b[:4])) and np.array_equal(a[4], b[4])


def test_no_topology_is_needed_and_a_pair_does_not_depend_on_the_list():
    pb, solved = _solved("B_t9_p130_masks")
    pairs = u.all_pairs(pb.T)
    with engine_from_problem(pb, rescale=RESCALE_NEVER, tip_mode="partials") as e:
        want = e.pairwise_distances(want_counts=True)
    with _engine_without_a_tree(pb, rescale=RESCALE_NEVER) as e:
        got = e.pairwise_distances(want_counts=True)
        assert _same(want, got) and np.array_equal(want[5], got[5])
        assert _same(want, e.pairwise_distances())  # two calls
        # the optional outputs do not change the others' bits
        bare = e.pairwise_distances(want_derivatives=False, want_iterations=False)
        assert bare[2] is None and bare[3] is None and bare[4] is None and bare[5] is None
        assert np.array_equal(_bits(bare[0]), _bits(want[0])) and np.array_equal(_bits(bare[1]), _bits(want[1]))
        # an explicit list in shuffled order, a pair twice, runs of one and of many pairs that share their first taxon
        order = np.random.default_rng(11).permutation(len(pairs))
        order = np.concatenate([order, order[:3]])
        got = e.pairwise_distances(pairs[order], want_counts=True)
        assert all(np.array_equal(_bits(x), _bits(y[order])) for x, y in zip(got[:4], want[:4]))
        assert np.array_equal(got[4], want[4][order]) and np.array_equal(got[5], want[5][order])
        one = e.pairwise_distances(pairs[[17]])
        assert all(_bits(x)[0] == _bits(y)[17] for x, y in zip(one[:4], want[:4]))
        # (j, i): pi on the other side; the model is reversible, so the same function up to rounding
        back = e.pairwise_distances(pairs[:, ::-1], want_counts=True)
        assert np.array_equal(back[5], want[5].transpose(0, 2, 1))
        assert np.all(np.abs(back[0] - want[0]) <= TOL), np.abs(back[0] - want[0]).max()
        assert np.all(np.abs(back[1] - want[1]) <= 1e-10 * np.abs(want[1]))
        # the caller's start: the restatement from the same start
        start = np.random.default_rng(5).uniform(0.01, 2.0, size=len(pairs))
        other = u.solve_case(pb, start=start)
        moved = e.pairwise_distances(start=start)
        for p, (t_ref, n_ref, good, _) in enumerate(other):
            if good:
                assert abs(moved[0][p] - t_ref) <= TOL and abs(int(moved[4][p]) - n_ref) <= 1, (p, moved[0][p], t_ref)
            if good and solved[p][2]:
                assert abs(moved[0][p] - solved[p][0]) <= 2 * TOL, p


def test_the_engine_is_untouched():
    pb, _ = _solved("D_t8_p100_saturated")
    with engine_from_problem(pb, rescale=RESCALE_AUTO) as e, engine_from_problem(pb, rescale=RESCALE_AUTO) as fresh:
        before = (e.log_likelihood(), e.gradient())
        first = e.pairwise_distances()
        e.nni_optimize()  # (the same scratch group)
        assert _same(first, e.pairwise_distances())
        after = (e.log_likelihood(), e.gradient())
        assert _bits(before[0]) == _bits(after[0])
        assert _bits(before[1][0]) == _bits(after[1][0]) and np.array_equal(_bits(before[1][1]), _bits(after[1][1]))
        node = 5 if pb.root != 5 else 6
        for eng in (e, fresh):
            eng.set_branch_length(node, 0.37)
        a, b = e.gradient(), fresh.gradient()
        assert _bits(a[0]) == _bits(b[0]) and np.array_equal(_bits(a[1]), _bits(b[1]))


def test_chunks_under_a_memory_cap_change_no_bit():
    pb, _ = _solved("B_t9_p130_masks")
    npairs = pb.T * (pb.T - 1) // 2
    per_pair = 8 + 8 + 2048 + 2048 + 8 + 32 + 4  # the two taxa, the group record, one segment, the table, the start, the results
    with engine_from_problem(pb, rescale=RESCALE_NEVER, tip_mode="partials") as e:
        e.log_likelihood()
        held = e.profile()["device_bytes"]
        want = e.pairwise_distances(want_counts=True)
        prof = e.distance_profile()
        assert prof["chunks"] == 1 and prof["scratch_bytes"] == npairs * per_pair and e.profile()["device_bytes"] >= held + prof["scratch_bytes"]
    ran = None
    for extra in range(0, 40 * npairs * per_pair, 4 * per_pair):  # room for four more pairs at a time: the first cap the call runs under
        cap = held + extra
        try:
            with engine_from_problem(pb, rescale=RESCALE_NEVER, tip_mode="partials", max_device_bytes=cap) as e:
                e.log_likelihood()
                if e.profile()["tiles"] != 1:
                    continue
                try:
                    got = e.pairwise_distances(want_counts=True)
                except EngineError as err:
                    assert err.code == EUNSUPPORTED and "scratch" in str(err) and "phyamd_pairwise_distances" in str(err), err
                    continue
                ran = e.distance_profile()
                print(f"cap = held + {extra}: {ran['chunks']} chunks; device_bytes {e.profile()['device_bytes']}")
                assert e.profile()["device_bytes"] <= cap
                assert _same(want, got) and np.array_equal(want[5], got[5])
                assert _same(want, e.pairwise_distances()) and e.profile()["device_bytes"] <= cap
                break
        except EngineError as err:  # (a cap that does not hold the engine itself)
            assert err.code != EUNSUPPORTED, err
            continue
    assert ran is not None and ran["chunks"] >= 2 and ran["pairs"] == npairs, ran


def test_one_iteration_returns_the_first_proposal():
    pb, solved = _solved("A_t6_p50")
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        dist, lnl, d1, d2, it, _ = e.pairwise_distances(max_iterations=1)
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


def _refused(e, code=EUNSUPPORTED, **kw):
    with pytest.raises(EngineError) as err:
        e.pairwise_distances(**kw)
    assert err.value.code == code, err.value
    assert "phyamd_pairwise_distances" in str(err.value), err.value
    print(err.value)
    return str(err.value)


def _still_usable(e, pb):
    ref = pb.log_likelihood()["lnl"]
    assert abs(e.log_likelihood() - ref) <= 1e-10 * abs(ref)


def test_twenty_states_are_refused():
    pb = random_problem(10, 200, 2, seed=20, S=20, gaps=0.03)
    with engine_from_problem(pb, rescale=RESCALE_AUTO) as e:
        assert "4 states" in _refused(e)
        assert "4 states" in _refused(e, counts_only=True)
        _still_usable(e, pb)


def test_a_tiled_engine_is_refused():
    pb = random_problem(40, 2000, 4, seed=13, gaps=0.03)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        e.gradient()
        base = e.profile()["device_bytes"]
    cap = None
    for frac in np.arange(0.9, 0.1, -0.05):  # (the search of tests/test_tree_batch_gpu.py for a cap that tiles)
        try:
            with engine_from_problem(pb, rescale=RESCALE_NEVER, max_device_bytes=int(frac * base)) as e:
                if e.profile()["tiles"] >= 2:
                    cap = int(frac * base)
                    break
        except EngineError:
            pass
    assert cap is not None, "no cap puts this problem into tiles"
    with engine_from_problem(pb, rescale=RESCALE_NEVER, max_device_bytes=cap) as e:
        assert e.profile()["tiles"] > 1
        assert "tiled" in _refused(e)
        _still_usable(e, pb)


def test_a_sharded_handle_is_refused():
    pb = random_problem(8, 200, 2, seed=3)
    with engine_from_problem(pb, rescale=RESCALE_NEVER, devices=[0, 0]) as e:
        assert e.shard_count == 2
        assert "shard" in _refused(e)
        _still_usable(e, pb)


def test_an_empty_mask_and_flags_are_refused():
    pb = random_problem(8, 100, 2, seed=3)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        assert "flags" in _refused(e, flags=1)
        e.pairwise_distances()
        part = u.partials_from_masks(u.masks_from_states(pb.tip_states[2]))
        part[7] = 0.0
        e.set_tip_partials(2, part)
        assert "empty" in _refused(e)
        assert "empty" in _refused(e, counts_only=True)


def test_invalid_arguments():
    pb = random_problem(8, 100, 2, seed=3)
    npairs = pb.T * (pb.T - 1) // 2
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        want = e.pairwise_distances()
        for bad in ([[2, 2]], [[0, 1], [5, 5]]):
            assert "different" in _refused(e, code=EINVAL, pairs=np.array(bad))
        for bad in ([[0, 8]], [[-1, 3]], [[0, 1], [9, 2]]):
            assert "outside" in _refused(e, code=EINVAL, pairs=np.array(bad))
        out = np.empty(npairs + 1)
        for count in (npairs - 1, npairs + 1, 0):  # a count that does not match null pairs
            rc = e._lib.phyamd_pairwise_distances(e._h, 0, count, None, None, LOWER, UPPER, TOL, 100, _ptr(out), None, None, None, None, None)
            assert rc == EINVAL
            with pytest.raises(EngineError) as err:
                e._check(rc)
            assert "count" in str(err.value) and "phyamd_pairwise_distances" in str(err.value), err.value
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
        e.pairwise_distances(lower=0.0, max_iterations=1000)  # the ends of what is allowed
        assert _same(want, e.pairwise_distances(start=np.full(npairs, 0.1)))
    with Engine(pb.T, pb.P, pb.S, pb.C, rescale=RESCALE_NEVER) as e:  # a tip that was never set
        e.set_pattern_weights(pb.weights)
        for t in range(pb.T - 1):
            e.set_tip_states(t, pb.tip_states[t])
        assert f"tip {pb.T - 1}" in _refused(e, code=EINVAL, counts_only=True)
