"""GPU: phyamd_spr_optimize -- the three branches that meet at the graft point of every SPR regraft, optimised one at a time, pass
after pass, in one call -- against the CPU oracle and the NumPy restatement of the rule (tests/spr_optimize_util.py: the batch
optimiser's restatement on the rearranged tree with p, w and u marked).

Bounds are the suite's for single evaluations: lnL 1e-10 relative.  At the returned lengths lnl is the oracle's lnL of the rearranged
tree, which recomputes everything from the tips.  Lengths are compared with the restatement on the entries that are qualified (the
restatement itself moves by less than tolerance / 10 under relative errors of 1e-9 on d1 and d2: at least nine in ten, confirmed for
the restatement alone in tests/test_spr_optimize_util.py), to within tolerance.  Then the existing device routine on the same trees,
the bounds, the bits the contract promises, a memory cap, underflow in band, and every refusal."""
import functools

import numpy as np
import pytest

import branch_optimize_util as b
import nni_optimize_util as u1
import spr_optimize_util as t
import test_spr_gpu as s
from gpu_util import engine_from_problem, random_problem
from physher_amd.engine import GRAD_FOLD_ROOT_FREQS, RESCALE_ALWAYS, RESCALE_AUTO, RESCALE_NEVER, EngineError
from test_batch_gpu import _bits, _deep
from test_nni_gpu import _parents
from test_tree_batch_gpu import _relabel

pytestmark = pytest.mark.gpu
EINVAL, EUNSUPPORTED = -1, -4
TOL, LOWER, UPPER = t.TOLERANCE, t.LOWER, t.UPPER
LNL = 1e-10  # relative


def _same(x, y):
    return all((p is None and q is None) or np.array_equal(_bits(p) if p.dtype == np.float64 else p, _bits(q) if q.dtype == np.float64 else q) for p, q in zip(x, y))


def _start(pb, p, w):
    return np.array([pb.branch_lengths[p], 0.5 * pb.branch_lengths[w], 0.5 * pb.branch_lengths[w]])


@functools.lru_cache(maxsize=None)
def _solved(case):
    """the case on its own engine, once: the SPR scores, the call with its defaults and its profile, and the call with one pass"""
    pb, tip_mode = t.problem(case)
    with engine_from_problem(pb, rescale=RESCALE_AUTO, tip_mode=tip_mode) as e:
        spr = e.spr_log_likelihoods()
        full = e.spr_optimize()
        prof = e.spr_optimize_profile()
        one = e.spr_optimize(max_passes=1)
        assert not e.rescaling
    return pb, spr, full, prof, one


@pytest.mark.parametrize("case", t.CASES)
def test_every_entry(case):
    pb, spr, (lengths, lnl, lnl0, passes), prof, _ = _solved(case)
    mask, parent = s._candidate_mask(pb), _parents(pb)
    # the NaN / 0 pattern is the candidate rule
    assert lengths.shape == (pb.N, pb.N, 3) and lnl.shape == lnl0.shape == passes.shape == (pb.N, pb.N) and passes.dtype == np.int32
    assert np.array_equal(np.isfinite(lnl), mask) and np.array_equal(np.isfinite(lnl0), mask) and np.array_equal(np.all(np.isfinite(lengths), axis=2), mask)
    assert np.all(np.isnan(lnl[~mask])) and np.all(np.isnan(lnl0[~mask])) and np.all(np.isnan(lengths[~mask])) and np.all(passes[~mask] == 0)
    # every candidate: bounds, the start, monotone, stopped by the rule
    assert np.all((lengths[mask] >= LOWER) & (lengths[mask] <= UPPER))
    err0 = np.abs(lnl0[mask] - spr[mask]) / np.abs(spr[mask])
    print(f"{case}: {int(mask.sum())} candidates, passes {passes[mask].min()}..{passes[mask].max()}, worst relative |initial_lnl - spr| {err0.max():.3e}; {prof}")
    assert np.all(err0 <= LNL)
    assert np.all(lnl[mask] >= lnl0[mask] - LNL * np.abs(lnl[mask]))
    assert np.all((passes[mask] != 0) & (np.abs(passes[mask]) <= t.MAX_PASSES))  # (a few candidates of a large tree climb a narrow ridge for more than 50 passes)
    assert prof["prunes"] == pb.N and prof["candidates"] == mask.sum() and prof["chunks"] == 1 and prof["scratch_bytes"] > 0
    assert prof["visits"] == 3 * int(np.abs(passes).sum()) and prof["iterations"] >= prof["visits"]
    if case == "t3":
        assert mask.sum() == 2
    # the entries: converged, lnl is the oracle's at the returned lengths, and a further restated pass gains no more than the call stopped on
    worst, most = 0.0, -np.inf
    for p, w in t.entries(case):
        assert 0 < passes[p, w] <= t.MAX_PASSES, (p, w, passes[p, w])
        q = t.at_lengths(pb, parent, p, w, lengths[p, w])
        want = q.log_likelihood()["lnl"]
        err = abs(lnl[p, w] - want) / abs(want)
        worst = max(worst, err)
        assert err <= LNL, (p, w, lnl[p, w], want)
        ended, after = b.one_pass(q, t.mask(pb, parent, p, w))
        assert ended is None
        most = max(most, after - want)
        assert after - want <= t.LNL_TOLERANCE + LNL * abs(want), (p, w, after - want)
    print(f"{case}: {len(t.entries(case))} entries, worst relative lnL error at the result {worst:.3e}, most a further restated pass gains {most:.3e}")


@pytest.mark.parametrize("case", t.CASES)
def test_one_pass_is_the_restatements(case):
    pb, _, _, _, (lengths, lnl, lnl0, passes) = _solved(case)
    mask = s._candidate_mask(pb)
    assert np.all(np.abs(passes[mask]) == 1) and np.all(passes[~mask] == 0)
    ref = t.one_pass_thrice(case)
    good, worst = 0, 0.0
    for (p, w), (three, qualified) in ref.items():
        if not qualified:
            continue
        good += 1
        err = np.abs(lengths[p, w] - three).max()
        worst = max(worst, err)
        assert err <= TOL, (p, w, lengths[p, w], three)
    print(f"{case}: {good} of {len(ref)} entries qualify, worst |t - t_ref| {worst:.3e}")
    assert good >= 0.9 * len(ref)


@pytest.mark.parametrize("case", ["t4_caterpillar", "t8_random_p65", "t8_relabelled_p64", "t37_gaps"])  # (most regrafts are wrong ones, whose t_u ends on the lower bound: at t3 and t4_balanced all of them)
def test_the_visit_of_u_ends_at_a_stationary_point(case):
    """The state before u's visit in the first pass is the returned (t_p, t_w) and the start's t_u.  Where the restated visit from
    there converged, was accepted and ended inside the bounds, the last Newton step was at most tolerance long, so at the returned
    t_u |d1| <= 2 |d2| tolerance by the oracle's derivatives (the factor 2 leaves room for the step itself and for d2 moving along it)"""
    pb, _, _, _, (lengths, lnl, lnl0, passes) = _solved(case)
    parent = _parents(pb)
    checked, worst = 0, 0.0
    for p, w in t.entries(case)[:60]:
        u = int(parent[p])
        before = lengths[p, w].copy()
        before[2] = 0.5 * pb.branch_lengths[w]
        f = b.Edge(t.at_lengths(pb, parent, p, w, before), u)
        t0 = min(max(before[2], LOWER), UPPER)
        t1, n = u1.optimise(f, t0)
        if n < 0 or not (f(t1)[0] >= f(t0)[0]) or not (LOWER + TOL < t1 < UPPER - TOL):
            continue
        assert abs(lengths[p, w, 2] - t1) <= TOL, (p, w, lengths[p, w, 2], t1)
        _, d1, d2 = f(lengths[p, w, 2])
        checked += 1
        worst = max(worst, abs(d1) / (abs(d2) * TOL))
        assert abs(d1) <= 2 * abs(d2) * TOL, (p, w, d1, d2)
    print(f"{case}: {checked} visits of u checked, worst |d1| / (|d2| tolerance) {worst:.3e}")
    assert checked >= 1


def test_against_the_batch_optimiser_on_the_rearranged_trees():
    """the existing device routine on a second engine: the same rearranged trees, the same mask, one pass"""
    case = "t8_random_p65"
    pb, _, _, _, (lengths, lnl, lnl0, passes) = _solved(case)
    parent, pairs = _parents(pb), t.entries(case)
    trees = [s._moved(pb, parent, p, w) for p, w in pairs]
    left, right, bl = (np.ascontiguousarray([x[i] for x in trees]) for i in range(3))
    marks = np.array([t.mask(pb, parent, p, w) for p, w in pairs], dtype=np.uint8)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as other:
        ref = other.optimize_branch_lengths((left, right, np.full(len(pairs), pb.root, dtype=np.int32)), bl, marks, max_passes=1)
    restated = t.one_pass_thrice(case)
    worst_t, worst_l, good = 0.0, 0.0, 0
    for i, (p, w) in enumerate(pairs):
        three = t.nodes(parent, p, w)
        worst_l = max(worst_l, abs(lnl[p, w] - ref[1][i]) / abs(ref[1][i]))
        assert abs(lnl[p, w] - ref[1][i]) <= LNL * abs(ref[1][i]), (p, w, lnl[p, w], ref[1][i])
        assert abs(lnl0[p, w] - ref[2][i]) <= LNL * abs(ref[2][i])
        assert passes[p, w] == ref[3][i]
        if restated[(p, w)][1]:
            good += 1
            worst_t = max(worst_t, np.abs(lengths[p, w] - ref[0][i, three]).max())
            assert np.all(np.abs(lengths[p, w] - ref[0][i, three]) <= TOL), (p, w, lengths[p, w], ref[0][i, three])
    print(f"{len(pairs)} entries against optimize_branch_lengths: worst relative lnL difference {worst_l:.3e}; {good} qualified, worst |t - t'| {worst_t:.3e}")
    assert good >= 0.9 * len(pairs)


def test_the_bounds_and_one_iteration():
    """An upper bound below the tree's branch lengths, and a lower bound above them: wherever one pass of the restatement under the
    same bounds leaves a branch on the bound (where lnL still rises towards it, the bracket closes onto the bound itself), the call
    ends within tolerance of it -- most branches under the upper bound, all of them under the lower one"""
    case = "t8_random_p65"
    pb, _ = t.problem(case)
    mask, parent = s._candidate_mask(pb), _parents(pb)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        for kw, bound, share in (({"upper": 2e-3}, 2e-3, 0.5), ({"lower": 0.5}, 0.5, 1.0)):
            lengths, lnl, lnl0, passes = e.spr_optimize(max_passes=1, **kw)
            lo, hi = kw.get("lower", LOWER), kw.get("upper", UPPER)
            assert np.all((lengths[mask] >= lo) & (lengths[mask] <= hi)) and np.all(np.abs(passes[mask]) == 1)
            on, seen, off = 0, 0, 0.0
            for p, w in t.entries(case)[::4]:
                q = t.rearranged(pb, parent, p, w)
                assert b.one_pass(q, t.mask(pb, parent, p, w), **kw)[0] is None
                there = np.abs(q.branch_lengths[t.nodes(parent, p, w)] - bound) <= TOL / 10
                on, seen = on + int(there.sum()), seen + 3
                if there.any():
                    off = max(off, np.abs(lengths[p, w][there] - bound).max())
            print(f"{kw}: {on} of {seen} restated branches end on the bound; the call's are at most {off:.3e} from it")
            assert on >= share * seen and off <= TOL
        lengths, lnl, lnl0, passes = e.spr_optimize(max_iterations=1, max_passes=3)
        assert np.all(np.isfinite(lengths[mask])) and np.all(np.isfinite(lnl[mask])) and np.all((lengths[mask] >= LOWER) & (lengths[mask] <= UPPER))
        assert np.all((passes[mask] == -3) | ((passes[mask] >= 1) & (passes[mask] <= 3)))
        assert np.all(lnl[mask] >= lnl0[mask] - LNL * np.abs(lnl[mask]))
        assert e.spr_optimize_profile()["iterations"] == e.spr_optimize_profile()["visits"]
        for p, w in t.entries(case)[::7]:  # (finite outputs that are what they say)
            want = t.at_lengths(pb, parent, p, w, lengths[p, w]).log_likelihood()["lnl"]
            assert abs(lnl[p, w] - want) <= LNL * abs(want)
        lengths, lnl, lnl0, passes = e.spr_optimize(max_passes=1, lnl_tolerance=0.0)
        assert np.all(passes[mask & (lnl > lnl0)] == -1)


def test_bit_for_bit_across_calls_and_the_engine_is_untouched():
    pb = random_problem(16, 130, 2, seed=31, gaps=0.05)
    bl = pb.branch_lengths[None, :] * np.random.default_rng(4).uniform(0.5, 1.8, size=(5, pb.N))
    other = random_problem(16, 130, 2, seed=32)  # (another tree, for the tree batch)
    trees = (other.left[None, :], other.right[None, :], np.array([other.root], dtype=np.int32), other.branch_lengths[None, :])
    with engine_from_problem(pb, rescale=RESCALE_AUTO) as e, engine_from_problem(pb, rescale=RESCALE_AUTO) as fresh:
        before = (e.log_likelihood(), e.gradient())
        first = e.spr_optimize()
        assert _same(first, e.spr_optimize())
        e.gradient_batch(bl)  # (the other calls run in the same scratch, with other op lists and fewer upper slots)
        e.gradient_batch_trees(*trees)
        e.nni_optimize()
        e.spr_log_likelihoods()
        e.optimize_branch_lengths(trees[:3], trees[3], max_passes=1)
        assert _same(first, e.spr_optimize())
        bare = e.spr_optimize(want_initial_lnl=False, want_passes=False)
        assert bare[2] is None and bare[3] is None and _same(first[:2], bare[:2])
        # a sublist and a permutation of prune, duplicates and rows without a candidate included
        prune = [5, 0, pb.root, 9, 5, 14, 3, 5, int(pb.left[pb.root]), 20]
        rows = e.spr_optimize(prune)
        assert rows[0].shape == (len(prune), pb.N, 3) and e.spr_optimize_profile()["prunes"] == len(prune)
        assert _same([x[prune] for x in first], rows)
        assert _same([x[[9]] for x in first], e.spr_optimize([9]))
        dead = [pb.root, int(pb.left[pb.root]), int(pb.right[pb.root])]
        none = e.spr_optimize(dead)
        assert np.all(np.isnan(none[0])) and np.all(np.isnan(none[1])) and np.all(none[3] == 0) and e.spr_optimize_profile()["candidates"] == 0
        after = (e.log_likelihood(), e.gradient())
        assert _bits(before[0]) == _bits(after[0])
        assert _bits(before[1][0]) == _bits(after[1][0]) and np.array_equal(_bits(before[1][1]), _bits(after[1][1]))
        # an engine that never made the call takes the same path from here on
        node = 5 if pb.root != 5 else 6
        for eng in (e, fresh):
            eng.set_branch_length(node, 0.37)
        x, y = e.gradient(), fresh.gradient()
        assert _bits(x[0]) == _bits(y[0]) and np.array_equal(_bits(x[1]), _bits(y[1]))
        assert not e.rescaling
    with engine_from_problem(pb, rescale=RESCALE_AUTO) as e:  # a scratch that held nothing before
        assert _same(first, e.spr_optimize())


def test_an_entry_does_not_depend_on_the_node_ids():
    """the same tree and data with the internal node ids permuted (children kept in their slots): every entry runs in another row
    at another place among the candidates, from partials stored at other places, and returns the same bits at its new ids"""
    a, _, oa, _, _ = _solved("t8_random_p65")
    c, _, oc, _, _ = _solved("t8_relabelled_p65")
    perm = _relabel((a.left, a.right, a.root, a.branch_lengths), np.random.default_rng(3), a.T)[1]  # (test_nni_gpu._relabelled's)
    assert np.array_equal(c.branch_lengths[perm], a.branch_lengths) and c.root == perm[a.root] and np.any(perm != np.arange(a.N))
    assert _same(oa, [x[np.ix_(perm, perm)] for x in oc])


def test_under_a_memory_cap():
    pb = random_problem(37, 238, 4, seed=99, gaps=0.05)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        e.gradient()
        held = e.profile()["device_bytes"]  # (what the engine holds besides the batch scratch)
        want = e.spr_optimize()
        prof = e.spr_optimize_profile()
        scratch, rows = prof["scratch_bytes"], pb.N - 3
        assert prof["chunks"] == 1 and scratch > 0 and e.profile()["device_bytes"] >= held + scratch
    chunks = 0
    for extra in (0.1, 0.2, 0.3, 0.45):  # the smallest of these caps that leaves room for a row: all of them are too small for all rows
        cap = int(held + extra * scratch)
        with engine_from_problem(pb, rescale=RESCALE_NEVER, max_device_bytes=cap) as e:
            e.gradient()  # (the engine's own buffers are made first: the room is what is left beside them)
            assert e.profile()["tiles"] == 1
            try:
                got = e.spr_optimize()
            except EngineError as err:
                assert err.code == EUNSUPPORTED and "scratch" in str(err), err
                continue
            chunks = e.spr_optimize_profile()["chunks"]
            print(f"cap = held + {extra} x scratch = {cap}: {chunks} chunks; device_bytes {e.profile()['device_bytes']}")
            assert chunks >= 2
            assert e.profile()["device_bytes"] <= cap
            assert _same(want, got)
            break
    assert chunks >= 2, "no cap left room for a row"
    tight = int(held + scratch / rows / 4)
    with engine_from_problem(pb, rescale=RESCALE_NEVER, max_device_bytes=tight) as e:
        assert e.profile()["tiles"] == 1
        assert "scratch" in _refused(e)
        _still_usable(e, pb)
        assert e.profile()["device_bytes"] <= tight


@pytest.mark.parametrize("rescale", [RESCALE_NEVER, RESCALE_AUTO])
def test_underflow_is_reported_in_band(rescale):
    pb = _deep(800, 100, 4, seed=5)
    parent = _parents(pb)
    prune = [n for n in (5, 400, pb.T + 300, pb.T + 700) if n != pb.root and parent[n] != pb.root]
    assert len(prune) >= 3
    with engine_from_problem(pb, rescale=rescale) as e:
        lengths, lnl, lnl0, passes = e.spr_optimize(prune)
        assert not e.rescaling  # never a switch to rescaling
    for i, p in enumerate(prune):
        row = s._candidate_row(pb, parent, p)
        assert row.sum() > 0 and not np.any(np.isfinite(lnl[i])) and not np.any(np.isfinite(lnl0[i])) and np.all(np.isnan(lnl[i, ~row]))
        assert np.all(passes[i, row] == -1) and np.all(passes[i, ~row] == 0)
        start = np.array([_start(pb, p, w) for w in np.flatnonzero(row)])
        assert np.array_equal(_bits(lengths[i, row]), _bits(start))  # the state before the visit that ended the entry


def _refused(e, code=EUNSUPPORTED, **kw):
    with pytest.raises(EngineError) as err:
        e.spr_optimize(**kw)
    assert err.value.code == code, err.value
    assert "phyamd_spr_optimize" in str(err.value), err.value
    print(err.value)
    return str(err.value)


def _still_usable(e, pb):
    ref = pb.log_likelihood()["lnl"]
    assert abs(e.log_likelihood() - ref) <= LNL * abs(ref)


def test_twenty_states_are_refused():
    pb = random_problem(10, 200, 2, seed=20, S=20, gaps=0.03)
    with engine_from_problem(pb, rescale=RESCALE_AUTO) as e:
        assert "4 states" in _refused(e)
        _still_usable(e, pb)


def test_nine_categories_are_refused():
    pb = random_problem(8, 100, 9, seed=9)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        assert "categories" in _refused(e)
        _still_usable(e, pb)


def test_a_rescaling_engine_is_refused():
    pb = random_problem(37, 238, 4, seed=12, gaps=0.03, rescale=1)
    with engine_from_problem(pb, rescale=RESCALE_ALWAYS) as e:
        assert "rescal" in _refused(e)
        ref = pb.log_likelihood()["lnl"]
        assert abs(e.log_likelihood() - ref) <= LNL * abs(ref)


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


def test_an_empty_tip_mask_is_refused():
    pb = random_problem(8, 100, 2, seed=23)
    tp = np.zeros((pb.T, pb.P, 4))
    for tip in range(pb.T):
        tp[tip, np.arange(pb.P), pb.tip_states[tip]] = 1.0
    tp[3, 40] = 0.0  # no state is compatible with this cell
    pb.tip_partials, pb.tip_states = tp, None
    with engine_from_problem(pb, rescale=RESCALE_NEVER, tip_mode="partials") as e:
        assert "empty state mask" in _refused(e)
        e.log_likelihood()


def test_explicit_matrices_are_refused():
    pb = random_problem(8, 100, 2, seed=3)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        e.gradient()
        e.set_node_matrices(2, e.node_matrices(2))
        assert "explicit matrices" in _refused(e)
        _still_usable(e, pb)


def test_flags_and_a_sharded_handle_are_refused():
    pb = random_problem(8, 100, 2, seed=3)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        assert "flags" in _refused(e, flags=GRAD_FOLD_ROOT_FREQS)
        _still_usable(e, pb)
        e.spr_optimize()
    with engine_from_problem(pb, rescale=RESCALE_NEVER, devices=[0, 0]) as e:
        assert "sharded" in _refused(e)
        _still_usable(e, pb)


def test_invalid_arguments_are_refused_by_name():
    pb = random_problem(8, 100, 2, seed=3)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        for kw, what in (({"lower": -1.0}, "bounds"), ({"lower": 1.0, "upper": 1.0}, "bounds"), ({"upper": np.inf}, "bounds"), ({"tolerance": 0.0}, "tolerance"),
                         ({"tolerance": np.nan}, "tolerance"), ({"max_iterations": 0}, "max_iterations"), ({"max_iterations": 1001}, "max_iterations"),
                         ({"lnl_tolerance": -1e-9}, "lnl_tolerance"), ({"lnl_tolerance": np.inf}, "lnl_tolerance"), ({"max_passes": 0}, "max_passes"),
                         ({"max_passes": 1001}, "max_passes"), ({"prune": []}, "count"), ({"prune": [3, 4, -1, 5]}, "prune[2]"),
                         ({"prune": [3, 4, pb.N, 5]}, "prune[2]")):
            assert what in _refused(e, code=EINVAL, **kw), kw
        _still_usable(e, pb)
        e.spr_optimize([3])


def test_no_eigen_system_is_refused():
    from physher_amd.engine import Engine
    pb = random_problem(8, 100, 2, seed=3)
    with Engine(pb.T, pb.P, pb.S, pb.C, rescale=RESCALE_NEVER) as e:
        e.set_topology(pb.left, pb.right, pb.root)
        e.set_branch_lengths(pb.branch_lengths)
        e.set_frequencies(pb.freqs)
        e.set_category_rates(pb.cat_rates, pb.cat_props)
        e.set_pattern_weights(pb.weights)
        for tip in range(pb.T):
            e.set_tip_states(tip, pb.tip_states[tip])
        assert "eigen" in _refused(e, code=EINVAL)
