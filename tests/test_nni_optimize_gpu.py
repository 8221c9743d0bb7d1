"""GPU: phyamd_nni_optimize -- the central branch of every NNI neighbour of the engine's tree optimised in one call -- entry by entry
against the CPU oracle and the NumPy restatement of the rule (tests/nni_optimize_util.py), on the cases of tests/test_nni_gpu.py.

At the returned t*: lnl and d1 against the oracle's evaluation of the rearranged tree (lnL 1e-10 relative, d1 1e-9 * max(1, |ref|):
the suite's bounds for single evaluations); d2 against hessian_util.branch_hessian_diagonal's row v, 1e-9 * max(1, |ref|) -- on the
37-taxon cases through the restatement's one-row evaluator, which is those formulas for the one row and pinned to them in
tests/test_nni_optimize_util.py (the whole diagonal per entry is 0.2 s on 700 patterns x 8 categories).  On the entries that
qualify there (their t* moves by less than tolerance / 10 under relative errors of 1e-9 on d1 and d2: at least nine in ten),
|t* - t_ref| <= tolerance and the iteration counts differ by at most one.  An interior converged entry has
|d1(t*)| <= 2 |d2(t*)| tolerance by the oracle (confirmed for the restatement in the CPU test).  Then the bounds, the iteration
cap, the invariants of the contract, underflow in band, and every refusal."""
import functools

import numpy as np
import pytest

import nni_optimize_util as u
from gpu_util import engine_from_problem, random_problem
from physher_amd.engine import RESCALE_ALWAYS, RESCALE_AUTO, RESCALE_NEVER, EngineError
from test_batch_gpu import _bits, _deep
from test_nni_gpu import CASES, _problem
from test_tree_batch_gpu import _relabel

pytestmark = pytest.mark.gpu
EINVAL, EUNSUPPORTED = -1, -4
TOL, LOWER, UPPER = u.TOLERANCE, u.LOWER, u.UPPER


@functools.lru_cache(maxsize=None)
def _solved(case):
    """the case's problem and the restatement's answer for every entry: computed once, shared, never changed"""
    pb, tip_mode = _problem(case)
    return pb, tip_mode, u.solve_case(pb)


def _interior(t, lower=LOWER, upper=UPPER):
    return lower + 2 * TOL < t < upper - 2 * TOL


def _columns_without_candidate(pb, out):
    lengths, lnl, d1, d2, it = out
    non = [n for n in range(pb.N) if n < pb.T or n == pb.root]
    for a in (lengths, lnl, d1, d2):
        assert a.shape == (3, pb.N) and np.all(np.isnan(a[:, non]))
    assert it.shape == (3, pb.N) and it.dtype == np.int32 and np.all(it[:, non] == 0)


@pytest.mark.parametrize("case", sorted(CASES))
def test_every_entry_matches_the_oracle_and_the_restatement(case):
    pb, tip_mode, solved = _solved(case)
    with engine_from_problem(pb, rescale=RESCALE_AUTO, tip_mode=tip_mode) as e:
        out = e.nni_optimize(lower=LOWER, upper=UPPER, tolerance=TOL, max_iterations=u.MAX_ITERATIONS)
        prof = e.nni_optimize_profile()
        assert not e.rescaling
    lengths, lnl, d1, d2, it = out
    _columns_without_candidate(pb, out)
    assert prof["candidates"] == pb.T - 2 and prof["chunks"] == 1 and prof["scratch_bytes"] > 0
    assert prof["iterations"] == int(np.abs(it).sum())
    worst, qualified = np.zeros(4), 0
    for (k, v), (t_ref, n_ref, good, f) in solved.items():
        t, n = lengths[k, v], int(it[k, v])
        assert LOWER <= t <= UPPER and 0 < n <= u.MAX_ITERATIONS, (case, k, v, t, n)
        if pb.T <= 8:
            rl, r1, r2 = u.evaluate(pb, v, k, t)
        else:
            r = u.rearranged_problem(pb, v, k, t).gradient()
            rl, r1, r2 = r["lnl"], u.branch_gradient_from_cat(r["cat_grad"], pb.cat_rates, pb.cat_props)[v], f(t)[2]
        err = np.array([abs(lnl[k, v] - rl) / abs(rl), abs(d1[k, v] - r1) / max(1.0, abs(r1)), abs(d2[k, v] - r2) / max(1.0, abs(r2)), 0.0])
        if good:
            qualified += 1
            err[3] = abs(t - t_ref)
        worst = np.maximum(worst, err)
        assert err[0] <= 1e-10, (case, k, v, lnl[k, v], rl)
        assert err[1] <= 1e-9, (case, k, v, d1[k, v], r1)
        assert err[2] <= 1e-9, (case, k, v, d2[k, v], r2)
        if good:
            assert err[3] <= TOL, (case, k, v, t, t_ref)
            assert abs(n - n_ref) <= 1, (case, k, v, n, n_ref)
        if _interior(t):
            assert r2 < 0 and abs(r1) <= 2 * abs(r2) * TOL, (case, k, v, t, r1, r2)
    print(f"{case}: {len(solved)} entries ({qualified} qualified), worst lnL {worst[0]:.3e} d1 {worst[1]:.3e} d2 {worst[2]:.3e} |t* - t_ref| {worst[3]:.3e}")
    assert qualified >= 0.9 * len(solved)


def test_start_lengths_are_the_callers():
    """another start per entry: the restatement from the same start, and the same optimum as from the engine's own lengths"""
    case = "t8_relabelled_p65"
    pb, tip_mode, solved = _solved(case)
    start = pb.branch_lengths[None, :] * np.random.default_rng(3).uniform(0.2, 5.0, size=(3, pb.N))
    start[:, 0] = -1.0  # a tip and the root are not read
    start[1, pb.root] = np.nan
    other = u.solve_case(pb, start)
    with engine_from_problem(pb, rescale=RESCALE_NEVER, tip_mode=tip_mode) as e:
        lengths, _, _, _, it = e.nni_optimize(start, lower=LOWER, upper=UPPER, tolerance=TOL, max_iterations=u.MAX_ITERATIONS)
    for (k, v), (t_ref, n_ref, good, _) in other.items():
        if good:
            assert abs(lengths[k, v] - t_ref) <= TOL and abs(int(it[k, v]) - n_ref) <= 1, (k, v, lengths[k, v], t_ref, it[k, v], n_ref)
        if good and solved[(k, v)][2]:  # two converged iterations towards the same optimum: each within a step of it
            assert abs(lengths[k, v] - solved[(k, v)][0]) <= 2 * TOL, (k, v)


def test_an_upper_bound_below_the_optima_and_a_lower_bound_above_them():
    """upper below every interior optimum: the entries that have one end within tolerance of upper with d1 > 0 (every other
    entry's lnL falls from the lower bound on: it ends there, as the restatement's does).  lower above every optimum, the start
    there: every entry has d1 < 0 and stays within tolerance of lower"""
    case = "t8_balanced_p65"
    pb, tip_mode, solved = _solved(case)
    inner = {kv: x[0] for kv, x in solved.items() if _interior(x[0])}
    assert len(inner) >= 3
    upper = 0.5 * min(inner.values())
    capped = u.solve_case(pb, upper=upper)
    with engine_from_problem(pb, rescale=RESCALE_NEVER, tip_mode=tip_mode) as e:
        lengths, _, d1, _, it = e.nni_optimize(lower=LOWER, upper=upper, tolerance=TOL, max_iterations=u.MAX_ITERATIONS)
        for (k, v), (t_ref, n_ref, good, _) in capped.items():
            if (k, v) in inner:
                assert 0 <= upper - lengths[k, v] <= TOL and d1[k, v] > 0 and it[k, v] > 0, (k, v, lengths[k, v], d1[k, v], it[k, v])
            else:
                assert lengths[k, v] - LOWER <= 2 * TOL and d1[k, v] < 0, (k, v, lengths[k, v], d1[k, v])
            if good:
                assert abs(lengths[k, v] - t_ref) <= TOL, (k, v, lengths[k, v], t_ref)
        lower = 2.0 * max(x[0] for x in solved.values())
        start = np.full((3, pb.N), lower)
        lengths, _, d1, _, it = e.nni_optimize(start, lower=lower, upper=UPPER, tolerance=TOL, max_iterations=u.MAX_ITERATIONS)
        for k, v in solved:
            assert 0 <= lengths[k, v] - lower <= TOL and d1[k, v] < 0 and it[k, v] > 0, (k, v, lengths[k, v], d1[k, v], it[k, v])


def test_one_iteration_returns_the_first_proposal():
    case = "t8_random_p65"
    pb, tip_mode, solved = _solved(case)
    with engine_from_problem(pb, rescale=RESCALE_NEVER, tip_mode=tip_mode) as e:
        lengths, lnl, d1, d2, it = e.nni_optimize(lower=LOWER, upper=UPPER, tolerance=TOL, max_iterations=1)
    compared = 0
    for (k, v), x in solved.items():
        f, s = x[3], pb.branch_lengths[v]
        t_ref, n_ref = u.optimise(f, s, max_iterations=1)
        assert n_ref == -1 and it[k, v] == -1, (k, v, n_ref, it[k, v])
        assert np.isfinite(lnl[k, v]) and np.isfinite(d1[k, v]) and np.isfinite(d2[k, v])
        # the proposal is the same midpoint, or the Newton step t - d1 / d2 from the same t with d1 and d2 as far off as the suite
        # allows them (1e-9 * max(1, |ref|) each): twice the first-order change of the step, and a rounding of t itself
        _, r1, r2 = f(s)
        bound = 2e-9 * (max(1.0, abs(r1)) + abs(t_ref - s) * max(1.0, abs(r2))) / abs(r2) + 4 * np.spacing(t_ref)
        if not all(abs(u.optimise(f, s, max_iterations=1, perturb=p)[0] - t_ref) <= bound for p in ((1e-9, -1e-9), (-1e-9, 1e-9))):
            continue  # (such errors change which of the two proposals is made)
        compared += 1
        assert abs(lengths[k, v] - t_ref) <= bound, (k, v, lengths[k, v], t_ref, bound)
    assert compared >= 0.9 * len(solved)


def _same(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a[:4], b[:4])) and np.array_equal(a[4], b[4])


def test_bit_for_bit_across_calls_and_the_engine_is_untouched():
    pb = random_problem(37, 700, 4, seed=31, gaps=0.05)
    with engine_from_problem(pb, rescale=RESCALE_AUTO) as e, engine_from_problem(pb, rescale=RESCALE_AUTO) as fresh:
        before = (e.log_likelihood(), e.gradient())
        first = e.nni_optimize()
        assert _same(first, e.nni_optimize())
        e.nni_log_likelihoods()  # (the same scratch group, with the trial matrices and the slab)
        e.gradient_batch(pb.branch_lengths[None, :] * np.array([[1.0], [1.1]]))
        assert _same(first, e.nni_optimize())
        # the optional outputs do not change the others' bits
        bare = e.nni_optimize(want_derivatives=False, want_iterations=False)
        assert bare[2] is None and bare[3] is None and bare[4] is None
        assert np.array_equal(_bits(bare[0]), _bits(first[0])) and np.array_equal(_bits(bare[1]), _bits(first[1]))
        after = (e.log_likelihood(), e.gradient())
        assert _bits(before[0]) == _bits(after[0])
        assert _bits(before[1][0]) == _bits(after[1][0]) and np.array_equal(_bits(before[1][1]), _bits(after[1][1]))
        assert not e.rescaling
        # the scores of the plain call at the optimised lengths: the definition of lnl, d1 and d2 (the eigen form differs by rounding)
        cand = u.candidates(pb)
        lnl, d1, d2 = e.nni_log_likelihoods(np.where(np.isnan(first[0]), 0.0, first[0]))
        assert np.all(np.abs(lnl[:, cand] - first[1][:, cand]) <= 1e-10 * np.abs(lnl[:, cand]))
        assert np.all(np.abs(d1[:, cand] - first[2][:, cand]) <= 1e-9 * np.maximum(1.0, np.abs(d1[:, cand])))
        assert np.all(np.abs(d2[:, cand] - first[3][:, cand]) <= 1e-9 * np.maximum(1.0, np.abs(d2[:, cand])))
        # an engine that never made the call takes the same path from here on
        node = 5 if pb.root != 5 else 6
        for eng in (e, fresh):
            eng.set_branch_length(node, 0.37)
        a, b = e.gradient(), fresh.gradient()
        assert _bits(a[0]) == _bits(b[0]) and np.array_equal(_bits(a[1]), _bits(b[1]))
    with engine_from_problem(pb, rescale=RESCALE_AUTO) as e:  # a scratch that held nothing before
        assert _same(first, e.nni_optimize())


def test_an_entry_does_not_depend_on_the_other_candidates():
    """the same tree and data with the internal node ids permuted (children kept in their slots): every entry runs at another
    place among the candidates, from partials stored at other places, and returns the same bits at its new id"""
    a, _, _ = _solved("t8_random_p65")
    b, _, _ = _solved("t8_relabelled_p65")
    perm = _relabel((a.left, a.right, a.root, a.branch_lengths), np.random.default_rng(3), a.T)[1]  # (test_nni_gpu._relabelled's)
    assert np.array_equal(b.branch_lengths[perm], a.branch_lengths) and b.root == perm[a.root]
    with engine_from_problem(a, rescale=RESCALE_NEVER) as ea, engine_from_problem(b, rescale=RESCALE_NEVER) as eb:
        oa, ob = ea.nni_optimize(), eb.nni_optimize()
    cand = u.candidates(a)
    assert any(perm[v] != v for v in cand)
    for x, y in zip(oa[:4], ob[:4]):
        assert np.array_equal(_bits(x[:, cand]), _bits(y[:, perm[cand]]))
    assert np.array_equal(oa[4][:, cand], ob[4][:, perm[cand]])


def test_chunks_under_a_memory_cap_change_no_bit():
    pb = random_problem(37, 700, 4, seed=99, gaps=0.05)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        e.gradient()
        e.branch_hessian_diagonal()
        held = e.profile()["device_bytes"]  # (what the engine holds besides the batch scratch)
        want = e.nni_optimize()
        prof = e.nni_optimize_profile()
        assert prof["chunks"] == 1 and prof["scratch_bytes"] > 0 and e.profile()["device_bytes"] >= held + prof["scratch_bytes"]
    cands = pb.T - 2
    per_candidate = 3 * pb.C * 4 * ((pb.P + 63) // 64 * 64) * 8 + 3 * 4 * 8 + 3 * 4  # the coefficients and results of three entries
    walk = prof["scratch_bytes"] - cands * per_candidate
    assert walk > 0
    ran = None
    for part in (0.3, 0.45, 0.6, 0.75, 0.9):  # room for the walk and that part of the candidates: the first cap the call runs under
        cap = int(held + walk + part * cands * per_candidate)
        with engine_from_problem(pb, rescale=RESCALE_NEVER, max_device_bytes=cap) as e:
            e.gradient()
            e.branch_hessian_diagonal()  # (the engine's own buffers are made first: the room is what is left beside them)
            assert e.profile()["tiles"] == 1
            try:
                got = e.nni_optimize()
            except EngineError as err:
                assert err.code == EUNSUPPORTED and "scratch" in str(err), err
                continue
            ran = e.nni_optimize_profile()
            print(f"cap = held + walk + {part} x candidates = {cap}: {ran['chunks']} chunks; device_bytes {e.profile()['device_bytes']}")
            assert e.profile()["device_bytes"] <= cap
            assert _same(want, got)
            assert _same(want, e.nni_optimize()) and e.profile()["device_bytes"] <= cap
            break
    assert ran is not None and ran["chunks"] >= 2 and ran["candidates"] == cands, ran
    tight = int(held + walk / 4)
    with engine_from_problem(pb, rescale=RESCALE_NEVER, max_device_bytes=tight) as e:
        assert e.profile()["tiles"] == 1
        msg = _refused(e)
        assert "scratch" in msg
        _still_usable(e, pb)
        assert e.profile()["device_bytes"] <= tight


@pytest.mark.parametrize("rescale", [RESCALE_NEVER, RESCALE_AUTO])
def test_underflow_is_reported_in_band(rescale):
    pb = _deep(800, 100, 4, seed=5)
    cand = u.candidates(pb)
    with engine_from_problem(pb, rescale=rescale) as e:
        lengths, lnl, d1, d2, it = e.nni_optimize()
        assert not e.rescaling  # never a switch to rescaling
    assert not np.any(np.isfinite(lnl[:, cand]))
    assert np.all(np.isnan(d1)) and np.all(np.isnan(d2))
    assert np.all(it[:, cand] < 0)
    assert np.array_equal(lengths[:, cand], np.broadcast_to(pb.branch_lengths[cand], (3, len(cand))))  # the iterate it happened at: the start


def _refused(e, code=EUNSUPPORTED, **kw):
    with pytest.raises(EngineError) as err:
        e.nni_optimize(**kw)
    assert err.value.code == code, err.value
    assert "phyamd_nni_optimize" in str(err.value) or code == EINVAL, err.value
    print(err.value)
    return str(err.value)


def _still_usable(e, pb):
    ref = pb.log_likelihood()["lnl"]
    assert abs(e.log_likelihood() - ref) <= 1e-10 * abs(ref)


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


def test_explicit_matrices_are_refused():
    pb = random_problem(8, 100, 2, seed=3)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        e.gradient()
        e.set_node_matrices(2, e.node_matrices(2))
        assert "explicit matrices" in _refused(e)
        _still_usable(e, pb)


def test_a_sharded_handle_is_refused():
    pb = random_problem(8, 200, 2, seed=3)
    with engine_from_problem(pb, rescale=RESCALE_NEVER, devices=[0, 0]) as e:
        assert e.shard_count == 2
        assert "shard" in _refused(e)
        _still_usable(e, pb)


def test_flags_are_refused():
    pb = random_problem(8, 100, 2, seed=3)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        assert "flags" in _refused(e, flags=1)
        _still_usable(e, pb)
        e.nni_optimize()


def test_invalid_arguments():
    pb = random_problem(8, 100, 2, seed=3)
    v = u.candidates(pb)[1]
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        want = e.nni_optimize()
        for kw in (dict(lower=-1e-3), dict(lower=0.5, upper=0.5), dict(lower=2.0, upper=1.0), dict(upper=np.inf), dict(lower=np.nan), dict(upper=np.nan)):
            assert "bounds" in _refused(e, code=EINVAL, **kw), kw
        for tol in (0.0, -1e-8, np.inf, np.nan):
            assert "tolerance" in _refused(e, code=EINVAL, tolerance=tol), tol
        for n in (0, -3, 1001):
            assert "max_iterations" in _refused(e, code=EINVAL, max_iterations=n), n
        start = np.tile(pb.branch_lengths, (3, 1))
        for bad in (-0.01, np.nan, np.inf):
            broken = start.copy()
            broken[2, v] = bad
            msg = _refused(e, code=EINVAL, start_lengths=broken)
            assert "start_lengths" in msg and f"[{v}]" in msg, msg
        e.nni_optimize(lower=0.0, max_iterations=1000)  # the ends of what is allowed
        assert _same(want, e.nni_optimize(start))


def test_no_eigen_system_is_refused():
    from physher_amd.engine import Engine
    pb = random_problem(8, 100, 2, seed=3)
    with Engine(pb.T, pb.P, pb.S, pb.C, rescale=RESCALE_NEVER) as e:
        e.set_topology(pb.left, pb.right, pb.root)
        e.set_branch_lengths(pb.branch_lengths)
        e.set_frequencies(pb.freqs)
        e.set_category_rates(pb.cat_rates, pb.cat_props)
        e.set_pattern_weights(pb.weights)
        for t in range(pb.T):
            e.set_tip_states(t, pb.tip_states[t])
        assert "eigen" in _refused(e, code=EINVAL)


def test_two_tips_have_no_candidate():
    pb = random_problem(2, 65, 2, seed=2)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        out = e.nni_optimize()
        assert e.nni_optimize_profile()["candidates"] == 0 and e.nni_optimize_profile()["chunks"] == 0
        assert all(np.all(np.isnan(a)) for a in out[:4]) and np.all(out[4] == 0)
