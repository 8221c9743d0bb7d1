"""GPU: phyamd_nni_optimize_general -- the central branch of every NNI neighbour of a 20-state engine's tree optimised in one call,
from the resident partials -- entry by entry against the CPU oracle and the NumPy restatement of the rule
(tests/nni_optimize_util.py, which knows no state count), on the seven cases of tests/test_nni_general_gpu.py.

At the returned t*: lnl and d1 against the oracle's evaluation of the rearranged tree (lnL 1e-10 relative, d1 1e-9 * max(1, |ref|):
the suite's bounds for single evaluations); d2 against hessian_util.branch_hessian_diagonal's row v, 1e-9 * max(1, |ref|) -- at
17 taxa through the restatement's one-row evaluator, which is those formulas for the one row and pinned to them on these cases in
tests/test_nni_optimize_general_util.py.  On the entries that qualify there (their t* moves by less than tolerance / 10 under
relative errors of 1e-9 on d1 and d2: at least nine in ten), |t* - t_ref| <= tolerance and the iteration counts differ by at most
one.  An interior converged entry has |d1(t*)| <= 2 |d2(t*)| tolerance by the oracle.  Then the call against its sibling
phyamd_nni_log_likelihoods_general at the returned lengths, the start lengths, the bounds, the iteration cap, folded uppers, the
bits, the engine afterwards, underflow in band, and every refusal."""
import functools

import numpy as np
import pytest

import nni_optimize_util as u
from gpu_util import engine_from_problem, random_problem
from physher_amd.engine import GRAD_FOLD_ROOT_FREQS, RESCALE_ALWAYS, RESCALE_AUTO, RESCALE_NEVER, Engine, EngineError
from test_batch_gpu import _bits, _deep
from test_nni_general_gpu import CASES, _case, _underflow_case

pytestmark = pytest.mark.gpu
EINVAL, EUNSUPPORTED = -1, -4
NAME = "phyamd_nni_optimize_general"
TOL, LOWER, UPPER = u.TOLERANCE, u.LOWER, u.UPPER
BIG = "t9_random_p130_c8_sets"  # a workgroup's patterns and a bit, the most categories, unknown cells and engine sets


@functools.lru_cache(maxsize=None)
def _solved(case):
    """the case's problem and the restatement's answer for every entry: computed once, shared, never changed"""
    pb, tip_mode = _case(case)[:2]
    return pb, tip_mode, u.solve_case(pb)


def _interior(t, lower=LOWER, upper=UPPER):
    return lower + 2 * TOL < t < upper - 2 * TOL


def _columns_without_candidate(pb, out):
    lengths, lnl, d1, d2, it = out
    non = [n for n in range(pb.N) if n < pb.T or n == pb.root]
    for a in (lengths, lnl, d1, d2):
        assert a.shape == (3, pb.N) and np.all(np.isnan(a[:, non]))
    assert it.shape == (3, pb.N) and it.dtype == np.int32 and np.all(it[:, non] == 0)


def _against_the_oracle(pb, solved, out, what, one_row=False):
    """every entry at the returned t* against the oracle, and against the restatement where it qualifies; the qualified count"""
    lengths, lnl, d1, d2, it = out
    worst, qualified = np.zeros(4), 0
    for (k, v), (t_ref, n_ref, good, f) in solved.items():
        t, n = lengths[k, v], int(it[k, v])
        assert LOWER <= t <= UPPER and 0 < n <= u.MAX_ITERATIONS, (what, k, v, t, n)
        if not one_row:
            rl, r1, r2 = u.evaluate(pb, v, k, t)
        else:
            r = u.rearranged_problem(pb, v, k, t).gradient()
            rl, r1, r2 = r["lnl"], u.branch_gradient_from_cat(r["cat_grad"], pb.cat_rates, pb.cat_props)[v], f(t)[2]
        err = np.array([abs(lnl[k, v] - rl) / abs(rl), abs(d1[k, v] - r1) / max(1.0, abs(r1)), abs(d2[k, v] - r2) / max(1.0, abs(r2)), 0.0])
        if good:
            qualified += 1
            err[3] = abs(t - t_ref)
        worst = np.maximum(worst, err)
        assert err[0] <= 1e-10, (what, k, v, lnl[k, v], rl)
        assert err[1] <= 1e-9, (what, k, v, d1[k, v], r1)
        assert err[2] <= 1e-9, (what, k, v, d2[k, v], r2)
        if good:
            assert err[3] <= TOL, (what, k, v, t, t_ref)
            assert abs(n - n_ref) <= 1, (what, k, v, n, n_ref)
        if _interior(t):
            assert r2 < 0 and abs(r1) <= 2 * abs(r2) * TOL, (what, k, v, t, r1, r2)
    print(f"{what}: {len(solved)} entries ({qualified} qualified), worst lnL {worst[0]:.3e} d1 {worst[1]:.3e} d2 {worst[2]:.3e} |t* - t_ref| {worst[3]:.3e}")
    return qualified


@pytest.mark.parametrize("case", sorted(CASES))
def test_every_entry_matches_the_oracle_and_the_restatement(case):
    pb, tip_mode, solved = _solved(case)
    with engine_from_problem(pb, rescale=RESCALE_AUTO, tip_mode=tip_mode) as e:
        out = e.nni_optimize_general(lower=LOWER, upper=UPPER, tolerance=TOL, max_iterations=u.MAX_ITERATIONS)
        prof = e.nni_optimize_profile()
        assert not e.rescaling
    _columns_without_candidate(pb, out)
    assert prof["candidates"] == pb.T - 2 and prof["chunks"] == 1 and prof["scratch_bytes"] > 0
    assert prof["iterations"] == int(np.abs(out[4]).sum())
    assert len(solved) == 3 * (pb.T - 2)
    qualified = _against_the_oracle(pb, solved, out, case, one_row=pb.T >= 17)
    assert qualified >= 0.9 * len(solved)


def test_the_sibling_call_returns_the_same_values_at_the_returned_lengths():
    """nni_log_likelihoods_general at central = the returned lengths: two evaluations of the same engine by the same coefficients,
    only the order of the sum over patterns differs (lnL 1e-12 relative, d1 and d2 1e-9 * max(1, |ref|))"""
    for case in ("t17_random_p200_c4", BIG):
        pb, tip_mode, _ = _solved(case)
        cand = u.candidates(pb)
        with engine_from_problem(pb, rescale=RESCALE_AUTO, tip_mode=tip_mode) as e:
            lengths, lnl, d1, d2, _ = e.nni_optimize_general()
            rl, r1, r2 = e.nni_log_likelihoods_general(np.where(np.isnan(lengths), 0.0, lengths))
        err = [np.abs(lnl[:, cand] - rl[:, cand]) / np.abs(rl[:, cand]), np.abs(d1[:, cand] - r1[:, cand]) / np.maximum(1.0, np.abs(r1[:, cand])),
               np.abs(d2[:, cand] - r2[:, cand]) / np.maximum(1.0, np.abs(r2[:, cand]))]
        print(f"{case} against the sibling: worst lnL {err[0].max():.3e} d1 {err[1].max():.3e} d2 {err[2].max():.3e}")
        assert err[0].max() <= 1e-12 and err[1].max() <= 1e-9 and err[2].max() <= 1e-9


def test_start_lengths_are_the_callers():
    """another start per entry: the restatement from the same start, and the same optimum as from the engine's own lengths"""
    case = "t9_relabelled_p64_c1"
    pb, tip_mode, solved = _solved(case)
    start = pb.branch_lengths[None, :] * np.random.default_rng(3).uniform(0.2, 5.0, size=(3, pb.N))
    start[:, 0] = -1.0  # a tip and the root are not read
    start[1, pb.root] = np.nan
    other = u.solve_case(pb, start)
    with engine_from_problem(pb, rescale=RESCALE_NEVER, tip_mode=tip_mode) as e:
        lengths, _, _, _, it = e.nni_optimize_general(start, lower=LOWER, upper=UPPER, tolerance=TOL, max_iterations=u.MAX_ITERATIONS)
    compared = 0
    for (k, v), (t_ref, n_ref, good, _) in other.items():
        if good:
            compared += 1
            assert abs(lengths[k, v] - t_ref) <= TOL and abs(int(it[k, v]) - n_ref) <= 1, (k, v, lengths[k, v], t_ref, it[k, v], n_ref)
        if good and solved[(k, v)][2]:  # two converged iterations towards the same optimum: each within a step of it
            assert abs(lengths[k, v] - solved[(k, v)][0]) <= 2 * TOL, (k, v)
    assert compared >= 0.9 * len(other)


def test_an_upper_bound_below_the_optima_and_a_lower_bound_above_them():
    """upper below every interior optimum: the entries that have one end within tolerance of upper with d1 > 0 (every other
    entry's lnL falls from the lower bound on: it ends there, as the restatement's does).  lower above every optimum, the start
    there: every entry has d1 < 0 (by the restatement too) and stays within tolerance of lower"""
    case = "t9_caterpillar_p70_c4_pinv"
    pb, tip_mode, solved = _solved(case)
    inner = {kv: x[0] for kv, x in solved.items() if _interior(x[0])}
    assert len(inner) >= 3
    upper = 0.5 * min(inner.values())
    capped = u.solve_case(pb, upper=upper)
    with engine_from_problem(pb, rescale=RESCALE_NEVER, tip_mode=tip_mode) as e:
        lengths, _, d1, _, it = e.nni_optimize_general(lower=LOWER, upper=upper, tolerance=TOL, max_iterations=u.MAX_ITERATIONS)
        for (k, v), (t_ref, n_ref, good, _) in capped.items():
            if (k, v) in inner:
                assert 0 <= upper - lengths[k, v] <= TOL and d1[k, v] > 0 and it[k, v] > 0, (k, v, lengths[k, v], d1[k, v], it[k, v])
            else:
                assert lengths[k, v] - LOWER <= 2 * TOL and d1[k, v] < 0, (k, v, lengths[k, v], d1[k, v])
            if good:
                assert abs(lengths[k, v] - t_ref) <= TOL, (k, v, lengths[k, v], t_ref)
        lower = 2.0 * max(x[0] for x in solved.values())
        assert all(x[3](lower)[1] < 0 for x in solved.values())
        start = np.full((3, pb.N), lower)
        lengths, _, d1, _, it = e.nni_optimize_general(start, lower=lower, upper=UPPER, tolerance=TOL, max_iterations=u.MAX_ITERATIONS)
        for k, v in solved:
            assert 0 <= lengths[k, v] - lower <= TOL and d1[k, v] < 0 and it[k, v] > 0, (k, v, lengths[k, v], d1[k, v], it[k, v])


def test_one_iteration_returns_the_first_proposal():
    pb, tip_mode, solved = _solved(BIG)
    with engine_from_problem(pb, rescale=RESCALE_NEVER, tip_mode=tip_mode) as e:
        lengths, lnl, d1, d2, it = e.nni_optimize_general(lower=LOWER, upper=UPPER, tolerance=TOL, max_iterations=1)
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


def test_folded_uppers_are_used_as_they_are():
    """after a PHYAMD_GRAD_FOLD_ROOT_FREQS keep-partials gradient the resident uppers carry pi and the call leaves pi out.  That
    arithmetic is the likelihood's for uniform frequencies only (include/physher_amd.h), so the problem has them
    (tests/test_nni_general_gpu.py's): every entry against the oracle and the restatement, under and beside the root"""
    from golden_util import reversible_eigen
    from invalidation_util import parents
    from oracle import phyoracle as po
    src = random_problem(9, 70, 2, seed=41, S=20, gaps=0.05)
    rng = np.random.default_rng(42)
    r = rng.uniform(0.5, 3.0, size=(20, 20))
    freqs = np.full(20, 1.0 / 20)
    ev, U, Ui = reversible_eigen(0.5 * (r + r.T), freqs)
    pb = po.Problem(src.left, src.right, src.root, src.weights, ev, U, Ui, freqs, src.cat_rates, src.cat_props, src.branch_lengths, tip_states=src.tip_states)
    parent = parents(pb)
    assert any(parent[v] == pb.root for v in u.candidates(pb)) and any(parent[v] != pb.root for v in u.candidates(pb))
    solved = u.solve_case(pb)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        e.set_keep_partials(True)
        e.gradient(GRAD_FOLD_ROOT_FREQS)
        folded = e.nni_optimize_general()
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        plain = e.nni_optimize_general()
    for out, what in ((folded, "folded uppers"), (plain, "plain uppers")):
        _columns_without_candidate(pb, out)
        assert _against_the_oracle(pb, solved, out, what) >= 0.9 * len(solved)


def _same(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a[:4], b[:4])) and np.array_equal(a[4], b[4])


def test_bits_do_not_depend_on_the_call_the_scratch_the_outputs_or_the_other_entries():
    pb, tip_mode, _ = _solved(BIG)
    cand = u.candidates(pb)
    start = pb.branch_lengths[None, :] * np.random.default_rng(5).uniform(0.5, 2.0, size=(3, pb.N))
    with engine_from_problem(pb, rescale=RESCALE_AUTO, tip_mode=tip_mode) as e:
        first = e.nni_optimize_general(start)
        assert _same(first, e.nni_optimize_general(start))
        e.pairwise_distances_general(counts_only=True, want_counts=True)  # (other calls in the same scratch)
        e.nni_log_likelihoods_general(start)
        assert _same(first, e.nni_optimize_general(start))
        # the optional outputs do not change the others' bits
        bare = e.nni_optimize_general(start, want_derivatives=False, want_iterations=False)
        assert bare[2] is None and bare[3] is None and bare[4] is None
        assert np.array_equal(_bits(bare[0]), _bits(first[0])) and np.array_equal(_bits(bare[1]), _bits(first[1]))
        # an entry's bits are its own: every other entry's start changed
        k, v = 1, cand[3]
        other = pb.branch_lengths[None, :] * np.random.default_rng(6).uniform(0.5, 2.0, size=(3, pb.N))
        other[k, v] = start[k, v]
        moved = e.nni_optimize_general(other)
        assert all(_bits(a[k, v]) == _bits(b[k, v]) for a, b in zip(moved[:4], first[:4])) and moved[4][k, v] == first[4][k, v]
        assert not np.array_equal(moved[4][:, cand], first[4][:, cand]) or not np.array_equal(_bits(moved[0][:, cand]), _bits(first[0][:, cand]))
        assert not e.rescaling
    with engine_from_problem(pb, rescale=RESCALE_AUTO, tip_mode=tip_mode) as e:  # a scratch that held nothing before
        assert _same(first, e.nni_optimize_general(start))


def test_chunks_under_a_memory_cap_change_no_bit():
    """a cap that cuts the candidates into at least two chunks: the same bits; one that leaves no room for a candidate: refused"""
    pb, tip_mode, _ = _solved(BIG)
    with engine_from_problem(pb, rescale=RESCALE_NEVER, tip_mode=tip_mode) as e:
        e.set_keep_partials(True)
        e.gradient()
        held = e.profile()["device_bytes"]  # (what the engine holds besides the batch scratch)
        want = e.nni_optimize_general()
        prof = e.nni_optimize_profile()
        scratch = prof["scratch_bytes"]
        assert prof["chunks"] == 1 and scratch > 0
    chunks = 0
    for extra in (0.6, 0.5, 0.4, 0.3, 0.2):  # the largest of these caps that cuts the candidates into two chunks or more
        cap = int(held + extra * scratch)
        with engine_from_problem(pb, rescale=RESCALE_NEVER, tip_mode=tip_mode, max_device_bytes=cap) as e:
            e.set_keep_partials(True)
            e.gradient()  # (the engine's own buffers are made first: the room is what is left beside them)
            assert e.profile()["tiles"] == 1
            try:
                got = e.nni_optimize_general()
            except EngineError as err:
                assert err.code == EUNSUPPORTED and "scratch" in str(err), err
                continue
            prof = e.nni_optimize_profile()
            print(f"cap = held + {extra} x scratch = {cap}: {prof['chunks']} chunks; device_bytes {e.profile()['device_bytes']}")
            assert e.profile()["device_bytes"] <= cap
            assert _same(want, got)
            assert _same(want, e.nni_optimize_general()) and e.profile()["device_bytes"] <= cap
            assert prof["candidates"] == pb.T - 2 and prof["iterations"] == int(np.abs(got[4]).sum())
            if prof["chunks"] >= 2:
                chunks = prof["chunks"]
                break
    assert chunks >= 2, "no cap cut the candidates into two chunks"
    refused = False
    for extra in (0.001, 0.005, 0.01, 0.02):  # the smallest of these caps that holds the engine: not a candidate's scratch beside it
        try:
            e = engine_from_problem(pb, rescale=RESCALE_NEVER, tip_mode=tip_mode, max_device_bytes=int(held + extra * scratch))
        except EngineError:
            continue
        with e:
            e.set_keep_partials(True)
            try:
                e.gradient()
            except EngineError:
                continue
            if e.profile()["tiles"] != 1:
                continue
            assert "scratch of one candidate" in _refused(e)
            _still_usable(e, pb)
            refused = True
            break
    assert refused, "no cap held the engine"


def test_the_engine_afterwards_is_a_keep_partials_engine_with_the_same_bits():
    """the engine after the call against a fresh engine with set_keep_partials(True) that never made the call: the same bits from
    every later evaluation, also after a change of a length; topology, lengths and models stay"""
    pb, tip_mode, _ = _solved(BIG)
    ref = pb.gradient()
    with engine_from_problem(pb, rescale=RESCALE_AUTO, tip_mode=tip_mode) as a, engine_from_problem(pb, rescale=RESCALE_AUTO, tip_mode=tip_mode) as b:
        first = a.nni_optimize_general()
        assert not a.rescaling
        b.set_keep_partials(True)
        b.gradient()
        at = a.branch_log_likelihood(0, float(pb.branch_lengths[0]))[0]  # read from the resident partials of a keep-partials engine
        assert abs(at - ref["lnl"]) <= 1e-10 * abs(ref["lnl"])
        for step in range(2):
            la, ga = a.gradient()
            lb, gb = b.gradient()
            assert _bits(np.array([la, a.log_likelihood()])).tolist() == _bits(np.array([lb, b.log_likelihood()])).tolist(), step
            assert np.array_equal(_bits(ga), _bits(gb)), step
            if step == 0:
                assert abs(la - ref["lnl"]) <= 1e-10 * abs(ref["lnl"])
                assert np.abs(ga - ref["cat_grad"]).max() <= 1e-9 * max(1.0, np.abs(ref["cat_grad"]).max())
                assert _same(a.nni_optimize_general(), first)  # a call on an engine already in that state changes nothing
                a.set_branch_length(3, 0.37)
                b.set_branch_length(3, 0.37)
        moved = a.nni_optimize_general()  # a pending change is evaluated by the call
        assert not np.array_equal(_bits(moved[1]), _bits(first[1]))
        assert _bits(np.array([a.log_likelihood()])).tolist() == _bits(np.array([b.log_likelihood()])).tolist()
        assert not a.rescaling


# ---- underflow --------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _underflowing():
    return _underflow_case()


def _in_band(pb, out, cols):
    """the in-band form at the entries `cols` (a boolean [3][N]): an iterate inside the bounds, a lnL that is not finite, NaN
    derivatives, a negative count"""
    lengths, lnl, d1, d2, it = out
    assert np.all((lengths[cols] >= LOWER) & (lengths[cols] <= UPPER))  # the iterate it happened at
    assert not np.any(np.isfinite(lnl[cols]))
    assert np.all(np.isnan(d1[cols])) and np.all(np.isnan(d2[cols]))
    assert np.all(it[cols] < 0)


def test_underflow_is_reported_in_band():
    """the deep caterpillar of tests/test_nni_general_gpu.py, where one pattern's site likelihood is 0 without rescaling: the in-band
    form alone (no value is compared with the oracle, whose unrescaled partials are not repeatable at an underflowed pattern)"""
    pb, site = _underflowing()
    assert site.min() < -330.0 and pb.weights[int(np.argmin(site))] > 0
    cand = u.candidates(pb)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        out = e.nni_optimize_general()  # returns: no error
        assert not e.rescaling  # never a switch to rescaling
    _columns_without_candidate(pb, out)
    cols = np.zeros((3, pb.N), dtype=bool)
    cols[:, cand] = True
    _in_band(pb, out, cols)


def test_an_auto_engine_is_never_switched_to_rescaling_by_the_call():
    """PHYAMD_RESCALE_AUTO on the deep caterpillars.  On the tree above the engine's OWN evaluation is -inf, so the gradient that makes
    the partials resident switches the engine to rescaling and the call refuses
    (test_an_engine_that_switches_to_rescaling_during_the_call_is_refused): under AUTO the in-band end can be met only where the
    engine's own lnL is finite.  So this is the deepest such tree the suite has -- tests/test_placement_general_gpu.py's, where one
    pattern's site likelihood is a subnormal number near 1e-313 --: the call returns, the engine is not rescaling afterwards, and
    every entry is either finite with a positive count or has the in-band form.  (On an MI355X all 678 entries are finite, also
    from a start of 10 inside [9, 10]: an NNI on this tree moves no site likelihood by the ten orders of magnitude left.)"""
    from test_placement_general_gpu import underflow_case
    pb = underflow_case()[0]
    cand = u.candidates(pb)
    with engine_from_problem(pb, rescale=RESCALE_AUTO) as e:
        out = e.nni_optimize_general()
        assert not e.rescaling
        own = e.log_likelihood()
        assert np.isfinite(own) and not e.rescaling
    _columns_without_candidate(pb, out)
    lengths, lnl, d1, d2, it = out
    cols = np.zeros((3, pb.N), dtype=bool)
    cols[:, cand] = True
    bad = cols & ~np.isfinite(lnl)
    print(f"AUTO, T = {pb.T}: {int(bad.sum())} of {int(cols.sum())} entries are not finite")
    _in_band(pb, out, bad)
    good = cols & ~bad
    assert np.all(it[good] > 0) and np.all(np.isfinite(d1[good])) and np.all(np.isfinite(d2[good]))
    assert np.all((lengths[good] >= LOWER) & (lengths[good] <= UPPER))


# ---- refusals ---------------------------------------------------------------------------------------------------------------------

def _refused(e, code=EUNSUPPORTED, **kw):
    with pytest.raises(EngineError) as err:
        e.nni_optimize_general(**kw)
    assert err.value.code == code, err.value
    print(err.value)
    assert NAME in str(err.value)
    return str(err.value)


def _still_usable(e, pb):
    ref = pb.log_likelihood()["lnl"]
    assert abs(e.log_likelihood() - ref) <= 1e-10 * abs(ref)


def _protein(T=8, P=100, C=2, seed=3, **kw):
    return random_problem(T, P, C, seed=seed, S=20, **kw)


def test_four_states_are_sent_to_the_four_state_call():
    pb = random_problem(8, 100, 2, seed=3)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        msg = _refused(e)
        assert "20 states" in msg and "use phyamd_nni_optimize)" in msg
        _still_usable(e, pb)


def test_sixty_one_states_are_not_built():
    pb = random_problem(5, 40, 1, seed=61, S=61)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        msg = _refused(e)
        assert "not built" in msg and "61" in msg
        _still_usable(e, pb)


def test_nine_categories_are_refused():
    pb = _protein(C=9, seed=9)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        assert "categories" in _refused(e)
        _still_usable(e, pb)


def test_flags_are_refused():
    pb = _protein()
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        assert "flags" in _refused(e, flags=1)
        _still_usable(e, pb)
        e.nni_optimize_general()


def test_a_missing_eigen_system_is_refused():
    pb = _protein()
    with Engine(pb.T, pb.P, 20, pb.C, rescale=RESCALE_NEVER) as e:
        e.set_topology(pb.left, pb.right, pb.root)
        e.set_branch_lengths(pb.branch_lengths)
        e.set_frequencies(pb.freqs)
        e.set_category_rates(pb.cat_rates, pb.cat_props)
        e.set_pattern_weights(pb.weights)
        for t in range(pb.T):
            e.set_tip_states(t, pb.tip_states[t])
        assert "eigen" in _refused(e, code=EINVAL)


def test_an_engine_that_is_not_ready_is_refused():
    pb = _protein()
    with Engine(pb.T, pb.P, 20, pb.C, rescale=RESCALE_NEVER) as e:
        e.set_topology(pb.left, pb.right, pb.root)
        with pytest.raises(EngineError) as err:
            e.nni_optimize_general()
        assert err.value.code == EINVAL, err.value


def test_a_rescaling_engine_is_refused():
    pb = _protein(T=20, P=60, C=2, seed=12, gaps=0.03, rescale=1)
    with engine_from_problem(pb, rescale=RESCALE_ALWAYS) as e:
        assert "rescal" in _refused(e)
        _still_usable(e, pb)


def test_an_engine_that_switches_to_rescaling_during_the_call_is_refused():
    pb = _deep(600, 20, 2, seed=5, S=20)
    with engine_from_problem(pb, rescale=RESCALE_AUTO) as e:
        assert not e.rescaling
        msg = _refused(e)
        assert "rescal" in msg and "PHYAMD_RESCALE_AUTO" in msg
        assert e.rescaling
        _still_usable(e, pb)


def test_a_tiled_engine_is_refused():
    pb = _protein(T=20, P=2000, C=2, seed=13, gaps=0.03)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        e.gradient()
        base = e.profile()["device_bytes"]
    cap = None
    for frac in np.arange(0.9, 0.1, -0.05):  # (the search of tests/test_nni_gpu.py for a cap that tiles)
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
    pb = _protein()
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        e.gradient()
        e.set_node_matrices(2, e.node_matrices(2))
        assert "explicit matrices" in _refused(e)
        _still_usable(e, pb)


def test_a_sharded_handle_is_refused():
    pb = _protein(P=200)
    with engine_from_problem(pb, rescale=RESCALE_NEVER, devices=[0, 0]) as e:
        assert e.shard_count == 2
        assert "shard" in _refused(e)
        _still_usable(e, pb)


def test_invalid_arguments():
    pb = _protein()
    v = u.candidates(pb)[1]
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        want = e.nni_optimize_general()
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
        e.nni_optimize_general(lower=0.0, max_iterations=1000)  # the ends of what is allowed
        assert _same(want, e.nni_optimize_general(start))


def test_null_outputs_are_refused_before_the_handle_is_looked_at():
    import ctypes
    from physher_amd import _lib
    lib = _lib.load()
    fn = getattr(lib, NAME)
    pb = _protein()
    out = (ctypes.c_double * (3 * pb.N))()
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        for lengths, lnl, word in ((None, out, b"null lengths"), (out, None, b"null lnl")):
            assert fn(e._h, 0, None, LOWER, UPPER, TOL, 100, lengths, lnl, None, None, None) == EINVAL
            msg = lib.phyamd_last_error()
            assert NAME.encode() in msg and word in msg, msg
        _still_usable(e, pb)


def test_two_tips_have_no_candidate():
    pb = random_problem(2, 65, 2, seed=2, S=20)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        out = e.nni_optimize_general()
        assert e.nni_optimize_profile()["candidates"] == 0 and e.nni_optimize_profile()["chunks"] == 0
        assert all(np.all(np.isnan(a)) for a in out[:4]) and np.all(out[4] == 0)
