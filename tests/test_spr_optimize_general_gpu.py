"""GPU: phyamd_spr_optimize_general -- the three branches that meet at the graft point of every SPR regraft of a 20-state engine's tree,
optimised one at a time, pass after pass, in one call -- against the CPU oracle and the NumPy restatement of the rule
(tests/spr_optimize_general_util.py: the batch optimiser's restatement on the rearranged tree with p, w and u marked), on the seven
cases of tests/test_spr_general_gpu.py.  One engine per case, solved once.

Bounds are the suite's for single evaluations: lnL 1e-10 relative.  initial_lnl is spr_log_likelihoods_general's entry of the same
engine; at the returned lengths lnl is the oracle's lnL of the rearranged tree, which recomputes everything from the tips; where the
entry stopped by the rule a further restated pass gains no more than the call stopped on.  Lengths after one pass are compared with the
restatement on the entries that are qualified (the restatement itself moves by less than tolerance / 10 under relative errors of 1e-9
on d1 and d2: at least nine in ten, confirmed for the restatement alone in tests/test_spr_optimize_general_util.py), to within
tolerance.  Then the bits the contract promises, a memory cap, the engine afterwards, folded uppers, the bounds, underflow in band,
PHYAMD_RESCALE_AUTO, and every refusal."""
import functools

import numpy as np
import pytest

import branch_optimize_util as b
import spr_optimize_general_util as t
import test_spr_gpu as s
from gpu_util import engine_from_problem, random_problem
from invalidation_util import parents as _parents
from physher_amd.engine import GRAD_FOLD_ROOT_FREQS, RESCALE_ALWAYS, RESCALE_AUTO, RESCALE_NEVER, Engine, EngineError
from test_batch_gpu import _bits, _deep
from test_nni_general_gpu import _underflow_case

pytestmark = pytest.mark.gpu
EINVAL, EUNSUPPORTED = -1, -4
NAME = "phyamd_spr_optimize_general"
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
        spr = e.spr_log_likelihoods_general()
        full = e.spr_optimize_general()
        prof = e.spr_optimize_profile()
        one = e.spr_optimize_general(max_passes=1)
        assert not e.rescaling
    return pb, spr, full, prof, one


@pytest.mark.parametrize("case", t.CASES)
def test_shapes_and_invariants(case):
    pb, spr, (lengths, lnl, lnl0, passes), prof, _ = _solved(case)
    mask = s._candidate_mask(pb)
    assert lengths.shape == (pb.N, pb.N, 3) and lnl.shape == lnl0.shape == passes.shape == (pb.N, pb.N)
    assert lengths.dtype == lnl.dtype == lnl0.dtype == np.float64 and passes.dtype == np.int32
    # the NaN / 0 pattern is the candidate rule, over the whole table
    assert np.array_equal(np.isfinite(lnl), mask) and np.array_equal(np.isfinite(lnl0), mask) and np.array_equal(np.all(np.isfinite(lengths), axis=2), mask)
    assert np.all(np.isnan(lnl[~mask])) and np.all(np.isnan(lnl0[~mask])) and np.all(np.isnan(lengths[~mask])) and np.all(passes[~mask] == 0)
    assert np.all((lengths[mask] >= LOWER) & (lengths[mask] <= UPPER))
    assert np.all(lnl[mask] >= lnl0[mask])
    assert np.all((passes[mask] != 0) & (np.abs(passes[mask]) <= t.MAX_PASSES))
    print(f"{case}: {int(mask.sum())} candidates, passes {passes[mask].min()}..{passes[mask].max()}; {prof}")
    assert prof["prunes"] == pb.N and prof["candidates"] == mask.sum() and prof["chunks"] == 1 and prof["scratch_bytes"] > 0
    assert prof["visits"] == 3 * int(np.abs(passes).sum()) and prof["iterations"] >= prof["visits"]
    for p, w in t.entries(case):
        assert mask[p, w] and passes[p, w] != 0


@pytest.mark.parametrize("case", t.CASES)
def test_every_checked_entry_against_the_oracle(case):
    pb, spr, (lengths, lnl, lnl0, passes), _, _ = _solved(case)
    parent = _parents(pb)
    worst0, worst, most, stopped = 0.0, 0.0, -np.inf, 0
    for p, w in t.entries(case):
        err0 = abs(lnl0[p, w] - spr[p, w]) / abs(spr[p, w])
        worst0 = max(worst0, err0)
        assert err0 <= LNL, (p, w, lnl0[p, w], spr[p, w])
        q = t.at_lengths(pb, parent, p, w, lengths[p, w])
        want = q.log_likelihood()["lnl"]
        err = abs(lnl[p, w] - want) / abs(want)
        worst = max(worst, err)
        assert err <= LNL, (p, w, lnl[p, w], want)
        if passes[p, w] > 0:
            stopped += 1
            ended, after = b.one_pass(q, t.mask(pb, parent, p, w))
            assert ended is None
            most = max(most, after - want)
            assert after - want <= t.LNL_TOLERANCE + LNL * abs(want), (p, w, after - want)
    print(f"{case}: {len(t.entries(case))} entries, worst relative |initial_lnl - spr| {worst0:.3e}, worst relative lnL error at the result {worst:.3e}; "
          f"{stopped} stopped by the rule, most a further restated pass gains {most:.3e}")


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


def test_bits_across_calls_prune_lists_and_optional_outputs():
    pb, tip_mode = t.problem("t9_random_p130_c8_sets")
    parent = _parents(pb)
    dead = [pb.root, int(pb.left[pb.root]), int(pb.right[pb.root])]
    with engine_from_problem(pb, rescale=RESCALE_AUTO, tip_mode=tip_mode) as e:
        first = e.spr_optimize_general()
        assert _same(first, _solved("t9_random_p130_c8_sets")[2])  # another engine
        assert _same(first, e.spr_optimize_general())
        e.pairwise_distances_general(counts_only=True, want_counts=True)  # (other calls in the same scratch)
        e.nni_optimize_general()
        e.spr_log_likelihoods_general()
        assert _same(first, e.spr_optimize_general())
        bare = e.spr_optimize_general(want_initial_lnl=False, want_passes=False)
        assert bare[2] is None and bare[3] is None and _same(first[:2], bare[:2])
        assert _same(first, e.spr_optimize_general(np.arange(pb.N)))  # None is range(N)
        prune = [5, 0, pb.root, 9, 5, 14, 3, 5, dead[1]]  # duplicates, a permuted order, the root and a child of it
        rows = e.spr_optimize_general(prune)
        assert rows[0].shape == (len(prune), pb.N, 3) and e.spr_optimize_profile()["prunes"] == len(prune)
        assert _same([x[prune] for x in first], rows)
        live = next(p for p in range(pb.N) if p not in dead and parent[p] != pb.root)
        assert _same([x[[live]] for x in first], e.spr_optimize_general([live]))  # a row alone
        assert _same([x[[live, live]] for x in first], e.spr_optimize_general([live, live]))  # a duplicated row
        assert np.any(np.isfinite(first[1][live]))
        none = e.spr_optimize_general(dead)
        assert np.all(np.isnan(none[0])) and np.all(np.isnan(none[1])) and np.all(np.isnan(none[2])) and np.all(none[3] == 0)
        assert e.spr_optimize_profile()["candidates"] == 0
        assert not e.rescaling


def test_under_a_memory_cap():
    pb, tip_mode = t.problem("t17_random_p200_c4")
    with engine_from_problem(pb, rescale=RESCALE_NEVER, tip_mode=tip_mode) as e:
        e.set_keep_partials(True)
        e.gradient()
        held = e.profile()["device_bytes"]  # (what the engine holds besides the batch scratch)
        want = e.spr_optimize_general()
        prof = e.spr_optimize_profile()
        scratch, rows = prof["scratch_bytes"], pb.N - 3
        assert prof["chunks"] == 1 and scratch > 0 and e.profile()["device_bytes"] >= held + scratch
    chunks = 0
    for extra in (0.1, 0.2, 0.3, 0.45):  # the smallest of these caps that leaves room for a row: all of them are too small for all rows
        cap = int(held + extra * scratch)
        with engine_from_problem(pb, rescale=RESCALE_NEVER, tip_mode=tip_mode, max_device_bytes=cap) as e:
            e.set_keep_partials(True)
            e.gradient()  # (the engine's own buffers are made first: the room is what is left beside them)
            assert e.profile()["tiles"] == 1
            try:
                got = e.spr_optimize_general()
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
    with engine_from_problem(pb, rescale=RESCALE_NEVER, tip_mode=tip_mode, max_device_bytes=tight) as e:
        e.set_keep_partials(True)
        e.gradient()
        assert e.profile()["tiles"] == 1
        msg = _refused(e)
        assert "scratch of one row" in msg and "memory budget" in msg
        _still_usable(e, pb)
        assert e.profile()["device_bytes"] <= tight


def test_the_engine_afterwards_is_a_keep_partials_engine_with_the_same_bits():
    """the engine after the call against a fresh engine with set_keep_partials(True) that never made the call: the same bits from
    every later evaluation, also after a change of a length; topology and lengths stay"""
    pb, tip_mode = t.problem("t9_random_p130_c8_sets")
    ref = pb.gradient()
    with engine_from_problem(pb, rescale=RESCALE_AUTO, tip_mode=tip_mode) as a, engine_from_problem(pb, rescale=RESCALE_AUTO, tip_mode=tip_mode) as c:
        first = a.spr_optimize_general()
        assert not a.rescaling
        c.set_keep_partials(True)
        c.gradient()
        for step in range(2):
            la, ga = a.gradient()
            lc, gc = c.gradient()
            assert _bits(np.array([la, a.log_likelihood()])).tolist() == _bits(np.array([lc, c.log_likelihood()])).tolist(), step
            assert np.array_equal(_bits(ga), _bits(gc)), step
            if step == 0:
                assert abs(la - ref["lnl"]) <= LNL * abs(ref["lnl"])  # the engine's tree and lengths are the problem's still
                assert np.abs(ga - ref["cat_grad"]).max() <= 1e-9 * max(1.0, np.abs(ref["cat_grad"]).max())
                assert _same(a.spr_optimize_general(), first)  # a call on an engine already in that state
                a.set_branch_length(3, 0.37)
                c.set_branch_length(3, 0.37)
        moved = a.spr_optimize_general()  # a pending change is evaluated by the call
        assert not _same(moved, first)
        assert _bits(np.array([a.log_likelihood()])).tolist() == _bits(np.array([c.log_likelihood()])).tolist()
        assert not a.rescaling


def test_folded_uppers_do_not_matter():
    """after a keep-partials PHYAMD_GRAD_FOLD_ROOT_FREQS gradient the resident uppers carry pi; the frequencies are not uniform,
    and the call returns the same bits: it reads no resident upper"""
    case = "t9_random_p130_c8_sets"
    pb, tip_mode = t.problem(case)
    assert np.ptp(pb.freqs) > 0.01
    with engine_from_problem(pb, rescale=RESCALE_NEVER, tip_mode=tip_mode) as e:
        e.set_keep_partials(True)
        e.gradient(GRAD_FOLD_ROOT_FREQS)
        folded = e.spr_optimize_general()
    assert _same(folded, _solved(case)[2])


def test_the_bounds_and_one_iteration():
    """a narrow [lower, upper] clamps the lengths, passes is still reported, and the result is still the oracle's lnL at the returned
    lengths; with one iteration per visit every visit makes one proposal"""
    case = "t9_relabelled_p64_c1"
    pb, tip_mode = t.problem(case)
    mask, parent = s._candidate_mask(pb), _parents(pb)
    with engine_from_problem(pb, rescale=RESCALE_NEVER, tip_mode=tip_mode) as e:
        for kw in ({"lower": 0.05, "upper": 0.06}, {"upper": 2e-3}, {"lower": 0.5}):
            lengths, lnl, lnl0, passes = e.spr_optimize_general(**kw)
            lo, hi = kw.get("lower", LOWER), kw.get("upper", UPPER)
            assert np.all((lengths[mask] >= lo) & (lengths[mask] <= hi))
            assert np.all((passes[mask] != 0) & (np.abs(passes[mask]) <= t.MAX_PASSES)) and np.all(passes[~mask] == 0)
            for p, w in t.entries(case)[::5]:
                want = t.at_lengths(pb, parent, p, w, lengths[p, w]).log_likelihood()["lnl"]
                assert abs(lnl[p, w] - want) <= LNL * abs(want), (kw, p, w)
                start = t.rearranged(pb, parent, p, w).log_likelihood()["lnl"]  # initial_lnl is at the start as given, not clamped
                assert abs(lnl0[p, w] - start) <= LNL * abs(start), (kw, p, w)
        lengths, lnl, lnl0, passes = e.spr_optimize_general(max_iterations=1, max_passes=3)
        assert np.all(np.isfinite(lengths[mask])) and np.all(np.isfinite(lnl[mask])) and np.all((lengths[mask] >= LOWER) & (lengths[mask] <= UPPER))
        assert np.all((passes[mask] == -3) | ((passes[mask] >= 1) & (passes[mask] <= 3)))
        assert np.all(lnl[mask] >= lnl0[mask])
        assert e.spr_optimize_profile()["iterations"] == e.spr_optimize_profile()["visits"]
        for p, w in t.entries(case)[::5]:  # (finite outputs that are what they say)
            want = t.at_lengths(pb, parent, p, w, lengths[p, w]).log_likelihood()["lnl"]
            assert abs(lnl[p, w] - want) <= LNL * abs(want)
        lengths, lnl, lnl0, passes = e.spr_optimize_general(max_passes=1, lnl_tolerance=0.0)
        assert np.all(passes[mask & (lnl > lnl0)] == -1)


# ---- underflow --------------------------------------------------------------------------------------------------------------------

def _live_rows(pb, parent, want):
    return [n for n in want if n != pb.root and parent[n] != pb.root]


def test_underflow_is_reported_in_band():
    """the deep caterpillar of tests/test_nni_general_gpu.py, where one pattern's site likelihood is 0 without rescaling: the call
    returns, every candidate of a live row ends in the first pass with a lnL that is not finite and the start as its lengths, and the
    engine is not switched"""
    pb, site = _underflow_case()
    assert site.min() < -330.0 and pb.weights[int(np.argmin(site))] > 0
    parent = _parents(pb)
    prune = _live_rows(pb, parent, (5, pb.T // 2, pb.T + pb.T // 3, pb.N - 3))
    assert len(prune) >= 3
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        lengths, lnl, lnl0, passes = e.spr_optimize_general(prune)  # returns: no error
        assert not e.rescaling
    for i, p in enumerate(prune):
        row = s._candidate_row(pb, parent, p)
        print(f"row of {p}: {int((passes[i, row] == -1).sum())} of {int(row.sum())} candidates end in the first pass")
        assert row.sum() > 0 and np.all(passes[i, row] == -1) and np.all(passes[i, ~row] == 0)
        assert not np.any(np.isfinite(lnl[i])) and not np.any(np.isfinite(lnl0[i])) and np.all(np.isnan(lnl[i, ~row]))
        start = np.array([_start(pb, p, w) for w in np.flatnonzero(row)])
        assert np.array_equal(_bits(lengths[i, row]), _bits(start))  # the state before the visit that ended the entry


def test_an_auto_engine_is_not_switched_where_its_own_lnl_is_finite():
    """PHYAMD_RESCALE_AUTO on the deepest tree the suite has whose own lnL is finite (tests/test_spr_general_gpu.py's choice): the
    call returns, the engine is not rescaling afterwards and every entry is finite or in band"""
    from test_placement_general_gpu import underflow_case
    pb = underflow_case()[0]
    parent = _parents(pb)
    prune = _live_rows(pb, parent, (5, pb.T // 2, pb.T + pb.T // 3, pb.N - 3))
    with engine_from_problem(pb, rescale=RESCALE_AUTO) as e:
        lengths, lnl, lnl0, passes = e.spr_optimize_general(prune)
        assert not e.rescaling
        own = e.log_likelihood()
        assert np.isfinite(own) and not e.rescaling
    for i, p in enumerate(prune):
        row = s._candidate_row(pb, parent, p)
        finite = np.isfinite(lnl[i]) & row
        print(f"AUTO, row of {p}: {int(finite.sum())} of {int(row.sum())} candidates are finite")
        assert row.sum() > 0 and np.all(np.isnan(lnl[i, ~row])) and np.all(passes[i, ~row] == 0)
        assert np.all(lnl[i, finite] < 0) and np.all(passes[i, finite] != 0) and np.all(np.isfinite(lengths[i, finite]))
        band = row & ~finite  # in band: a negative pass index, the state before the visit
        assert np.all(passes[i, band] < 0) and np.all(np.isfinite(lengths[i, band]))


def test_an_engine_that_switches_to_rescaling_during_the_call_is_refused():
    pb = _deep(600, 20, 2, seed=5, S=20)
    with engine_from_problem(pb, rescale=RESCALE_AUTO) as e:
        assert not e.rescaling
        msg = _refused(e, prune=[3])
        assert "rescal" in msg and "PHYAMD_RESCALE_AUTO" in msg
        assert e.rescaling
        _still_usable(e, pb)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------

def _refused(e, code=EUNSUPPORTED, **kw):
    with pytest.raises(EngineError) as err:
        e.spr_optimize_general(**kw)
    assert err.value.code == code, err.value
    print(err.value)
    assert NAME in str(err.value)
    return str(err.value)


def _still_usable(e, pb):
    ref = pb.log_likelihood()["lnl"]
    assert abs(e.log_likelihood() - ref) <= LNL * abs(ref)


def _protein(T=8, P=100, C=2, seed=3, **kw):
    return random_problem(T, P, C, seed=seed, S=20, **kw)


def test_four_states_are_sent_to_the_four_state_call():
    pb = random_problem(8, 100, 2, seed=3)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        msg = _refused(e)
        assert "20 states" in msg and "use phyamd_spr_optimize)" in msg
        _still_usable(e, pb)
        assert np.any(np.isfinite(e.spr_optimize()[1]))


@pytest.mark.parametrize("S", [60, 61])
def test_codon_state_counts_are_not_built(S):
    pb = random_problem(5, 40, 1, seed=S, S=S)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        msg = _refused(e)
        assert "not built" in msg and str(S) in msg
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
        e.spr_optimize_general()


def test_a_missing_eigen_system_and_an_engine_that_is_not_ready_are_refused():
    pb = _protein()
    with Engine(pb.T, pb.P, 20, pb.C, rescale=RESCALE_NEVER) as e:
        e.set_topology(pb.left, pb.right, pb.root)
        e.set_branch_lengths(pb.branch_lengths)
        e.set_frequencies(pb.freqs)
        e.set_category_rates(pb.cat_rates, pb.cat_props)
        e.set_pattern_weights(pb.weights)
        for tip in range(pb.T - 1):
            e.set_tip_states(tip, pb.tip_states[tip])
        assert "eigen" in _refused(e, code=EINVAL)
        e.set_eigen(pb.eval, pb.evec, pb.ivec)
        assert "has no data" in _refused(e, code=EINVAL)  # the last tip: not ready
        e.set_tip_states(pb.T - 1, pb.tip_states[pb.T - 1])
        assert np.any(np.isfinite(e.spr_optimize_general()[1]))


def test_invalid_arguments_are_refused_by_name():
    pb = _protein()
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        for kw, what in (({"lower": -1.0}, "bounds"), ({"lower": 1.0, "upper": 1.0}, "bounds"), ({"upper": np.inf}, "bounds"), ({"tolerance": 0.0}, "tolerance"),
                         ({"tolerance": np.nan}, "tolerance"), ({"max_iterations": 0}, "max_iterations"), ({"max_iterations": 1001}, "max_iterations"),
                         ({"lnl_tolerance": -1e-9}, "lnl_tolerance"), ({"lnl_tolerance": np.inf}, "lnl_tolerance"), ({"max_passes": 0}, "max_passes"),
                         ({"max_passes": 1001}, "max_passes"), ({"prune": []}, "count"), ({"prune": [3, 4, -1, 5]}, "prune[2]"),
                         ({"prune": [3, 4, pb.N, 5]}, "prune[2]")):
            assert what in _refused(e, code=EINVAL, **kw), kw
        out = np.empty((3, pb.N, 3))
        rc = e._lib.phyamd_spr_optimize_general(e._h, 0, 3, None, 1e-8, 10.0, 1e-8, 100, 1e-6, 50, out.ctypes.data, out.ctypes.data, None, None)  # a null list, not N rows
        msg = e._lib.phyamd_last_error().decode()
        print(msg)
        assert rc == EINVAL and NAME in msg and "prune is null" in msg and str(pb.N) in msg
        _still_usable(e, pb)
        e.spr_optimize_general([3])


def test_a_rescaling_engine_is_refused():
    pb = _protein(T=20, P=60, C=2, seed=12, gaps=0.03, rescale=1)
    with engine_from_problem(pb, rescale=RESCALE_ALWAYS) as e:
        assert "rescal" in _refused(e)
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


def test_the_four_state_call_keeps_refusing_twenty_states():
    pb = _protein()
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        with pytest.raises(EngineError) as err:
            e.spr_optimize()
        assert err.value.code == EUNSUPPORTED and "4 states" in str(err.value)
