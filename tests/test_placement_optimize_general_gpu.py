"""GPU: phyamd_placement_optimize_general -- the three branches around chosen (query, edge) placements of a 20-state engine, optimised
one at a time, pass after pass, in one call -- against the CPU oracle and the NumPy restatement of the rule
(tests/placement_optimize_general_util.py: the batch optimiser's restatement on the placed tree with n, x and z marked).  It mirrors
tests/test_placement_optimize_gpu.py.

Bounds are the suite's for single evaluations: lnL 1e-10 relative.  At the returned lengths lnl is the oracle's lnL of the placed
tree, which recomputes everything from the tips.  Lengths are compared with the restatement on the entries that are qualified (the
restatement itself moves by less than tolerance / 10 under relative errors of 1e-9 on d1 and d2: at least nine in ten of a case,
confirmed for the restatement alone in tests/test_placement_optimize_general_util.py), to within tolerance.  Then the placement
scores at the start, the bits the contract promises, a memory cap, the engine afterwards, an lnL that is not finite, and every
refusal.

The queries are random sequences, so distal and proximal are strongly correlated and some entries use up max_passes = 50:
passes = -50, as the rule says.  A further restated pass gains no more than lnl_tolerance on every entry whose stop test held
(passes > 0); on the others the rule promises no such thing, and they are checked for everything else.  At least one entry of every
case, and at least half of all entries, are stopped by the rule."""
import copy
import ctypes
import functools

import numpy as np
import pytest

import branch_optimize_util as b
import placement_general_util as u
import placement_optimize_general_util as t
from gpu_util import engine_from_problem, random_problem
from physher_amd.engine import RESCALE_ALWAYS, RESCALE_AUTO, RESCALE_NEVER, Engine, EngineError
from test_batch_gpu import _bits, _deep
from test_placement_general_gpu import underflow_case

pytestmark = pytest.mark.gpu
EINVAL, EUNSUPPORTED = -1, -4
NAME = "phyamd_placement_optimize_general"
TOL, LOWER, UPPER = t.TOLERANCE, t.LOWER, t.UPPER
LNL = 1e-10  # relative
SUBSETS = {"t9_caterpillar_p70_c4": (2, 5)}  # the case whose one pass is also restated with branches = 5; every case runs branches = 2


def _same(x, y):
    return all((p is None and q is None) or np.array_equal(_bits(p) if p.dtype == np.float64 else p, _bits(q) if q.dtype == np.float64 else q) for p, q in zip(x, y))


def _starts(pb, cands, split, pendant=t.PENDANT):
    return np.array([t.start(pb, n, split, pendant) for _, n in cands])


@functools.lru_cache(maxsize=None)
def _solved(name):
    """the case on its own engine, once: the call with its defaults and its profile, the placement scores at the start, the call
    with one pass, and one pass with the pendant length alone (and, for one case, with the two edge halves alone)"""
    pb, tip_mode, codes, sets, split, cands = t.case(name)
    with engine_from_problem(pb, rescale=RESCALE_AUTO, tip_mode=tip_mode) as e:
        full = e.placement_optimize_general(codes, cands, sets, split=split)
        prof = e.placement_optimize_profile()
        scores = e.placement_log_likelihoods_general(codes, [t.PENDANT], split=split, sets=sets)[0][0]
        one = e.placement_optimize_general(codes, cands, sets, split=split, max_passes=1)
        subsets = {br: (e.placement_optimize_general(codes, cands, sets, split=split, branches=br, max_passes=1), e.placement_optimize_profile())
                   for br in SUBSETS.get(name, (2,))}
        assert not e.rescaling
    return full, prof, scores, one, subsets


@pytest.mark.parametrize("name", sorted(t.CASES))
def test_every_entry(name):
    pb, _, codes, sets, split, cands = t.case(name)
    (lengths, lnl, lnl0, passes), prof, scores, _, _ = _solved(name)
    count = len(cands)
    # 1. shapes, bounds, monotone, stopped by the rule, the profile
    assert lengths.shape == (count, 3) and lnl.shape == lnl0.shape == passes.shape == (count,)
    assert lengths.dtype == lnl.dtype == lnl0.dtype == np.float64 and passes.dtype == np.int32
    assert np.all((lengths >= LOWER) & (lengths <= UPPER)) and np.all(np.isfinite(lnl)) and np.all(np.isfinite(lnl0))
    assert np.all(lnl >= lnl0)
    assert np.all((passes != 0) & (np.abs(passes) <= t.MAX_PASSES))
    assert prof["candidates"] == count and prof["edges"] == len(set(cands[:, 1].tolist())) == pb.N - 1 and prof["chunks"] == 1 and prof["scratch_bytes"] > 0, prof
    assert prof["visits"] == 3 * int(np.abs(passes).sum()) and prof["iterations"] >= prof["visits"], prof
    # 2. the start is the placement call's entry
    want0 = scores[cands[:, 0], cands[:, 1]]
    err0 = np.abs(lnl0 - want0) / np.abs(want0)
    print(f"{name}: {count} candidates, passes {passes.min()}..{passes.max()} ({int((passes < 0).sum())} at the cap), "
          f"worst relative |initial_lnl - placement score| {err0.max():.3e}; {prof}")
    assert np.all(err0 <= LNL)
    # 3. lnl is the oracle's at the returned lengths, and a further restated pass gains no more than the call stopped on
    worst, most = 0.0, -np.inf
    for i, (q, n) in enumerate(cands):
        p = t.placed(pb, n, codes[q], sets, lengths[i], t.reference(name))
        want = p.log_likelihood()["lnl"]
        err = abs(lnl[i] - want) / abs(want)
        worst = max(worst, err)
        assert err <= LNL, (q, n, lnl[i], want)
        if passes[i] < 0:
            assert passes[i] == -t.MAX_PASSES, (q, n, passes[i])  # finite all the way: only the cap ends an entry with passes < 0
            continue
        ended, after = b.one_pass(p, t.mask(pb, n))
        assert ended is None
        most = max(most, after - want)
        assert after - want <= t.LNL_TOLERANCE + LNL * abs(want), (q, n, after - want)
    print(f"{name}: worst relative lnL error at the result {worst:.3e}, most a further restated pass gains {most:.3e}")
    assert np.any(passes > 0)  # at least one entry of the case stops by the rule


def test_half_of_all_entries_stop_by_the_rule():
    passes = np.concatenate([_solved(name)[0][3] for name in sorted(t.CASES)])
    print(f"{int((passes > 0).sum())} of {len(passes)} entries stop by the rule")
    assert 2 * int((passes > 0).sum()) >= len(passes)


def _compare_one_pass(name, branches, got, what):
    pb, _, codes, sets, split, cands = t.case(name)
    lengths, lnl, lnl0, passes = got
    assert np.all(np.abs(passes) == 1)
    start = _starts(pb, cands, split)
    marked = np.array([bool(branches >> k & 1) for k in range(3)])
    assert np.array_equal(_bits(lengths[:, ~marked]), _bits(start[:, ~marked]))  # what is not marked: the start, bit for bit
    ref = t.one_pass_thrice(name, branches)
    good, worst = 0, 0.0
    for i, (q, n) in enumerate(cands.tolist()):
        three, qualified = ref[(q, n)]
        if not qualified:
            continue
        good += 1
        # a query that is unknown at every pattern: P(t) 1 = 1, so lnL does not depend on its pendant length at all, d1 and d2 are
        # rounding noise around 0 whose sign steers the bisection, and relative errors on them qualify nothing.  Its distal and
        # proximal lengths (which do not depend on the pendant length either) are compared like everybody's
        determined = [0, 2] if np.all(codes[q] == u.UNKNOWN) else [0, 1, 2]
        err = np.abs(lengths[i] - three)[determined].max()
        worst = max(worst, err)
        assert err <= TOL, (what, q, n, lengths[i], three)
        want = t.placed(pb, n, codes[q], sets, lengths[i], t.reference(name)).log_likelihood()["lnl"]
        assert abs(lnl[i] - want) <= LNL * abs(want)
    qualified = sum(1 for _, ok in ref.values() if ok)
    print(f"{name}, {what}: {qualified} of {len(ref)} entries qualify, worst |t - t_ref| {worst:.3e}")
    assert qualified >= 0.9 * len(ref) and good >= 0.9 * len(cands)


@pytest.mark.parametrize("name", sorted(t.CASES))
def test_one_pass_is_the_restatements(name):
    _compare_one_pass(name, 7, _solved(name)[3], "all three branches")


@pytest.mark.parametrize("name", sorted(t.CASES))
def test_a_subset_of_the_branches(name):
    _, _, _, _, _, cands = t.case(name)
    for branches, (got, prof) in _solved(name)[4].items():
        _compare_one_pass(name, branches, got, f"branches {branches}")
        assert prof["visits"] == bin(branches).count("1") * len(cands), prof
    assert 2 in _solved(name)[4]
    assert set(_solved("t9_caterpillar_p70_c4")[4]) == {2, 5}


def test_duplicates_return_the_same_bits():
    cands = t.case("t4_p66_c1_twice")[5]
    assert t.CASES["t4_p66_c1_twice"][8] == 5
    full = _solved("t4_p66_c1_twice")[0]
    for i in range(len(cands) - 5, len(cands)):
        j = next(k for k in range(i) if np.array_equal(cands[k], cands[i]))
        assert _same([x[[i]] for x in full], [x[[j]] for x in full]), (i, j)


@pytest.mark.parametrize("name", ["t9_p130_c8", "t5_p300_c2"])
def test_bits_do_not_depend_on_the_call_the_order_or_the_batch(name):
    """more tiles than waves, all eleven sets; and past 256 patterns"""
    pb, tip_mode, codes, sets, split, cands = t.case(name)
    first = _solved(name)[0]
    call = lambda e, c, cd, *a, **kw: e.placement_optimize_general(c, cd, sets, *a, split=split, **kw)
    with engine_from_problem(pb, rescale=RESCALE_AUTO, tip_mode=tip_mode) as e:
        assert _same(first, call(e, codes, cands))  # another engine, a scratch that held nothing
        assert _same(first, call(e, codes, cands))
        e.pairwise_distances_general(counts_only=True, want_counts=True)  # (other calls in the same scratch)
        e.placement_log_likelihoods_general(codes, [0.3], sets=sets)
        perm = np.random.default_rng(9).permutation(len(cands))
        assert _same([x[perm] for x in first], call(e, codes, cands[perm]))
        subset = perm[:len(cands) // 3]
        assert _same([x[subset] for x in first], call(e, codes, cands[subset]))
        for i in range(len(cands)):  # every candidate as its own call, with its query alone
            q, n = cands[i]
            assert _same([x[[i]] for x in first], call(e, codes[q:q + 1], [[0, n]])), i
        more = np.concatenate([codes, u.random_codes(np.random.default_rng(77), 1, pb.P, len(sets))])  # an unrelated query and its candidates, in between
        extra = np.array([(len(codes), n) for n in u.edges(pb)[::3]], dtype=np.int32)
        mixed = np.concatenate([cands[:5], extra, cands[5:], cands[2:4]])  # (and two duplicates)
        got = call(e, more, mixed)
        keep = np.r_[0:5, 5 + len(extra):5 + len(extra) + len(cands) - 5]
        assert _same(first, [x[keep] for x in got])
        assert _same([x[2:4] for x in first], [x[-2:] for x in got])
        bare = call(e, codes, cands, want_initial_lnl=False, want_passes=False)
        assert bare[2] is None and bare[3] is None and _same(first[:2], bare[:2])
        starts = np.full(len(cands), t.PENDANT)  # the default start, spelled out
        assert _same(first, call(e, codes, cands, starts))
        assert not e.rescaling


def test_under_a_memory_cap():
    """a cap that cuts the candidates into at least two chunks: the same bits; one that leaves no room for a candidate: refused"""
    name = "t9_caterpillar_p70_c4"
    pb, tip_mode, codes, sets, split, cands = t.case(name)
    want = _solved(name)[0]
    call = lambda e: e.placement_optimize_general(codes, cands, sets, split=split)
    with engine_from_problem(pb, rescale=RESCALE_NEVER, tip_mode=tip_mode) as e:
        e.set_keep_partials(True)
        e.gradient()
        held = e.profile()["device_bytes"]  # (what the engine holds besides the batch scratch)
        assert _same(want, call(e))
        prof = e.placement_optimize_profile()
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
                got = call(e)
            except EngineError as err:
                assert err.code == EUNSUPPORTED and "scratch" in str(err), err
                continue
            prof = e.placement_optimize_profile()
            print(f"cap = held + {extra} x scratch = {cap}: {prof['chunks']} chunks; device_bytes {e.profile()['device_bytes']}")
            assert e.profile()["device_bytes"] <= cap
            assert _same(want, got)
            assert prof["candidates"] == len(cands) and prof["edges"] == pb.N - 1
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
            msg = _refused(e, codes, cands, sets=sets, split=split)
            assert "scratch of one candidate" in msg
            _still_usable(e, pb)
            refused = True
            break
    assert refused, "no cap held the engine"


def test_the_engine_afterwards_is_a_keep_partials_engine_with_the_same_bits():
    """the engine after the call against a fresh engine built with set_keep_partials(True) that never made the call: the same bits
    from every later evaluation, also after a change of a length; topology and lengths unchanged"""
    name = "t9_p130_c8"
    pb, tip_mode, codes, sets, split, cands = t.case(name)
    ref = pb.gradient()
    with engine_from_problem(pb, rescale=RESCALE_AUTO, tip_mode=tip_mode) as a, engine_from_problem(pb, rescale=RESCALE_AUTO, tip_mode=tip_mode) as c:
        first = a.placement_optimize_general(codes, cands, sets, split=split)
        assert _same(first, _solved(name)[0])
        c.set_keep_partials(True)
        c.gradient()
        for n in range(pb.N):  # the lengths, through the matrices the engine holds for them (the topology: through every bit below)
            if n != pb.root:
                assert np.array_equal(_bits(a.node_matrices(n)), _bits(c.node_matrices(n))), n
        lnl, cg = a.gradient()
        assert abs(lnl - ref["lnl"]) <= 1e-10 * abs(ref["lnl"])
        assert np.abs(cg - ref["cat_grad"]).max() <= 1e-9 * max(1.0, np.abs(ref["cat_grad"]).max())
        for step in range(2):
            la, ga = a.gradient()
            lc, gc = c.gradient()
            assert _bits(np.array([la, a.log_likelihood()])).tolist() == _bits(np.array([lc, c.log_likelihood()])).tolist(), step
            assert np.array_equal(_bits(ga), _bits(gc)), step
            if step == 0:
                assert _same(a.placement_optimize_general(codes, cands, sets, split=split), first)  # a call on an engine already in that state
                a.set_branch_length(3, 0.37)
                c.set_branch_length(3, 0.37)
        moved = a.placement_optimize_general(codes, cands, sets, split=split)  # a pending change is evaluated by the call
        assert not np.array_equal(_bits(moved[1]), _bits(first[1]))
        assert _bits(np.array([a.log_likelihood()])).tolist() == _bits(np.array([c.log_likelihood()])).tolist()
        assert not a.rescaling


def test_an_lnl_that_is_not_finite_ends_the_entry_in_band():
    """the deep caterpillar of tests/test_placement_general_gpu.py, at that test's point: split 0 and a pendant start of 1e-20, where
    query 0's site likelihood at one pattern is exactly 0 on the `dead` tip edges, and only the proximal branch marked, so that
    distal and pendant stay there.  (In the proximal length the zero is a product of a subnormal number and one below 1e-15, term by
    term: exactly 0 whatever the arithmetic.)  Queries 1 and 2 are unknown at that pattern and stay finite on the same edges.

    What the restatement's run returns for an entry whose start is not finite is read off the rule and the oracle's own lnL at the
    start, not off branch_optimize_util.Edge: on this tree the oracle's gradient(want_partials=True) without rescaling returns
    partials that differ from call to call at the underflowed pattern (three Edges of one placed problem gave lnL -inf, -inf and
    -371 at the same length), while its log_likelihood is -inf every time.  The start's proximal length lies inside the bounds, so
    the first iterate of the first visit is the start itself: the rule ends the entry there with passes = -1, the start's lengths
    and that lnL.  The finite entries go through the restatement as everywhere else, and their lengths are compared where its
    three runs agree"""
    pb, codes, k, dead = underflow_case()
    plain = copy.copy(pb)
    plain.rescale = 0  # the restatement on partials that are not rescaled, like the engine's
    edges = [int(n) for n in dead[:2]] + [n for n in (pb.T + 5, pb.T + 100) if n != pb.root]
    cands = np.array([(0, n) for n in edges[:2]] + [(q, n) for q in (1, 2) for n in edges], dtype=np.int32)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        lengths, lnl, lnl0, passes = e.placement_optimize_general(codes, cands, None, np.full(len(cands), 1e-20), split=0.0, branches=4)
        assert not e.rescaling
    reference = u.reference_partials(plain)
    kind = lambda v: "nan" if np.isnan(v) else "-inf" if np.isneginf(v) else "+inf" if np.isposinf(v) else "finite"
    seen = set()
    for i, (q, n) in enumerate(cands.tolist()):
        s = t.start(pb, n, 0.0, 1e-20)
        assert LOWER <= s[2] <= UPPER
        at_start = t.placed(plain, n, codes[q], [], s, reference).log_likelihood()["lnl"]
        print(f"query {q} on edge {n}: passes {passes[i]}, lnl {lnl[i]}, initial {lnl0[i]} (the oracle's at the start {at_start}), lengths {lengths[i]}")
        assert kind(lnl0[i]) == kind(at_start), (q, n)
        assert np.array_equal(_bits(lengths[i, :2]), _bits(s[:2]))  # not marked: the start, bit for bit
        seen.add(kind(lnl[i]))
        if kind(at_start) != "finite":  # ended in band at the first iterate: the state before that visit
            assert passes[i] == -1 and kind(lnl[i]) == kind(at_start) and np.array_equal(_bits(lengths[i]), _bits(s)), (q, n, lengths[i], s)
            continue
        assert abs(lnl0[i] - at_start) <= LNL * abs(at_start)
        ref = t.placed(plain, n, codes[q], [], lengths[i], reference).log_likelihood()["lnl"]
        assert abs(lnl[i] - ref) <= LNL * abs(ref) and lnl[i] >= lnl0[i], (q, n, lnl[i], ref)
        runs = [t.run(plain, n, codes[q], [], 0.0, 4, pendant=1e-20, reference=reference, perturb=p) for p in b.PERTURBATIONS]
        three, want, initial, p = runs[0]
        if all(r[3] == p and abs(r[0][2] - three[2]) < TOL / 10 for r in runs[1:]):  # qualified
            assert np.sign(passes[i]) == np.sign(p) and abs(lengths[i, 2] - three[2]) <= TOL, (q, n, lengths[i], three)
    assert seen == {"-inf", "finite"}
    assert np.all(np.isneginf(lnl[:2])) and np.all(np.isneginf(lnl0[:2])) and np.all(passes[:2] == -1)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------

def _refused(e, codes, cands, code=EUNSUPPORTED, **kw):
    with pytest.raises(EngineError) as err:
        e.placement_optimize_general(codes, cands, **kw)
    assert err.value.code == code, err.value
    print(err.value)
    assert NAME in str(err.value), err.value
    return str(err.value)


def _still_usable(e, pb):
    ref = pb.log_likelihood()["lnl"]
    assert abs(e.log_likelihood() - ref) <= 1e-10 * abs(ref)


def _queries(pb, Q=2):
    codes = u.random_codes(np.random.default_rng(0), Q, pb.P)
    return codes, np.array([(q, n) for q in range(Q) for n in u.edges(pb)[:4]], dtype=np.int32)


def _protein(T=8, P=100, C=2, seed=3, **kw):
    return random_problem(T, P, C, seed=seed, S=20, **kw)


def test_invalid_arguments():
    pb = _protein()
    codes, cands = _queries(pb, 3)
    sets = np.array([0b110, 1 << 19 | 1], dtype=np.uint64)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        want = e.placement_optimize_general(codes, cands, sets)
        for node in (pb.root, -1, pb.N, pb.N + 5):
            bad = cands.copy()
            bad[5, 1] = node
            msg = _refused(e, codes, bad, code=EINVAL)
            assert "candidates[5]" in msg and ("root" in msg if node == pb.root else "node is outside" in msg)
        for query in (-1, 3):
            bad = cands.copy()
            bad[2, 0] = query
            msg = _refused(e, codes, bad, code=EINVAL)
            assert "candidates[2]" in msg and "query" in msg
        assert "queries" in _refused(e, codes[:0], cands, code=EINVAL)
        assert "count" in _refused(e, codes, cands[:0], code=EINVAL)
        for branches in (0, 8):
            assert "branches" in _refused(e, codes, cands, code=EINVAL, branches=branches)
        for split in (-1e-9, 1.0 + 1e-9, np.nan, np.inf):
            assert "split" in _refused(e, codes, cands, code=EINVAL, split=split)
        for bad in (0.0, -0.2, np.nan, np.inf):
            start = np.full(len(cands), 0.1)
            start[4] = bad
            assert "pendant_start[4]" in _refused(e, codes, cands, code=EINVAL, pendant_start=start)
        assert "bounds" in _refused(e, codes, cands, code=EINVAL, lower=1.0, upper=0.5)
        assert "tolerance" in _refused(e, codes, cands, code=EINVAL, tolerance=0.0)
        assert "max_iterations" in _refused(e, codes, cands, code=EINVAL, max_iterations=0)
        assert "lnl_tolerance" in _refused(e, codes, cands, code=EINVAL, lnl_tolerance=-1.0)
        assert "max_passes" in _refused(e, codes, cands, code=EINVAL, max_passes=1001)
        assert "set_count" in _refused(e, codes, cands, code=EINVAL, sets=np.arange(1, 13, dtype=np.uint64))
        for word in (0, 1 << 20, 1 << 40):
            assert "sets[1]" in _refused(e, codes, cands, code=EINVAL, sets=np.array([3, word], dtype=np.uint64))
        for value, given in ((21, None), (23, sets), (32, sets), (255, sets)):
            wrong = codes.copy()
            wrong[2, 57] = value
            msg = _refused(e, wrong, cands, code=EINVAL, sets=given)
            assert "query 2" in msg and "pattern 57" in msg and str(value) in msg
        lib, out, lnl = e._lib, np.empty((len(cands), 3)), np.empty(len(cands))
        ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        call = lambda m, nsets, st, c, le, ln: lib.phyamd_placement_optimize_general(e._h, 0, 3, m, nsets, st, len(cands), c, None, 0.5, 7, 1e-8, 10.0, 1e-8, 100, 1e-6, 50, le,
                                                                                     ln, None, None)
        for args, word in (((None, 0, None, ptr(cands), ptr(out), ptr(lnl)), b"null codes"), ((ptr(codes), 0, None, None, ptr(out), ptr(lnl)), b"null candidates"),
                           ((ptr(codes), 0, None, ptr(cands), None, ptr(lnl)), b"null lengths"), ((ptr(codes), 0, None, ptr(cands), ptr(out), None), b"null lnl"),
                           ((ptr(codes), 2, None, ptr(cands), ptr(out), ptr(lnl)), b"null sets")):
            assert call(*args) == EINVAL and word in lib.phyamd_last_error()
        assert lib.phyamd_placement_optimize_general(None, 0, 3, ptr(codes), 0, None, len(cands), ptr(cands), None, 0.5, 7, 1e-8, 10.0, 1e-8, 100, 1e-6, 50, ptr(out), ptr(lnl),
                                                     None, None) == EINVAL and b"null engine" in lib.phyamd_last_error()
        with pytest.raises(ValueError):
            e.placement_optimize_general(codes[:, :-1], cands)
        with pytest.raises(ValueError):
            e.placement_optimize_general(codes, cands[:, :1])
        with pytest.raises(ValueError):
            e.placement_optimize_general(codes, cands, None, np.full(len(cands) + 1, 0.1))
        assert _same(want, e.placement_optimize_general(codes, cands, sets))
        _still_usable(e, pb)


def test_flags_are_refused():
    pb = _protein()
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        assert "flags" in _refused(e, *_queries(pb), flags=1)
        _still_usable(e, pb)
        e.placement_optimize_general(*_queries(pb))


def test_a_missing_eigen_system_is_refused():
    pb = _protein()
    with Engine(pb.T, pb.P, 20, pb.C, rescale=RESCALE_NEVER) as e:
        e.set_topology(pb.left, pb.right, pb.root)
        e.set_branch_lengths(pb.branch_lengths)
        e.set_frequencies(pb.freqs)
        e.set_category_rates(pb.cat_rates, pb.cat_props)
        e.set_pattern_weights(pb.weights)
        for tip in range(pb.T):
            e.set_tip_states(tip, pb.tip_states[tip])
        assert "eigen" in _refused(e, *_queries(pb), code=EINVAL)


def test_four_states_are_sent_to_the_four_state_call():
    pb = random_problem(8, 100, 2, seed=3)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        msg = _refused(e, *_queries(pb))
        assert "20 states" in msg and "use phyamd_placement_optimize" in msg
        _still_usable(e, pb)


@pytest.mark.parametrize("S", [60, 61])
def test_codon_state_counts_are_not_built(S):
    pb = random_problem(5, 40, 1, seed=S, S=S)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        msg = _refused(e, *_queries(pb))
        assert "not built" in msg and str(S) in msg
        _still_usable(e, pb)


def test_nine_categories_are_refused():
    pb = _protein(C=9, seed=9)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        assert "categories" in _refused(e, *_queries(pb))
        _still_usable(e, pb)


def test_a_rescaling_engine_is_refused():
    pb = _protein(T=20, P=60, C=2, seed=12, gaps=0.03, rescale=1)
    with engine_from_problem(pb, rescale=RESCALE_ALWAYS) as e:
        assert "rescal" in _refused(e, *_queries(pb))
        _still_usable(e, pb)


def test_an_engine_that_switches_to_rescaling_during_the_call_is_refused():
    pb = _deep(600, 20, 2, seed=5, S=20)
    with engine_from_problem(pb, rescale=RESCALE_AUTO) as e:
        assert not e.rescaling
        msg = _refused(e, *_queries(pb))
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
        assert "tiled" in _refused(e, *_queries(pb))
        _still_usable(e, pb)


def test_explicit_matrices_are_refused():
    pb = _protein()
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        e.gradient()
        e.set_node_matrices(2, e.node_matrices(2))
        assert "explicit matrices" in _refused(e, *_queries(pb))
        _still_usable(e, pb)


def test_a_sharded_handle_is_refused():
    pb = _protein(P=200)
    with engine_from_problem(pb, rescale=RESCALE_NEVER, devices=[0, 0]) as e:
        assert e.shard_count == 2
        assert "shard" in _refused(e, *_queries(pb))
        _still_usable(e, pb)
