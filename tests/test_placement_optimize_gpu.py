"""GPU: phyamd_placement_optimize -- the three branches around chosen (query, edge) placements, optimised one at a time, pass after
pass, in one call -- against the CPU oracle and the NumPy restatement of the rule (tests/placement_optimize_util.py: the batch
optimiser's restatement on the placed tree with n, x and z marked).

Bounds are the suite's for single evaluations: lnL 1e-10 relative.  At the returned lengths lnl is the oracle's lnL of the placed
tree, which recomputes everything from the tips.  Lengths are compared with the restatement on the entries that are qualified (the
restatement itself moves by less than tolerance / 10 under relative errors of 1e-9 on d1 and d2: at least nine in ten, confirmed for
the restatement alone in tests/test_placement_optimize_util.py), to within tolerance.  Then the existing device routes -- the
placement scores at the start, phyamd_spr_optimize on the tree that holds the query -- the bits the contract promises, a memory
cap, underflow in band, and every refusal.

The queries are random sequences, so on most edges the pendant length climbs to the upper bound along a flat ridge, and some
entries (2 of 20 up to 9 of 64 per case in the restatement) use up max_passes = 50: passes = -50, as the rule says.  A further
restated pass gains no more than lnl_tolerance on every entry whose stop test held (passes > 0); on the others the rule promises no
such thing, and they are checked for everything else."""
import ctypes
import functools

import numpy as np
import pytest

import branch_optimize_util as b
import placement_optimize_util as t
import placement_util as u
from gpu_util import engine_from_problem, random_problem
from physher_amd.engine import RESCALE_ALWAYS, RESCALE_AUTO, RESCALE_NEVER, Engine, EngineError
from test_batch_gpu import _bits, _deep

pytestmark = pytest.mark.gpu
EINVAL, EUNSUPPORTED = -1, -4
TOL, LOWER, UPPER = t.TOLERANCE, t.LOWER, t.UPPER
LNL = 1e-10  # relative
SUBSETS = {"t9_p65_c2": (2, 5)}  # the case whose one pass is also restated with branches = 5; every case runs branches = 2


def _same(x, y):
    return all((p is None and q is None) or np.array_equal(_bits(p) if p.dtype == np.float64 else p, _bits(q) if q.dtype == np.float64 else q) for p, q in zip(x, y))


def _starts(pb, cands, split, pendant=t.PENDANT):
    return np.array([t.start(pb, n, split, pendant) for _, n in cands])


@functools.lru_cache(maxsize=None)
def _solved(name):
    """the case on its own engine, once: the call with its defaults and its profile, the placement scores at the start, the call
    with one pass, and one pass with the pendant length alone (and, for one case, with the two edge halves alone)"""
    pb, tip_mode, masks, split, cands = t.case(name)
    with engine_from_problem(pb, rescale=RESCALE_AUTO, tip_mode=tip_mode) as e:
        full = e.placement_optimize(masks, cands, split=split)
        prof = e.placement_optimize_profile()
        scores = e.placement_log_likelihoods(masks, [t.PENDANT], split=split)[0][0]
        one = e.placement_optimize(masks, cands, split=split, max_passes=1)
        subsets = {br: (e.placement_optimize(masks, cands, split=split, branches=br, max_passes=1), e.placement_optimize_profile()) for br in SUBSETS.get(name, (2,))}
        assert not e.rescaling
    return full, prof, scores, one, subsets


@pytest.mark.parametrize("name", sorted(t.CASES))
def test_every_entry(name):
    pb, _, masks, split, cands = t.case(name)
    (lengths, lnl, lnl0, passes), prof, scores, _, _ = _solved(name)
    count = len(cands)
    # 1. shapes, bounds, monotone, stopped by the rule, the profile
    assert lengths.shape == (count, 3) and lnl.shape == lnl0.shape == passes.shape == (count,)
    assert lengths.dtype == lnl.dtype == lnl0.dtype == np.float64 and passes.dtype == np.int32
    assert np.all((lengths >= LOWER) & (lengths <= UPPER)) and np.all(np.isfinite(lnl)) and np.all(np.isfinite(lnl0))
    assert np.all(lnl >= lnl0 - LNL * np.abs(lnl))
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
        p = t.placed(pb, n, masks[q], lengths[i])
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
    assert np.any(passes > 0)


def _compare_one_pass(name, branches, got, what):
    pb, _, masks, split, cands = t.case(name)
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
        err = np.abs(lengths[i] - three).max()
        worst = max(worst, err)
        assert err <= TOL, (what, q, n, lengths[i], three)
        want = t.placed(pb, n, masks[q], lengths[i]).log_likelihood()["lnl"]
        assert abs(lnl[i] - want) <= LNL * abs(want)
    qualified = sum(1 for _, ok in ref.values() if ok)
    print(f"{name}, {what}: {qualified} of {len(ref)} entries qualify, worst |t - t_ref| {worst:.3e}")
    assert qualified >= 0.9 * len(ref) and good >= 0.9 * len(cands)


@pytest.mark.parametrize("name", sorted(t.CASES))
def test_one_pass_is_the_restatements(name):
    _compare_one_pass(name, 7, _solved(name)[3], "all three branches")


@pytest.mark.parametrize("name", sorted(t.CASES))
def test_a_subset_of_the_branches(name):
    pb, _, _, _, cands = t.case(name)
    for branches, (got, prof) in _solved(name)[4].items():
        _compare_one_pass(name, branches, got, f"branches {branches}")
        assert prof["visits"] == bin(branches).count("1") * len(cands), prof
    assert 2 in _solved(name)[4]
    assert set(_solved("t9_p65_c2")[4]) == {2, 5}


def test_duplicates_return_the_same_bits():
    _, _, _, _, cands = t.case("t4_p66_c1_twice")
    assert t.CASES["t4_p66_c1_twice"][7] == 5
    full = _solved("t4_p66_c1_twice")[0]
    for i in range(len(cands) - 5, len(cands)):
        j = next(k for k in range(i) if np.array_equal(cands[k], cands[i]))
        assert _same([x[[i]] for x in full], [x[[j]] for x in full]), (i, j)


def test_agrees_with_the_spr_call_on_the_tree_that_holds_the_query():
    """a tip x of a 10-taxon tree that is the right child of its parent, pruned as SPR_move prunes it; x placed on the 9-taxon base
    tree with split 0.5 and the start t_x is row x of spr_optimize on the 10-taxon engine, one pass: in its rearranged trees x keeps
    its slot, so the visit order (target, x, their parent) is (n, x, z) (placement_util.pruned_base holds the id mapping)"""
    pb = random_problem(10, 130, 4, seed=41, gaps=0.05)
    parent = u.parents(pb)
    x = next(k for k in range(pb.T) if parent[k] != pb.root and parent[parent[k]] != pb.root and pb.right[parent[k]] == k)
    base, new_id, row, tx = u.pruned_base(pb, x)
    with engine_from_problem(pb, rescale=RESCALE_AUTO) as e:
        spr = [a[0] for a in e.spr_optimize([x], max_passes=1)]
    targets = np.nonzero(np.isfinite(spr[1]))[0]
    assert len(targets) == pb.N - 4 and np.all(new_id[targets] >= 0)  # all but the root, x, its parent and its sibling
    cands = np.stack([np.zeros(len(targets), dtype=np.int32), new_id[targets].astype(np.int32)], axis=1)
    with engine_from_problem(base, rescale=RESCALE_AUTO, tip_mode="partials") as e:
        lengths, lnl, lnl0, passes = e.placement_optimize(row[None, :], cands, np.full(len(cands), tx), split=0.5, max_passes=1)
    good, worst_t, worst_l = 0, 0.0, 0.0
    for i, w in enumerate(targets):
        other = spr[0][w][[1, 0, 2]]  # (t_p, t_w, t_u) -> (distal t_w, pendant t_p, proximal t_u)
        worst_l = max(worst_l, abs(lnl[i] - spr[1][w]) / abs(spr[1][w]))
        assert abs(lnl[i] - spr[1][w]) <= LNL * abs(spr[1][w]) and abs(lnl0[i] - spr[2][w]) <= LNL * abs(spr[2][w]), (w, lnl[i], spr[1][w])
        assert passes[i] == spr[3][w]
        n, runs = int(cands[i, 1]), []
        for perturb in b.PERTURBATIONS:
            p = t.placed(base, n, row, t.start(base, n, 0.5, tx))
            assert b.one_pass(p, t.mask(base, n), perturb)[0] is None
            runs.append(p.branch_lengths[t.nodes(base, n)])
        if np.all([np.abs(r - runs[0]) < TOL / 10 for r in runs[1:]]):
            good += 1
            worst_t = max(worst_t, np.abs(lengths[i] - other).max())
            assert np.all(np.abs(lengths[i] - other) <= TOL), (w, lengths[i], other)
    print(f"{len(targets)} targets against spr_optimize: worst relative lnL difference {worst_l:.3e}; {good} qualified, worst |t - t'| {worst_t:.3e}")
    assert good >= 0.9 * len(targets)


def test_bits_do_not_depend_on_the_call_the_order_or_the_batch():
    name = "t9_p130_c8"
    pb, tip_mode, masks, split, cands = t.case(name)
    first = _solved(name)[0]
    with engine_from_problem(pb, rescale=RESCALE_AUTO, tip_mode=tip_mode) as e:
        before = (e.log_likelihood(), e.gradient())
        assert _same(first, e.placement_optimize(masks, cands, split=split))  # another engine, a scratch that held nothing
        assert _same(first, e.placement_optimize(masks, cands, split=split))
        e.nni_optimize()  # (other calls in the same scratch)
        e.placement_log_likelihoods(masks, [0.3])
        e.spr_optimize([3], max_passes=1)
        perm = np.random.default_rng(9).permutation(len(cands))
        assert _same([x[perm] for x in first], e.placement_optimize(masks, cands[perm], split=split))
        for i in range(len(cands)):  # every candidate as its own call, with its query alone
            q, n = cands[i]
            one = e.placement_optimize(masks[q:q + 1], [[0, n]], split=split)
            assert _same([x[[i]] for x in first], one), i
        more = np.concatenate([masks, u.random_masks(np.random.default_rng(77), 1, pb.P)])  # an unrelated query and its candidates, in between
        extra = np.array([(len(masks), n) for n in u.edges(pb)[::3]], dtype=np.int32)
        mixed = np.concatenate([cands[:10], extra, cands[10:]])
        got = e.placement_optimize(more, mixed, split=split)
        keep = np.r_[0:10, 10 + len(extra):len(mixed)]
        assert _same(first, [x[keep] for x in got])
        bare = e.placement_optimize(masks, cands, split=split, want_initial_lnl=False, want_passes=False)
        assert bare[2] is None and bare[3] is None and _same(first[:2], bare[:2])
        starts = np.full(len(cands), t.PENDANT)  # the default start, spelled out
        assert _same(first, e.placement_optimize(masks, cands, starts, split=split))
        after = (e.log_likelihood(), e.gradient())
        assert _bits(before[0]) == _bits(after[0])
        assert _bits(before[1][0]) == _bits(after[1][0]) and np.array_equal(_bits(before[1][1]), _bits(after[1][1]))
        assert not e.rescaling


def test_bits_do_not_depend_on_the_order_or_the_batch_past_256_patterns():
    """600 patterns, three trips of a thread through qopt_coefficients: shuffled candidates, and every candidate as its own call"""
    name = "t4_p600_c4"
    pb, tip_mode, masks, split, cands = t.case(name)
    assert pb.P > 2 * 256
    first = _solved(name)[0]
    with engine_from_problem(pb, rescale=RESCALE_AUTO, tip_mode=tip_mode) as e:
        assert _same(first, e.placement_optimize(masks, cands, split=split))  # another engine, a scratch that held nothing
        perm = np.random.default_rng(9).permutation(len(cands))
        assert _same([x[perm] for x in first], e.placement_optimize(masks, cands[perm], split=split))
        for i in range(len(cands)):  # every candidate as its own call, with its query alone
            q, n = cands[i]
            one = e.placement_optimize(masks[q:q + 1], [[0, n]], split=split)
            assert _same([x[[i]] for x in first], one), i
        assert not e.rescaling


def test_under_a_memory_cap():
    """a cap that cuts the 64 candidates into at least three chunks: the same bits; one that leaves no room for a candidate: refused"""
    name = "t9_p130_c8"
    pb, tip_mode, masks, split, cands = t.case(name)
    want = _solved(name)[0]
    with engine_from_problem(pb, rescale=RESCALE_NEVER, tip_mode=tip_mode) as e:
        e.gradient()
        held = e.profile()["device_bytes"]  # (what the engine holds besides the batch scratch)
        assert _same(want, e.placement_optimize(masks, cands, split=split))
        prof = e.placement_optimize_profile()
        scratch = prof["scratch_bytes"]
        assert prof["chunks"] == 1 and scratch > 0
    chunks = 0
    for extra in (0.6, 0.5, 0.4, 0.3, 0.2):  # the largest of these caps that cuts the candidates into three chunks or more
        cap = int(held + extra * scratch)
        with engine_from_problem(pb, rescale=RESCALE_NEVER, tip_mode=tip_mode, max_device_bytes=cap) as e:
            e.gradient()  # (the engine's own buffers are made first: the room is what is left beside them)
            assert e.profile()["tiles"] == 1
            try:
                got = e.placement_optimize(masks, cands, split=split)
            except EngineError as err:
                assert err.code == EUNSUPPORTED and "scratch" in str(err), err
                continue
            prof = e.placement_optimize_profile()
            print(f"cap = held + {extra} x scratch = {cap}: {prof['chunks']} chunks; device_bytes {e.profile()['device_bytes']}")
            assert e.profile()["device_bytes"] <= cap
            assert _same(want, got)
            assert prof["candidates"] == len(cands) and prof["edges"] == pb.N - 1
            if prof["chunks"] >= 3:
                chunks = prof["chunks"]
                break
    assert chunks >= 3, "no cap cut the candidates into three chunks"
    refused = False
    for extra in (0.02, 0.05, 0.1, 0.15):  # the smallest of these caps that holds the engine: none holds the walk's partials beside it
        try:
            e = engine_from_problem(pb, rescale=RESCALE_NEVER, tip_mode=tip_mode, max_device_bytes=int(held + extra * scratch))
        except EngineError:
            continue
        with e:
            if e.profile()["tiles"] != 1:
                continue
            msg = _refused(e, masks, cands, split=split)
            assert "scratch of one candidate" in msg
            _still_usable(e, pb)
            refused = True
            break
    assert refused, "no cap held the engine"


@pytest.mark.parametrize("rescale", [RESCALE_NEVER, RESCALE_AUTO])
def test_underflow_is_reported_in_band(rescale):
    pb = _deep(800, 100, 4, seed=5)
    masks = u.random_masks(np.random.default_rng(1), 3, pb.P)
    nodes = [n for n in (5, 400, pb.T + 300, pb.T + 700) if n != pb.root]
    cands = np.array([(q, n) for q in range(3) for n in nodes], dtype=np.int32)
    with engine_from_problem(pb, rescale=rescale) as e:
        lengths, lnl, lnl0, passes = e.placement_optimize(masks, cands, split=0.4)
        assert not e.rescaling  # never a switch to rescaling
    assert np.all(np.isneginf(lnl)) and np.all(np.isneginf(lnl0)) and np.all(passes == -1)
    assert np.array_equal(_bits(lengths), _bits(_starts(pb, cands, 0.4)))  # the state before the visit that ended the entry


def _refused(e, masks, cands, code=EUNSUPPORTED, **kw):
    with pytest.raises(EngineError) as err:
        e.placement_optimize(masks, cands, **kw)
    assert err.value.code == code, err.value
    print(err.value)
    assert "phyamd_placement_optimize" in str(err.value), err.value
    return str(err.value)


def _still_usable(e, pb):
    ref = pb.log_likelihood()["lnl"]
    assert abs(e.log_likelihood() - ref) <= 1e-10 * abs(ref)


def _queries(pb, Q=2):
    masks = u.random_masks(np.random.default_rng(0), Q, pb.P)
    return masks, np.array([(q, n) for q in range(Q) for n in u.edges(pb)[:4]], dtype=np.int32)


def test_invalid_arguments():
    pb = random_problem(8, 100, 2, seed=3)
    masks, cands = _queries(pb, 3)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        want = e.placement_optimize(masks, cands)
        for node in (pb.root, -1, pb.N, pb.N + 5):
            bad = cands.copy()
            bad[5, 1] = node
            msg = _refused(e, masks, bad, code=EINVAL)
            assert "candidates[5]" in msg and ("root" in msg if node == pb.root else "node is outside" in msg)
        for query in (-1, 3):
            bad = cands.copy()
            bad[2, 0] = query
            msg = _refused(e, masks, bad, code=EINVAL)
            assert "candidates[2]" in msg and "query" in msg
        assert "queries" in _refused(e, masks[:0], cands, code=EINVAL)
        assert "count" in _refused(e, masks, cands[:0], code=EINVAL)
        for branches in (0, 8):
            assert "branches" in _refused(e, masks, cands, code=EINVAL, branches=branches)
        for split in (-1e-9, 1.0 + 1e-9, np.nan, np.inf):
            assert "split" in _refused(e, masks, cands, code=EINVAL, split=split)
        for bad in (0.0, -0.2, np.nan, np.inf):
            start = np.full(len(cands), 0.1)
            start[4] = bad
            assert "pendant_start[4]" in _refused(e, masks, cands, code=EINVAL, pendant_start=start)
        for value in (0, 16, 255):
            wrong = masks.copy()
            wrong[2, 57] = value
            msg = _refused(e, wrong, cands, code=EINVAL)
            assert "query 2" in msg and "pattern 57" in msg and str(value) in msg
        assert "bounds" in _refused(e, masks, cands, code=EINVAL, lower=1.0, upper=0.5)
        assert "tolerance" in _refused(e, masks, cands, code=EINVAL, tolerance=0.0)
        assert "max_iterations" in _refused(e, masks, cands, code=EINVAL, max_iterations=0)
        assert "lnl_tolerance" in _refused(e, masks, cands, code=EINVAL, lnl_tolerance=-1.0)
        assert "max_passes" in _refused(e, masks, cands, code=EINVAL, max_passes=1001)
        lib, out, lnl = e._lib, np.empty((len(cands), 3)), np.empty(len(cands))
        ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        call = lambda m, c, le, ln: lib.phyamd_placement_optimize(e._h, 0, 3, m, len(cands), c, None, 0.5, 7, 1e-8, 10.0, 1e-8, 100, 1e-6, 50, le, ln, None, None)
        for args, word in (((None, ptr(cands), ptr(out), ptr(lnl)), b"null masks"), ((ptr(masks), None, ptr(out), ptr(lnl)), b"null candidates"),
                           ((ptr(masks), ptr(cands), None, ptr(lnl)), b"null lengths"), ((ptr(masks), ptr(cands), ptr(out), None), b"null lnl")):
            assert call(*args) == EINVAL and word in lib.phyamd_last_error()
        with pytest.raises(ValueError):
            e.placement_optimize(masks[:, :-1], cands)
        with pytest.raises(ValueError):
            e.placement_optimize(masks, cands[:, :1])
        with pytest.raises(ValueError):
            e.placement_optimize(masks, cands, np.full(len(cands) + 1, 0.1))
        assert _same(want, e.placement_optimize(masks, cands))
        _still_usable(e, pb)


def test_flags_are_refused():
    pb = random_problem(8, 100, 2, seed=3)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        assert "flags" in _refused(e, *_queries(pb), flags=1)
        _still_usable(e, pb)
        e.placement_optimize(*_queries(pb))


def test_a_missing_eigen_system_is_refused():
    pb = random_problem(8, 100, 2, seed=3)
    with Engine(pb.T, pb.P, 4, pb.C, rescale=RESCALE_NEVER) as e:
        e.set_topology(pb.left, pb.right, pb.root)
        e.set_branch_lengths(pb.branch_lengths)
        e.set_frequencies(pb.freqs)
        e.set_category_rates(pb.cat_rates, pb.cat_props)
        e.set_pattern_weights(pb.weights)
        for tip in range(pb.T):
            e.set_tip_states(tip, pb.tip_states[tip])
        assert "eigen" in _refused(e, *_queries(pb), code=EINVAL)


def test_twenty_states_are_refused():
    pb = random_problem(10, 200, 2, seed=20, S=20, gaps=0.03)
    with engine_from_problem(pb, rescale=RESCALE_AUTO) as e:
        assert "4 states" in _refused(e, *_queries(pb))
        _still_usable(e, pb)


def test_nine_categories_are_refused():
    pb = random_problem(8, 100, 9, seed=9)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        assert "categories" in _refused(e, *_queries(pb))
        _still_usable(e, pb)


def test_a_rescaling_engine_is_refused():
    pb = random_problem(37, 238, 4, seed=12, gaps=0.03, rescale=1)
    with engine_from_problem(pb, rescale=RESCALE_ALWAYS) as e:
        assert "rescal" in _refused(e, *_queries(pb))
        _still_usable(e, pb)


def test_a_tiled_engine_is_refused():
    pb = random_problem(40, 2000, 4, seed=13, gaps=0.03)
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


def test_an_empty_tip_mask_is_refused():
    pb = random_problem(8, 100, 2, seed=23)
    tp = np.zeros((pb.T, pb.P, 4))
    for tip in range(pb.T):
        tp[tip, np.arange(pb.P), pb.tip_states[tip]] = 1.0
    tp[3, 40] = 0.0  # no state is compatible with this cell
    pb.tip_partials, pb.tip_states = tp, None
    with engine_from_problem(pb, rescale=RESCALE_NEVER, tip_mode="partials") as e:
        assert "empty state mask" in _refused(e, *_queries(pb))
        e.log_likelihood()


def test_explicit_matrices_are_refused():
    pb = random_problem(8, 100, 2, seed=3)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        e.gradient()
        e.set_node_matrices(2, e.node_matrices(2))
        assert "explicit matrices" in _refused(e, *_queries(pb))
        _still_usable(e, pb)


def test_a_sharded_handle_is_refused():
    pb = random_problem(8, 200, 2, seed=3)
    with engine_from_problem(pb, rescale=RESCALE_NEVER, devices=[0, 0]) as e:
        assert e.shard_count == 2
        assert "shard" in _refused(e, *_queries(pb))
        _still_usable(e, pb)
