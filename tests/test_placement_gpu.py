"""GPU: phyamd_placement_log_likelihoods -- query sequences scored on every edge of the engine's tree from one walk, one table per
edge and a gather-and-add per (query, edge) -- entry by entry against the CPU oracle's tree with T + 1 tips built from the
definition (tests/placement_util.py), which knows nothing of the shortcut.  The tolerance is the suite's for single evaluations
(tests/test_spr_gpu.py, tests/test_nni_gpu.py): 1e-10 relative on lnL.  Then the best edge, the cross-check with
phyamd_spr_log_likelihoods, bits across calls, query orders, batch sizes and chunks, the engine afterwards, underflow, the same
past the first segment of patterns and the first block of queries, and every refusal."""
import ctypes
import functools

import numpy as np
import pytest

import placement_util as u
from gpu_util import engine_from_problem, random_problem
from periodic_util import periodic_pair
from physher_amd.engine import RESCALE_ALWAYS, RESCALE_AUTO, RESCALE_NEVER, Engine, EngineError
from test_batch_gpu import _ambiguous_partials, _bits, _deep

pytestmark = pytest.mark.gpu
EINVAL, EUNSUPPORTED = -1, -4

# (T, shape, P, C, Q, pendant lengths, sigma, ambiguity codes in the tips): the smallest shapes where the kernels can go wrong --
# no internal edge (T = 2), one (T = 3), a root child that is a tip (caterpillar); less than a block of patterns, exactly one, one
# and a bit, three with a ragged end; one category wave, four and the most; one query and more than a wave of them; fewer pendant
# lengths than category waves, and as many as or more than them (C = 1 with three lengths); both ends of the split
CASES = {
    "t2_p5_c1": (2, "random", 5, 1, 1, (0.13,), 0.5, False),
    "t3_p64_c4": (3, "random", 64, 4, 67, (0.2,), 0.25, False),
    "t9_p130_c8": (9, "random", 130, 8, 67, (0.05, 0.4, 1.7), 0.5, True),
    "t9_caterpillar_p70_c4": (9, "caterpillar", 70, 4, 67, (0.3, 0.01, 0.9), 0.0, False),
    "t9_p70_c1_l3": (9, "random", 70, 1, 1, (0.3, 0.01, 0.9), 1.0, True),
    "t9_p5_c8": (9, "random", 5, 8, 1, (0.11,), 0.25, False),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(problem, tip mode, query masks [Q][P], pendant lengths, sigma, the oracle's [L][Q][N]), computed once"""
    T, shape, P, C, Q, pendant, sigma, ambig = CASES[name]
    pb = random_problem(T, P, C, seed=7 * T + P + C, shape=shape, gaps=0.08)  # (gaps: all-gap cells in the tips)
    assert len(set(pb.weights)) > 1 or P < 3  # weights that are not uniform
    if ambig:
        _ambiguous_partials(pb, 3)
    masks = u.random_masks(np.random.default_rng(P + Q), Q, P, gaps=0.1, ambiguous=0.15)
    if Q > 1:
        masks[1] = 15  # an all-gap query
    ref = u.oracle_all(pb, masks, pendant, sigma)
    ref.setflags(write=False)
    return pb, ("partials" if ambig else "states"), masks, np.array(pendant), sigma, ref


def _check_best(lnl, node, best, root):
    """best_node / best_lnl are the first argmax and the max of the returned lnl over the non-root columns"""
    assert node.dtype == np.int32 and node.shape == best.shape == lnl.shape[:2]
    assert np.all(node != root)
    masked = lnl.copy()
    masked[:, :, root] = -np.inf
    largest = (masked == masked.max(axis=2, keepdims=True)) & (np.arange(lnl.shape[2]) != root)
    first = np.argmax(largest, axis=2)  # (the first True: the smallest node id with the largest lnL)
    assert np.array_equal(node, first), (node, first)
    assert np.array_equal(_bits(best), _bits(np.take_along_axis(lnl, first[:, :, None], axis=2)[:, :, 0]))


@pytest.mark.parametrize("case", sorted(CASES))
def test_every_entry_matches_the_oracle(case):
    pb, tip_mode, masks, pendant, sigma, ref = _case(case)
    with engine_from_problem(pb, rescale=RESCALE_AUTO, tip_mode=tip_mode) as e:
        lnl, node, best = e.placement_log_likelihoods(masks, pendant, split=sigma)
        prof = e.placement_profile()
        assert not e.rescaling
    assert prof["queries"] == len(masks) and prof["lengths"] == len(pendant) and prof["edges"] == pb.N - 1, prof
    assert prof["edge_chunks"] == 1 and prof["query_chunks"] == 1 and prof["scratch_bytes"] > 0, prof
    assert lnl.shape == ref.shape == (len(pendant), len(masks), pb.N)
    assert np.all(np.isnan(lnl[:, :, pb.root])) and np.all(np.isfinite(np.delete(lnl, pb.root, axis=2)))
    err = np.abs(lnl - ref) / np.abs(ref)
    worst = np.nanmax(err)
    print(f"{case}: {np.isfinite(ref).sum()} entries, worst relative lnL error {worst:.3e}")
    assert worst <= 1e-10, np.unravel_index(np.nanargmax(err), err.shape)
    _check_best(lnl, node, best, pb.root)
    if len(masks) > 1:  # the all-gap query scores the base tree's own lnL on every edge
        base = pb.log_likelihood()["lnl"]
        assert np.nanmax(np.abs(lnl[:, 1] - base)) <= 1e-10 * abs(base)


def test_the_best_edge_is_the_oracles_where_it_is_clear():
    """(length, query) pairs whose two largest oracle values differ by more than 1e-8 relative: best_node is the oracle's argmax"""
    kept = 0
    for case in ("t9_p130_c8", "t9_caterpillar_p70_c4", "t3_p64_c4"):
        pb, tip_mode, masks, pendant, sigma, ref = _case(case)
        with engine_from_problem(pb, rescale=RESCALE_AUTO, tip_mode=tip_mode) as e:
            _, node, best = e.placement_log_likelihoods(masks, pendant, split=sigma, want_lnl=False)
        filled = np.where(np.isnan(ref), -np.inf, ref)
        order = np.sort(filled, axis=2)
        clear = (order[:, :, -1] - order[:, :, -2]) > 1e-8 * np.abs(order[:, :, -1])
        kept += int(clear.sum())
        assert np.array_equal(node[clear], np.argmax(filled, axis=2)[clear])
        assert np.all(np.abs(best[clear] - order[:, :, -1][clear]) <= 1e-10 * np.abs(order[:, :, -1][clear]))
    print(f"{kept} clear (length, query) pairs")
    assert kept >= 1


def test_agrees_with_the_spr_call_on_the_tree_that_holds_the_query():
    """a tip x of a 10-taxon tree pruned as SPR_move prunes it; x placed on the 9-taxon base tree with split 0.5 and pendant t_x is
    row x of spr_log_likelihoods on the 10-taxon engine, column by column (placement_util.pruned_base holds the id mapping)"""
    pb = random_problem(10, 130, 4, seed=41, gaps=0.05)
    parent = u.parents(pb)
    x = next(t for t in range(pb.T) if parent[t] != pb.root and parent[parent[t]] != pb.root)
    base, new_id, row, tx = u.pruned_base(pb, x)
    with engine_from_problem(pb, rescale=RESCALE_AUTO) as e:
        spr = e.spr_log_likelihoods([x])[0]
    with engine_from_problem(base, rescale=RESCALE_AUTO, tip_mode="partials") as e:
        lnl, _, _ = e.placement_log_likelihoods(row[None, :], [tx], split=0.5)
    targets = np.nonzero(np.isfinite(spr))[0]
    assert len(targets) == pb.N - 4 and np.all(new_id[targets] >= 0)  # all but the root, x, its parent and its sibling
    got = lnl[0, 0, new_id[targets]]
    err = np.abs(got - spr[targets]) / np.abs(spr[targets])
    print(f"{len(targets)} targets: worst relative difference {err.max():.3e}")
    assert np.all(err <= 1e-10)


def test_bits_do_not_depend_on_the_call_the_order_or_the_batch():
    pb, tip_mode, masks, pendant, sigma, _ = _case("t9_p130_c8")
    with engine_from_problem(pb, rescale=RESCALE_AUTO, tip_mode=tip_mode) as e:
        before = (e.log_likelihood(), e.gradient())
        first = e.placement_log_likelihoods(masks, pendant, split=sigma)
        second = e.placement_log_likelihoods(masks, pendant, split=sigma)
        for a, b in zip(first, second):
            assert np.array_equal(_bits(a) if a.dtype == np.float64 else a, _bits(b) if b.dtype == np.float64 else b)
        e.nni_log_likelihoods()  # (another call in the same scratch)
        perm = np.random.default_rng(9).permutation(len(masks))
        shuffled = e.placement_log_likelihoods(masks[perm], pendant, split=sigma)
        assert np.array_equal(_bits(shuffled[0]), _bits(first[0][:, perm])) and np.array_equal(shuffled[1], first[1][:, perm])
        assert np.array_equal(_bits(shuffled[2]), _bits(first[2][:, perm]))
        for q in range(len(masks)):  # 67 queries as 67 calls
            one = e.placement_log_likelihoods(masks[q:q + 1], pendant, split=sigma)
            assert np.array_equal(_bits(one[0][:, 0]), _bits(first[0][:, q])) and np.array_equal(one[1][:, 0], first[1][:, q]), q
            assert np.array_equal(_bits(one[2][:, 0]), _bits(first[2][:, q]))
        single = e.placement_log_likelihoods(masks, pendant[1:2], split=sigma)  # a length alone
        assert np.array_equal(_bits(single[0][0]), _bits(first[0][1]))
        none, node, best = e.placement_log_likelihoods(masks, pendant, split=sigma, want_lnl=False)
        assert none is None and np.array_equal(node, first[1]) and np.array_equal(_bits(best), _bits(first[2]))
        lnl, nobody, nothing = e.placement_log_likelihoods(masks, pendant, split=sigma, want_best=False)
        assert nobody is None and nothing is None and np.array_equal(_bits(lnl), _bits(first[0]))
        after = (e.log_likelihood(), e.gradient())
        assert _bits(before[0]) == _bits(after[0])
        assert _bits(before[1][0]) == _bits(after[1][0]) and np.array_equal(_bits(before[1][1]), _bits(after[1][1]))
        assert not e.rescaling
    with engine_from_problem(pb, rescale=RESCALE_AUTO, tip_mode=tip_mode) as e:  # a scratch that held nothing before
        assert np.array_equal(_bits(first[0]), _bits(e.placement_log_likelihoods(masks, pendant, split=sigma)[0]))


def test_under_a_memory_cap():
    """a cap that cuts the edges into at least two chunks and the 67 queries into at least two: the same bits"""
    pb, tip_mode, masks, pendant, sigma, _ = _case("t9_p130_c8")
    with engine_from_problem(pb, rescale=RESCALE_NEVER, tip_mode=tip_mode) as e:
        e.gradient()
        held = e.profile()["device_bytes"]  # (what the engine holds besides the batch scratch)
        want = e.placement_log_likelihoods(masks, pendant, split=sigma)
        prof = e.placement_profile()
        scratch = prof["scratch_bytes"]
        assert prof["edge_chunks"] == 1 and prof["query_chunks"] == 1 and scratch > 0
    found = None
    for extra in (0.7, 0.6, 0.5, 0.4, 0.3, 0.2, 0.1):  # the largest of these caps that cuts both axes
        cap = int(held + extra * scratch)
        with engine_from_problem(pb, rescale=RESCALE_NEVER, tip_mode=tip_mode, max_device_bytes=cap) as e:
            e.gradient()  # (the engine's own buffers are made first: the room is what is left beside them)
            assert e.profile()["tiles"] == 1
            try:
                got = e.placement_log_likelihoods(masks, pendant, split=sigma)
            except EngineError as err:
                assert err.code == EUNSUPPORTED and "scratch" in str(err), err
                continue
            prof = e.placement_profile()
            print(f"cap = held + {extra} x scratch = {cap}: {prof['edge_chunks']} edge chunks x {prof['query_chunks']} query chunks")
            assert e.profile()["device_bytes"] <= cap
            for a, b in zip(got, want):
                assert np.array_equal(_bits(a) if a.dtype == np.float64 else a, _bits(b) if b.dtype == np.float64 else b)
            best_only = e.placement_log_likelihoods(masks, pendant, split=sigma, want_lnl=False)
            assert np.array_equal(best_only[1], want[1]) and np.array_equal(_bits(best_only[2]), _bits(want[2]))
            if prof["edge_chunks"] >= 2 and prof["query_chunks"] >= 2:
                found = prof
                break
    assert found is not None, "no cap cut both the edges and the queries"
    refused = False
    for extra in (0.05, 0.1, 0.15, 0.2, 0.25):  # the smallest of these caps that holds the engine: none holds the walk's partials (8 C planes of 16 nodes, over 0.25 of the scratch) beside it
        try:
            e = engine_from_problem(pb, rescale=RESCALE_NEVER, tip_mode=tip_mode, max_device_bytes=int(held + extra * scratch))
        except EngineError:
            continue
        with e:
            if e.profile()["tiles"] != 1:
                continue
            with pytest.raises(EngineError) as err:
                e.placement_log_likelihoods(masks, pendant, split=sigma)
            print(err.value)
            assert err.value.code == EUNSUPPORTED and "scratch" in str(err.value)
            _still_usable(e, pb)
            refused = True
            break
    assert refused, "no cap held the engine"


@pytest.mark.parametrize("rescale", [RESCALE_NEVER, RESCALE_AUTO])
def test_underflow_is_reported_in_band(rescale):
    pb = _deep(800, 100, 4, seed=5)
    masks = u.random_masks(np.random.default_rng(1), 3, pb.P)
    with engine_from_problem(pb, rescale=rescale) as e:
        lnl, node, best = e.placement_log_likelihoods(masks, [0.1, 0.5])
        assert not e.rescaling  # never a switch to rescaling
    assert np.all(np.isnan(lnl[:, :, pb.root])) and np.all(np.isneginf(np.delete(lnl, pb.root, axis=2)))
    assert np.all(np.isneginf(best)) and np.all(node == (1 if pb.root == 0 else 0))


# ---- past the first segment of patterns and the first block of queries ------------------------------------------------------------
#
# k_place_score4 adds a fixed segment of 4096 patterns (REWEIGHT_SEGMENT) per workgroup and takes at most 1024 queries
# (PLACE_MAX_QUERIES) as lanes; k_place_finish adds a column's segments and takes 256 (length, query) threads per block.  4096 + 70
# patterns are two segments, the second ragged (66 blocks of 64, the last ragged); 1100 queries are two blocks of lanes, the second
# with 76 live ones; 2 x 1100 (length, query) threads are nine blocks of the finish.  The scratch is padded to whole blocks, so a
# wrong offset reads valid memory and returns a plausible lnL: only a reference shows it.

P_SEGMENTS = 4096 + 70
Q_BLOCKS, Q_DISTINCT = 1100, 24
SEGMENT_PENDANT, SEGMENT_SPLIT = (0.05, 0.4), 0.3


@functools.lru_cache(maxsize=None)
def _segment_case(ambig):
    """(problem, tip mode, the 24 distinct query rows, row [1100]: which of them query q is, the oracle's [2][24][N]): the oracle
    runs the distinct rows only; the 1100 queries are the 24 tiled and then shuffled"""
    T, C = 5, 2
    pb = random_problem(T, P_SEGMENTS, C, seed=7 * T + P_SEGMENTS + C, gaps=0.08)
    if ambig:
        _ambiguous_partials(pb, 3)
    distinct = u.random_masks(np.random.default_rng(P_SEGMENTS + Q_BLOCKS), Q_DISTINCT, P_SEGMENTS, gaps=0.1, ambiguous=0.15)
    distinct[1] = 15  # an all-gap query
    row = np.random.default_rng(17).permutation(np.arange(Q_BLOCKS) % Q_DISTINCT)
    ref = u.oracle_all(pb, distinct, SEGMENT_PENDANT, SEGMENT_SPLIT)
    for a in (distinct, row, ref):
        a.setflags(write=False)
    return pb, ("partials" if ambig else "states"), distinct, row, ref


def _reached_two_segments_and_two_query_blocks(e, masks):
    """FAILS where the case no longer crosses the boundaries it is there for.  The call's profile does not report its segments; a
    counts-only pairwise_distances call on the same engine does, and both are computed from the same constant, REWEIGHT_SEGMENT
    (phyamd_reweight.inc): a later change of the constant shows here and not as a test that quietly covers less"""
    assert len(masks) > 1024, f"{len(masks)} queries are one block of k_place_score4's lanes (PLACE_MAX_QUERIES = 1024)"
    e.pairwise_distances([[0, 1]], counts_only=True)
    segments = e.distance_profile()["segments"]
    assert segments >= 2, f"{e.P} patterns are {segments} segment(s) of REWEIGHT_SEGMENT patterns: the pattern count of this case is too small"


def _same_outputs(got, want):
    return all(np.array_equal(_bits(a) if a.dtype == np.float64 else a, _bits(b) if b.dtype == np.float64 else b) for a, b in zip(got, want))


@pytest.mark.parametrize("ambig", [True, False], ids=["ambiguous", "states"])
def test_two_segments_and_two_query_blocks_match_the_oracle(ambig):
    pb, tip_mode, distinct, row, ref = _segment_case(ambig)
    masks = distinct[row]
    assert masks.shape == (Q_BLOCKS, P_SEGMENTS) and len(SEGMENT_PENDANT) * Q_BLOCKS > 8 * 256  # nine blocks of k_place_finish
    assert np.array_equal(np.bincount(row, minlength=Q_DISTINCT) > 0, np.ones(Q_DISTINCT, dtype=bool))
    with engine_from_problem(pb, rescale=RESCALE_AUTO, tip_mode=tip_mode) as e:
        lnl, node, best = e.placement_log_likelihoods(masks, SEGMENT_PENDANT, split=SEGMENT_SPLIT)
        prof = e.placement_profile()
        assert not e.rescaling
        _reached_two_segments_and_two_query_blocks(e, masks)
    assert prof["queries"] == Q_BLOCKS and prof["lengths"] == 2 and prof["edges"] == pb.N - 1, prof
    assert prof["edge_chunks"] == 1 and prof["query_chunks"] == 1, prof
    assert lnl.shape == (2, Q_BLOCKS, pb.N)
    assert np.all(np.isnan(lnl[:, :, pb.root])) and np.all(np.isfinite(np.delete(lnl, pb.root, axis=2)))
    want = ref[:, row]
    err = np.abs(lnl - want) / np.abs(want)
    worst = np.nanmax(err)
    print(f"{'ambiguous' if ambig else 'states'}: {np.isfinite(want).sum()} entries, worst relative lnL error {worst:.3e} ({worst / 1e-10:.2e} of the tolerance)")
    assert worst <= 1e-10, np.unravel_index(np.nanargmax(err), err.shape)
    for r in range(Q_DISTINCT):  # copies of one row, wherever they stand: the same bits
        at = np.nonzero(row == r)[0]
        assert len(at) >= 2
        assert np.all(_bits(np.delete(lnl[:, at], pb.root, axis=2)) == _bits(np.delete(lnl[:, at[:1]], pb.root, axis=2))), r
        assert np.all(node[:, at] == node[:, at[:1]]) and np.all(_bits(best[:, at]) == _bits(best[:, at[:1]])), r
    _check_best(lnl, node, best, pb.root)
    base = pb.log_likelihood()["lnl"]  # the all-gap row scores the base tree's own lnL on every edge
    assert np.nanmax(np.abs(lnl[:, row == 1] - base)) <= 1e-10 * abs(base)


def test_two_segments_and_two_query_blocks_under_a_memory_cap():
    """the largest cap of the ladder that cuts the edges into at least two chunks and the 1100 queries into at least two, so that a
    chunk's slab holds two segments and the best edge so far is resumed across edge chunks at every query chunk's offset: the same
    bits as the uncapped call, with and without the lnL rows"""
    pb, tip_mode, distinct, row, _ = _segment_case(True)
    masks = distinct[row]
    with engine_from_problem(pb, rescale=RESCALE_NEVER, tip_mode=tip_mode) as e:
        e.gradient()
        held = e.profile()["device_bytes"]  # (what the engine holds besides the batch scratch)
        want = e.placement_log_likelihoods(masks, SEGMENT_PENDANT, split=SEGMENT_SPLIT)
        prof = e.placement_profile()
        scratch = prof["scratch_bytes"]
        assert prof["edge_chunks"] == 1 and prof["query_chunks"] == 1 and scratch > 0
        _reached_two_segments_and_two_query_blocks(e, masks)
    found = None
    for extra in (0.7, 0.6, 0.5, 0.4, 0.3, 0.2, 0.1):  # (test_under_a_memory_cap's ladder)
        cap = int(held + extra * scratch)
        with engine_from_problem(pb, rescale=RESCALE_NEVER, tip_mode=tip_mode, max_device_bytes=cap) as e:
            e.gradient()  # (the engine's own buffers are made first: the room is what is left beside them)
            assert e.profile()["tiles"] == 1
            try:
                got = e.placement_log_likelihoods(masks, SEGMENT_PENDANT, split=SEGMENT_SPLIT)
            except EngineError as err:
                assert err.code == EUNSUPPORTED and "scratch" in str(err), err
                continue
            prof = e.placement_profile()
            print(f"cap = held + {extra} x scratch = {cap}: {prof['edge_chunks']} edge chunks x {prof['query_chunks']} query chunks")
            assert e.profile()["device_bytes"] <= cap
            assert _same_outputs(got, want)
            best_only = e.placement_log_likelihoods(masks, SEGMENT_PENDANT, split=SEGMENT_SPLIT, want_lnl=False)
            assert best_only[0] is None and _same_outputs(best_only[1:], want[1:])
            if prof["edge_chunks"] >= 2 and prof["query_chunks"] >= 2:
                found = prof
                break
    assert found is not None, "no cap cut both the edges and the queries"


@pytest.mark.parametrize("rescale", [RESCALE_NEVER, RESCALE_AUTO])
def test_underflow_is_reported_in_band_across_two_segments(rescale):
    """test_underflow_is_reported_in_band's 100 columns repeated over 4096 + 70 patterns: every segment sum is -inf"""
    pb = periodic_pair(_deep(800, 100, 4, seed=5), P_SEGMENTS, seed=5)[0]
    masks = u.random_masks(np.random.default_rng(1), 3, pb.P)
    with engine_from_problem(pb, rescale=rescale) as e:
        lnl, node, best = e.placement_log_likelihoods(masks, [0.1, 0.5])
        assert not e.rescaling  # never a switch to rescaling
        e.pairwise_distances([[0, 1]], counts_only=True)
        assert e.distance_profile()["segments"] >= 2  # (the same REWEIGHT_SEGMENT: see _reached_two_segments_and_two_query_blocks)
    assert np.all(np.isnan(lnl[:, :, pb.root])) and np.all(np.isneginf(np.delete(lnl, pb.root, axis=2)))
    assert np.all(np.isneginf(best)) and np.all(node == (1 if pb.root == 0 else 0))


def _refused(e, masks, pendant, code=EUNSUPPORTED, **kw):
    with pytest.raises(EngineError) as err:
        e.placement_log_likelihoods(masks, pendant, **kw)
    assert err.value.code == code, err.value
    print(err.value)
    assert "phyamd_placement_log_likelihoods" in str(err.value) or code == EINVAL
    return str(err.value)


def _still_usable(e, pb):
    ref = pb.log_likelihood()["lnl"]
    assert abs(e.log_likelihood() - ref) <= 1e-10 * abs(ref)


def _queries(pb, Q=2):
    return u.random_masks(np.random.default_rng(0), Q, pb.P), [0.1]


def test_invalid_arguments():
    pb = random_problem(8, 100, 2, seed=3)
    masks, pendant = _queries(pb, 3)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        want = e.placement_log_likelihoods(masks, pendant)
        assert "null lnl" in _refused(e, masks, pendant, code=EINVAL, want_lnl=False, want_best=False)
        assert "queries" in _refused(e, masks[:0], pendant, code=EINVAL)
        assert "lengths" in _refused(e, masks, [], code=EINVAL)
        for split in (-1e-9, 1.0 + 1e-9, np.nan, np.inf):
            assert "split" in _refused(e, masks, pendant, code=EINVAL, split=split)
        for bad in (0.0, -0.2, np.nan, np.inf):
            assert "pendant[1]" in _refused(e, masks, [0.1, bad], code=EINVAL)
        for value in (0, 16, 255):
            wrong = masks.copy()
            wrong[2, 57] = value
            msg = _refused(e, wrong, pendant, code=EINVAL)
            assert "query 2" in msg and "pattern 57" in msg and str(value) in msg
        lib, out = e._lib, np.empty((1, 3, pb.N))
        ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        pd = np.array(pendant)
        assert lib.phyamd_placement_log_likelihoods(e._h, 0, 3, None, 1, ptr(pd), 0.5, ptr(out), None, None) == EINVAL
        assert b"null masks" in lib.phyamd_last_error()
        assert lib.phyamd_placement_log_likelihoods(e._h, 0, 3, ptr(masks), 1, None, 0.5, ptr(out), None, None) == EINVAL
        assert b"null pendant" in lib.phyamd_last_error()
        assert lib.phyamd_placement_log_likelihoods(e._h, 0, 3, ptr(masks), 1, ptr(pd), 0.5, ptr(out), None, ptr(np.empty((1, 3)))) == EINVAL
        assert b"best_lnl without best_node" in lib.phyamd_last_error()
        with pytest.raises(ValueError):
            e.placement_log_likelihoods(masks[:, :-1], pendant)
        again = e.placement_log_likelihoods(masks, pendant)
        assert np.array_equal(_bits(want[0]), _bits(again[0]))
        _still_usable(e, pb)


def test_flags_are_refused():
    pb = random_problem(8, 100, 2, seed=3)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        assert "flags" in _refused(e, *_queries(pb), flags=1)
        _still_usable(e, pb)
        e.placement_log_likelihoods(*_queries(pb))


def test_a_missing_eigen_system_is_refused():
    pb = random_problem(8, 100, 2, seed=3)
    with Engine(pb.T, pb.P, 4, pb.C, rescale=RESCALE_NEVER) as e:
        e.set_topology(pb.left, pb.right, pb.root)
        e.set_branch_lengths(pb.branch_lengths)
        e.set_frequencies(pb.freqs)
        e.set_category_rates(pb.cat_rates, pb.cat_props)
        e.set_pattern_weights(pb.weights)
        for t in range(pb.T):
            e.set_tip_states(t, pb.tip_states[t])
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
    for t in range(pb.T):
        tp[t, np.arange(pb.P), pb.tip_states[t]] = 1.0
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
