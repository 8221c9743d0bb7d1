"""GPU: phyamd_placement_log_likelihoods_general -- query sequences of a 20-state engine scored on every edge of its tree from the
resident partials, one table of 32 classes per edge and a gather-and-add per (query, edge) -- entry by entry against the CPU
oracle's tree with T + 1 tips built from the definition (tests/placement_general_util.py), which knows nothing of the shortcut.
The tolerance is the suite's for single evaluations (tests/test_placement_gpu.py, tests/test_general_tiles_gpu.py): 1e-10 relative
on lnL.  Then the best edge, bits across calls, query orders, batch sizes and chunks, the same past the first segment of patterns
and the first block of queries, underflow, the engine afterwards, and every refusal."""
import copy
import ctypes
import functools

import numpy as np
import pytest

import pair_distance_general_util as gu
import placement_general_util as u
from gpu_util import engine_from_problem, random_problem
from physher_amd.engine import RESCALE_ALWAYS, RESCALE_AUTO, RESCALE_NEVER, Engine, EngineError
from test_batch_gpu import _bits, _deep

pytestmark = pytest.mark.gpu
EINVAL, EUNSUPPORTED = -1, -4
NAME = "phyamd_placement_log_likelihoods_general"

# (T, shape, P, C, Q, pendant lengths, sigma, engine sets in the reference tips, sets of the call): the smallest shapes where the
# kernels can go wrong -- no internal edge (T = 2), one (T = 3), a root child that is a tip (caterpillar); less than one 16-pattern
# tile, exactly one, a workgroup's 128 patterns and a bit, four tiles and a ragged fifth; one category, four and the most; one
# query and more than a wave of them; one pendant length and three; both ends of the split and two inner values; reference tips
# from states and from ambiguous partials; queries without sets, with a few and with all eleven
CASES = {
    "t2_p5_c1": (2, "random", 5, 1, 1, (0.13,), 0.5, 0, 0),
    "t3_p16_c4": (3, "random", 16, 4, 67, (0.2,), 0.25, 0, 3),
    "t9_p130_c8_all_sets": (9, "random", 130, 8, 8, (0.05, 0.4, 1.7), 0.5, 3, 11),
    "t9_caterpillar_p70_c4": (9, "caterpillar", 70, 4, 67, (0.3, 0.01), 0.0, 0, 2),
    "t9_p70_c1_l3": (9, "random", 70, 1, 1, (0.3, 0.01, 0.9), 1.0, 3, 3),
    "t9_p5_c8": (9, "random", 5, 8, 1, (0.11,), 0.25, 0, 0),
}


def _build(T, shape, P, C, Q, tip_sets, set_count, seed):
    pb = random_problem(T, P, C, seed=seed, S=20, shape=shape, gaps=0.08)  # (gaps: unknown cells in the tips)
    if tip_sets:
        gu.with_sets(pb, tip_sets, 0.1, seed + 1)
    rng = np.random.default_rng(P + Q)
    sets = u.random_sets(rng, set_count)
    codes = u.random_codes(rng, Q, P, set_count, unknown=0.1, in_sets=0.2)
    if Q > 1:
        codes[1] = u.UNKNOWN  # an all-unknown query
    return pb, ("partials" if tip_sets else "states"), codes, sets


@functools.lru_cache(maxsize=None)
def _case(name):
    """(problem, tip mode, query codes [Q][P], the call's sets, pendant lengths, sigma, the oracle's [L][Q][N]), computed once"""
    T, shape, P, C, Q, pendant, sigma, tip_sets, set_count = CASES[name]
    pb, tip_mode, codes, sets = _build(T, shape, P, C, Q, tip_sets, set_count, 7 * T + P + C)
    assert len(set(pb.weights)) > 1 or P < 3  # weights that are not uniform
    if set_count == u.MAX_SETS:
        assert set(codes.ravel().tolist()) == set(range(32))  # every class: both row tiles of the class image in full
    ref = u.oracle_all(pb, codes, sets, pendant, sigma)
    for a in (codes, sets, ref):
        a.setflags(write=False)
    return pb, tip_mode, codes, sets, np.array(pendant), sigma, ref


@functools.lru_cache(maxsize=None)
def _wide():
    """the problem of t9_p130_c8_all_sets with 67 queries, for the tests that compare bits and need no oracle"""
    T, shape, P, C, _, pendant, sigma, tip_sets, set_count = CASES["t9_p130_c8_all_sets"]
    pb, tip_mode, codes, sets = _build(T, shape, P, C, 67, tip_sets, set_count, 7 * T + P + C)
    for a in (codes, sets):
        a.setflags(write=False)
    return pb, tip_mode, codes, sets, np.array(pendant), sigma, None


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


def _same_outputs(got, want):
    return all((a is None and b is None) or np.array_equal(_bits(a) if a.dtype == np.float64 else a, _bits(b) if b.dtype == np.float64 else b)
               for a, b in zip(got, want))


@pytest.mark.parametrize("case", sorted(CASES))
def test_every_entry_matches_the_oracle(case):
    pb, tip_mode, codes, sets, pendant, sigma, ref = _case(case)
    with engine_from_problem(pb, rescale=RESCALE_AUTO, tip_mode=tip_mode) as e:
        lnl, node, best = e.placement_log_likelihoods_general(codes, pendant, split=sigma, sets=sets)
        prof = e.placement_profile()
        assert not e.rescaling
    assert prof["queries"] == len(codes) and prof["lengths"] == len(pendant) and prof["edges"] == pb.N - 1, prof
    assert prof["edge_chunks"] == 1 and prof["query_chunks"] == 1 and prof["scratch_bytes"] > 0, prof
    assert lnl.shape == ref.shape == (len(pendant), len(codes), pb.N)
    assert np.all(np.isnan(lnl[:, :, pb.root])) and np.all(np.isfinite(np.delete(lnl, pb.root, axis=2)))
    err = np.abs(lnl - ref) / np.abs(ref)
    worst = np.nanmax(err)
    print(f"{case}: {np.isfinite(ref).sum()} entries, worst relative lnL error {worst:.3e}")
    assert worst <= 1e-10, np.unravel_index(np.nanargmax(err), err.shape)
    _check_best(lnl, node, best, pb.root)
    if len(codes) > 1:  # the all-unknown query scores the base tree's own lnL on every edge
        base = pb.log_likelihood()["lnl"]
        assert np.nanmax(np.abs(lnl[:, 1] - base)) <= 1e-10 * abs(base)


def test_the_best_edge_is_the_oracles_where_it_is_clear():
    """(length, query) pairs whose two largest oracle values differ by more than 1e-8 relative: best_node is the oracle's argmax"""
    kept = 0
    for case in ("t9_p130_c8_all_sets", "t9_caterpillar_p70_c4", "t3_p16_c4"):
        pb, tip_mode, codes, sets, pendant, sigma, ref = _case(case)
        with engine_from_problem(pb, rescale=RESCALE_AUTO, tip_mode=tip_mode) as e:
            none, node, best = e.placement_log_likelihoods_general(codes, pendant, split=sigma, sets=sets, want_lnl=False)
        assert none is None
        filled = np.where(np.isnan(ref), -np.inf, ref)
        order = np.sort(filled, axis=2)
        clear = (order[:, :, -1] - order[:, :, -2]) > 1e-8 * np.abs(order[:, :, -1])
        kept += int(clear.sum())
        assert np.array_equal(node[clear], np.argmax(filled, axis=2)[clear])
        assert np.all(np.abs(best[clear] - order[:, :, -1][clear]) <= 1e-10 * np.abs(order[:, :, -1][clear]))
    print(f"{kept} clear (length, query) pairs")
    assert kept >= 1


def test_bits_do_not_depend_on_the_call_the_order_or_the_batch():
    pb, tip_mode, codes, sets, pendant, sigma, _ = _wide()
    call = lambda e, c, p=pendant, **kw: e.placement_log_likelihoods_general(c, p, split=sigma, sets=sets, **kw)
    with engine_from_problem(pb, rescale=RESCALE_AUTO, tip_mode=tip_mode) as e:
        first = call(e, codes)
        assert _same_outputs(call(e, codes), first)
        e.pairwise_distances_general(counts_only=True, want_counts=True)  # (another call in the same scratch)
        perm = np.random.default_rng(9).permutation(len(codes))
        shuffled = call(e, codes[perm])
        assert _same_outputs(shuffled, (first[0][:, perm], first[1][:, perm], first[2][:, perm]))
        for q in range(0, len(codes), 6):  # a query alone
            one = call(e, codes[q:q + 1])
            assert _same_outputs(one, (first[0][:, q:q + 1], first[1][:, q:q + 1], first[2][:, q:q + 1])), q
        single = call(e, codes, pendant[1:2])  # a length alone
        assert np.array_equal(_bits(single[0][0]), _bits(first[0][1]))
        none, node, best = call(e, codes, want_lnl=False)
        assert none is None and np.array_equal(node, first[1]) and np.array_equal(_bits(best), _bits(first[2]))
        lnl, nobody, nothing = call(e, codes, want_best=False)
        assert nobody is None and nothing is None and np.array_equal(_bits(lnl), _bits(first[0]))
        assert not e.rescaling
    with engine_from_problem(pb, rescale=RESCALE_AUTO, tip_mode=tip_mode) as e:  # a scratch that held nothing before
        assert _same_outputs(call(e, codes), first)


def _capped(pb, tip_mode, call, want, held, scratch):
    """the largest cap of the ladder that cuts the edges into at least two chunks and the queries into at least two: the same bits,
    with and without the lnL rows"""
    found = None
    for extra in (0.7, 0.6, 0.5, 0.4, 0.3, 0.2, 0.1, 0.05):
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
            prof = e.placement_profile()
            print(f"cap = held + {extra} x scratch = {cap}: {prof['edge_chunks']} edge chunks x {prof['query_chunks']} query chunks")
            assert e.profile()["device_bytes"] <= cap
            assert _same_outputs(got, want)
            best_only = call(e, want_lnl=False)
            assert best_only[0] is None and _same_outputs(best_only[1:], want[1:])
            if prof["edge_chunks"] >= 2 and prof["query_chunks"] >= 2:
                found = prof
                break
    assert found is not None, "no cap cut both the edges and the queries"


def _uncapped(pb, tip_mode, call):
    with engine_from_problem(pb, rescale=RESCALE_NEVER, tip_mode=tip_mode) as e:
        e.set_keep_partials(True)
        e.gradient()
        held = e.profile()["device_bytes"]  # (what the engine holds besides the batch scratch)
        want = call(e)
        prof = e.placement_profile()
        assert prof["edge_chunks"] == 1 and prof["query_chunks"] == 1 and prof["scratch_bytes"] > 0
    return want, held, prof["scratch_bytes"]


def test_under_a_memory_cap():
    pb, tip_mode, codes, sets, pendant, sigma, _ = _wide()
    call = lambda e, **kw: e.placement_log_likelihoods_general(codes, pendant, split=sigma, sets=sets, **kw)
    want, held, scratch = _uncapped(pb, tip_mode, call)
    _capped(pb, tip_mode, call, want, held, scratch)
    refused = False
    for extra in (0.001, 0.005, 0.01, 0.02, 0.05):  # the smallest of these caps that holds the engine: not the matrices and images beside it
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
            with pytest.raises(EngineError) as err:
                call(e)
            print(err.value)
            assert err.value.code == EUNSUPPORTED and "scratch" in str(err.value) and NAME in str(err.value)
            _still_usable(e, pb)
            refused = True
            break
    assert refused, "no cap held the engine"


# ---- past the first segment of patterns and the first block of queries ------------------------------------------------------------

P_SEGMENTS = 4096 + 70


@functools.lru_cache(maxsize=None)
def _segment_case():
    """T = 3, 4096 + 70 patterns, 67 queries: two segments of the gather, the second ragged, and two blocks of the finish"""
    pb, tip_mode, codes, sets = _build(3, "random", P_SEGMENTS, 2, 67, 2, 4, 7 * 3 + P_SEGMENTS + 2)
    pendant, sigma = (0.4,), 0.3
    ref = u.oracle_all(pb, codes, sets, pendant, sigma)
    for a in (codes, sets, ref):
        a.setflags(write=False)
    return pb, tip_mode, codes, sets, np.array(pendant), sigma, ref


def test_two_segments_match_the_oracle_and_keep_their_bits_under_a_cap():
    pb, tip_mode, codes, sets, pendant, sigma, ref = _segment_case()
    assert pb.P > gu.SEGMENT and len(codes) > 64
    call = lambda e, **kw: e.placement_log_likelihoods_general(codes, pendant, split=sigma, sets=sets, **kw)
    want, held, scratch = _uncapped(pb, tip_mode, call)
    lnl, node, best = want
    err = np.abs(lnl - ref) / np.abs(ref)
    worst = np.nanmax(err)
    print(f"{np.isfinite(ref).sum()} entries, worst relative lnL error {worst:.3e}")
    assert worst <= 1e-10, np.unravel_index(np.nanargmax(err), err.shape)
    _check_best(lnl, node, best, pb.root)
    base = pb.log_likelihood()["lnl"]
    assert np.nanmax(np.abs(lnl[:, 1] - base)) <= 1e-10 * abs(base)
    _capped(pb, tip_mode, call, want, held, scratch)


# ---- underflow --------------------------------------------------------------------------------------------------------------------

def underflow_case():
    """A caterpillar deep enough that one pattern's site likelihood is a subnormal number while the base evaluation stays finite
    (placement_general_util's restatement picks the depth on the CPU).  With split 0 and a pendant length of 1e-20 both P_lo and
    P(l r_c) are the identity up to rounding (off-diagonal entries below 1e-15), so on a TIP edge whose cell at that pattern is the
    single state a, a query cell of another single state j selects a site likelihood below 1e-15 of a subnormal number: exactly 0,
    whatever the order of the additions.  Returns (problem, codes [3][P], pattern, the tip edges that must be -inf for query 0):
    query 0 holds j at that pattern, query 1 is all unknown, query 2 is query 0 with the cell unknown."""
    for T in range(220, 260):
        pb = _deep(T, 6, 2, seed=11, S=20)
        r = pb.log_likelihood()
        site = np.asarray(r["pattern_lk"]) / np.log(10.0)  # log10 site likelihoods (the oracle rescales: exact past the underflow)
        k = int(np.argmin(site))
        if -316.0 < site[k] < -310.0 and np.all(np.delete(site, k) > site[k] + 1.0):  # the others: larger, finite for an unknown cell
            codes = np.full((3, pb.P), u.UNKNOWN, dtype=np.uint8)
            tips = [t for t in range(pb.T) if pb.tip_states[t, k] < 20 and t != pb.root]
            j = int(np.bincount(pb.tip_states[tips, k], minlength=20).argmin())
            codes[0, k] = j
            return pb, codes, k, [t for t in tips if pb.tip_states[t, k] != j]
    raise AssertionError("no depth puts a pattern's site likelihood between 1e-316 and 1e-310")


def test_underflow_is_in_band_and_reaches_only_the_queries_that_select_it():
    pb, codes, k, dead = underflow_case()
    assert len(dead) >= 1
    plain = copy.copy(pb)
    plain.rescale = 0  # the restatement on partials that are not rescaled, like the engine's: what it predicts, on the CPU
    assert np.isfinite(plain.log_likelihood()["lnl"])
    F = u.class_likelihoods(plain, [], [1e-20], 0.0)[0][:, k]  # [N][32] at the pattern
    assert np.all(F[dead, codes[0, k]] == 0.0) and np.all(np.delete(F[:, u.UNKNOWN], pb.root) > 1e-318)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        assert np.isfinite(e.log_likelihood())
        lnl, node, best = e.placement_log_likelihoods_general(codes, [1e-20], split=0.0)
        assert not e.rescaling
    assert np.all(np.isnan(lnl[:, :, pb.root]))
    assert np.all(np.isneginf(lnl[0, 0, dead])), lnl[0, 0, dead]
    others = np.delete(lnl[0, 1:], pb.root, axis=1)
    assert np.all(np.isfinite(others)), "a query that does not select the underflowed entries stays finite"
    assert np.array_equal(_bits(lnl[0, 1]), _bits(lnl[0, 2]))
    assert np.all(np.isfinite(best[0, 1:]))
    _check_best(lnl, node, best, pb.root)


# ---- the engine afterwards --------------------------------------------------------------------------------------------------------

def test_the_engine_afterwards_is_a_keep_partials_engine_with_the_same_bits():
    """the engine after the call against a fresh engine built with set_keep_partials(True) that never made the call: the same bits
    from every later evaluation, also after a change of a length; its gradient is the oracle's; a second call returns its bits"""
    pb, tip_mode, codes, sets, pendant, sigma, _ = _wide()
    ref = pb.gradient()
    call = lambda e: e.placement_log_likelihoods_general(codes, pendant, split=sigma, sets=sets)
    with engine_from_problem(pb, rescale=RESCALE_AUTO, tip_mode=tip_mode) as a, engine_from_problem(pb, rescale=RESCALE_AUTO, tip_mode=tip_mode) as b:
        first = call(a)
        b.set_keep_partials(True)
        b.gradient()
        at = a.branch_log_likelihood(0, float(pb.branch_lengths[0]))[0]  # read from the resident partials of a keep-partials engine
        assert abs(at - ref["lnl"]) <= 1e-10 * abs(ref["lnl"])
        lnl, cg = a.gradient()
        assert abs(lnl - ref["lnl"]) <= 1e-10 * abs(ref["lnl"])
        assert np.abs(cg - ref["cat_grad"]).max() <= 1e-9 * max(1.0, np.abs(ref["cat_grad"]).max())
        for step in range(2):
            la, ga = a.gradient()
            lb, gb = b.gradient()
            assert _bits(np.array([la, a.log_likelihood()])).tolist() == _bits(np.array([lb, b.log_likelihood()])).tolist(), step
            assert np.array_equal(_bits(ga), _bits(gb)), step
            if step == 0:
                assert _same_outputs(call(a), first)  # a call on an engine already in that state changes nothing
                a.set_branch_length(3, 0.37)
                b.set_branch_length(3, 0.37)
        moved = call(a)  # a pending change is evaluated by the call
        assert not np.array_equal(_bits(moved[0]), _bits(first[0]))
        assert _bits(np.array([a.log_likelihood()])).tolist() == _bits(np.array([b.log_likelihood()])).tolist()
        assert not a.rescaling


# ---- refusals ---------------------------------------------------------------------------------------------------------------------

def _refused(e, codes, pendant, code=EUNSUPPORTED, **kw):
    with pytest.raises(EngineError) as err:
        e.placement_log_likelihoods_general(codes, pendant, **kw)
    assert err.value.code == code, err.value
    print(err.value)
    assert NAME in str(err.value) or code == EINVAL
    return str(err.value)


def _still_usable(e, pb):
    ref = pb.log_likelihood()["lnl"]
    assert abs(e.log_likelihood() - ref) <= 1e-10 * abs(ref)


def _queries(pb, Q=2):
    return u.random_codes(np.random.default_rng(0), Q, pb.P), [0.1]


def _protein(T=8, P=100, C=2, seed=3, **kw):
    return random_problem(T, P, C, seed=seed, S=20, **kw)


def test_invalid_arguments():
    pb = _protein()
    codes, pendant = _queries(pb, 3)
    sets = np.array([0b110, 1 << 19 | 1], dtype=np.uint64)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        want = e.placement_log_likelihoods_general(codes, pendant, sets=sets)
        assert "null lnl" in _refused(e, codes, pendant, code=EINVAL, want_lnl=False, want_best=False)
        assert "queries" in _refused(e, codes[:0], pendant, code=EINVAL)
        assert "lengths" in _refused(e, codes, [], code=EINVAL)
        for split in (-1e-9, 1.0 + 1e-9, np.nan, np.inf):
            assert "split" in _refused(e, codes, pendant, code=EINVAL, split=split)
        for bad in (0.0, -0.2, np.nan, np.inf):
            assert "pendant[1]" in _refused(e, codes, [0.1, bad], code=EINVAL)
        assert "set_count" in _refused(e, codes, pendant, code=EINVAL, sets=np.arange(1, 13, dtype=np.uint64))
        for word in (0, 1 << 20, 1 << 40):
            assert "sets[1]" in _refused(e, codes, pendant, code=EINVAL, sets=np.array([3, word], dtype=np.uint64))
        for value, given in ((21, ()), (23, sets), (32, sets), (255, sets)):
            wrong = codes.copy()
            wrong[2, 57] = value
            msg = _refused(e, wrong, pendant, code=EINVAL, sets=given)
            assert NAME in msg and "query 2" in msg and "pattern 57" in msg and str(value) in msg
        lib, out = e._lib, np.empty((1, 3, pb.N))
        ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        pd = np.array(pendant)
        fn = lib.phyamd_placement_log_likelihoods_general
        assert fn(e._h, 0, 3, None, 0, None, 1, ptr(pd), 0.5, ptr(out), None, None) == EINVAL and b"null codes" in lib.phyamd_last_error()
        assert fn(e._h, 0, 3, ptr(codes), 0, None, 1, None, 0.5, ptr(out), None, None) == EINVAL and b"null pendant" in lib.phyamd_last_error()
        assert fn(e._h, 0, 3, ptr(codes), 2, None, 1, ptr(pd), 0.5, ptr(out), None, None) == EINVAL and b"null sets" in lib.phyamd_last_error()
        assert fn(e._h, 0, 3, ptr(codes), 0, None, 1, ptr(pd), 0.5, ptr(out), None, ptr(np.empty((1, 3)))) == EINVAL
        assert b"best_lnl without best_node" in lib.phyamd_last_error()
        with pytest.raises(ValueError):
            e.placement_log_likelihoods_general(codes[:, :-1], pendant)
        assert _same_outputs(e.placement_log_likelihoods_general(codes, pendant, sets=sets), want)
        _still_usable(e, pb)


def test_flags_are_refused():
    pb = _protein()
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        assert "flags" in _refused(e, *_queries(pb), flags=1)
        _still_usable(e, pb)
        e.placement_log_likelihoods_general(*_queries(pb))


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
        msg = _refused(e, *_queries(pb), code=EINVAL)
        assert NAME in msg and "eigen" in msg


def test_four_states_are_sent_to_the_four_state_call():
    pb = random_problem(8, 100, 2, seed=3)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        msg = _refused(e, *_queries(pb))
        assert "20 states" in msg and "use phyamd_placement_log_likelihoods" in msg
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
