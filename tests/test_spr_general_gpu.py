"""GPU: phyamd_spr_log_likelihoods_general -- lnL of every SPR regraft of chosen subtrees of a 20-state engine's tree, per prune node
from a walk of the messages and uppers that pruning changes and one launch over the target edges -- entry by entry against the CPU
oracle alone, which knows nothing of the shortcut.  Entry (p, w): the rearranged tree is built in numpy from the move's definition
(tests/test_spr_gpu.py::_moved) and the reference is log_likelihood()["lnl"] of that oracle problem.  The tolerance is the suite's for
this quantity (tests/test_spr_gpu.py, tests/test_nni_general_gpu.py): 1e-10 relative on lnL; the NaN pattern is compared exactly
against the candidate rule.  Every candidate of every row is checked for T <= 9; at T = 17 a seeded sample of 160 of the 812 that
holds every class (the oracle loop over all of them takes about six seconds on the CPU).  Then prune lists, bits across calls, a memory cap, the engine afterwards, folded uppers, a second GPU
engine, underflow in band and every refusal."""
import copy
import functools

import numpy as np
import pytest

import pair_distance_general_util as gu
from gpu_util import engine_from_problem, random_problem
from invalidation_util import parents as _parents
from physher_amd.engine import GRAD_FOLD_ROOT_FREQS, RESCALE_ALWAYS, RESCALE_AUTO, RESCALE_NEVER, Engine, EngineError
from test_batch_gpu import _bits, _deep
from test_nni_general_gpu import _underflow_case
from test_spr_gpu import CLASSES, _candidate_mask, _candidate_row, _check, _classes, _moved, _pairs, _reference, _sibling
from test_tree_batch_gpu import _relabel

pytestmark = pytest.mark.gpu
EINVAL, EUNSUPPORTED = -1, -4
NAME = "phyamd_spr_log_likelihoods_general"
TILE, BLOCK = 16, 128  # patterns of a wave's tile and of a workgroup
MORE_CLASSES = ("s a tip", "s internal", "w on the path with its path child the slot of u")

# (T, shape, P, C, gaps, pinv, engine tip sets, relabelled): the smallest shapes where the kernels can go wrong
CASES = {
    "t3_p5_c1": (3, "random", 5, 1, 0.0, None, 0, False),
    "t4_caterpillar_p16_c4": (4, "caterpillar", 16, 4, 0.0, None, 0, False),
    "t4_balanced_p17_c2": (4, "balanced", 17, 2, 0.0, None, 0, False),
    "t9_random_p130_c8_sets": (9, "random", 130, 8, 0.08, None, 3, False),
    "t9_caterpillar_p70_c4_pinv": (9, "caterpillar", 70, 4, 0.0, 0.25, 0, False),
    "t9_relabelled_p64_c1": (9, "random", 64, 1, 0.0, None, 0, True),
    "t17_random_p200_c4": (17, "random", 200, 4, 0.0, None, 0, False),
}


def _depths(pb, parent):
    d = np.zeros(pb.N, dtype=int)
    for n in range(pb.N):
        a = n
        while a != pb.root:
            a = parent[a]
            d[n] += 1
    return d


def _more_classes(pb, parent, p, w):
    u = parent[p]
    found = {"s a tip" if _sibling(pb, parent, p) < pb.T else "s internal"}
    if w == parent[u]:  # w = g: the path child of w is u's slot, which holds P_u m_s
        found.add("w on the path with its path child the slot of u")
    return found


SAMPLE = 160  # entries checked at T = 17, where the oracle loop over all 812 candidates takes about six seconds on the CPU


def _all_classes(pb, parent, p, w):
    return _classes(pb, parent, p, w) | _more_classes(pb, parent, p, w)


def _sample(pb, count):
    """a seeded sample of `count` candidates that holds every class: first one pair per class still missing, then whatever comes"""
    mask, parent = _candidate_mask(pb), _parents(pb)
    pairs = _pairs(mask)
    order = np.random.default_rng(48).permutation(len(pairs))
    sample, missing = [], set(CLASSES) | set(MORE_CLASSES)
    for i in order:
        got = _all_classes(pb, parent, *pairs[i])
        if got & missing:
            sample.append(pairs[i])
            missing -= got
    assert not missing, missing
    for i in order:
        if len(sample) == count:
            break
        if pairs[i] not in sample:
            sample.append(pairs[i])
    return sample


def _reference_table(pb, pairs=None):
    """the oracle's lnL of the candidates `pairs` (None: every candidate): [N][N], NaN everywhere else"""
    mask, parent = _candidate_mask(pb), _parents(pb)
    ref = np.full((pb.N, pb.N), np.nan)
    for p, w in _pairs(mask) if pairs is None else pairs:
        assert mask[p, w]
        ref[p, w] = _reference(pb, parent, p, w)
    return ref


@functools.lru_cache(maxsize=None)
def _case(name):
    """(problem, tip mode, the oracle's table), computed once and left unchanged"""
    T, shape, P, C, gaps, pinv, tip_sets, relabel = CASES[name]
    pb = random_problem(T, P, C, seed=7 * T + P + C, S=20, shape=shape, gaps=gaps, pinv=pinv)
    if relabel:
        tree, _ = _relabel((pb.left, pb.right, pb.root, pb.branch_lengths), np.random.default_rng(3), pb.T)
        pb.left, pb.right, pb.root, pb.branch_lengths = tree[0], tree[1], tree[2], tree[3]
    if tip_sets:
        gu.with_sets(pb, tip_sets, 0.1, 7 * T + P + C + 1)
    ref = _reference_table(pb, _sample(pb, SAMPLE) if T == 17 else None)  # every candidate for T <= 9
    ref.setflags(write=False)
    return pb, ("partials" if tip_sets else "states"), ref


def _compare(pb, got, ref, what):
    """the NaN pattern exactly against the candidate rule, every entry of the oracle's table at 1e-10 relative"""
    mask = _candidate_mask(pb)
    assert got.shape == mask.shape, what
    assert np.array_equal(np.isnan(got), ~mask) and np.all(np.isfinite(got[mask])), what
    checked = ~np.isnan(ref)
    assert checked.any() and not np.any(checked & ~mask)
    err = np.abs(got[checked] - ref[checked]) / np.abs(ref[checked])
    print(f"{what}: {int(checked.sum())} entries of {int(mask.sum())} candidates, worst relative lnL error {err.max():.3e}")
    assert err.max() <= 1e-10, (what, _pairs(checked)[int(np.argmax(err))])


@pytest.mark.parametrize("case", sorted(CASES))
def test_every_candidate_of_every_row_matches_the_oracle(case):
    pb, tip_mode, ref = _case(case)
    mask, parent = _candidate_mask(pb), _parents(pb)
    tip = lambda n: n < pb.T
    if case == "t3_p5_c1":  # one candidate per live row: w the sibling of u, x the root, everything a tip; less than one tile
        assert mask.sum() == 2 and pb.P < TILE
        for p, w in _pairs(mask):
            assert mask[p].sum() == 1 and w == _sibling(pb, parent, parent[p]) and parent[w] == pb.root
            assert tip(p) and tip(w) and tip(_sibling(pb, parent, p))
    if case == "t4_caterpillar_p16_c4":
        assert pb.P == TILE
    if case == "t4_balanced_p17_c2":
        assert TILE < pb.P < 2 * TILE and all(not tip(c) for c in (pb.left[pb.root], pb.right[pb.root]))
    if case == "t9_random_p130_c8_sets":  # a workgroup's patterns and a bit, the most categories, unknown cells and engine sets
        codes = gu.codes_from_problem(pb)[0]
        assert BLOCK < pb.P < BLOCK + TILE and pb.C == 8 and np.any(codes == 20) and np.any(codes > 20)
    if case == "t9_caterpillar_p70_c4_pinv":  # a zero-rate category; the longest path: every internal node but the root and u's parent's slot
        assert pb.cat_rates[0] == 0.0 and pb.cat_props[0] == 0.25
        depth = _depths(pb, parent)
        assert max(depth[parent[p]] - 1 for p in range(pb.N) if mask[p].any()) == pb.T - 3
    if case == "t9_relabelled_p64_c1":  # internal ids permuted, the root not 2T-2
        assert pb.root != pb.N - 1
    if case == "t17_random_p200_c4":  # the sample holds every class
        found = set().union(*(_all_classes(pb, parent, p, w) for p, w in _pairs(~np.isnan(ref))))
        assert found == set(CLASSES) | set(MORE_CLASSES), (set(CLASSES) | set(MORE_CLASSES)) - found
        assert np.count_nonzero(~np.isnan(ref)) == SAMPLE
    else:
        assert np.array_equal(~np.isnan(ref), mask)  # every candidate
    assert len(set(pb.weights)) > 1  # weights that are not uniform
    with engine_from_problem(pb, rescale=RESCALE_AUTO, tip_mode=tip_mode) as e:
        got = e.spr_log_likelihoods_general()
        prof = e.spr_profile()
        assert prof["prunes"] == pb.N and prof["candidates"] == mask.sum() and prof["chunks"] == 1 and prof["scratch_bytes"] > 0 and not e.rescaling, prof
    _compare(pb, got, ref, case)


def test_prune_lists():
    pb, tip_mode, _ = _case("t9_random_p130_c8_sets")
    parent = _parents(pb)
    dead = [pb.root, int(pb.left[pb.root]), int(pb.right[pb.root])]
    with engine_from_problem(pb, rescale=RESCALE_AUTO, tip_mode=tip_mode) as e:
        full = e.spr_log_likelihoods_general()
        assert np.array_equal(_bits(full), _bits(e.spr_log_likelihoods_general(np.arange(pb.N))))  # None is range(N)
        prune = [5, 0, pb.root, 9, 5, 14, 3, 5, dead[1]]  # duplicates, a permuted order, the root and a child of it
        got = e.spr_log_likelihoods_general(prune)
        assert got.shape == (len(prune), pb.N) and e.spr_profile()["prunes"] == len(prune)
        for i, p in enumerate(prune):
            assert np.array_equal(_bits(got[i]), _bits(full[p])), (i, p)
        live = next(p for p in range(pb.N) if p not in dead and parent[p] != pb.root)
        assert np.array_equal(_bits(e.spr_log_likelihoods_general([live])[0]), _bits(full[live]))  # a row alone
        assert np.any(np.isfinite(full[live]))
        assert np.all(np.isnan(full[dead])) and np.all(np.isnan(e.spr_log_likelihoods_general(dead)))
        assert e.spr_profile()["candidates"] == 0


def test_two_calls_return_identical_bits_whatever_the_scratch_held():
    pb, tip_mode, _ = _case("t17_random_p200_c4")
    with engine_from_problem(pb, rescale=RESCALE_AUTO, tip_mode=tip_mode) as e:
        first = e.spr_log_likelihoods_general()
        assert np.array_equal(_bits(first), _bits(e.spr_log_likelihoods_general()))
        e.pairwise_distances_general(counts_only=True, want_counts=True)  # (other calls in the same scratch)
        e.nni_log_likelihoods_general()
        assert np.array_equal(_bits(first), _bits(e.spr_log_likelihoods_general()))
        assert not e.rescaling
    with engine_from_problem(pb, rescale=RESCALE_AUTO, tip_mode=tip_mode) as e:  # a scratch that held nothing before
        assert np.array_equal(_bits(first), _bits(e.spr_log_likelihoods_general()))


def test_under_a_memory_cap():
    pb, tip_mode, _ = _case("t17_random_p200_c4")
    with engine_from_problem(pb, rescale=RESCALE_NEVER, tip_mode=tip_mode) as e:
        e.set_keep_partials(True)
        e.gradient()
        held = e.profile()["device_bytes"]  # (what the engine holds besides the batch scratch)
        want = e.spr_log_likelihoods_general()
        prof = e.spr_profile()
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
                got = e.spr_log_likelihoods_general()
            except EngineError as err:
                assert err.code == EUNSUPPORTED and "scratch" in str(err), err
                continue
            chunks = e.spr_profile()["chunks"]
            print(f"cap = held + {extra} x scratch = {cap}: {chunks} chunks; device_bytes {e.profile()['device_bytes']}")
            assert chunks >= 2
            assert e.profile()["device_bytes"] <= cap
            assert np.array_equal(_bits(want), _bits(got))
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
    pb, tip_mode, _ = _case("t9_random_p130_c8_sets")
    ref = pb.gradient()
    with engine_from_problem(pb, rescale=RESCALE_AUTO, tip_mode=tip_mode) as a, engine_from_problem(pb, rescale=RESCALE_AUTO, tip_mode=tip_mode) as b:
        first = a.spr_log_likelihoods_general()
        assert not a.rescaling
        b.set_keep_partials(True)
        b.gradient()
        for step in range(2):
            la, ga = a.gradient()
            lb, gb = b.gradient()
            assert _bits(np.array([la, a.log_likelihood()])).tolist() == _bits(np.array([lb, b.log_likelihood()])).tolist(), step
            assert np.array_equal(_bits(ga), _bits(gb)), step
            if step == 0:
                assert abs(la - ref["lnl"]) <= 1e-10 * abs(ref["lnl"])  # the engine's tree and lengths are the problem's still
                assert np.abs(ga - ref["cat_grad"]).max() <= 1e-9 * max(1.0, np.abs(ref["cat_grad"]).max())
                assert np.array_equal(_bits(a.spr_log_likelihoods_general()), _bits(first))  # a call on an engine already in that state
                a.set_branch_length(3, 0.37)
                b.set_branch_length(3, 0.37)
        moved = a.spr_log_likelihoods_general()  # a pending change is evaluated by the call
        assert not np.array_equal(_bits(moved), _bits(first))
        assert _bits(np.array([a.log_likelihood()])).tolist() == _bits(np.array([b.log_likelihood()])).tolist()
        assert not a.rescaling


def test_folded_uppers_do_not_matter():
    """after a keep-partials PHYAMD_GRAD_FOLD_ROOT_FREQS gradient the resident uppers carry pi; the frequencies are not uniform,
    and every entry still meets the oracle: the call reads no resident upper"""
    pb, tip_mode, ref = _case("t9_random_p130_c8_sets")
    assert np.ptp(pb.freqs) > 0.01
    with engine_from_problem(pb, rescale=RESCALE_NEVER, tip_mode=tip_mode) as e:
        e.set_keep_partials(True)
        e.gradient(GRAD_FOLD_ROOT_FREQS)
        folded = e.spr_log_likelihoods_general()
    _compare(pb, folded, ref, "folded uppers")


def test_a_second_engine_given_the_rearranged_tree_agrees():
    pb, tip_mode, _ = _case("t17_random_p200_c4")
    mask, parent = _candidate_mask(pb), _parents(pb)
    pairs = _pairs(mask)
    sample = [pairs[i] for i in np.random.default_rng(9).permutation(len(pairs))[:6]]
    with engine_from_problem(pb, rescale=RESCALE_NEVER, tip_mode=tip_mode) as e:
        got = e.spr_log_likelihoods_general()
    with engine_from_problem(pb, rescale=RESCALE_NEVER, tip_mode=tip_mode) as other:
        for p, w in sample:
            left, right, bl = _moved(pb, parent, p, w)
            other.set_topology(left, right, pb.root)
            other.set_branch_lengths(bl)
            ref = other.log_likelihood()
            assert abs(got[p, w] - ref) <= 1e-10 * abs(ref), (p, w, got[p, w], ref)


# ---- underflow --------------------------------------------------------------------------------------------------------------------

def _live_rows(pb, parent, want):
    return [n for n in want if n != pb.root and parent[n] != pb.root]


def test_underflow_is_reported_in_band():
    """the deep caterpillar of tests/test_nni_general_gpu.py, where one pattern's site likelihood is 0 without rescaling: the call
    returns, every candidate holds a number or an lnL that is not finite, every other cell NaN, and the engine is not switched"""
    pb, site = _underflow_case()
    assert site.min() < -330.0 and pb.weights[int(np.argmin(site))] > 0
    parent = _parents(pb)
    prune = _live_rows(pb, parent, (5, pb.T // 2, pb.T + pb.T // 3, pb.N - 3))
    assert len(prune) >= 3
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        got = e.spr_log_likelihoods_general(prune)  # returns: no error
        assert not e.rescaling
    for i, p in enumerate(prune):
        row = _candidate_row(pb, parent, p)
        bad = ~np.isfinite(got[i, row])
        print(f"row of {p}: {int(bad.sum())} of {int(row.sum())} candidates are not finite")
        assert row.sum() > 0 and bad.any() and np.all(np.isnan(got[i, ~row]))
        assert np.all(got[i, row][~bad] < 0)  # a finite candidate is a log-likelihood


def test_an_engine_that_switches_to_rescaling_during_the_call_is_refused():
    pb = _deep(600, 20, 2, seed=5, S=20)
    with engine_from_problem(pb, rescale=RESCALE_AUTO) as e:
        assert not e.rescaling
        msg = _refused(e, prune=[3])
        assert "rescal" in msg and "PHYAMD_RESCALE_AUTO" in msg
        assert e.rescaling
        _still_usable(e, pb)


def test_an_auto_engine_is_not_switched_where_its_own_lnl_is_finite():
    """PHYAMD_RESCALE_AUTO on the deepest tree the suite has whose own lnL is finite (tests/test_placement_general_gpu.py's, one
    pattern's site likelihood a subnormal number): the call returns and the engine is not rescaling afterwards"""
    from test_placement_general_gpu import underflow_case
    pb = underflow_case()[0]
    parent = _parents(pb)
    prune = _live_rows(pb, parent, (5, pb.T // 2, pb.T + pb.T // 3, pb.N - 3))
    with engine_from_problem(pb, rescale=RESCALE_AUTO) as e:
        got = e.spr_log_likelihoods_general(prune)
        assert not e.rescaling
        own = e.log_likelihood()
        assert np.isfinite(own) and not e.rescaling
    for i, p in enumerate(prune):
        row = _candidate_row(pb, parent, p)
        print(f"AUTO, row of {p}: {int((~np.isfinite(got[i, row])).sum())} of {int(row.sum())} candidates are not finite")
        assert row.sum() > 0 and np.all(np.isnan(got[i, ~row]))
        assert np.all(got[i, row][np.isfinite(got[i, row])] < 0)  # a finite candidate is a log-likelihood


# ---- refusals ---------------------------------------------------------------------------------------------------------------------

def _refused(e, code=EUNSUPPORTED, **kw):
    with pytest.raises(EngineError) as err:
        e.spr_log_likelihoods_general(**kw)
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
        assert "20 states" in msg and "use phyamd_spr_log_likelihoods)" in msg
        _still_usable(e, pb)
        assert np.any(np.isfinite(e.spr_log_likelihoods()))


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
        e.spr_log_likelihoods_general()


def test_a_missing_eigen_system_and_an_engine_that_is_not_ready_are_refused():
    pb = _protein()
    with Engine(pb.T, pb.P, 20, pb.C, rescale=RESCALE_NEVER) as e:
        e.set_topology(pb.left, pb.right, pb.root)
        e.set_branch_lengths(pb.branch_lengths)
        e.set_frequencies(pb.freqs)
        e.set_category_rates(pb.cat_rates, pb.cat_props)
        e.set_pattern_weights(pb.weights)
        for t in range(pb.T - 1):
            e.set_tip_states(t, pb.tip_states[t])
        assert "eigen" in _refused(e, code=EINVAL)
        e.set_eigen(pb.eval, pb.evec, pb.ivec)
        assert "has no data" in _refused(e, code=EINVAL)  # the last tip: not ready
        e.set_tip_states(pb.T - 1, pb.tip_states[pb.T - 1])
        assert np.any(np.isfinite(e.spr_log_likelihoods_general()))


def test_a_bad_prune_list_is_refused():
    pb = _protein()
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        for bad in (-1, pb.N):
            msg = _refused(e, code=EINVAL, prune=[3, 4, bad, 5])
            assert "prune[2]" in msg
        out = np.empty((3, pb.N))
        rc = e._lib.phyamd_spr_log_likelihoods_general(e._h, 0, 0, None, out.ctypes.data)  # count < 1
        msg = e._lib.phyamd_last_error().decode()
        print(msg)
        assert rc == EINVAL and NAME in msg and "count must be >= 1" in msg
        rc = e._lib.phyamd_spr_log_likelihoods_general(e._h, 0, 3, None, out.ctypes.data)  # a null list with another count than N
        msg = e._lib.phyamd_last_error().decode()
        print(msg)
        assert rc == EINVAL and NAME in msg and "prune is null" in msg and str(pb.N) in msg
        _still_usable(e, pb)


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
