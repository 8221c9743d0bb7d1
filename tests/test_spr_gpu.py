"""GPU: phyamd_spr_log_likelihoods -- lnL of every SPR regraft of chosen subtrees, per prune node from one post-order walk, one
pre-order walk of the tree without it and one launch over the target edges -- entry by entry against references that know
nothing of the shortcut.  Entry (p, w): the rearranged tree is built in numpy from the move's definition (the sibling takes the
parent's place with both lengths, the parent goes onto the edge above w, which is halved); its log-likelihood is the CPU
oracle's, and in one test the tree batch's on a second engine.  The tolerance is the suite's for single evaluations
(tests/test_nni_gpu.py, tests/test_tree_batch_gpu.py): 1e-10 relative on lnL.  Then prune lists, bits across calls, stale lists,
a memory cap, every refusal, underflowing partials and a sharded handle."""
import copy
import functools

import numpy as np
import pytest

from gpu_util import engine_from_problem, random_problem
from physher_amd.engine import GRAD_FOLD_ROOT_FREQS, RESCALE_ALWAYS, RESCALE_AUTO, RESCALE_NEVER, EngineError
from test_batch_gpu import _ambiguous_partials, _bits, _deep
from test_nni_gpu import _parents, _relabelled

pytestmark = pytest.mark.gpu
EINVAL, EUNSUPPORTED = -1, -4
CLASSES = ("p a tip", "p internal", "w a tip", "w a proper ancestor of u", "w = g", "w the sibling of u", "w a child of the root", "w a child of s")


def _sibling(pb, parent, n):
    x = parent[n]
    return pb.right[x] if pb.left[x] == n else pb.left[x]


def _below(pb, p):
    """p and its descendants"""
    out, stack = [], [p]
    while stack:
        n = stack.pop()
        out.append(n)
        if n >= pb.T:
            stack += [pb.left[n], pb.right[n]]
    return out


def _candidate_row(pb, parent, p):
    """the candidate rule: which columns of row p hold a number"""
    row = np.zeros(pb.N, dtype=bool)
    if p == pb.root or parent[p] == pb.root:
        return row
    row[:] = True
    row[[pb.root, parent[p], _sibling(pb, parent, p)] + _below(pb, p)] = False
    return row


def _candidate_mask(pb):
    parent = _parents(pb)
    return np.array([_candidate_row(pb, parent, p) for p in range(pb.N)])


def _moved(pb, parent, p, w):
    """(left, right, branch_lengths) after pruning p and regrafting it onto the edge above w: the move's definition"""
    left, right, bl = pb.left.copy(), pb.right.copy(), pb.branch_lengths.copy()
    u = parent[p]
    s, g, x = _sibling(pb, parent, p), parent[u], parent[w]
    (left if pb.left[g] == u else right)[g] = s  # g's slot of u now holds s
    bl[s] = pb.branch_lengths[s] + pb.branch_lengths[u]
    (left if pb.left[x] == w else right)[x] = u  # x's slot of w now holds u (x = g: its other slot, or the one s has just left)
    (left if pb.left[u] == s else right)[u] = w  # u keeps p and gets w where s was
    bl[u] = bl[w] = 0.5 * pb.branch_lengths[w]
    return left, right, bl


def _reference(pb, parent, p, w):
    q = copy.copy(pb)
    q.left, q.right, q.branch_lengths = _moved(pb, parent, p, w)
    return q.log_likelihood()["lnl"]


def _classes(pb, parent, p, w):
    u = parent[p]
    s, g = _sibling(pb, parent, p), parent[u]
    ancestors, n = [], parent[u]
    while n >= 0:
        ancestors.append(n)
        n = parent[n]
    found = {"p a tip" if p < pb.T else "p internal"}
    if w < pb.T:
        found.add("w a tip")
    if w in ancestors:
        found.add("w a proper ancestor of u")
    if w == g:
        found.add("w = g")
    if w == _sibling(pb, parent, u):
        found.add("w the sibling of u")
    if parent[w] == pb.root:
        found.add("w a child of the root")
    if parent[w] == s:
        found.add("w a child of s")
    return found


def _pairs(mask):
    return [(int(p), int(w)) for p, w in zip(*np.nonzero(mask))]


def _check(pb, got, pairs, what):
    """the entries `pairs` of a full [N, N] result against the oracle, and its NaN pattern against the rule"""
    mask, parent = _candidate_mask(pb), _parents(pb)
    assert got.shape == (pb.N, pb.N) and np.array_equal(np.isfinite(got), mask), what
    assert np.all(np.isnan(got[~mask]))
    worst = 0.0
    for p, w in pairs:
        assert mask[p, w]
        ref = _reference(pb, parent, p, w)
        err = abs(got[p, w] - ref) / abs(ref)
        worst = max(worst, err)
        assert err <= 1e-10, (what, p, w, got[p, w], ref)
    print(f"{what}: {len(pairs)} entries of {int(mask.sum())} candidates, worst relative lnL error {worst:.3e}")


# (T, P, C, shape, relabel, gaps, ambiguity codes)
CASES = {
    "t3": (3, 1, 1, "random", False, 0.0, False),
    "t4_caterpillar": (4, 63, 2, "caterpillar", False, 0.0, False),
    "t4_balanced": (4, 65, 2, "balanced", False, 0.0, False),
    "t37_gaps": (37, 238, 4, "random", False, 0.05, False),
    "t37_ambiguity": (37, 238, 4, "random", False, 0.05, True),
    "t37_c8": (37, 700, 8, "random", False, 0.0, False),
}
for _shape in ("caterpillar", "balanced", "random", "relabelled"):
    for _P in (64, 65):
        CASES[f"t8_{_shape}_p{_P}"] = (8, _P, 1, "random" if _shape == "relabelled" else _shape, _shape == "relabelled", 0.0, False)


@functools.lru_cache(maxsize=None)
def _problem(case):
    T, P, C, shape, relabel, gaps, ambig = CASES[case]
    pb = random_problem(T, P, C, seed=11 * T + P + C, shape=shape, gaps=gaps)
    if relabel:
        _relabelled(pb, 3)
    if ambig:
        _ambiguous_partials(pb, 3)
    return pb, ("partials" if ambig else "states")


@pytest.mark.parametrize("case", sorted(CASES))
def test_every_candidate_of_every_row_matches_the_oracle(case):
    pb, tip_mode = _problem(case)
    mask, parent = _candidate_mask(pb), _parents(pb)
    if case == "t3":  # the smallest tree with a candidate: either tip of the cherry onto the third tip's edge
        assert mask.sum() == 2
    if case.startswith("t8"):
        found = set().union(*(_classes(pb, parent, p, w) for p, w in _pairs(mask)))
        assert found == set(CLASSES), set(CLASSES) - found
    with engine_from_problem(pb, rescale=RESCALE_AUTO, tip_mode=tip_mode) as e:
        got = e.spr_log_likelihoods()
        prof = e.spr_profile()
        assert prof["prunes"] == pb.N and prof["candidates"] == mask.sum() and prof["chunks"] == 1 and not e.rescaling, prof
    _check(pb, got, _pairs(mask), case)


def test_two_hundred_taxa():
    """a fixed seeded sample of 48 (p, w) pairs that holds every class, and the NaN pattern of the whole [N, N] result"""
    pb = random_problem(200, 63, 4, seed=200, gaps=0.02)
    mask, parent = _candidate_mask(pb), _parents(pb)
    pairs = _pairs(mask)
    order = np.random.default_rng(48).permutation(len(pairs))
    sample, missing = [], set(CLASSES)
    for i in order:  # first one pair per class still missing, then whatever comes
        got = _classes(pb, parent, *pairs[i])
        if got & missing:
            sample.append(pairs[i])
            missing -= got
    assert not missing, missing
    for i in order:
        if len(sample) == 48:
            break
        if pairs[i] not in sample:
            sample.append(pairs[i])
    assert len(sample) == 48 and set().union(*(_classes(pb, parent, p, w) for p, w in sample)) == set(CLASSES)
    with engine_from_problem(pb, rescale=RESCALE_AUTO) as e:
        got = e.spr_log_likelihoods()
        assert e.spr_profile()["candidates"] == mask.sum()
    _check(pb, got, sample, "t200")


def test_every_candidate_matches_the_tree_batch():
    """without the oracle: every candidate's tree through gradient_batch_trees on a second engine, in batches of at most 512"""
    pb = random_problem(37, 238, 4, seed=17, gaps=0.05)
    mask, parent = _candidate_mask(pb), _parents(pb)
    pairs = _pairs(mask)
    with engine_from_problem(pb, rescale=RESCALE_AUTO) as e:
        got = e.spr_log_likelihoods()
    assert np.array_equal(np.isfinite(got), mask)
    worst = 0.0
    with engine_from_problem(pb, rescale=RESCALE_AUTO) as other:
        for first in range(0, len(pairs), 512):
            chunk = pairs[first:first + 512]
            trees = [_moved(pb, parent, p, w) for p, w in chunk]
            left, right, bl = (np.ascontiguousarray([t[i] for t in trees]) for i in range(3))
            ref, _ = other.gradient_batch_trees(left, right, np.full(len(chunk), pb.root, dtype=np.int32), bl, want_gradient=False)
            err = np.abs(np.array([got[p, w] for p, w in chunk]) - ref) / np.abs(ref)
            worst = max(worst, err.max())
            assert np.all(err <= 1e-10), (chunk[int(err.argmax())], err.max())
    print(f"{len(pairs)} candidates against the tree batch: worst relative lnL difference {worst:.3e}")


def test_prune_lists():
    pb = random_problem(8, 65, 2, seed=83, gaps=0.03)
    parent = _parents(pb)
    dead = [pb.root, int(pb.left[pb.root]), int(pb.right[pb.root])]
    with engine_from_problem(pb, rescale=RESCALE_AUTO) as e:
        full = e.spr_log_likelihoods()
        prune = [5, 0, pb.root, 9, 5, 14, 3, 5, dead[1]]  # duplicates, a permuted order, rows without a candidate
        got = e.spr_log_likelihoods(prune)
        assert got.shape == (len(prune), pb.N) and e.spr_profile()["prunes"] == len(prune)
        for i, p in enumerate(prune):
            assert np.array_equal(_bits(got[i]), _bits(full[p])), (i, p)
        live = next(p for p in range(pb.N) if p not in dead)
        assert np.array_equal(_bits(e.spr_log_likelihoods([live])[0]), _bits(full[live]))
        assert np.all(np.isnan(full[dead])) and np.all(np.isnan(e.spr_log_likelihoods(dead)))
        assert np.any(np.isfinite(full[live])) and parent[live] != pb.root
        for bad in (-1, pb.N):
            with pytest.raises(EngineError) as err:
                e.spr_log_likelihoods([3, 4, bad, 5])
            print(err.value)
            assert err.value.code == EINVAL and "prune[2]" in str(err.value)
        _still_usable(e, pb)


def test_two_tips_have_no_candidate():
    pb = random_problem(2, 65, 2, seed=2)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        got = e.spr_log_likelihoods()
        assert got.shape == (3, 3) and np.all(np.isnan(got)) and e.spr_profile()["candidates"] == 0
        _still_usable(e, pb)


def test_bit_for_bit_across_calls_and_the_engine_is_untouched():
    pb = random_problem(37, 700, 4, seed=31, gaps=0.05)
    bl = pb.branch_lengths[None, :] * np.random.default_rng(4).uniform(0.5, 1.8, size=(5, pb.N))
    other = random_problem(37, 700, 4, seed=32)  # (another tree, for the tree batch)
    trees = (other.left[None, :], other.right[None, :], np.array([other.root], dtype=np.int32), other.branch_lengths[None, :])
    with engine_from_problem(pb, rescale=RESCALE_AUTO) as e, engine_from_problem(pb, rescale=RESCALE_AUTO) as fresh:
        before = (e.log_likelihood(), e.gradient())
        first = e.spr_log_likelihoods()
        second = e.spr_log_likelihoods()
        assert np.array_equal(_bits(first), _bits(second))
        e.gradient_batch(bl)  # (the batch kinds run in the same scratch, with other op lists and fewer upper slots)
        e.gradient_batch_trees(*trees)
        e.nni_log_likelihoods()
        third = e.spr_log_likelihoods()
        assert np.array_equal(_bits(first), _bits(third))
        after = (e.log_likelihood(), e.gradient())
        assert _bits(before[0]) == _bits(after[0])
        assert _bits(before[1][0]) == _bits(after[1][0]) and np.array_equal(_bits(before[1][1]), _bits(after[1][1]))
        # an engine that never made the call takes the same path from here on
        node = 5 if pb.root != 5 else 6
        for eng in (e, fresh):
            eng.set_branch_length(node, 0.37)
        a, b = e.gradient(), fresh.gradient()
        assert _bits(a[0]) == _bits(b[0]) and np.array_equal(_bits(a[1]), _bits(b[1]))
        assert not e.rescaling
    with engine_from_problem(pb, rescale=RESCALE_AUTO) as e:  # a scratch that held nothing before
        assert np.array_equal(_bits(first), _bits(e.spr_log_likelihoods()))


def test_stale_lists():
    """after set_topology to another tree, and after set_branch_lengths, the call is the new tree's"""
    pb = random_problem(8, 65, 2, seed=84, shape="caterpillar")
    other = random_problem(8, 65, 2, seed=85, shape="balanced")
    assert not np.array_equal(pb.left, other.left)
    with engine_from_problem(pb, rescale=RESCALE_AUTO) as e:
        _check(pb, e.spr_log_likelihoods(), _pairs(_candidate_mask(pb)), "the first tree")
        q = copy.copy(pb)
        q.left, q.right, q.root, q.branch_lengths = other.left, other.right, other.root, other.branch_lengths
        e.set_topology(q.left, q.right, q.root)
        e.set_branch_lengths(q.branch_lengths)
        _check(q, e.spr_log_likelihoods(), _pairs(_candidate_mask(q)), "after set_topology")
        q = copy.copy(q)
        q.branch_lengths = q.branch_lengths * np.random.default_rng(6).uniform(0.5, 2.0, size=q.N)
        e.set_branch_lengths(q.branch_lengths)
        _check(q, e.spr_log_likelihoods(), _pairs(_candidate_mask(q)), "after set_branch_lengths")


def test_under_a_memory_cap():
    pb = random_problem(37, 700, 4, seed=99, gaps=0.05)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        e.gradient()
        held = e.profile()["device_bytes"]  # (what the engine holds besides the batch scratch)
        want = e.spr_log_likelihoods()
        prof = e.spr_profile()
        scratch, rows = prof["scratch_bytes"], pb.N - 3
        assert prof["chunks"] == 1 and scratch > 0 and e.profile()["device_bytes"] >= held + scratch
    chunks = 0
    for extra in (0.1, 0.2, 0.3, 0.45):  # the smallest of these caps that leaves room for a row: all of them are too small for all rows
        cap = int(held + extra * scratch)
        with engine_from_problem(pb, rescale=RESCALE_NEVER, max_device_bytes=cap) as e:
            e.gradient()  # (the engine's own buffers are made first: the room is what is left beside them)
            assert e.profile()["tiles"] == 1
            try:
                got = e.spr_log_likelihoods()
            except EngineError as err:
                assert err.code == EUNSUPPORTED and "scratch" in str(err), err
                continue
            chunks = e.spr_profile()["chunks"]
            print(f"cap = held + {extra} x scratch = {cap}: {chunks} chunks; device_bytes {e.profile()['device_bytes']}")
            assert chunks >= 2
            assert e.profile()["device_bytes"] <= cap
            assert np.array_equal(_bits(want), _bits(got))
            e.gradient()
            assert e.profile()["device_bytes"] <= cap
            break
    assert chunks >= 2, "no cap left room for a row"
    tight = int(held + scratch / rows / 4)
    with engine_from_problem(pb, rescale=RESCALE_NEVER, max_device_bytes=tight) as e:
        assert e.profile()["tiles"] == 1
        with pytest.raises(EngineError) as err:
            e.spr_log_likelihoods()
        print(err.value)
        assert err.value.code == EUNSUPPORTED and "scratch" in str(err.value)
        _still_usable(e, pb)
        assert e.profile()["device_bytes"] <= tight


def _refused(e, code=EUNSUPPORTED, **kw):
    with pytest.raises(EngineError) as err:
        e.spr_log_likelihoods(**kw)
    assert err.value.code == code, err.value
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


def test_an_auto_engine_that_has_switched_is_refused():
    pb = _deep(800, 100, 4, seed=5)
    with engine_from_problem(pb, rescale=RESCALE_AUTO) as e:
        e.log_likelihood()
        assert e.rescaling
        assert "rescal" in _refused(e, prune=[3])
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


def test_an_empty_tip_mask_is_refused():
    pb = random_problem(8, 100, 2, seed=23)
    tp = np.zeros((pb.T, pb.P, 4))
    for t in range(pb.T):
        tp[t, np.arange(pb.P), pb.tip_states[t]] = 1.0
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


def test_flags_are_refused():
    pb = random_problem(8, 100, 2, seed=3)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        assert "flags" in _refused(e, flags=GRAD_FOLD_ROOT_FREQS)
        _still_usable(e, pb)
        e.spr_log_likelihoods()


@pytest.mark.parametrize("rescale", [RESCALE_NEVER, RESCALE_AUTO])
def test_underflow_is_reported_in_band(rescale):
    pb = _deep(800, 100, 4, seed=5)
    parent = _parents(pb)
    prune = [n for n in (5, 400, pb.T + 300, pb.T + 700) if n != pb.root and parent[n] != pb.root]
    assert len(prune) >= 3
    with engine_from_problem(pb, rescale=rescale) as e:
        got = e.spr_log_likelihoods(prune)
        assert not e.rescaling  # never a switch to rescaling
    for i, p in enumerate(prune):
        row = _candidate_row(pb, parent, p)
        assert row.sum() > 0 and not np.any(np.isfinite(got[i])) and np.all(np.isnan(got[i, ~row]))


def test_shards_agree_with_one_engine():
    pb = random_problem(37, 700, 4, seed=21, gaps=0.05)
    with engine_from_problem(pb, rescale=RESCALE_AUTO) as e:
        one = e.spr_log_likelihoods()
    with engine_from_problem(pb, rescale=RESCALE_AUTO, devices=[0, 0]) as e:
        assert e.shard_count == 2
        two = e.spr_log_likelihoods()
    mask = _candidate_mask(pb)
    assert np.array_equal(np.isfinite(one), mask) and np.array_equal(np.isnan(two), np.isnan(one))
    err = np.abs(two[mask] - one[mask]) / np.abs(one[mask])
    print(f"two shards: worst relative lnL difference {err.max():.3e}")
    assert np.all(err <= 1e-10)
