"""GPU: phyamd_optimize_branch_lengths -- every branch length of a batch of trees optimised one branch at a time, pass after pass, in
one call -- against the CPU oracle and the NumPy restatement of the rule (tests/branch_optimize_util.py).

Bounds are the suite's for single evaluations: lnL 1e-10 relative.  At the returned lengths lnl is the oracle's, which recomputes
everything from the tips: a partial that went stale during the sweep shows there.  Lengths are compared with the restatement where
the restatement itself is stable under relative errors of 1e-9 on d1 and d2 (it moves by less than tolerance / 10: at least nine
visits, or branches of a pass, in ten, confirmed for the restatement alone in tests/test_branch_optimize_util.py), to within
tolerance.  Then convergence, the caps, the invariants of the contract, underflow in band, and every refusal."""
import copy
import functools

import numpy as np
import pytest

import branch_optimize_util as b
from gpu_util import engine_from_problem, random_problem
from physher_amd.engine import GRAD_FOLD_ROOT_FREQS, RESCALE_ALWAYS, RESCALE_AUTO, RESCALE_NEVER, EngineError
from test_batch_gpu import _bits, _deep
from test_tree_batch_gpu import Items, _mixed

pytestmark = pytest.mark.gpu
EINVAL, EUNSUPPORTED = -1, -4
TOL, LOWER, UPPER = b.TOLERANCE, b.LOWER, b.UPPER
LNL = 1e-10  # relative


def _trees(pb, count=1):
    return (np.tile(pb.left, (count, 1)), np.tile(pb.right, (count, 1)), np.full(count, pb.root, dtype=np.int32))


def _oracle_lnl(pb, tree, lengths):
    q = copy.copy(pb)
    q.left, q.right, q.root = np.array(tree[0]), np.array(tree[1]), int(tree[2])
    q.branch_lengths = np.array(lengths, dtype=np.float64)
    return q.log_likelihood()["lnl"]


def _same(x, y):
    return all((p is None and q is None) or np.array_equal(_bits(p) if p.dtype == np.float64 else p, _bits(q) if q.dtype == np.float64 else q) for p, q in zip(x, y))


@functools.lru_cache(maxsize=None)
def _converged(case):
    """the case run to convergence from start_lengths on its own engine, then again from the returned lengths: computed once"""
    pb = b.problem(case)
    start = b.start_lengths(pb)
    with engine_from_problem(pb, rescale=RESCALE_AUTO) as e:
        first = e.optimize_branch_lengths(_trees(pb), start[None, :])
        prof = e.branch_optimize_profile()
        at_result = e.gradient_batch_trees(*_trees(pb), first[0], want_gradient=False)[0]
        second = e.optimize_branch_lengths(_trees(pb), first[0])
        assert not e.rescaling
    return pb, start, first, prof, at_result, second


@pytest.mark.parametrize("case", sorted(b.CASES))
def test_lnl_at_the_result_is_the_oracles(case):
    pb, start, (lengths, lnl, lnl0, passes), prof, at_result, second = _converged(case)
    tree = (pb.left, pb.right, pb.root)
    want, want0 = _oracle_lnl(pb, tree, lengths[0]), _oracle_lnl(pb, tree, start)
    print(f"{case}: lnL {lnl0[0]!r} -> {lnl[0]!r} in {passes[0]} passes (oracle at the result {want!r}, tree batch {at_result[0]!r}); {prof}")
    assert abs(lnl[0] - want) <= LNL * abs(want)
    assert abs(lnl[0] - at_result[0]) <= LNL * abs(want)
    assert abs(lnl0[0] - want0) <= LNL * abs(want0)
    assert lnl[0] >= lnl0[0] - LNL * abs(lnl[0])
    visited = [n for n in range(pb.N) if n != pb.root]
    assert np.all((lengths[0, visited] >= LOWER) & (lengths[0, visited] <= UPPER))
    assert _bits(lengths[0, pb.root]) == _bits(start[pb.root])
    assert prof["items"] == 1 and prof["chunks"] == 1 and prof["passes"] == abs(passes[0]) and prof["scratch_bytes"] > 0
    assert prof["visits"] == abs(passes[0]) * (pb.N - 1) and prof["iterations"] >= prof["visits"]
    # converged: a further pass of the restatement gains no more than the tolerance the call stopped on
    assert 0 < passes[0] <= b.MAX_PASSES
    again = b.with_lengths(pb, lengths[0])
    gain = b.one_pass(again)[1] - want
    print(f"{case}: one further restated pass gains {gain:.3e}")
    assert gain <= b.LNL_TOLERANCE + LNL * abs(want)
    assert second[1][0] >= lnl[0] - LNL * abs(want) and second[3][0] > 0


@pytest.mark.parametrize("case", b.T8)
def test_one_visit_alone(case):
    """every node of the tree, tips and both root children among them, visited alone: one item per node, one pass"""
    pb = b.problem(case)
    start, ref = b.start_lengths(pb), b.one_visit(case)
    nodes = sorted(ref)
    mask = np.zeros((len(nodes), pb.N), dtype=np.uint8)
    mask[np.arange(len(nodes)), nodes] = 1
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        lengths, lnl, lnl0, passes = e.optimize_branch_lengths(_trees(pb, len(nodes)), np.tile(start, (len(nodes), 1)), mask, max_passes=1)
    worst, good = 0.0, 0
    for i, n in enumerate(nodes):
        others = [x for x in range(pb.N) if x != n]
        assert np.array_equal(_bits(lengths[i, others]), _bits(start[others])), (n, "another entry moved")
        assert LOWER <= lengths[i, n] <= UPPER and abs(passes[i]) == 1 and lnl[i] >= lnl0[i] - LNL * abs(lnl[i])
        want = _oracle_lnl(pb, (pb.left, pb.right, pb.root), lengths[i])
        assert abs(lnl[i] - want) <= LNL * abs(want), (n, lnl[i], want)
        if ref[n][1]:
            good += 1
            worst = max(worst, abs(lengths[i, n] - ref[n][0]))
            assert abs(lengths[i, n] - ref[n][0]) <= TOL, (n, lengths[i, n], ref[n][0])
    print(f"{case}: {good} of {len(nodes)} visits qualify, worst |t - t_ref| {worst:.3e}")
    assert good >= 0.9 * len(nodes)


@pytest.mark.parametrize("case", b.PASS_CASES)
def test_a_whole_pass(case):
    pb = b.problem(case)
    start = b.start_lengths(pb)
    ref, good = b.one_pass_thrice(case)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        lengths, lnl, lnl0, passes = e.optimize_branch_lengths(_trees(pb), start[None, :], max_passes=1)
    want = _oracle_lnl(pb, (pb.left, pb.right, pb.root), lengths[0])
    assert abs(lnl[0] - want) <= LNL * abs(want) and abs(passes[0]) == 1
    err = np.abs(lengths[0] - ref)
    print(f"{case}: {int(good.sum())} of {pb.N - 1} branches qualify, worst |t - t_ref| {err[good].max():.3e}, passes {passes[0]}")
    assert good.sum() >= 0.9 * (pb.N - 1)
    assert np.all(err[good] <= TOL), (np.flatnonzero(good & (err > TOL)), err)


@functools.lru_cache(maxsize=None)
def _batch64():
    """64 mixed 37-tip trees on one alignment, run once in one batch"""
    pb = random_problem(37, 238, 4, seed=7 * 37 + 238 + 4, gaps=0.05)
    items = _mixed(37, ["random"] * 60 + ["caterpillar", "balanced"] * 2, 37, relabel=(1, 17, 40))
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        e.gradient()
        before = e.gradient()
        out = e.optimize_branch_lengths((items.left, items.right, items.roots), items.bl)
        prof = e.branch_optimize_profile()
        again = e.optimize_branch_lengths((items.left, items.right, items.roots), items.bl)
        alone = e.optimize_branch_lengths((items.left[17:18], items.right[17:18], items.roots[17:18]), items.bl[17:18])
        moved = e.optimize_branch_lengths((items.left[[5, 17]], items.right[[5, 17]], items.roots[[5, 17]]), items.bl[[5, 17]], want_initial=False, want_passes=False)
        after = e.gradient()
    return pb, items, out, prof, again, alone, moved, before, after


def test_a_batch_of_sixty_four_trees():
    pb, items, (lengths, lnl, lnl0, passes), prof, again, alone, moved, before, after = _batch64()
    assert prof["items"] == 64 and prof["chunks"] == 1 and prof["passes"] == int(np.abs(passes).max())
    worst = 0.0
    for i in range(64):
        tree = (items.left[i], items.right[i], items.roots[i])
        want = _oracle_lnl(pb, tree, lengths[i])
        worst = max(worst, abs(lnl[i] - want) / abs(want))
        assert abs(lnl[i] - want) <= LNL * abs(want), (i, lnl[i], want)
        assert passes[i] > 0 and lnl[i] >= lnl0[i]
        assert _bits(lengths[i, items.roots[i]]) == _bits(items.bl[i, items.roots[i]])
    print(f"64 trees: passes {passes.min()}..{passes.max()}, worst relative lnL error at the result {worst:.3e}; {prof}")


def test_bits_do_not_depend_on_the_batch_and_the_engine_is_untouched():
    pb, items, out, prof, again, alone, moved, before, after = _batch64()
    assert _same(out, again)  # two calls
    assert _same([x[17:18] for x in out], alone)  # alone and at position 17 of 64
    assert _same([x[17:18] for x in out[:2]], [x[1:2] for x in moved[:2]]) and moved[2] is None and moved[3] is None  # another position, no optional outputs
    assert before[0] == after[0] and np.array_equal(_bits(before[1]), _bits(after[1]))


def test_chunks_under_a_memory_cap():
    pb, items, out, prof, *_ = _batch64()
    per_item = prof["scratch_bytes"] / 64
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        e.gradient()
        held = e.profile()["device_bytes"]
    take = np.arange(12)
    with engine_from_problem(pb, rescale=RESCALE_NEVER, max_device_bytes=int(held + 5.5 * per_item)) as e:
        e.gradient()
        got = e.optimize_branch_lengths((items.left[take], items.right[take], items.roots[take]), items.bl[take])
        capped = e.branch_optimize_profile()
    print(f"scratch per item {per_item:.0f} bytes; under the cap: {capped}")
    assert capped["items"] == 12 and capped["chunks"] >= 3
    assert _same([x[take] for x in out], got)


def test_the_engines_own_tree_and_the_calls_beside_it():
    pb = b.problem("t37_gaps_pinv")
    start = b.start_lengths(pb)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        nni = e.nni_optimize()
        batch = e.gradient_batch_trees(*_trees(pb, 2), np.stack([start, pb.branch_lengths]))
        explicit = e.optimize_branch_lengths(_trees(pb, 2), np.stack([start, pb.branch_lengths]))
        own = e.optimize_branch_lengths(None, np.stack([start, pb.branch_lengths]))
        assert _same(explicit, own)
        default = e.optimize_branch_lengths()  # one item on the engine's own lengths
        assert _same([x[1:2] for x in explicit], default)
        # the scratch is shared: the calls beside it return the bits they return without it
        assert _same(nni, e.nni_optimize())
        assert _same(batch, e.gradient_batch_trees(*_trees(pb, 2), np.stack([start, pb.branch_lengths])))


def test_the_caps_and_an_empty_mask():
    pb = b.problem("t8_random_p65")
    start = b.start_lengths(pb)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        lengths, lnl, lnl0, passes = e.optimize_branch_lengths(_trees(pb), start[None, :], max_passes=1)
        assert passes[0] == -1 and lnl[0] > lnl0[0]
        lengths, lnl, lnl0, passes = e.optimize_branch_lengths(_trees(pb), start[None, :], max_iterations=1, max_passes=3)
        want = _oracle_lnl(pb, (pb.left, pb.right, pb.root), lengths[0])
        assert lnl[0] >= lnl0[0] - LNL * abs(lnl[0]) and abs(lnl[0] - want) <= LNL * abs(want)
        lengths, lnl, lnl0, passes = e.optimize_branch_lengths(_trees(pb), start[None, :], np.zeros((1, pb.N), dtype=np.uint8))
        assert passes[0] == 0 and _bits(lnl[0]) == _bits(lnl0[0]) and np.array_equal(_bits(lengths[0]), _bits(start))
        assert e.branch_optimize_profile()["visits"] == 0
        # a node that is not visited keeps its length through whole passes, and the rest converges around it
        mask = np.ones((1, pb.N), dtype=np.uint8)
        mask[0, [1, pb.left[pb.root]]] = 0
        lengths, lnl, lnl0, passes = e.optimize_branch_lengths(_trees(pb), start[None, :], mask)
        want = _oracle_lnl(pb, (pb.left, pb.right, pb.root), lengths[0])
        assert passes[0] > 0 and abs(lnl[0] - want) <= LNL * abs(want)
        kept = [1, pb.left[pb.root], pb.root]
        assert np.array_equal(_bits(lengths[0, kept]), _bits(start[kept]))


@pytest.mark.parametrize("rescale", [RESCALE_NEVER, RESCALE_AUTO])
def test_underflow_is_reported_in_band(rescale):
    """the recipe of tests/test_site_lnl_gpu.py: on this caterpillar the short lengths underflow and the long ones do not"""
    pb = _deep(480, 100, 4, seed=5)
    short = 0.02 * pb.branch_lengths
    with engine_from_problem(pb, rescale=rescale) as e:
        alone = e.optimize_branch_lengths(_trees(pb), pb.branch_lengths[None, :], max_passes=1)
        lengths, lnl, lnl0, passes = e.optimize_branch_lengths(_trees(pb, 2), np.stack([short, pb.branch_lengths]), max_passes=1)
        assert not e.rescaling  # never a switch to rescaling
    assert not np.isfinite(lnl[0]) and not np.isfinite(lnl0[0]) and passes[0] == -1
    assert np.array_equal(_bits(lengths[0]), _bits(short))  # the state before the visit that ended the item
    assert np.isfinite(lnl0[1]) and _same([x[1:2] for x in (lengths, lnl, lnl0, passes)], alone)  # the finite item is unaffected


def _refused(e, pb, code=EUNSUPPORTED, trees=True, lengths=None, **kw):
    with pytest.raises(EngineError) as err:
        e.optimize_branch_lengths(_trees(pb) if trees else None, pb.branch_lengths[None, :] if lengths is None else lengths, **kw)
    assert err.value.code == code, err.value
    assert "phyamd_optimize_branch_lengths" in str(err.value), err.value
    return str(err.value)


def _still_usable(e, pb):
    ref = pb.log_likelihood()["lnl"]
    assert abs(e.log_likelihood() - ref) <= LNL * abs(ref)


def test_twenty_states_are_refused():
    pb = random_problem(10, 200, 2, seed=20, S=20, gaps=0.03)
    with engine_from_problem(pb, rescale=RESCALE_AUTO) as e:
        assert "4 states" in _refused(e, pb)
        _still_usable(e, pb)


def test_nine_categories_are_refused():
    pb = random_problem(8, 100, 9, seed=9)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        assert "categories" in _refused(e, pb)
        _still_usable(e, pb)


def test_a_rescaling_engine_is_refused():
    pb = random_problem(37, 238, 4, seed=12, gaps=0.03, rescale=1)
    with engine_from_problem(pb, rescale=RESCALE_ALWAYS) as e:
        assert "rescal" in _refused(e, pb)
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
        assert "tiled" in _refused(e, pb)
        _still_usable(e, pb)


def test_an_empty_tip_mask_is_refused():
    pb = random_problem(8, 100, 2, seed=23)
    tp = np.zeros((pb.T, pb.P, 4))
    for t in range(pb.T):
        tp[t, np.arange(pb.P), pb.tip_states[t]] = 1.0
    tp[3, 40] = 0.0  # no state is compatible with this cell
    pb.tip_partials, pb.tip_states = tp, None
    with engine_from_problem(pb, rescale=RESCALE_NEVER, tip_mode="partials") as e:
        assert "empty state mask" in _refused(e, pb)
        e.log_likelihood()


def test_explicit_matrices_are_refused():
    pb = random_problem(8, 100, 2, seed=3)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        e.gradient()
        e.set_node_matrices(2, e.node_matrices(2))
        assert "explicit matrices" in _refused(e, pb)
        _still_usable(e, pb)


def test_scratch_beyond_the_cap_is_refused():
    pb = random_problem(37, 700, 4, seed=99, gaps=0.05)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        e.gradient()
        held = e.profile()["device_bytes"]
        e.optimize_branch_lengths(_trees(pb), pb.branch_lengths[None, :], max_passes=1)
        per_item = e.branch_optimize_profile()["scratch_bytes"]
    with engine_from_problem(pb, rescale=RESCALE_NEVER, max_device_bytes=int(held + 0.5 * per_item)) as e:
        e.gradient()
        assert "does not fit the memory budget" in _refused(e, pb)
        _still_usable(e, pb)


def test_flags_and_a_sharded_handle_are_refused():
    pb = random_problem(8, 100, 2, seed=3)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        assert "flags" in _refused(e, pb, flags=GRAD_FOLD_ROOT_FREQS)
        _still_usable(e, pb)
    with engine_from_problem(pb, rescale=RESCALE_NEVER, devices=[0, 0]) as e:
        assert "sharded" in _refused(e, pb)
        _still_usable(e, pb)


def test_invalid_arguments_are_refused_by_name():
    pb = random_problem(8, 100, 2, seed=3)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        for kw, what in (({"lower": -1.0}, "bounds"), ({"lower": 1.0, "upper": 1.0}, "bounds"), ({"upper": np.inf}, "bounds"), ({"tolerance": 0.0}, "tolerance"),
                         ({"tolerance": np.nan}, "tolerance"), ({"max_iterations": 0}, "max_iterations"), ({"max_iterations": 1001}, "max_iterations"),
                         ({"lnl_tolerance": -1e-9}, "lnl_tolerance"), ({"lnl_tolerance": np.inf}, "lnl_tolerance"), ({"max_passes": 0}, "max_passes"),
                         ({"max_passes": 1001}, "max_passes")):
            assert what in _refused(e, pb, code=EINVAL, **kw), kw
        _still_usable(e, pb)


def test_an_invalid_item_is_refused_by_its_index_with_nothing_launched():
    pb = random_problem(8, 100, 2, seed=3)
    trees = _trees(pb, 3)
    bl = np.tile(pb.branch_lengths, (3, 1))
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        e.gradient()
        held = e.profile()["device_bytes"]
        for bad in (-0.01, np.nan, np.inf):
            broken = bl.copy()
            broken[2, 5] = bad
            with pytest.raises(EngineError) as err:
                e.optimize_branch_lengths(trees, broken)
            assert err.value.code == EINVAL and "item 2" in str(err.value) and "branch_lengths[5]" in str(err.value), err.value
            # ... but not at a node the item does not visit, nor at the root
            mask = np.ones((3, pb.N), dtype=np.uint8)
            mask[2, 5] = 0
            broken[1, pb.root] = bad
            if np.isfinite(bad):
                e.optimize_branch_lengths(trees, broken, mask, max_passes=1)
        left = trees[0].copy()
        left[1, pb.root] = 0  # a tip with two parents
        with pytest.raises(EngineError) as err:
            e.optimize_branch_lengths((left, trees[1], trees[2]), bl)
        assert err.value.code == EINVAL and "item 1" in str(err.value), err.value
        _still_usable(e, pb)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:  # nothing launched: a fresh engine holds no scratch after the refusal
        e.gradient()
        broken = bl.copy()
        broken[2, 5] = -1.0
        with pytest.raises(EngineError):
            e.optimize_branch_lengths(trees, broken)
        assert e.profile()["device_bytes"] == held and e.branch_optimize_profile()["scratch_bytes"] == 0
