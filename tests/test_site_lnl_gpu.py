"""GPU: phyamd_pattern_log_likelihoods_trees -- the per-pattern log-likelihoods of many TREES on one engine's data and models, their
weighted sums and RELL replicates of them in one call -- against the CPU oracle item by item (Problem.log_likelihood() on the item's
arrays), bit for bit across batch sizes, positions, chunks of items and of replicates and optional outputs, with the engine
untouched, and through every refusal.  Tolerances: pattern_lnl rtol = atol = 1e-11 and lnL 1e-10 relative, the suite's for
pattern_log_likelihoods and for batch lnL; a replicate entry against W @ ell_oracle.T within
    1e-11 * sum_k W[r,k] (1 + |ell[b,k]|)  +  P * 2^-52 * sum_k W[r,k] |ell[b,k]|:
the per-pattern tolerance carried through the sum, plus the bound of a sum of P terms in any order."""
import copy

import numpy as np
import pytest

from gpu_util import engine_from_problem, random_problem
from physher_amd import _lib, resampling
from physher_amd.engine import GRAD_FOLD_ROOT_FREQS, RESCALE_ALWAYS, RESCALE_AUTO, RESCALE_NEVER, EngineError
from test_batch_gpu import _ambiguous_partials, _bits, _deep
from test_tree_batch_gpu import CASES, Items, _invalid, _mixed, _own, _relabel, _still_usable, _three_taxa  # noqa: F401

pytestmark = pytest.mark.gpu
EINVAL, EUNSUPPORTED = -1, -4


def _oracle(pb, items, b):
    q = copy.copy(pb)
    q.left, q.right, q.root = items.left[b].copy(), items.right[b].copy(), int(items.roots[b])
    q.branch_lengths = items.bl[b].copy()
    return q.log_likelihood()


def _oracle_rows(pb, items):
    refs = [_oracle(pb, items, b) for b in range(len(items))]
    return np.array([r["lnl"] for r in refs]), np.array([r["pattern_lk"] for r in refs])


def _check_rows(lnl, rows, ref_lnl, ref_rows):
    for b in range(len(ref_lnl)):
        print(f"item {b}: lnL {lnl[b]!r} oracle {ref_lnl[b]!r}  max|d ell| {np.abs(rows[b] - ref_rows[b]).max():.3e}")
        np.testing.assert_allclose(rows[b], ref_rows[b], rtol=1e-11, atol=1e-11)
        assert abs(lnl[b] - ref_lnl[b]) <= 1e-10 * abs(ref_lnl[b]), (b, lnl[b], ref_lnl[b])


def _check_replicates(rep, W, ref_rows):
    P = W.shape[1]
    bound = 1e-11 * (W @ (1.0 + np.abs(ref_rows)).T) + P * 2.0 ** -52 * (W @ np.abs(ref_rows).T)
    d = np.abs(rep - W @ ref_rows.T)
    print(f"replicates: max |d| {d.max():.3e}, smallest bound {bound.min():.3e}, worst ratio {np.max(d / np.maximum(bound, 1e-300)):.3e}")
    assert np.all(d <= bound)


def _run(e, items, W=None, want_patterns=True):
    out = e.pattern_log_likelihoods_trees(*items.args(), replicate_weights=W, want_patterns=want_patterns)
    prof = e.site_lnl_profile()
    assert prof["items"] == len(items) and prof["chunks"] >= 1, prof
    assert not e.rescaling
    return out


def _same(a, b):
    return all((x is None and y is None) or np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _slots(items, b):
    lib = _lib.load()
    left, right = np.ascontiguousarray(items.left[b]), np.ascontiguousarray(items.right[b])
    slots = np.zeros(1, dtype=np.int32)
    n = lib.phyamd_post_order_slots((len(left) + 1) // 2, left.ctypes.data, right.ctypes.data, int(items.roots[b]), None, 0, slots.ctypes.data)
    assert n == (len(left) + 1) // 2 - 1
    return int(slots[0])


@pytest.mark.parametrize("case", sorted(CASES))
def test_matches_oracle_item_by_item(case):
    T, P, C, fold, pinv, gaps, ambig, make = CASES[case]
    pb = random_problem(T, P, C, seed=7 * T + P + C, gaps=gaps, pinv=pinv)
    if ambig:
        _ambiguous_partials(pb, 3)
    items = make()
    W = resampling.bootstrap_weights(pb.weights, 3, np.random.default_rng(T))
    with engine_from_problem(pb, rescale=RESCALE_AUTO, tip_mode="partials" if ambig else "states") as e:
        lnl, rows, rep = _run(e, items, W)
        assert e.site_lnl_profile()["lower_slots"] == max(_slots(items, b) for b in range(len(items)))
        # the engine's own tree, named and by default
        scale = np.random.default_rng(P).uniform(0.7, 1.4, size=(min(2, len(items)), pb.N))
        mine = Items([(pb.left, pb.right, pb.root, pb.branch_lengths * s) for s in scale])
        named = _run(e, mine, W)
        default = e.pattern_log_likelihoods_trees(None, None, None, mine.bl, replicate_weights=W)
        assert _same(named, default)
    assert rows.shape == (len(items), P) and rep.shape == (3, len(items))
    ref_lnl, ref_rows = _oracle_rows(pb, items)
    _check_rows(lnl, rows, ref_lnl, ref_rows)
    _check_replicates(rep, W, ref_rows)
    mine_lnl, mine_rows = _oracle_rows(pb, mine)
    _check_rows(named[0], named[1], mine_lnl, mine_rows)


# 8 tips, P = 4100: two segments of the product (the second ragged) and a ragged last block; C = 2; 33 items, 17 bootstrap rows
@pytest.fixture(scope="module")
def rell():
    pb = random_problem(8, 4100, 2, seed=4100, gaps=0.03)
    items = _mixed(8, ["random"] * 29 + ["balanced", "caterpillar"] * 2, 33, relabel=(1, 20))
    assert len(items) == 33
    W = resampling.bootstrap_weights(pb.weights, 17, np.random.default_rng(17))
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        e.gradient()  # (the engine's own buffers are made: what it holds besides the batch scratch)
        held = e.profile()["device_bytes"]
        out = _run(e, items, W)
        prof = e.site_lnl_profile()
        again = _run(e, items, W)
    assert prof["chunks"] == 1 and prof["replicate_chunks"] == 1, prof
    assert _same(out, again)  # twice in a row
    return pb, items, W, out, held, prof


def test_replicates_match_the_oracles_product(rell):
    pb, items, W, (lnl, rows, rep), _, _ = rell
    ref_lnl, ref_rows = _oracle_rows(pb, items)
    _check_rows(lnl, rows, ref_lnl, ref_rows)
    _check_replicates(rep, W, ref_rows)
    assert (W == 0).any() and np.all(rows[:, -1] != 0.0)


def test_an_item_and_a_replicate_do_not_depend_on_their_batch(rell):
    pb, items, W, (lnl, rows, rep), _, _ = rell
    order = np.random.default_rng(2).permutation(33)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        l1, r1, p1 = _run(e, items.take(17), W)  # alone
        assert np.array_equal(_bits(l1[0]), _bits(lnl[17])) and np.array_equal(_bits(r1[0]), _bits(rows[17])) and np.array_equal(_bits(p1[:, 0]), _bits(rep[:, 17]))
        many = items.take(np.r_[order, order[:31]])  # in a batch of 64, at other positions
        l64, r64, p64 = _run(e, many, W)
        assert np.array_equal(_bits(l64[:33]), _bits(lnl[order])) and np.array_equal(_bits(r64[33:]), _bits(rows[order[:31]]))
        assert np.array_equal(_bits(p64[:, :33]), _bits(rep[:, order]))
        # with and without the optional outputs
        assert _same(_run(e, items), (lnl, rows, None))
        assert _same(_run(e, items, W, want_patterns=False), (lnl, None, rep))
        assert _same(_run(e, items, want_patterns=False), (lnl, None, None))
        # replicate 5 alone and among 17
        assert np.array_equal(_bits(_run(e, items, W[5:6], want_patterns=False)[2][0]), _bits(rep[5]))
        # after an unrelated batch has dirtied the scratch
        e.gradient_batch(pb.branch_lengths[None, :] * np.random.default_rng(3).uniform(0.5, 1.5, size=(5, pb.N)))
        e.gradient_batch_weights(W[:3])
        assert _same(_run(e, items, W), (lnl, rows, rep))


def test_chunks_of_items_and_of_replicates_do_not_change_a_bit(rell):
    pb, items, W, want, held, prof = rell
    with engine_from_problem(pb, rescale=RESCALE_NEVER, max_device_bytes=int(held + prof["scratch_bytes"] / 3.5)) as e:
        e.gradient()
        assert e.profile()["tiles"] == 1
        got = _run(e, items, W)
        assert e.site_lnl_profile()["chunks"] >= 3, e.site_lnl_profile()
        assert _same(got, want)
    # a replicate chunk takes at most a quarter of the scratch's room: room for about 5 weight rows there, if one item fits beside
    row = 8 * 64 * ((pb.P + 63) // 64)
    seen = None
    for rows_of_room in (5.9, 7.9, 11.9, 15.9):
        with engine_from_problem(pb, rescale=RESCALE_NEVER, max_device_bytes=int(held + 4 * row * rows_of_room)) as e:
            e.gradient()
            assert e.profile()["tiles"] == 1
            try:
                got = _run(e, items, W)
            except EngineError as err:
                assert err.code == EUNSUPPORTED and "does not fit" in str(err), err
                continue
            seen = e.site_lnl_profile()
            print(rows_of_room, seen)
            assert _same(got, want)
            if seen["replicate_chunks"] >= 2:
                break
    assert seen is not None and seen["replicate_chunks"] >= 2 and seen["chunks"] >= 3, seen


def test_the_footprint_is_the_parked_partials():
    pb = random_problem(37, 700, 4, seed=99, gaps=0.05)
    items = _mixed(37, ["random"] * 62 + ["balanced", "caterpillar"], 64, relabel=(3, 17))
    most = max(_slots(items, b) for b in range(64))
    assert 1 <= most <= 4  # floor(log2 37) - 1
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        e.gradient()
        held = e.profile()["device_bytes"]
        want_trees = e.gradient_batch_trees(*items.args(), want_gradient=False)[0]
        scratch = e.batch_profile()["scratch_bytes"]
        flat = items.take([63])
        _run(e, flat)
        assert e.site_lnl_profile()["lower_slots"] == 0  # a caterpillar parks nothing
    with engine_from_problem(pb, rescale=RESCALE_NEVER, max_device_bytes=int(held + scratch / 3.5)) as e:
        e.gradient()
        assert e.profile()["tiles"] == 1
        e.gradient_batch_trees(*items.args(), want_gradient=False)
        tree_chunks = e.batch_profile()["chunks"]
        lnl, rows, _ = _run(e, items)
        prof = e.site_lnl_profile()
    print(prof, "tree batch chunks", tree_chunks)
    assert prof["lower_slots"] == most
    assert tree_chunks >= 3 and prof["chunks"] < tree_chunks
    assert np.abs(lnl - want_trees).max() <= 1e-12 * np.abs(want_trees).max()  # (the same sums, formed by another kernel)


@pytest.mark.parametrize("capped", [False, True])
def test_the_engine_is_untouched(capped):
    """capped: under a cap that cuts the items into >= 3 chunks (found as tests/test_tree_batch_gpu.py finds its own), where the
    scratch is released whenever an array of the engine itself needs the room"""
    pb = random_problem(37, 700, 4, seed=31, gaps=0.05)
    items = _mixed(37, ["random"] * (64 if capped else 16), 2)
    W = resampling.bootstrap_weights(pb.weights, 4, np.random.default_rng(1))
    rescale, kw = RESCALE_AUTO, {}
    if capped:
        rescale = RESCALE_NEVER
        with engine_from_problem(pb, rescale=rescale) as e:
            e.gradient()
            held = e.profile()["device_bytes"]
            _run(e, items, W)
            kw = dict(max_device_bytes=int(held + e.site_lnl_profile()["scratch_bytes"] / 3.5))
    node = 5 if pb.root != 5 else 6
    with engine_from_problem(pb, rescale=rescale, **kw) as e, engine_from_problem(pb, rescale=rescale, **kw) as fresh:
        before = e.gradient()
        plk = e.pattern_log_likelihoods()
        _run(e, items, W)
        assert e.site_lnl_profile()["chunks"] >= (3 if capped else 1), e.site_lnl_profile()
        after = e.gradient()
        assert _bits(before[0]) == _bits(after[0]) and np.array_equal(_bits(before[1]), _bits(after[1]))
        assert np.array_equal(_bits(plk), _bits(e.pattern_log_likelihoods()))
        fresh.gradient()
        _run(e, items.take([0, 1, 2]), W)
        for eng in (e, fresh):
            eng.set_branch_length(node, 0.37)
        a, b = e.gradient(), fresh.gradient()
        assert _bits(a[0]) == _bits(b[0]) and np.array_equal(_bits(a[1]), _bits(b[1]))
        assert _bits(e.log_likelihood()) == _bits(fresh.log_likelihood())
        if capped:
            assert e.profile()["device_bytes"] <= kw["max_device_bytes"]


@pytest.mark.parametrize("rescale", [RESCALE_NEVER, RESCALE_AUTO])
def test_underflowing_items_are_reported_in_band(rescale):
    # 480 tips: on its own lengths a pattern's likelihood is about 0.25^480, small but a double; on short branches the same data
    # cost a substitution at most tips and the likelihood underflows to 0
    pb = _deep(480, 100, 4, seed=5)
    bl = 0.02 * pb.branch_lengths[None, :] * np.random.default_rng(8).uniform(0.9, 1.2, size=(4, pb.N))
    bl[2] = pb.branch_lengths  # an item that does not underflow, among three that do
    items = Items([(pb.left, pb.right, pb.root, bl[b]) for b in range(4)])
    W = resampling.bootstrap_weights(pb.weights, 3, np.random.default_rng(2))
    with engine_from_problem(pb, rescale=rescale) as e:
        lnl, rows, rep = _run(e, items, W)  # (and the engine is still not rescaling)
        alone = _run(e, items.take(2), W)
    under = [0, 1, 3]
    assert not np.any(np.isfinite(lnl[under])) and np.all(np.isnan(rep[:, under]))
    assert not np.all(np.isfinite(rows[under]))  # the rows as computed
    assert np.isfinite(lnl[2]) and np.all(np.isfinite(rows[2])) and np.all(np.isfinite(rep[:, 2]))
    assert _bits(alone[0][0]) == _bits(lnl[2]) and np.array_equal(_bits(alone[1][0]), _bits(rows[2])) and np.array_equal(_bits(alone[2][:, 0]), _bits(rep[:, 2]))


def _refused(e, items, flags=0):
    with pytest.raises(EngineError) as err:
        e.pattern_log_likelihoods_trees(*items.args(), flags=flags)
    assert err.value.code == EUNSUPPORTED, err.value
    assert "phyamd_pattern_log_likelihoods_trees" in str(err.value)
    print(err.value)
    return str(err.value)


def test_twenty_states_are_refused():
    pb = random_problem(10, 200, 2, seed=20, S=20, gaps=0.03)
    with engine_from_problem(pb, rescale=RESCALE_AUTO) as e:
        assert "4 states" in _refused(e, _own(pb))
        _still_usable(e, pb)


def test_a_rescaling_engine_is_refused():
    pb = random_problem(37, 238, 4, seed=12, gaps=0.03, rescale=1)
    with engine_from_problem(pb, rescale=RESCALE_ALWAYS) as e:
        assert "rescal" in _refused(e, _own(pb))
        _still_usable(e, pb)


def test_an_auto_engine_that_has_switched_is_refused():
    pb = _deep(800, 100, 4, seed=5)
    with engine_from_problem(pb, rescale=RESCALE_AUTO) as e:
        e.log_likelihood()
        assert e.rescaling
        assert "rescal" in _refused(e, _own(pb))
        _still_usable(e, pb)


def test_a_tiled_engine_is_refused():
    pb = random_problem(40, 2000, 4, seed=13, gaps=0.03)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        e.gradient()
        base = e.profile()["device_bytes"]
    cap = None
    for frac in np.arange(0.9, 0.1, -0.05):  # (the search of tests/test_batch_gpu.py for a cap that tiles)
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
        assert "tiled" in _refused(e, _own(pb))
        _still_usable(e, pb)


def test_an_empty_tip_mask_is_refused():
    pb = random_problem(8, 100, 2, seed=23)
    tp = np.zeros((pb.T, pb.P, 4))
    for t in range(pb.T):
        tp[t, np.arange(pb.P), pb.tip_states[t]] = 1.0
    tp[3, 40] = 0.0  # no state is compatible with this cell
    pb.tip_partials, pb.tip_states = tp, None
    with engine_from_problem(pb, rescale=RESCALE_NEVER, tip_mode="partials") as e:
        assert "empty state mask" in _refused(e, _own(pb))
        e.log_likelihood()


def test_explicit_matrices_are_refused():
    pb = random_problem(8, 100, 2, seed=3)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        e.gradient()
        e.set_node_matrices(2, e.node_matrices(2))
        assert "explicit matrices" in _refused(e, _own(pb))
        _still_usable(e, pb)


def test_flags_are_refused():
    pb = random_problem(8, 100, 2, seed=3)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        for flags in (GRAD_FOLD_ROOT_FREQS, 2, 4):
            assert "flags" in _refused(e, _own(pb), flags=flags)
        _still_usable(e, pb)
        _run(e, _own(pb))


@pytest.mark.parametrize("kind", ["two_parents", "cycle", "tip_with_children", "root_is_a_tip", "root_is_a_child", "child_out_of_range"])
def test_invalid_topologies_name_the_item(kind):
    pb = random_problem(8, 65, 2, seed=9, shape="balanced")
    items = _invalid(kind, pb)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        with pytest.raises(EngineError) as err:
            e.pattern_log_likelihoods_trees(*items.args())
        print(err.value)
        assert err.value.code == EINVAL and "phyamd_pattern_log_likelihoods_trees: item 1" in str(err.value), err.value
        good = items.take([0, 2])
        lnl, rows, _ = _run(e, good)
    _check_rows(lnl, rows, *_oracle_rows(pb, good))


@pytest.mark.parametrize("bad", [-1.0, np.nan, np.inf])
def test_a_bad_replicate_weight_names_the_replicate(bad):
    pb = random_problem(8, 65, 2, seed=9)
    W = resampling.bootstrap_weights(pb.weights, 4, np.random.default_rng(1))
    W[2, 40] = bad
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        with pytest.raises(EngineError) as err:
            e.pattern_log_likelihoods_trees(*_own(pb).args(), replicate_weights=W)
        print(err.value)
        assert err.value.code == EINVAL and "replicate 2" in str(err.value) and "replicate_weights" in str(err.value), err.value
        _still_usable(e, pb)
        _run(e, _own(pb), W[:2])


def test_an_engine_that_is_not_ready_is_refused():
    from physher_amd.engine import Engine
    pb = random_problem(8, 65, 2, seed=9)
    with Engine(pb.T, pb.P, pb.S, pb.C, rescale=RESCALE_NEVER) as e:
        with pytest.raises(EngineError) as err:
            e.pattern_log_likelihoods_trees(*_own(pb).args())
        assert err.value.code == EINVAL and "phyamd_pattern_log_likelihoods_trees" in str(err.value) and "not ready" in str(err.value), err.value


@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0, 0]])
def test_shards_agree_with_one_engine(devices):
    """a pattern's arithmetic is lane-local: pattern_lnl has one engine's bits; lnl and replicate_lnl are sums added in shard order"""
    pb = random_problem(37, 700, 4, seed=21, gaps=0.05)
    items = _mixed(37, ["random"] * 6 + ["balanced", "caterpillar"], 6)
    W = resampling.bootstrap_weights(pb.weights, 5, np.random.default_rng(5))
    with engine_from_problem(pb, rescale=RESCALE_AUTO) as e:
        lnl, rows, rep = _run(e, items, W)
    with engine_from_problem(pb, rescale=RESCALE_AUTO, devices=devices) as e:
        ls, rs, ps = _run(e, items, W)
        lo, none, _ = _run(e, items, want_patterns=False)
    assert none is None and np.array_equal(_bits(rs), _bits(rows)) and np.array_equal(_bits(lo), _bits(ls))
    ref_lnl, ref_rows = _oracle_rows(pb, items)
    _check_rows(ls, rs, ref_lnl, ref_rows)
    _check_replicates(ps, W, ref_rows)
    _check_replicates(rep, W, ref_rows)
