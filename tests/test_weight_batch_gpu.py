"""GPU: phyamd_gradient_batch_weights -- lnL and the per-category branch gradient of many pattern-weight vectors in one call --
against the CPU oracle replicate by replicate on both fast paths (shared lengths: one walk and a product on the matrix pipe;
per-item lengths: the batched walk with a weight row per item), bit for bit across batch sizes, positions and chunks, under
pattern chunks, through every defined fallback, and on sharded handles.  Tolerances are the suite's for single evaluations
(tests/test_batch_gpu.py): lnL 1e-10 relative, gradient 1e-9 * max(1, max|g|).  Every parity case also asserts which path the
items took: a silent fallback must not pass."""
import copy

import numpy as np
import pytest

from gpu_util import engine_from_problem, random_problem
from physher_amd import resampling
from physher_amd.engine import GRAD_FOLD_ROOT_FREQS, RESCALE_ALWAYS, RESCALE_AUTO, RESCALE_NEVER, EngineError
from test_batch_gpu import _ambiguous_partials, _bits, _deep, _lengths

pytestmark = pytest.mark.gpu
EINVAL, EUNSUPPORTED = -1, -4


def _oracle(pb, weights, lengths=None, fold=False):
    q = copy.copy(pb)
    q.weights = np.ascontiguousarray(weights, dtype=np.float64)
    if lengths is not None:
        q.branch_lengths = np.ascontiguousarray(lengths, dtype=np.float64)
    q.fold_root_freqs = 1 if fold else 0
    return q.gradient()


def _check_against_oracle(pb, W, lnl, g, bl=None, fold=False):
    shares = [0.0, 0.0]  # the worst share of each tolerance that an item used
    for b in range(len(W)):
        ref = _oracle(pb, W[b], None if bl is None else bl[b], fold)
        print(f"item {b}: lnL {lnl[b]!r} oracle {ref['lnl']!r}  max|dg| {np.abs(g[b] - ref['cat_grad']).max():.3e}")
        shares[0] = max(shares[0], abs(lnl[b] - ref["lnl"]) / (1e-10 * abs(ref["lnl"])))
        shares[1] = max(shares[1], np.abs(g[b] - ref["cat_grad"]).max() / (1e-9 * max(1.0, np.abs(ref["cat_grad"]).max())))
        assert abs(lnl[b] - ref["lnl"]) <= 1e-10 * abs(ref["lnl"]), (b, lnl[b], ref["lnl"])
        assert np.abs(g[b] - ref["cat_grad"]).max() <= 1e-9 * max(1.0, np.abs(ref["cat_grad"]).max()), b
    print(f"{len(W)} items: worst share of the lnL tolerance {shares[0]:.2e}, of the gradient tolerance {shares[1]:.2e}")


def _replicates(pb, B, seed, kind="bootstrap", keep_first=False):
    """B weight rows: bootstrap draws of the problem's own sites, or fractional weights with some zeros (item 0: the problem's
    own weights if keep_first)"""
    rng = np.random.default_rng(seed)
    if kind == "bootstrap":
        W = resampling.bootstrap_weights(pb.weights, B, rng)
    else:
        W = pb.weights[None, :] * rng.uniform(0.0, 2.0, size=(B, pb.P)) * (rng.random((B, pb.P)) > 0.1)
    if keep_first:
        W[0] = pb.weights
    return np.ascontiguousarray(W)


# (shape, T, P, C, B, fold, pinv, gaps, ambiguity codes, weights).  The last two: 4096 + 70 patterns are two segments of
# k_reweight_mfma's K axis (REWEIGHT_SEGMENT = 4096), the second ragged, so k_reweight_finish adds two terms; 8 taxa and 2 categories
# are 1 + 15 x 2 = 31 rows, two row tiles of 16 with the second ragged, and 17 or 33 replicates two or three replicate tiles
SHARED = [
    ("random", 2, 1, 1, 1, False, None, 0.0, False, "bootstrap"),
    ("caterpillar", 3, 63, 2, 3, True, None, 0.0, False, "bootstrap"),
    ("random", 37, 238, 4, 17, False, None, 0.05, False, "bootstrap"),
    ("random", 37, 700, 4, 33, False, 0.25, 0.0, False, "fractional"),
    ("caterpillar", 200, 65, 8, 16, False, None, 0.0, False, "bootstrap"),
    ("random", 37, 238, 4, 3, False, None, 0.05, True, "bootstrap"),
    ("random", 8, 4096 + 70, 2, 17, False, None, 0.03, False, "bootstrap"),
    ("random", 8, 4096 + 70, 2, 33, True, None, 0.03, False, "fractional"),
]


def _segments(e):
    """segments of REWEIGHT_SEGMENT patterns of the engine's pattern axis.  The call's own profile does not report them; a
    counts-only pairwise_distances call does, from the same constant (phyamd_reweight.inc), so a change of the constant shows in the
    tests that rely on it"""
    e.pairwise_distances([[0, 1]], counts_only=True)
    return e.distance_profile()["segments"]


@pytest.mark.parametrize("shape,T,P,C,B,fold,pinv,gaps,ambig,kind", SHARED)
def test_shared_lengths_match_oracle_replicate_by_replicate(shape, T, P, C, B, fold, pinv, gaps, ambig, kind):
    pb = random_problem(T, P, C, seed=7 * T + P + C, shape=shape, gaps=gaps, pinv=pinv)
    if ambig:
        _ambiguous_partials(pb, 3)
    W = _replicates(pb, B, seed=B, kind=kind)
    if P > 1 and kind == "bootstrap":
        assert (W == 0).any()  # replicates that miss patterns
    with engine_from_problem(pb, rescale=RESCALE_AUTO, tip_mode="partials" if ambig else "states") as e:
        lnl, g = e.gradient_batch_weights(W, flags=GRAD_FOLD_ROOT_FREQS if fold else 0)
        prof = e.weight_batch_profile()
        assert prof["items_fast"] == B and prof["items_sequential"] == 0, prof
        assert prof["walks"] == 1 and prof["pattern_chunks"] == 1, prof
        assert not e.rescaling
        assert np.all(g[:, pb.root, :] == 0.0)
        assert P <= 4096 or _segments(e) >= 2  # the rows past 4096 patterns are there for the second segment: fail, not pass, without it
        e.log_likelihood()
        plk = e.pattern_log_likelihoods()
    for b in range(B):  # lnl is the weighted sum of the pattern log-likelihoods of ONE evaluation
        assert abs(lnl[b] - W[b] @ plk) <= 1e-10 * abs(lnl[b]), (b, lnl[b], W[b] @ plk)
    _check_against_oracle(pb, W, lnl, g, fold=fold)


@pytest.mark.parametrize("T,P,C,B", [(37, 238, 4, 17), (3, 700, 1, 64)])
def test_per_item_lengths_match_oracle(T, P, C, B):
    pb = random_problem(T, P, C, seed=7 * T + P + C, gaps=0.05)
    W = _replicates(pb, B, seed=B, keep_first=True)
    bl = _lengths(pb, B, seed=B)
    with engine_from_problem(pb, rescale=RESCALE_AUTO) as e:
        lnl, g = e.gradient_batch_weights(W, bl)
        prof = e.weight_batch_profile()
        assert prof["items_fast"] == B and prof["items_sequential"] == 0 and prof["walks"] == B, prof
        l0, g0 = e.gradient_batch(bl[:1])
        assert e.batch_profile()["items_fast"] == 1
        lo, none = e.gradient_batch_weights(W, bl, want_gradient=False)
        assert none is None and e.weight_batch_profile()["walks"] == B
    assert _bits(lnl[0]) == _bits(l0[0]) and np.array_equal(_bits(g[0]), _bits(g0[0]))  # item 0 carries the engine's own weights
    assert np.array_equal(_bits(lo), _bits(lnl))
    _check_against_oracle(pb, W, lnl, g, bl=bl)


def test_a_replicate_does_not_depend_on_its_batch():
    """shared lengths: replicate x alone, at position 17 of 64, and in a batch cut into >= 3 chunks of replicates by a memory cap:
    the same bits; the lnL-only form returns the same lnL bits; two calls return identical bits"""
    pb = random_problem(37, 700, 4, seed=99, gaps=0.05)
    W = _replicates(pb, 64, seed=5)
    x = W[17]
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        e.gradient()  # (the engine's own buffers are made: what it holds besides the batch scratch)
        held = e.profile()["device_bytes"]
        l1, g1 = e.gradient_batch_weights(x[None, :])
        one = e.weight_batch_profile()
        assert one["item_chunks"] == 1 and one["items_fast"] == 1, one
        l64, g64 = e.gradient_batch_weights(W)
        prof = e.weight_batch_profile()
        assert prof["items_fast"] == 64 and prof["item_chunks"] == 1 and prof["pattern_chunks"] == 1, prof
        again = e.gradient_batch_weights(W)
        lo, none = e.gradient_batch_weights(W, want_gradient=False)
        assert none is None and e.weight_batch_profile()["items_fast"] == 64
    assert _bits(l1[0]) == _bits(l64[17]) and np.array_equal(_bits(g1[0]), _bits(g64[17]))
    assert np.array_equal(_bits(again[0]), _bits(l64)) and np.array_equal(_bits(again[1]), _bits(g64))
    assert np.array_equal(_bits(lo), _bits(l64))
    # a cap with room for 64 / 3.5 replicates beside the walk's arrays.  What one replicate needs for itself is the difference of
    # the two calls' scratch per replicate; the least cap that still takes all 64 at once is found by bisection (the engine keeps a
    # reserve of its own beside what it holds, which no profile reports)
    per_item = (prof["scratch_bytes"] - one["scratch_bytes"]) / 63

    def capped(cap):
        try:
            with engine_from_problem(pb, rescale=RESCALE_NEVER, max_device_bytes=int(cap)) as e:
                e.gradient()
                if e.profile()["tiles"] != 1:
                    return None, None, None
                lc, gc = e.gradient_batch_weights(W)
                return lc, gc, e.weight_batch_profile()
        except EngineError:  # (the cap does not hold the engine, or not one block of the call's scratch)
            return None, None, None

    low, high = held, held + prof["scratch_bytes"] + (8 << 20)
    assert capped(high)[2]["item_chunks"] == 1
    for _ in range(14):
        mid = (low + high) / 2
        p = capped(mid)[2]
        if p is not None and p["item_chunks"] == 1 and p["pattern_chunks"] == 1:
            high = mid
        else:
            low = mid
    lc, gc, prof = capped(high - 64 * per_item * (1 - 1 / 3.5))
    print(prof)
    assert prof["item_chunks"] >= 3 and prof["pattern_chunks"] == 1 and prof["items_fast"] == 64 and prof["items_sequential"] == 0, prof
    assert np.array_equal(_bits(lc), _bits(l64)) and np.array_equal(_bits(gc), _bits(g64))


def test_pattern_chunks_under_a_cap():
    """shared lengths: a cap below the rows of all patterns runs the patterns in >= 3 chunks of whole blocks; the sums agree with
    the uncapped call to the suite's tolerances and the engine stays within the cap"""
    pb = random_problem(37, 700, 4, seed=99, gaps=0.05)
    W = _replicates(pb, 5, seed=8)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        e.gradient()
        held = e.profile()["device_bytes"]
        lnl, g = e.gradient_batch_weights(W)
        prof = e.weight_batch_profile()
        assert prof["pattern_chunks"] == 1, prof
        scratch = prof["scratch_bytes"]
    cap = int(held + scratch / 2.5)  # (the rows of 11 blocks are nearly all of it: room for at most 4 blocks at a time)
    with engine_from_problem(pb, rescale=RESCALE_NEVER, max_device_bytes=cap) as e:
        e.gradient()
        assert e.profile()["tiles"] == 1
        lc, gc = e.gradient_batch_weights(W)
        prof = e.weight_batch_profile()
        print(prof)
        assert prof["pattern_chunks"] >= 3 and prof["walks"] == prof["pattern_chunks"], prof
        assert prof["items_fast"] == 5 and prof["items_sequential"] == 0, prof
        assert e.profile()["device_bytes"] <= cap
    assert np.abs(lc - lnl).max() <= 1e-10 * np.abs(lnl).max()
    assert np.abs(gc - g).max() <= 1e-9 * max(1.0, np.abs(g).max())
    _check_against_oracle(pb, W, lc, gc)


def test_a_pattern_chunk_wider_than_a_segment_under_a_cap():
    """shared lengths, 3 x 4096 + 70 patterns: the largest cap of the ladder that cuts the patterns into at least two chunks of
    more than 4096 patterns on average.  Chunks are equal but for the last, so the first spans at least two segments, with its own
    k0 and Pc and (but by chance) a boundary that is no multiple of a segment.  The oracle at the suite's tolerances, and the
    uncapped call to 1e-12 relative (the bits may depend on the cap: the chunks are added in chunk order)"""
    P = 3 * 4096 + 70
    pb = random_problem(8, P, 2, seed=7 * 8 + P + 2, gaps=0.03)
    W = _replicates(pb, 17, seed=17)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        e.gradient()
        held = e.profile()["device_bytes"]
        lnl, g = e.gradient_batch_weights(W)
        prof = e.weight_batch_profile()
        assert prof["pattern_chunks"] == 1 and prof["items_fast"] == 17, prof
        scratch = prof["scratch_bytes"]
        assert _segments(e) >= 4
    found = None
    for extra in (0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3):
        cap = int(held + extra * scratch)
        with engine_from_problem(pb, rescale=RESCALE_NEVER, max_device_bytes=cap) as e:
            e.gradient()
            assert e.profile()["tiles"] == 1
            lc, gc = e.gradient_batch_weights(W)
            prof = e.weight_batch_profile()
            print(f"cap = held + {extra} x scratch = {cap}: {prof}")
            assert e.profile()["device_bytes"] <= cap
            if prof["pattern_chunks"] >= 2:
                found = prof
                break
    assert found is not None, "no cap cut the patterns"
    assert P / found["pattern_chunks"] > 4096, found  # (else the ladder needs a rung between this cap and the one before)
    assert found["walks"] == found["pattern_chunks"] and found["items_fast"] == 17 and found["items_sequential"] == 0, found
    print(f"against the uncapped call: lnL {np.abs(lc - lnl).max() / np.abs(lnl).max():.3e} relative, "
          f"gradient {np.abs(gc - g).max() / max(1.0, np.abs(g).max()):.3e}")
    assert np.abs(lc - lnl).max() <= 1e-12 * np.abs(lnl).max()
    assert np.abs(gc - g).max() <= 1e-12 * max(1.0, np.abs(g).max())
    _check_against_oracle(pb, W, lc, gc)


def test_the_engine_is_untouched():
    pb = random_problem(37, 700, 4, seed=31, gaps=0.05)
    W = _replicates(pb, 16, seed=2)
    bl = _lengths(pb, 16, seed=2)
    with engine_from_problem(pb, rescale=RESCALE_AUTO) as e:
        before = e.gradient()
        plk = e.pattern_log_likelihoods()
        for lengths in (None, bl):
            e.gradient_batch_weights(W, lengths)
            assert e.weight_batch_profile()["items_fast"] == 16
            after = e.gradient()
            assert _bits(before[0]) == _bits(after[0]) and np.array_equal(_bits(before[1]), _bits(after[1]))
            assert np.array_equal(_bits(plk), _bits(e.pattern_log_likelihoods()))
    with engine_from_problem(pb, rescale=RESCALE_ALWAYS) as e:  # a call that goes item by item: weights and lengths come back
        before = e.gradient()
        for lengths in (None, bl[:3]):
            e.gradient_batch_weights(W[:3], lengths)
            assert e.weight_batch_profile()["items_sequential"] == 3
            after = e.gradient()
            assert _bits(before[0]) == _bits(after[0]) and np.array_equal(_bits(before[1]), _bits(after[1]))


def _fallback(pb, e, B, seed, with_lengths):
    W = _replicates(pb, B, seed=seed)
    bl = _lengths(pb, B, seed=seed) if with_lengths else None
    lnl, g = e.gradient_batch_weights(W, bl)
    prof = e.weight_batch_profile()
    assert prof["items_sequential"] == B and prof["items_fast"] == 0, prof
    return W, bl, lnl, g


@pytest.mark.parametrize("with_lengths", [False, True])
def test_other_state_counts_go_item_by_item(with_lengths):
    pb = random_problem(8, 65, 2, seed=20, S=20, gaps=0.03)
    with engine_from_problem(pb, rescale=RESCALE_AUTO) as e:
        W, bl, lnl, g = _fallback(pb, e, 3, 20, with_lengths)
        ref = pb.log_likelihood()["lnl"]
        assert abs(e.log_likelihood() - ref) <= 1e-10 * abs(ref)  # the engine's weights and lengths are back
    _check_against_oracle(pb, W, lnl, g, bl=bl)


@pytest.mark.parametrize("with_lengths", [False, True])
def test_rescaling_engine_goes_item_by_item(with_lengths):
    pb = random_problem(37, 238, 4, seed=12, gaps=0.03, rescale=1)
    with engine_from_problem(pb, rescale=RESCALE_ALWAYS) as e:
        W, bl, lnl, g = _fallback(pb, e, 4, 1, with_lengths)
    _check_against_oracle(pb, W, lnl, g, bl=bl)


def test_tiled_engine_goes_item_by_item():
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
        W, bl, lnl, g = _fallback(pb, e, 3, 4, False)
    _check_against_oracle(pb, W, lnl, g)


def test_an_empty_tip_mask_goes_item_by_item():
    pb = random_problem(8, 100, 2, seed=23)
    tp = np.zeros((pb.T, pb.P, 4))
    for t in range(pb.T):
        tp[t, np.arange(pb.P), pb.tip_states[t]] = 1.0
    tp[3, 40] = 0.0  # no state is compatible with this cell
    pb.tip_partials, pb.tip_states = tp, None
    with engine_from_problem(pb, rescale=RESCALE_NEVER, tip_mode="partials") as e:
        W, bl, lnl, g = _fallback(pb, e, 3, 2, False)
        for b in range(3):
            e.set_pattern_weights(W[b])
            l, cg = e.gradient()
            assert np.array_equal(lnl[b], l, equal_nan=True) and np.array_equal(g[b], cg, equal_nan=True)


@pytest.mark.parametrize("with_lengths", [False, True])
def test_underflow_switches_an_auto_engine_to_rescaling(with_lengths):
    pb = _deep(800, 100, 4, seed=5)
    with engine_from_problem(pb, rescale=RESCALE_AUTO) as e:
        assert not e.rescaling
        # (no zero weight: 0 * -inf is a NaN, and the lazy switch goes by an infinite lnL alone, treelikelihood.c:1496-1519)
        W = _replicates(pb, 3, seed=8, kind="fractional") + 0.5
        bl = pb.branch_lengths[None, :] * np.random.default_rng(8).uniform(0.9, 1.2, size=(3, pb.N)) if with_lengths else None
        lnl, g = e.gradient_batch_weights(W, bl)
        prof = e.weight_batch_profile()
        assert prof["items_sequential"] == 3 and prof["items_fast"] == 0, prof
        assert e.rescaling
    _check_against_oracle(pb, W, lnl, g, bl=bl)


@pytest.mark.parametrize("with_lengths", [False, True])
def test_underflow_is_reported_in_band_without_rescaling(with_lengths):
    pb = _deep(800, 100, 4, seed=5)
    W = _replicates(pb, 3, seed=8, kind="fractional") + 0.5  # (no zero weight: 0 * -inf would be a NaN, not an inf)
    bl = pb.branch_lengths[None, :] * np.random.default_rng(8).uniform(0.9, 1.2, size=(3, pb.N)) if with_lengths else None
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        lnl, g = e.gradient_batch_weights(W, bl)
        prof = e.weight_batch_profile()
        assert prof["items_fast"] == 3 and prof["items_sequential"] == 0, prof
        assert not e.rescaling
    assert not np.any(np.isfinite(lnl)) and np.all(np.isnan(g))


def test_refusals():
    pb = random_problem(8, 100, 2, seed=3)
    W = _replicates(pb, 4, seed=1)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        before = e.gradient()
        for bad in (-1.0, np.nan, np.inf):
            V = W.copy()
            V[2, 17] = bad
            with pytest.raises(EngineError) as err:
                e.gradient_batch_weights(V)
            assert err.value.code == EINVAL
            assert "phyamd_gradient_batch_weights" in str(err.value) and "weights" in str(err.value) and "item 2" in str(err.value), str(err.value)
        after = e.gradient()
        assert _bits(before[0]) == _bits(after[0]) and np.array_equal(_bits(before[1]), _bits(after[1]))
        e.set_node_matrices(2, e.node_matrices(2))
        with pytest.raises(EngineError) as err:
            e.gradient_batch_weights(W, _lengths(pb, 4, seed=1))
        assert err.value.code == EUNSUPPORTED
        lnl, g = e.gradient_batch_weights(W)  # the engine's own lengths: its matrices serve as they are
        assert e.weight_batch_profile()["items_fast"] == 4
    _check_against_oracle(pb, W, lnl, g)


@pytest.mark.parametrize("devices", [[0], [0, 0], [0, 0, 0, 0]])
def test_shards_agree_with_one_engine(devices):
    """every shard takes its own pattern columns of the weight rows; per-item results are added in shard order: equal to 1e-12
    relative (the comparison of tests/test_batch_gpu.py)"""
    pb = random_problem(37, 700, 4, seed=21, gaps=0.05)
    W = _replicates(pb, 8, seed=6)
    bl = _lengths(pb, 8, seed=6)
    with engine_from_problem(pb, rescale=RESCALE_AUTO) as e:
        lnl, g = e.gradient_batch_weights(W)
        lnl_i, g_i = e.gradient_batch_weights(W, bl)
    with engine_from_problem(pb, rescale=RESCALE_AUTO, devices=devices) as e:
        assert e.shard_count == len(devices)
        ls, gs = e.gradient_batch_weights(W)
        prof = e.weight_batch_profile()
        assert prof["items_fast"] == 8 and prof["items_sequential"] == 0 and prof["walks"] == 1, prof
        lo, _ = e.gradient_batch_weights(W, want_gradient=False)
        li, gi = e.gradient_batch_weights(W, bl)
        prof = e.weight_batch_profile()
        assert prof["items_fast"] == 8 and prof["walks"] == 8, prof
    assert np.abs(ls - lnl).max() <= 1e-12 * np.abs(lnl).max()
    assert np.abs(lo - lnl).max() <= 1e-12 * np.abs(lnl).max()
    assert np.abs(gs - g).max() <= 1e-12 * max(1.0, np.abs(g).max())
    assert np.abs(li - lnl_i).max() <= 1e-12 * np.abs(lnl_i).max()
    assert np.abs(gi - g_i).max() <= 1e-12 * max(1.0, np.abs(g_i).max())
