"""GPU: phyamd_gradient_batch -- lnL and the per-category branch gradient of many branch-length vectors in one call -- against the
CPU oracle item by item, against a reference fixture, bit for bit across batch sizes, positions and chunks, and through every
defined fallback.  Tolerances are the suite's for single evaluations: lnL 1e-10 relative, gradient 1e-9 * max(1, max|g|).
Every parity case also asserts that all items took the batched walk (items_fast == B): a silent fallback must not pass."""
import copy

import numpy as np
import pytest

from golden_util import load, oracle_problem, read_spec
from gpu_util import engine_from_problem, random_problem
from physher_amd.engine import GRAD_FOLD_ROOT_FREQS, RESCALE_ALWAYS, RESCALE_AUTO, RESCALE_NEVER, EngineError

pytestmark = pytest.mark.gpu
EUNSUPPORTED = -4


def _lengths(pb, B, seed, keep_first=False):
    """B branch-length vectors around the problem's own (item 0: exactly those if keep_first)"""
    rng = np.random.default_rng(seed)
    bl = pb.branch_lengths[None, :] * rng.uniform(0.5, 1.8, size=(B, pb.N))
    if keep_first:
        bl[0] = pb.branch_lengths
    return np.ascontiguousarray(bl)


def _oracle(pb, lengths, fold=False):
    q = copy.copy(pb)
    q.branch_lengths = np.ascontiguousarray(lengths, dtype=np.float64)
    q.fold_root_freqs = 1 if fold else 0
    return q.gradient()


def _check_against_oracle(pb, bl, lnl, g, fold=False):
    for b in range(len(bl)):
        ref = _oracle(pb, bl[b], fold)
        print(f"item {b}: lnL {lnl[b]!r} oracle {ref['lnl']!r}  max|dg| {np.abs(g[b] - ref['cat_grad']).max():.3e}")
        assert abs(lnl[b] - ref["lnl"]) <= 1e-10 * abs(ref["lnl"]), (b, lnl[b], ref["lnl"])
        assert np.abs(g[b] - ref["cat_grad"]).max() <= 1e-9 * max(1.0, np.abs(ref["cat_grad"]).max()), b


def _ambiguous_partials(pb, seed):
    rng = np.random.default_rng(seed)
    tp = np.zeros((pb.T, pb.P, 4))
    for t in range(pb.T):
        s = pb.tip_states[t]
        for k in range(pb.P):
            if s[k] >= 4:
                tp[t, k] = 1.0
            else:
                tp[t, k, s[k]] = 1.0
                if rng.random() < 0.05:  # a two-state ambiguity code (R, Y, ...)
                    tp[t, k, (s[k] + 1 + rng.integers(3)) % 4] = 1.0
    pb.tip_partials, pb.tip_states = tp, None


# (shape, T, P, C, B, fold, pinv, gaps, ambiguity codes)
CASES = [
    ("random", 2, 1, 1, 1, False, None, 0.0, False),
    ("caterpillar", 3, 63, 2, 3, True, None, 0.0, False),
    ("random", 3, 700, 1, 64, False, None, 0.05, False),
    ("random", 37, 238, 4, 64, False, None, 0.05, False),
    ("caterpillar", 37, 700, 5, 3, False, None, 0.0, False),
    ("random", 37, 700, 4, 3, False, 0.25, 0.03, False),
    ("random", 37, 238, 4, 3, True, None, 0.05, True),
    ("random", 200, 238, 8, 3, True, None, 0.02, False),
    ("caterpillar", 200, 63, 4, 200, False, None, 0.02, False),
    ("random", 200, 1, 2, 64, False, None, 0.0, False),
]


@pytest.mark.parametrize("shape,T,P,C,B,fold,pinv,gaps,ambig", CASES)
def test_matches_oracle_item_by_item(shape, T, P, C, B, fold, pinv, gaps, ambig):
    pb = random_problem(T, P, C, seed=7 * T + P + C, shape=shape, gaps=gaps, pinv=pinv)
    if ambig:
        _ambiguous_partials(pb, 3)
    bl = _lengths(pb, B, seed=B)
    with engine_from_problem(pb, rescale=RESCALE_AUTO, tip_mode="partials" if ambig else "states") as e:
        lnl, g = e.gradient_batch(bl, GRAD_FOLD_ROOT_FREQS if fold else 0)
        prof = e.batch_profile()
        assert prof["items_fast"] == B and prof["items_sequential"] == 0, prof
        assert not e.rescaling
        assert np.all(g[:, pb.root, :] == 0.0)
    _check_against_oracle(pb, bl, lnl, g, fold)


def test_matches_reference_fixture():
    case = "gtr_g4_t16"
    gold = load(case)
    pb = oracle_problem(case, gold)
    N = gold["node_count"]
    bl = _lengths(pb, 5, seed=16, keep_first=True)
    from oracle import phyoracle as po
    with engine_from_problem(pb, rescale=RESCALE_AUTO, tip_mode="states" if read_spec(case)["tipstates"] == "1" else "partials") as e:
        lnl, cg = e.gradient_batch(bl)
        prof = e.batch_profile()
        assert prof["items_fast"] == 5 and prof["items_sequential"] == 0, prof
    assert abs(lnl[0] - gold["lnl"]) <= 1e-10 * abs(gold["lnl"])
    ref = gold["gradient_all"][:N]
    g = po.branch_gradient_from_cat(cg[0], gold["cat_rates_without_mu"], gold["cat_proportions"], zero_node=gold["right"][gold["root"]])
    assert np.abs(g - ref).max() <= 1e-9 * max(1.0, np.abs(ref[np.isfinite(ref)]).max())
    _check_against_oracle(pb, bl[1:], lnl[1:], cg[1:])


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_an_item_does_not_depend_on_its_batch():
    """item x alone, at position 17 of 64, and in a batch cut into >= 3 chunks by a memory cap: the same bits; the lnL-only form
    returns the same lnL bits"""
    pb = random_problem(37, 700, 4, seed=99, gaps=0.05)
    bl = _lengths(pb, 64, seed=5)
    x = bl[17]
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        e.gradient()  # (the engine's own buffers are made: what it holds besides the batch scratch)
        held = e.profile()["device_bytes"]
        l1, g1 = e.gradient_batch(x[None, :])
        assert e.batch_profile()["chunks"] == 1
        l64, g64 = e.gradient_batch(bl)
        prof = e.batch_profile()
        assert prof["items_fast"] == 64 and prof["chunks"] == 1, prof
        scratch = prof["scratch_bytes"]
        lo, none = e.gradient_batch(bl, want_gradient=False)
        assert none is None and e.batch_profile()["items_fast"] == 64
    assert _bits(l1[0]) == _bits(l64[17]) and np.array_equal(_bits(g1[0]), _bits(g64[17]))
    assert np.array_equal(_bits(lo), _bits(l64))
    with engine_from_problem(pb, rescale=RESCALE_NEVER, max_device_bytes=int(held + scratch / 3.5)) as e:
        e.gradient()
        assert e.profile()["tiles"] == 1
        lc, gc = e.gradient_batch(bl)
        prof = e.batch_profile()
        assert prof["chunks"] >= 3 and prof["items_fast"] == 64 and prof["items_sequential"] == 0, prof
    assert np.array_equal(_bits(lc), _bits(l64)) and np.array_equal(_bits(gc), _bits(g64))


def test_the_engine_is_untouched():
    pb = random_problem(37, 700, 4, seed=31, gaps=0.05)
    bl = _lengths(pb, 16, seed=2)
    node = 5 if pb.root != 5 else 6
    with engine_from_problem(pb, rescale=RESCALE_AUTO) as e, engine_from_problem(pb, rescale=RESCALE_AUTO) as fresh:
        before = e.gradient()
        plk = e.pattern_log_likelihoods()
        e.gradient_batch(bl)
        assert e.batch_profile()["items_fast"] == 16
        after = e.gradient()
        assert _bits(before[0]) == _bits(after[0]) and np.array_equal(_bits(before[1]), _bits(after[1]))
        assert np.array_equal(_bits(plk), _bits(e.pattern_log_likelihoods()))
        fresh.gradient()
        e.gradient_batch(bl[:3])
        for eng in (e, fresh):
            eng.set_branch_length(node, 0.37)
        a, b = e.gradient(), fresh.gradient()
        assert _bits(a[0]) == _bits(b[0]) and np.array_equal(_bits(a[1]), _bits(b[1]))
        assert _bits(e.log_likelihood()) == _bits(fresh.log_likelihood())


@pytest.mark.parametrize("S,T,P,C", [(20, 10, 200, 2), (61, 6, 100, 1)])
def test_other_state_counts_go_item_by_item(S, T, P, C):
    pb = random_problem(T, P, C, seed=S, S=S, gaps=0.03)
    bl = _lengths(pb, 3, seed=S)
    with engine_from_problem(pb, rescale=RESCALE_AUTO) as e:
        lnl, g = e.gradient_batch(bl)
        prof = e.batch_profile()
        assert prof["items_sequential"] == 3 and prof["items_fast"] == 0, prof
        assert abs(e.log_likelihood() - pb.log_likelihood()["lnl"]) <= 1e-10 * abs(pb.log_likelihood()["lnl"])  # the engine's lengths are back
    _check_against_oracle(pb, bl, lnl, g)


def test_rescaling_engine_goes_item_by_item():
    pb = random_problem(37, 238, 4, seed=12, gaps=0.03, rescale=1)
    bl = _lengths(pb, 4, seed=1)
    with engine_from_problem(pb, rescale=RESCALE_ALWAYS) as e:
        lnl, g = e.gradient_batch(bl)
        prof = e.batch_profile()
        assert prof["items_sequential"] == 4 and prof["items_fast"] == 0, prof
    _check_against_oracle(pb, bl, lnl, g)


def test_tiled_engine_goes_item_by_item():
    pb = random_problem(40, 2000, 4, seed=13, gaps=0.03)
    bl = _lengths(pb, 3, seed=4)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        e.gradient()
        base = e.profile()["device_bytes"]
    cap = None
    for frac in np.arange(0.9, 0.1, -0.05):  # (the search of tests/test_branch_hessian_gpu.py for a cap that tiles)
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
        lnl, g = e.gradient_batch(bl)
        prof = e.batch_profile()
        assert prof["items_sequential"] == 3 and prof["items_fast"] == 0, prof
    _check_against_oracle(pb, bl, lnl, g)


def _deep(T, P, C, seed, **kw):
    """the recipe of tests/test_branch_hessian_gpu.py: a caterpillar deep enough that the partials underflow without rescaling"""
    return random_problem(T, P, C, seed=seed, shape="caterpillar", bl=(0.5, 1.5), rescale=1, **kw)


def test_underflowing_items_switch_an_auto_engine_to_rescaling():
    pb = _deep(800, 100, 4, seed=5)
    bl = pb.branch_lengths[None, :] * np.random.default_rng(8).uniform(0.9, 1.2, size=(3, pb.N))
    with engine_from_problem(pb, rescale=RESCALE_AUTO) as e:
        assert not e.rescaling
        lnl, g = e.gradient_batch(bl)
        prof = e.batch_profile()
        assert prof["items_sequential"] == 3 and prof["items_fast"] == 0, prof
        assert e.rescaling
    _check_against_oracle(pb, bl, lnl, g)


def test_underflowing_items_are_reported_in_band_without_rescaling():
    pb = _deep(800, 100, 4, seed=5)
    bl = pb.branch_lengths[None, :] * np.random.default_rng(8).uniform(0.9, 1.2, size=(3, pb.N))
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        lnl, g = e.gradient_batch(bl)
        prof = e.batch_profile()
        assert prof["items_fast"] == 3 and prof["items_sequential"] == 0, prof
        assert not np.any(np.isfinite(lnl)) and np.all(np.isnan(g))


def test_explicit_matrices_are_refused():
    pb = random_problem(8, 100, 2, seed=3)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        e.gradient()
        e.set_node_matrices(2, e.node_matrices(2))
        with pytest.raises(EngineError) as err:
            e.gradient_batch(_lengths(pb, 2, seed=1))
        assert err.value.code == EUNSUPPORTED


@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0, 0]])
def test_shards_agree_with_one_engine(devices):
    """per-item results are added in shard order (pairwise for 2 / 4 shards, like phyamd_gradient's): equal to 1e-12 relative"""
    pb = random_problem(37, 700, 4, seed=21, gaps=0.05)
    bl = _lengths(pb, 8, seed=6)
    with engine_from_problem(pb, rescale=RESCALE_AUTO) as e:
        lnl, g = e.gradient_batch(bl)
    with engine_from_problem(pb, rescale=RESCALE_AUTO, devices=devices) as e:
        ls, gs = e.gradient_batch(bl)
        prof = e.batch_profile()
        assert prof["items_fast"] == 8 and prof["items_sequential"] == 0, prof
        lo, _ = e.gradient_batch(bl, want_gradient=False)
    assert np.abs(ls - lnl).max() <= 1e-12 * np.abs(lnl).max()
    assert np.abs(lo - lnl).max() <= 1e-12 * np.abs(lnl).max()
    assert np.abs(gs - g).max() <= 1e-12 * max(1.0, np.abs(g).max())


def test_capped_engine_is_untouched_by_a_chunked_batch_made_first():
    """under max_device_bytes the batch scratch yields to the engine: a batch cut into >= 3 chunks BEFORE any other evaluation, then
    gradient() and the Hessian diagonal succeed within the cap with the bits of a capped engine that never made the call"""
    pb = random_problem(37, 700, 4, seed=99, gaps=0.05)
    bl = _lengths(pb, 64, seed=5)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        e.gradient()
        e.branch_hessian_diagonal()
        held = e.profile()["device_bytes"]
        l64, g64 = e.gradient_batch(bl)
        scratch = e.batch_profile()["scratch_bytes"]
    cap = int(held + scratch / 3.5)
    with engine_from_problem(pb, rescale=RESCALE_NEVER, max_device_bytes=cap) as fresh, \
            engine_from_problem(pb, rescale=RESCALE_NEVER, max_device_bytes=cap) as e:
        assert e.profile()["tiles"] == 1
        lc, gc = e.gradient_batch(bl)
        prof = e.batch_profile()
        assert prof["chunks"] >= 3 and prof["items_fast"] == 64 and prof["items_sequential"] == 0, prof
        assert e.profile()["device_bytes"] <= cap
        assert np.array_equal(_bits(lc), _bits(l64)) and np.array_equal(_bits(gc), _bits(g64))
        a, b = e.gradient(), fresh.gradient()
        assert _bits(a[0]) == _bits(b[0]) and np.array_equal(_bits(a[1]), _bits(b[1]))
        ha, hb = e.branch_hessian_diagonal(), fresh.branch_hessian_diagonal()
        assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(ha, hb))
        assert e.profile()["device_bytes"] <= cap
        lc, gc = e.gradient_batch(bl)  # and the batch again, beside the engine's buffers
        assert e.batch_profile()["items_fast"] == 64 and e.profile()["device_bytes"] <= cap
        assert np.array_equal(_bits(lc), _bits(l64)) and np.array_equal(_bits(gc), _bits(g64))


def test_underflowing_items_under_a_cap():
    """RESCALE_AUTO under max_device_bytes: the item that underflows in the first chunk goes through the ordinary path, whose
    buffers (uppers, scale factors of the lazy switch) get the scratch's room"""
    pb = _deep(800, 100, 4, seed=5)
    bl = pb.branch_lengths[None, :] * np.random.default_rng(8).uniform(0.9, 1.2, size=(6, pb.N))
    with engine_from_problem(pb, rescale=RESCALE_AUTO) as e:
        e.gradient()
        assert e.rescaling
        held = e.profile()["device_bytes"]
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        e.gradient_batch(bl[:3])
        item = e.batch_profile()["scratch_bytes"] / 3
    with engine_from_problem(pb, rescale=RESCALE_AUTO, max_device_bytes=int(held + 4 * item)) as e:
        assert e.profile()["tiles"] == 1
        lnl, g = e.gradient_batch(bl)
        prof = e.batch_profile()
        assert prof["chunks"] >= 1 and prof["items_sequential"] == 6 and prof["items_fast"] == 0, prof
        assert e.rescaling
    _check_against_oracle(pb, bl, lnl, g)


def test_pattern_bound_of_the_fast_path(monkeypatch):
    """more than 8192 patterns: the items go one by one (the loop is faster there); with the bound lifted -- the switch of the
    crossover sweep -- the batched walk serves the same problem"""
    pb = random_problem(8, 8256, 2, seed=17, gaps=0.02)
    bl = _lengths(pb, 2, seed=9)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        lnl, g = e.gradient_batch(bl)
        prof = e.batch_profile()
        assert prof["items_sequential"] == 2 and prof["items_fast"] == 0, prof
    _check_against_oracle(pb, bl, lnl, g)
    monkeypatch.setenv("PHYAMD_BATCH_MAX_PATTERNS", "100000")
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        lnl, g = e.gradient_batch(bl)
        prof = e.batch_profile()
        assert prof["items_fast"] == 2 and prof["items_sequential"] == 0, prof
    _check_against_oracle(pb, bl, lnl, g)


def test_an_empty_tip_mask_goes_item_by_item():
    pb = random_problem(8, 100, 2, seed=23)
    tp = np.zeros((pb.T, pb.P, 4))
    for t in range(pb.T):
        tp[t, np.arange(pb.P), pb.tip_states[t]] = 1.0
    tp[3, 40] = 0.0  # no state is compatible with this cell
    pb.tip_partials, pb.tip_states = tp, None
    bl = _lengths(pb, 3, seed=2)
    with engine_from_problem(pb, rescale=RESCALE_NEVER, tip_mode="partials") as e:
        lnl, g = e.gradient_batch(bl)
        prof = e.batch_profile()
        assert prof["items_sequential"] == 3 and prof["items_fast"] == 0, prof
        for b in range(3):
            e.set_branch_lengths(bl[b])
            l, cg = e.gradient()
            assert np.array_equal(lnl[b], l, equal_nan=True) and np.array_equal(g[b], cg, equal_nan=True)
