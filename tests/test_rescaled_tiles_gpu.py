"""GPU: rescaled evaluations where the engine's two rescaling conventions meet -- pattern tiles, memory caps, shards -- and the
+I root term, against the CPU oracle.

A rescaled 4-state evaluation of the streamed walks scales every category by its own powers of two (SCALE == 2: the stored
lowers are in the CarriedExp2 form, the root's categories in different units, exponents in d_Ec).  Everything else uses one
scale factor per pattern, shared by the categories, as the reference does.  Every problem here that claims to exercise
SCALE == 2 first asserts, from the oracle, that the walks' exponents must differ between categories (assert_real_exponents).

The +I term is read from FRESH engines: a pass that needs the reference's form turns the streamed walks' own forms off for good,
so only the first evaluations of an engine show whether a reader got the form it expects.
"""
import functools

import numpy as np
import pytest

from gpu_util import engine_from_problem, random_problem
from oracle import phyoracle as po
from physher_amd.engine import RESCALE_ALWAYS, RESCALE_AUTO, RESCALE_NEVER, EngineError

pytestmark = pytest.mark.gpu

ENOMEM = -3
GAP4 = 4 + 13  # the tip code random_problem(gaps=...) writes for 4 states: no data (every state allowed)
ORACLE_RESCALE = {RESCALE_NEVER: 0, RESCALE_ALWAYS: 1, RESCALE_AUTO: 2}
ENVS = {"default": {}, "no_exp2": {"PHYAMD_SCALE_EXP2": "0"}, "no_tform": {"PHYAMD_STREAM_TFORM": "0"}}


def _variant(pb, **kw):
    """pb with some fields replaced (tip_states, weights, rescale)"""
    f = dict(tip_states=pb.tip_states, weights=pb.weights, rescale=pb.rescale)
    f.update(kw)
    return po.Problem(pb.left, pb.right, pb.root, f["weights"], pb.eval, pb.evec, pb.ivec, pb.freqs, pb.cat_rates, pb.cat_props, pb.branch_lengths,
                      tip_states=f["tip_states"], rescale=f["rescale"])


def _with_constant_patterns(pb, every=8):
    """every `every`-th pattern made constant (one state at every tip with data): at those the invariant class holds most of the
    root site likelihood, in units of its own, while the other categories of a deep tree are far below it"""
    states = pb.tip_states.copy()
    cols = np.arange(0, pb.P, every)
    sub = states[:, cols]
    states[:, cols] = np.where(sub < pb.S, (cols % pb.S).astype(np.uint8)[None, :], sub)
    return _variant(pb, tip_states=states)


def assert_real_exponents(pb):
    """For some pattern, two categories' root site likelihoods lie more than 2^140 apart.  Partial entries are <= 1, so the smaller
    one has fallen below the 1e-40 threshold somewhere on its way to the root while the larger one need not have: the
    power-of-two walks give the two categories different exponents.  Each category is evaluated as a problem of its own (with
    its own scale factors), so that none is lost to underflow beside the others."""
    logs = np.array([po.Problem(pb.left, pb.right, pb.root, pb.weights, pb.eval, pb.evec, pb.ivec, pb.freqs, pb.cat_rates[c:c + 1], [1.0],
                                pb.branch_lengths, tip_states=pb.tip_states, rescale=1).log_likelihood()["pattern_lk"] for c in range(pb.C)])
    logs = np.where(np.isfinite(logs), logs, np.nan)
    spread = np.nanmax(logs, axis=0) - np.nanmin(logs, axis=0)
    assert np.nanmax(spread) > 140 * np.log(2.0), f"precondition: categories at most 2^{np.nanmax(spread) / np.log(2.0):.0f} apart"


def _per_tile(P, tiles):
    return ((P + tiles - 1) // tiles + 255) // 256 * 256


def _untiled_bytes(pb, rescale, evaluated=True):
    """device_bytes of an untiled engine, before any evaluation or after a gradient (which makes the buffers made on demand)"""
    with engine_from_problem(pb, rescale=rescale) as whole:
        assert whole.profile()["tiles"] == 1
        if evaluated:
            whole.gradient()
        return whole.profile()["device_bytes"]


def _tiling_cap(pb, rescale, base, **kw):
    """the largest cap, in steps of 5 % of `base` from 1.5 base down, at which the engine is built in two tiles or more (smaller
    caps may be refused at construction: that is allowed, an error inside an evaluation is not)"""
    for frac in np.arange(1.5, 0.1, -0.05):
        cap = int(frac * base)
        try:
            with engine_from_problem(pb, rescale=rescale, max_device_bytes=cap, **kw) as e:
                if e.profile()["tiles"] >= 2:
                    return cap
        except EngineError as err:
            assert err.code == ENOMEM, str(err)
    pytest.fail("no cap puts this problem into tiles")


def _close(a, b, rel):
    return abs(a - b) <= rel * max(1.0, abs(b))


# ---------------------------------------------------------------------------------------------------------
# (a) the +I root term against the oracle: untiled and tiled, fresh engines, three reading points
# ---------------------------------------------------------------------------------------------------------
CASES = {
    # name: (S, T, P, C, shape, branch lengths, pinv, engine rescaling, real exponents)
    "4s_deep_always_c4": (4, 300, 1237, 4, "random", (0.3, 0.9), 0.2, RESCALE_ALWAYS, True),
    "4s_caterpillar_auto_c5": (4, 650, 1100, 5, "caterpillar", (0.5, 1.5), 0.15, RESCALE_AUTO, True),
    "4s_deep_auto_c2": (4, 650, 999, 2, "random", (0.5, 1.5), 0.3, RESCALE_AUTO, True),
    "4s_shallow_never_c2": (4, 40, 2777, 2, "random", (0.01, 0.1), 0.25, RESCALE_NEVER, False),
    "20s_deep_auto_c4": (20, 300, 500, 4, "random", (0.5, 1.5), 0.2, RESCALE_AUTO, False),
    "61s_always_c2": (61, 40, 1201, 2, "random", (0.3, 0.9), 0.3, RESCALE_ALWAYS, False),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    S, T, P, C, shape, bl, pinv, rescale, real = CASES[name]
    pb = _with_constant_patterns(random_problem(T, P, C, seed=600 + T + P + S, S=S, shape=shape, gaps=0.03, bl=bl, rescale=ORACLE_RESCALE[rescale], pinv=pinv))
    if real:
        assert_real_exponents(pb)
    ref = pb.log_likelihood()
    if rescale == RESCALE_AUTO:
        assert ref["rescaled"], "precondition: the unscaled likelihood underflows"
    return pb, ref["lnl"], po.root_invariant_term(pb), _untiled_bytes(pb, rescale)


READINGS = {
    "after_lnl": lambda e: e.log_likelihood(),
    "after_gradient": lambda e: e.gradient()[0],
    "after_second_evaluation": lambda e: (e.log_likelihood(), e.gradient()[0])[1],
}


def _check_invariant_term(pb, rescale, lnl_ref, term_ref, **kw):
    for reading, evaluate in READINGS.items():
        with engine_from_problem(pb, rescale=rescale, **kw) as e:
            if "max_device_bytes" in kw:
                assert e.profile()["tiles"] >= 2
            lnl = evaluate(e)
            assert abs(lnl - lnl_ref) <= 1e-10 * abs(lnl_ref), reading
            term = e.root_invariant_term()
            assert _close(term, term_ref, 1e-10), (reading, term, term_ref)
            if "max_device_bytes" in kw:
                assert e.profile()["device_bytes"] <= kw["max_device_bytes"]


@pytest.mark.parametrize("env", list(ENVS))
@pytest.mark.parametrize("name", [n for n in CASES if CASES[n][0] == 4])
def test_invariant_term_of_4_state_engines_matches_oracle(monkeypatch, name, env):
    for k, v in ENVS[env].items():
        monkeypatch.setenv(k, v)
    pb, lnl_ref, term_ref, untiled_bytes = _case(name)
    rescale = CASES[name][7]
    _check_invariant_term(pb, rescale, lnl_ref, term_ref)
    _check_invariant_term(pb, rescale, lnl_ref, term_ref, max_device_bytes=_tiling_cap(pb, rescale, untiled_bytes))


@pytest.mark.parametrize("name", [n for n in CASES if CASES[n][0] != 4])
def test_invariant_term_of_generic_engines_matches_oracle(name):
    """20 and 61 states: the planes layout [C][S][Pp] with padded Pp, a ragged last tile.  Under RESCALE_AUTO the lazy switch
    rebuilds the schedule without fusion or tree walk inside a tile: the tiles are sized for that schedule too."""
    pb, lnl_ref, term_ref, untiled_bytes = _case(name)
    rescale = CASES[name][7]
    _check_invariant_term(pb, rescale, lnl_ref, term_ref)
    _check_invariant_term(pb, rescale, lnl_ref, term_ref, max_device_bytes=_tiling_cap(pb, rescale, untiled_bytes))


# ---------------------------------------------------------------------------------------------------------
# (b) tiled rescaled evaluations with real exponents
# ---------------------------------------------------------------------------------------------------------
EASY = 900  # leading patterns that do not underflow unscaled


@functools.lru_cache(maxsize=None)
def _ordered_problem():
    """T = 700, C = 4, deep.  The first EASY patterns keep the data of 30 tips only (the others unknown): unscaled they do not
    underflow, so under RESCALE_AUTO the first tile runs unscaled and the lazy switch fires in a later one."""
    pb = random_problem(700, 2000, 4, seed=4242, gaps=0.02, bl=(0.5, 1.5), rescale=1)
    states = pb.tip_states.copy()
    keep = np.random.default_rng(1).choice(pb.T, size=30, replace=False)
    hide = np.ones(pb.T, dtype=bool)
    hide[keep] = False
    states[np.ix_(hide, np.arange(EASY))] = GAP4
    pb = _variant(pb, tip_states=states)
    assert_real_exponents(pb)
    assert np.isfinite(_variant(pb, tip_states=states[:, :EASY], weights=pb.weights[:EASY], rescale=0).log_likelihood()["lnl"])
    assert not np.isfinite(_variant(pb, rescale=0).log_likelihood()["lnl"])
    return pb, pb.gradient(), _untiled_bytes(pb, RESCALE_ALWAYS)


@pytest.mark.parametrize("rescale", [RESCALE_ALWAYS, RESCALE_AUTO])
def test_tiled_rescaled_evaluations_with_real_exponents(rescale):
    pb, ref, untiled_bytes = _ordered_problem()
    tol = 1e-9 * max(1.0, np.abs(ref["cat_grad"]).max())
    with engine_from_problem(pb, rescale=rescale, max_device_bytes=int(0.4 * untiled_bytes)) as e:
        tiles = e.profile()["tiles"]
        assert tiles >= 2 and _per_tile(pb.P, tiles) <= EASY < pb.P, tiles
        lnl, cg = e.gradient()  # (no flags: the streamed pre-order walk in its power-of-two form)
        assert abs(lnl - ref["lnl"]) <= 1e-10 * abs(ref["lnl"])
        np.testing.assert_allclose(e.pattern_log_likelihoods(), ref["pattern_lk"], rtol=1e-11, atol=1e-11)
        assert np.abs(cg - ref["cat_grad"]).max() <= tol
        lnl2, cg2 = e.gradient()
        assert abs(lnl2 - ref["lnl"]) <= 1e-10 * abs(ref["lnl"]) and np.abs(cg2 - ref["cat_grad"]).max() <= tol
        if rescale == RESCALE_ALWAYS:
            assert lnl2 == lnl and np.array_equal(cg2, cg)
        lnl3, cg3 = e.gradient()
        assert lnl3 == lnl2 and np.array_equal(cg3, cg2)
        assert e.log_likelihood() == lnl2
        np.testing.assert_allclose(e.pattern_log_likelihoods(), ref["pattern_lk"], rtol=1e-11, atol=1e-11)
        assert e.rescaling
        assert e.profile()["device_bytes"] <= int(0.4 * untiled_bytes)


# ---------------------------------------------------------------------------------------------------------
# (c) a sweep of memory caps: refused at construction, or every call succeeds within the cap and matches the oracle
# ---------------------------------------------------------------------------------------------------------
SWEEP = {
    "always": (300, 1500, (0.3, 0.9), RESCALE_ALWAYS, True),
    "auto_switching": (650, 1000, (0.5, 1.5), RESCALE_AUTO, True),
    "never": (60, 1500, (0.01, 0.1), RESCALE_NEVER, False),
}


@pytest.mark.parametrize("name", list(SWEEP))
def test_memory_cap_sweep(name):
    T, P, bl, rescale, real = SWEEP[name]
    pb = _with_constant_patterns(random_problem(T, P, 4, seed=7000 + T + P, gaps=0.03, bl=bl, rescale=ORACLE_RESCALE[rescale], pinv=0.25))
    if real:
        assert_real_exponents(pb)
    ref = pb.gradient()
    assert ref["rescaled"] == (rescale != RESCALE_NEVER)
    term_ref = po.root_invariant_term(pb)
    dQ = np.random.default_rng(5).normal(size=(2, 4, 4))
    dQ -= dQ.sum(axis=2, keepdims=True) * np.eye(4)[None]
    _, pg_ref = po.parameter_gradient(pb, dQ)
    gtol = 1e-9 * max(1.0, np.abs(ref["cat_grad"]).max())
    untiled_bytes = _untiled_bytes(pb, rescale, evaluated=False)
    accepted, tiled = 0, 0
    for frac in np.linspace(0.2, 1.0, 10):
        cap = int(frac * untiled_bytes)
        try:
            e = engine_from_problem(pb, rescale=rescale, max_device_bytes=cap)
        except EngineError as err:
            assert err.code == ENOMEM, (frac, str(err))
            continue
        with e:
            accepted += 1
            tiled += e.profile()["tiles"] >= 2
            where = (frac, e.profile()["tiles"])
            lnl = e.log_likelihood()
            assert abs(lnl - ref["lnl"]) <= 1e-10 * abs(ref["lnl"]), where
            assert e.profile()["device_bytes"] <= cap, where
            lnl, cg = e.gradient()
            assert abs(lnl - ref["lnl"]) <= 1e-10 * abs(ref["lnl"]) and np.abs(cg - ref["cat_grad"]).max() <= gtol, where
            assert e.profile()["device_bytes"] <= cap, where
            assert _close(e.root_invariant_term(), term_ref, 1e-10), where
            assert e.profile()["device_bytes"] <= cap, where
            e.set_rate_matrix_derivatives(dQ)
            lnl, cg, pg = e.parameter_gradient()
            assert abs(lnl - ref["lnl"]) <= 1e-10 * abs(ref["lnl"]) and np.abs(cg - ref["cat_grad"]).max() <= gtol, where
            assert np.abs(pg - pg_ref).max() <= 1e-8 * max(1.0, np.abs(pg_ref).max()), where
            assert e.profile()["device_bytes"] <= cap, where
            assert e.rescaling == (rescale != RESCALE_NEVER)
    assert accepted >= 3 and tiled >= 2, (accepted, tiled)


def test_memory_cap_sweep_20_states_lazy_switch():
    """20 states under RESCALE_AUTO: the lazy switch inside a tile rebuilds the schedule without fringe fusion or tree walk, which
    stores more nodes and upper slots.  Every cap the engine accepts must hold that schedule too."""
    pb, lnl_ref, term_ref, untiled_bytes = _case("20s_deep_auto_c4")
    accepted, tiled = 0, 0
    for frac in np.linspace(0.2, 1.0, 9):
        cap = int(frac * untiled_bytes)
        try:
            e = engine_from_problem(pb, rescale=RESCALE_AUTO, max_device_bytes=cap)
        except EngineError as err:
            assert err.code == ENOMEM, (frac, str(err))
            continue
        with e:
            accepted += 1
            tiled += e.profile()["tiles"] >= 2
            lnl, _ = e.gradient()
            assert e.rescaling and abs(lnl - lnl_ref) <= 1e-10 * abs(lnl_ref), frac
            assert _close(e.root_invariant_term(), term_ref, 1e-10), frac
            assert e.profile()["device_bytes"] <= cap, frac
    assert accepted >= 2 and tiled >= 2, (accepted, tiled)


# ---------------------------------------------------------------------------------------------------------
# (d) shards (the same device repeated), with and without a per-shard cap
# ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _shard_problem():
    pb = _with_constant_patterns(random_problem(300, 4001, 4, seed=8080, gaps=0.03, bl=(0.3, 0.9), rescale=1, pinv=0.2))
    assert_real_exponents(pb)
    return pb, pb.gradient(), po.root_invariant_term(pb), _untiled_bytes(pb, RESCALE_ALWAYS)


@pytest.mark.parametrize("capped", [False, True])
@pytest.mark.parametrize("n", [2, 3])
def test_sharded_rescaled_engine_with_invariant_class(n, capped):
    """max_device_bytes holds for every shard: capped, each shard runs its own pattern range in tiles"""
    pb, ref, term_ref, untiled_bytes = _shard_problem()
    kw = dict(max_device_bytes=_tiling_cap(pb, RESCALE_ALWAYS, untiled_bytes / n, devices=[0] * n)) if capped else {}
    tol = 1e-9 * max(1.0, np.abs(ref["cat_grad"]).max())
    with engine_from_problem(pb, rescale=RESCALE_ALWAYS, devices=[0] * n, **kw) as e:
        assert e.shard_count == n and (e.profile()["tiles"] >= 2) == capped
        lnl, cg = e.gradient()
        assert abs(lnl - ref["lnl"]) <= 1e-10 * abs(ref["lnl"]) and np.abs(cg - ref["cat_grad"]).max() <= tol
        assert _close(e.root_invariant_term(), term_ref, 1e-10)
        assert abs(e.log_likelihood() - ref["lnl"]) <= 1e-10 * abs(ref["lnl"])
        assert _close(e.root_invariant_term(), term_ref, 1e-10)
        if capped:
            assert e.profile()["device_bytes"] <= n * kw["max_device_bytes"]  # (the profile adds the shards' bytes up)
    with engine_from_problem(pb, rescale=RESCALE_ALWAYS, devices=[0] * n, **kw) as e:  # fresh: the term after the post-order pass alone
        assert abs(e.log_likelihood() - ref["lnl"]) <= 1e-10 * abs(ref["lnl"])
        assert _close(e.root_invariant_term(), term_ref, 1e-10)
