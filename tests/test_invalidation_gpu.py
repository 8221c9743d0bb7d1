"""GPU: what every input of an engine invalidates -- resident uppers of a keep-partials gradient, the root terms of an untiled
and of a tiled engine -- against the CPU oracle at the NEW inputs.

The shapes are the smallest that still have every node kind: 4 states, 9 taxa x 65 patterns x 2 categories (fringe, DEEP and
stored nodes, a ragged second wave), unscaled and rescaled, and 20 states, 6 taxa x 17 patterns x 2 categories.
"""
import functools

import numpy as np
import pytest

from golden_util import reversible_eigen
from gpu_util import engine_from_problem, random_problem
from oracle import phyoracle as po
from physher_amd.engine import RESCALE_ALWAYS, RESCALE_NEVER, EngineError

pytestmark = pytest.mark.gpu

# name: (S, T, P, C, engine rescaling)
SHAPES = {
    "4s": (4, 9, 65, 2, RESCALE_NEVER),
    "4s_rescaled": (4, 9, 65, 2, RESCALE_ALWAYS),
    "20s": (20, 6, 17, 2, RESCALE_NEVER),
}
TILED_P = 600  # tiles are sized in multiples of 256 patterns: 65 patterns cannot tile


@functools.lru_cache(maxsize=None)
def _problem(name, pinv=None, P=None):
    S, T, P0, C, rescale = SHAPES[name]
    forced = rescale == RESCALE_ALWAYS
    return random_problem(T, P or P0, C, seed=500 + S + T, S=S, gaps=0.03, bl=(0.3, 0.9) if forced else (0.01, 0.1), rescale=1 if forced else 0,
                          pinv=pinv)


def _replace(pb, **kw):
    """pb with some fields replaced"""
    f = dict(weights=pb.weights, eval_=pb.eval, evec=pb.evec, ivec=pb.ivec, freqs=pb.freqs, cat_rates=pb.cat_rates, cat_props=pb.cat_props,
             branch_lengths=pb.branch_lengths.copy(), tip_states=pb.tip_states)
    f.update(kw)
    return po.Problem(pb.left, pb.right, pb.root, f["weights"], f["eval_"], f["evec"], f["ivec"], f["freqs"], f["cat_rates"], f["cat_props"],
                      f["branch_lengths"], tip_states=f["tip_states"], rescale=pb.rescale)


def _new_frequencies(pb):
    return np.random.default_rng(11).dirichlet(np.full(pb.S, 5.0))


# setter name -> (the problem with changed values, the call that brings an engine there[, the problem the engine starts from])
def _set_branch_lengths(pb):
    bl = pb.branch_lengths * np.random.default_rng(1).uniform(0.5, 1.5, size=pb.N)
    return _replace(pb, branch_lengths=bl), lambda e: e.set_branch_lengths(bl)


def _set_eigen(pb):
    r = np.random.default_rng(2).uniform(0.5, 3.0, size=(pb.S, pb.S))
    ev, U, Ui = reversible_eigen(0.5 * (r + r.T), pb.freqs)
    return _replace(pb, eval_=ev, evec=U, ivec=Ui), lambda e: e.set_eigen(ev, U, Ui)


def _set_frequencies(pb):
    """The single-branch evaluation weighs the branch's upper end with pi, as the reference's does (k_branch_eval4): it is the
    likelihood only where the model is reversible with respect to pi.  So the engine starts from an eigen system that is reversible
    with respect to the NEW frequencies and holds the old ones; the setter alone makes the two agree."""
    f = _new_frequencies(pb)
    r = np.random.default_rng(4).uniform(0.5, 3.0, size=(pb.S, pb.S))
    ev, U, Ui = reversible_eigen(0.5 * (r + r.T), f)
    start = _replace(pb, eval_=ev, evec=U, ivec=Ui)
    return _replace(start, freqs=f), lambda e: e.set_frequencies(f), start


def _set_category_rates(pb):
    rates, props = np.array([0.3, 1.4]), np.array([0.4, 0.6])
    rates = rates / (rates * props).sum()
    return _replace(pb, cat_rates=rates, cat_props=props), lambda e: e.set_category_rates(rates, props)


def _set_tip_states(pb):
    states = pb.tip_states.copy()
    states[0] = (states[0] + 1 + np.arange(pb.P) % (pb.S - 1)) % pb.S  # tip 0: another state at every pattern
    return _replace(pb, tip_states=states), lambda e: e.set_tip_states(0, states[0])


def _set_pattern_weights(pb):
    w = np.random.default_rng(3).integers(1, 9, size=pb.P).astype(np.float64)
    return _replace(pb, weights=w), lambda e: e.set_pattern_weights(w)


def _update_all_nodes(pb):
    return _replace(pb), lambda e: e.update_all_nodes()


SETTERS = {"set_branch_lengths": _set_branch_lengths, "set_eigen": _set_eigen, "set_frequencies": _set_frequencies,
           "set_category_rates": _set_category_rates, "set_tip_states": _set_tip_states, "set_pattern_weights": _set_pattern_weights,
           "update_all_nodes": _update_all_nodes}


def _branch_nodes(pb):
    """one tip and one internal node that is not the root"""
    return [1, next(n for n in range(pb.T, pb.N) if n != pb.root)]


@functools.lru_cache(maxsize=None)
def _changed(name, setter):
    """the problem an engine starts from, the call that applies the change, and the oracle at the changed problem: lnL and d1 of
    each trial branch, the uppers"""
    new, apply, start = (SETTERS[setter](_problem(name)) + (_problem(name),))[:3]
    trials = {}
    for n in _branch_nodes(new):
        t = 1.3 * new.branch_lengths[n] + 0.01
        o = _replace(new, branch_lengths=np.where(np.arange(new.N) == n, t, new.branch_lengths)).gradient()
        trials[n] = (t, o["lnl"], po.branch_gradient_from_cat(o["cat_grad"], new.cat_rates, new.cat_props)[n], np.abs(o["cat_grad"]).max())
    return start, apply, trials, new.gradient(want_partials=True)


def check_branch_values(e, trials):
    """branch_log_likelihood at a trial length against the oracle at the engine's new inputs (the tolerances of
    test_single_branch_evaluation); returns the failures instead of asserting, so that a script can list them"""
    bad = []
    for n, (t, lnl_ref, d1_ref, gmax) in trials.items():
        lnl, d1, _ = e.branch_log_likelihood(n, t)
        print(f"node {n}: lnL {lnl!r} (oracle {lnl_ref!r}), d1 {d1!r} (oracle {d1_ref!r})")
        if not abs(lnl - lnl_ref) <= 1e-10 * abs(lnl):
            bad.append((n, "lnL", lnl, lnl_ref))
        if not abs(d1 - d1_ref) <= 1e-9 * max(1.0, gmax):
            bad.append((n, "d1", d1, d1_ref))
    return bad


@pytest.mark.parametrize("setter", list(SETTERS))
@pytest.mark.parametrize("name", list(SHAPES))
def test_every_setter_drops_the_resident_uppers(name, setter):
    """After a keep-partials gradient the single-branch evaluation reads the resident uppers.  Any input that changes the partials
    drops them: reading them is refused, the single-branch evaluation rebuilds the one upper it needs from the new inputs, and the
    next gradient makes them resident again."""
    start, apply, trials, ref = _changed(name, setter)
    rescale = SHAPES[name][4]
    with engine_from_problem(start, rescale=rescale) as e:
        e.set_keep_partials(True)
        e.gradient()
        for n in trials:
            e.partials(n, upper=True)  # resident now
        apply(e)
        for n in trials:
            with pytest.raises(EngineError, match="upper partials need"):
                e.partials(n, upper=True)
        assert check_branch_values(e, trials) == []
        lnl, cg = e.gradient()
        assert abs(lnl - ref["lnl"]) <= 1e-10 * abs(ref["lnl"])
        assert np.abs(cg - ref["cat_grad"]).max() <= 1e-9 * max(1.0, np.abs(ref["cat_grad"]).max())
        for n in trials:
            up = e.partials(n, upper=True)
            if not ref["rescaled"]:
                np.testing.assert_allclose(up, ref["upper"][n], rtol=1e-9, atol=1e-300)
        assert check_branch_values(e, trials) == []  # (the resident route again)


# ---------------------------------------------------------------------------------------------------------
# the two root terms: current after an evaluation, refused after a setter until the next one
# ---------------------------------------------------------------------------------------------------------
def _close(a, b, rel=1e-10):
    return np.all(np.abs(np.asarray(a) - np.asarray(b)) <= rel * np.maximum(1.0, np.abs(b)))


def _dq(S):
    dQ = np.random.default_rng(5).normal(size=(2, S, S))
    return dQ - dQ.sum(axis=2, keepdims=True) * np.eye(S)[None]


def _check_root_terms(e, pb, evaluate):
    """the three steps: both terms after an evaluation, refused after set_frequencies, at the new frequencies after the next one"""
    evaluate(e)
    inv, freq = e.root_invariant_term(), e.root_frequency_term()
    print("invariant term", inv, po.root_invariant_term(pb), "frequency term", freq, po.root_frequency_term(pb))
    assert _close(inv, po.root_invariant_term(pb)) and _close(freq, po.root_frequency_term(pb))
    new = _replace(pb, freqs=_new_frequencies(pb))
    e.set_frequencies(new.freqs)
    with pytest.raises(EngineError, match="no evaluation has been run yet"):
        e.root_invariant_term()
    with pytest.raises(EngineError, match="no evaluation has been run yet|comes with phyamd_parameter_gradient: call that first"):
        e.root_frequency_term()
    evaluate(e)
    inv, freq = e.root_invariant_term(), e.root_frequency_term()
    print("invariant term", inv, po.root_invariant_term(new), "frequency term", freq, po.root_frequency_term(new))
    assert _close(inv, po.root_invariant_term(new)) and _close(freq, po.root_frequency_term(new))


@pytest.mark.parametrize("name", list(SHAPES))
def test_root_terms_follow_the_frequencies(name):
    pb = _problem(name, pinv=0.25)
    with engine_from_problem(pb, rescale=SHAPES[name][4]) as e:
        assert e.profile()["tiles"] == 1
        _check_root_terms(e, pb, lambda e: e.log_likelihood())


def _tiling_cap(pb, rescale, untiled_bytes):
    """A cap below the untiled working set, as a fraction of the untiled engine's device_bytes after a gradient.  What stays
    resident whatever the tile size is most of so small an engine, so one fixed fraction either tiles or is refused when the engine
    is made: the largest fraction, in steps of 5 %, at which the engine is built in two tiles or more."""
    for frac in np.arange(1.5, 0.1, -0.05):
        try:
            with engine_from_problem(pb, rescale=rescale, max_device_bytes=int(frac * untiled_bytes)) as e:
                if e.profile()["tiles"] >= 2:
                    return int(frac * untiled_bytes)
        except EngineError as err:
            assert err.code == -3, str(err)  # PHYAMD_ENOMEM: refused when the engine is made
    pytest.fail("no cap puts this problem into tiles")


@pytest.mark.parametrize("name", [n for n in SHAPES if SHAPES[n][0] == 4])
def test_root_terms_of_a_tiled_engine_follow_the_frequencies(name):
    """Tiled, the terms are sums the last evaluation formed tile by tile (the frequency term: the last parameter gradient)."""
    pb = _problem(name, pinv=0.25, P=TILED_P)
    rescale = SHAPES[name][4]
    with engine_from_problem(pb, rescale=rescale) as whole:
        whole.gradient()
        untiled_bytes = whole.profile()["device_bytes"]
    with engine_from_problem(pb, rescale=rescale, max_device_bytes=_tiling_cap(pb, rescale, untiled_bytes)) as e:
        assert e.profile()["tiles"] >= 2
        e.set_rate_matrix_derivatives(_dq(pb.S))
        _check_root_terms(e, pb, lambda e: e.parameter_gradient())
