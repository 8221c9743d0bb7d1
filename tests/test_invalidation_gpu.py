"""GPU: what every input of an engine invalidates -- resident uppers of a keep-partials gradient, the root terms of an untiled
and of a tiled engine -- against the CPU oracle at the NEW inputs.

The shapes are the smallest that still have every node kind: 4 states, 9 taxa x 65 patterns x 2 categories (fringe, DEEP and
stored nodes, a ragged second wave), unscaled and rescaled, and 20 states, 6 taxa x 17 patterns x 2 categories.

Every row of the engine's invalidation table (enum class Input, phyamd_shard.inc) is driven in the same way -- one known state, one
call, then every product against the oracle at the new inputs (check_everything) -- from two start states:
    "resident"  set_keep_partials(True), then gradient(): the level kernels, stored lowers in the Reference form, resident uppers;
    "default"   a plain gradient() on an engine that was never asked to keep partials: the tree walks (4 states: k_lower4_stream /
                k_upper4_stream, stored lowers in a Carried form; 20 states: k_lower_gen_walk, whose pre-order pass has no walk and
                stays with the level kernels).
The tiny shapes do reach the walks (there is no size threshold on them), so they are not enlarged.  The "default" cases assert it
from the profile: a walk reports 1 or 2 launches, the level kernels one per tree level, and the 9-taxon tree has seven levels of
internal nodes (the 6-taxon tree five; there general_profile()["lower_family"] names the walk as well).  The helpers that build
other trees and explicit matrices are pinned on the oracle alone in tests/test_invalidation_util.py.
"""
import functools

import numpy as np
import pytest

import invalidation_util as iu
from golden_util import reversible_eigen
from gpu_util import engine_from_problem, random_problem
from oracle import phyoracle as po
from physher_amd.engine import GRAD_FOLD_ROOT_FREQS, RESCALE_ALWAYS, RESCALE_AUTO, RESCALE_NEVER, Engine, EngineError
from state_posteriors_util import GAP, oracle_site_rates, oracle_state_posteriors

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


_replace = iu.replace  # pb with some fields replaced


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


# ---------------------------------------------------------------------------------------------------------
# the rest of the table, and every row from both start states
# ---------------------------------------------------------------------------------------------------------
STARTS = ("resident", "default")
EINVAL, EUNSUPPORTED = -1, -4


def _internal(pb, under_root=None):
    """internal nodes other than the root (under_root: only those whose parent is / is not the root)"""
    par = iu.parents(pb)
    return [n for n in range(pb.T, pb.N) if n != pb.root and (under_root is None or (par[n] == pb.root) == under_root)]


def _perm(pb, seed=7):
    """a permutation of the internal ids that moves the root off the last id"""
    rng = np.random.default_rng(seed)
    while True:
        perm = np.concatenate([np.arange(pb.T), pb.T + rng.permutation(pb.T - 1)])
        if perm[pb.root] != pb.N - 1:
            return perm


def _one_branch(node_of):
    def row(pb):
        nodes = node_of(pb)
        bl = pb.branch_lengths.copy()
        bl[nodes] = 1.6 * bl[nodes] + 0.02

        def apply(e):
            for n in nodes:
                e.set_branch_length(n, bl[n])
        return _replace(pb, branch_lengths=bl), apply
    return row


def _explicit_nodes(pb):
    """a tip and an internal node other than the root, neither of them a node of _branch_nodes"""
    return [0, _internal(pb)[-1]]


def _set_node_matrices(pb):
    nodes = _explicit_nodes(pb)
    bl = pb.branch_lengths.copy()
    bl[nodes] = 1.8 * bl[nodes] + 0.03
    mats = iu.matrices_at(pb, bl)

    def apply(e):
        for n in nodes:
            e.set_node_matrices(n, mats[n])
    return _replace(pb, branch_lengths=bl), apply, pb, set(nodes)


def _set_matrices(pb):
    bl = 0.7 * pb.branch_lengths
    mats = iu.matrices_at(pb, bl)
    return _replace(pb, branch_lengths=bl), lambda e: e.set_matrices(mats), pb, set(range(pb.N))


def _set_matrices_then_set_eigen(pb):
    mats = iu.matrices_at(pb, 0.7 * pb.branch_lengths)

    def apply(e):
        e.set_matrices(mats)
        e.set_eigen(pb.eval, pb.evec, pb.ivec)  # clears the explicit matrices
    return _replace(pb), apply


def _set_tip_partials(pb):
    """tip 0: another state at every pattern as a 0/1 vector, a set of two states at pattern 0 and an all-ones row at pattern 1"""
    tp = iu.tip_vectors(pb).copy()
    states = (pb.tip_states[0] % pb.S + 1 + np.arange(pb.P) % (pb.S - 1)) % pb.S
    tp[0] = 0.0
    tp[0, np.arange(pb.P), states] = 1.0
    tp[0, 0, (states[0] + 1) % pb.S] = 1.0
    tp[0, 1, :] = 1.0
    assert tp[0, 0].sum() == 2 and tp[0, 1].sum() == pb.S
    return _replace(pb, tip_states=None, tip_partials=tp), lambda e: e.set_tip_partials(0, tp[0])


def _to_tree(new):
    def apply(e):
        e.set_topology(new.left, new.right, new.root)
        e.set_branch_lengths(new.branch_lengths)
    return apply


def _set_topology_nni(pb):
    new = iu.neighbour(pb, _internal(pb, under_root=False)[0], 1)
    return new, _to_tree(new)


def _set_topology_shape(first, then):
    def row(pb):
        start, new = iu.other_tree(pb, first, 3), iu.other_tree(pb, then, 4)
        assert iu.levels(start) != iu.levels(new)
        return new, _to_tree(new), start
    return row


def _set_topology_relabelled(pb):
    new = iu.relabel(pb, _perm(pb))
    return new, _to_tree(new)


def _set_topology_refused(pb):
    """the child of an internal node becomes the root's left child as well: two parents for one node, none for another"""
    left = pb.left.copy()
    left[pb.root] = pb.left[_internal(pb)[0]]

    def apply(e):
        with pytest.raises(EngineError, match="two parents") as err:
            e.set_topology(left, pb.right, pb.root)
        assert err.value.code == EINVAL
    return _replace(pb), apply


def _set_keep_partials(pb):
    return _replace(pb), "toggle keep_partials"


def _set_rescaling(pb):
    """NEVER -> ALWAYS; an engine made with ALWAYS goes to NEVER, on branches short enough for the unscaled answer to be finite"""
    if pb.rescale:
        start = _replace(pb, branch_lengths=0.1 * pb.branch_lengths)
        return _replace(start, rescale=0), lambda e: e.set_rescaling(RESCALE_NEVER), start
    return _replace(pb, rescale=1), lambda e: e.set_rescaling(RESCALE_ALWAYS)


NEW_ROWS = {
    "set_branch_length_tip": _one_branch(lambda pb: [2]),
    "set_branch_length_under_root": _one_branch(lambda pb: _internal(pb, under_root=True)[:1]),
    "set_branch_length_two": _one_branch(lambda pb: [3, _internal(pb, under_root=False)[0]]),
    "set_node_matrices": _set_node_matrices,
    "set_matrices": _set_matrices,
    "set_matrices_then_set_eigen": _set_matrices_then_set_eigen,
    "set_tip_partials": _set_tip_partials,
    "set_topology_nni": _set_topology_nni,
    "set_topology_shape_to_caterpillar": _set_topology_shape("balanced", "caterpillar"),
    "set_topology_shape_to_balanced": _set_topology_shape("caterpillar", "balanced"),
    "set_topology_relabelled": _set_topology_relabelled,
    "set_topology_refused": _set_topology_refused,
    "set_keep_partials": _set_keep_partials,
    "set_rescaling": _set_rescaling,
}
ROWS = {**SETTERS, **NEW_ROWS}


def _normalised(row, pb):
    """(the new problem, the call, the problem the engine starts from, the nodes that hold explicit matrices afterwards)"""
    r = tuple(ROWS[row](pb))
    if len(r) == 2:
        r += (pb,)
    return r if len(r) == 4 else r + (set(),)


@functools.lru_cache(maxsize=None)
def _case(name, row):
    """everything the oracle says about a row, once per module: the trial branches (nodes without explicit matrices), the gradient
    with all partials, the posteriors, and the same row on the shape's +I variant with its root term"""
    new, apply, start, explicit = _normalised(row, _problem(name))
    trials = {}
    for n in _branch_nodes(new):
        if n in explicit:
            continue
        t = 1.3 * new.branch_lengths[n] + 0.01
        o = _replace(new, branch_lengths=np.where(np.arange(new.N) == n, t, new.branch_lengths)).gradient()
        trials[n] = (t, o["lnl"], po.branch_gradient_from_cat(o["cat_grad"], new.cat_rates, new.cat_props)[n], np.abs(o["cat_grad"]).max())
    J, _ = oracle_state_posteriors(new)
    post = J / J.sum(axis=2, keepdims=True)
    top = np.sort(post, axis=2)
    inv_new, inv_apply, inv_start, _ = _normalised(row, _problem(name, pinv=0.25))
    return dict(start=start, apply=apply, new=new, trials=trials, ref=new.gradient(want_partials=True), post=post, states=post.argmax(axis=2),
                gap=top[:, :, -1] - top[:, :, -2], rates=oracle_site_rates(new), inv=(inv_start, inv_apply, po.root_invariant_term(inv_new)))


def _begin(e, start, pb):
    """bring a new engine into one of the two start states; returns whether uppers are resident"""
    e.set_profiling(True)
    if start == "resident":
        e.set_keep_partials(True)
        e.gradient()
        p = e.profile()
        print("resident:", p["lower_launches"], "post-order and", p["upper_launches"], "pre-order launches (the level kernels: one per level)")
        return True
    e.gradient()
    p = e.profile()
    print("default:", p["lower_launches"], "post-order and", p["upper_launches"], "pre-order launches")
    assert p["lower_launches"] in (1, 2), "the post-order pass did not run a tree walk"
    if pb.S == 4:
        assert iu.levels(pb) >= 4  # (so that the level kernels would have reported more)
        assert p["upper_launches"] in (1, 2), "the pre-order pass did not run a tree walk"
    else:
        assert e.general_profile()["lower_family"] == 1  # (k_lower_gen_walk; the 20-state pre-order pass is always the level kernels')
    return False


def _apply(e, apply, start):
    if apply == "toggle keep_partials":
        e.set_keep_partials(start != "resident")
    else:
        apply(e)


def _check_gradient(e, ref, what, flags=0, scale=1.0):
    lnl, cg = e.gradient(flags)
    plk = e.pattern_log_likelihoods()
    gmax = max(1.0, scale * np.abs(ref["cat_grad"]).max())
    print(f"{what}: lnL {lnl!r} (oracle {ref['lnl']!r}); gradient off by {np.abs(cg - scale * ref['cat_grad']).max():.3e} of {gmax:.3e}; "
          f"per-pattern lnL off by {np.abs(plk - ref['pattern_lk']).max():.3e}")
    assert abs(lnl - ref["lnl"]) <= 1e-10 * abs(ref["lnl"])
    np.testing.assert_allclose(plk, ref["pattern_lk"], rtol=1e-11, atol=1e-11)
    assert np.abs(cg - scale * ref["cat_grad"]).max() <= 1e-9 * gmax
    lnl2, cg2 = e.gradient(flags)  # nothing changed: the same bits
    assert lnl2 == lnl and np.array_equal(cg2, cg)
    return lnl, cg


def check_everything(e, case, refused_uppers):
    """every product of an engine against the oracle at case["new"], the tolerances of DESIGN.md section 4"""
    new, trials, ref = case["new"], case["trials"], case["ref"]
    tip, inner = _branch_nodes(new)
    if refused_uppers:
        for n in (tip, inner):
            with pytest.raises(EngineError, match="upper partials need"):
                e.partials(n, upper=True)
        assert check_branch_values(e, trials) == []  # (rebuilds the one upper it needs from the new inputs)
        _check_gradient(e, ref, "as the call left the engine")
    else:  # the gradient first: it meets the walks' stored lowers as the call left them; the single-branch evaluation then settles the form itself
        _check_gradient(e, ref, "as the call left the engine")
        assert check_branch_values(e, trials) == []
    e.set_keep_partials(True)
    _check_gradient(e, ref, "keeping partials")
    if not ref["rescaled"]:
        for n in (new.root, inner):
            np.testing.assert_allclose(e.partials(n), ref["lower"][n], rtol=1e-9, atol=1e-300)
        for n in (tip, inner):
            np.testing.assert_allclose(e.partials(n, upper=True), ref["upper"][n], rtol=1e-9, atol=1e-300)
    assert check_branch_values(e, trials) == []  # (the resident route)
    post, states = e.state_posteriors()
    sure = case["gap"] >= GAP
    print(f"posteriors off by {np.abs(post - case['post']).max():.3e}; cells below the gap {np.count_nonzero(~sure)}")
    assert np.abs(post - case["post"]).max() <= 1e-9
    assert np.array_equal(states[sure], case["states"][sure])
    R, mean = e.site_rate_posteriors()
    assert np.abs(R - case["rates"][0]).max() <= 1e-9 and np.abs(mean - case["rates"][1]).max() <= 1e-9 * max(1.0, np.abs(case["rates"][1]).max())


@pytest.mark.parametrize("row", list(ROWS))
@pytest.mark.parametrize("name", list(SHAPES))
@pytest.mark.parametrize("start", STARTS)
def test_every_row_from_both_states(start, name, row):
    case = _case(name, row)
    rescale = SHAPES[name][4]
    with engine_from_problem(case["start"], rescale=rescale) as e:
        resident = _begin(e, start, case["start"])
        _apply(e, case["apply"], start)
        check_everything(e, case, refused_uppers=resident)
    inv_start, inv_apply, inv_ref = case["inv"]
    with engine_from_problem(inv_start, rescale=rescale) as e:  # the shape's +I variant: the root term after the same call
        _begin(e, start, inv_start)
        _apply(e, inv_apply, start)
        e.log_likelihood()
        inv = e.root_invariant_term()
        print("invariant term", inv, inv_ref)
        assert _close(inv, inv_ref)


# ---------------------------------------------------------------------------------------------------------
# Input::RateMatrix: everything made from Q is formed again, nothing else
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, GRAD_FOLD_ROOT_FREQS])
@pytest.mark.parametrize("name", ["4s", "20s"])
@pytest.mark.parametrize("start", STARTS)
def test_set_rate_matrix_rescales_the_gradient_and_nothing_else(start, name, flags):
    """An engine on explicit matrices P = exp(Q t r) with the model's own Q: s Q instead leaves lnL as it is, bit for bit, and
    multiplies every branch term by s -- in the image of Q, in the image of diag(pi) Q and, at 20 states, in the tip rate products."""
    pb, s = _problem(name), 1.75
    q = _replace(pb)
    q.fold_root_freqs = 1 if flags else 0
    ref = q.gradient()
    with engine_from_problem(pb, rescale=SHAPES[name][4]) as e:
        e.set_matrices(iu.matrices_at(pb, pb.branch_lengths))
        e.set_rate_matrix(iu.rate_matrix(pb))
        e.set_profiling(True)
        if start == "resident":
            e.set_keep_partials(True)
        e.gradient(flags)
        if start == "default":
            assert e.profile()["lower_launches"] in (1, 2), "the post-order pass did not run a tree walk"
        before, _ = _check_gradient(e, ref, "Q", flags)
        e.set_rate_matrix(s * iu.rate_matrix(pb))
        after, _ = _check_gradient(e, ref, "1.75 Q", flags, scale=s)
        assert after == before
        e.set_rate_matrix(iu.rate_matrix(pb))
        _check_gradient(e, ref, "Q again", flags)


# ---------------------------------------------------------------------------------------------------------
# Input::RateMatrixDerivatives
# ---------------------------------------------------------------------------------------------------------
def _dqs(S, count, seed):
    dQ = np.random.default_rng(seed).normal(size=(count, S, S))
    return dQ - dQ.sum(axis=2, keepdims=True) * np.eye(S)[None]


@pytest.mark.parametrize("name", list(SHAPES))
@pytest.mark.parametrize("start", STARTS)
def test_a_second_set_of_rate_matrix_derivatives(start, name):
    """two dQ, three others, one; then set_eigen in between (the tolerance of test_parameter_gradient_random_problems)"""
    pb = _problem(name)
    changed, set_eigen = _set_eigen(pb)

    def check(e, q, dQ, what):
        _, og = po.parameter_gradient(q, dQ)
        ref = q.gradient()
        e.set_rate_matrix_derivatives(dQ)
        lnl, cg, pg = e.parameter_gradient()
        print(f"{what}: parameter gradient off by {np.abs(pg - og).max():.3e} of {np.abs(og).max():.3e}")
        assert pg.shape == (len(dQ),)
        assert abs(lnl - ref["lnl"]) <= 1e-10 * abs(ref["lnl"])
        assert np.abs(pg - og).max() <= 1e-9 * max(1.0, np.abs(og).max())
        assert np.abs(cg - ref["cat_grad"]).max() <= 1e-9 * max(1.0, np.abs(ref["cat_grad"]).max())

    with engine_from_problem(pb, rescale=SHAPES[name][4]) as e:
        if start == "resident":
            e.set_keep_partials(True)
        e.gradient()
        check(e, pb, _dqs(pb.S, 2, 21), "two")
        check(e, pb, _dqs(pb.S, 3, 22), "three others")
        check(e, pb, _dqs(pb.S, 1, 23), "one")
        set_eigen(e)
        check(e, changed, _dqs(pb.S, 1, 23), "the same one after set_eigen")
        check(e, changed, _dqs(pb.S, 3, 24), "three after set_eigen")


# ---------------------------------------------------------------------------------------------------------
# matrices that are no exponential of the engine's Q
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["4s", "20s"])
def test_arbitrary_matrices_against_the_pruning_pass(name):
    pb = _problem(name)
    mats = iu.reversible_matrices(pb, 31)
    ref = iu.prune(pb, mats, iu.rate_matrix(pb))
    assert abs(ref["lnl"] - pb.log_likelihood()["lnl"]) > 1e-3  # (not the eigen system's matrices)
    with engine_from_problem(pb, rescale=SHAPES[name][4]) as e:
        e.set_matrices(mats)
        _check_gradient(e, ref, "each node's own model")
        e.set_keep_partials(True)
        _check_gradient(e, ref, "keeping partials")


# ---------------------------------------------------------------------------------------------------------
# phyamd_get_node_matrices
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["4s", "20s"])
def test_node_matrices_and_their_derivatives(name):
    """An eigen node: P and dP/d(t r) of the eigen system, the derivative WITHOUT the factor r_c (k_transition_matrices).  An explicit
    node: what was set, and Q P -- not what the eigen system left in the buffer before set_node_matrices."""
    pb = _problem(name)
    Q = iu.rate_matrix(pb)
    eigen_node, explicit_node = _branch_nodes(pb)[1], _explicit_nodes(pb)[1]
    other = iu.matrices_at(pb, 2.5 * pb.branch_lengths + 0.05)[explicit_node]
    with engine_from_problem(pb, rescale=SHAPES[name][4]) as e:
        e.gradient()  # (the eigen system's P and dP of every node are in the buffers now)

        def check_eigen(n):
            for c in range(pb.C):
                t = pb.branch_lengths[n] * pb.cat_rates[c]
                np.testing.assert_allclose(e.node_matrices(n)[c], po.p_t(pb.S, pb.eval, pb.evec, pb.ivec, t), rtol=1e-12, atol=1e-15)
                np.testing.assert_allclose(e.node_matrices(n, derivative=True)[c], po.p_t(pb.S, pb.eval, pb.evec, pb.ivec, t, derivative=True),
                                           rtol=1e-12, atol=1e-14)
        check_eigen(eigen_node)
        check_eigen(explicit_node)
        e.set_node_matrices(explicit_node, other)
        assert np.array_equal(e.node_matrices(explicit_node), other)
        d = e.node_matrices(explicit_node, derivative=True)
        print("derivative of an explicit node off Q P by", np.abs(d - Q @ other).max())
        np.testing.assert_allclose(d, Q @ other, rtol=1e-12, atol=1e-14)
        e.gradient()
        np.testing.assert_allclose(e.node_matrices(explicit_node, derivative=True), Q @ other, rtol=1e-12, atol=1e-14)
        e.set_rate_matrix(1.75 * Q)
        np.testing.assert_allclose(e.node_matrices(explicit_node, derivative=True), 1.75 * Q @ other, rtol=1e-12, atol=1e-14)
        check_eigen(eigen_node)
        e.set_eigen(pb.eval, pb.evec, pb.ivec)  # the node is an eigen node again
        check_eigen(explicit_node)
    with Engine(pb.T, pb.P, pb.S, pb.C, rescale=SHAPES[name][4]) as e:  # explicit matrices and no Q at all: refused by name
        e.set_topology(pb.left, pb.right, pb.root)
        e.set_branch_lengths(pb.branch_lengths)
        e.set_frequencies(pb.freqs)
        e.set_category_rates(pb.cat_rates, pb.cat_props)
        e.set_pattern_weights(pb.weights)
        for t in range(pb.T):
            e.set_tip_states(t, pb.tip_states[t])
        mats = iu.matrices_at(pb, pb.branch_lengths)
        e.set_matrices(mats)
        ref = pb.log_likelihood()["lnl"]
        assert abs(e.log_likelihood() - ref) <= 1e-10 * abs(ref)
        assert np.array_equal(e.node_matrices(explicit_node), mats[explicit_node])
        with pytest.raises(EngineError, match="their derivative is Q P") as err:
            e.node_matrices(explicit_node, derivative=True)
        assert err.value.code == EINVAL


# ---------------------------------------------------------------------------------------------------------
# a new root id without new lengths
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
@pytest.mark.parametrize("start", STARTS)
def test_lengths_sent_before_a_change_of_root_stay(start, name):
    """Lengths go by node id (phyamd_set_topology's header): sent in the NEW ids' order while the engine is still on the old tree,
    they hold after set_topology moves the root to another id -- the old root's id has the length sent for it, not 0."""
    pb = _problem(name)
    new = iu.relabel(pb, _perm(pb))
    assert new.root != pb.root and new.branch_lengths[pb.root] > 0.0
    ref = new.gradient()
    with engine_from_problem(pb, rescale=SHAPES[name][4]) as e:
        _begin(e, start, pb)
        e.set_branch_lengths(new.branch_lengths)
        e.set_topology(new.left, new.right, new.root)
        _check_gradient(e, ref, "the relabelled tree")
        n = pb.root  # one branch afterwards: the old root's id, now an ordinary node
        bl = new.branch_lengths.copy()
        bl[n] *= 1.5
        e.set_branch_length(n, bl[n])
        _check_gradient(e, _replace(new, branch_lengths=bl).gradient(), "one branch afterwards")


# ---------------------------------------------------------------------------------------------------------
# store and restore across the new rows
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", ["set_branch_length_tip", "set_keep_partials", "set_rescaling"])
@pytest.mark.parametrize("name", ["4s", "20s"])
def test_store_and_restore_across_a_row(name, row):
    case = _case(name, row)
    pb = case["start"]
    stored = pb.gradient()
    with engine_from_problem(pb, rescale=SHAPES[name][4]) as e:
        _begin(e, "default", pb)
        e.store()
        lnl_stored = e.log_likelihood()
        assert abs(lnl_stored - stored["lnl"]) <= 1e-10 * abs(stored["lnl"])
        _apply(e, case["apply"], "default")
        _check_gradient(e, case["ref"], "after the call")
        e.restore()
        back = e.log_likelihood()
        print(f"stored {lnl_stored!r} restored {back!r} oracle {stored['lnl']!r}")
        assert abs(back - stored["lnl"]) <= 1e-10 * abs(stored["lnl"])
        if row == "set_branch_length_tip":  # the slots were not reassigned: the stored partials themselves, the root integrated again
            assert back == lnl_stored
        _check_gradient(e, stored, "restored")


@pytest.mark.parametrize("name", ["4s", "20s"])
def test_store_and_restore_refusals(name):
    pb = _problem(name)
    new, to_tree = _set_topology_nni(pb)
    with engine_from_problem(pb, rescale=SHAPES[name][4]) as e:
        _begin(e, "default", pb)
        e.store()
        to_tree(e)
        with pytest.raises(EngineError, match="nothing is stored") as err:
            e.restore()
        assert err.value.code == EINVAL
        _check_gradient(e, new.gradient(), "the neighbour, after the refused restore")
        e.set_node_matrices(0, iu.matrices_at(new, new.branch_lengths)[0])
        with pytest.raises(EngineError, match="phyamd_store does not cover explicit node matrices") as err:
            e.store()
        assert err.value.code == EUNSUPPORTED
        _check_gradient(e, new.gradient(), "after the refused store")


# ---------------------------------------------------------------------------------------------------------
# the lazy switch in mid-life
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,T,P,C,seed", [(4, 900, 64, 4, 13), (20, 400, 20, 2, 21)])
def test_lazy_rescaling_switch_in_mid_life(S, T, P, C, seed):
    """the sizes of test_lazy_rescaling_switch and test_generic_states_lazy_rescaling_switch (nine taxa cannot underflow), on an
    engine that has evaluated unscaled before its lengths grow.  The data are evolved on the short branches, so that those do not
    underflow; such nearly constant columns cost about log(1 / S) per tip on saturated branches only, hence lengths of 2 to 6
    where those tests, whose data are evolved on the long branches, have 0.5 to 1.5"""
    short = random_problem(T, P, C, seed=seed, S=S, bl=(0.001, 0.01), rescale=2)
    long_bl = np.random.default_rng(seed).uniform(2.0, 6.0, size=short.N)
    ref_short, ref_long = short.gradient(), _replace(short, branch_lengths=long_bl).gradient()
    assert not ref_short["rescaled"] and ref_long["rescaled"] and np.isfinite(ref_long["lnl"])
    with engine_from_problem(short, rescale=RESCALE_AUTO) as e:
        _check_gradient(e, ref_short, "short branches")
        assert not e.rescaling
        e.set_branch_lengths(long_bl)
        _check_gradient(e, ref_long, "long branches")
        assert e.rescaling
        e.set_branch_lengths(short.branch_lengths)
        _check_gradient(e, _replace(short, rescale=1).gradient(), "short branches again")
        assert e.rescaling
        bl = short.branch_lengths.copy()
        bl[5] = 0.3
        e.set_branch_length(5, bl[5])
        _check_gradient(e, _replace(short, rescale=1, branch_lengths=bl).gradient(), "one branch after that")
        assert e.rescaling
