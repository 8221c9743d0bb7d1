"""GPU: the 20 / 60 / 61-state kernels against the oracle at sizes where a wave takes several 16-pattern tiles (k_lower_gen,
k_upper_gen with FOLD, SCALE and HESS, and the kernels that follow them per level) and a workgroup of the post-order walk several
work units (k_lower_gen_walk).

The engine runs a periodic alignment (tests/periodic_util.py): P patterns, column j = column j mod 257 of a 257-pattern problem,
independent integer weights; the oracle runs the 257 patterns with the weights summed per residue class.  Sums over patterns (lnL,
gradients, the Hessian diagonal, the parameter gradient) are compared with the oracle's, per-pattern lnL and the partials read
back at every position j with the oracle's at j mod 257, and positions j and j + 257 of the engine's own arrays bit for bit.

Every case asks phyamd_get_general_profile whether the pass it checks took more than one tile per wave (the walk: at least two
units per workgroup) and FAILS if not: on another card, or after a change to the chooser, the pattern counts below have to grow.
They are the smallest of 1024 n + 27 (never a multiple of 16) at which every case's conditions still hold with twice the resident
workgroups measured on the MI355X (768 / 512 at 20 states, 256 at 60 and 61, 512 for the walk).  Tolerances: DESIGN.md section 4, the Hessian rows as tests/test_branch_hessian_gpu.py, the parameter
gradient as test_parameter_gradient_generic_states."""
import functools

import numpy as np
import pytest

from gpu_util import engine_from_problem, random_problem
from hessian_util import branch_hessian_diagonal
from oracle import phyoracle as po
from periodic_util import K, assert_periodic_bits, expand, level_tiles, node_levels, periodic_pair
from physher_amd.engine import GRAD_COMPAT_SCALED, GRAD_FOLD_ROOT_FREQS, RESCALE_ALWAYS, RESCALE_NEVER, EngineError

pytestmark = pytest.mark.gpu

P_LEVELS = 16411  # cases a-f (case d, 24 taxa x 1 category at 256 slots, is the one that needs it): 1025 tiles and 11 patterns
P_INCREMENTAL = 50203  # case h: a pass of ONE op per level takes a second tile beyond slots / C workgroups of 128 patterns: 4 x 393 > 2 x 768
P_WALK = 65563  # case g: 513 pattern groups x 4 categories = 2052 units >= 2 x (2 x 512) workgroups


# ---- problems and references, made once ------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _pair(S, T, C, rescale, P):
    period = random_problem(T, K, C, seed=7000 + S + T + C + rescale, S=S, gaps=0.05, bl=(0.3, 0.9) if rescale else (0.01, 0.1), rescale=rescale)
    return periodic_pair(period, P, seed=S + T)


@functools.lru_cache(maxsize=None)
def _oracle(S, T, C, rescale, P, fold=0, compat=0, partials=False):
    """the oracle's gradient call on the 257 patterns (shared between the cases: read, never written)"""
    small = _pair(S, T, C, rescale, P)[1]
    small.fold_root_freqs, small.compat_scaled_gradient = fold, compat
    try:
        return small.gradient(want_partials=partials)
    finally:
        small.fold_root_freqs = small.compat_scaled_gradient = 0


@functools.lru_cache(maxsize=None)
def _oracle_hessian(S, T, C, rescale, P):
    return branch_hessian_diagonal(_pair(S, T, C, rescale, P)[1])


# ---- the conditions: which launches the checks below have reached ---------------------------------------------------------------

def _reached(e, lower=False, upper=False, spread=False, hess=False):
    """the last post-order (lower) / pre-order (upper) pass took at least two tiles per wave on some level; spread: and fewer on
    another"""
    g = e.general_profile()
    msg = f"slots: post-order {g['lower_slots']}, pre-order {g['upper_slots']}; the pattern counts of this file are too small for this card: {g}"
    if lower:
        assert g["lower_family"] == 0 and g["lower_tiles_max"] >= 2, msg
        assert not spread or g["lower_tiles_min"] < g["lower_tiles_max"], msg
    if upper:
        assert g["upper_levels"] >= 1 and g["upper_hess"] == int(hess) and g["upper_tiles_max"] >= 2, msg
        assert not spread or g["upper_tiles_min"] < g["upper_tiles_max"], msg
    return g


# ---- comparisons -----------------------------------------------------------------------------------------------------------------

def _check_sums(lnl, cg, ref, what):
    err = np.abs(cg - ref["cat_grad"]).max()
    tol = 1e-9 * max(1.0, np.abs(ref["cat_grad"]).max())
    print(f"{what}: lnL {lnl!r} (oracle {ref['lnl']!r}), gradient error {err:.3e} (bound {tol:.3e})")
    assert abs(lnl - ref["lnl"]) <= 1e-10 * abs(ref["lnl"]), (what, lnl, ref["lnl"])
    assert err <= tol, (what, err, tol, np.unravel_index(np.abs(cg - ref["cat_grad"]).argmax(), cg.shape))


def _check_pattern_lnl(e, ref):
    plk = e.pattern_log_likelihoods()
    np.testing.assert_allclose(plk, expand(ref["pattern_lk"], e.P, 0), rtol=1e-11, atol=1e-11)
    assert_periodic_bits(plk, 0)


def _check_partials(e, node, want, upper=False):
    """node's partial [C][P][S] at every position against the oracle's [C][257][S]"""
    got = e.partials(node, upper=upper)
    np.testing.assert_allclose(got, expand(want[node], e.P, 1), rtol=1e-9, atol=1e-300, err_msg=f"{'upper' if upper else 'lower'} of node {node}")
    assert_periodic_bits(got, 1)


def _lower_nodes(small, P, g):
    """Nodes to read back on an engine that stores every internal node: the root, a cherry's parent, and for every tile count of
    the post-order pass the parent of a node computed with it (a node's partial is formed from its children's stored arrays: it is
    the parent's that shows them).  Also pins the restatement of the chooser to what the launcher reported."""
    height, depth, parent = node_levels(small)
    tiles = level_tiles(small, P, g["lower_slots"], height)
    assert (min(tiles.values()), max(tiles.values())) == (g["lower_tiles_min"], g["lower_tiles_max"]), (tiles, g)
    nodes = {small.root}
    cherry = next(n for n in range(small.T, small.N) if small.left[n] < small.T and small.right[n] < small.T and n != small.root)
    nodes.add(int(parent[cherry]))
    for count in sorted(set(tiles.values())):
        lv = next(l for l, t in tiles.items() if t == count)
        m = next(n for n in range(small.T, small.N) if height[n] == lv)
        nodes.add(int(parent[m]) if m != small.root else m)
    return sorted(nodes)


def _upper_nodes(small, P, g):
    """a tip and an internal node whose uppers to read: the deepest tip, and a child of the widest pre-order level"""
    height, depth, parent = node_levels(small)
    tiles = level_tiles(small, P, g["upper_slots"], depth)
    assert (min(tiles.values()), max(tiles.values())) == (g["upper_tiles_min"], g["upper_tiles_max"]), (tiles, g)
    tip = int(np.argmax(depth[:small.T]))
    widest = max(tiles, key=lambda lv: (tiles[lv], lv))
    inner = next((n for n in range(small.T, small.N) if depth[n] == widest + 1), None)
    if inner is None:
        inner = next(n for n in range(small.T, small.N) if n != small.root)
    return tip, int(inner)


def _plain_case(S, T, C, spread, P=P_LEVELS):
    """cases a, c (plain), d: lnL, per-pattern lnL, the default and the folded gradient; then with every partial kept: the same, the
    chosen lowers and two uppers.  spread: the passes must also take several tile counts in one evaluation"""
    key = (S, T, C, 0, P)
    big, small = _pair(*key)
    ref, ref_fold = _oracle(*key, partials=True), _oracle(*key, fold=1)
    with engine_from_problem(big, rescale=RESCALE_NEVER) as e:
        lnl, cg = e.gradient()
        g = _reached(e, lower=e.general_profile()["lower_family"] == 0, upper=True, spread=spread)
        _check_sums(lnl, cg, ref, f"default schedule (post-order family {g['lower_family']})")
        _check_pattern_lnl(e, ref)
        _check_sums(*e.gradient(GRAD_FOLD_ROOT_FREQS), ref_fold, "default schedule, folded")
        _reached(e, upper=True, spread=spread)
        e.set_keep_partials(True)
        lnl, cg = e.gradient()
        g = _reached(e, lower=True, upper=True, spread=spread)
        print(f"slots {g['lower_slots']} / {g['upper_slots']}, tiles {g['lower_tiles_min']}-{g['lower_tiles_max']} / {g['upper_tiles_min']}-{g['upper_tiles_max']}")
        _check_sums(lnl, cg, ref, "every node stored")
        _check_pattern_lnl(e, ref)
        for n in _lower_nodes(small, P, g):
            _check_partials(e, n, ref["lower"])
        for n in _upper_nodes(small, P, g):
            _check_partials(e, n, ref["upper"], upper=True)
        _check_sums(*e.gradient(GRAD_FOLD_ROOT_FREQS), ref_fold, "every node stored, folded")
        _reached(e, upper=True, spread=spread)


def _rescaled_case(S, T, C, spread, P=P_LEVELS):
    """cases b, c (rescaled): the three gradient modes, per-pattern lnL (the scale factors), the chosen lowers"""
    key = (S, T, C, 1, P)
    big, small = _pair(*key)
    ref = _oracle(*key, partials=True)
    assert ref["rescaled"]
    with engine_from_problem(big, rescale=RESCALE_ALWAYS) as e:
        lnl, cg = e.gradient()
        assert e.rescaling
        g = _reached(e, lower=True, upper=True, spread=spread)
        print(f"slots {g['lower_slots']} / {g['upper_slots']}, tiles {g['lower_tiles_min']}-{g['lower_tiles_max']} / {g['upper_tiles_min']}-{g['upper_tiles_max']}")
        _check_sums(lnl, cg, ref, "rescaled, default")
        _check_pattern_lnl(e, ref)
        for n in _lower_nodes(small, P, g):  # (rescaled evaluations store every internal node)
            _check_partials(e, n, ref["lower"])
        _check_sums(*e.gradient(GRAD_COMPAT_SCALED), _oracle(*key, compat=1), "rescaled, per-category denominators")
        _reached(e, upper=True, spread=spread)
        _check_sums(*e.gradient(GRAD_FOLD_ROOT_FREQS), _oracle(*key, fold=1), "rescaled, folded")
        _reached(e, upper=True, spread=spread)


def test_profile_before_a_pass_on_shards_and_at_four_states():
    """nothing launched: family -1 and no levels; a sharded handle reports its first shard, which chooses its tiles from its own
    pattern count; a 4-state engine is refused with the condition in the message"""
    big, small = _pair(20, 64, 2, 1, P_LEVELS)
    with engine_from_problem(big, rescale=RESCALE_ALWAYS) as one, engine_from_problem(big, rescale=RESCALE_ALWAYS, devices=[0, 0]) as two:
        g = one.general_profile()
        assert g["lower_family"] == -1 and g["lower_levels"] == 0 and g["upper_levels"] == 0 and g["walk_units"] == 0, g
        lnl = one.log_likelihood()
        g = one.general_profile()
        assert g["lower_family"] == 0 and g["upper_levels"] == 0, g  # (a post-order pass alone leaves the pre-order record as it was)
        assert abs(two.gradient()[0] - lnl) <= 1e-12 * abs(lnl)
        h = two.general_profile()
        height, depth, parent = node_levels(small)
        first = (P_LEVELS + 63) // 64 // 2 * 64  # (two shards: the range of 64-pattern blocks, bisected)
        half = level_tiles(small, first, h["lower_slots"], height)
        assert (h["lower_tiles_min"], h["lower_tiles_max"]) == (min(half.values()), max(half.values())) != (g["lower_tiles_min"], g["lower_tiles_max"]), (h, g)
    with engine_from_problem(random_problem(5, 40, 1, seed=1)) as e:
        e.log_likelihood()
        with pytest.raises(EngineError) as err:
            e.general_profile()
        assert err.value.code == -4 and "phyamd_get_general_profile" in str(err.value) and "4 states" in str(err.value)


def test_a_20_states_plain():
    _plain_case(20, 64, 4, spread=True)


def test_b_20_states_rescaled():
    _rescaled_case(20, 64, 2, spread=False)


@pytest.mark.parametrize("rescale", [0, 1])
def test_c_61_states(rescale):
    (_rescaled_case if rescale else _plain_case)(61, 32, 2, spread=True)


def test_d_60_states_plain():
    _plain_case(60, 24, 1, spread=False)


@pytest.mark.parametrize("S,T,C,rescale", [(20, 64, 4, 0), (20, 64, 2, 1), (61, 32, 2, 0)])
def test_e_hessian_diagonal(S, T, C, rescale):
    """k_upper_gen's HESS form with several tiles per wave, k_hess_gen over the bisected slab's workgroups"""
    key = (S, T, C, rescale, P_LEVELS)
    big, small = _pair(*key)
    lr, r1, r2 = _oracle_hessian(*key)
    with engine_from_problem(big, rescale=RESCALE_ALWAYS if rescale else RESCALE_NEVER) as e:
        lnl, d1, d2 = e.branch_hessian_diagonal()
        g = _reached(e, lower=e.general_profile()["lower_family"] == 0, upper=True, hess=True)
        e1, e2 = np.abs(d1 - r1).max(), np.abs(d2 - r2).max()
        print(f"slots {g['lower_slots']} / {g['upper_slots']}, pre-order tiles {g['upper_tiles_min']}-{g['upper_tiles_max']}; d1 error {e1:.3e}, d2 error {e2:.3e}")
        assert abs(lnl - lr) <= 1e-10 * abs(lr), (lnl, lr)
        assert e1 <= 1e-9 * max(1.0, np.abs(r1).max()), (e1, int(np.abs(d1 - r1).argmax()))
        assert e2 <= 1e-9 * max(1.0, np.abs(r2).max()), (e2, int(np.abs(d2 - r2).argmax()))
        assert d1[small.root] == 0.0 and d2[small.root] == 0.0


def test_f_parameter_gradient():
    """the parameter kernels' grids over patterns and k_param_sum_gen's sum over (branch, category) rows, on the partials a
    several-tile evaluation stored"""
    S, T, C = 20, 17, 3
    big, small = _pair(S, T, C, 0, P_LEVELS)
    rng = np.random.default_rng(S + T)
    dQ = rng.normal(size=(5, S, S))
    dQ -= dQ.sum(axis=2, keepdims=True) * np.eye(S)[None]
    _, want = po.parameter_gradient(small, dQ)
    ref = _oracle(S, T, C, 0, P_LEVELS)
    with engine_from_problem(big, rescale=RESCALE_NEVER) as e:
        e.set_rate_matrix_derivatives(dQ)
        lnl, cg, pg = e.parameter_gradient()
        g = _reached(e, lower=True, upper=True)
        err = np.abs(pg - want).max()
        print(f"slots {g['lower_slots']} / {g['upper_slots']}, tiles {g['lower_tiles_min']}-{g['lower_tiles_max']} / {g['upper_tiles_min']}-{g['upper_tiles_max']}; parameter gradient error {err:.3e} of {np.abs(want).max():.3e}")
        _check_sums(lnl, cg, ref, "parameter gradient's own branch gradient")
        assert err <= 1e-9 * max(1.0, np.abs(want).max()), (err, pg, want)
        np.testing.assert_allclose(e.root_frequency_term(), po.root_frequency_term(small), rtol=1e-10)


def test_g_post_order_walk_with_several_units_per_workgroup():
    """k_lower_gen_walk: a workgroup that draws a second unit from the counter stages its LDS images again behind the barrier in
    front of next_unit"""
    key = (20, 12, 4, 0, P_WALK)
    big, small = _pair(*key)
    ref = _oracle(*key, partials=True)
    with engine_from_problem(big, rescale=RESCALE_NEVER) as e:
        lnl, cg = e.gradient()
        g = e.general_profile()
        print(f"walk: slots {g['lower_slots']}, units {g['walk_units']}, workgroups {g['walk_workgroups']}")
        assert g["lower_family"] == 1 and g["walk_units"] >= 2 * g["walk_workgroups"] >= 2, f"slots: {g['lower_slots']}; too few patterns for this card: {g}"
        _check_sums(lnl, cg, ref, "walk")
        _check_pattern_lnl(e, ref)
        # what the walk stores: the root's partial, read as it is, and the stored children of nodes whose partials are re-formed from them
        stored = [n for n in range(small.T, small.N) if n == small.root or not (small.left[n] < small.T and small.right[n] < small.T)]
        _, _, parent = node_levels(small)
        deepest = next(n for n in stored if all(ch < small.T or ch not in stored for ch in (small.left[n], small.right[n])))
        for n in sorted({small.root, int(parent[deepest]) if deepest != small.root else deepest}):
            _check_partials(e, n, ref["lower"])
        assert e.general_profile()["lower_family"] == 1  # (reading back has launched no other post-order pass)


@pytest.mark.parametrize("keep", [False, True])
def test_h_incremental_pass_after_one_branch_length(keep):
    """one op per level: the incremental post-order pass (always k_lower_gen) chooses other tile counts than the pass that stored
    the partials it reads -- the walk on a default engine, k_lower_gen over whole levels on one that keeps every partial"""
    S, T, C = 20, 64, 4
    big, small = _pair(S, T, C, 0, P_INCREMENTAL)
    height, depth, parent = node_levels(small)
    node = int(np.argmax(np.where(np.arange(small.N) >= small.T, depth, -1)))  # the deepest internal node
    changed = po.Problem(small.left, small.right, small.root, small.weights, small.eval, small.evec, small.ivec, small.freqs, small.cat_rates,
                         small.cat_props, small.branch_lengths.copy(), tip_states=small.tip_states)
    changed.branch_lengths[node] *= 1.7
    ref = changed.gradient(want_partials=True)
    with engine_from_problem(big, rescale=RESCALE_NEVER) as e:
        e.set_keep_partials(keep)
        e.gradient()
        full = _reached(e, lower=keep, upper=True, spread=True)
        assert full["lower_family"] == (0 if keep else 1), full
        e.set_branch_length(node, changed.branch_lengths[node])
        lnl, cg = e.gradient()
        g = _reached(e, lower=True, upper=True)
        print(f"slots {g['lower_slots']} / {g['upper_slots']}: full pass family {full['lower_family']}, {full['lower_levels']} levels, tiles "
              f"{full['lower_tiles_min']}-{full['lower_tiles_max']}; incremental pass {g['lower_levels']} levels, tiles {g['lower_tiles_min']}-{g['lower_tiles_max']}")
        if keep:  # the node itself and every ancestor, each alone on its level
            assert g["lower_levels"] == depth[node] + 1, (g, depth[node])
            assert (g["lower_tiles_min"], g["lower_tiles_max"]) != (full["lower_tiles_min"], full["lower_tiles_max"]), (g, full)
        _check_sums(lnl, cg, ref, "after one branch length")
        _check_pattern_lnl(e, ref)
        _check_partials(e, small.root, ref["lower"])
