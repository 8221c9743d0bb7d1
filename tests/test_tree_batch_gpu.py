"""GPU: phyamd_gradient_batch_trees -- lnL and the per-category branch gradient of many TREES on one engine's data and models in one
call -- against the CPU oracle item by item (the oracle Problem with the item's left / right / root / branch_lengths), bit for bit
across batch sizes, positions, chunks and labellings, with the engine untouched, and through every refusal.  Tolerances are the
suite's for single evaluations (tests/test_batch_gpu.py): lnL 1e-10 relative, gradient 1e-9 * max(1, max|g|).  Every parity case
also asserts that all items took the batched walk (items_fast == B, items_sequential == 0) and that the engine is not rescaling."""
import copy

import numpy as np
import pytest

from gpu_util import engine_from_problem, random_problem
from physher_amd import synth
from physher_amd.engine import (GRAD_COMPAT_SCALED, GRAD_FOLD_ROOT_FREQS, RESCALE_ALWAYS, RESCALE_AUTO, RESCALE_NEVER, EngineError)
from test_batch_gpu import _ambiguous_partials, _bits, _deep

pytestmark = pytest.mark.gpu
EINVAL, EUNSUPPORTED = -1, -4


class Items:
    """a batch of trees: left, right [B, N], roots [B], bl [B, N] by the item's node ids"""

    def __init__(self, trees):
        self.left = np.ascontiguousarray([t[0] for t in trees], dtype=np.int32)
        self.right = np.ascontiguousarray([t[1] for t in trees], dtype=np.int32)
        self.roots = np.ascontiguousarray([t[2] for t in trees], dtype=np.int32)
        self.bl = np.ascontiguousarray([t[3] for t in trees], dtype=np.float64)

    def __len__(self):
        return len(self.roots)

    def take(self, idx):
        idx = np.atleast_1d(idx)
        return Items([(self.left[i], self.right[i], self.roots[i], self.bl[i]) for i in idx])

    def args(self):
        return self.left, self.right, self.roots, self.bl


def _tree(T, rng, shape="random"):
    t = synth.random_tree(T, rng, shape=shape)
    bl = t.length.copy()
    bl[t.root] = 0.0
    return t.left.copy(), t.right.copy(), int(t.root), bl


def _relabel(tree, rng, T):
    """the same tree with its internal ids permuted at random, the root somewhere below 2T-2; returns (tree, perm): new = perm[old]"""
    left, right, root, bl = tree
    N = 2 * T - 1
    while True:
        perm = np.concatenate([np.arange(T), T + rng.permutation(T - 1)])
        if T < 3 or perm[root] != N - 1:
            break
    l2, r2, b2 = -np.ones(N, dtype=np.int32), -np.ones(N, dtype=np.int32), np.zeros(N)
    for n in range(N):
        b2[perm[n]] = bl[n]
        if n >= T:
            l2[perm[n]], r2[perm[n]] = perm[left[n]], perm[right[n]]
    return (l2, r2, int(perm[root]), b2), perm


def _mixed(T, shapes, seed, relabel=(1,)):
    rng = np.random.default_rng(seed)
    trees = [_tree(T, rng, s) for s in shapes]
    for i in relabel:
        if i < len(trees):
            trees[i] = _relabel(trees[i], rng, T)[0]
    return Items(trees)


def _oracle(pb, items, b, fold=False):
    q = copy.copy(pb)
    q.left, q.right, q.root = items.left[b].copy(), items.right[b].copy(), int(items.roots[b])
    q.branch_lengths = items.bl[b].copy()
    q.fold_root_freqs = 1 if fold else 0
    return q.gradient()


def _check_against_oracle(pb, items, lnl, g, fold=False):
    for b in range(len(items)):
        ref = _oracle(pb, items, b, fold)
        print(f"item {b}: lnL {lnl[b]!r} oracle {ref['lnl']!r}  max|dg| {np.abs(g[b] - ref['cat_grad']).max():.3e}")
        assert abs(lnl[b] - ref["lnl"]) <= 1e-10 * abs(ref["lnl"]), (b, lnl[b], ref["lnl"])
        assert np.abs(g[b] - ref["cat_grad"]).max() <= 1e-9 * max(1.0, np.abs(ref["cat_grad"]).max()), b
        assert np.all(g[b, items.roots[b], :] == 0.0)


def _run(e, items, flags=0, want_gradient=True):
    lnl, g = e.gradient_batch_trees(*items.args(), flags=flags, want_gradient=want_gradient)
    prof = e.batch_profile()
    assert prof["items_fast"] == len(items) and prof["items_sequential"] == 0, prof
    assert not e.rescaling
    return lnl, g


def _three_taxa():
    """all three rooted topologies of three tips under both labellings of the two internal nodes"""
    trees = []
    for a, b, c in [(0, 1, 2), (0, 2, 1), (1, 2, 0)]:
        for cherry, root in [(3, 4), (4, 3)]:
            left, right = -np.ones(5, dtype=np.int32), -np.ones(5, dtype=np.int32)
            left[cherry], right[cherry] = a, b
            left[root], right[root] = cherry, c
            bl = 0.02 + 0.01 * np.arange(5) + 0.003 * len(trees)
            bl[root] = 0.0
            trees.append((left, right, root, bl))
    return Items(trees)


# (T, P, C, fold, pinv, gaps, ambiguity codes, items)
CASES = {
    "one_op": (2, 1, 1, False, None, 0.0, False, lambda: Items([(np.array([-1, -1, 0]), np.array([-1, -1, 1]), 2, np.array([0.03, 0.07, 0.0]))])),
    "three_taxa": (3, 63, 2, False, None, 0.0, False, _three_taxa),
    "t8_mixed": (8, 65, 1, False, None, 0.0, False, lambda: _mixed(8, ["caterpillar", "balanced"] + ["random"] * 4, 8, relabel=(1, 3))),
    "t37_b64": (37, 238, 4, False, None, 0.05, False, lambda: _mixed(37, ["random"] * 64, 37, relabel=(1, 17, 40))),
    "t37_c8_fold": (37, 700, 8, True, None, 0.0, False, lambda: _mixed(37, ["balanced", "random", "caterpillar"], 38)),
    "t37_ambiguity_fold": (37, 238, 4, True, None, 0.05, True, lambda: _mixed(37, ["random", "random", "balanced"], 39)),
    "t200_b16": (200, 63, 4, False, None, 0.02, False, lambda: _mixed(200, ["caterpillar", "random"] * 8, 200, relabel=(0, 1))),
    "t37_pinv": (37, 238, 4, False, 0.25, 0.03, False, lambda: _mixed(37, ["random", "caterpillar", "balanced"], 41)),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_matches_oracle_item_by_item(case):
    T, P, C, fold, pinv, gaps, ambig, make = CASES[case]
    pb = random_problem(T, P, C, seed=7 * T + P + C, gaps=gaps, pinv=pinv)
    if ambig:
        _ambiguous_partials(pb, 3)
    items = make()
    if len(items) > 1:
        assert any(items.roots[b] != 2 * T - 2 for b in range(len(items)))  # an item with permuted ids and another root id
    with engine_from_problem(pb, rescale=RESCALE_AUTO, tip_mode="partials" if ambig else "states") as e:
        lnl, g = _run(e, items, GRAD_FOLD_ROOT_FREQS if fold else 0)
    _check_against_oracle(pb, items, lnl, g, fold)


def _nni_neighbourhood(pb):
    """all 2 x (internal non-root edges) NNI rearrangements of the problem's tree, lengths carried over by node id"""
    T, N = pb.T, pb.N
    parent = -np.ones(N, dtype=np.int64)
    for n in range(T, N):
        parent[pb.left[n]] = parent[pb.right[n]] = n
    trees = []
    for v in range(T, N):
        if v == pb.root:
            continue
        p = parent[v]
        for side in ("left", "right"):  # this child of v changes places with v's sibling
            left, right = pb.left.copy(), pb.right.copy()
            kids = left if side == "left" else right
            if left[p] == v:
                kids[v], right[p] = right[p], kids[v]
            else:
                kids[v], left[p] = left[p], kids[v]
            trees.append((left, right, pb.root, pb.branch_lengths.copy()))
    return trees


def test_nni_neighbourhood_of_the_engines_tree():
    pb = random_problem(16, 238, 4, seed=16, gaps=0.03)
    trees = _nni_neighbourhood(pb)
    assert len(trees) == 2 * (pb.T - 2)
    own = len(trees)
    items = Items(trees + [(pb.left, pb.right, pb.root, pb.branch_lengths)])
    with engine_from_problem(pb, rescale=RESCALE_AUTO) as e:
        lnl, g = _run(e, items)
        lb, gb = e.gradient_batch(pb.branch_lengths[None, :])
        assert e.batch_profile()["items_fast"] == 1
        l1, g1 = e.gradient()
    _check_against_oracle(pb, items, lnl, g)
    assert len({float(x) for x in lnl[:own]}) > 1  # the neighbours are other trees
    # the engine's own tree: the op builder and the kernel of the lengths batch, hence its bits
    assert _bits(lnl[own]) == _bits(lb[0]) and np.array_equal(_bits(g[own]), _bits(gb[0]))
    assert abs(lnl[own] - l1) <= 1e-10 * abs(l1) and np.abs(g[own] - g1).max() <= 1e-9 * max(1.0, np.abs(g1).max())


def test_an_item_does_not_depend_on_its_batch():
    """item 17 alone, at position 17 of 64 and in a batch cut into >= 3 chunks by a memory cap: the same bits; the lnL-only form
    gives the same lnL bits; permuted items give permuted results"""
    pb = random_problem(37, 700, 4, seed=99, gaps=0.05)
    items = _mixed(37, ["random"] * 64, 64, relabel=(3, 17))
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        e.gradient()  # (the engine's own buffers are made: what it holds besides the batch scratch)
        held = e.profile()["device_bytes"]
        l1, g1 = _run(e, items.take(17))
        assert e.batch_profile()["chunks"] == 1
        l64, g64 = _run(e, items)
        prof = e.batch_profile()
        assert prof["chunks"] == 1, prof
        scratch = prof["scratch_bytes"]
        lo, none = _run(e, items, want_gradient=False)
        assert none is None
        order = np.random.default_rng(1).permutation(64)
        lp, gp = _run(e, items.take(order))
    assert _bits(l1[0]) == _bits(l64[17]) and np.array_equal(_bits(g1[0]), _bits(g64[17]))
    assert np.array_equal(_bits(lo), _bits(l64))
    assert np.array_equal(_bits(lp), _bits(l64[order])) and np.array_equal(_bits(gp), _bits(g64[order]))
    with engine_from_problem(pb, rescale=RESCALE_NEVER, max_device_bytes=int(held + scratch / 3.5)) as e:
        e.gradient()
        assert e.profile()["tiles"] == 1
        lc, gc = _run(e, items)
        assert e.batch_profile()["chunks"] >= 3, e.batch_profile()
    assert np.array_equal(_bits(lc), _bits(l64)) and np.array_equal(_bits(gc), _bits(g64))


def test_relabelling_permutes_the_rows_bit_for_bit():
    """the op order is label-independent (the builder breaks ties by left / right, never by node id), so the same tree under
    another labelling of its internal nodes runs the same arithmetic: the same lnL bits, the gradient's rows permuted"""
    T = 37
    pb = random_problem(T, 238, 4, seed=5, gaps=0.05)
    rng = np.random.default_rng(12)
    trees, perms = [], []
    for shape in ("random", "balanced", "caterpillar"):
        t = _tree(T, rng, shape)
        t2, perm = _relabel(t, rng, T)
        trees += [t, t2]
        perms.append(perm)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        lnl, g = _run(e, Items(trees))
    for i, perm in enumerate(perms):
        assert _bits(lnl[2 * i]) == _bits(lnl[2 * i + 1])
        assert np.array_equal(_bits(g[2 * i + 1][perm]), _bits(g[2 * i]))


def test_the_engine_is_untouched():
    pb = random_problem(37, 700, 4, seed=31, gaps=0.05)
    items = _mixed(37, ["random"] * 16, 2)
    node = 5 if pb.root != 5 else 6
    with engine_from_problem(pb, rescale=RESCALE_AUTO) as e, engine_from_problem(pb, rescale=RESCALE_AUTO) as fresh:
        before = e.gradient()
        plk = e.pattern_log_likelihoods()
        _run(e, items)
        after = e.gradient()
        assert _bits(before[0]) == _bits(after[0]) and np.array_equal(_bits(before[1]), _bits(after[1]))
        assert np.array_equal(_bits(plk), _bits(e.pattern_log_likelihoods()))
        fresh.gradient()
        _run(e, items.take([0, 1, 2]))
        for eng in (e, fresh):
            eng.set_branch_length(node, 0.37)
        a, b = e.gradient(), fresh.gradient()
        assert _bits(a[0]) == _bits(b[0]) and np.array_equal(_bits(a[1]), _bits(b[1]))
        assert _bits(e.log_likelihood()) == _bits(fresh.log_likelihood())


def test_the_two_batches_share_the_scratch():
    """a lengths batch, tree batches that park in fewer and in more upper slots than the engine's tree, the lengths batch again:
    neither kind reads the other's op lists or runs in too few upper slots"""
    pb = random_problem(37, 238, 4, seed=77, shape="caterpillar", gaps=0.03)  # (the engine's tree parks nothing)
    bl = pb.branch_lengths[None, :] * np.random.default_rng(4).uniform(0.5, 1.8, size=(8, pb.N))
    flat = _mixed(37, ["caterpillar"] * 8, 5)
    deep = _mixed(37, ["balanced", "random"] * 4, 6)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as fresh:
        ld, gd = _run(fresh, deep)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        first = e.gradient_batch(bl)
        assert e.batch_profile()["items_fast"] == 8
        lf, gf = _run(e, flat)
        l2, g2 = _run(e, deep)
        last = e.gradient_batch(bl)
        assert e.batch_profile()["items_fast"] == 8
        lf2, gf2 = _run(e, flat)
    assert np.array_equal(_bits(first[0]), _bits(last[0])) and np.array_equal(_bits(first[1]), _bits(last[1]))
    assert np.array_equal(_bits(l2), _bits(ld)) and np.array_equal(_bits(g2), _bits(gd))
    assert np.array_equal(_bits(lf), _bits(lf2)) and np.array_equal(_bits(gf), _bits(gf2))
    _check_against_oracle(pb, flat.take([0, 1]), lf, gf)


def test_capped_engine_is_untouched_by_a_chunked_tree_batch_made_first():
    pb = random_problem(37, 700, 4, seed=99, gaps=0.05)
    items = _mixed(37, ["random"] * 64, 64)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        e.gradient()
        e.branch_hessian_diagonal()
        held = e.profile()["device_bytes"]
        l64, g64 = _run(e, items)
        scratch = e.batch_profile()["scratch_bytes"]
    cap = int(held + scratch / 3.5)
    with engine_from_problem(pb, rescale=RESCALE_NEVER, max_device_bytes=cap) as fresh, \
            engine_from_problem(pb, rescale=RESCALE_NEVER, max_device_bytes=cap) as e:
        assert e.profile()["tiles"] == 1
        lc, gc = _run(e, items)
        assert e.batch_profile()["chunks"] >= 3, e.batch_profile()
        assert e.profile()["device_bytes"] <= cap
        assert np.array_equal(_bits(lc), _bits(l64)) and np.array_equal(_bits(gc), _bits(g64))
        a, b = e.gradient(), fresh.gradient()
        assert _bits(a[0]) == _bits(b[0]) and np.array_equal(_bits(a[1]), _bits(b[1]))
        assert e.profile()["device_bytes"] <= cap
        ha, hb = e.branch_hessian_diagonal(), fresh.branch_hessian_diagonal()
        assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(ha, hb))
        assert e.profile()["device_bytes"] <= cap
        lc, gc = _run(e, items)  # and the batch again, beside the engine's buffers
        assert e.profile()["device_bytes"] <= cap
        assert np.array_equal(_bits(lc), _bits(l64)) and np.array_equal(_bits(gc), _bits(g64))


def _refused(e, items, flags=0):
    with pytest.raises(EngineError) as err:
        e.gradient_batch_trees(*items.args(), flags=flags)
    assert err.value.code == EUNSUPPORTED, err.value
    print(err.value)
    return str(err.value)


def _own(pb, B=2):
    return Items([(pb.left, pb.right, pb.root, pb.branch_lengths)] * B)


def _still_usable(e, pb):
    ref = pb.log_likelihood()["lnl"]
    assert abs(e.log_likelihood() - ref) <= 1e-10 * abs(ref)


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


def test_the_compat_flag_is_refused():
    pb = random_problem(8, 100, 2, seed=3)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        assert "flags" in _refused(e, _own(pb), flags=GRAD_COMPAT_SCALED | GRAD_FOLD_ROOT_FREQS)
        _still_usable(e, pb)
        _run(e, _own(pb), flags=GRAD_FOLD_ROOT_FREQS)


@pytest.mark.parametrize("rescale", [RESCALE_NEVER, RESCALE_AUTO])
def test_underflowing_items_are_reported_in_band(rescale):
    pb = _deep(800, 100, 4, seed=5)
    bl = pb.branch_lengths[None, :] * np.random.default_rng(8).uniform(0.9, 1.2, size=(3, pb.N))
    items = Items([(pb.left, pb.right, pb.root, bl[b]) for b in range(3)])
    with engine_from_problem(pb, rescale=rescale) as e:
        lnl, g = _run(e, items)  # (items_fast == 3, and the engine is still not rescaling)
        assert not np.any(np.isfinite(lnl)) and np.all(np.isnan(g))


def _invalid(kind, pb):
    """item 1 of three is broken"""
    T, N = pb.T, pb.N
    left, right, root = pb.left.copy(), pb.right.copy(), pb.root
    inner = [n for n in range(T, N) if n != root]
    if kind == "two_parents":  # a node that is the child of two nodes
        a, b = inner[0], inner[1]
        left[b] = left[a]
    elif kind == "cycle":  # a and its parent p become each other's child; p's place under its own parent goes to a's old child:
        parent = {int(c): n for n in range(T, N) for c in (left[n], right[n])}  # every node keeps one parent, the root reaches no loop
        a = next(n for n in inner if parent[n] != root)
        p = parent[a]
        g, x = parent[p], left[a]
        left[a] = p
        if left[g] == p:
            left[g] = x
        else:
            right[g] = x
    elif kind == "tip_with_children":
        left[2], right[2] = 0, 1
    elif kind == "root_is_a_tip":
        root = 1
    elif kind == "root_is_a_child":
        root = inner[0]
    elif kind == "child_out_of_range":
        right[inner[0]] = N
    else:
        raise ValueError(kind)
    good = (pb.left, pb.right, pb.root, pb.branch_lengths)
    return Items([good, (left, right, root, pb.branch_lengths), good])


@pytest.mark.parametrize("kind", ["two_parents", "cycle", "tip_with_children", "root_is_a_tip", "root_is_a_child", "child_out_of_range"])
def test_invalid_topologies_name_the_item(kind):
    pb = random_problem(8, 65, 2, seed=9, shape="balanced")
    items = _invalid(kind, pb)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        with pytest.raises(EngineError) as err:
            e.gradient_batch_trees(*items.args())
        print(err.value)
        assert err.value.code == EINVAL and "item 1" in str(err.value), err.value
        good = items.take([0, 2])
        lnl, g = _run(e, good)
    _check_against_oracle(pb, good.take([0]), lnl, g)


@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0, 0]])
def test_shards_agree_with_one_engine(devices):
    """per-item results are added in shard order, as the lengths batch's: equal to 1e-12 relative"""
    pb = random_problem(37, 700, 4, seed=21, gaps=0.05)
    items = _mixed(37, ["random"] * 6 + ["balanced", "caterpillar"], 6)
    with engine_from_problem(pb, rescale=RESCALE_AUTO) as e:
        lnl, g = _run(e, items)
    with engine_from_problem(pb, rescale=RESCALE_AUTO, devices=devices) as e:
        ls, gs = _run(e, items)
        lo, _ = _run(e, items, want_gradient=False)
    assert np.abs(ls - lnl).max() <= 1e-12 * np.abs(lnl).max()
    assert np.abs(lo - lnl).max() <= 1e-12 * np.abs(lnl).max()
    assert np.abs(gs - g).max() <= 1e-12 * max(1.0, np.abs(g).max())
