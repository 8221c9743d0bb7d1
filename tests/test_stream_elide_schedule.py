"""CPU-only: the stored nodes the streamed 4-state walks do not store (phyamd_stream_elisions: build_schedule,
build_stream_tables and stream_elide, no device).

stream_elide_util.check_rule derives the elided set again from the two older exports (phyamd_post_order_parks for the sources
and chunks, phyamd_pre_order_schedule for the sides and the pre-order cuts) and the tree, and holds the export against it node by
node; the trees are upper_park_util's named set (a 64-tip caterpillar of subtrees and a balanced tree of 64 tips among them), a
64-tip ladder, three small trees built for single cases, every one of them with its mirror image, and the bench tree.  The two older exports are built with the switch off, and must be byte for byte what they
were before the switch existed: their digests over the named set are pinned below."""
import hashlib

import numpy as np
import pytest

import lower_park_util as lp
import stream_elide_util as se
import upper_park_util as u
from physher_amd import _lib, synth


@pytest.mark.parametrize("mirror", [False, True])
@pytest.mark.parametrize("name", se.ALL)
def test_rule_node_by_node(name, mirror):
    r = se.reach(name, mirror)
    print(name, "mirrored" if mirror else "", r)
    assert r["count"] <= r["shaped"]
    if mirror:  # both walks order an op's children by subtree size, ties by left / right: of these trees only tie-breaks could move a side
        assert r["count"] == se.reach(name)["count"] and r["shaped"] == se.reach(name)["shaped"]


def test_bench_tree_count():
    """cfg5's tree: 94 shaped nodes (47 beside a tip, 47 beside a cherry), 77 of them elidable when no two may follow each other;
    the reach rule takes one (it waits in the second park slot).  cfg2's tree: 31 of 173 stored nodes (32 by shape, one next to
    a cut)"""
    r = se.check_rule(se.make_tree("bench"))
    print("bench tree:", r)
    assert r["shaped"] == 94
    assert r["count"] <= 77
    assert r["count"] == se.BENCH_ELIDED
    assert r["refused_slot1"] + r["refused_memory"] == 77 - se.BENCH_ELIDED
    cfg2 = se.check_rule(synth.random_tree(500, np.random.default_rng(1)))
    print("cfg2 tree:", cfg2)
    assert cfg2["count"] == se.CFG2_ELIDED


@pytest.mark.parametrize("case", sorted(se.CASES))
def test_cases_are_reached(case):
    name, shown = se.CASES[case]
    assert shown(se.reach(name)), f"{name} no longer reaches: {case}"
    assert se.make_tree(name).tip_count <= 200


def test_chains_alternate():
    """a ladder: 58 shaped rungs in a row; bottom-up, every other one goes (check_rule asserts the alternation inside a chunk)"""
    r = se.reach("caterpillar64")
    assert r["chain"] >= 3 and r["kind_sides"] == {(u.TIP, 0)}
    assert (r["shaped"], r["count"]) == (58, 29)


def test_no_elision_without_the_shape():
    for name in ("balanced64", "balanced40m", "caterpillar", "reuse56m"):
        for mirror in (False, True):
            assert se.reach(name, mirror)["shaped"] == 0 and se.reach(name, mirror)["count"] == 0


def _digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, dtype=np.int32).tobytes())
    return h.hexdigest()


def test_older_exports_are_unchanged():
    """phyamd_pre_order_schedule and phyamd_post_order_parks build their tables with the switch off: the records of every named
    tree, all forms and both slot counts, digest to what they did before stream_elide existed"""
    pre, post, moved = [], [], []
    for name in u.NAMED:
        tree = u.make_tree(name)
        mine = ([], [])
        for form in (0, 1, 2):
            ops, slots = u.pre_order_schedule(tree, form)
            mine[0].extend([ops, np.array([slots])])
        for second in (True, False):
            mine[1].append(lp.post_order_parks(tree, second))
        pre += mine[0]
        post += mine[1]
        got = (_digest(mine[0])[:16], _digest(mine[1])[:16])
        print(f'    "{name}": ("{got[0]}", "{got[1]}"),')
        if got != se.EXPORT_DIGESTS[name]:
            moved.append(name)
    print("pre-order digest", _digest(pre))
    print("post-order digest", _digest(post))
    assert not moved, f"the older exports of these trees have changed: {moved}"
    assert _digest(pre) == se.PRE_ORDER_DIGEST
    assert _digest(post) == se.POST_ORDER_DIGEST


def test_arguments():
    lib = _lib.load()
    tree = u.make_tree("balanced64")
    left = np.ascontiguousarray(tree.left, dtype=np.int32)
    right = np.ascontiguousarray(tree.right, dtype=np.int32)
    assert lib.phyamd_stream_elisions(1, left.ctypes.data, right.ctypes.data, 0, None, 0) == _lib.EINVAL
    assert lib.phyamd_stream_elisions(64, None, right.ctypes.data, 126, None, 0) == _lib.EINVAL
    assert lib.phyamd_stream_elisions(64, left.ctypes.data, right.ctypes.data, 3, None, 0) == _lib.EINVAL  # a tip is no root
    assert lib.phyamd_stream_elisions(64, left.ctypes.data, right.ctypes.data, 126, None, 5) == _lib.EINVAL  # capacity without out
    assert lib.phyamd_stream_elisions(64, left.ctypes.data, right.ctypes.data, 126, None, 0) == 0  # nothing to elide in a balanced tree
    t200 = se.make_tree("random200")
    l2 = np.ascontiguousarray(t200.left, dtype=np.int32)
    r2 = np.ascontiguousarray(t200.right, dtype=np.int32)
    assert lib.phyamd_stream_elisions(200, l2.ctypes.data, r2.ctypes.data, int(t200.root), None, 0) == 10  # capacity 0: the count alone
    assert lib.phyamd_abi_version() == 5
