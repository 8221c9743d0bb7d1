"""CPU: the operands the streamed pre-order walk keeps in registers from an elided node's parent's op to the node's own op
(stream_keep, phyamd_tree_schedule.h; phyamd_stream_keeps: host code only, no device) held against the rule, node by node
(stream_keep_util.check_rule, over phyamd_pre_order_schedule and phyamd_stream_elisions), on the named trees of upper_park_util,
those of stream_elide_util and of stream_pairs_util, every one with its mirror image, and on the bench tree.  The requests of both
descriptor sets that know elided kinds change at the kept nodes alone; the older exports are what they were."""
import numpy as np
import pytest

import stream_elide_util as se
import stream_keep_util as sk
import test_stream_elide_schedule as older
import upper_park_util as u


@pytest.mark.parametrize("mirror", [False, True])
@pytest.mark.parametrize("name", sk.ALL)
def test_rule_node_by_node(name, mirror):
    r = sk.reach(name, mirror)
    print(name, "mirrored" if mirror else "", r)
    assert r["count"] == len(se.stream_elisions(sk.make_tree(name, mirror=mirror)))
    assert r["kept"] == r["reasons"].get(sk.KEPT, 0) and sum(r["reasons"].values()) == r["count"]
    assert sk.OFF not in r["reasons"]
    if mirror:  # (the sides follow the subtree sizes, not left and right: only a tie-break can move a decision)
        assert r["count"] == sk.reach(name)["count"]


def test_bench_tree_count():
    r = sk.check_rule(sk.make_tree("bench"))
    print("bench tree:", r)
    assert r["count"] == se.BENCH_ELIDED == 76
    assert r["kept"] == sk.BENCH_KEPT == 44
    assert sk.OFF not in r["reasons"]


@pytest.mark.parametrize("case", sorted(sk.CASES))
def test_gpu_trees_reach_their_cases(case):
    name, shown = sk.CASES[case]
    assert shown(sk.reach(name)), f"{name} does not reach: {case}: {sk.reach(name)}"
    assert sk.make_tree(name).tip_count <= 200


def test_switch_off_keeps_nothing():
    """(check_rule holds the switch-off records of every tree; here: that a tree with kept operands has none then)"""
    tree = sk.make_tree("caterpillar64")
    on, off = sk.stream_keeps(tree, 1), sk.stream_keeps(tree, 0)
    assert (on[:, sk.REASON] == sk.KEPT).sum() > 0
    assert (off[:, sk.REASON] == sk.OFF).all() and len(off) == len(on)
    assert (off[:, [sk.REQUEST_TF, sk.REQUEST_PLAIN]] == 1).all()


def test_nothing_to_keep_without_an_elision():
    for name in ("balanced64", "balanced40m", "caterpillar", "reuse56m"):
        assert len(sk.stream_keeps(sk.make_tree(name))) == 0


def test_older_exports_are_unchanged():
    """phyamd_pre_order_schedule and phyamd_post_order_parks (pinned in stream_elide_util), phyamd_stream_elisions and
    phyamd_stream_pairs (pinned in stream_keep_util) build their tables without stream_keep"""
    older.test_older_exports_are_unchanged()
    elisions, pairs = sk.older_export_digests()
    print("elisions", elisions)
    print("pairs", pairs)
    assert elisions == sk.ELISIONS_DIGEST
    assert pairs == sk.PAIRS_DIGEST


def test_arguments():
    from physher_amd import _lib
    lib = _lib.load()
    tree = sk.make_tree("random200")
    left = np.ascontiguousarray(tree.left, dtype=np.int32)
    right = np.ascontiguousarray(tree.right, dtype=np.int32)
    assert lib.phyamd_stream_keeps(1, left.ctypes.data, right.ctypes.data, 0, 1, None, 0) == _lib.EINVAL
    assert lib.phyamd_stream_keeps(200, None, right.ctypes.data, int(tree.root), 1, None, 0) == _lib.EINVAL
    assert lib.phyamd_stream_keeps(200, left.ctypes.data, right.ctypes.data, 3, 1, None, 0) == _lib.EINVAL  # a tip is no root
    assert lib.phyamd_stream_keeps(200, left.ctypes.data, right.ctypes.data, int(tree.root), 1, None, 5) == _lib.EINVAL  # capacity without out
    assert lib.phyamd_stream_keeps(200, left.ctypes.data, right.ctypes.data, int(tree.root), 1, None, 0) == len(se.stream_elisions(tree))
    balanced = u.make_tree("balanced64")
    bl = np.ascontiguousarray(balanced.left, dtype=np.int32)
    br = np.ascontiguousarray(balanced.right, dtype=np.int32)
    assert lib.phyamd_stream_keeps(64, bl.ctypes.data, br.ctypes.data, int(balanced.root), 1, None, 0) == 0
