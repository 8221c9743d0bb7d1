"""CPU: the pair ops of the streamed pre-order walk (stream_pairs, phyamd_tree_schedule.h; phyamd_stream_pairs: host code only, no
device) held against the rule, op by op, on the named trees of upper_park_util, those of stream_elide_util and a few built for
this (stream_pairs_util.check_rule): a pair only where every condition holds and every op that meets them fused; none across a
chunk boundary; a second DEEP child, a fringe sibling, an elided sibling and a tip beside a DEEP child of five or six tips
refused; every branch term once, at the slab position it has in the two-op form; the op behind a pair with a stored sibling
reading registers and no slot; the tables every other pass reads the same bytes with the switch on and off."""
import numpy as np
import pytest

import stream_pairs_util as sp
import upper_park_util as u


@pytest.mark.parametrize("name", sp.ALL)
def test_export_follows_the_rule(name):
    r = sp.reach(name)
    print(name, {k: r[k] for k in ("count", "core", "tip", "carry", "carry_from", "parent_src", "reasons")})
    assert r["count"] == r["reasons"].get(sp.FUSED, 0) == r["reasons"].get(sp.ABSORBED, 0) == r["core"] + r["tip"]
    assert r["carry"] <= r["core"]


@pytest.mark.parametrize("case", sorted(sp.CASES))
def test_gpu_trees_reach_their_cases(case):
    tree, shown = sp.CASES[case]
    assert shown(sp.reach(tree)), f"{tree} does not reach: {case}"


def test_refusals_by_kind():
    """pairs_gallery puts every DEEP shape beside a tip and a stored node, and one beside a cherry, a cherry + tip and a second DEEP node"""
    tree = sp.make_tree("pairs_gallery")
    rec = sp.stream_pairs(tree)
    refused = rec[rec[:, sp.REASON] == sp.BAD_SIBLING]
    assert {u.CHERRY, u.CHERRY_TIP, u.DEEP} <= set(refused[:, sp.SIBLING_KIND].tolist())
    room = rec[rec[:, sp.REASON] == sp.NO_ROOM]
    assert len(room) > 0 and (room[:, sp.SIBLING_KIND] == u.TIP).all() and set(room[:, sp.CHILD_TIPS].tolist()) == {5, 6}
    fused = rec[rec[:, sp.REASON] == sp.FUSED]
    assert (fused[fused[:, sp.SIBLING_KIND] == u.TIP][:, sp.CHILD_TIPS] == 4).all()


def test_an_elided_sibling_is_refused():
    """random200: a DEEP child beside a stored node that the walks do not store (phyamd_stream_elisions) keeps its own op"""
    rec = sp.stream_pairs(sp.make_tree("random200"))
    kinds = set(rec[rec[:, sp.REASON] == sp.BAD_SIBLING][:, sp.SIBLING_KIND].tolist())
    assert kinds & {sp.SK_CORE_TIP, sp.SK_CORE_CHERRY}, kinds


def test_chunked_walk():
    """target: three chunks; no pair's two ops sit in different chunks and no cut root is handed on in registers (check_rule
    asserts both for every tree; here: that the tree has chunks and pairs at all)"""
    rec = sp.stream_pairs(sp.make_tree("target"))
    assert rec[:, sp.CHUNK].max() >= 2 and (rec[:, sp.REASON] == sp.FUSED).sum() > 0


def test_bench_tree_count():
    r = sp.check_rule(sp.make_tree("bench"))
    print("bench tree:", {k: r[k] for k in ("count", "core", "tip", "carry", "carry_from", "reasons")})
    assert r["count"] == sp.BENCH_PAIRS


def test_bad_arguments():
    from physher_amd import _lib
    lib = _lib.load()
    tree = sp.make_tree("root_pair")
    left = np.ascontiguousarray(tree.left, dtype=np.int32)
    right = np.ascontiguousarray(tree.right, dtype=np.int32)
    assert lib.phyamd_stream_pairs(1, left.ctypes.data, right.ctypes.data, 0, 1, None, 0) < 0
    assert lib.phyamd_stream_pairs(tree.tip_count, None, right.ctypes.data, int(tree.root), 1, None, 0) < 0
    assert lib.phyamd_stream_pairs(tree.tip_count, left.ctypes.data, right.ctypes.data, int(tree.root), 1, None, 4) < 0
    assert lib.phyamd_stream_pairs(tree.tip_count, left.ctypes.data, right.ctypes.data, int(tree.root), 1, None, 0) == len(sp.stream_pairs(tree))
