"""CPU-only: the post-order walk's park slots in the host schedule (phyamd_post_order_parks: build_schedule and
chunk_post_order, no device).  A stored child waits in one of a wave's two register slots while its sibling's subtree is
walked; the kernel neither checks that a slot is free when it writes it nor that it holds the right node when it reads it, so the
schedule has to: no slot holds two values at once, every slot read finds the value its own chunk wrote, every carried child is
the result of the op in front, and nothing is left parked at a chunk's end."""
import numpy as np
import pytest

from lower_park_util import (CARRIED, CHUNK, CUT, LEFT, MEMORY, NODE, PARK, RIGHT, SLOT0, SLOT1, SRC_LEFT, SRC_RIGHT, TREES, make_tree,
                             post_order_parks, sources)
from physher_amd import _lib, synth

BENCH = "bench1000"


def _tree(name):
    return synth.random_tree(1000, np.random.default_rng(1)) if name == BENCH else make_tree(name)


def _check_invariants(ops):
    slot = {SLOT0: None, SLOT1: None}
    prev, chunk, stored = None, -1, set()
    for op in ops:
        if op[CHUNK] != chunk:
            assert slot == {SLOT0: None, SLOT1: None}, f"chunk {chunk} ends with a value parked: {slot}"
            assert op[CHUNK] == chunk + 1
            chunk, prev = int(op[CHUNK]), None
        for child, src, bit in ((op[LEFT], op[SRC_LEFT], 1), (op[RIGHT], op[SRC_RIGHT], 2)):
            if src < 0:
                assert child not in stored, f"node {child} has an op but is not read as a stored child"
                continue
            assert child in stored, f"node {child} is read before it is written"
            if src == CARRIED:
                assert prev == child, f"op {op[NODE]}: carried child {child}, the op in front made {prev}"
            elif src in (SLOT0, SLOT1):
                assert slot[src] == child, f"op {op[NODE]}: slot {src - SLOT0} holds {slot[src]}, not {child}"
                slot[src] = None
                assert not op[CUT] & bit, f"op {op[NODE]}: a park spans a chunk boundary"
            else:
                assert src == MEMORY
        for s, bit in ((SLOT0, 1), (SLOT1, 2)):
            if op[PARK] & bit:
                assert slot[s] is None, f"op {op[NODE]}: slot {s - SLOT0} still holds {slot[s]}"
                slot[s] = int(op[NODE])
        stored.add(int(op[NODE]))
        prev = int(op[NODE])
    assert slot == {SLOT0: None, SLOT1: None}, f"the walk ends with a value parked: {slot}"


@pytest.mark.parametrize("name", TREES + (BENCH,))
@pytest.mark.parametrize("second_slot", [True, False])
def test_park_invariants(name, second_slot):
    ops = post_order_parks(_tree(name), second_slot)
    assert len(ops) > 0
    _check_invariants(ops)
    if not second_slot:
        assert not (ops[:, [SRC_LEFT, SRC_RIGHT]] == SLOT1).any() and not (ops[:, PARK] & 2).any()


@pytest.mark.parametrize("name", TREES + (BENCH,))
def test_second_slot_only_moves_memory_reads(name):
    """same ops in the same order; a child takes slot 1 only where the one-slot schedule read it from memory, nothing else moves"""
    tree = _tree(name)
    one, two = post_order_parks(tree, False), post_order_parks(tree, True)
    assert (one[:, :4] == two[:, :4]).all() and (one[:, CUT] == two[:, CUT]).all()
    for col in (SRC_LEFT, SRC_RIGHT):
        moved = one[:, col] != two[:, col]
        assert (one[moved, col] == MEMORY).all() and (two[moved, col] == SLOT1).all()
    assert ((one[:, PARK] & 1) == (two[:, PARK] & 1)).all()


@pytest.mark.parametrize("name", TREES)
def test_test_trees_reach_the_second_slot_and_memory(name):
    slot1, memory = sources(name)
    assert slot1 >= 1 and memory >= 1, (slot1, memory)


def test_bench_tree_counts():
    """the counts DESIGN.md section 3 records for the headline tree: 32 stored children come from memory with one slot -- 5 beside a
    cut, 22 that the second slot takes, 5 nested deeper"""
    tree = _tree(BENCH)
    one, two = post_order_parks(tree, False), post_order_parks(tree, True)
    mem1 = one[:, [SRC_LEFT, SRC_RIGHT]] == MEMORY
    beside_cut = np.stack([(one[:, CUT] & 1) != 0, (one[:, CUT] & 2) != 0], axis=1)
    took = two[:, [SRC_LEFT, SRC_RIGHT]] == SLOT1
    assert len(one) == 360
    assert int(mem1.sum()) == 32
    assert int((mem1 & beside_cut).sum()) == 5
    assert int(took.sum()) == 22 and not (took & beside_cut).any()
    assert int((mem1 & ~beside_cut & ~took).sum()) == 5


def test_bad_arguments_are_reported():
    lib = _lib.load()
    tree = make_tree("balanced64")
    left, right = tree.left.copy(), tree.right.copy()
    assert lib.phyamd_post_order_parks(1, left.ctypes.data, right.ctypes.data, 0, 1, None, 0) == _lib.EINVAL
    assert lib.phyamd_post_order_parks(64, None, right.ctypes.data, 126, 1, None, 0) == _lib.EINVAL
    assert lib.phyamd_post_order_parks(64, left.ctypes.data, right.ctypes.data, 3, 1, None, 0) == _lib.EINVAL  # a tip is no root
    assert b"root" in lib.phyamd_last_error()
    assert lib.phyamd_post_order_parks(64, left.ctypes.data, right.ctypes.data, 126, 1, None, 0) == 15  # capacity 0: the count alone
