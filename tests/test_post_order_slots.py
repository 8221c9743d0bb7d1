"""CPU-only: the contract of the post-order pass that phyamd_pattern_log_likelihoods_trees walks (phyamd_post_order_slots: the host
schedule alone, no device).  k_sitelnl_walk4 checks none of it, so the schedule has to:
  * the ops are the internal nodes in the batched walk's post-order: depth first, the larger subtree first, ties by left / right;
  * a tip child has no source; every internal child is read from exactly where its op put it -- the registers of the op directly in
    front, or a slot that still holds it -- and every result is read once;
  * no slot is written while it holds an unread result (a slot an op has read may be the one it fills), indices are below `slots`;
  * slots <= max(0, floor(log2 T) - 1): the result that waits while a sibling subtree is walked belongs to a subtree at least as
    large, so a subtree of n tips parks at most d(n) = max(d(larger), 1 + d(smaller)) with smaller <= n / 2 and d(2) = d(3) = 0;
  * a caterpillar uses none, a perfectly balanced tree of 2^k tips k - 1."""
import math

import numpy as np
import pytest

import upper_park_util as u
from physher_amd import _lib, synth

TIP, CARRY, ROOT = -1, -2, -1


def post_order_slots(tree):
    lib = _lib.load()
    T = tree.tip_count
    left = np.ascontiguousarray(tree.left, dtype=np.int32)
    right = np.ascontiguousarray(tree.right, dtype=np.int32)
    out = np.full((T, 6), -7, dtype=np.int32)
    slots = np.full(1, -7, dtype=np.int32)
    n = lib.phyamd_post_order_slots(T, left.ctypes.data, right.ctypes.data, int(tree.root), out.ctypes.data, T, slots.ctypes.data)
    assert n >= 0, lib.phyamd_last_error()
    assert n == T - 1
    return out[:n], int(slots[0])


def _expected_order(tree):
    """the internal nodes depth first, the larger subtree first, ties by left / right"""
    T, left, right = tree.tip_count, tree.left, tree.right
    size = {}
    stack = [(int(tree.root), False)]
    while stack:
        n, done = stack.pop()
        if n < T:
            size[n] = 1
        elif done:
            size[n] = 1 + size[int(left[n])] + size[int(right[n])]
        else:
            stack += [(n, True), (int(left[n]), False), (int(right[n]), False)]
    order, stack = [], [(int(tree.root), False)]
    while stack:
        n, done = stack.pop()
        if done:
            order.append(n)
            continue
        l, r = int(left[n]), int(right[n])
        first, second = (l, r) if size[l] >= size[r] else (r, l)
        stack.append((n, True))
        if second >= T:
            stack.append((second, False))
        if first >= T:
            stack.append((first, False))
    return order


def check_contract(tree, ops, slots):
    T = tree.tip_count
    assert [int(x) for x in ops[:, 0]] == _expected_order(tree)
    holds = {}      # slot -> the node whose unread result it holds
    in_regs = None  # the node whose result the op in front handed on
    most = 0
    for i, (node, l, r, src_l, src_r, dst) in enumerate(ops.tolist()):
        assert (l, r) == (int(tree.left[node]), int(tree.right[node]))
        carried = 0
        for child, src in ((l, src_l), (r, src_r)):
            if child < T:
                assert src == TIP, (i, child, src)
            elif src == CARRY:
                assert in_regs == child, (i, child, in_regs)
                carried += 1
            else:
                assert 0 <= src < slots and holds.pop(src, None) == child, (i, child, src, holds)
        assert carried == (1 if in_regs is not None else 0), (i, "a result handed on in registers is read by the very next op")
        in_regs = None
        if i == len(ops) - 1:
            assert dst == ROOT and node == tree.root
        elif dst == CARRY:
            in_regs = node
            assert node in (int(ops[i + 1, 1]), int(ops[i + 1, 2]))
        else:
            assert 0 <= dst < slots and dst not in holds, (i, dst, holds)
            assert node not in (int(ops[i + 1, 1]), int(ops[i + 1, 2])), (i, "stored although the next op is its parent")
            holds[dst] = node
        most = max(most, len(holds))
    assert not holds and in_regs is None
    assert slots == most  # (every slot counted is used at once: the list wastes none)
    assert slots <= max(0, int(math.floor(math.log2(T))) - 1), (T, slots)
    return slots


@pytest.mark.parametrize("name", u.NAMED)
def test_named_trees(name):
    tree = u.make_tree(name)
    for t in (tree, u.mirrored(tree)):
        check_contract(t, *post_order_slots(t))


def test_random_trees():
    rng = np.random.default_rng(2024)
    seen = set()
    for i in range(500):
        T = int(rng.integers(2, 301))
        shape = ("random", "random", "random", "balanced", "caterpillar")[i % 5]
        tree = synth.random_tree(T, np.random.default_rng(1000 + i), shape=shape)
        seen.add(check_contract(tree, *post_order_slots(tree)))
    assert {0, 1, 2, 3} <= seen, seen


def _nested(shape):
    return u.from_nested(shape)


def test_small_trees_built_here():
    two = _nested((0, 0))
    ops, slots = post_order_slots(two)
    assert ops.tolist() == [[2, 0, 1, TIP, TIP, ROOT]] and slots == 0
    four = _nested(((0, 0), (0, 0)))  # tips 0..3, cherries 4 and 5, root 6: the tie goes to the left cherry
    ops, slots = post_order_slots(four)
    assert ops.tolist() == [[4, 0, 1, TIP, TIP, 0], [5, 2, 3, TIP, TIP, CARRY], [6, 4, 5, 0, CARRY, ROOT]] and slots == 1
    five = _nested((0, ((0, 0), (0, 0))))  # the larger subtree is on the right: walked first, handed on in registers
    ops, slots = post_order_slots(five)
    check_contract(five, ops, slots)
    assert slots == 1 and int(ops[-1, 4]) == CARRY and int(ops[-1, 3]) == TIP
    # a slot an op has read is the one it fills: ((c, c), (c, c)) under a root with a fifth subtree keeps to two slots
    eight = _nested((((0, 0), (0, 0)), ((0, 0), (0, 0))))
    ops, slots = post_order_slots(eight)
    check_contract(eight, ops, slots)
    assert slots == 2 and ops[2].tolist()[3:] == [0, CARRY, 0]


@pytest.mark.parametrize("T", [2, 3, 4, 5, 17, 64, 200, 300])
def test_a_caterpillar_parks_nothing(T):
    tree = synth.random_tree(T, np.random.default_rng(T), shape="caterpillar")
    for t in (tree, u.mirrored(tree)):
        ops, slots = post_order_slots(t)
        check_contract(t, ops, slots)
        assert slots == 0 and not (ops[:, 3:] >= 0).any()


def _perfect(k):
    return (_perfect(k - 1), _perfect(k - 1)) if k else 0


@pytest.mark.parametrize("k", range(1, 8))
def test_a_perfectly_balanced_tree_uses_k_minus_one_slots(k):
    tree = _nested(_perfect(k))
    assert tree.tip_count == 2 ** k
    ops, slots = post_order_slots(tree)
    check_contract(tree, ops, slots)
    assert slots == k - 1


def test_bad_arguments_are_refused():
    lib = _lib.load()
    tree = _nested(((0, 0), 0))
    left = np.ascontiguousarray(tree.left, dtype=np.int32)
    right = np.ascontiguousarray(tree.right, dtype=np.int32)
    out = np.zeros((2, 6), dtype=np.int32)
    fn = lib.phyamd_post_order_slots
    assert fn(1, left.ctypes.data, right.ctypes.data, 4, out.ctypes.data, 2, None) == _lib.EINVAL
    assert b"phyamd_post_order_slots: tip_count" in lib.phyamd_last_error()
    assert fn(3, None, right.ctypes.data, 4, out.ctypes.data, 2, None) == _lib.EINVAL
    assert fn(3, left.ctypes.data, right.ctypes.data, 4, None, 2, None) == _lib.EINVAL
    assert fn(3, left.ctypes.data, right.ctypes.data, 1, out.ctypes.data, 2, None) == _lib.EINVAL  # the root is a tip
    assert b"phyamd_post_order_slots" in lib.phyamd_last_error() and b"root" in lib.phyamd_last_error()
    assert fn(3, left.ctypes.data, right.ctypes.data, int(tree.root), None, 0, None) == 2  # counting alone
    assert fn(3, left.ctypes.data, right.ctypes.data, int(tree.root), out.ctypes.data, 1, None) == 2  # at most `capacity` are written
    assert out[1].tolist() == [0] * 6
