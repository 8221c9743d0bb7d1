"""Trees whose post-order walk nests its waits two deep and deeper, and the host schedule's account of them
(phyamd_post_order_parks), shared by the CPU and GPU tests of the post-order walk's second park slot."""
import functools

import numpy as np

from physher_amd import _lib, synth

# columns of a phyamd_post_order_parks record
CHUNK, NODE, LEFT, RIGHT, SRC_LEFT, SRC_RIGHT, PARK, CUT = range(8)
MEMORY, CARRIED, SLOT0, SLOT1 = 0, 1, 2, 3


def _join(groups, left, right):
    """balanced joins of a list of node ids, appended to left / right; returns the subtree's root"""
    while len(groups) > 1:
        nxt = []
        for i in range(0, len(groups) - 1, 2):
            left.append(groups[i])
            right.append(groups[i + 1])
            nxt.append(len(left) - 1)
        if len(groups) % 2:
            nxt.append(groups[-1])
        groups = nxt
    return groups[0]


def _tree(left, right, seed, bl):
    rng = np.random.default_rng(seed)
    N = len(left)
    length = rng.uniform(bl[0], bl[1], size=N)
    length[N - 1] = 0.0
    T = (N + 1) // 2
    return synth.SynthTree(np.array(left, dtype=np.int32), np.array(right, dtype=np.int32), length, [f"t{i}" for i in range(T)])


def balanced_tree(T, seed, bl):
    left, right = [-1] * T, [-1] * T
    _join(list(range(T)), left, right)
    return _tree(left, right, seed, bl)


def caterpillar_of_subtrees(sizes, seed, bl):
    """a ladder whose rungs are balanced subtrees of `sizes` tips: 8 tips are one stored node, 16 tips nest one wait, 32 tips two"""
    T = sum(sizes)
    left, right = [-1] * T, [-1] * T
    roots, t0 = [], 0
    for s in sizes:
        roots.append(_join(list(range(t0, t0 + s)), left, right))
        t0 += s
    spine = roots[0]
    for r in roots[1:]:
        left.append(spine)
        right.append(r)
        spine = len(left) - 1
    return _tree(left, right, seed, bl)


CATERPILLAR_SIZES = (16, 16, 32, 16, 32, 16, 16, 8)
TREES = ("caterpillar", "balanced64", "random200")


def make_tree(name, bl=(0.01, 0.1)):
    if name == "caterpillar":
        return caterpillar_of_subtrees(CATERPILLAR_SIZES, 11, bl)
    if name == "balanced64":
        return balanced_tree(64, 12, bl)
    if name == "random200":
        return synth.random_tree(200, np.random.default_rng(3), bl_low=bl[0], bl_high=bl[1])
    raise ValueError(name)


def post_order_parks(tree, second_slot=True):
    lib = _lib.load()
    T = tree.tip_count
    left = np.ascontiguousarray(tree.left, dtype=np.int32)
    right = np.ascontiguousarray(tree.right, dtype=np.int32)
    out = np.zeros((T, 8), dtype=np.int32)
    n = lib.phyamd_post_order_parks(T, left.ctypes.data, right.ctypes.data, int(tree.root), int(second_slot), out.ctypes.data, T)
    assert n >= 0, lib.phyamd_last_error()
    assert n <= T
    return out[:n]


@functools.lru_cache(maxsize=None)
def sources(name):
    """(slot-1 reads, memory reads) of the named tree's two-slot schedule"""
    ops = post_order_parks(make_tree(name))
    src = ops[:, [SRC_LEFT, SRC_RIGHT]]
    return int((src == SLOT1).sum()), int((src == MEMORY).sum())
