"""CPU-only: phyamd_branch_sweep_schedule -- one pass of phyamd_optimize_branch_lengths as the device runs it -- replayed
symbolically.  Every branch length has a version that its visit bumps; every plane holds the set of (node, version) pairs of the
lengths it was built from.  Starting from "every lower current, no O" and over two consecutive passes: every op's operands exist,
at every visit O_n and p_n were built from the current versions of exactly the lengths they depend on, and the visits are the
post-order.  A stale partial is how this feature goes wrong, and this finds it without a GPU."""

import numpy as np
import pytest

from physher_amd import _lib, synth
from test_tree_batch_gpu import _relabel

UPPER, LOWER, VISIT, ROOT = 0, 1, 2, -3


def schedule(left, right, root, T):
    lib = _lib.load()
    l, r = np.ascontiguousarray(left, dtype=np.int32), np.ascontiguousarray(right, dtype=np.int32)
    n = lib.phyamd_branch_sweep_schedule(T, l.ctypes.data, r.ctypes.data, int(root), None, 0)
    assert n == 5 * T - 6, lib.phyamd_last_error()
    out = np.full((n, 6), -99, dtype=np.int32)
    assert lib.phyamd_branch_sweep_schedule(T, l.ctypes.data, r.ctypes.data, int(root), out.ctypes.data, n) == n
    return out


def trees(T):
    rng = np.random.default_rng(100 + T)
    for shape in ("caterpillar", "balanced", "random"):
        t = synth.random_tree(T, rng, shape=shape)
        yield shape, (np.asarray(t.left), np.asarray(t.right), int(t.root))
    t = synth.random_tree(T, rng, shape="random")
    yield "relabelled", _relabel((t.left, t.right, int(t.root), t.length), rng, T)[0][:3]  # (internal ids permuted, the root not last)


def subtree(left, right, n, T):
    out, stack = [], [n]
    while stack:
        x = stack.pop()
        out.append(x)
        if x >= T:
            stack += [int(left[x]), int(right[x])]
    return out


@pytest.mark.parametrize("T", [2, 3, 4, 8, 37, 200])
def test_two_passes_never_read_a_stale_plane(T):
    for shape, (left, right, root) in trees(T):
        N = 2 * T - 1
        ops = schedule(left, right, root, T)
        parent = {int(c): n for n in range(T, N) for c in (left[n], right[n])}
        below = {n: frozenset(subtree(left, right, n, T)) for n in range(N)}
        version = np.zeros(N, dtype=np.int64)

        def current(nodes):
            return frozenset((n, int(version[n])) for n in nodes)
        # plane -> what it was built from.  Start: every lower current (p_n depends on the lengths strictly below n), no O
        plane = {N + (n - T): current(below[n] - {n}) for n in range(T, N)}

        def message(x):  # P_x p_x: x's own length and everything below it
            if x >= T:
                assert N + (x - T) in plane, (shape, "p of", x, "does not exist")
                return plane[N + (x - T)] | current([x])
            return current([x])
        post = []

        def post_order(n):
            if n >= T:
                post_order(int(left[n])), post_order(int(right[n]))
            if n != root:
                post.append(n)
        post_order(root)
        for _ in range(2):
            visited, last_visit = [], -1
            for visit, kind, node, a, b, written in ops.tolist():
                assert visit in (last_visit, last_visit + 1), (shape, "visit indices rise by one")
                if kind == UPPER:
                    assert parent[node] == (root if a == ROOT else a) and {node, b} == {int(left[parent[node]]), int(right[parent[node]])}
                    above = frozenset()
                    if a != ROOT:
                        assert a in plane, (shape, "O of", a, "does not exist")
                        above = plane[a] | current([a])
                    assert written == node
                    plane[node] = above | message(b)
                elif kind == LOWER:
                    assert node >= T and (a, b) == (left[node], right[node]) and written == N + (node - T)
                    plane[written] = message(a) | message(b)
                else:
                    assert kind == VISIT and written == -1 and a == node and b == (N + (node - T) if node >= T else -1)
                    assert visit == last_visit + 1
                    last_visit = visit
                    # O_n: every length outside n's subtree but the root's; p_n: every length strictly below n -- all current
                    outside = frozenset(range(N)) - below[node] - {root}
                    assert plane.get(a) == current(outside), (shape, "O of", node, "is stale or wrong")
                    if node >= T:
                        assert plane[b] == current(below[node] - {node}), (shape, "p of", node, "is stale or wrong")
                    version[node] += 1  # the visit moves t_node
                    visited.append(node)
            assert visited == post, (shape, "the visits are not the post-order")


def test_arguments_are_checked():
    lib = _lib.load()
    left, right = np.array([-1, -1, 0], dtype=np.int32), np.array([-1, -1, 1], dtype=np.int32)
    out = np.zeros((4, 6), dtype=np.int32)
    assert lib.phyamd_branch_sweep_schedule(1, left.ctypes.data, right.ctypes.data, 2, out.ctypes.data, 4) == _lib.EINVAL
    assert lib.phyamd_branch_sweep_schedule(2, None, right.ctypes.data, 2, out.ctypes.data, 4) == _lib.EINVAL
    assert lib.phyamd_branch_sweep_schedule(2, left.ctypes.data, right.ctypes.data, 2, None, 4) == _lib.EINVAL
    assert lib.phyamd_branch_sweep_schedule(2, left.ctypes.data, right.ctypes.data, 0, out.ctypes.data, 4) == _lib.EINVAL  # a tip as the root
    assert b"phyamd_branch_sweep_schedule" in lib.phyamd_last_error()
    assert lib.phyamd_branch_sweep_schedule(2, left.ctypes.data, right.ctypes.data, 2, out.ctypes.data, 4) == 4
    assert out.tolist() == [[0, 0, 0, -3, 1, 0], [0, 2, 0, 0, -1, -1], [1, 0, 1, -3, 0, 1], [1, 2, 1, 1, -1, -1]]
