"""The elided nodes whose own pre-order op takes its stored child's plane from its parent's op in registers (phyamd_stream_keeps),
the rule that chooses them written out again over the older schedule exports, and the trees on which the CPU and GPU tests run.

The rule (stream_keep, phyamd_tree_schedule.h), over the streamed list (phyamd_pre_order_schedule, form 1) and the elided nodes
(phyamd_stream_elisions).  The op of an elided node n's parent is handed the plane of n's stored child s on the side n has there.
It does not request that plane for the next op, and the next op reads it from the registers it is still in, where
  * n's own op does not open a chunk (a chunk's prologue fetches the operands of its first op),
  * n's own op is the next op of its parent's chunk (not so where n's upper is parked, or the other child's op comes first),
  * s sits in n's op on the side n has in its parent's op (register set A serves left children, B right ones).
Every other elided node keeps the request, and so does every one with the switch off."""
import collections
import functools
import hashlib

import numpy as np

import stream_elide_util as se
import stream_pairs_util as sp
import upper_park_util as u
from physher_amd import _lib

# columns of a phyamd_stream_keeps record
NODE, PARENT, SIDE, REASON, REQUEST_TF, REQUEST_PLAIN = range(6)
COLUMNS = 6
KEPT, NOT_NEXT, OTHER_SIDE, OPENER, OFF = range(5)

BENCH_KEPT = 44  # the bench tree, synth.random_tree(1000, default_rng(1)): of its 76 elided nodes (stream_elide_util.BENCH_ELIDED)

# sha256 over the records of phyamd_stream_elisions and of phyamd_stream_pairs (pairs = 1, then 0) of every tree of ALL, in that
# order, recorded from the library before stream_keep existed (older_export_digests prints them again)
ELISIONS_DIGEST = "63d9b5382712aba34cc3f909918506a490bba27782125fcf0995f52e82e1ef58"
PAIRS_DIGEST = "39b4dfe3deabb507bfced2c2a461fb46ca450162a40f0b48e8fb3f549080e139"

ALL = tuple(dict.fromkeys(se.ALL + sp.ALL))


def make_tree(name, bl=(0.01, 0.1), mirror=False):
    if name in se.ALL or name == "bench":
        return se.make_tree(name, bl, mirror)
    return u.mirrored(sp.make_tree(name, bl)) if mirror else sp.make_tree(name, bl)


def stream_keeps(tree, keep=1):
    lib = _lib.load()
    T = tree.tip_count
    left = np.ascontiguousarray(tree.left, dtype=np.int32)
    right = np.ascontiguousarray(tree.right, dtype=np.int32)
    out = np.full((T, COLUMNS), -7, dtype=np.int32)
    n = lib.phyamd_stream_keeps(T, left.ctypes.data, right.ctypes.data, int(tree.root), keep, out.ctypes.data, T)
    assert n >= 0, lib.phyamd_last_error()
    assert n <= T
    return out[:n]


def expected(tree):
    """the rule over phyamd_pre_order_schedule (form 1) and phyamd_stream_elisions: [(node, parent, side, reason)] in the elisions'
    order, and for every elided node where its own op takes its upper from (upper_park_util's source codes)"""
    pre, _ = u.pre_order_schedule(tree, 1)
    at = {int(op[u.NODE]): i for i, op in enumerate(pre)}
    openers = {b for b, _ in u.chunk_bounds(pre)}
    want, source = [], {}
    for r in se.stream_elisions(tree):
        n, p, s, side = int(r[se.NODE]), int(r[se.PARENT]), int(r[se.STORED]), int(r[se.SIDE])
        i, j = at[p], at[n]
        assert int(pre[i, u.RIGHT if side else u.LEFT]) == n
        if j in openers:
            reason = OPENER
        elif j != i + 1 or pre[j, u.CHUNK] != pre[i, u.CHUNK]:
            reason = NOT_NEXT
        elif int(pre[j, u.RIGHT if side else u.LEFT]) != s:
            reason = OTHER_SIDE
        else:
            reason = KEPT
        want.append((n, p, side, reason))
        source[n] = int(pre[j, u.SRC])
    return want, source


def check_rule(tree):
    """the export against the rule, node by node, with the switch on and off; returns what the tree reaches of the cases the tests need"""
    rec, off = stream_keeps(tree, 1), stream_keeps(tree, 0)
    assert (rec != -7).all() and (off != -7).all(), "a column was not written"
    want, source = expected(tree)
    el = se.stream_elisions(tree)
    assert len(rec) == len(off) == len(el) == len(want), "one record per elided node"
    assert [tuple(int(x) for x in r[[NODE, PARENT, SIDE, REASON]]) for r in rec] == want, "the export differs from the rule"
    # the switch off: nothing is kept, and the requests differ from the switch on at the kept nodes alone, in both descriptor sets
    assert (off[:, [NODE, PARENT, SIDE]] == rec[:, [NODE, PARENT, SIDE]]).all() and (off[:, REASON] == OFF).all()
    kept = rec[:, REASON] == KEPT
    for col in (REQUEST_TF, REQUEST_PLAIN):
        assert (rec[kept, col] == 0).all() and (off[kept, col] == 1).all(), "a kept operand is requested, or was never requested"
        assert (rec[~kept, col] == off[~kept, col]).all(), "a request moved at a node that is not kept"
    pre, _ = u.pre_order_schedule(tree, 1)
    at = {int(op[u.NODE]): i for i, op in enumerate(pre)}
    openers = {b for b, _ in u.chunk_bounds(pre)}
    kind_of = {int(r[se.NODE]): int(r[se.SIBLING_KIND]) for r in el}
    kept_nodes = {int(r[NODE]) for r in rec[kept]}
    stored_of = {int(r[se.NODE]): int(r[se.STORED]) for r in el}
    # chains: a kept node whose stored child's stored child is elided and kept again (alternate rungs of a ladder of shaped nodes)
    parent_of = {int(r[se.NODE]): int(r[se.PARENT]) for r in el}
    elided_over = {s: n for n, s in stored_of.items()}  # stored child -> the elided node above it
    longest = 0
    for n in kept_nodes:
        run, v = 1, n
        while elided_over.get(parent_of[v]) in kept_nodes:  # v's parent is the stored child of a kept node
            v = elided_over[parent_of[v]]
            run += 1
        longest = max(longest, run)
    not_next = [int(r[NODE]) for r in rec if r[REASON] == NOT_NEXT]
    return dict(count=len(rec),
                kept=int(kept.sum()),
                reasons=dict(collections.Counter(int(x) for x in rec[:, REASON])),
                kept_kind_sides={(kind_of[int(r[NODE])], int(r[SIDE])) for r in rec[kept]},
                parked=sum(1 for n in not_next if source[n] in (u.LDS0, u.LDS1, u.HBM)),
                parked_sources={source[n] for n in not_next if source[n] in (u.LDS0, u.LDS1, u.HBM)},
                opener=int((rec[:, REASON] == OPENER).sum()),
                other_side=int((rec[:, REASON] == OTHER_SIDE).sum()),
                kept_behind_prologue=sum(1 for r in rec[kept] if at[int(r[PARENT])] in openers),
                unkept_behind_prologue_sides={int(r[SIDE]) for r in rec[~kept] if at[int(r[PARENT])] in openers},
                chain=longest)


@functools.lru_cache(maxsize=None)
def reach(name, mirror=False):
    return check_rule(make_tree(name, mirror=mirror))


def _sha(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, dtype=np.int32).tobytes())
    return h.hexdigest()


def older_export_digests():
    """(phyamd_stream_elisions, phyamd_stream_pairs) over ALL: these exports build their tables without stream_keep"""
    trees = [make_tree(name) for name in ALL]
    return _sha([se.stream_elisions(t) for t in trees]), _sha([sp.stream_pairs(t, pairs) for t in trees for pairs in (1, 0)])


# the cases and the tree that is in the GPU test for each (test_stream_keep_schedule.py asserts that it reaches it)
CASES = {
    "an operand kept beside a tip and beside a cherry": ("random200", lambda r: {k for k, _ in r["kept_kind_sides"]} == {u.TIP, u.CHERRY}),
    "an elided node that is not kept because its upper is parked": ("random200", lambda r: r["parked"] > 0),
    "an elided node that is not kept because its own op opens a chunk": ("target", lambda r: r["opener"] > 0),
    "an operand the chunk's prologue fetched, kept by the op that opens the chunk": ("target", lambda r: r["kept_behind_prologue"] > 0),
    "an elided right child of an op that opens a chunk, not kept": ("prologue_right", lambda r: 1 in r["unkept_behind_prologue_sides"] and r["kept"] > 0),
    "a chain of shaped nodes, alternate ones elided and every one of those kept": ("caterpillar64", lambda r: r["chain"] >= 3 and r["kept"] == r["count"]),
    "a ladder that is rescaled several times, operands kept beside both kinds": ("ladder160", lambda r: {k for k, _ in r["kept_kind_sides"]} == {u.TIP, u.CHERRY}),
}
GPU_TREES = tuple(sorted({name for name, _ in CASES.values()}))
