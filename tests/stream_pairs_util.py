"""The pair ops of the streamed pre-order walk (phyamd_stream_pairs), the rule that chooses them written out again over the older
schedule exports, and the trees on which the CPU and GPU tests of the pairs run.

The rule (stream_pairs, phyamd_tree_schedule.h), over the streamed list (phyamd_pre_order_schedule, form 1) with the child kinds
of phyamd_stream_elisions: the op of node n and the op of its DEEP child d become one when
  * d is n's left child (the one walked first), d's op is the next one of the same chunk and takes its upper in registers;
  * n's other child s is stored (CORE) or a tip in the descriptor: no fringe child, no second DEEP child, no elided node;
  * s is stored, or d has four tips (the block's other side holds s's 320 bytes and 160 per tip of d).
Where s is stored and its own op is the one behind d's, that op takes s's upper in registers and n neither parks nor stores it."""
import functools

import numpy as np

import stream_elide_util as se
import upper_park_util as u
from physher_amd import _lib, synth

COLUMNS = 48
(CHUNK, NODE, REASON, CHILD, SIBLING, SIBLING_KIND, CHILD_TIPS, CARRY, SRC, DST_RIGHT, PREFETCH, NEXT, BOTH_PIECES, DIGEST, PAIR_DIGEST) = range(15)
TAB_NODE, TAB_POS = 16, 32
FUSED, NO_DEEP, NOT_NEXT, BAD_SIBLING, NO_ROOM, ABSORBED = range(6)
SK_CORE_TIP, SK_CORE_CHERRY = 5, 6
HALF_TIPS = {u.TIP: 1, u.CHERRY: 2, u.CHERRY_TIP: 3}

BENCH_PAIRS = 55  # the bench tree, synth.random_tree(1000, default_rng(1)): of its 141 DEEP ops; 22 beside a stored node, 33 beside a tip


def stream_pairs(tree, pairs=1):
    lib = _lib.load()
    T = tree.tip_count
    left = np.ascontiguousarray(tree.left, dtype=np.int32)
    right = np.ascontiguousarray(tree.right, dtype=np.int32)
    out = np.full((T, COLUMNS), -7, dtype=np.int32)
    n = lib.phyamd_stream_pairs(T, left.ctypes.data, right.ctypes.data, int(tree.root), pairs, out.ctypes.data, T)
    assert n >= 0, lib.phyamd_last_error()
    assert n <= T
    return out[:n]


def expected(tree):
    """the rule over phyamd_pre_order_schedule (form 1) and phyamd_stream_elisions: per op (reason, child, sibling, sibling kind,
    child tips, carry)"""
    pre, _ = u.pre_order_schedule(tree, 1)
    elided = {(int(r[se.PARENT]), int(r[se.NODE])): SK_CORE_TIP if r[se.SIBLING_KIND] == u.TIP else SK_CORE_CHERRY for r in se.stream_elisions(tree)}
    out = []
    for i, op in enumerate(pre):
        n = int(op[u.NODE])
        if out and out[-1][0] == FUSED:
            out.append((ABSORBED, -1, -1, -1, 0, 0))
            continue
        kinds = [elided.get((n, int(op[u.LEFT])), int(op[u.KIND_LEFT])), elided.get((n, int(op[u.RIGHT])), int(op[u.KIND_RIGHT]))]
        if u.DEEP not in kinds:
            out.append((NO_DEEP, -1, -1, -1, 0, 0))
            continue
        here = i + 1 < len(pre) and pre[i + 1, u.CHUNK] == op[u.CHUNK]
        # (two DEEP children: the one whose op is next)
        side = 0 if kinds[0] == u.DEEP and not (kinds[1] == u.DEEP and here and pre[i + 1, u.NODE] == op[u.RIGHT]) else 1
        child, sibling = (int(op[u.LEFT]), int(op[u.RIGHT])) if side == 0 else (int(op[u.RIGHT]), int(op[u.LEFT]))
        halves = op[[u.HALF_L0, u.HALF_L1]] if side == 0 else op[[u.HALF_R0, u.HALF_R1]]
        tips = sum(HALF_TIPS[int(h)] for h in halves)
        sk = kinds[1 - side]
        if side != 0 or not here or pre[i + 1, u.NODE] != child or pre[i + 1, u.SRC] != u.CARRY:
            reason = NOT_NEXT
        elif sk not in (u.CORE, u.TIP):
            reason = BAD_SIBLING
        elif sk == u.TIP and tips > 4:
            reason = NO_ROOM
        else:
            reason = FUSED
        carry = int(reason == FUSED and sk == u.CORE and i + 2 < len(pre) and pre[i + 2, u.CHUNK] == op[u.CHUNK] and pre[i + 2, u.NODE] == sibling)
        out.append((reason, child, sibling, sk, tips, carry))
    return pre, out


def check_rule(tree):
    """the export against the rule, op by op, and what a pair must leave of the walk; returns what the tree reaches"""
    rec, off = stream_pairs(tree, 1), stream_pairs(tree, 0)
    assert (rec != -7).all() and (off != -7).all(), "a column was not written"
    pre, want = expected(tree)
    assert len(rec) == len(off) == len(pre)
    assert (rec[:, [CHUNK, NODE]] == pre[:, [u.CHUNK, u.NODE]]).all()
    # switch off: nothing but the walk itself, and the tables every other pass reads are the same bytes
    assert (off[:, [CHUNK, NODE, DIGEST]] == rec[:, [CHUNK, NODE, DIGEST]]).all(), "the unfused tables differ with the switch on"
    assert (np.delete(off, [CHUNK, NODE, DIGEST], axis=1) == -1).all()
    got = [tuple(int(x) for x in r[[REASON, CHILD, SIBLING, SIBLING_KIND, CHILD_TIPS, CARRY]]) for r in rec]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"op {i} (node {int(rec[i, NODE])}): export {g}, rule {w}"
    # slab positions: the walk order of the branch terms of the two-op form
    pos, at = {}, 0
    for op in pre:
        for q in op[u.Q0:u.Q0 + op[u.QCOUNT]]:
            assert int(q) not in pos
            pos[int(q)] = at
            at += 1
    assert len(pos) == 2 * tree.tip_count - 2, "the two-op form does not produce every branch once"
    bounds = u.chunk_bounds(pre)
    last_of_chunk = {e - 1 for _, e in bounds}
    cut_roots = {ch for op in pre for side, ch, _, _, _ in u.children(op) if op[u.CUT] & (1 << side)}
    produced = []
    stats = dict(count=0, core=0, tip=0, carry=0, carry_from={}, parent_src=set(), root_parent=0, beside_cut=0, reasons={},
                 half_kinds=set(), tip_sibling_tips=set(), core_sibling_tips=set())
    for i, r in enumerate(rec):
        op = pre[i]
        stats["reasons"][int(r[REASON])] = stats["reasons"].get(int(r[REASON]), 0) + 1
        if r[REASON] == ABSORBED:
            assert rec[i - 1, REASON] == FUSED and rec[i - 1, CHILD] == r[NODE]
            continue
        nxt = i + 2 if r[REASON] == FUSED else i + 1
        assert r[NEXT] == (nxt if nxt - 1 not in last_of_chunk and i not in last_of_chunk else -1)
        if r[NEXT] >= 0 and rec[r[NEXT], REASON] == FUSED:
            assert r[BOTH_PIECES] == 1, f"op {i}: the pair behind it needs both pieces of its block"
        if r[SRC] != op[u.SRC]:  # only the op behind a pair that hands its stored sibling on: a carry and no slot
            assert i >= 2 and rec[i - 2, REASON] == FUSED and rec[i - 2, CARRY] == 1 and r[SRC] == u.CARRY and op[u.SRC] in (u.LDS0, u.LDS1, u.HBM)
            stats["carry_from"][int(op[u.SRC])] = stats["carry_from"].get(int(op[u.SRC]), 0) + 1
        else:
            assert not (i >= 2 and rec[i - 2, REASON] == FUSED and rec[i - 2, CARRY] == 1)
        if r[REASON] != FUSED:
            assert (r[TAB_NODE:] == -1).all()
            produced += [int(q) for q in op[u.Q0:u.Q0 + op[u.QCOUNT]]]
            continue
        d = pre[i + 1]
        assert i not in last_of_chunk and d[u.CHUNK] == op[u.CHUNK], "a pair across a chunk boundary"
        assert op[u.LEFT] == r[CHILD] == d[u.NODE] and op[u.KIND_LEFT] == u.DEEP and d[u.SRC] == u.CARRY and op[u.DST_LEFT] == u.CARRY
        assert r[CHILD] not in cut_roots
        assert op[u.RIGHT] == r[SIBLING] and op[u.KIND_RIGHT] == r[SIBLING_KIND] and r[SIBLING_KIND] in (u.TIP, u.CORE)
        assert r[SIBLING_KIND] == u.CORE or r[CHILD_TIPS] == 4
        # every term of both ops once, at its own slab position
        nodes, places = r[TAB_NODE:TAB_NODE + 16], r[TAB_POS:TAB_POS + 16]
        terms = [int(q) for q in op[u.Q0:u.Q0 + op[u.QCOUNT]]] + [int(q) for q in d[u.Q0:u.Q0 + d[u.QCOUNT]]]
        assert sorted(int(x) for x in nodes[nodes >= 0]) == sorted(terms) and len(terms) <= 12 and (nodes[12:] == -1).all()
        assert all(places[j] == pos[int(nodes[j])] for j in range(16) if nodes[j] >= 0)
        assert nodes[0] == r[CHILD] and nodes[4] == r[SIBLING]
        produced += terms
        if r[CARRY]:
            assert rec[i + 2, NODE] == r[SIBLING] and rec[i + 2, SRC] == u.CARRY and r[DST_RIGHT] == 0 and r[PREFETCH] == -1
            assert r[SIBLING] not in cut_roots
        else:
            assert r[DST_RIGHT] == (0 if op[u.DST_RIGHT] in (u.NONE, u.CARRY) else op[u.DST_RIGHT])
            assert r[PREFETCH] == d[u.PREFETCH]
        stats["count"] += 1
        stats["core" if r[SIBLING_KIND] == u.CORE else "tip"] += 1
        stats["carry"] += int(r[CARRY])
        stats["parent_src"].add(int(op[u.SRC]))
        stats["root_parent"] += int(op[u.SRC] == u.ROOT)
        stats["beside_cut"] += int(r[SIBLING] in cut_roots)
        stats["half_kinds"].add((int(op[u.HALF_L0]), int(op[u.HALF_L1])))
        stats["tip_sibling_tips" if r[SIBLING_KIND] == u.TIP else "core_sibling_tips"].add(int(r[CHILD_TIPS]))
    assert sorted(produced) == sorted(pos), "a branch term is produced twice or not at all"
    return stats


# ---- trees -----------------------------------------------------------------------------------------------------------------

def _spine(rungs):
    s = rungs[0]
    for i, r in enumerate(rungs[1:]):
        s = (s, r) if i % 2 else (r, s)
    return s


def pairs_gallery():
    """a spine whose rungs put a DEEP child of every pair of half kinds beside a tip and beside a stored node, and one beside a
    cherry, a cherry + tip and a second DEEP child"""
    core = (u.deep_shape(u.CHERRY, u.CHERRY), 0)
    rungs = []
    for a, b in u.DEEP_PAIRS:
        deep = u.deep_shape(a, b)
        rungs += [(deep, 0), (core, deep)]
    deep = u.deep_shape(u.CHERRY, u.CHERRY)
    rungs += [(deep, (0, 0)), (deep, ((0, 0), 0)), (deep, u.deep_shape(u.CHERRY_TIP, u.CHERRY))]
    return _spine(rungs)


# "root_pair": the root's children are a DEEP node and a stored one -- the root's op is a pair and hands the stored child on
_CORE = (u.deep_shape(u.CHERRY, u.CHERRY), 0)
ROOT_PAIR_SHAPE = (u.deep_shape(u.CHERRY_TIP, u.CHERRY), (_CORE, _CORE))
EXTRA = ("pairs_gallery", "root_pair")


@functools.lru_cache(maxsize=None)
def _make(name, bl):
    if name in se.ALL:
        return se.make_tree(name, bl)
    if name == "pairs_gallery":
        return u.from_nested(pairs_gallery(), 41, bl)
    if name == "root_pair":
        return u.from_nested(ROOT_PAIR_SHAPE, 42, bl)
    if name == "bench":
        return synth.random_tree(1000, np.random.default_rng(1))
    raise ValueError(name)


def make_tree(name, bl=(0.01, 0.1)):
    return _make(name, tuple(bl))


ALL = se.ALL + EXTRA


@functools.lru_cache(maxsize=None)
def reach(name):
    return check_rule(make_tree(name))


# the cases and the tree that is in the GPU test for each (test_stream_pairs_schedule.py asserts that it reaches it)
CASES = {
    "a pair with a stored sibling and one with a tip sibling": ("pairs_gallery", lambda r: r["core"] > 0 and r["tip"] > 0),
    "every pair of half kinds in a pair; five and six tips beside a stored sibling": (
        "pairs_gallery", lambda r: r["half_kinds"] == set(u.DEEP_PAIRS) and {5, 6} <= r["core_sibling_tips"] and r["tip_sibling_tips"] == {4}),
    "refusals: a fringe sibling, a second DEEP child, a tip beside five or six tips": (
        "pairs_gallery", lambda r: r["reasons"].get(BAD_SIBLING, 0) > 0 and r["reasons"].get(NO_ROOM, 0) > 0),
    "the stored sibling's op takes its upper in registers": ("pairs_gallery", lambda r: r["carry"] > 0),
    "a parent whose upper arrives in registers, from each LDS slot and from HBM": (
        "random200", lambda r: {u.CARRY, u.LDS0, u.LDS1, u.HBM} <= r["parent_src"]),
    "a stored sibling that had waited in an LDS slot": ("random200", lambda r: r["carry_from"].get(u.LDS0, 0) > 0),
    "the root as the parent of a pair": ("root_pair", lambda r: r["root_parent"] == 1),
    "a tree without a pair (its DEEP nodes all sit beside a fringe or a second DEEP child)": ("balanced64", lambda r: r["count"] == 0),
    "pairs in a tree whose walk is cut into chunks": ("target", lambda r: True),
}
GPU_TREES = tuple(sorted({name for name, _ in CASES.values()}))
