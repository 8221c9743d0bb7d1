"""The stored nodes the streamed 4-state walks do not store (phyamd_stream_elisions), the rule that chooses them written out again
over the two older schedule exports, and the trees on which the CPU and GPU tests of the elision run.

The rule (stream_elide, phyamd_tree_schedule.h), bottom-up over the chunked post-order list: a node n is elided if
  * n is stored (CORE) and not the root;
  * one child s is stored and not elided itself, the other child f is a tip or a cherry;
  * the post-order walk hands n to its parent in registers inside one chunk: as the result of the op in front (source 1) or from
    park slot 0 (source 2) -- not from memory (source 0: next to a cut), not from the second slot (source 3)."""
import functools

import numpy as np

import lower_park_util as lp
import upper_park_util as u
from physher_amd import _lib, synth

# columns of a phyamd_stream_elisions record
NODE, PARENT, STORED, SIBLING, SIBLING_KIND, SOURCE, SIDE, CHUNK = range(8)

BENCH_ELIDED = 76  # the bench tree, synth.random_tree(1000, default_rng(1)): 77 by the shape rule alone, one lost to the reach rule
CFG2_ELIDED = 31   # synth.random_tree(500, default_rng(1)), of 173 stored nodes
# sha256 over the records of phyamd_pre_order_schedule (forms 0, 1, 2, each followed by its slot count) and phyamd_post_order_parks
# (two slots, one slot) of upper_park_util.NAMED, recorded from the library before stream_elide existed
PRE_ORDER_DIGEST = "eb4a118d9b596b8d8f5ae8510e016bd784bd33430f2da7a4b74eedb372f006e0"
POST_ORDER_DIGEST = "5c828fde6b7f751884059f41870e1fe19df4f55095f01aa86cc26edee7bf7377"
# ... and per tree (pre-order records, post-order records; the first 16 hex digits), so that a change can be located.  To record them
# again: run test_older_exports_are_unchanged with -s on a checkout of the commit to compare against; it prints this table
EXPORT_DIGESTS = {
    "caterpillar": ("6b3d9b8ee622f228", "8002edc2036d7c86"),
    "balanced64": ("5faae3ecb14ab344", "0a91735f807b8663"),
    "random200": ("3efdee63757b8327", "fbd38ea9e7ac73e7"),
    "gallery": ("70889d359f5342ca", "e4503fb18f03c5c6"),
    "ops31": ("08ea06ab818e6c5a", "3cd2b4de08551586"),
    "ops32": ("986edebc74ed2036", "2787d9ae460173b4"),
    "ops33": ("4faedce562cdc134", "239bbdb165ac1aba"),
    "target": ("a0f39defd1fcad6e", "25c8808109473ad8"),
    "random97": ("bb3765d23cbc8109", "f615ce9ef38619e0"),
    "random150m": ("6a126b4ce2792b35", "e2eb7ae2a58c7ce5"),
    "balanced40m": ("e227d3f2f99c882f", "0fef987f6f412b94"),
    "reuse56m": ("d1b481cabd0460ca", "5a02a29d9fe005ac"),
}


def stream_elisions(tree):
    lib = _lib.load()
    T = tree.tip_count
    left = np.ascontiguousarray(tree.left, dtype=np.int32)
    right = np.ascontiguousarray(tree.right, dtype=np.int32)
    out = np.full((T, 8), -7, dtype=np.int32)
    n = lib.phyamd_stream_elisions(T, left.ctypes.data, right.ctypes.data, int(tree.root), out.ctypes.data, T)
    assert n >= 0, lib.phyamd_last_error()
    assert n <= T
    return out[:n]


def node_kinds(tree):
    """build_schedule's classification from the tree alone (as upper_park_util.check_contract derives it)"""
    T, N = tree.tip_count, 2 * tree.tip_count - 1
    left, right = np.asarray(tree.left), np.asarray(tree.right)
    kind = [u.TIP] * T + [u.CORE] * (N - T)
    order, stack = [], [int(tree.root)]
    while stack:
        v = stack.pop()
        order.append(v)
        if v >= T:
            stack += [int(left[v]), int(right[v])]
    for v in reversed(order):
        if v < T or v == tree.root:
            continue
        l, r = int(left[v]), int(right[v])
        if l < T and r < T:
            kind[v] = u.CHERRY
        elif (l < T and kind[r] == u.CHERRY) or (r < T and kind[l] == u.CHERRY):
            kind[v] = u.CHERRY_TIP
        elif kind[l] not in (u.CORE, u.DEEP) and kind[r] not in (u.CORE, u.DEEP):
            kind[v] = u.DEEP
    return kind


def expected(tree):
    """The rule over phyamd_post_order_parks and the tree.  Returns (elided: node -> (parent, stored child, sibling, sibling kind,
    source, post-order chunk), shaped: node -> (stored child, source) for every node with the rule's shape -- stored, not the root,
    one stored child and one tip or cherry child -- whatever its source and whether or not its stored child was elided)"""
    kind = node_kinds(tree)
    parks = lp.post_order_parks(tree, True)
    row_of = {int(r[lp.NODE]): r for r in parks}
    parent = {}
    for r in parks:
        parent[int(r[lp.LEFT])] = int(r[lp.NODE])
        parent[int(r[lp.RIGHT])] = int(r[lp.NODE])
    elided, shaped = {}, {}
    for r in parks:  # launch order: the cut subtrees' chunks, then the top part -- children before parents
        n, l, rr = int(r[lp.NODE]), int(r[lp.LEFT]), int(r[lp.RIGHT])
        assert kind[n] == u.CORE
        if n == tree.root:
            continue
        if kind[l] == u.CORE and kind[rr] in (u.TIP, u.CHERRY):
            s, f = l, rr
        elif kind[rr] == u.CORE and kind[l] in (u.TIP, u.CHERRY):
            s, f = rr, l
        else:
            continue
        p = row_of[parent[n]]
        source = int(p[lp.SRC_LEFT] if p[lp.LEFT] == n else p[lp.SRC_RIGHT])
        shaped[n] = (s, source)
        if s in elided or source not in (lp.CARRIED, lp.SLOT0):
            continue
        assert p[lp.CHUNK] == r[lp.CHUNK], "a child handed on in registers sits in its parent's chunk"
        elided[n] = (int(p[lp.NODE]), s, f, kind[f], source, int(r[lp.CHUNK]))
    return elided, shaped


def check_rule(tree):
    """the export against the rule, node by node; returns what the tree reaches of the six cases the tests need"""
    rec = stream_elisions(tree)
    assert (rec != -7).all(), "a column was not written"
    want, shaped = expected(tree)
    got = {int(r[NODE]): tuple(int(x) for x in r[[PARENT, STORED, SIBLING, SIBLING_KIND, SOURCE, CHUNK]]) for r in rec}
    assert len(got) == len(rec), "a node is listed twice"
    assert got == want, f"elided nodes differ from the rule: {sorted(set(got) ^ set(want))[:10]}"
    parks = lp.post_order_parks(tree, True)
    chunk_of = {int(r[lp.NODE]): int(r[lp.CHUNK]) for r in parks}
    last_of_chunk = {int(parks[i, lp.NODE]) for i in range(len(parks)) if i + 1 == len(parks) or parks[i + 1, lp.CHUNK] != parks[i, lp.CHUNK]}
    pre, _ = u.pre_order_schedule(tree, 1)
    side_of = {}
    for op in pre:
        side_of[int(op[u.LEFT])] = 0
        side_of[int(op[u.RIGHT])] = 1
    pre_cut_roots = {ch for op in pre for side, ch, _, _, _ in u.children(op) if op[u.CUT] & (1 << side)}
    chunk_openers = {int(pre[b, u.NODE]) for b, _ in u.chunk_bounds(pre)}  # their operands are requested by the chunk's prologue
    kind = node_kinds(tree)
    for r in rec:
        n = int(r[NODE])
        assert n != tree.root and kind[n] == u.CORE
        assert kind[int(r[STORED])] == u.CORE and int(r[STORED]) not in got, f"node {n}: its stored child is elided too"
        assert r[SIBLING_KIND] in (u.TIP, u.CHERRY) and kind[int(r[SIBLING])] == r[SIBLING_KIND]
        assert r[SOURCE] in (lp.CARRIED, lp.SLOT0)
        assert chunk_of[n] == chunk_of[int(r[PARENT])] == r[CHUNK] and n not in last_of_chunk
        assert r[SIDE] == side_of[n], f"node {n}: side {r[SIDE]}, its parent's streamed op has it on side {side_of[n]}"
    # chains of shaped nodes, each the stored child of the next
    longest = 0
    for n in shaped:
        run = [n]
        while shaped[run[-1]][0] in shaped:
            run.append(shaped[run[-1]][0])
        if all(src in (lp.CARRIED, lp.SLOT0) for src in (shaped[v][1] for v in run)):
            # bottom-up and greedy: the lowest is elided, then every other one
            assert [v in got for v in reversed(run)] == [i % 2 == 0 for i in range(len(run))], f"chain {run}"
            longest = max(longest, len(run))
    return dict(count=len(rec),
                kind_sides={(int(r[SIBLING_KIND]), int(r[SIDE])) for r in rec},
                slot0=sum(1 for r in rec if r[SOURCE] == lp.SLOT0),
                chain=longest,
                refused_memory=sum(1 for n, (s, src) in shaped.items() if src == lp.MEMORY and s not in got),
                refused_slot1=sum(1 for n, (s, src) in shaped.items() if src == lp.SLOT1 and s not in got),
                pre_cut_roots=sum(1 for n in got if n in pre_cut_roots),
                prologue_sides={int(r[SIDE]) for r in rec if int(r[PARENT]) in chunk_openers},
                shaped=len(shaped))


# ---- trees -----------------------------------------------------------------------------------------------------------------

EXTRA = ("caterpillar64", "slot1", "ladder160", "prologue_right")


def _mixed_ladder(rungs):
    """a ladder whose rungs are tips and cherries (one tip, then two cherries, and so on), on alternating sides"""
    s = ((0, 0), 0)
    for i in range(rungs):
        f = 0 if i % 3 == 0 else (0, 0)
        s = (s, f) if i % 2 else (f, s)
    return s


def _balanced_shape(n):
    return 0 if n == 1 else (_balanced_shape(n // 2), _balanced_shape(n // 2))


# "slot1" (36 tips, one chunk): a ladder of three shaped nodes over a balanced 16-tip subtree, beside another such subtree whose
# walk nests one wait -- the ladder's top waits in the second slot (source 3) while its own stored child is not elided
SLOT1_SHAPE = (((((_balanced_shape(16), 0), 0), 0), _balanced_shape(16)), 0)


# "prologue_right" (16 tips, one chunk): the root's children are a shaped node beside a cherry, over a ladder of six stored nodes,
# and a smaller ladder.  The pre-order walk enters the smaller one first, so the shaped node is the RIGHT child of the op that
# opens the chunk, whose prologue must ask for its stored child; the post-order walk takes it from park slot 0.  (The side a
# child has in a streamed op follows the subtree sizes, not left and right: a mirror image keeps every side)
PROLOGUE_RIGHT_SHAPE = ((u.ops_shape(6), (0, 0)), u.ops_shape(2))


@functools.lru_cache(maxsize=None)
def _make(name, bl):
    if name in u.NAMED:
        return u.make_tree(name, bl)
    if name == "caterpillar64":  # a ladder of 64 tips: every rung is shaped, every other one is elided
        return u.from_nested(u.ops_shape(61), 31, bl)
    if name == "prologue_right":
        return u.from_nested(PROLOGUE_RIGHT_SHAPE, 34, bl)
    if name == "ladder160":  # 160 tips: deep enough to be rescaled several times (GPU test), both sibling kinds (the stored child of a ladder is the carried, left one)
        return u.from_nested(_mixed_ladder(94), 33, bl)
    if name == "slot1":
        return u.from_nested(SLOT1_SHAPE, 32, bl)
    if name == "bench":
        return synth.random_tree(1000, np.random.default_rng(1))
    raise ValueError(name)


def make_tree(name, bl=(0.01, 0.1), mirror=False):
    return u.mirrored(_make(name, tuple(bl))) if mirror else _make(name, tuple(bl))


ALL = u.NAMED + EXTRA


@functools.lru_cache(maxsize=None)
def reach(name, mirror=False):
    return check_rule(make_tree(name, mirror=mirror))


# the cases and the tree that is in the GPU test for each (test_stream_elide_schedule.py asserts that it reaches it)
CASES = {
    "both new kinds on both sides": ("random200", lambda r: r["kind_sides"] == {(u.TIP, 0), (u.TIP, 1), (u.CHERRY, 0), (u.CHERRY, 1)}),
    "an elided node taken from park slot 0": ("random200", lambda r: r["slot0"] > 0),
    "a chain of three shaped nodes, alternate ones elided": ("random200", lambda r: r["chain"] >= 3),
    "a shaped node refused for source 0 (memory)": ("target", lambda r: r["refused_memory"] > 0),
    "a shaped node refused for source 3 (the second slot)": ("slot1", lambda r: r["refused_slot1"] > 0),
    "an elided node that opens a chunk of the pre-order walk": ("target", lambda r: r["pre_cut_roots"] > 0),
    "an elided left child of an op that opens a pre-order chunk (the prologue requests its stored child)": ("target", lambda r: 0 in r["prologue_sides"]),
    "an elided right child of an op that opens a pre-order chunk": ("prologue_right", lambda r: 1 in r["prologue_sides"]),
}
GPU_TREES = tuple(sorted({name for name, _ in CASES.values()}))
