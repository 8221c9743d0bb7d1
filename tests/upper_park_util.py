"""The host schedule's account of the 4-state pre-order walk (phyamd_pre_order_schedule), a checker of its contract, and the
trees on which the CPU and GPU tests of the walk's carries, LDS parks and HBM slots run.

One record per op, in launch order (the top part, then the cut subtrees' chunks); the columns are those of include/physher_amd.h:
  CHUNK | NODE | LEFT | RIGHT | KIND_LEFT | KIND_RIGHT (TIP, CORE = stored, DEEP, CHERRY, CHERRY_TIP)
  HALF_L0 HALF_L1 | HALF_R0 HALF_R1   kinds of a DEEP child's halves (-1: the child is not DEEP)
  SRC | SRC_SLOT                      where the node's own upper comes from: ROOT, CARRY, LDS0, LDS1, HBM; its HBM slot
  DST_LEFT | SLOT_LEFT | DST_RIGHT | SLOT_RIGHT   where each child's upper goes: NONE, CARRY, LDS0, LDS1, HBM; the slot stored to
  PREFETCH                            form 1: the HBM slot requested for the next op (-1: none)
  CUT                                 bit 0 / 1: the left / right child is the root of a cut subtree
  CARRIED                             0 none, 1 left, 2 right (forms 0 and 2: as scheduled, even where a cut sent it through HBM)
  QCOUNT | Q0 .. Q9                   the nodes whose branch terms the op produces
Forms: 0 = the chunked list (k_upper4_walk), 1 = the streamed walk's rewrite of it (k_upper4_stream), 2 = the one unchunked list
(k_upper4_walk's parameter form)."""
import functools
import itertools

import numpy as np

from lower_park_util import _tree, balanced_tree, caterpillar_of_subtrees
from lower_park_util import make_tree as lower_make_tree
from physher_amd import _lib, synth

COLUMNS = 30
(CHUNK, NODE, LEFT, RIGHT, KIND_LEFT, KIND_RIGHT, HALF_L0, HALF_L1, HALF_R0, HALF_R1, SRC, SRC_SLOT, DST_LEFT, SLOT_LEFT, DST_RIGHT, SLOT_RIGHT,
 PREFETCH, CUT, CARRIED, QCOUNT, Q0) = range(21)
TIP, CORE, DEEP, CHERRY, CHERRY_TIP = range(5)
KIND_NAMES = ("TIP", "CORE", "DEEP", "CHERRY", "CHERRY_TIP")
ROOT, CARRY, LDS0, LDS1, HBM = range(5)  # sources; destinations use the same codes with 0 = NONE
NONE = 0
CHUNK_MIN_OPS, CHUNK_MIN_TARGET, WALK_CHUNKS = 32, 16, 3  # chunk_pre_order


def chunk_target(n):
    return max(CHUNK_MIN_TARGET, -(-n // WALK_CHUNKS))


def pre_order_schedule(tree, form):
    """(records [ops][COLUMNS], HBM slots the list needs)"""
    lib = _lib.load()
    T = tree.tip_count
    left = np.ascontiguousarray(tree.left, dtype=np.int32)
    right = np.ascontiguousarray(tree.right, dtype=np.int32)
    out = np.full((T, COLUMNS), -7, dtype=np.int32)
    slots = np.zeros(1, dtype=np.int32)
    n = lib.phyamd_pre_order_schedule(T, left.ctypes.data, right.ctypes.data, int(tree.root), form, out.ctypes.data, T, slots.ctypes.data)
    assert n >= 0, lib.phyamd_last_error()
    assert n <= T
    return out[:n], int(slots[0])


# ---- trees -----------------------------------------------------------------------------------------------------------------

def from_nested(shape, seed=1, bl=(0.01, 0.1)):
    """a tree from nested pairs: 0 (or any non-tuple) is a tip, (a, b) an internal node; tips are numbered left to right"""
    count = itertools.count()

    def tips(s):
        return [tips(s[0]), tips(s[1])] if isinstance(s, tuple) else next(count)

    named = tips(shape)
    T = next(count)
    left, right = [-1] * T, [-1] * T

    def build(s):
        if not isinstance(s, list):
            return s
        l, r = build(s[0]), build(s[1])
        left.append(l)
        right.append(r)
        return len(left) - 1

    build(named)
    return _tree(left, right, seed, bl)


def mirrored(tree):
    """left and right swapped at every internal node"""
    return synth.SynthTree(np.array(tree.right, dtype=np.int32), np.array(tree.left, dtype=np.int32), np.array(tree.length), list(tree.names))


def ops_shape(n):
    """a nested shape whose pre-order walk has exactly n ops with no park: a ladder of n stored nodes over a cherry + tip foot"""
    s = ((0, 0), 0)
    for _ in range(n):
        s = (s, 0)
    return s


def bushy_ops_shape(n):
    """a nested shape with exactly n ops whose walk parks: park-free ladders of at most 5 ops joined pairwise"""
    if n <= 5:
        return ops_shape(n) if n > 0 else ((0, 0), 0)
    rest = n - 1
    a = rest // 2
    return (bushy_ops_shape(rest - a), bushy_ops_shape(a))


FRINGE_SHAPES = {TIP: 0, CHERRY: (0, 0), CHERRY_TIP: ((0, 0), 0)}


def fringe_pair_shapes():
    """name -> (nested shape, kinds): trees of 2 to 6 tips that put every ordered pair of fringe kinds under the root, the only
    op whose children can both be tips or fringe without the node being fringe or DEEP itself (a DEEP node's own op aside)"""
    return {f"{KIND_NAMES[a]}-{KIND_NAMES[b]}": ((FRINGE_SHAPES[a], FRINGE_SHAPES[b]), (a, b)) for a, b in itertools.product(FRINGE_SHAPES, repeat=2)}


def deep_shape(a, b):
    """a DEEP node with halves of kinds a and b (two tips make a cherry, a cherry and a tip a cherry + tip: those pairs are not DEEP)"""
    return (FRINGE_SHAPES[a], FRINGE_SHAPES[b])


DEEP_PAIRS = tuple((a, b) for a, b in itertools.product((TIP, CHERRY, CHERRY_TIP), repeat=2) if {a, b} not in ({TIP}, {TIP, CHERRY}))


def kinds_gallery():
    """one tree that holds every ordered pair (kind_left, kind_right) with a CORE or DEEP side, and every kind of half in both
    halves of a DEEP child on both sides: a spine whose rungs are the pairs"""
    core = (deep_shape(CHERRY, CHERRY), 0)  # the smallest stored node below the root: a DEEP child and a tip
    deep = deep_shape(CHERRY, CHERRY)
    rungs = []
    for k in (TIP, CHERRY, CHERRY_TIP):
        rungs += [(FRINGE_SHAPES[k], core), (core, FRINGE_SHAPES[k]), (FRINGE_SHAPES[k], deep), (deep, FRINGE_SHAPES[k])]
    rungs += [(core, core), (core, deep), (deep, core)]
    rungs += [(deep_shape(a, b), deep_shape(a, b)) for a, b in DEEP_PAIRS]  # (two DEEP children are never swapped: both sides, both forms)
    spine = rungs[0]
    for i, r in enumerate(rungs[1:]):
        spine = (spine, r) if i % 2 else (r, spine)
    return spine


NAMED = ("caterpillar", "balanced64", "random200", "gallery", "ops31", "ops32", "ops33", "target", "random97", "random150m", "balanced40m",
         "reuse56m")


@functools.lru_cache(maxsize=None)
def _named_shape_tree(name, bl):
    if name in ("caterpillar", "balanced64", "random200"):
        return lower_make_tree(name, bl)
    if name == "gallery":
        return from_nested(kinds_gallery(), 21, bl)
    if name in ("ops31", "ops32", "ops33"):
        return from_nested(bushy_ops_shape(int(name[3:])), 22, bl)
    if name == "target":
        return from_nested(TARGET_SHAPE, 23, bl)
    if name == "random97":
        return synth.random_tree(97, np.random.default_rng(5), bl_low=bl[0], bl_high=bl[1])
    if name == "random150m":
        return mirrored(synth.random_tree(150, np.random.default_rng(8), bl_low=bl[0], bl_high=bl[1]))
    if name == "balanced40m":
        return mirrored(balanced_tree(40, 24, bl))
    if name == "reuse56m":  # (found by search: the streamed form, with its second LDS slot, still recycles an HBM slot inside one chunk)
        return mirrored(caterpillar_of_subtrees((8, 32, 16), 25, bl))
    raise ValueError(name)


def make_tree(name, bl=(0.01, 0.1)):
    return _named_shape_tree(name, tuple(bl))


# "target": n ops in all with target = ceil(n / 3); under a short top ladder, siblings of exactly target and target + 1 ops (the
# first is cut whole, the second is descended into: its children are cut) and one more subtree that keeps n where it is.
# n = 66: target 22.  Ops: subtrees 22 + 23 + 17, their two joins, and a top ladder of 2 = 66.
TARGET_SHAPE = ((((ops_shape(22), (ops_shape(11), ops_shape(11))), ops_shape(17)), 0), 0)


@functools.lru_cache(maxsize=None)
def named_schedule(name, form):
    ops, slots = pre_order_schedule(make_tree(name), form)
    ops.setflags(write=False)
    return ops, slots


# ---- the contract ----------------------------------------------------------------------------------------------------------

def children(op):
    """(side, child node, kind, destination, stored slot) of both children"""
    return ((0, int(op[LEFT]), int(op[KIND_LEFT]), int(op[DST_LEFT]), int(op[SLOT_LEFT])),
            (1, int(op[RIGHT]), int(op[KIND_RIGHT]), int(op[DST_RIGHT]), int(op[SLOT_RIGHT])))


def chunk_bounds(ops):
    """[begin, end) of every chunk; asserts that chunk numbers count up from 0 without gaps"""
    chunk = ops[:, CHUNK]
    assert chunk[0] == 0 and ((np.diff(chunk) == 0) | (np.diff(chunk) == 1)).all(), "chunk numbers do not count up"
    starts = [0] + [int(i) + 1 for i in np.flatnonzero(np.diff(chunk))]
    return list(zip(starts, starts[1:] + [len(ops)]))


def check_contract(tree, ops, slots, form):
    """every rule of the pre-order schedule's contract that can be read off one form's records; returns statistics"""
    T, N = tree.tip_count, 2 * tree.tip_count - 1
    left, right = np.asarray(tree.left), np.asarray(tree.right)
    n = len(ops)
    assert (ops != -7).all(), "a column was not written"
    op_of = {}
    for i, op in enumerate(ops):
        assert int(op[NODE]) not in op_of, f"node {op[NODE]} has two ops"
        op_of[int(op[NODE])] = i
        assert {int(op[LEFT]), int(op[RIGHT])} == {int(left[op[NODE]]), int(right[op[NODE]])}, f"op {op[NODE]}: not the tree's children"
        if form != 1:
            assert op[LEFT] == left[op[NODE]], f"op {op[NODE]}: children swapped outside the streamed form"
    # -- coverage: kinds from the tree itself (build_schedule's fringe rule), one op per CORE / DEEP internal node
    kind = [TIP] * T + [CORE] * (N - T)
    order, stack = [], [int(tree.root)]
    while stack:
        v = stack.pop()
        order.append(v)
        if v >= T:
            stack += [int(left[v]), int(right[v])]
    assert len(order) == N
    for v in reversed(order):
        if v < T or v == tree.root:
            continue
        l, r = int(left[v]), int(right[v])
        if l < T and r < T:
            kind[v] = CHERRY
        elif (l < T and kind[r] == CHERRY) or (r < T and kind[l] == CHERRY):
            kind[v] = CHERRY_TIP
        elif kind[l] not in (CORE, DEEP) and kind[r] not in (CORE, DEEP):
            kind[v] = DEEP
    with_op = {v for v in range(T, N) if kind[v] in (CORE, DEEP)}
    assert set(op_of) == with_op, f"ops and CORE / DEEP nodes differ: {sorted(set(op_of) ^ with_op)}"
    for op in ops:
        for side, ch, k, dst, slot in children(op):
            assert k == kind[ch], f"op {op[NODE]}: child {ch} is {KIND_NAMES[kind[ch]]}, the record says {KIND_NAMES[k]}"
            halves = (int(op[HALF_R0 if side else HALF_L0]), int(op[HALF_R1 if side else HALF_L1]))
            if k == DEEP:
                # (the streamed form swaps an op's children, never a DEEP child's halves)
                assert halves == (kind[left[ch]], kind[right[ch]]), f"op {op[NODE]}: halves of DEEP child {ch}"
            else:
                assert halves == (-1, -1)
    roots = [int(op[NODE]) for op in ops if op[SRC] == ROOT]
    assert roots == [int(tree.root)] and ops[0, NODE] == tree.root, f"source ROOT at {roots}"
    # -- branch terms: every non-root node exactly once
    qnodes = [int(q) for op in ops for q in op[Q0:Q0 + op[QCOUNT]]]
    assert sorted(qnodes) == sorted(set(range(N)) - {int(tree.root)}), "branch terms are not every non-root node exactly once"
    for op in ops:
        assert (op[Q0 + op[QCOUNT]:Q0 + 10] == -1).all()

    bounds = chunk_bounds(ops)
    target = chunk_target(n)
    # -- chunks
    if n < CHUNK_MIN_OPS:
        assert len(bounds) == 1, f"{n} ops in {len(bounds)} chunks"
    size = {}
    for v in reversed(order):
        size[v] = 1 + size.get(int(left[v]), 0) + size.get(int(right[v]), 0) if v in op_of else 0
    cut_roots = set()
    for op in ops:
        for side, ch, k, dst, slot in children(op):
            if op[CUT] & (1 << side):
                cut_roots.add(ch)
    if form == 2:
        assert len(bounds) == 1 and not cut_roots
    first_nodes = [int(ops[b, NODE]) for b, _ in bounds[1:]]
    assert sorted(first_nodes) == sorted(cut_roots), "the chunks' first ops are not the cut children"
    lengths = [e - b for b, e in bounds[1:]]
    assert lengths == sorted(lengths, reverse=True), f"cut subtrees are not longest first: {lengths}"
    for (b, e), root in zip(bounds[1:], first_nodes):
        assert e - b == size[root] <= target, f"chunk of {root}: {e - b} ops, subtree {size[root]}, target {target}"
        inside = {root}
        for op in ops[b:e]:  # contiguous subtree, parents before children
            assert int(op[NODE]) in inside, f"op {op[NODE]} is not in the subtree of {root}"
            inside |= {int(op[LEFT]), int(op[RIGHT])}
        assert op_of[_parent(tree, root)] < bounds[0][1], f"cut subtree {root} does not hang off the top part"
    for op in ops[bounds[0][0]:bounds[0][1]]:  # top part: a child is cut exactly when its subtree fits the target
        for side, ch, k, dst, slot in children(op):
            if ch in op_of and len(bounds) > 1:
                assert (ch in cut_roots) == (size[ch] <= target), f"child {ch} of {op[NODE]}: {size[ch]} ops against target {target}"
    if n >= CHUNK_MIN_OPS and form != 2:
        assert size[int(tree.root)] == n > target and len(bounds) > 1, "a list of 32 ops or more is cut"

    # -- the walk: carries, LDS slots per chunk, HBM slots globally
    hbm = {}          # slot -> (node, writer op index), unread
    hbm_writes = {}   # slot -> [writer chunk, ...] over the whole walk
    hbm_chunks = {}   # slot -> chunks that touch it
    cross_slots = set()
    stats = dict(ops=n, chunks=len(bounds), src=set(), dst=set(), internal_reuse=0, both_cut=0, right_carried=0, cut_carried=0, cut_parked=0,
                 parks=0)
    written = {}      # node -> ("carry" | "lds0" | "lds1" | "hbm", writer op index)
    reads = []        # (reader index, slot, writer index)
    for b, e in bounds:
        lds = {LDS0: None, LDS1: None}
        for i in range(b, e):
            op = ops[i]
            node, src = int(op[NODE]), int(op[SRC])
            stats["src"].add(src)
            if src == ROOT:
                assert op[SRC_SLOT] == -1
            elif src == CARRY:
                assert i > b, f"op {node}: the first op of a chunk takes its upper from registers"
                prev = ops[i - 1]
                assert node in (int(prev[LEFT]), int(prev[RIGHT])), f"op {node}: CARRY, but the op in front is {prev[NODE]}, not its parent"
                side = 0 if node == prev[LEFT] else 1
                assert prev[CARRIED] == side + 1, f"op {node}: CARRY, but parent {prev[NODE]} carries child {prev[CARRIED]}"
                assert prev[DST_RIGHT if side else DST_LEFT] == CARRY, f"op {node}: CARRY, but parent {prev[NODE]} sends it elsewhere"
                if form == 1:
                    assert side == 0, f"op {node}: the streamed walk carries the left child's upper only"
            elif src in (LDS0, LDS1):
                assert form == 1 or src == LDS0, f"op {node}: slot 1 outside the streamed form"
                assert form != 2, f"op {node}: the parameter form has no LDS slot"
                assert lds[src] is not None and lds[src][0] == node, f"op {node}: LDS slot {src - LDS0} holds {lds[src]}"
                assert ops[lds[src][1], NODE] == _parent(tree, node)
                lds[src] = None
            else:
                assert src == HBM
                s = int(op[SRC_SLOT])
                assert 0 <= s < slots, f"op {node}: reads slot {s} of {slots}"
                assert s in hbm and hbm[s][0] == node, f"op {node}: HBM slot {s} holds {hbm.get(s)}"
                w = hbm.pop(s)[1]
                assert ops[w, NODE] == _parent(tree, node)
                reads.append((i, s, w))
                hbm_chunks.setdefault(s, set()).add(int(op[CHUNK]))
                if ops[w, CHUNK] != op[CHUNK]:
                    assert i == b and ops[w, CHUNK] == 0, f"op {node}: slot {s} crosses chunks, but not from the top part to a chunk's first op"
                    cross_slots.add(s)
            if src != CARRY and i > b and node in (int(ops[i - 1, LEFT]), int(ops[i - 1, RIGHT])) and form == 1:
                # the prefetch of this op's slot is issued inside the op in front: that op must not be the writer
                assert src != HBM, f"op {node}: reads the HBM slot the op in front has only just stored"
            for side, ch, k, dst, slot in children(op):
                stats["dst"].add(dst)
                if ch not in op_of:
                    assert dst == NONE and slot == -1, f"op {node}: child {ch} has no op but its upper goes to {dst} / slot {slot}"
                    continue
                cut = bool(op[CUT] & (1 << side))
                assert dst != NONE, f"op {node}: the upper of child {ch} goes nowhere"
                assert (dst == HBM) == (slot >= 0), f"op {node}: child {ch}: destination {dst} with slot {slot}"
                if cut:
                    assert dst == HBM, f"op {node}: cut child {ch} does not go through HBM"
                    stats["cut_carried" if op[CARRIED] == side + 1 else "cut_parked"] += 1 if form == 0 else 0
                if dst == CARRY:
                    assert op[CARRIED] == side + 1
                    assert i + 1 < e and ops[i + 1, NODE] == ch and ops[i + 1, SRC] == CARRY, f"op {node}: carried child {ch} is not the next op"
                elif dst in (LDS0, LDS1):
                    assert form == 1 or dst == LDS0, f"op {node}: slot 1 outside the streamed form"
                    assert form != 2
                    assert lds[dst] is None, f"op {node}: LDS slot {dst - LDS0} still holds {lds[dst]}"
                    lds[dst] = (ch, i)
                    stats["parks"] += 1
                else:
                    assert 0 <= slot < slots, f"op {node}: writes slot {slot} of {slots}"
                    assert slot not in hbm, f"op {node}: HBM slot {slot} still holds {hbm[slot]}"
                    assert not (src == HBM and slot == op[SRC_SLOT]), f"op {node}: writes slot {slot}, which it reads its own upper from"
                    hbm[slot] = (ch, i)
                    hbm_writes.setdefault(slot, []).append(int(op[CHUNK]))
                    hbm_chunks.setdefault(slot, set()).add(int(op[CHUNK]))
                    stats["parks"] += 0 if cut else 1
                assert written.setdefault(ch, (dst, i))[1] == i
            if op[CUT] == 3:
                stats["both_cut"] += 1
            if op[CARRIED] == 2:
                stats["right_carried"] += 1
            if form == 1:
                assert op[CARRIED] in (0, 1)
        assert lds == {LDS0: None, LDS1: None}, f"chunk {ops[b, CHUNK]} ends with a value parked: {lds}"
    assert not hbm, f"HBM slots written and never read: {hbm}"
    for v in with_op - {int(tree.root)}:
        assert v in written, f"node {v}: nobody produces its upper"
    for s, writers in hbm_writes.items():
        if s in cross_slots:
            assert writers == [0] and len(hbm_chunks[s]) == 2, f"cross slot {s}: written by chunks {writers}, touched by {hbm_chunks[s]}"
        else:  # chunks of one pattern block may run at the same time: a recycled slot belongs to one of them
            assert len(hbm_chunks[s]) == 1, f"slot {s} is recycled inside chunk {writers[0]} and touched by chunks {hbm_chunks[s]}"
            if len(writers) > 1:
                stats["internal_reuse"] += 1
    # -- prefetch (form 1)
    if form == 1:
        for b, e in bounds:
            for i in range(b, e):
                want = int(ops[i + 1, SRC_SLOT]) if i + 1 < e and ops[i + 1, SRC] == HBM else -1
                assert ops[i, PREFETCH] == want, f"op {ops[i, NODE]}: prefetches {ops[i, PREFETCH]}, the next op reads {want}"
        for i, s, w in reads:
            if not any(i == b for b, _ in bounds):
                assert w < i - 1, f"op {ops[i, NODE]}: slot {s} is prefetched inside op {i - 1}, which is the op that writes it"
    else:
        assert (ops[:, PREFETCH] == -1).all()
    stats["cut_sizes"] = sorted(lengths)
    stats["target"] = target
    stats["kind_pairs"] = {(int(op[KIND_LEFT]), int(op[KIND_RIGHT])) for op in ops}
    stats["halves"] = {(side, h, int(op[(HALF_L0, HALF_L1, HALF_R0, HALF_R1)[2 * side + h]])) for op in ops for side in (0, 1) for h in (0, 1)
                       if op[KIND_RIGHT if side else KIND_LEFT] == DEEP}
    stats["descended"] = sorted(size[ch] for op in ops[bounds[0][0]:bounds[0][1]] for _, ch, _, _, _ in children(op)
                                if ch in op_of and ch not in cut_roots and len(bounds) > 1)
    return stats


def _parent(tree, node):
    p = getattr(tree, "_parent_cache", None)
    if p is None:
        p = {}
        for v in range(tree.tip_count, 2 * tree.tip_count - 1):
            p[int(tree.left[v])] = v
            p[int(tree.right[v])] = v
        try:
            tree._parent_cache = p
        except AttributeError:
            pass
    return p[node]


def check_forms_agree(zero, one):
    """form 1 is form 0 op by op but for what stream_pre_order documents: children swapped where the carried child was the right
    one, the registers of the op in front instead of an HBM slot that op stored, and slot-1 parks instead of HBM parks"""
    assert len(zero) == len(one)
    assert (zero[:, CHUNK] == one[:, CHUNK]).all() and (zero[:, NODE] == one[:, NODE]).all(), "not the same ops in the same order"
    moved = dict(swapped=0, from_prev=0, slot1=0)
    dst_of = {}  # form-1 destination of every node's upper
    for a, b in zip(zero, one):
        swapped = a[LEFT] != b[LEFT]
        if swapped:
            moved["swapped"] += 1
            assert (a[LEFT], a[RIGHT]) == (b[RIGHT], b[LEFT])
        carried = int(a[CARRIED]) - 1  # the side (of form 0) whose upper the next op takes in registers; -1: none
        for side in (0, 1):
            t = 1 - side if swapped else side
            col = lambda l, r, s: r if s else l
            assert a[col(KIND_LEFT, KIND_RIGHT, side)] == b[col(KIND_LEFT, KIND_RIGHT, t)]
            assert a[col(HALF_L0, HALF_R0, side)] == b[col(HALF_L0, HALF_R0, t)] and a[col(HALF_L1, HALF_R1, side)] == b[col(HALF_L1, HALF_R1, t)]
            assert bool(a[CUT] & (1 << side)) == bool(b[CUT] & (1 << t))
            da, db = int(a[col(DST_LEFT, DST_RIGHT, side)]), int(b[col(DST_LEFT, DST_RIGHT, t)])
            sa, sb = int(a[col(SLOT_LEFT, SLOT_RIGHT, side)]), int(b[col(SLOT_LEFT, SLOT_RIGHT, t)])
            dst_of[int(a[col(LEFT, RIGHT, side)])] = (da, db)
            if (da, sa) == (db, sb):
                continue
            assert da == HBM and not a[CUT] & (1 << side), f"op {a[NODE]}: a destination other than an uncut HBM park moved: {da} -> {db}"
            assert db in (CARRY, LDS1), f"op {a[NODE]}: HBM park became {db}"
            moved["from_prev" if db == CARRY else "slot1"] += 1
            if db == CARRY:  # the scheduled carry went to a cut subtree: the registers are free for the parked child
                assert carried < 0 or a[CUT] & (1 << carried), f"op {a[NODE]}: two carried children"
                carried = side
        assert swapped == (carried == 1), f"op {a[NODE]}: children {'swapped' if swapped else 'kept'}, carried side {carried}"
        assert sorted(a[Q0:Q0 + a[QCOUNT]]) == sorted(b[Q0:Q0 + b[QCOUNT]]), f"op {a[NODE]}: the forms produce different branch terms"
    for a, b in zip(zero, one):
        if (a[SRC], a[SRC_SLOT]) == (b[SRC], b[SRC_SLOT]):
            continue
        da, db = dst_of[int(a[NODE])]
        assert a[SRC] == HBM and (b[SRC], db) in ((CARRY, CARRY), (LDS1, LDS1)), f"op {a[NODE]}: source {a[SRC]} -> {b[SRC]}, destination {da} -> {db}"
    return moved


# ---- what each named tree is in the set for ----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def named_stats(name):
    """(statistics of form 0, of form 1, what stream_pre_order moved) of a named tree, contract checked"""
    tree = make_tree(name)
    st = [check_contract(tree, *named_schedule(name, form), form) for form in (0, 1)]
    return st[0], st[1], check_forms_agree(named_schedule(name, 0)[0], named_schedule(name, 1)[0])


def chosen_for(name):
    """(what the tree is in the named set for, whether its schedule shows it)"""
    s0, s1, moved = named_stats(name)
    every = {ROOT, CARRY, LDS0, LDS1, HBM}
    op_kinds = (CORE, DEEP)
    if name == "caterpillar":
        return "a cut carried child whose parked sibling takes the registers (from_prev), and an op with both children cut", \
            s0["cut_carried"] > 0 and moved["from_prev"] > 0 and s0["both_cut"] > 0
    if name == "balanced64":
        return "31 ops in one chunk that use every source and destination of the streamed form", \
            s1["ops"] == 31 and s1["chunks"] == 1 and s1["src"] == every and s1["dst"] == every
    if name == "random200":
        return "a random tree: children swapped, slot-1 parks, recycled slots in the chunked list, cut children carried and parked", \
            moved["swapped"] > 0 and moved["slot1"] > 0 and s0["internal_reuse"] > 0 and s0["cut_carried"] > 0 and s0["cut_parked"] > 0
    if name == "gallery":
        pairs = {(a, b) for a in range(5) for b in range(5) if a in op_kinds or b in op_kinds}
        halves = {(side, h, k) for side in (0, 1) for h in (0, 1) for k in (TIP, CHERRY, CHERRY_TIP)}
        return "every pair of child kinds with an op on one side, every kind in every half of a DEEP child on both sides", \
            s0["kind_pairs"] >= pairs and s0["halves"] >= halves and s1["halves"] >= halves
    if name in ("ops31", "ops32", "ops33"):
        n = int(name[3:])
        return f"{n} ops: {'one chunk' if n < CHUNK_MIN_OPS else 'the shortest list that is cut'}", \
            s0["ops"] == n and (s0["chunks"] == 1) == (n < CHUNK_MIN_OPS) and s0["parks"] > 0
    if name == "target":
        return "a cut subtree of exactly `target` ops beside one of target + 1 that is descended into", \
            s0["target"] in s0["cut_sizes"] and s0["target"] + 1 in s0["descended"]
    if name == "random97":
        return "a small random tree just past the threshold: target 17, two ops with both children cut", s0["target"] == 17 and s0["both_cut"] == 2
    if name == "random150m":
        return "a mirrored random tree: right carries in the chunked list, a cut subtree of one op", s0["right_carried"] > 0 and 1 in s0["cut_sizes"]
    if name == "balanced40m":
        return "under the threshold: one chunk with a recycled slot in the chunked list and slot-1 parks in the streamed form", \
            s0["chunks"] == 1 and s0["internal_reuse"] > 0 and moved["slot1"] > 0
    if name == "reuse56m":
        return "an HBM slot written twice in one chunk of the streamed form", s1["internal_reuse"] > 0
    raise ValueError(name)
