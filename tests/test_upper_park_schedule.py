"""CPU-only: the contract of the 4-state pre-order walk's host schedule (phyamd_pre_order_schedule: build_schedule,
chunk_pre_order and stream_pre_order, no device).  An op's own upper arrives in the registers of the op in front, from one of a
wave's two LDS park slots, from an HBM slot recycled inside a chunk or from one that crosses from the top part to a cut subtree;
k_upper4_walk and k_upper4_stream check none of it, so the schedule has to (upper_park_util.check_contract):
  * coverage: one op per CORE / DEEP node, the root's the only one without a source, every non-root branch term once;
  * carry: a carried upper is the marked child of the op directly in front, in the same chunk (streamed form: its left child);
  * LDS: written only when empty, read by the node it holds, written by that node's parent in the same chunk, empty at a chunk's
    end, slot 1 in the streamed form only;
  * HBM: indices below the returned count, a read finds its own node as the last write, no write over an unread value, every value
    read once, no op writes the slot it reads, a recycled slot stays inside one chunk, a crossing slot is written once by the top
    part, read by the first op of one other chunk and never recycled;
  * prefetch (streamed form): op i requests exactly the slot op i + 1 reads, which an op before i wrote; a chunk's last op none;
  * chunks: under 32 ops one chunk, else the top part and contiguous subtrees of at most `target` ops, longest first;
  * the streamed form against the chunked list: the same ops, differing only by stream_pre_order's documented rewrites.
Form 2 (the unchunked list) is what k_upper4_walk's parameter form reads: one chunk, no LDS slot, the free_w slots."""
import time

import numpy as np
import pytest

import upper_park_util as u
from physher_amd import _lib, synth

BENCH = "bench1000"
FORMS = (0, 1, 2)


def _tree(name):
    mirror = name.endswith("~")
    base = name.rstrip("~")
    tree = synth.random_tree(1000, np.random.default_rng(1)) if base == BENCH else u.make_tree(base)
    return u.mirrored(tree) if mirror else tree


def _check_all_forms(tree):
    recs = {}
    for form in FORMS:
        ops, slots = u.pre_order_schedule(tree, form)
        assert len(ops) > 0
        u.check_contract(tree, ops, slots, form)
        recs[form] = ops
    u.check_forms_agree(recs[0], recs[1])
    assert sorted(recs[0][:, u.NODE]) == sorted(recs[2][:, u.NODE])
    if recs[0][-1, u.CHUNK] == 0:
        assert (recs[0][:, u.NODE] == recs[2][:, u.NODE]).all(), "an uncut list has the one list's order"
    return len(recs[0])


ALL_NAMES = tuple(n + m for n in u.NAMED + (BENCH,) for m in ("", "~"))  # "~": the mirror image


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ALL_NAMES)
def test_contract(name, form):
    tree = _tree(name)
    ops, slots = u.pre_order_schedule(tree, form)
    stats = u.check_contract(tree, ops, slots, form)
    if form == 0:
        assert u.LDS1 not in stats["src"] | stats["dst"]  # those parks are in HBM there
    if form == 2:
        assert not {u.LDS0, u.LDS1} & (stats["src"] | stats["dst"]) and stats["chunks"] == 1


@pytest.mark.parametrize("name", ALL_NAMES)
def test_streamed_form_differs_from_the_chunked_list_only_as_documented(name):
    tree = _tree(name)
    u.check_forms_agree(u.pre_order_schedule(tree, 0)[0], u.pre_order_schedule(tree, 1)[0])


def test_seeded_sweep():
    """random, caterpillar and balanced trees and their mirror images from 2 tips through the chunking threshold (32 ops: 40 to 70
    tips, by shape) and past it, all three forms and the comparison of forms 0 and 1"""
    t0 = time.perf_counter()
    trees, most_ops, seen_ops = 0, 0, set()
    sizes = list(range(2, 97)) + [101, 127, 128, 129, 160, 193, 256, 300, 400]
    for T in sizes:
        for shape, seeds in (("random", 3 if T < 97 else 2), ("caterpillar", 1), ("balanced", 1)):
            for seed in range(seeds):
                tree = synth.random_tree(T, np.random.default_rng(100 * T + seed), shape=shape)
                for t in (tree, u.mirrored(tree)):
                    n = _check_all_forms(t)
                    trees += 1
                    most_ops = max(most_ops, n)
                    seen_ops.add(n)
    print(f"sweep: {trees} trees, up to {most_ops} ops, {time.perf_counter() - t0:.1f} s")
    assert {31, 32, 33} <= seen_ops, "the sweep does not straddle the chunking threshold"


@pytest.mark.parametrize("name", sorted(u.fringe_pair_shapes()))
def test_every_pair_of_fringe_kinds_under_the_root(name):
    shape, want = u.fringe_pair_shapes()[name]
    tree = u.from_nested(shape)
    for t in (tree, u.mirrored(tree)):
        _check_all_forms(t)
    ops, _ = u.pre_order_schedule(tree, 0)
    assert len(ops) == 1 and (int(ops[0, u.KIND_LEFT]), int(ops[0, u.KIND_RIGHT])) == want, (name, ops[0, :6])
    assert ops[0, u.SRC] == u.ROOT and ops[0, u.QCOUNT] == 2 * tree.tip_count - 2


def test_chunking_threshold():
    for name, chunks in (("ops31", 1), ("ops32", 3), ("ops33", 3)):
        for form in (0, 1):
            ops, _ = u.named_schedule(name, form)
            assert len(ops) == int(name[3:]) and ops[-1, u.CHUNK] + 1 == chunks, (name, form, len(ops), ops[-1, u.CHUNK] + 1)


def _reach():
    """what the named set reaches, from the exports alone"""
    got = dict(src1=set(), dst1=set(), reuse0=[], reuse1=[], cut_carried=[], cut_parked=[], from_prev=[], both_cut=[], right_carried0=[], ops=set(),
               cut_target=[], descended_target1=[], pairs0=set(), pairs1=set(), halves0=set(), halves1=set())
    for name in u.NAMED:
        tree = u.make_tree(name)
        assert tree.tip_count <= 310
        st = {}
        for form in (0, 1):
            ops, slots = u.named_schedule(name, form)
            st[form] = u.check_contract(tree, ops, slots, form)
        moved = u.check_forms_agree(u.named_schedule(name, 0)[0], u.named_schedule(name, 1)[0])
        got["src1"] |= st[1]["src"]
        got["dst1"] |= st[1]["dst"]
        got["ops"].add(st[0]["ops"])
        for key, form, stat in (("reuse0", 0, "internal_reuse"), ("reuse1", 1, "internal_reuse"), ("cut_carried", 0, "cut_carried"), ("cut_parked", 0, "cut_parked"),
                                ("both_cut", 1, "both_cut"), ("right_carried0", 0, "right_carried")):
            if st[form][stat]:
                got[key].append(name)
        if moved["from_prev"]:
            got["from_prev"].append(name)
        if st[0]["target"] in st[0]["cut_sizes"]:
            got["cut_target"].append(name)
            if st[0]["target"] + 1 in st[0]["descended"]:
                got["descended_target1"].append(name)
        for form in (0, 1):
            got[f"pairs{form}"] |= st[form]["kind_pairs"]
            got[f"halves{form}"] |= st[form]["halves"]
    return got


def test_named_set_reaches_every_case():
    got = _reach()
    for key, value in got.items():
        print(f"reached {key}: {sorted(value)}")
    assert got["src1"] == {u.ROOT, u.CARRY, u.LDS0, u.LDS1, u.HBM} and got["dst1"] == {u.NONE, u.CARRY, u.LDS0, u.LDS1, u.HBM}
    assert got["reuse0"] and got["reuse1"], "no INTERNAL slot is written twice in one chunk"
    assert got["cut_carried"] and got["from_prev"], "no cut child was its parent's carried child with the parked one taking the registers"
    assert got["cut_parked"] and got["both_cut"] and got["right_carried0"]
    assert {31, 32, 33} <= got["ops"]
    assert got["cut_target"] and got["descended_target1"], "no cut subtree of exactly target ops beside one of target + 1"
    op_kinds, kinds = (u.CORE, u.DEEP), range(5)
    pairs = {(a, b) for a in kinds for b in kinds if a in op_kinds or b in op_kinds}
    assert got["pairs0"] >= pairs
    # streamed form: the child the next op takes in registers is made the left one -- an only child with an op is that child, and of
    # CORE beside DEEP it is the DEEP one (the smaller subtree: one op), so (no op, op) and (CORE, DEEP) cannot occur there
    unreachable1 = {(a, b) for a, b in pairs if a not in op_kinds} | {(u.CORE, u.DEEP)}
    assert got["pairs1"] >= pairs - unreachable1 and not got["pairs1"] & unreachable1
    halves = {(side, h, k) for side in (0, 1) for h in (0, 1) for k in (u.TIP, u.CHERRY, u.CHERRY_TIP)}
    assert got["halves0"] >= halves and got["halves1"] >= halves


def test_bench_tree_counts():
    tree = _tree(BENCH)
    zero, one = u.pre_order_schedule(tree, 0), u.pre_order_schedule(tree, 1)
    assert len(zero[0]) == len(one[0]) == 501 and zero[1] == one[1]
    moved = u.check_forms_agree(zero[0], one[0])
    assert moved["from_prev"] >= 1 and moved["slot1"] >= 1 and moved["swapped"] >= 1


def test_bad_arguments_are_reported():
    lib = _lib.load()
    assert lib.phyamd_abi_version() == 5  # an appended entry point: no signature changed
    tree = u.make_tree("balanced64")
    left, right = tree.left.copy(), tree.right.copy()
    call = lib.phyamd_pre_order_schedule
    assert call(1, left.ctypes.data, right.ctypes.data, 0, 0, None, 0, None) == _lib.EINVAL
    assert call(64, None, right.ctypes.data, 126, 0, None, 0, None) == _lib.EINVAL
    assert call(64, left.ctypes.data, right.ctypes.data, 126, 3, None, 0, None) == _lib.EINVAL
    assert b"form" in lib.phyamd_last_error()
    assert call(64, left.ctypes.data, right.ctypes.data, 126, 1, None, 5, None) == _lib.EINVAL
    assert call(64, left.ctypes.data, right.ctypes.data, 3, 1, None, 0, None) == _lib.EINVAL  # a tip is no root
    assert b"root" in lib.phyamd_last_error()
    for form in FORMS:
        assert call(64, left.ctypes.data, right.ctypes.data, 126, form, None, 0, None) == 31  # capacity 0: the count alone
    few = np.full((4, u.COLUMNS), -7, dtype=np.int32)
    assert call(64, left.ctypes.data, right.ctypes.data, 126, 1, few.ctypes.data, 3, None) == 31
    assert (few[:3] != -7).all() and (few[3] == -7).all()  # at most `capacity` records are written
