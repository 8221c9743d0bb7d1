#!/usr/bin/env python3
"""Where the stored children of the streamed post-order walk come from, counted on the host schedule (no GPU):
phyamd_post_order_parks for a tree, with the second park slot off and on.

A stored child read from memory is one node plane (C x P x 4 doubles: 128 MB at the headline shape) fetched per evaluation.
Classes of the memory sources of the one-slot schedule: beside a cut (the child is the root of a cut subtree, written by another
workgroup: stays), second tier (the two-slot schedule takes it from slot 1), deeper (stays).

usage: lower_park_count.py [taxa] [seed]      (default: the bench tree, 1000 taxa, seed 1)
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from physher_amd import _lib, synth  # noqa: E402

PLANE_GB = 1e6 * 4 * 4 * 8 / 1e9  # the headline shape: 1e6 patterns x 4 categories x 4 states, doubles
MS_PER_GB = 0.37                  # what a GB read beside the store stream costs the pass


def parks(left, right, root, second_slot):
    lib = _lib.load()
    left = np.ascontiguousarray(left, dtype=np.int32)
    right = np.ascontiguousarray(right, dtype=np.int32)
    T = (len(left) + 1) // 2
    out = np.zeros((T, 8), dtype=np.int32)
    n = lib.phyamd_post_order_parks(T, left.ctypes.data, right.ctypes.data, int(root), int(second_slot), out.ctypes.data, T)
    if n < 0:
        raise RuntimeError(lib.phyamd_last_error().decode())
    return out[:n]


def count(left, right, root):
    one, two = parks(left, right, root, 0), parks(left, right, root, 1)
    assert (one[:, :4] == two[:, :4]).all()  # same ops in the same order
    res = {"ops": int(len(one)), "chunks": int(one[-1, 0]) + 1, "memory_one_slot": 0, "beside_cut": 0, "second_tier": 0, "deeper": 0,
           "slot0": 0, "carried": 0}
    for a, b in zip(one, two):
        for side in (0, 1):
            s1, s2 = int(a[4 + side]), int(b[4 + side])
            res["slot0"] += s2 == 2
            res["carried"] += s2 == 1
            if s1 != 0:
                continue
            res["memory_one_slot"] += 1
            if a[7] & (1 << side):
                assert s2 == 0
                res["beside_cut"] += 1
            elif s2 == 3:
                res["second_tier"] += 1
            else:
                assert s2 == 0
                res["deeper"] += 1
    res["memory_two_slots"] = res["beside_cut"] + res["deeper"]
    res["removed_gb"] = round(res["second_tier"] * PLANE_GB, 3)
    res["expected_gain_ms"] = round(res["second_tier"] * PLANE_GB * MS_PER_GB, 3)
    return res


def main():
    taxa = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    tree = synth.random_tree(taxa, np.random.default_rng(seed))
    res = {"taxa": taxa, "seed": seed}
    res.update(count(tree.left, tree.right, tree.root))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
