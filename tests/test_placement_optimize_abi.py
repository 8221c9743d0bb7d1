"""CPU-only: phyamd_placement_optimize -- the three branches around chosen placements optimised in one call -- is declared, exported
and bound without an ABI bump, refuses null arguments and bad values with a message that names the function and the argument
before it looks at the handle, and its kernels are single code-object entries that spill nothing and use no scratch memory
(profiles/kernel_resources.py reads the code object; no GPU needed)."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "physher_amd", "libphysher_amd.so")
LLVM = "/opt/rocm/lib/llvm/bin"
NAME = "phyamd_placement_optimize"
PROFILE = "phyamd_get_placement_optimize_profile"


def test_symbols_are_declared_exported_and_bound():
    from physher_amd import _lib
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "physher_amd.h")) as f:
        raw = f.read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"\b%s\s*\(" % NAME, text) and re.search(r"\b%s\s*\(" % PROFILE, text)
    assert re.search(r"typedef struct \{ int32_t candidates, edges, chunks; int64_t visits, iterations, scratch_bytes; double ms; \} phyamd_placement_optimize_profile;", text)
    assert text.index(NAME) > text.index("phyamd_get_placement_profile")  # appended
    assert hasattr(lib, NAME) and hasattr(lib, PROFILE)
    bound = {n: args for n, _, args in _lib.SYMBOLS}
    assert NAME in bound and len(bound[NAME]) == 19
    assert PROFILE in bound
    assert ctypes.sizeof(_lib.PlacementOptimizeProfile) == 48  # three int32, padding, three int64 and a double
    assert lib.phyamd_abi_version() == 5  # appended entry points: no signature changed


def test_the_header_states_the_rule():
    with open(os.path.join(ROOT, "include", "physher_amd.h")) as f:
        raw = f.read()
    doc = raw[raw.index("/* --- the three branches around chosen placements --- */"):raw.index("int phyamd_placement_optimize(")]
    doc = re.sub(r"\s*\n \* ?", " ", doc)  # (the comment's line breaks)
    for words in ("phyamd_optimize_branch_lengths returns for ONE item", "order n, x, z", "phyamd_spr_optimize's", "bit for bit", "branches = 7", "branches = 2",
                  "PHYAMD_EUNSUPPORTED", "PHYAMD_EINVAL", "pendant_start NULL: 0.1", "Duplicates"):
        assert words in doc, words
    assert "t' = t - d1 / d2" not in doc  # phyamd_spr_optimize's text is referred to, not repeated


def test_the_wrappers_exist():
    from physher_amd.engine import Engine
    from physher_amd import placement
    assert callable(getattr(Engine, "placement_optimize")) and callable(getattr(Engine, "placement_optimize_profile"))
    assert callable(placement.top_candidates)
    with open(os.path.join(ROOT, "include", "phycpp_amd", "physher.hpp")) as f:
        assert re.search(r"\bvoid PlacementOptimize\(", f.read())
    from physher_amd import _phycpp_amd as pc
    assert hasattr(pc.TreeLikelihoodInterface, "placement_optimize")


def test_top_candidates_and_sparse_weight_ratios():
    from physher_amd.placement import likelihood_weight_ratios, top_candidates
    lnl = np.array([[1.0, np.nan, 3.0, 3.0, 0.0], [5.0, np.nan, 5.0, 1.0, 2.0], [-np.inf, np.nan, -7.0, -np.inf, -np.inf]])
    got = top_candidates(lnl, 2)
    assert got.dtype == np.int32 and got.tolist() == [[0, 2], [0, 3], [1, 0], [1, 2], [2, 2], [2, 0]]  # ties: the smaller id; never the root's NaN column
    assert top_candidates(lnl, 9).shape == (12, 2) and 1 not in top_candidates(lnl, 9)[:, 1]
    assert top_candidates(np.array([3, 0, 2], dtype=np.int32), 1).tolist() == [[0, 3], [1, 0], [2, 2]]
    with pytest.raises(ValueError):
        top_candidates(lnl, 0)
    cands = top_candidates(lnl[:2], 3)
    sparse = lnl[cands[:, 0], cands[:, 1]]
    perm = np.random.default_rng(0).permutation(len(cands))
    w = likelihood_weight_ratios(sparse[perm], cands[perm, 0])
    for q in (0, 1):
        mine = cands[perm, 0] == q
        assert abs(w[mine].sum() - 1.0) < 1e-15
        dense = np.full(5, np.nan)
        dense[cands[perm, 1][mine]] = sparse[perm][mine]
        assert np.allclose(w[mine], likelihood_weight_ratios(dense)[cands[perm, 1][mine]], rtol=0, atol=1e-15)  # (the same three terms added in another order: a few ulps of 1)
    assert np.array_equal(likelihood_weight_ratios(np.array([-np.inf, -3.0]), np.array([4, 4])), [0.0, 1.0])


def test_null_arguments_and_bad_values_are_refused_with_a_message():
    from physher_amd import _lib
    lib = _lib.load()
    fn = getattr(lib, NAME)
    masks = (ctypes.c_uint8 * 8)(*([1] * 8))
    cands = (ctypes.c_int32 * 4)(0, 1, 1, 0)
    start = (ctypes.c_double * 2)(0.1, 0.2)
    lengths, lnl, lnl0 = (ctypes.c_double * 6)(), (ctypes.c_double * 2)(), (ctypes.c_double * 2)()
    passes = (ctypes.c_int32 * 2)()
    good = dict(e=None, flags=0, queries=2, masks=masks, count=2, candidates=cands, start=start, split=0.5, branches=7, lower=1e-8, upper=10.0, tolerance=1e-8,
                max_iterations=100, lnl_tolerance=1e-6, max_passes=50, lengths=lengths, lnl=lnl, initial=lnl0, passes=passes)

    def refused(**kw):
        args = dict(good, **kw)
        assert fn(*args.values()) == _lib.EINVAL
        msg = lib.phyamd_last_error()
        assert NAME.encode() in msg, msg
        return msg

    assert b"null engine" in refused()  # everything else is in order
    assert b"null engine" in refused(start=None, initial=None, passes=None)
    for arg in ("masks", "candidates", "lengths", "lnl"):
        assert b"null " + arg.encode() in refused(**{arg: None})
    for count in (0, -2):
        assert b"queries" in refused(queries=count)
        assert b"count" in refused(count=count)
    for q in (-1, 2):
        msg = refused(candidates=(ctypes.c_int32 * 4)(0, 1, q, 0))
        assert b"candidates[1]" in msg and b"query" in msg
    for branches in (0, 8, -1):
        assert b"branches" in refused(branches=branches)
    for split in (-0.01, 1.01, float("nan"), float("inf")):
        assert b"split" in refused(split=split)
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        assert b"pendant_start[1]" in refused(start=(ctypes.c_double * 2)(0.1, bad))
    for lower, upper in ((-1e-9, 10.0), (1.0, 1.0), (0.0, float("inf")), (float("nan"), 1.0)):
        assert b"bounds" in refused(lower=lower, upper=upper)
    for tolerance in (0.0, -1.0, float("nan"), float("inf")):
        assert b" tolerance" in refused(tolerance=tolerance)
    for n in (0, 1001):
        assert b"max_iterations" in refused(max_iterations=n)
        assert b"max_passes" in refused(max_passes=n)
    for tolerance in (-1e-9, float("nan"), float("inf")):
        assert b"lnl_tolerance" in refused(lnl_tolerance=tolerance)
    assert getattr(lib, PROFILE)(None, None) == _lib.EINVAL
    assert b"null engine" in lib.phyamd_last_error()


def _kernels(prefix):
    if not os.path.exists(LIB) or not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("built library or llvm tools missing")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "profiles", "kernel_resources.py"), prefix], check=True, capture_output=True,
                         text=True).stdout
    return json.loads(out)["kernels"]


def test_qopt_kernels_appear_once_and_spill_nothing():
    kernels = _kernels("k_qopt")
    assert len(kernels) == 2, sorted(kernels)
    for name in ("k_qopt_upper4", "k_qopt_solve4"):
        hits = [k for n, k in kernels.items() if n == name or n.startswith(name + "(")]
        assert len(hits) == 1, (name, sorted(kernels))
        assert hits[0]["vgpr_spill_count"] == 0 and hits[0]["sgpr_spill_count"] == 0 and hits[0]["scratch_bytes"] == 0, (name, hits[0])
