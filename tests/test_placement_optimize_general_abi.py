"""CPU-only: phyamd_placement_optimize_general -- the three branches around chosen placements of a 20-state engine optimised in one
call -- is declared, exported and bound without an ABI bump, its header states the rule in full, it refuses null arguments and bad
values with a message that names the function and the argument before it looks at the handle, and its solve kernel is a single
code-object entry that spills no vector register, uses no scratch memory and stays under 64 KB of static LDS
(profiles/kernel_resources.py reads the code object; no GPU needed)."""
import ctypes
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "physher_amd", "libphysher_amd.so")
LLVM = "/opt/rocm/lib/llvm/bin"
NAME = "phyamd_placement_optimize_general"
PROFILE = "phyamd_get_placement_optimize_profile"


def test_the_symbol_is_declared_exported_and_bound():
    from physher_amd import _lib
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "physher_amd.h")) as f:
        raw = f.read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"\b%s\s*\(" % NAME, text)
    assert text.index(NAME) > text.index("phyamd_placement_log_likelihoods_general")  # appended
    assert hasattr(lib, NAME) and hasattr(lib, PROFILE)
    bound = {n: args for n, _, args in _lib.SYMBOLS}
    assert NAME in bound and len(bound[NAME]) == 21
    assert lib.phyamd_abi_version() == 5  # an appended entry point: no signature changed


def test_the_header_states_the_rule_in_full():
    with open(os.path.join(ROOT, "include", "physher_amd.h")) as f:
        raw = f.read()
    doc = raw[raw.index("/* --- the three branches around chosen placements, 20 states --- */"):raw.index("int %s(" % NAME)]
    doc = re.sub(r"\s*\n \* ?", " ", doc)  # (the comment's line breaks)
    for words in ("T + 1 tips", "left child n and the right child x", "split t_n", "pendant_start NULL: 0.1", "(1 - split) t_n", "order n, x, z", "[lower, upper]",
                  "t - d1 / d2", "midpoint", "finite and not below", "passes = k", "-max_passes", "IN BAND", "bit for bit", "Duplicates", "|V e^(lambda t r_c) V^-1|",
                  "21 + q", "set_count <= 11", "phyamd_set_keep_partials(1)", "PHYAMD_EUNSUPPORTED", "PHYAMD_EINVAL", "use phyamd_placement_optimize", "not built",
                  "PHYAMD_RESCALE_AUTO", "no fallback"):
        assert words in doc, words


def test_the_wrappers_exist():
    from physher_amd.engine import Engine
    assert callable(getattr(Engine, "placement_optimize_general"))
    with open(os.path.join(ROOT, "include", "phycpp_amd", "physher.hpp")) as f:
        assert re.search(r"\bvoid PlacementOptimizeGeneral\(", f.read())
    from physher_amd import _phycpp_amd as pc
    assert hasattr(pc.TreeLikelihoodInterface, "placement_optimize_general")


def test_null_arguments_and_bad_values_are_refused_with_a_message():
    from physher_amd import _lib
    lib = _lib.load()
    fn = getattr(lib, NAME)
    codes = (ctypes.c_uint8 * 8)(*([1] * 8))
    sets = (ctypes.c_uint64 * 2)(3, 5)
    cands = (ctypes.c_int32 * 4)(0, 1, 1, 0)
    start = (ctypes.c_double * 2)(0.1, 0.2)
    lengths, lnl, lnl0 = (ctypes.c_double * 6)(), (ctypes.c_double * 2)(), (ctypes.c_double * 2)()
    passes = (ctypes.c_int32 * 2)()
    good = dict(e=None, flags=0, queries=2, codes=codes, set_count=2, sets=sets, count=2, candidates=cands, start=start, split=0.5, branches=7, lower=1e-8, upper=10.0,
                tolerance=1e-8, max_iterations=100, lnl_tolerance=1e-6, max_passes=50, lengths=lengths, lnl=lnl, initial=lnl0, passes=passes)

    def refused(**kw):
        args = dict(good, **kw)
        assert fn(*args.values()) == _lib.EINVAL
        msg = lib.phyamd_last_error()
        assert NAME.encode() in msg, msg
        return msg

    assert b"null engine" in refused()  # everything else is in order
    assert b"null engine" in refused(start=None, initial=None, passes=None, set_count=0, sets=None)
    for arg in ("codes", "candidates", "lengths", "lnl"):
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
    for n in (-1, 12):
        assert b"set_count" in refused(set_count=n)
    assert b"null sets" in refused(sets=None)
    for word in (0, 1 << 20):
        assert b"sets[1]" in refused(sets=(ctypes.c_uint64 * 2)(3, word))


def _kernels(prefix):
    if not os.path.exists(LIB) or not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("built library or llvm tools missing")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "profiles", "kernel_resources.py"), prefix], check=True, capture_output=True,
                         text=True).stdout
    return json.loads(out)["kernels"]


def test_the_solve_kernel_appears_once_spills_nothing_and_fits_the_lds():
    kernels = _kernels("k_classopt")
    hits = [k for n, k in kernels.items() if n == "k_classopt_solve" or n.startswith("k_classopt_solve(")]
    assert len(hits) == 1 and len(kernels) == 1, sorted(kernels)
    k = hits[0]
    print(k)
    assert k["vgpr_spill_count"] == 0 and k["scratch_bytes"] == 0, k
    assert 0 < k["lds_static_bytes"] < 64 * 1024, k
