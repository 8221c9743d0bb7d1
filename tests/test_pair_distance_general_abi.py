"""CPU-only: phyamd_pairwise_distances_general -- the ML distance of pairs of taxa of a 20-state engine in one call -- is declared,
exported and bound without an ABI bump, refuses null arguments with a message before it looks at the handle's state, and its two
kernels are single code-object entries that spill nothing and use no scratch memory (profiles/kernel_resources.py reads the code
object; no GPU needed)."""
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
NAME = "phyamd_pairwise_distances_general"
PROFILE = "phyamd_get_distance_profile"


def test_symbol_is_declared_exported_and_bound():
    from physher_amd import _lib
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "physher_amd.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % NAME, text)
    assert m, "the signature is not in the header"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["phyamd_engine *e", "int flags", "int32_t count", "const int32_t *pairs", "const double *start", "double lower", "double upper", "double tolerance",
                      "int32_t max_iterations", "double *distances", "double *lnl", "double *d1", "double *d2", "int32_t *iterations", "double *counts",
                      "uint64_t *class_members"], params
    assert hasattr(lib, NAME) and hasattr(lib, PROFILE)
    bound = {n: args for n, _, args in _lib.SYMBOLS}
    assert NAME in bound and len(bound[NAME]) == 16
    assert len(bound["phyamd_pairwise_distances"]) == 15     # the 4-state call is as it was
    assert [n for n, _ in _lib.DistanceProfile._fields_] == ["pairs", "chunks", "segments", "scratch_bytes", "iterations", "ms"]
    assert ctypes.sizeof(_lib.DistanceProfile) == 40         # the struct is unchanged
    assert lib.phyamd_abi_version() == 5                     # appended entry point: no signature changed


def test_engine_and_seam_b_have_the_method():
    from physher_amd.engine import Engine
    assert callable(getattr(Engine, "pairwise_distances_general"))
    with open(os.path.join(ROOT, "include", "phycpp_amd", "physher.hpp")) as f:
        assert re.search(r"\bPairwiseDistancesGeneral\s*\(", f.read())
    from physher_amd import _phycpp_amd
    assert callable(getattr(_phycpp_amd.TreeLikelihoodInterface, "pairwise_distances_general"))
    from physher_amd import distances
    for fn in ("state_counts_general", "p_distance_general", "kimura_protein"):
        assert callable(getattr(distances, fn))


def test_null_arguments_are_refused_with_a_message():
    from physher_amd import _lib
    lib = _lib.load()
    fn = getattr(lib, NAME)
    out = (ctypes.c_double * 1024)()
    members = (ctypes.c_uint64 * 32)()
    assert fn(None, 0, 1, None, None, 1e-8, 10.0, 1e-8, 100, out, out, None, None, None, None, members) == _lib.EINVAL  # null handle
    msg = lib.phyamd_last_error()
    assert NAME.encode() in msg and b"null engine" in msg, msg
    assert fn(None, 0, 1, None, None, 1e-8, 10.0, 1e-8, 100, None, None, None, None, None, out, None) == _lib.EINVAL  # ... counting only
    assert b"null engine" in lib.phyamd_last_error()
    assert fn(None, 0, 1, None, None, 1e-8, 10.0, 1e-8, 100, None, None, None, None, None, None, members) == _lib.EINVAL
    msg = lib.phyamd_last_error()
    assert NAME.encode() in msg and b"null" in msg and b"distances" in msg and b"counts" in msg, msg
    it = (ctypes.c_int32 * 1)()
    for args, what in (((out, None, None, None), b"lnl"), ((None, out, None, None), b"d1"), ((None, None, out, None), b"d2"), ((None, None, None, it), b"iterations")):
        assert fn(None, 0, 1, None, None, 1e-8, 10.0, 1e-8, 100, None, *args, out, None) == _lib.EINVAL
        msg = lib.phyamd_last_error()
        assert NAME.encode() in msg and what in msg and b"without distances" in msg, msg


def _kernels(prefix):
    if not os.path.exists(LIB) or not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("built library or llvm tools missing")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "profiles", "kernel_resources.py"), prefix], check=True, capture_output=True,
                         text=True).stdout
    return json.loads(out)["kernels"]


def test_the_new_kernels_appear_once_and_spill_nothing():
    """k_classpair_counts holds four accumulator tiles for each of its partners: a spill would put them through scratch memory in
    the loop"""
    kernels = _kernels("k_classpair")
    assert sorted(kernels) == ["k_classpair_counts", "k_classpair_solve"], sorted(kernels)
    for name, k in kernels.items():
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["scratch_bytes"] == 0, (name, k)
    assert kernels["k_classpair_counts"]["vgpr_count"] <= 256 and kernels["k_classpair_counts"]["lds_static_bytes"] == 0
    assert kernels["k_classpair_solve"]["lds_static_bytes"] <= 16384
