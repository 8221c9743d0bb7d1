"""CPU-only: phyamd_pairwise_distances -- the ML distance of pairs of taxa in one call -- is declared, exported and bound without an
ABI bump, refuses null arguments with a message before it looks at the handle's state, and its three kernels are single
code-object entries that spill nothing and use no scratch memory (profiles/kernel_resources.py reads the code object; no GPU
needed)."""
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
NAME = "phyamd_pairwise_distances"
PROFILE = "phyamd_get_distance_profile"


def test_symbol_is_declared_exported_and_bound():
    from physher_amd import _lib
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "physher_amd.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert re.search(r"\b%s\s*\(" % NAME, text)
    assert re.search(r"\b%s\s*\(" % PROFILE, text)
    assert re.search(r"\bphyamd_distance_profile\b", text)
    assert hasattr(lib, NAME) and hasattr(lib, PROFILE)
    bound = {n: args for n, _, args in _lib.SYMBOLS}
    assert NAME in bound and len(bound[NAME]) == 15
    assert PROFILE in bound
    assert [n for n, _ in _lib.DistanceProfile._fields_] == ["pairs", "chunks", "segments", "scratch_bytes", "iterations", "ms"]
    assert ctypes.sizeof(_lib.DistanceProfile) == 40
    assert lib.phyamd_abi_version() == 5  # appended entry points: no signature changed


def test_engine_and_seam_b_have_the_method():
    from physher_amd.engine import Engine
    assert callable(getattr(Engine, "pairwise_distances"))
    assert callable(getattr(Engine, "distance_profile"))
    with open(os.path.join(ROOT, "include", "phycpp_amd", "physher.hpp")) as f:
        assert re.search(r"\bPairwiseDistances\s*\(", f.read())
    from physher_amd import _phycpp_amd
    assert callable(getattr(_phycpp_amd.TreeLikelihoodInterface, "pairwise_distances"))
    from physher_amd import distances
    for fn in ("square", "p_distance", "jc69", "k2p"):
        assert callable(getattr(distances, fn))


def test_null_arguments_are_refused_with_a_message():
    from physher_amd import _lib
    lib = _lib.load()
    fn = getattr(lib, NAME)
    out = (ctypes.c_double * 256)()
    assert fn(None, 0, 1, None, None, 1e-8, 10.0, 1e-8, 100, out, out, None, None, None, None) == _lib.EINVAL  # null handle
    msg = lib.phyamd_last_error()
    assert NAME.encode() in msg and b"null engine" in msg, msg
    assert fn(None, 0, 1, None, None, 1e-8, 10.0, 1e-8, 100, None, None, None, None, None, out) == _lib.EINVAL  # ... counting only
    assert b"null engine" in lib.phyamd_last_error()
    assert fn(None, 0, 1, None, None, 1e-8, 10.0, 1e-8, 100, None, None, None, None, None, None) == _lib.EINVAL
    msg = lib.phyamd_last_error()
    assert NAME.encode() in msg and b"null" in msg and b"distances" in msg and b"counts" in msg, msg
    it = (ctypes.c_int32 * 1)()
    for args, what in (((out, None, None, None), b"lnl"), ((None, out, None, None), b"d1"), ((None, None, out, None), b"d2"), ((None, None, None, it), b"iterations")):
        assert fn(None, 0, 1, None, None, 1e-8, 10.0, 1e-8, 100, None, *args, out) == _lib.EINVAL
        msg = lib.phyamd_last_error()
        assert NAME.encode() in msg and what in msg and b"without distances" in msg, msg
    assert getattr(lib, PROFILE)(None, None) == _lib.EINVAL
    assert b"null engine" in lib.phyamd_last_error()


def _kernels(prefix):
    if not os.path.exists(LIB) or not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("built library or llvm tools missing")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "profiles", "kernel_resources.py"), prefix], check=True, capture_output=True,
                         text=True).stdout
    return json.loads(out)["kernels"]


def test_the_new_kernels_appear_once_and_spill_nothing():
    kernels = _kernels("k_pairdist")
    assert len(kernels) == 3, sorted(kernels)
    for name in ("k_pairdist_counts4", "k_pairdist_finish", "k_pairdist_solve4"):
        hits = [k for n, k in kernels.items() if n == name or n.startswith(name + "(")]
        assert len(hits) == 1, (name, sorted(kernels))
        assert hits[0]["vgpr_spill_count"] == 0 and hits[0]["sgpr_spill_count"] == 0 and hits[0]["scratch_bytes"] == 0, (name, hits[0])
