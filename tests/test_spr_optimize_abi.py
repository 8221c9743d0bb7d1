"""CPU-only: phyamd_spr_optimize -- the three graft branches of every SPR regraft optimised in one call -- is declared, exported and
bound without an ABI bump, refuses null and out-of-range arguments with a message before it looks at the handle's state, its three
kernels are single code-object entries that spill nothing and use no scratch memory, and the SPR call's family keeps its three
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
NAME = "phyamd_spr_optimize"
PROFILE = "phyamd_get_spr_optimize_profile"


def test_symbol_is_declared_exported_and_bound():
    from physher_amd import _lib
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "physher_amd.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert re.search(r"\b%s\s*\(" % NAME, text)
    assert re.search(r"\b%s\s*\(" % PROFILE, text)
    assert re.search(r"\bphyamd_spr_optimize_profile\s*;", text)
    assert hasattr(lib, NAME) and hasattr(lib, PROFILE)
    bound = {n: args for n, _, args in _lib.SYMBOLS}
    assert NAME in bound and len(bound[NAME]) == 14
    assert PROFILE in bound
    assert [k for k, _ in _lib.SprOptimizeProfile._fields_] == ["prunes", "chunks", "candidates", "visits", "iterations", "scratch_bytes", "ms"]
    assert lib.phyamd_abi_version() == 5  # appended entry points: no signature changed


def test_engine_and_seam_b_have_the_method():
    from physher_amd.engine import Engine
    assert callable(getattr(Engine, "spr_optimize"))
    assert callable(getattr(Engine, "spr_optimize_profile"))
    with open(os.path.join(ROOT, "include", "phycpp_amd", "physher.hpp")) as f:
        assert re.search(r"\bSPROptimize\s*\(", f.read())
    from physher_amd import _phycpp_amd
    assert callable(getattr(_phycpp_amd.TreeLikelihoodInterface, "spr_optimize"))


def _call(lib, handle=None, count=5, lengths=True, lnl=True, lower=1e-8, upper=10.0, tolerance=1e-8, max_iterations=100, lnl_tolerance=1e-6, max_passes=50):
    out = (ctypes.c_double * 75)()
    return getattr(lib, NAME)(handle, 0, count, None, lower, upper, tolerance, max_iterations, lnl_tolerance, max_passes, out if lengths else None,
                              out if lnl else None, None, None)


def test_null_arguments_are_refused_with_a_message():
    from physher_amd import _lib
    lib = _lib.load()
    assert _call(lib) == _lib.EINVAL  # null handle
    assert b"null engine" in lib.phyamd_last_error()
    for kw, what in (({"lengths": False}, b"lengths"), ({"lnl": False}, b"lnl")):
        assert _call(lib, **kw) == _lib.EINVAL
        msg = lib.phyamd_last_error()
        assert NAME.encode() in msg and b"null" in msg and what in msg, msg
    assert _call(lib, count=0) == _lib.EINVAL
    assert NAME.encode() in lib.phyamd_last_error() and b"count" in lib.phyamd_last_error()
    assert getattr(lib, PROFILE)(None, None) == _lib.EINVAL
    assert b"null engine" in lib.phyamd_last_error()


def _kernels(prefix):
    if not os.path.exists(LIB) or not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("built library or llvm tools missing")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "profiles", "kernel_resources.py"), prefix], check=True, capture_output=True,
                         text=True).stdout
    return json.loads(out)["kernels"]


def test_the_new_kernels_appear_once_and_spill_nothing():
    kernels = _kernels("k_tripod")
    assert len(kernels) == 3, sorted(kernels)
    for name in ("k_tripod_upper4", "k_tripod_solve4", "k_tripod_finish"):
        hits = [k for n, k in kernels.items() if n == name or n.startswith(name + "(")]
        assert len(hits) == 1, (name, sorted(kernels))
        assert hits[0]["vgpr_spill_count"] == 0 and hits[0]["sgpr_spill_count"] == 0 and hits[0]["scratch_bytes"] == 0, (name, hits[0])


def test_the_spr_family_keeps_its_three_kernels():
    """the walk of the call is k_spr_walk4 itself: no new kernel of the family"""
    assert sorted(n.split("(")[0] for n in _kernels("k_spr")) == ["k_spr4", "k_spr_finish", "k_spr_walk4"]
