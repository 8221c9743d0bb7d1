"""CPU-only: phyamd_optimize_branch_lengths -- every branch length of a batch of trees optimised in one call -- and its profile are
declared, exported and bound without an ABI bump; Engine, the seam-B header and the pybind module have the method; null arguments
are refused with the function's and the argument's name before the handle's state is looked at; and its kernels are single
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
NAME = "phyamd_optimize_branch_lengths"
PROFILE = "phyamd_get_branch_optimize_profile"
SCHEDULE = "phyamd_branch_sweep_schedule"


def test_symbols_are_declared_exported_and_bound():
    from physher_amd import _lib
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "physher_amd.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    bound = {n: args for n, _, args in _lib.SYMBOLS}
    for name in (NAME, PROFILE, SCHEDULE):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(lib, name) and name in bound, name
    assert len(bound[NAME]) == 18 and len(bound[SCHEDULE]) == 6
    assert re.search(r"int32_t items, chunks, passes; int64_t visits, iterations, scratch_bytes; double ms;\s*}\s*phyamd_branch_optimize_profile", text)
    assert [k for k, _ in _lib.BranchOptimizeProfile._fields_] == ["items", "chunks", "passes", "visits", "iterations", "scratch_bytes", "ms"]
    assert lib.phyamd_abi_version() == 5  # appended entry points: no signature changed


def test_engine_and_seam_b_have_the_method():
    from physher_amd.engine import Engine
    assert callable(getattr(Engine, "optimize_branch_lengths"))
    assert callable(getattr(Engine, "branch_optimize_profile"))
    with open(os.path.join(ROOT, "include", "phycpp_amd", "physher.hpp")) as f:
        assert re.search(r"\bOptimizeBranchLengths\s*\(", f.read())
    from physher_amd import _phycpp_amd
    assert callable(getattr(_phycpp_amd.TreeLikelihoodInterface, "optimize_branch_lengths"))


def _call(lib, engine=None, count=1, trees=(None, None, None), start=True, lengths=True, lnl=True, lower=1e-8, upper=10.0, tolerance=1e-8, max_iterations=100,
          lnl_tolerance=1e-6, max_passes=50):
    buf = (ctypes.c_double * 9)()
    ids = (ctypes.c_int32 * 9)()
    left, right, roots = (ids if t else None for t in trees)
    return getattr(lib, NAME)(engine, 0, count, left, right, roots, buf if start else None, None, lower, upper, tolerance, max_iterations, lnl_tolerance, max_passes,
                              buf if lengths else None, buf if lnl else None, None, None)


def test_arguments_are_refused_by_name_before_the_handle_is_looked_at():
    from physher_amd import _lib
    lib = _lib.load()

    def refused(what, **kw):
        assert _call(lib, **kw) == _lib.EINVAL, what
        msg = lib.phyamd_last_error()
        assert NAME.encode() in msg and what in msg, msg
    refused(b"null engine")
    refused(b"null branch_lengths", start=False)
    refused(b"null lengths", lengths=False)
    refused(b"null lnl", lnl=False)
    refused(b"null right", trees=(True, False, True))
    refused(b"null left", trees=(False, True, True))
    refused(b"null roots", trees=(True, True, False))
    refused(b"count", count=0)
    assert getattr(lib, PROFILE)(None, None) == _lib.EINVAL
    assert b"null engine" in lib.phyamd_last_error()


def _kernels(prefix):
    if not os.path.exists(LIB) or not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("built library or llvm tools missing")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "profiles", "kernel_resources.py"), prefix], check=True, capture_output=True,
                         text=True).stdout
    return json.loads(out)["kernels"]


def test_the_new_kernels_appear_once_and_spill_nothing():
    kernels = _kernels("k_blopt")
    assert len(kernels) == 2, sorted(kernels)
    for name in ("k_blopt_step4", "k_blopt_solve4"):
        hits = [k for n, k in kernels.items() if n == name or n.startswith(name + "(")]
        assert len(hits) == 1, (name, sorted(kernels))
        assert hits[0]["vgpr_spill_count"] == 0 and hits[0]["sgpr_spill_count"] == 0 and hits[0]["scratch_bytes"] == 0, (name, hits[0])
