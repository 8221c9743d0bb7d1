"""CPU-only: phyamd_branch_hessian -- the full branch-length Hessian of lnL in one call -- and phyamd_get_hessian_profile are
declared, exported and bound without an ABI bump, refuse null arguments with a message that names the function and the argument
before they look at the handle's state, every k_bhess* kernel spills nothing and uses no scratch, and the batched walk still has
exactly its four kernels (profiles/kernel_resources.py reads the code object; no GPU needed)."""
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
NAMES = {"phyamd_branch_hessian": 5, "phyamd_get_hessian_profile": 2}
KERNELS = ("k_bhess_matrices", "k_bhess_site", "k_bhess_walk", "k_bhess_cousins", "k_bhess_outer", "k_bhess_finish")


def test_symbols_are_declared_exported_and_bound():
    from physher_amd import _lib
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "physher_amd.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    bound = {n: args for n, _, args in _lib.SYMBOLS}
    for name, nargs in NAMES.items():
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(lib, name), name
        assert name in bound and len(bound[name]) == nargs, name
    assert lib.phyamd_abi_version() == 5  # appended entry points: no signature changed


def test_engine_has_the_methods():
    from physher_amd.engine import Engine
    assert callable(getattr(Engine, "branch_hessian"))
    assert callable(getattr(Engine, "hessian_profile"))


def test_null_arguments_are_refused_with_a_message():
    from physher_amd import _lib
    lib = _lib.load()
    fn = lib.phyamd_branch_hessian
    lnl = ctypes.c_double()
    out = (ctypes.c_double * 9)()
    assert fn(None, 0, ctypes.byref(lnl), None, out) == _lib.EINVAL  # null handle
    msg = lib.phyamd_last_error()
    assert b"phyamd_branch_hessian" in msg and b"null engine" in msg, msg
    assert fn(None, 0, None, None, out) == _lib.EINVAL  # null lnl: the arguments are looked at before the handle
    msg = lib.phyamd_last_error()
    assert b"phyamd_branch_hessian" in msg and b"null" in msg and b"lnl" in msg, msg
    assert fn(None, 0, ctypes.byref(lnl), out, None) == _lib.EINVAL  # null hessian
    msg = lib.phyamd_last_error()
    assert b"phyamd_branch_hessian" in msg and b"null" in msg and b"hessian" in msg, msg
    assert lib.phyamd_get_hessian_profile(None, None) == _lib.EINVAL
    assert b"null engine" in lib.phyamd_last_error()


def _kernels(prefix):
    if not os.path.exists(LIB) or not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("built library or llvm tools missing")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "profiles", "kernel_resources.py"), prefix], check=True, capture_output=True,
                         text=True).stdout
    return json.loads(out)["kernels"]


def test_hessian_kernels_appear_once_and_spill_nothing():
    kernels = _kernels("k_bhess")
    assert len(kernels) == len(KERNELS), sorted(kernels)
    for name in KERNELS:
        hits = [k for n, k in kernels.items() if n == name or n.startswith(name + "(")]
        assert len(hits) == 1, (name, sorted(kernels))
        assert hits[0]["vgpr_spill_count"] == 0 and hits[0]["sgpr_spill_count"] == 0 and hits[0]["scratch_bytes"] == 0, (name, hits[0])


def test_the_batched_walk_still_has_its_four_kernels():
    kernels = _kernels("k_batch_")
    names = sorted(n.split("(")[0] for n in kernels)
    assert names == ["k_batch_finish", "k_batch_matrices", "k_batch_walk4<false>", "k_batch_walk4<true>"], sorted(kernels)
