"""CPU-only: phyamd_gradient_batch_trees -- lnL and the branch gradient of a batch of trees in one launch -- is declared, exported and
bound without an ABI bump, refuses null arguments with a message before it looks at the handle's state, and the four kernels of
the batched walk are still single code-object entries that spill nothing (profiles/kernel_resources.py reads the code object; no
GPU needed)."""
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
NAME = "phyamd_gradient_batch_trees"


def test_symbol_is_declared_exported_and_bound():
    from physher_amd import _lib
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "physher_amd.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert re.search(r"\b%s\s*\(" % NAME, text)
    assert hasattr(lib, NAME)
    bound = {n: args for n, _, args in _lib.SYMBOLS}
    assert NAME in bound and len(bound[NAME]) == 9
    assert lib.phyamd_abi_version() == 5  # an appended entry point: no signature changed


def test_engine_has_the_method():
    from physher_amd.engine import Engine
    assert callable(getattr(Engine, "gradient_batch_trees"))


def test_null_arguments_are_refused_with_a_message():
    from physher_amd import _lib
    lib = _lib.load()
    fn = lib.phyamd_gradient_batch_trees
    left, right = (ctypes.c_int32 * 3)(-1, -1, 0), (ctypes.c_int32 * 3)(-1, -1, 1)
    roots = (ctypes.c_int32 * 1)(2)
    lengths = (ctypes.c_double * 3)()
    lnl = (ctypes.c_double * 1)()
    assert fn(None, 0, 1, left, right, roots, lengths, lnl, None) == _lib.EINVAL  # null handle
    assert b"null engine" in lib.phyamd_last_error()
    good = [left, right, roots, lengths, lnl]
    for i, what in enumerate(["left", "right", "roots", "branch_lengths", "lnl"]):
        args = list(good)
        args[i] = None
        assert fn(None, 0, 1, *args, None) == _lib.EINVAL, what
        msg = lib.phyamd_last_error()
        assert b"phyamd_gradient_batch_trees" in msg and b"null" in msg and what.encode() in msg, (what, msg)
    for count in (0, -3):
        assert fn(None, 0, count, *good, None) == _lib.EINVAL
        assert b"count" in lib.phyamd_last_error()


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(LIB) or not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("built library or llvm tools missing")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "profiles", "kernel_resources.py"), "k_batch_"], check=True, capture_output=True,
                         text=True).stdout
    return json.loads(out)["kernels"]


@pytest.mark.parametrize("name", ["k_batch_walk4<false>", "k_batch_walk4<true>", "k_batch_matrices", "k_batch_finish"])
def test_batch_kernels_appear_once_and_spill_nothing(kernels, name):
    """per-item op lists and roots are launch arguments, not new instantiations or overloads"""
    hits = [k for n, k in kernels.items() if n == name or n.startswith(name + "(")]
    assert len(hits) == 1, (name, sorted(kernels))
    assert len(kernels) == 4, sorted(kernels)
    k = hits[0]
    assert k["vgpr_spill_count"] == 0 and k["scratch_bytes"] == 0, k
