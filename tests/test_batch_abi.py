"""CPU-only: the batched evaluation's two entry points (phyamd_gradient_batch, phyamd_get_batch_profile) are declared, exported and
bound, refuse null arguments with a message, and every instantiation of the batched walk is in the built library's code object
without spilling registers (profiles/kernel_resources.py reads the code object; no GPU needed)."""
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
NAMES = ["phyamd_gradient_batch", "phyamd_get_batch_profile"]


def test_symbols_are_declared_exported_and_bound():
    from physher_amd import _lib
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "physher_amd.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    bound = [n for n, _, _ in _lib.SYMBOLS]
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(lib, name), name
        assert name in bound, name
    assert lib.phyamd_abi_version() == 5  # appended entry points: no signature changed


def test_null_arguments_are_refused_with_a_message():
    from physher_amd import _lib
    lib = _lib.load()
    lengths = (ctypes.c_double * 5)()
    lnl = (ctypes.c_double * 1)()
    assert lib.phyamd_gradient_batch(None, 0, 1, lengths, lnl, None) == _lib.EINVAL  # null handle
    assert b"null engine" in lib.phyamd_last_error()
    assert lib.phyamd_gradient_batch(None, 0, 1, None, lnl, None) == _lib.EINVAL  # null arrays
    assert b"null branch_lengths or lnl" in lib.phyamd_last_error()
    assert lib.phyamd_gradient_batch(None, 0, 1, lengths, None, None) == _lib.EINVAL
    assert b"null branch_lengths or lnl" in lib.phyamd_last_error()
    assert lib.phyamd_gradient_batch(None, 0, 0, lengths, lnl, None) == _lib.EINVAL
    assert b"count" in lib.phyamd_last_error()
    prof = _lib.BatchProfile()
    assert lib.phyamd_get_batch_profile(None, ctypes.byref(prof)) == _lib.EINVAL
    assert b"null" in lib.phyamd_last_error()


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(LIB) or not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("built library or llvm tools missing")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "profiles", "kernel_resources.py"), "k_batch_"], check=True, capture_output=True,
                         text=True).stdout
    return json.loads(out)["kernels"]


@pytest.mark.parametrize("name", ["k_batch_walk4<false>", "k_batch_walk4<true>", "k_batch_matrices", "k_batch_finish"])
def test_batch_kernels_spill_nothing(kernels, name):
    hits = [k for n, k in kernels.items() if n == name or n.startswith(name + "(")]
    assert len(hits) == 1, (name, sorted(kernels))
    k = hits[0]
    assert k["vgpr_spill_count"] == 0 and k["scratch_bytes"] == 0, k
