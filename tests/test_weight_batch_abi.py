"""CPU-only: the weight batch's two entry points (phyamd_gradient_batch_weights, phyamd_get_weight_batch_profile) are declared,
exported and bound, refuse null arguments and a bad count with a message that names the function and the argument, and the
kernels of the shared-lengths path are in the built library's code object, once each, without spilling registers
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
NAMES = ["phyamd_gradient_batch_weights", "phyamd_get_weight_batch_profile"]


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
    fields = [n for n, _ in _lib.WeightBatchProfile._fields_]
    assert fields == ["items_fast", "items_sequential", "item_chunks", "pattern_chunks", "walks", "scratch_bytes", "ms"]
    assert ctypes.sizeof(_lib.WeightBatchProfile) == 40  # five int32, padding, int64, double
    from physher_amd.engine import Engine
    assert hasattr(Engine, "gradient_batch_weights") and hasattr(Engine, "weight_batch_profile")


def test_null_arguments_and_a_bad_count_are_refused_with_a_message():
    from physher_amd import _lib
    lib = _lib.load()
    fn = lib.phyamd_gradient_batch_weights
    weights = (ctypes.c_double * 5)()
    lnl = (ctypes.c_double * 1)()
    assert fn(None, 0, 1, weights, None, lnl, None) == _lib.EINVAL  # null handle
    assert b"phyamd_gradient_batch_weights: null engine" in lib.phyamd_last_error()
    assert fn(None, 0, 1, None, None, lnl, None) == _lib.EINVAL
    assert b"phyamd_gradient_batch_weights: null weights" in lib.phyamd_last_error()
    assert fn(None, 0, 1, weights, None, None, None) == _lib.EINVAL
    assert b"phyamd_gradient_batch_weights: null lnl" in lib.phyamd_last_error()
    for count in (0, -3):
        assert fn(None, 0, count, weights, None, lnl, None) == _lib.EINVAL
        msg = lib.phyamd_last_error()
        assert b"phyamd_gradient_batch_weights: count" in msg and str(count).encode() in msg, msg
    prof = _lib.WeightBatchProfile()
    assert lib.phyamd_get_weight_batch_profile(None, ctypes.byref(prof)) == _lib.EINVAL
    assert b"null" in lib.phyamd_last_error()


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(LIB) or not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("built library or llvm tools missing")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "profiles", "kernel_resources.py"), "k_reweight_"], check=True, capture_output=True,
                         text=True).stdout
    return json.loads(out)["kernels"]


@pytest.mark.parametrize("name", ["k_reweight_terms4<false>", "k_reweight_terms4<true>", "k_reweight_mfma", "k_reweight_finish"])
def test_reweight_kernels_are_there_once_and_spill_nothing(kernels, name):
    hits = [k for n, k in kernels.items() if n == name or n.startswith(name + "(")]
    assert len(hits) == 1, (name, sorted(kernels))
    k = hits[0]
    assert k["vgpr_spill_count"] == 0 and k["scratch_bytes"] == 0, k
