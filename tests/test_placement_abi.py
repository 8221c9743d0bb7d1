"""CPU-only: phyamd_placement_log_likelihoods -- query sequences scored on every edge of the engine's tree in one call -- is
declared, exported and bound without an ABI bump, refuses null arguments, bad counts, a bad split and bad pendant lengths with a
message before it looks at the handle's state, and its kernels are single code-object entries that spill nothing
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
NAME = "phyamd_placement_log_likelihoods"


def test_symbols_are_declared_exported_and_bound():
    from physher_amd import _lib
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "physher_amd.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert re.search(r"\b%s\s*\(" % NAME, text)
    assert re.search(r"\bphyamd_get_placement_profile\s*\(", text)
    assert hasattr(lib, NAME) and hasattr(lib, "phyamd_get_placement_profile")
    bound = {n: args for n, _, args in _lib.SYMBOLS}
    assert NAME in bound and len(bound[NAME]) == 10
    assert "phyamd_get_placement_profile" in bound
    assert ctypes.sizeof(_lib.PlacementProfile) == 40  # five int32, padding, an int64 and a double
    assert lib.phyamd_abi_version() == 5  # appended entry points: no signature changed


def test_engine_has_the_methods():
    from physher_amd.engine import Engine
    assert callable(getattr(Engine, "placement_log_likelihoods"))
    assert callable(getattr(Engine, "placement_profile"))


def test_null_arguments_and_bad_values_are_refused_with_a_message():
    from physher_amd import _lib
    lib = _lib.load()
    fn = getattr(lib, NAME)
    masks = (ctypes.c_uint8 * 8)(*([1] * 8))
    pend = (ctypes.c_double * 2)(0.1, 0.2)
    lnl = (ctypes.c_double * 64)()
    node = (ctypes.c_int32 * 8)()
    best = (ctypes.c_double * 8)()

    def refused(*args):
        assert fn(*args) == _lib.EINVAL
        msg = lib.phyamd_last_error()
        assert NAME.encode() in msg, msg
        return msg

    assert b"null engine" in refused(None, 0, 1, masks, 2, pend, 0.5, lnl, node, best)  # everything else is in order
    msg = refused(None, 0, 1, masks, 2, pend, 0.5, None, None, None)
    assert b"null lnl" in msg and b"best_node" in msg
    assert b"best_lnl without best_node" in refused(None, 0, 1, masks, 2, pend, 0.5, lnl, None, best)
    assert b"null masks" in refused(None, 0, 1, None, 2, pend, 0.5, lnl, node, best)
    assert b"null pendant" in refused(None, 0, 1, masks, 2, None, 0.5, lnl, node, best)
    for count in (0, -2):
        assert b"queries" in refused(None, 0, count, masks, 2, pend, 0.5, lnl, node, best)
        assert b"lengths" in refused(None, 0, 1, masks, count, pend, 0.5, lnl, node, best)
    for split in (-0.01, 1.01, float("nan"), float("inf")):
        assert b"split" in refused(None, 0, 1, masks, 2, pend, split, lnl, node, best)
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        msg = refused(None, 0, 1, masks, 2, (ctypes.c_double * 2)(0.1, bad), 0.5, lnl, node, best)
        assert b"pendant[1]" in msg
    assert lib.phyamd_get_placement_profile(None, None) == _lib.EINVAL
    assert b"null engine" in lib.phyamd_last_error()


def _kernels(prefix):
    if not os.path.exists(LIB) or not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("built library or llvm tools missing")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "profiles", "kernel_resources.py"), prefix], check=True, capture_output=True,
                         text=True).stdout
    return json.loads(out)["kernels"]


def test_place_kernels_appear_once_and_spill_nothing():
    kernels = _kernels("k_place")
    assert len(kernels) == 4, sorted(kernels)
    for name in ("k_place_table4", "k_place_masks", "k_place_score4", "k_place_finish"):
        hits = [k for n, k in kernels.items() if n == name or n.startswith(name + "(")]
        assert len(hits) == 1, (name, sorted(kernels))
        assert hits[0]["vgpr_spill_count"] == 0 and hits[0]["sgpr_spill_count"] == 0 and hits[0]["scratch_bytes"] == 0, (name, hits[0])
