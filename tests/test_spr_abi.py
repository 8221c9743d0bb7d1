"""CPU-only: phyamd_spr_log_likelihoods -- every SPR regraft of chosen subtrees scored in one call -- is declared, exported and
bound without an ABI bump, refuses null arguments and an empty list with a message before it looks at the handle's state, and its
three kernels are single code-object entries that spill nothing (profiles/kernel_resources.py reads the code object; no GPU
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
NAME = "phyamd_spr_log_likelihoods"


def test_symbols_are_declared_exported_and_bound():
    from physher_amd import _lib
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "physher_amd.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert re.search(r"\b%s\s*\(" % NAME, text)
    assert re.search(r"\bphyamd_get_spr_profile\s*\(", text)
    assert hasattr(lib, NAME) and hasattr(lib, "phyamd_get_spr_profile")
    bound = {n: args for n, _, args in _lib.SYMBOLS}
    assert NAME in bound and len(bound[NAME]) == 5
    assert "phyamd_get_spr_profile" in bound
    assert lib.phyamd_abi_version() == 5  # appended entry points: no signature changed


def test_engine_has_the_methods():
    from physher_amd.engine import Engine
    assert callable(getattr(Engine, "spr_log_likelihoods"))
    assert callable(getattr(Engine, "spr_profile"))


def test_null_arguments_and_an_empty_list_are_refused_with_a_message():
    from physher_amd import _lib
    lib = _lib.load()
    fn = getattr(lib, NAME)
    out = (ctypes.c_double * 9)()
    assert fn(None, 0, 3, None, out) == _lib.EINVAL  # null handle
    assert b"null engine" in lib.phyamd_last_error()
    assert fn(None, 0, 3, None, None) == _lib.EINVAL  # null lnl
    msg = lib.phyamd_last_error()
    assert NAME.encode() in msg and b"null" in msg and b"lnl" in msg, msg
    for count in (0, -2):
        assert fn(None, 0, count, None, out) == _lib.EINVAL
        msg = lib.phyamd_last_error()
        assert NAME.encode() in msg and b"count" in msg, msg
    assert lib.phyamd_get_spr_profile(None, None) == _lib.EINVAL
    assert b"null engine" in lib.phyamd_last_error()


def _kernels(prefix):
    if not os.path.exists(LIB) or not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("built library or llvm tools missing")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "profiles", "kernel_resources.py"), prefix], check=True, capture_output=True,
                         text=True).stdout
    return json.loads(out)["kernels"]


def test_spr_kernels_appear_once_and_spill_nothing():
    kernels = _kernels("k_spr")
    assert len(kernels) == 3, sorted(kernels)
    for name in ("k_spr_walk4", "k_spr4", "k_spr_finish"):
        hits = [k for n, k in kernels.items() if n == name or n.startswith(name + "(")]
        assert len(hits) == 1, (name, sorted(kernels))
        assert hits[0]["vgpr_spill_count"] == 0 and hits[0]["sgpr_spill_count"] == 0 and hits[0]["scratch_bytes"] == 0, (name, hits[0])
