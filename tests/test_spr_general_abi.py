"""CPU-only: phyamd_spr_log_likelihoods_general -- every SPR regraft of chosen subtrees of a 20-state engine's tree scored in one
call from the resident lower partials -- is declared, exported and bound without an ABI bump or a change of the profile struct,
refuses null arguments with a message that names it before it looks at the handle's state, and its two kernels are single
code-object entries that spill nothing and keep their static LDS under 64 KB (profiles/kernel_resources.py reads the code object; no
GPU needed).  The kernels are k_classspr_walk and k_classspr: tests/test_spr_abi.py and tests/test_spr_optimize_abi.py count the
kernels whose names hold "k_spr" and expect the 4-state calls' three (phyamd_spr_gen.inc)."""
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
NAME = "phyamd_spr_log_likelihoods_general"


def test_symbol_is_declared_exported_and_bound():
    from physher_amd import _lib
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "physher_amd.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert re.search(r"\b%s\s*\(" % NAME, text)
    assert hasattr(lib, NAME)
    bound = {n: args for n, _, args in _lib.SYMBOLS}
    assert NAME in bound and len(bound[NAME]) == 5
    assert bound[NAME] == bound["phyamd_spr_log_likelihoods"]  # the 4-state call's signature
    assert lib.phyamd_abi_version() == 5  # an appended entry point: no signature changed


def test_the_profile_struct_is_unchanged():
    """phyamd_get_spr_profile serves both calls: int32 prunes, chunks, int64 candidates, scratch_bytes, double ms"""
    from physher_amd import _lib
    assert ctypes.sizeof(_lib.SprProfile) == 32
    assert [n for n, _ in _lib.SprProfile._fields_] == ["prunes", "chunks", "candidates", "scratch_bytes", "ms"]


def test_engine_has_the_method():
    from physher_amd.engine import Engine
    assert callable(getattr(Engine, "spr_log_likelihoods_general"))
    assert callable(getattr(Engine, "spr_profile"))


def test_the_model_interface_has_the_method():
    from physher_amd import _phycpp_amd as pc
    assert callable(getattr(pc.TreeLikelihoodInterface, "spr_log_likelihoods_general"))


def test_null_arguments_are_refused_with_a_message():
    from physher_amd import _lib
    lib = _lib.load()
    fn = getattr(lib, NAME)
    out = (ctypes.c_double * 9)()
    assert fn(None, 0, 3, None, out) == _lib.EINVAL  # null handle
    msg = lib.phyamd_last_error()
    assert NAME.encode() in msg and b"null engine" in msg, msg
    assert fn(None, 0, 3, None, None) == _lib.EINVAL  # null lnl, reported before the handle is looked at
    msg = lib.phyamd_last_error()
    assert NAME.encode() in msg and b"null lnl" in msg, msg


def _kernels(pattern):
    assert os.path.exists(LIB), "the engine library is not built"
    if not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("llvm tools missing")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "profiles", "kernel_resources.py"), pattern], check=True, capture_output=True, text=True).stdout
    return json.loads(out)["kernels"]


@pytest.fixture(scope="module")
def kernels():
    return _kernels("k_classspr")


def test_the_kernels_appear_once_each(kernels):
    assert sorted(n.split("(")[0] for n in kernels) == ["k_classspr", "k_classspr_walk"], sorted(kernels)


@pytest.mark.parametrize("kernel", ["k_classspr_walk", "k_classspr"])
def test_the_hot_kernels_spill_nothing(kernels, kernel):
    (k,) = [v for n, v in kernels.items() if n.split("(")[0] == kernel]
    assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["scratch_bytes"] == 0, k
    assert k["lds_static_bytes"] < 64 * 1024, k


def test_the_four_state_family_is_what_it_was():
    assert sorted(n.split("(")[0] for n in _kernels("k_spr")) == ["k_spr4", "k_spr_finish", "k_spr_walk4"]
