"""CPU-only: phyamd_nni_log_likelihoods_general -- every NNI neighbour of a 20-state engine's tree scored in one call from the resident
partials -- is declared, exported and bound without an ABI bump or a change of the profile struct, refuses null arguments with a
message that names it before it looks at the handle's state, and its kernel is a single code-object entry that spills nothing and
keeps its static LDS under 64 KB (profiles/kernel_resources.py reads the code object; no GPU needed).  The kernel is the issue's
k_classnni: tests/test_nni_abi.py counts the kernels whose names hold "k_nni" and expects the 4-state call's two
(phyamd_nni_gen.inc)."""
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
NAME = "phyamd_nni_log_likelihoods_general"


def test_symbol_is_declared_exported_and_bound():
    from physher_amd import _lib
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "physher_amd.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert re.search(r"\b%s\s*\(" % NAME, text)
    assert hasattr(lib, NAME)
    bound = {n: args for n, _, args in _lib.SYMBOLS}
    assert NAME in bound and len(bound[NAME]) == 6
    assert bound[NAME] == bound["phyamd_nni_log_likelihoods"]  # the 4-state call's signature
    assert lib.phyamd_abi_version() == 5  # an appended entry point: no signature changed


def test_the_profile_struct_is_unchanged():
    """phyamd_get_nni_profile serves both calls: int32 candidates, int64 scratch_bytes, double ms"""
    from physher_amd import _lib
    assert ctypes.sizeof(_lib.NniProfile) == 24
    assert [n for n, _ in _lib.NniProfile._fields_] == ["candidates", "scratch_bytes", "ms"]


def test_engine_has_the_method():
    from physher_amd.engine import Engine
    assert callable(getattr(Engine, "nni_log_likelihoods_general"))
    assert callable(getattr(Engine, "nni_profile"))


def test_the_model_interface_has_the_method():
    from physher_amd import _phycpp_amd as pc
    assert callable(getattr(pc.TreeLikelihoodInterface, "nni_log_likelihoods_general"))


def test_null_arguments_are_refused_with_a_message():
    from physher_amd import _lib
    lib = _lib.load()
    fn = getattr(lib, NAME)
    out = (ctypes.c_double * 9)()
    assert fn(None, 0, None, out, None, None) == _lib.EINVAL  # null handle
    msg = lib.phyamd_last_error()
    assert NAME.encode() in msg and b"null engine" in msg, msg
    assert fn(None, 0, None, None, out, out) == _lib.EINVAL  # null lnl, reported before the handle is looked at
    msg = lib.phyamd_last_error()
    assert NAME.encode() in msg and b"null lnl" in msg, msg


@pytest.fixture(scope="module")
def kernels():
    assert os.path.exists(LIB), "the engine library is not built"
    if not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("llvm tools missing")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "profiles", "kernel_resources.py"), "k_classnni"], check=True, capture_output=True,
                         text=True).stdout
    return json.loads(out)["kernels"]


def test_the_kernel_appears_once(kernels):
    assert sorted(n.split("(")[0] for n in kernels) == ["k_classnni"], sorted(kernels)


def test_the_hot_kernel_spills_nothing(kernels):
    (k,) = [v for n, v in kernels.items() if n.split("(")[0] == "k_classnni"]
    assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["scratch_bytes"] == 0, k
    assert k["lds_static_bytes"] < 64 * 1024, k
