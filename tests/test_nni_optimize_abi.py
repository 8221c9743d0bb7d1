"""CPU-only: phyamd_nni_optimize -- the central branch of every NNI neighbour optimised in one call -- is declared, exported and
bound without an ABI bump, refuses null arguments with a message before it looks at the handle's state, its two kernels are
single code-object entries that spill nothing and use no scratch memory, and the kernel families it stands beside keep their
counts (profiles/kernel_resources.py reads the code object; no GPU needed)."""
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
NAME = "phyamd_nni_optimize"
PROFILE = "phyamd_get_nni_optimize_profile"


def test_symbol_is_declared_exported_and_bound():
    from physher_amd import _lib
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "physher_amd.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert re.search(r"\b%s\s*\(" % NAME, text)
    assert re.search(r"\b%s\s*\(" % PROFILE, text)
    assert hasattr(lib, NAME) and hasattr(lib, PROFILE)
    bound = {n: args for n, _, args in _lib.SYMBOLS}
    assert NAME in bound and len(bound[NAME]) == 12
    assert PROFILE in bound
    assert lib.phyamd_abi_version() == 5  # appended entry points: no signature changed


def test_engine_and_seam_b_have_the_method():
    from physher_amd.engine import Engine
    assert callable(getattr(Engine, "nni_optimize"))
    assert callable(getattr(Engine, "nni_optimize_profile"))
    with open(os.path.join(ROOT, "include", "phycpp_amd", "physher.hpp")) as f:
        assert re.search(r"\bNNIOptimize\s*\(", f.read())
    from physher_amd import _phycpp_amd
    assert callable(getattr(_phycpp_amd.TreeLikelihoodInterface, "nni_optimize"))


def test_null_arguments_are_refused_with_a_message():
    from physher_amd import _lib
    lib = _lib.load()
    fn = getattr(lib, NAME)
    out = (ctypes.c_double * 9)()
    assert fn(None, 0, None, 1e-8, 10.0, 1e-8, 100, out, out, None, None, None) == _lib.EINVAL  # null handle
    assert b"null engine" in lib.phyamd_last_error()
    for lengths, lnl, what in ((None, out, b"lengths"), (out, None, b"lnl")):
        assert fn(None, 0, None, 1e-8, 10.0, 1e-8, 100, lengths, lnl, None, None, None) == _lib.EINVAL
        msg = lib.phyamd_last_error()
        assert NAME.encode() in msg and b"null" in msg and what in msg, msg
    assert getattr(lib, PROFILE)(None, None) == _lib.EINVAL
    assert b"null engine" in lib.phyamd_last_error()


def _kernels(prefix):
    if not os.path.exists(LIB) or not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("built library or llvm tools missing")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "profiles", "kernel_resources.py"), prefix], check=True, capture_output=True,
                         text=True).stdout
    return json.loads(out)["kernels"]


def test_the_new_kernels_appear_once_and_spill_nothing():
    kernels = _kernels("k_cbopt")
    assert len(kernels) == 2, sorted(kernels)
    for name in ("k_cbopt_coeff4", "k_cbopt_solve4"):
        hits = [k for n, k in kernels.items() if n == name or n.startswith(name + "(")]
        assert len(hits) == 1, (name, sorted(kernels))
        assert hits[0]["vgpr_spill_count"] == 0 and hits[0]["sgpr_spill_count"] == 0 and hits[0]["scratch_bytes"] == 0, (name, hits[0])


def test_the_families_beside_it_keep_their_kernels():
    """the walk of the call is k_batch_walk4<false> with the NNI call's op list: no new instantiation, no new kernel of either family"""
    assert sorted(n.split("(")[0] for n in _kernels("k_nni")) == ["k_nni4", "k_nni_finish"]
    names = sorted(n.split("(")[0] for n in _kernels("k_batch_"))
    assert names == ["k_batch_finish", "k_batch_matrices", "k_batch_walk4<false>", "k_batch_walk4<true>"], names
