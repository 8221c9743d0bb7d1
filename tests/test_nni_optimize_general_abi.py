"""CPU-only: phyamd_nni_optimize_general -- the central branch of every NNI neighbour of a 20-state engine's tree optimised in one
call from the resident partials -- is declared, exported and bound with phyamd_nni_optimize's signature and without an ABI bump or
a change of the profile struct, refuses null arguments with a message that names it before it looks at the handle's state, and
its two kernels are single code-object entries that use no scratch memory, spill nothing and keep the registers and the static LDS
measured when they were written, up to the next occupancy step (profiles/kernel_resources.py reads the code object; no GPU needed):
k_classcb_coeff 120 VGPRs and 32256 bytes (six matrix images), k_classcb_solve 117 VGPRs and 4192 bytes.  The kernels are the
issue's k_classcb_*: the resource tests of the calls beside it count kernels by "k_nni", "k_cbopt", "k_classnni" and "k_classopt"
and expect their own, which are unchanged."""
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
NAME = "phyamd_nni_optimize_general"


def test_symbol_is_declared_exported_and_bound():
    from physher_amd import _lib
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "physher_amd.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % NAME, text)
    assert decl, "not declared in include/physher_amd.h"
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    assert hasattr(lib, NAME)
    bound = {n: args for n, _, args in _lib.SYMBOLS}
    assert NAME in bound and len(bound[NAME]) == len(params) == 12
    assert bound[NAME] == bound["phyamd_nni_optimize"]  # the 4-state call's signature
    # the declaration's parameters, one by one, against the bound types
    kinds = {"phyamd_engine *": ctypes.c_void_p, "int ": ctypes.c_int, "const double *": ctypes.c_void_p, "double ": ctypes.c_double, "int32_t ": ctypes.c_int32,
             "double *": ctypes.c_void_p, "int32_t *": ctypes.c_void_p}
    for p, bound_type in zip(params, bound[NAME]):
        kind = re.sub(r"\w+$", "", p)
        assert kinds[kind] is bound_type, (p, bound_type)
    four = re.search(r"\bint\s+phyamd_nni_optimize\s*\(([^;]*)\)\s*;", text)
    assert [" ".join(p.split()) for p in four.group(1).split(",")] == params  # word for word
    assert lib.phyamd_abi_version() == 5  # an appended entry point: no signature changed


def test_the_profile_struct_is_unchanged():
    """phyamd_get_nni_optimize_profile serves both calls: int32 candidates, chunks, int64 scratch_bytes, iterations, double ms"""
    from physher_amd import _lib
    assert ctypes.sizeof(_lib.NniOptimizeProfile) == 32
    assert [n for n, _ in _lib.NniOptimizeProfile._fields_] == ["candidates", "chunks", "scratch_bytes", "iterations", "ms"]


def test_engine_has_the_method():
    from physher_amd.engine import Engine
    assert callable(getattr(Engine, "nni_optimize_general"))
    assert callable(getattr(Engine, "nni_optimize_profile"))


def test_the_model_interface_has_the_method():
    from physher_amd import _phycpp_amd as pc
    assert callable(getattr(pc.TreeLikelihoodInterface, "nni_optimize_general"))


def test_null_arguments_are_refused_with_a_message():
    from physher_amd import _lib
    lib = _lib.load()
    fn = getattr(lib, NAME)
    out = (ctypes.c_double * 9)()
    assert fn(None, 0, None, 1e-8, 10.0, 1e-8, 100, out, out, None, None, None) == _lib.EINVAL  # null handle
    msg = lib.phyamd_last_error()
    assert NAME.encode() in msg and b"null engine" in msg, msg
    for lengths, lnl, what in ((None, out, b"null lengths"), (out, None, b"null lnl")):  # reported before the handle is looked at
        assert fn(None, 0, None, 1e-8, 10.0, 1e-8, 100, lengths, lnl, out, out, None) == _lib.EINVAL
        msg = lib.phyamd_last_error()
        assert NAME.encode() in msg and what in msg, msg


def _kernels(prefix):
    assert os.path.exists(LIB), "the engine library is not built"
    if not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("llvm tools missing")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "profiles", "kernel_resources.py"), prefix], check=True, capture_output=True,
                         text=True).stdout
    return {n.split("(")[0]: k for n, k in json.loads(out)["kernels"].items()}


def test_the_new_kernels_appear_once_use_no_scratch_and_keep_their_resources():
    kernels = _kernels("k_classcb")
    assert sorted(kernels) == ["k_classcb_coeff", "k_classcb_solve"], sorted(kernels)
    for name, k in kernels.items():
        print(name, k)
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["scratch_bytes"] == 0, (name, k)
        assert k["vgpr_count"] <= 128, (name, k)  # four waves per SIMD
    assert 0 < kernels["k_classcb_coeff"]["lds_static_bytes"] <= 40 * 1024  # four workgroups share a CU's 160 KB
    assert 0 < kernels["k_classcb_solve"]["lds_static_bytes"] <= 8 * 1024


def test_the_families_beside_it_keep_their_kernels():
    assert sorted(_kernels("k_nni")) == ["k_nni4", "k_nni_finish"]
    assert sorted(_kernels("k_cbopt")) == ["k_cbopt_coeff4", "k_cbopt_solve4"]
    assert sorted(_kernels("k_classnni")) == ["k_classnni"]
    assert sorted(_kernels("k_classopt")) == ["k_classopt_solve"]
