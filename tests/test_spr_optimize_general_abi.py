"""CPU-only: phyamd_spr_optimize_general -- the three graft branches of every SPR regraft of a 20-state engine's tree optimised in one
call -- is declared, exported and bound with phyamd_spr_optimize's signature and without an ABI bump or a change of the profile
struct, refuses null and invalid arguments with a message that names it before it looks at the handle's state, and its two kernels
are single code-object entries that use no scratch memory, spill nothing and keep their static LDS under 64 KB
(profiles/kernel_resources.py reads the code object; no GPU needed).  The kernels are k_classgraft_upper and k_classgraft_solve:
the resource tests of the calls beside it count kernels by "k_classspr", "k_classopt" and "k_tripod" and expect their own, which
are unchanged (k_tripod_finish serves both optimise calls)."""
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
NAME = "phyamd_spr_optimize_general"


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
    assert NAME in bound and len(bound[NAME]) == len(params) == 14
    assert bound[NAME] == bound["phyamd_spr_optimize"]  # the 4-state call's signature
    kinds = {"phyamd_engine *": ctypes.c_void_p, "int ": ctypes.c_int, "const int32_t *": ctypes.c_void_p, "double ": ctypes.c_double, "int32_t ": ctypes.c_int32,
             "double *": ctypes.c_void_p, "int32_t *": ctypes.c_void_p}
    for p, bound_type in zip(params, bound[NAME]):
        kind = re.sub(r"\w+$", "", p)
        assert kinds[kind] is bound_type, (p, bound_type)
    four = re.search(r"\bint\s+phyamd_spr_optimize\s*\(([^;]*)\)\s*;", text)
    assert [" ".join(p.split()) for p in four.group(1).split(",")] == params  # argument for argument
    assert lib.phyamd_abi_version() == 5  # an appended entry point: no signature changed


def test_the_profile_struct_is_unchanged():
    """phyamd_get_spr_optimize_profile serves both calls: int32 prunes, chunks, int64 candidates, visits, iterations, scratch_bytes,
    double ms"""
    from physher_amd import _lib
    assert ctypes.sizeof(_lib.SprOptimizeProfile) == 48
    assert [n for n, _ in _lib.SprOptimizeProfile._fields_] == ["prunes", "chunks", "candidates", "visits", "iterations", "scratch_bytes", "ms"]


def test_engine_has_the_method():
    from physher_amd.engine import Engine
    assert callable(getattr(Engine, "spr_optimize_general"))
    assert callable(getattr(Engine, "spr_optimize_profile"))


def test_the_model_interface_has_the_method():
    from physher_amd import _phycpp_amd as pc
    assert callable(getattr(pc.TreeLikelihoodInterface, "spr_optimize_general"))


def test_null_and_invalid_arguments_are_refused_with_a_message():
    """the argument checks come before the handle's state is looked at: every one of them is reported on a null handle"""
    from physher_amd import _lib
    lib = _lib.load()
    fn = getattr(lib, NAME)
    out = (ctypes.c_double * 27)()
    good = dict(count=3, lower=1e-8, upper=10.0, tolerance=1e-8, max_iterations=100, lnl_tolerance=1e-6, max_passes=50, lengths=out, lnl=out)

    def call(**kw):
        a = dict(good, **kw)
        rc = fn(None, 0, a["count"], None, a["lower"], a["upper"], a["tolerance"], a["max_iterations"], a["lnl_tolerance"], a["max_passes"], a["lengths"], a["lnl"], None,
                None)
        msg = lib.phyamd_last_error()
        assert rc == _lib.EINVAL and NAME.encode() in msg, (kw, rc, msg)
        return msg
    assert b"null engine" in call()
    assert b"null lengths" in call(lengths=None)
    assert b"null lnl" in call(lnl=None)
    assert b"count must be >= 1" in call(count=0)
    # (with every pointer given, the null handle is reported first and the rest needs an engine: tests/test_spr_optimize_general_gpu.py)


def _kernels(prefix):
    assert os.path.exists(LIB), "the engine library is not built"
    if not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("llvm tools missing")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "profiles", "kernel_resources.py"), prefix], check=True, capture_output=True,
                         text=True).stdout
    return {n.split("(")[0]: k for n, k in json.loads(out)["kernels"].items()}


def test_the_new_kernels_appear_once_and_spill_nothing():
    kernels = _kernels("k_classgraft")
    assert sorted(kernels) == ["k_classgraft_solve", "k_classgraft_upper"], sorted(kernels)
    for name, k in kernels.items():
        print(name, k)
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["scratch_bytes"] == 0, (name, k)
        assert 0 < k["lds_static_bytes"] < 64 * 1024, (name, k)


def test_the_families_beside_it_keep_their_kernels():
    assert sorted(_kernels("k_classspr")) == ["k_classspr", "k_classspr_walk"]
    assert sorted(_kernels("k_classopt")) == ["k_classopt_solve"]
    assert sorted(_kernels("k_tripod")) == ["k_tripod_finish", "k_tripod_solve4", "k_tripod_upper4"]
