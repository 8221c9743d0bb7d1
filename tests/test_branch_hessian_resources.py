"""The Hessian form of the level pre-order kernel (k_upper4<..., HESS = true>) in every workgroup size and rescaling variant is in
the built library and spills nothing to memory (profiles/kernel_resources.py reads the code object; no GPU needed).  Like every
level pre-order kernel it parks the wave-uniform matrices' surplus scalar registers in vector-register lanes (sgpr_spill_count),
which costs no memory traffic."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "physher_amd", "libphysher_amd.so")
LLVM = "/opt/rocm/lib/llvm/bin"


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(LIB) or not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("built library or llvm tools missing")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "profiles", "kernel_resources.py"), "k_upper4<"], check=True, capture_output=True,
                         text=True).stdout
    return json.loads(out)["kernels"]


@pytest.mark.parametrize("waves", [4, 8, 16])
@pytest.mark.parametrize("scale", ["false", "true"])
def test_hessian_variants_spill_nothing(kernels, waves, scale):
    k = kernels[f"k_upper4<{waves}, {scale}, false, false, false, true>"]
    assert k["vgpr_spill_count"] == 0 and k["scratch_bytes"] == 0, k


@pytest.mark.parametrize("rt_kt", ["2, 5", "4, 15", "4, 16"])
@pytest.mark.parametrize("scale", ["false", "true"])
def test_generic_hessian_variants_spill_nothing(rt_kt, scale):
    if not os.path.exists(LIB) or not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("built library or llvm tools missing")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "profiles", "kernel_resources.py"), "k_upper_gen<|k_hess_gen"], check=True, capture_output=True,
                         text=True).stdout
    table = json.loads(out)["kernels"]
    k = table["k_hess_gen"]
    assert k["vgpr_spill_count"] == 0 and k["scratch_bytes"] == 0, k
    k = table[f"k_upper_gen<{rt_kt}, false, {scale}, true>"]
    if rt_kt == "4, 16":
        # 61 states: the second product leaves the 256-register budget short by a few registers (at most 16 bytes of scratch
        # per lane; DESIGN.md, "Every branch's second derivative in one pass")
        assert k["vgpr_spill_count"] <= 4 and k["scratch_bytes"] <= 16, k
    else:
        assert k["vgpr_spill_count"] == 0 and k["scratch_bytes"] == 0, k
