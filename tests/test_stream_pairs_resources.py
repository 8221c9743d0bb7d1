"""The register budget of the one instantiation of the streamed pre-order walk that runs pair ops (stream_pairs: the plain TF form,
with and without folded root frequencies), read from the code object of the built library (profiles/kernel_resources.py): four
waves per SIMD -- at most 128 registers -- with nothing spilled and no scratch.  A build-time property, checked without a GPU."""
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
    out = subprocess.run([sys.executable, os.path.join(ROOT, "profiles", "kernel_resources.py"), "k_upper4_stream"], check=True, capture_output=True, text=True).stdout
    return json.loads(out)["kernels"]


@pytest.mark.parametrize("fold", ("false", "true"))
def test_pair_instantiation_keeps_four_waves(kernels, fold):
    k = kernels[f"k_upper4_stream<{fold}, 0, false, true>"]
    print(k)
    assert k["vgpr_count"] <= 128, k
    assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["scratch_bytes"] == 0, k
