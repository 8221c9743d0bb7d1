"""The two hot kernels of phyamd_placement_log_likelihoods_general are in the built library, spill nothing to memory and keep their
static LDS under 64 KB per workgroup (profiles/kernel_resources.py reads the code object; no GPU needed).  They are the issue's
k_place_table_gen and k_place_score_gen under the names k_classplace_table and k_classplace_score: tests/test_placement_abi.py
counts the kernels whose names hold "k_place" and expects the 4-state call's four (phyamd_place_gen.inc)."""
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
    out = subprocess.run([sys.executable, os.path.join(ROOT, "profiles", "kernel_resources.py"), "k_classplace"], check=True, capture_output=True,
                         text=True).stdout
    return json.loads(out)["kernels"]


def test_the_six_kernels_appear_once(kernels):
    assert sorted(kernels) == ["k_classplace_codes", "k_classplace_images", "k_classplace_own", "k_classplace_score", "k_classplace_table", "k_classplace_transposed_images"]


@pytest.mark.parametrize("name", ["k_classplace_table", "k_classplace_score"])
def test_the_hot_kernels_spill_nothing(kernels, name):
    k = kernels[name]
    assert k["vgpr_spill_count"] == 0 and k["scratch_bytes"] == 0, k
    assert k["lds_static_bytes"] < 64 * 1024, k
