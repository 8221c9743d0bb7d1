"""CPU-only: phyamd_state_posteriors and phyamd_site_rate_posteriors -- marginal ancestral states and site-rate posteriors per
pattern -- are declared, exported and bound without an ABI bump, refuse null arguments with a message before they look at the
handle's state, their three kernels are single code-object entries that spill nothing and use no scratch, and the batched walk
still has exactly its four kernels (profiles/kernel_resources.py reads the code object; no GPU needed)."""
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
NAMES = {"phyamd_state_posteriors": 6, "phyamd_site_rate_posteriors": 3}


def test_symbols_are_declared_exported_and_bound():
    from physher_amd import _lib
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "physher_amd.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    bound = {n: args for n, _, args in _lib.SYMBOLS}
    for name, nargs in NAMES.items():
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(lib, name), name
        assert name in bound and len(bound[name]) == nargs, name
    assert lib.phyamd_abi_version() == 5  # appended entry points: no signature changed


def test_engine_has_the_methods():
    from physher_amd.engine import Engine
    assert callable(getattr(Engine, "state_posteriors"))
    assert callable(getattr(Engine, "site_rate_posteriors"))


def test_null_arguments_are_refused_with_a_message():
    from physher_amd import _lib
    lib = _lib.load()
    out = (ctypes.c_double * 4)()
    assert lib.phyamd_state_posteriors(None, 0, 1, None, out, None) == _lib.EINVAL  # null handle
    assert b"null engine" in lib.phyamd_last_error()
    assert lib.phyamd_site_rate_posteriors(None, out, None) == _lib.EINVAL
    assert b"null engine" in lib.phyamd_last_error()


def _kernels(prefix):
    if not os.path.exists(LIB) or not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("built library or llvm tools missing")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "profiles", "kernel_resources.py"), prefix], check=True, capture_output=True,
                         text=True).stdout
    return json.loads(out)["kernels"]


def test_posterior_kernels_appear_once_and_spill_nothing():
    for prefix, names in (("k_post", ("k_post4", "k_post_gen")), ("k_site_rate_post", ("k_site_rate_post",))):
        kernels = _kernels(prefix)
        assert len(kernels) == len(names), sorted(kernels)
        for name in names:
            hits = [k for n, k in kernels.items() if n == name or n.startswith(name + "(")]
            assert len(hits) == 1, (name, sorted(kernels))
            assert hits[0]["vgpr_spill_count"] == 0 and hits[0]["sgpr_spill_count"] == 0 and hits[0]["scratch_bytes"] == 0, (name, hits[0])


def test_the_batched_walk_still_has_its_four_kernels():
    kernels = _kernels("k_batch_")
    names = sorted(n.split("(")[0] for n in kernels)
    assert names == ["k_batch_finish", "k_batch_matrices", "k_batch_walk4<false>", "k_batch_walk4<true>"], sorted(kernels)
