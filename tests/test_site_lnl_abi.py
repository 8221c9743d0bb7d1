"""CPU-only: the entry points of the per-pattern lnL of a batch of trees (phyamd_pattern_log_likelihoods_trees,
phyamd_get_site_lnl_profile, phyamd_post_order_slots) are declared, exported and bound, refuse null and half-given arguments with a
message that names the function and the argument before the handle is looked at, and the call's kernels are in the built library's
code object, once each, without spilling registers (profiles/kernel_resources.py reads the code object; no GPU needed)."""
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
NAME = "phyamd_pattern_log_likelihoods_trees"
NAMES = [NAME, "phyamd_get_site_lnl_profile", "phyamd_post_order_slots"]


def test_symbols_are_declared_exported_and_bound():
    from physher_amd import _lib
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "physher_amd.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    bound = {n: args for n, _, args in _lib.SYMBOLS}
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(lib, name), name
        assert name in bound, name
    declared = re.search(r"\b%s\s*\(([^)]*)\)" % NAME, text).group(1)
    assert len(declared.split(",")) == 12 and len(bound[NAME]) == 12
    assert len(bound["phyamd_post_order_slots"]) == 7
    assert lib.phyamd_abi_version() == 5  # appended entry points: no signature changed
    fields = [n for n, _ in _lib.SiteLnlProfile._fields_]
    assert fields == ["items", "chunks", "replicate_chunks", "lower_slots", "scratch_bytes", "ms"]
    assert ctypes.sizeof(_lib.SiteLnlProfile) == 32  # four int32, int64, double
    from physher_amd.engine import Engine
    assert hasattr(Engine, "pattern_log_likelihoods_trees") and hasattr(Engine, "site_lnl_profile")


def test_null_and_half_given_arguments_are_refused_before_the_handle_is_looked_at():
    from physher_amd import _lib
    lib = _lib.load()
    fn = getattr(lib, NAME)
    ints = (ctypes.c_int32 * 3)()
    bl = (ctypes.c_double * 3)()
    lnl = (ctypes.c_double * 1)()
    w = (ctypes.c_double * 1)()
    rep = (ctypes.c_double * 1)()

    def refused(*args):
        assert fn(*args) == _lib.EINVAL, args
        msg = lib.phyamd_last_error()
        assert msg.startswith(NAME.encode() + b": "), msg
        return msg

    # (the handle is null throughout: every other argument is judged first)
    assert b"null engine" in refused(None, 0, 1, ints, ints, ints, bl, lnl, None, 0, None, None)
    assert b"null engine" in refused(None, 0, 1, None, None, None, bl, lnl, None, 1, w, rep)
    assert b"null branch_lengths" in refused(None, 0, 1, ints, ints, ints, None, lnl, None, 0, None, None)
    assert b"null lnl" in refused(None, 0, 1, ints, ints, ints, bl, None, None, 0, None, None)
    for count in (0, -3):
        msg = refused(None, 0, count, ints, ints, ints, bl, lnl, None, 0, None, None)
        assert b"count" in msg and str(count).encode() in msg, msg
    for missing, name in ((0, b"left"), (1, b"right"), (2, b"roots")):
        for given in ([i for i in range(3) if i != missing], [(missing + 1) % 3]):  # one missing, and only one given
            trees = [ints if i in given else None for i in range(3)]
            msg = refused(None, 0, 1, *trees, bl, lnl, None, 0, None, None)
            first = (b"left", b"right", b"roots")[min(i for i in range(3) if i not in given)]
            assert b"null " + first in msg, msg
    msg = refused(None, 0, 1, ints, ints, ints, bl, lnl, None, -2, None, None)
    assert b"replicate_count" in msg and b"-2" in msg, msg
    assert b"null replicate_lnl" in refused(None, 0, 1, ints, ints, ints, bl, lnl, None, 1, w, None)
    assert b"null replicate_weights" in refused(None, 0, 1, ints, ints, ints, bl, lnl, None, 1, None, rep)
    assert b"replicate_weights given with replicate_count 0" in refused(None, 0, 1, ints, ints, ints, bl, lnl, None, 0, w, None)
    assert b"replicate_lnl given with replicate_count 0" in refused(None, 0, 1, ints, ints, ints, bl, lnl, None, 0, None, rep)
    prof = _lib.SiteLnlProfile()
    assert lib.phyamd_get_site_lnl_profile(None, ctypes.byref(prof)) == _lib.EINVAL
    assert b"null" in lib.phyamd_last_error()


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(LIB) or not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("built library or llvm tools missing")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "profiles", "kernel_resources.py"), "k_sitelnl_"], check=True, capture_output=True,
                         text=True).stdout
    return json.loads(out)["kernels"]


@pytest.mark.parametrize("name", ["k_sitelnl_walk4", "k_sitelnl_rell_finish"])
def test_site_lnl_kernels_are_there_once_and_spill_nothing(kernels, name):
    hits = [k for n, k in kernels.items() if n == name or n.startswith(name + "(")]
    assert len(hits) == 1, (name, sorted(kernels))
    k = hits[0]
    assert k["vgpr_spill_count"] == 0 and k["scratch_bytes"] == 0, k


def test_no_other_site_lnl_kernel(kernels):
    assert len(kernels) == 2, sorted(kernels)
