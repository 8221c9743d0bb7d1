"""CPU-only: phyamd_get_pass_profile -- which 4-state kernel the last post-order and pre-order passes launched -- is declared,
exported and bound without an ABI bump, its binding has the header's fields in the header's order, and it refuses null arguments
with a message that names the function.  What it reports is checked where it is used: tests/test_pass_kernels_gpu.py."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIELDS = ["lower_family", "lower_form", "lower_scale", "lower_ambiguous", "lower_incremental", "lower_waves", "lower_ppt",
          "upper_family", "upper_scale", "upper_ambiguous", "upper_waves", "upper_tf", "upper_fold", "upper_compat", "upper_params", "upper_catblk",
          "upper_pair_ops"]


def _header():
    with open(os.path.join(ROOT, "include", "physher_amd.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def test_symbol_is_declared_exported_and_bound():
    from physher_amd import _lib
    lib = _lib.load()
    assert re.search(r"\bphyamd_get_pass_profile\s*\(", _header())
    assert hasattr(lib, "phyamd_get_pass_profile")
    bound = {n: args for n, _, args in _lib.SYMBOLS}
    assert len(bound["phyamd_get_pass_profile"]) == 2
    assert lib.phyamd_abi_version() == 5  # an appended entry point: no signature changed
    from physher_amd.engine import Engine
    assert callable(getattr(Engine, "pass_profile"))


def test_binding_has_the_header_fields_in_order():
    from physher_amd import _lib
    body = re.search(r"typedef struct \{([^}]*)\} phyamd_pass_profile;", _header()).group(1)
    assert set(re.findall(r"\b(int32_t|int64_t|double|int)\b", body)) == {"int32_t"}
    names = re.findall(r"\b([a-z_]+)\s*[,;]", body)
    assert names == FIELDS  # the fields the issue of the profile names, in its order
    assert names == [k for k, _ in _lib.PassProfile._fields_]
    assert all(t is ctypes.c_int32 for _, t in _lib.PassProfile._fields_)
    assert ctypes.sizeof(_lib.PassProfile) == 4 * len(names)


def test_null_arguments_are_refused_with_a_message():
    from physher_amd import _lib
    lib = _lib.load()
    out = _lib.PassProfile()
    assert lib.phyamd_get_pass_profile(None, ctypes.byref(out)) == _lib.EINVAL
    msg = lib.phyamd_last_error()
    assert b"phyamd_get_pass_profile" in msg and b"null engine" in msg, msg
    # (a null `out` is refused the same way behind a live engine, which takes a GPU: tests/test_pass_kernels_gpu.py)
