"""CPU-only: phyamd_get_general_profile -- how the 20 / 60 / 61-state kernels of the last passes were launched -- is declared,
exported and bound without an ABI bump, its binding has the header's fields in the header's order, and it refuses null arguments
with a message that names the function.  What it reports is checked where it is used: tests/test_general_tiles_gpu.py."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_declared_exported_and_bound():
    from physher_amd import _lib
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "physher_amd.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert re.search(r"\bphyamd_get_general_profile\s*\(", text)
    assert hasattr(lib, "phyamd_get_general_profile")
    bound = {n: args for n, _, args in _lib.SYMBOLS}
    assert len(bound["phyamd_get_general_profile"]) == 2
    assert lib.phyamd_abi_version() == 5  # an appended entry point: no signature changed
    from physher_amd.engine import Engine
    assert callable(getattr(Engine, "general_profile"))


def test_binding_has_the_header_fields_in_order():
    from physher_amd import _lib
    with open(os.path.join(ROOT, "include", "physher_amd.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\} phyamd_general_profile;", text).group(1)
    assert set(re.findall(r"\b(int32_t|int64_t|double|int)\b", body)) == {"int32_t"}
    names = re.findall(r"\b([a-z_]+)\s*[,;]", body)
    assert names == [k for k, _ in _lib.GeneralProfile._fields_]
    assert ctypes.sizeof(_lib.GeneralProfile) == 4 * len(names)


def test_null_arguments_are_refused_with_a_message():
    from physher_amd import _lib
    lib = _lib.load()
    out = _lib.GeneralProfile()
    assert lib.phyamd_get_general_profile(None, ctypes.byref(out)) == _lib.EINVAL
    msg = lib.phyamd_last_error()
    assert b"phyamd_get_general_profile" in msg and b"null engine" in msg, msg
