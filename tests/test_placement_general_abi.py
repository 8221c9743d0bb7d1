"""CPU-only: phyamd_placement_log_likelihoods_general -- query sequences of a 20-state engine scored on every edge of its tree in
one call -- is declared, exported and bound without an ABI bump, and refuses null arguments, bad counts, a bad split, bad pendant
lengths and bad sets with a message that names the function and the argument before it looks at the handle."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "phyamd_placement_log_likelihoods_general"


def test_symbols_are_declared_exported_and_bound():
    from physher_amd import _lib
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "physher_amd.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert re.search(r"\b%s\s*\(" % NAME, text)
    assert hasattr(lib, NAME)
    bound = {n: args for n, _, args in _lib.SYMBOLS}
    assert NAME in bound and len(bound[NAME]) == 12
    assert len(bound["phyamd_placement_log_likelihoods"]) == 10  # the 4-state call's signature is unchanged
    assert ctypes.sizeof(_lib.PlacementProfile) == 40  # the shared profile is unchanged
    assert lib.phyamd_abi_version() == 5  # appended entry points: no signature changed


def test_engine_and_helpers_have_the_methods():
    from physher_amd import placement
    from physher_amd.engine import Engine
    assert callable(getattr(Engine, "placement_log_likelihoods_general"))
    assert callable(placement.codes_from_protein)


def test_null_arguments_and_bad_values_are_refused_with_a_message():
    from physher_amd import _lib
    lib = _lib.load()
    fn = getattr(lib, NAME)
    codes = (ctypes.c_uint8 * 8)(*([20] * 8))
    sets = (ctypes.c_uint64 * 2)(0b11, 1 << 19 | 1)
    pend = (ctypes.c_double * 2)(0.1, 0.2)
    lnl = (ctypes.c_double * 64)()
    node = (ctypes.c_int32 * 8)()
    best = (ctypes.c_double * 8)()

    def refused(*args):
        assert fn(*args) == _lib.EINVAL
        msg = lib.phyamd_last_error()
        assert NAME.encode() in msg, msg
        return msg

    assert b"null engine" in refused(None, 0, 1, codes, 2, sets, 2, pend, 0.5, lnl, node, best)  # everything else is in order
    assert b"null engine" in refused(None, 0, 1, codes, 0, None, 2, pend, 0.5, lnl, node, best)  # no sets at all
    msg = refused(None, 0, 1, codes, 2, sets, 2, pend, 0.5, None, None, None)
    assert b"null lnl" in msg and b"best_node" in msg
    assert b"best_lnl without best_node" in refused(None, 0, 1, codes, 2, sets, 2, pend, 0.5, lnl, None, best)
    assert b"null codes" in refused(None, 0, 1, None, 2, sets, 2, pend, 0.5, lnl, node, best)
    assert b"null pendant" in refused(None, 0, 1, codes, 2, sets, 2, None, 0.5, lnl, node, best)
    for count in (0, -2):
        assert b"queries" in refused(None, 0, count, codes, 2, sets, 2, pend, 0.5, lnl, node, best)
        assert b"lengths" in refused(None, 0, 1, codes, 2, sets, count, pend, 0.5, lnl, node, best)
    for split in (-0.01, 1.01, float("nan"), float("inf")):
        assert b"split" in refused(None, 0, 1, codes, 2, sets, 2, pend, split, lnl, node, best)
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        msg = refused(None, 0, 1, codes, 2, sets, 2, (ctypes.c_double * 2)(0.1, bad), 0.5, lnl, node, best)
        assert b"pendant[1]" in msg
    for count in (-1, 12):
        assert b"set_count" in refused(None, 0, 1, codes, count, sets, 2, pend, 0.5, lnl, node, best)
    assert b"null sets" in refused(None, 0, 1, codes, 2, None, 2, pend, 0.5, lnl, node, best)
    for word in (0, 1 << 20, (1 << 63) | 1):
        assert b"sets[1]" in refused(None, 0, 1, codes, 2, (ctypes.c_uint64 * 2)(0b11, word), 2, pend, 0.5, lnl, node, best)
