"""GPU: the whole-tree query calls share one scratch group -- gradient_batch, branch_hessian, nni_log_likelihoods,
gradient_batch_trees, spr_log_likelihoods and state_posteriors alternate on ONE engine, uncapped and under max_device_bytes, and
every call returns the bits the same call returns on a fresh engine that has run only gradient().  The calls are documented as
returning identical bits call after call, so there is no tolerance.  The per-feature tests never alternate the calls: what one
call leaves in the scratch (kept, regrown, released under a cap) is what the next one finds.  A longer uncapped sequence puts
gradient_batch_weights (with and without lengths), pattern_log_likelihoods_trees with replicates and nni_optimize between them."""
import functools

import numpy as np
import pytest

from gpu_util import engine_from_problem, random_problem
from physher_amd.engine import RESCALE_NEVER
from test_batch_gpu import _lengths
from test_tree_batch_gpu import _mixed

pytestmark = pytest.mark.gpu

# three 64-pattern blocks, the last one partial; NNI and SPR candidates present
T, P, C = 11, 130, 2
# the cap is held + scratch / CAP_DIVISOR (held: device_bytes after gradient(), scratch: the largest scratch_bytes a call of the
# uncapped sequence reports).  At 2.5 no call is refused for want of a whole item (NNI and SPR need one) and the SPR rows run in
# three chunks
CAP_DIVISOR = 2.5


@functools.lru_cache(maxsize=None)
def _problem():
    pb = random_problem(T, P, C, seed=4711, gaps=0.05)
    return pb, _lengths(pb, 8, seed=12), _mixed(T, ["random", "caterpillar", "balanced", "random"], seed=13)


def _weights(rows, seed):
    """pattern-weight rows [rows, P]: small counts, zeros among them"""
    return np.random.default_rng(seed).integers(0, 4, size=(rows, P)).astype(np.float64)


def _calls(bl, trees):
    """(name, call, profile getter or None) in the order the sequence makes them"""
    batch = ("gradient_batch", lambda e: e.gradient_batch(bl), lambda e: e.batch_profile())
    hessian = ("branch_hessian", lambda e: e.branch_hessian(), lambda e: e.hessian_profile())
    return [batch, hessian,
            ("nni_log_likelihoods", lambda e: e.nni_log_likelihoods(), lambda e: e.nni_profile()),
            ("gradient_batch_trees", lambda e: e.gradient_batch_trees(*trees.args()), lambda e: e.batch_profile()),
            ("spr_log_likelihoods", lambda e: (e.spr_log_likelihoods(),), lambda e: e.spr_profile()),
            ("state_posteriors", lambda e: e.state_posteriors(), None),
            hessian, batch]


def _calls_with_the_newer_kinds(bl, trees):
    """_calls' sequence with gradient_batch_weights (per-item lengths: the batched walk with a weight row per item; without: the
    shared-lengths product), pattern_log_likelihoods_trees on the same four trees with three replicate rows, and nni_optimize
    between its calls"""
    batch, hessian, nni, tree_batch, spr, posteriors, hessian2, batch2 = _calls(bl, trees)
    w, reps = _weights(len(bl), seed=14), _weights(3, seed=15)
    weights_lengths = ("gradient_batch_weights with lengths", lambda e: e.gradient_batch_weights(w, bl), lambda e: e.weight_batch_profile())
    weights_shared = ("gradient_batch_weights", lambda e: e.gradient_batch_weights(w), lambda e: e.weight_batch_profile())
    site_lnl = ("pattern_log_likelihoods_trees", lambda e: e.pattern_log_likelihoods_trees(*trees.args(), replicate_weights=reps),
                lambda e: e.site_lnl_profile())
    nni_optimize = ("nni_optimize", lambda e: e.nni_optimize(), lambda e: e.nni_optimize_profile())
    return [batch, weights_lengths, hessian, nni, nni_optimize, tree_batch, weights_shared, spr, site_lnl, posteriors, nni_optimize, hessian2,
            weights_lengths, site_lnl, nni, weights_shared, batch2]


def _same_bits(a, b):
    if len(a) != len(b):
        return False
    for x, y in zip(a, b):
        if x is None or y is None:
            if x is not y:
                return False
            continue
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
            return False
    return True


_fresh = {}  # name -> the call's result on an engine of its own that has run only gradient(): made once, never written again


def fresh_results(pb, calls):
    """each distinct call on an engine of its own that has run only gradient()"""
    for name, call, _ in calls:
        if name not in _fresh:
            with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
                e.gradient()
                _fresh[name] = call(e)
    return _fresh


def run_sequence(pb, calls, cap=0):
    """the calls in order on one engine -> (held, [(name, result, profile or None, device_bytes after the call)])"""
    out = []
    with engine_from_problem(pb, rescale=RESCALE_NEVER, max_device_bytes=cap) as e:
        e.gradient()  # (the engine's own buffers are made: what it holds besides the scratch)
        held = e.profile()["device_bytes"]
        for name, call, profile in calls:
            res = call(e)
            out.append((name, res, profile(e) if profile else None, e.profile()["device_bytes"]))
    return held, out


def test_alternating_calls_return_a_fresh_engines_bits():
    """eight calls of six kinds on one engine, then again under max_device_bytes = held + scratch / 2.5 (CAP_DIVISOR: no call is
    refused there, and the SPR rows run in chunks): every result has a fresh engine's bits, and under the cap device_bytes stays
    within it after every call and at least one call reports chunks >= 2"""
    pb, bl, trees = _problem()
    calls = _calls(bl, trees)
    ref = fresh_results(pb, calls)
    held, seq = run_sequence(pb, calls)
    for i, (name, res, prof, bytes_after) in enumerate(seq):
        print(f"uncapped {i} {name}: {prof} device_bytes {bytes_after}")
        assert _same_bits(res, ref[name]), (i, name)
    scratch = max(prof["scratch_bytes"] for _, _, prof, _ in seq if prof)
    cap = int(held + scratch / CAP_DIVISOR)
    _, capped = run_sequence(pb, calls, cap)
    for i, (name, res, prof, bytes_after) in enumerate(capped):
        print(f"cap {cap} {i} {name}: {prof} device_bytes {bytes_after}")
        assert bytes_after <= cap, (i, name, bytes_after, cap)
        assert _same_bits(res, ref[name]), (i, name)
    assert max(prof["chunks"] for _, _, prof, _ in capped if prof and "chunks" in prof) >= 2


def test_alternating_calls_with_the_newer_kinds_return_a_fresh_engines_bits():
    """seventeen calls of ten kinds on one uncapped engine -- the six kinds above, gradient_batch_weights with and without lengths,
    pattern_log_likelihoods_trees with three replicate rows and nni_optimize with its defaults, interleaved: every result has a
    fresh engine's bits"""
    pb, bl, trees = _problem()
    calls = _calls_with_the_newer_kinds(bl, trees)
    ref = fresh_results(pb, calls)
    _, seq = run_sequence(pb, calls)
    for i, (name, res, prof, bytes_after) in enumerate(seq):
        print(f"uncapped {i} {name}: {prof} device_bytes {bytes_after}")
        assert _same_bits(res, ref[name]), (i, name)
