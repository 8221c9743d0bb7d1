"""GPU: the plain streamed pre-order walk with pair ops (stream_pairs, PHYAMD_STREAM_PAIRS, on by default: the op of a DEEP child
runs inside its parent's op) against the CPU oracle, on the trees whose host schedule provably reaches each case
(stream_pairs_util.CASES: a stored and a tip sibling, every pair of half kinds, the sibling's upper handed on in registers, a
parent whose upper arrives in registers, from each LDS slot and from HBM, the root as parent, a tree without a pair, a walk cut
into chunks).

A mistake in a pair shows as a wrong gradient at the branches of one DEEP node or in the subtree of its sibling: every case holds
Engine.gradient() against the oracle at the tolerances of tests/test_upper_park_gpu.py -- lnL 1e-10 relative, the per-category
gradient of every node 1e-9 max(1, |g|inf), per-pattern lnL 1e-11.  130 patterns are two full blocks of 64 and a ragged one."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import stream_pairs_util as sp
from golden_util import reversible_eigen
from gpu_util import engine_from_problem
from oracle import phyoracle as po
from physher_amd import synth
from physher_amd.engine import RESCALE_ALWAYS, RESCALE_NEVER

pytestmark = pytest.mark.gpu

MASKS = np.array([m for m in range(1, 15) if bin(m).count("1") in (2, 3)])


@functools.lru_cache(maxsize=None)
def _case(name, C, mode, P=130):
    """the problem and the oracle's answer, computed once and left unchanged"""
    rescaled = mode == "rescaled"
    tree = sp.make_tree(name, bl=(0.5, 1.5) if rescaled else (0.01, 0.1))
    assert tree.tip_count <= 200
    rng = np.random.default_rng(15000 + 100 * sp.ALL.index(name) + 10 * C + P)
    states = synth.evolve(tree, P, 4, rng)
    states = np.where(rng.random(states.shape) < 0.03, 4 + 13, states).astype(np.uint8)
    weights = rng.integers(1, 5, size=P).astype(np.float64)
    freqs = rng.dirichlet(np.full(4, 5.0))
    r = rng.uniform(0.5, 3.0, size=(4, 4))
    ev, U, Ui = reversible_eigen(0.5 * (r + r.T), freqs)
    rates = np.sort(rng.gamma(0.5, 2.0, size=C)) + 0.05
    props = np.full(C, 1.0 / C)
    rates = rates / (rates * props).sum()
    tp = None
    if mode == "ambiguous":  # ONE tip cell holds a two-state mask with the observed state in it: the whole pass takes the AMBIG instantiation
        known = states < 4
        mask = np.where(known, 1 << np.minimum(states, 3).astype(np.int64), 15)
        t, k = np.argwhere(known)[len(np.argwhere(known)) // 2]
        mask[t, k] |= 1 << ((int(states[t, k]) + 1) % 4)
        tp = ((mask[:, :, None] >> np.arange(4)) & 1).astype(np.float64)
    pb = po.Problem(tree.left, tree.right, tree.root, weights, ev, U, Ui, freqs, rates, props, tree.length, tip_states=states, tip_partials=tp,
                    rescale=1 if rescaled else 0)
    ref = pb.gradient()
    for key in ("cat_grad", "pattern_lk"):
        ref[key].setflags(write=False)
    return pb, ref


def _assert_reached(name):
    for case, (tree, shown) in sp.CASES.items():
        if tree == name:
            assert shown(sp.reach(name)), f"{name} no longer reaches: {case}"


def _compare(label, lnl, cg, plk, ref):
    rel = abs(lnl - ref["lnl"]) / abs(ref["lnl"])
    gerr = np.abs(cg - ref["cat_grad"])
    gtol = 1e-9 * max(1.0, np.abs(ref["cat_grad"]).max())
    perr = np.abs(plk - ref["pattern_lk"])
    ptol = 1e-11 + 1e-11 * np.abs(ref["pattern_lk"])
    worst = int(np.unravel_index(np.argmax(gerr), gerr.shape)[0]) if np.isfinite(gerr).all() else -1
    print(f"{label}: lnL {lnl!r} (oracle {ref['lnl']!r}) rel {rel:.2e} (bound 1e-10); max |dg| {np.nanmax(gerr):.2e} at node {worst} (bound {gtol:.2e}); "
          f"max per-pattern |dlnL| / bound {np.nanmax(perr / ptol):.2e} (bound 1)")
    assert np.isfinite(lnl) and rel <= 1e-10
    assert np.isfinite(cg).all() and (gerr <= gtol).all(), f"nodes off: {sorted(set(np.argwhere(~(gerr <= gtol))[:, 0].tolist()))[:20]}"
    assert (perr <= ptol).all()


def _gradient(e):
    lnl, cg = e.gradient()
    return lnl, np.array(cg), np.array(e.pattern_log_likelihoods())


def _engine(pb, mode):
    return engine_from_problem(pb, rescale=RESCALE_ALWAYS if mode == "rescaled" else RESCALE_NEVER, tip_mode="partials" if mode == "ambiguous" else "states")


@pytest.mark.parametrize("name,C,P", [(n, 4, 130) for n in sp.GPU_TREES] + [("pairs_gallery", 1, 130), ("random200", 1, 130), ("pairs_gallery", 4, 64)])
def test_gradient(name, C, P):
    _assert_reached(name)
    pb, ref = _case(name, C, "plain", P)
    with _engine(pb, "plain") as e:
        _compare(f"{name} C={C} P={P}", *_gradient(e), ref)


@pytest.mark.parametrize("name", ("pairs_gallery", "random200"))
def test_rescaled_takes_the_two_op_form(name):
    """RESCALE_ALWAYS: the rescaled instantiation reads the descriptors without pair ops, and the table blocks it shares with the
    plain pass -- which hold a pair's extra rows -- serve it as before"""
    pb, ref = _case(name, 4, "rescaled")
    with _engine(pb, "rescaled") as e:
        assert e.rescaling
        _compare(f"{name} C=4 rescaled", *_gradient(e), ref)


@pytest.mark.parametrize("name", ("pairs_gallery", "random200"))
def test_one_partial_ambiguity_code_takes_the_two_op_form(name):
    pb, ref = _case(name, 4, "ambiguous")
    between = (pb.tip_partials.sum(axis=2) > 1) & (pb.tip_partials.sum(axis=2) < 4)
    assert between.sum() == 1
    with _engine(pb, "ambiguous") as e:
        _compare(f"{name} C=4, one ambiguity code", *_gradient(e), ref)


_CHILD = """
import sys
import numpy as np
sys.path[:0] = {paths!r}
import test_stream_pairs_gpu as t
pb, ref = t._case({name!r}, 4, "plain")
with t._engine(pb, "plain") as e:
    lnl, cg, plk = t._gradient(e)
np.savez({out!r}, lnl=lnl, cg=cg, plk=plk)
"""


def test_on_against_off(tmp_path):
    """the same problem in a fresh process with PHYAMD_STREAM_PAIRS=0 (read once, when an engine is created).  Every branch term of
    a pair has an accumulator row of its own and every message is formed by the instructions of the two-op form: the gradients
    are equal, bit for bit"""
    name = "pairs_gallery"
    pb, ref = _case(name, 4, "plain")
    out = str(tmp_path / "off.npz")
    tests = os.path.dirname(os.path.abspath(__file__))
    code = _CHILD.format(paths=[tests, os.path.dirname(tests)], name=name, out=out)
    done = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PHYAMD_STREAM_PAIRS="0"), capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stdout + done.stderr
    off = np.load(out)
    _compare(f"{name}: PHYAMD_STREAM_PAIRS=0", float(off["lnl"]), off["cg"], off["plk"], ref)
    assert "PHYAMD_STREAM_PAIRS" not in os.environ
    with _engine(pb, "plain") as e:
        lnl, cg, plk = _gradient(e)
    _compare(f"{name}: pairs on", lnl, cg, plk, ref)
    print(f"{name}: on against off: |d lnL| {abs(lnl - float(off['lnl'])):.2e}, max |dg| {np.abs(cg - off['cg']).max():.2e}, "
          f"bit-equal gradient rows {int((cg == off['cg']).all(axis=1).sum())} of {len(cg)}")
    assert lnl == float(off["lnl"]) and np.array_equal(cg, off["cg"])
