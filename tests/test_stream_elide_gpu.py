"""GPU: the streamed 4-state walks without the stored nodes the pre-order walk can form beside a tip or a cherry (stream_elide,
PHYAMD_STREAM_ELIDE, on by default) against the CPU oracle, on the trees whose host schedule provably reaches each case of the
rule (stream_elide_util.CASES: both new child kinds on both sides, an elided node from park slot 0, alternate nodes of a chain,
refusals for memory and for the second slot, an elided node that opens a pre-order chunk, and an elided left and an elided right
child of an op that opens one, whose stored children the chunk's prologue requests).

An elided array holds stale data, so a mistake shows as a wrong gradient in the subtree behind one op, or as wrong partials in a
later call that reads the array: every case holds Engine.gradient() against the oracle at the tolerances of
tests/test_upper_park_gpu.py -- lnL 1e-10 relative, the per-category gradient of every node 1e-9 max(1, |g|inf), per-pattern lnL
1e-11 -- and the sequences below read the arrays back after a gradient.  200 patterns are three full blocks of 64 and a ragged
one."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import stream_elide_util as se
import upper_park_util as u
from golden_util import reversible_eigen
from gpu_util import engine_from_problem
from hessian_util import branch_hessian_diagonal
from oracle import phyoracle as po
from physher_amd import synth
from physher_amd.engine import GRAD_FOLD_ROOT_FREQS, RESCALE_ALWAYS, RESCALE_NEVER

pytestmark = pytest.mark.gpu

P = 200
MASKS = np.array([m for m in range(1, 15) if bin(m).count("1") in (2, 3)])
SCALING_THRESHOLD = 1e-40


@functools.lru_cache(maxsize=None)
def _case(name, C, mode):
    """the problem and the oracle's answer, computed once and left unchanged"""
    rescaled = mode == "rescaled"
    tree = se.make_tree(name, bl=(0.5, 1.5) if rescaled else (0.01, 0.1))
    rng = np.random.default_rng(12000 + 100 * se.ALL.index(name) + 10 * C)
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
    if mode == "ambiguous":  # one tip cell in eight holds one of the ten two- or three-state masks, with the observed state in it
        known = states < 4
        mask = np.where(known, 1 << np.minimum(states, 3).astype(np.int64), 15)
        wide = known & (rng.random(states.shape) < 0.125)
        mask = np.where(wide, mask | MASKS[rng.integers(10, size=states.shape)], mask)
        tp = ((mask[:, :, None] >> np.arange(4)) & 1).astype(np.float64)
    pb = po.Problem(tree.left, tree.right, tree.root, weights, ev, U, Ui, freqs, rates, props, tree.length, tip_states=states, tip_partials=tp,
                    rescale=1 if rescaled else 0, fold_root_freqs=1 if mode == "fold" else 0)
    ref = pb.gradient(want_partials=mode == "plain")
    for key in ("cat_grad", "pattern_lk", "lower"):
        if ref[key] is not None:
            ref[key].setflags(write=False)
    return pb, ref


def _assert_reached(name):
    for case, (tree, shown) in se.CASES.items():
        if tree == name:
            assert shown(se.reach(name)), f"{name} no longer reaches: {case}"
    assert se.reach(name)["count"] > 0


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


def _gradient(e, flags=0):
    lnl, cg = e.gradient(flags)
    return lnl, np.array(cg), np.array(e.pattern_log_likelihoods())


def _engine(pb, mode):
    return engine_from_problem(pb, rescale=RESCALE_ALWAYS if mode == "rescaled" else RESCALE_NEVER, tip_mode="partials" if mode == "ambiguous" else "states")


@pytest.mark.parametrize("name,C", [(n, 4) for n in se.GPU_TREES] + [("random200", 1)])
def test_gradient(name, C):
    _assert_reached(name)
    pb, ref = _case(name, C, "plain")
    with _engine(pb, "plain") as e:
        _compare(f"{name} C={C}", *_gradient(e), ref)


@pytest.mark.parametrize("name", se.GPU_TREES)
def test_folded_root_frequencies(name):
    pb, ref = _case(name, 4, "fold")
    with _engine(pb, "fold") as e:
        _compare(f"{name} C=4 GRAD_FOLD_ROOT_FREQS", *_gradient(e, GRAD_FOLD_ROOT_FREQS), ref)


@pytest.mark.parametrize("name", se.GPU_TREES)
def test_partial_ambiguity_codes(name):
    """the AMBIG instantiations: the elided child's mask group carries the flag bit of its own tips"""
    pb, ref = _case(name, 4, "ambiguous")
    assert pb.tip_partials is not None and ((pb.tip_partials.sum(axis=2) > 1) & (pb.tip_partials.sum(axis=2) < 4)).any()
    with _engine(pb, "ambiguous") as e:
        _compare(f"{name} C=4 ambiguous", *_gradient(e), ref)


def test_rescaled_ladder():
    """RESCALE_ALWAYS, C = 4, a ladder of 160 tips with branch lengths 0.5-1.5: the walks rescale by powers of two per category
    (LowerForm::CarriedExp2) and an elided node is formed in the units of its stored child.  That the categories' exponents differ
    is read off the oracle's unscaled partials: somewhere on the ladder one category's partial has fallen below the threshold for
    a pattern and another's has not"""
    name = "ladder160"
    r = se.reach(name)
    assert r["kind_sides"] == {(u.TIP, 0), (u.CHERRY, 0)} and r["count"] >= 40
    pb, ref = _case(name, 4, "rescaled")
    assert ref["rescaled"]
    plain = po.Problem(pb.left, pb.right, pb.root, pb.weights, pb.eval, pb.evec, pb.ivec, pb.freqs, pb.cat_rates, pb.cat_props, pb.branch_lengths,
                       tip_states=pb.tip_states, rescale=0).log_likelihood(want_lower=True)["lower"]
    elided = se.stream_elisions(se.make_tree(name))[:, se.NODE]
    peak = plain[elided].max(axis=3)  # [node][C][P]
    below = peak < SCALING_THRESHOLD
    assert (below.any(axis=1) & ~below.all(axis=1)).any(), "no elided node at which the categories' exponents differ"
    with _engine(pb, "rescaled") as e:
        assert e.rescaling
        _compare(f"{name} C=4 rescaled", *_gradient(e), ref)


def test_read_back_between_gradients():
    """one engine: a gradient (the elided arrays are stale), the stored partials of every elided node and of its stored child
    read back (the post-order pass runs again and stores every node), a gradient again"""
    name = "random200"
    pb, ref = _case(name, 4, "plain")
    rec = se.stream_elisions(se.make_tree(name))
    with _engine(pb, "plain") as e:
        _compare(f"{name}: first gradient", *_gradient(e), ref)
        for node in sorted(set(rec[:, se.NODE].tolist()) | set(rec[:, se.STORED].tolist()) | set(rec[:, se.PARENT].tolist())):
            # (the tolerance of the other read-back tests, tests/test_sharded_gpu.py: a stale array is off by orders of magnitude)
            np.testing.assert_allclose(e.partials(int(node)), ref["lower"][node], rtol=1e-9, atol=1e-300, err_msg=f"lower partials of node {node}")
        _compare(f"{name}: gradient after the read-back", *_gradient(e), ref)


def test_hessian_between_gradients():
    """one engine: a gradient, the branch Hessian's diagonal (it reads every stored partial in the reference's form and leaves the
    engine on its own form), a gradient again -- with nothing stored for the elided nodes once more"""
    name = "target"
    pb, ref = _case(name, 4, "plain")
    lr, r1, r2 = branch_hessian_diagonal(pb)
    with _engine(pb, "plain") as e:
        _compare(f"{name}: first gradient", *_gradient(e), ref)
        lnl, d1, d2 = e.branch_hessian_diagonal()
        print(f"{name}: Hessian diagonal: max |d d1| {np.abs(d1 - r1).max():.2e}, max |d d2| {np.abs(d2 - r2).max():.2e}")
        assert abs(lnl - lr) <= 1e-10 * abs(lr)
        assert np.abs(d1 - r1).max() <= 1e-9 * max(1.0, np.abs(r1).max())
        assert np.abs(d2 - r2).max() <= 1e-9 * max(1.0, np.abs(r2).max())
        _compare(f"{name}: gradient after the Hessian", *_gradient(e), ref)
        e.set_branch_length(int(pb.left[pb.root]), float(pb.branch_lengths[pb.left[pb.root]]))  # (an incremental update over the walks' own form)
        _compare(f"{name}: gradient after a branch was set again", *_gradient(e), ref)


_CHILD = """
import json, sys
import numpy as np
sys.path[:0] = {paths!r}
import test_stream_elide_gpu as t
pb, ref = t._case({name!r}, 4, "plain")
with t._engine(pb, "plain") as e:
    lnl, cg, plk = t._gradient(e)
np.savez({out!r}, lnl=lnl, cg=cg, plk=plk)
"""


def test_on_against_off(tmp_path):
    """the same problem in a fresh process with PHYAMD_STREAM_ELIDE=0 (read once, when an engine is created): both answers within
    the tolerances of the oracle.  Equal bits are not demanded (under power-of-two rescaling an elided node's message is formed
    from an unrescaled p_n); the plain form repeats the post-order walk's own arithmetic, and the figures are printed"""
    name = "random200"
    pb, ref = _case(name, 4, "plain")
    out = str(tmp_path / "off.npz")
    tests = os.path.dirname(os.path.abspath(__file__))
    code = _CHILD.format(paths=[tests, os.path.dirname(tests)], name=name, out=out)
    done = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PHYAMD_STREAM_ELIDE="0"), capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stdout + done.stderr
    off = np.load(out)
    _compare(f"{name}: PHYAMD_STREAM_ELIDE=0", float(off["lnl"]), off["cg"], off["plk"], ref)
    assert "PHYAMD_STREAM_ELIDE" not in os.environ
    with _engine(pb, "plain") as e:
        lnl, cg, plk = _gradient(e)
    _compare(f"{name}: elision on", lnl, cg, plk, ref)
    print(f"{name}: on against off: |d lnL| {abs(lnl - float(off['lnl'])):.2e}, max |dg| {np.abs(cg - off['cg']).max():.2e}, "
          f"bit-equal gradient rows {int((cg == off['cg']).all(axis=1).sum())} of {len(cg)}")
