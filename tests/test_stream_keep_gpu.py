"""GPU: the streamed pre-order walk with an elided node's stored child kept in registers from its parent's op to its own
(stream_keep, PHYAMD_STREAM_KEEP, on by default) against the same walk with the switch off, bit for bit, and against the CPU
oracle, on the trees whose host schedule provably reaches each case (stream_keep_util.CASES: an operand kept beside a tip and
beside a cherry, a node that is not kept because its upper is parked, one whose own op opens a chunk, an operand the prologue
fetched and the opening op kept, an elided right child of an opening op, a chain of shaped nodes, a ladder that is rescaled
several times).

The switch moves no arithmetic: a kept operand is the value the request would have fetched again, and under power-of-two
rescaling its exponent stays with it.  A mistake leaves another plane, or a stale one, in the register set: a wrong gradient in
the subtree behind one op.  Every case holds Engine.gradient() with the switch on against the switch off for equal bits, and
against the oracle at the tolerances of tests/test_stream_elide_gpu.py -- lnL 1e-10 relative, the per-category gradient of every
node 1e-9 max(1, |g|inf), per-pattern lnL 1e-11.  130 patterns are two full blocks of 64 and a ragged one, 300 four and a ragged
one."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import stream_keep_util as sk
from golden_util import reversible_eigen
from gpu_util import engine_from_problem
from oracle import phyoracle as po
from physher_amd import synth
from physher_amd.engine import RESCALE_ALWAYS, RESCALE_NEVER

pytestmark = pytest.mark.gpu

MASKS = np.array([m for m in range(1, 15) if bin(m).count("1") in (2, 3)])
MODES = ("plain", "rescaled", "ambiguous", "rescaled+ambiguous")
# (tree, patterns): every tree of the cases at 130 patterns, the two with the most kept operands at 300 as well
RUNS = tuple((name, 130) for name in sk.GPU_TREES) + (("random200", 300), ("ladder160", 300))


@functools.lru_cache(maxsize=None)
def _case(name, mode, P):
    """the problem and the oracle's answer, computed once and left unchanged"""
    rescaled, ambiguous = "rescaled" in mode, "ambiguous" in mode
    tree = sk.make_tree(name, bl=(0.5, 1.5) if rescaled else (0.01, 0.1))
    assert tree.tip_count <= 200
    rng = np.random.default_rng(16000 + 100 * sk.ALL.index(name) + P)
    C = 4
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
    if ambiguous:  # one tip cell in eight holds one of the ten two- or three-state masks, with the observed state in it
        known = states < 4
        mask = np.where(known, 1 << np.minimum(states, 3).astype(np.int64), 15)
        wide = known & (rng.random(states.shape) < 0.125)
        mask = np.where(wide, mask | MASKS[rng.integers(10, size=states.shape)], mask)
        tp = ((mask[:, :, None] >> np.arange(4)) & 1).astype(np.float64)
    pb = po.Problem(tree.left, tree.right, tree.root, weights, ev, U, Ui, freqs, rates, props, tree.length, tip_states=states, tip_partials=tp,
                    rescale=1 if rescaled else 0)
    ref = pb.gradient()
    for key in ("cat_grad", "pattern_lk"):
        ref[key].setflags(write=False)
    return pb, ref


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
    return engine_from_problem(pb, rescale=RESCALE_ALWAYS if "rescaled" in mode else RESCALE_NEVER, tip_mode="partials" if "ambiguous" in mode else "states")


def _evaluate(name, mode, P):
    pb, _ = _case(name, mode, P)
    with _engine(pb, mode) as e:
        assert e.rescaling == ("rescaled" in mode)
        out = _gradient(e)
        # the pass that reads the rewritten descriptors: the streamed walk on carried partials, rescaled by powers of two or not at all
        ran = e.pass_profile()
        assert (ran["upper_family"], ran["upper_tf"], ran["upper_scale"], ran["upper_ambiguous"]) == (2, 1, 2 if "rescaled" in mode else 0, int("ambiguous" in mode)), ran
        return out


# every run of the module with the switch off, in ONE fresh process (the switch is read once, when an engine is created)
_CHILD = """
import sys
import numpy as np
sys.path[:0] = {paths!r}
import test_stream_keep_gpu as t
out = {{}}
for name, P in t.RUNS:
    for mode in t.MODES:
        lnl, cg, plk = t._evaluate(name, mode, P)
        out[f"{{name}}/{{mode}}/{{P}}/lnl"], out[f"{{name}}/{{mode}}/{{P}}/cg"], out[f"{{name}}/{{mode}}/{{P}}/plk"] = lnl, cg, plk
np.savez({out!r}, **out)
"""


@pytest.fixture(scope="module")
def switched_off(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("stream_keep") / "off.npz")
    tests = os.path.dirname(os.path.abspath(__file__))
    code = _CHILD.format(paths=[tests, os.path.dirname(tests)], out=out)
    done = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PHYAMD_STREAM_KEEP="0"), capture_output=True, text=True, timeout=600)
    assert done.returncode == 0, done.stdout + done.stderr
    assert "PHYAMD_STREAM_KEEP" not in os.environ
    return np.load(out)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,P", RUNS)
def test_on_against_off_and_oracle(name, P, mode, switched_off):
    for case, (tree, shown) in sk.CASES.items():
        if tree == name:
            assert shown(sk.reach(name)), f"{name} no longer reaches: {case}"
    assert sk.reach(name)["kept"] > 0
    _, ref = _case(name, mode, P)
    if "rescaled" in mode:
        assert ref["rescaled"]
    lnl, cg, plk = _evaluate(name, mode, P)
    key = f"{name}/{mode}/{P}/"
    off_lnl, off_cg, off_plk = float(switched_off[key + "lnl"]), switched_off[key + "cg"], switched_off[key + "plk"]
    _compare(f"{name} {mode} P={P}: PHYAMD_STREAM_KEEP=0", off_lnl, off_cg, off_plk, ref)
    _compare(f"{name} {mode} P={P}: kept", lnl, cg, plk, ref)
    print(f"{name} {mode} P={P}: on against off: |d lnL| {abs(lnl - off_lnl):.2e}, max |dg| {np.abs(cg - off_cg).max():.2e}, "
          f"bit-equal gradient rows {int((cg == off_cg).all(axis=1).sum())} of {len(cg)}")
    assert lnl == off_lnl and np.array_equal(cg, off_cg) and np.array_equal(plk, off_plk)
