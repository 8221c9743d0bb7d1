"""GPU: the streamed post-order walk's second park slot (k_lower4_stream, LowerDesc source 3 / flag bit 26).

The slot is used only where the schedule asks for it, so every tree here is chosen on the host (lower_park_util.sources) to
hold at least one slot-1 park and at least one stored child that still comes from memory.  130 patterns are three blocks of 64,
the last one ragged.  Each run is held against the CPU oracle (lnL 1e-10 relative, gradient 1e-9 max(1, |g|inf)) and,
bit for bit per pattern, against an engine created with PHYAMD_LOWER_PARK2=0: the arithmetic and its order are the same, only
where an operand waits differs.  The AMBIG instantiations keep one slot (lstream_park_slots) and read such a child from memory:
for them the comparison says that the two-slot descriptors are read correctly by a one-slot kernel."""
import functools

import numpy as np
import pytest

from golden_util import reversible_eigen
from gpu_util import engine_from_problem
from lower_park_util import TREES, make_tree, sources
from oracle import phyoracle as po
from physher_amd import synth
from physher_amd.engine import RESCALE_ALWAYS, RESCALE_NEVER

pytestmark = pytest.mark.gpu

P = 130
MODES = ("plain", "rescaled", "ambiguous")


@functools.lru_cache(maxsize=None)
def _case(name, C, mode):
    """the problem and the oracle's answer, computed once"""
    rescaled = mode == "rescaled"
    tree = make_tree(name, bl=(0.5, 1.5) if rescaled else (0.01, 0.1))  # long branches: the parked partials carry exponents
    rng = np.random.default_rng(7000 + 10 * TREES.index(name) + C)
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
        masks = [m for m in range(1, 15) if bin(m).count("1") in (2, 3)]
        tp = np.zeros((tree.tip_count, P, 4))
        for t in range(tree.tip_count):
            for k in range(P):
                code = states[t, k]
                if code >= 4:
                    tp[t, k, :] = 1.0
                elif rng.random() < 0.125:
                    m = masks[rng.integers(10)] | (1 << int(code))
                    tp[t, k, :] = [(m >> i) & 1 for i in range(4)]
                else:
                    tp[t, k, code] = 1.0
    pb = po.Problem(tree.left, tree.right, tree.root, weights, ev, U, Ui, freqs, rates, props, tree.length, tip_states=states, tip_partials=tp,
                    rescale=1 if rescaled else 0)
    ref = pb.gradient()
    ref["cat_grad"].setflags(write=False)
    ref["pattern_lk"].setflags(write=False)
    return pb, ref


def _run(pb, mode):
    with engine_from_problem(pb, rescale=RESCALE_ALWAYS if mode == "rescaled" else RESCALE_NEVER,
                             tip_mode="partials" if mode == "ambiguous" else "states") as e:
        lnl, cg = e.gradient()
        return lnl, np.array(cg), np.array(e.pattern_log_likelihoods())


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("C", [1, 4])
@pytest.mark.parametrize("name", TREES)
def test_second_park_slot(name, C, mode, monkeypatch):
    slot1, memory = sources(name)
    assert slot1 >= 1 and memory >= 1, (slot1, memory)
    pb, ref = _case(name, C, mode)
    lnl, cg, plk = _run(pb, mode)
    monkeypatch.setenv("PHYAMD_LOWER_PARK2", "0")
    lnl1, cg1, plk1 = _run(pb, mode)
    rel = abs(lnl - ref["lnl"]) / abs(ref["lnl"])
    gerr = np.abs(cg - ref["cat_grad"]).max()
    gtol = 1e-9 * max(1.0, np.abs(ref["cat_grad"]).max())
    print(f"{name} C={C} {mode}: lnL {lnl!r} (oracle {ref['lnl']!r}, rel {rel:.2e}), max |dg| {gerr:.2e} (bound {gtol:.2e}), "
          f"per-pattern lnL differing from the one-slot engine: {int((plk != plk1).sum())}")
    assert np.isfinite(lnl) and rel <= 1e-10
    assert gerr <= gtol
    assert np.array_equal(plk, plk1)
    assert lnl == lnl1 and np.array_equal(cg, cg1)
