"""GPU: the 4-state pre-order walk on trees whose host schedule provably reaches each way an upper partial can travel
(upper_park_util.NAMED, chosen_for: carries, both LDS park slots, recycled and crossing HBM slots, the from_prev rewrite, the
chunking threshold, every pair of child kinds).  The kernels check none of the schedule, so a hazard shows as a wrong gradient in
one subtree of one tree shape: every case first asserts, from phyamd_pre_order_schedule, what its tree is here for, then holds
Engine.gradient() against the CPU oracle at DESIGN.md section 4's tolerances: lnL 1e-10 relative, the per-category gradient of
every node 1e-9 max(1, |g|inf), per-pattern lnL 1e-11.

130 patterns are three waves of 64, the last one ragged; 300 patterns reach a second workgroup of the streamed walk.  Modes:
plain; rescaled (RESCALE_ALWAYS, branch lengths 0.5-1.5: the parked uppers carry exponents); ambiguous (tip partials with two-
and three-state masks: the AMBIG instantiation).  Which kernel reads which list (upper_kernel, phyamd_shard.inc):
  * gradient(): k_upper4_stream on the streamed form (form 1) -- also with PHYAMD_SCALE_EXP2=0 and C <= 4, its SCALE == 1
    instantiation with the LDS exchange;
  * gradient() with PHYAMD_SCALE_EXP2=0, rescaled, C = 6 > STREAM_WAVES: k_upper4_walk on the chunked list (form 0);
  * parameter_gradient(): k_upper4_walk's PARAMS form on the unchunked list (form 2)."""
import functools

import numpy as np
import pytest

import upper_park_util as u
from golden_util import reversible_eigen
from gpu_util import engine_from_problem
from oracle import phyoracle as po
from physher_amd import synth
from physher_amd.engine import RESCALE_ALWAYS, RESCALE_NEVER

pytestmark = pytest.mark.gpu

MODES = ("plain", "rescaled", "ambiguous")
MASKS = np.array([m for m in range(1, 15) if bin(m).count("1") in (2, 3)])


@functools.lru_cache(maxsize=None)
def _case(name, C, mode, P=130):
    """the problem and the oracle's answer, computed once"""
    rescaled = mode == "rescaled"
    tree = u.make_tree(name, bl=(0.5, 1.5) if rescaled else (0.01, 0.1))
    rng = np.random.default_rng(9000 + 100 * u.NAMED.index(name) + 10 * C + P % 7)
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
                    rescale=1 if rescaled else 0)
    ref = pb.gradient()
    ref["cat_grad"].setflags(write=False)
    ref["pattern_lk"].setflags(write=False)
    return pb, ref


def _assert_chosen(name):
    what, shown = u.chosen_for(name)
    assert shown, f"{name} no longer reaches what it is here for: {what}"


def _check_gradient(label, pb, ref, mode):
    with engine_from_problem(pb, rescale=RESCALE_ALWAYS if mode == "rescaled" else RESCALE_NEVER,
                             tip_mode="partials" if mode == "ambiguous" else "states") as e:
        lnl, cg = e.gradient()
        cg = np.array(cg)
        plk = np.array(e.pattern_log_likelihoods())
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


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("C", [1, 4])
@pytest.mark.parametrize("name", u.NAMED)
def test_streamed_walk(name, C, mode):
    _assert_chosen(name)
    pb, ref = _case(name, C, mode)
    _check_gradient(f"{name} C={C} {mode}", pb, ref, mode)


@pytest.mark.parametrize("name", u.NAMED)
def test_second_workgroup(name):
    """300 patterns are five blocks of 64: a second workgroup of four waves, its last wave ragged"""
    _assert_chosen(name)
    pb, ref = _case(name, 4, "plain", 300)
    _check_gradient(f"{name} C=4 plain P=300", pb, ref, "plain")


def _most_parks():
    return sorted(u.NAMED, key=lambda n: -u.named_stats(n)[1]["parks"])[:3]


@pytest.mark.parametrize("rank", [0, 1, 2])
def test_reference_rescaling(rank, monkeypatch):
    """the three named trees with the most parks, rescaled as the reference does: the SCALE == 1 instantiation of the streamed
    walk, whose category waves exchange their maxima through LDS beside the park slots"""
    name = _most_parks()[rank]
    _assert_chosen(name)
    assert u.named_stats(name)[1]["parks"] >= 15
    pb, ref = _case(name, 4, "rescaled")
    monkeypatch.setenv("PHYAMD_SCALE_EXP2", "0")
    _check_gradient(f"{name} C=4 rescaled, PHYAMD_SCALE_EXP2=0", pb, ref, "rescaled")


@pytest.mark.parametrize("name", u.NAMED)
def test_chunked_list_reader(name, monkeypatch):
    """six categories rescaled as the reference does do not fit the streamed walk's workgroup (stream_shape_fits): the pre-order
    pass is k_upper4_walk on the chunked list itself (form 0: one LDS slot, the other parks in recycled HBM slots)"""
    _assert_chosen(name)
    pb, ref = _case(name, 6, "rescaled")
    monkeypatch.setenv("PHYAMD_SCALE_EXP2", "0")
    _check_gradient(f"{name} C=6 rescaled, PHYAMD_SCALE_EXP2=0", pb, ref, "rescaled")


@pytest.mark.parametrize("name", u.NAMED)
def test_parameter_walk(name):
    """parameter_gradient runs k_upper4_walk in its PARAMS form (form 2: the unchunked list, every park in an HBM slot of the
    free_w list); comparison and tolerance of test_engine_gpu.py::test_parameter_gradient_random_problems"""
    _assert_chosen(name)
    tree = u.make_tree(name)
    ops, slots = u.pre_order_schedule(tree, 2)
    u.check_contract(tree, ops, slots, 2)
    pb, ref = _case(name, 4, "plain")
    rng = np.random.default_rng(7)
    dQ = rng.normal(size=(9, 4, 4))
    dQ -= dQ.sum(axis=2, keepdims=True) * np.eye(4)[None]  # rows sum to zero like any dQ/dtheta
    _, og = po.parameter_gradient(pb, dQ)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        e.set_rate_matrix_derivatives(dQ)
        lnl, cg, pg = e.parameter_gradient()
    scale = max(1.0, np.abs(og).max())
    gtol = 1e-9 * max(1.0, np.abs(ref["cat_grad"]).max())
    print(f"{name} parameters: max |dp| {np.abs(pg - og).max():.2e} (bound {1e-9 * scale:.2e}); max |dg| {np.abs(cg - ref['cat_grad']).max():.2e} (bound {gtol:.2e})")
    assert np.abs(pg - og).max() <= 1e-9 * scale
    assert np.abs(cg - ref["cat_grad"]).max() <= gtol
