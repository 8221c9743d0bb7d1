"""CPU: the gate of tests/test_edge_lengths_gpu.py.  For every (shape, family, rescale) and every call that file makes, the oracle
and its eigen-reversed copy (the same problem in another rounding) agree within ONE TENTH of the GPU tolerance, so that a GPU
tolerance is at least ten times the yardstick's own rounding sensitivity.  The tenth is a condition on the cases, not a
measurement: a case that missed it would be dropped for that call (edge_inputs_util.PARTIAL_FLOOR is the one place where that
happened), never given a looser tolerance.  Then the three facts the construction relies on.
"""
import numpy as np
import pytest

import edge_inputs_util as eu
from hessian_util import branch_hessian_diagonal
from oracle import phyoracle as po
from physher_amd import synth

GATE = 0.1
CORE = [(s, f, r) for s in eu.SHAPES for f in eu.FAMILIES for r in (0, 1)]
FOUR = [s for s in eu.SHAPES if eu.SHAPES[s][0] == 4]


def _assert_gate(shares, what):
    print(what, {k: f"{v:.2e}" for k, v in shares.items()})
    for k, v in shares.items():
        assert v <= GATE, (what, k, v)


# ---------------------------------------------------------------------------------------------------------
# the construction
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", eu.FAMILIES)
@pytest.mark.parametrize("shape", list(eu.SHAPES))
def test_families_are_what_they_are_named_for(shape, family):
    pb = eu.case(shape, family)
    bl, inner = pb.branch_lengths, eu.internal_branches(pb)
    parts = family.split("+")
    zero_inner = [n for n in inner if bl[n] == 0.0]
    if "polytomy" in parts:
        assert len(zero_inner) == len(inner)
    elif "zero_internal" in parts:
        assert len(zero_inner) == (len(inner) + 1) // 2
    else:
        assert not zero_inner
    cherry = eu.cherry_left_tips(pb)
    assert cherry
    zero_tips = [n for n in range(pb.T) if bl[n] == 0.0]
    assert zero_tips == (sorted(cherry) if "zero_tips" in parts else [])
    tiny = [n for n in inner if 0.0 < bl[n] < 1e-5]
    assert len(tiny) == ((len(inner) + 1) // 2 if "tiny_internal" in parts else 0)
    assert all(1e-12 <= bl[n] <= 1e-6 for n in tiny)
    long_ = [n for n in range(pb.N) if bl[n] >= 20.0]
    assert len(long_) == (max(1, (pb.N - 1) // 4) if "long" in parts else 0) and np.all(bl <= 100.0)
    assert bl[pb.root] == 0.0 and np.all(bl >= 0.0)
    assert np.any(pb.tip_states >= pb.S) or shape == "61s"  # gaps (6 x 17 cells at 3 % may hold none)
    assert eu.case(shape, family) is pb and np.array_equal(eu.edge_problem(*eu.SHAPES[shape], family, eu.seed_of(shape, family)).tip_states, pb.tip_states)


def test_eigen_reversed_is_the_same_model():
    pb = eu.case("4s_t9", "long")
    q = eu.eigen_reversed(pb)
    assert np.array_equal(q.eval, pb.eval[::-1]) and np.array_equal(q.evec, pb.evec[:, ::-1]) and np.array_equal(q.ivec, pb.ivec[::-1])
    np.testing.assert_allclose((q.evec * q.eval) @ q.ivec, (pb.evec * pb.eval) @ pb.ivec, rtol=0, atol=1e-15)
    assert q.tip_states is pb.tip_states and np.array_equal(q.branch_lengths, pb.branch_lengths)


@pytest.mark.parametrize("S", [4, 20, 61])
def test_a_zero_length_branch_gets_no_substitution(S):
    """synth.evolve keeps the parent's state with probability 1 / S + (1 - 1 / S) e^0, which must round to 1 at every state count,
    or a zero-length tip would differ from its sibling's parent once in 2^53 draws -- and the oracle would then hang on P(0)'s
    off-diagonals"""
    assert 1.0 / S + (1.0 - 1.0 / S) * np.exp(-S / (S - 1.0) * 0.0) >= 1.0
    rng = np.random.default_rng(S)
    tree = synth.random_tree(8, rng)
    tree.length = np.zeros(tree.node_count)
    states = synth.evolve(tree, 5000, S, rng)
    assert np.all(states == states[0])  # every branch of length 0: every tip is the root


@pytest.mark.parametrize("family", ["zero_tips", "zero_tips+zero_internal", "zero_tips+polytomy+long"])
@pytest.mark.parametrize("shape", list(eu.SHAPES))
def test_a_zero_length_tip_repeats_what_lies_behind_it(shape, family):
    """the cherry's other tip hangs on its own branch; the zero-length one IS the cherry's node, so the posterior of that node is
    the tip's indicator (tests/test_edge_lengths_gpu.py): where both tips of a cherry are observed and its sibling's branch is
    zero too, they agree"""
    pb = eu.case(shape, family)
    for n in range(pb.T, pb.N):
        l, r = pb.left[n], pb.right[n]
        if l < pb.T and r < pb.T and pb.branch_lengths[l] == 0.0 and pb.branch_lengths[r] == 0.0:
            both = (pb.tip_states[l] < pb.S) & (pb.tip_states[r] < pb.S)
            assert np.array_equal(pb.tip_states[l][both], pb.tip_states[r][both])


# ---------------------------------------------------------------------------------------------------------
# the gate
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,family,rescale", CORE)
def test_gate_core(shape, family, rescale):
    """lnL, per-pattern lnL, the per-category gradient, the lower and upper partials of every node; the folded gradient at 4 states;
    and the Hessian diagonal where the GPU file asks for it (4 and 20 states)"""
    pb = eu.case(shape, family, rescale)
    assert pb.gradient()["rescaled"] == bool(rescale)
    shares = eu.gate_core(pb, eu.partial_floor(family))
    if pb.S == 4:
        a = eu.with_fields(pb, fold_root_freqs=1).gradient()
        b = eu.with_fields(eu.eigen_reversed(pb), fold_root_freqs=1).gradient()
        shares["folded gradient"] = eu.share_gradient(b["cat_grad"], a["cat_grad"])
    if pb.S in (4, 20):
        (_, a1, a2), (_, b1, b2) = branch_hessian_diagonal(pb), branch_hessian_diagonal(eu.eigen_reversed(pb))
        shares["d1"], shares["d2"] = eu.share_gradient(b1, a1), eu.share_gradient(b2, a2)
    _assert_gate(shares, f"{shape} {family} rescale={rescale}:")


def test_the_entrywise_partial_bound_is_dropped_where_the_gate_says_so():
    """PARTIAL_FLOOR's reason, kept true: without the floor every family but `long` misses the gate on its partials"""
    for family in eu.FAMILIES:
        pb = eu.case("4s_t24", family)
        s = eu.gate_core(pb, 0.0)
        print(f"{family}: entry-by-entry shares lower {s['lower']:.2e} upper {s['upper']:.2e}")
        assert (max(s["lower"], s["upper"]) <= GATE) == (family == "long")


@pytest.mark.parametrize("family", eu.FAMILIES)
@pytest.mark.parametrize("shape", list(eu.SHAPES))
def test_gate_branch_trials_and_parameters(shape, family):
    """branch_log_likelihood's trials (t = 0, 1e-10, 50 on ordinary branches; an ordinary t on a zero-length one) and the
    substitution-parameter gradient with a random dQ"""
    pb = eu.case(shape, family)
    rev = eu.eigen_reversed(pb)
    shares = {}
    if pb.S in (4, 20):
        trials = eu.branch_trials(shape, family)
        assert [t for _, t in trials[:3]] == list(eu.TRIAL_LENGTHS) and eu.ordinary(pb, trials[0][0])  # the gate left a branch to try
        assert all(pb.branch_lengths[n] == 0.0 and t == eu.TRIAL_ON_ZERO for n, t in trials[3:])
        assert len(trials) > 3 or not np.any(pb.branch_lengths[np.arange(pb.N) != pb.root] == 0.0)
        for n, t in trials:
            shares[f"node {n} t={t:g}"] = eu.gate_branch(pb, n, t)
    dQ = eu.random_dq(pb.S, 2, seed=5)
    (_, ga), (_, gb) = po.parameter_gradient(pb, dQ), po.parameter_gradient(rev, dQ)
    shares["parameters"] = eu.share_gradient(gb, ga)
    _assert_gate(shares, f"{shape} {family}:")


def test_gate_beyond_the_range_of_exp():
    """one branch at 700: the oracle's lnL, gradient and parameter gradient are finite and stand the gate"""
    pb = eu.beyond_exp_case()
    rev = eu.eigen_reversed(pb)
    dQ = eu.random_dq(pb.S, 2, seed=5)
    a, b = pb.gradient(), rev.gradient()
    (_, ga), (_, gb) = po.parameter_gradient(pb, dQ), po.parameter_gradient(rev, dQ)
    assert np.all(np.isfinite(ga)) and np.isfinite(a["lnl"]) and np.all(np.isfinite(a["cat_grad"]))
    _assert_gate(dict(lnl=eu.share_lnl(b["lnl"], a["lnl"]), gradient=eu.share_gradient(b["cat_grad"], a["cat_grad"]), parameters=eu.share_gradient(gb, ga)),
                 "20s long, one branch at 700:")


@pytest.mark.parametrize("family", eu.FAMILIES)
@pytest.mark.parametrize("shape", FOUR)
def test_gate_batch_items(shape, family):
    """gradient_batch / gradient_batch_trees: the case's lengths and the same with every positive length halved and doubled"""
    pb = eu.case(shape, family)
    shares = {}
    for f in eu.BATCH_FACTORS:
        a, b = eu.scaled(pb, f).gradient(), eu.eigen_reversed(eu.scaled(pb, f)).gradient()
        shares[f"x{f:g} lnL"], shares[f"x{f:g} gradient"] = eu.share_lnl(b["lnl"], a["lnl"]), eu.share_gradient(b["cat_grad"], a["cat_grad"])
    _assert_gate(shares, f"{shape} {family}:")


@pytest.mark.parametrize("family", eu.FAMILIES)
def test_gate_full_hessian(family):
    """branch_hessian on the 9-taxon shape: the brute-force restatement (tests/full_hessian_util.py) in both roundings"""
    from full_hessian_util import brute_force
    pb = eu.case("4s_t9", family)
    (la, ga, Ha), (lb, gb, Hb) = brute_force(pb), brute_force(eu.eigen_reversed(pb))
    _assert_gate(dict(lnl=eu.share_lnl(lb, la), g=eu.share_gradient(gb, ga), H=eu.share_gradient(Hb, Ha)), f"4s_t9 {family}:")


@pytest.mark.parametrize("family", eu.POSTERIOR_FAMILIES)
@pytest.mark.parametrize("shape", list(eu.SHAPES))
def test_gate_posteriors(shape, family):
    """state and site-rate posteriors (absolute 1e-9, as the suite holds them), and where the most probable state is compared"""
    from state_posteriors_util import GAP
    pb = eu.case(shape, family)
    a, b = eu.posteriors(pb), eu.posteriors(eu.eigen_reversed(pb))
    shares = dict(states=np.abs(b["post"] - a["post"]).max() / 1e-9, rates=np.abs(b["R"] - a["R"]).max() / 1e-9,
                  mean_rate=np.abs(b["mean"] - a["mean"]).max() / (1e-9 * max(1.0, np.abs(a["mean"]).max())))
    _assert_gate(shares, f"{shape} {family}:")
    sure = a["gap"] >= GAP
    assert np.array_equal(a["states"][sure], b["states"][sure])
    if "zero_tips" in family:  # the node above a zero-length tip IS the tip: the tip's indicator wherever the tip is observed
        n = 0
        for tip, parent, seen in eu.zero_tip_parents(pb):
            ind = np.eye(pb.S)[pb.tip_states[tip][seen]]
            assert np.abs(a["post"][parent][seen] - ind).max() <= 1e-10
            n += np.count_nonzero(seen)
        assert n > 0


@pytest.mark.parametrize("central", eu.NNI_CENTRALS)
@pytest.mark.parametrize("family", eu.NNI_FAMILIES)
@pytest.mark.parametrize("shape", FOUR)
def test_gate_nni(shape, family, central):
    _assert_gate(eu.gate_nni(eu.case(shape, family), central), f"{shape} {family} central={central}:")


# ---------------------------------------------------------------------------------------------------------
# two facts about NNI entries at the ends of the range
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", FOUR)
def test_the_arrangements_of_a_zero_length_edge_are_one_tree(shape):
    """a zero-length central edge joins four subtrees in one point: the three arrangements are the same tree, lnL to 1e-13 relative"""
    for family, central in (("zero_internal", "own"), ("polytomy", "own"), ("long", 0.0)):
        pb = eu.case(shape, family)
        lnl, _ = eu.nni_oracle(pb, central)
        edges = [v for v in eu.nni_candidates(pb) if central != "own" or pb.branch_lengths[v] == 0.0]
        assert edges
        spread = np.abs(lnl[1:, edges] - lnl[0, edges]).max() / np.abs(lnl[0, edges]).min()
        print(f"{shape} {family} central={central}: {len(edges)} zero-length edges, spread {spread:.2e}")
        assert spread <= 1e-13


@pytest.mark.parametrize("family", eu.NNI_FAMILIES)
@pytest.mark.parametrize("shape", FOUR)
def test_d1_vanishes_on_a_saturated_central_edge(shape, family):
    """With the central edge at 30 and ONE rate category of rate 1 every e^{lambda t} but the zero eigenvalue's is below e^{-30}:
    the two halves of the tree are independent and |d1| < 1e-9.  The cases' own mixtures do NOT have that property -- their slowest
    category has a rate of 0.03 to 0.4, e^{lambda 30 r} is up to 0.3 there and |d1| is 1e-5 to 0.11 (printed) -- so at 30 the GPU file
    compares a d1 that is small, not one that is zero; the gate above covers it either way."""
    pb = eu.case(shape, family)
    _, d1 = eu.nni_oracle(pb, 30.0)
    one = eu.with_fields(pb, cat_rates=np.array([1.0]), cat_props=np.array([1.0]), C=1)
    _, d1_one = eu.nni_oracle(one, 30.0)
    print(f"{shape} {family}: at 30 |d1| <= {np.nanmax(np.abs(d1_one)):.2e} with one category, {np.nanmax(np.abs(d1)):.2e} with the case's "
          f"(slowest rate {pb.cat_rates.min():.3f})")
    assert np.nanmax(np.abs(d1_one)) < 1e-9
