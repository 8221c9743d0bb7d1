"""GPU: TreeLikelihoodInterface.PlacementOptimizeGeneral through the pybind module returns the C ABI's bits: a 7-taxon random tree
with its lengths and 20-state sequences (with gaps) under a general 20-state model + Gamma(4), against an Engine given the object's
own patterns, weights, node table and model; each query's three best edges, all three branches and the pendant length alone, no
sets at all, and the object's own state afterwards."""
import numpy as np
import pytest

import placement_general_util as u
from gpu_util import random_problem
from physher_amd.engine import Engine
from physher_amd.placement import likelihood_weight_ratios, top_candidates
from test_spr_optimize_phycpp_gpu import _newick

pytestmark = pytest.mark.gpu
LETTERS = "ARNDCQEGHILKMFPSTWYV"


def test_seven_taxa_return_the_c_abis_bits():
    from physher_amd import _phycpp_amd as pc
    pb = random_problem(7, 70, 4, seed=78, S=20, gaps=0.05)
    names = [f"t{i}" for i in range(pb.T)]
    seqs = ["".join(LETTERS[s] if s < 20 else "-" for s in pb.tip_states[t]) for t in range(pb.T)]
    rng = np.random.default_rng(3)
    freqs = list(rng.dirichlet(np.full(20, 5.0)))
    rates = list(rng.uniform(0.5, 3.0, size=190))
    dt = pc.GeneralDataTypeInterface(list(LETTERS))
    tree = pc.UnRootedTreeModelInterface(_newick(pb, names, pb.root), names)
    subst = pc.GeneralSubstitutionModelInterface(dt, rates, freqs, list(range(190)), True)
    site = pc.GammaSiteModelInterface(0.6, 4, None, None)
    tlk = pc.TreeLikelihoodInterface(list(zip(names, seqs)), tree, subst, site, None)
    before = tlk.log_likelihood()
    p0 = tree.get_parameters()

    d = tree.describe()
    T, P = pb.T, tlk.get_pattern_count()
    left, right, root = np.array(d["left"], dtype=np.int32), np.array(d["right"], dtype=np.int32), int(d["root"])
    lengths = np.array(d["distance"], dtype=np.float64)
    lengths[root] = 0.0
    states = tlk.pattern_states()  # [taxon in alignment order][pattern]
    ev, U, Ui, _ = subst.eigen_system()
    rng = np.random.default_rng(4)
    sets = u.random_sets(rng, 3)
    codes = u.random_codes(rng, 5, P, 3)  # over the object's own patterns
    same = lambda a, b: np.array_equal(a.view(np.uint64), b.view(np.uint64))
    with Engine(T, P, 20, 4, rescale=0) as e:
        e.set_topology(left, right, root)
        e.set_branch_lengths(lengths)
        e.set_eigen(ev, U, Ui)
        e.set_frequencies(freqs)
        e.set_category_rates(site.rates(), site.proportions())
        e.set_pattern_weights(tlk.pattern_weights())
        for tip in range(T):
            e.set_tip_states(tip, states[names.index(d["name"][tip])])
        own = e.log_likelihood()
        assert abs(own - before) <= 1e-10 * abs(before)  # the two sides hold the same problem
        cands = top_candidates(e.placement_log_likelihoods_general(codes, [0.1], split=0.3, sets=sets)[0][0], 3)
        assert cands.shape == (15, 2) and root not in cands[:, 1]
        start = np.linspace(0.05, 0.4, len(cands))
        want = e.placement_optimize_general(codes, cands, sets, start, split=0.3)
        got = tlk.placement_optimize_general(codes, cands, sets, start, split=0.3)
        assert got[0].shape == want[0].shape == (15, 3) and got[1].shape == got[2].shape == got[3].shape == (15,) and got[3].dtype == np.int32
        assert all(same(a, b) for a, b in zip(got[:3], want[:3]))
        assert np.array_equal(got[3], want[3]) and np.all(want[3] != 0) and np.all(want[1] >= want[2])
        w = likelihood_weight_ratios(want[1], cands[:, 0])  # the sparse form serves this call too
        assert all(abs(w[cands[:, 0] == q].sum() - 1.0) < 1e-12 for q in range(5))
        plain = np.minimum(codes, 20)
        pend = tlk.placement_optimize_general(plain, cands, branches=2, max_passes=3)  # no sets, the start defaults to 0.1, the split to 0.5
        ref = e.placement_optimize_general(plain, cands, branches=2, max_passes=3)
        assert all(same(a, b) for a, b in zip(pend[:3], ref[:3]))
        assert np.array_equal(pend[3], ref[3]) and np.array_equal(ref[0][:, 0], 0.5 * lengths[cands[:, 1]])
    assert np.array_equal(tree.get_parameters(), p0) and abs(tlk.log_likelihood() - before) <= 1e-10 * abs(before)
    bad = cands.copy()
    bad[0, 1] = root
    with pytest.raises(pc.PhyamdError):
        tlk.placement_optimize_general(codes, bad, sets)
    with pytest.raises(pc.PhyamdError):  # the 4-state call keeps refusing 20 states
        tlk.placement_optimize(np.ones((1, P), dtype=np.uint8), cands[:1] * 0 + [[0, cands[0, 1]]])
