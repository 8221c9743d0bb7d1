"""GPU: TreeLikelihoodInterface.PlacementLogLikelihoods through the pybind module returns the C ABI's bits: a 9-taxon random tree
with its lengths, sequences and frequencies under HKY + Gamma(4), against an Engine given the object's own patterns, weights, node
table and model; all outputs, the best edges alone, and the object's own state afterwards."""
import numpy as np
import pytest

import placement_util as u
from gpu_util import random_problem
from physher_amd.engine import Engine
from test_spr_optimize_phycpp_gpu import _newick

pytestmark = pytest.mark.gpu


def test_nine_taxa_return_the_c_abis_bits():
    from physher_amd import _phycpp_amd as pc
    pb = random_problem(9, 130, 4, seed=77)
    names = [f"t{i}" for i in range(pb.T)]
    seqs = ["".join("ACGT"[x] for x in pb.tip_states[i]) for i in range(pb.T)]
    tree = pc.UnRootedTreeModelInterface(_newick(pb, names, pb.root), names)
    freqs = [float(x) for x in pb.freqs]
    subst = pc.HKYInterface(2.0, freqs)
    site = pc.GammaSiteModelInterface(0.6, 4, None, None)
    tlk = pc.TreeLikelihoodInterface(list(zip(names, seqs)), tree, subst, site, None)
    before = tlk.log_likelihood()
    p0 = tree.get_parameters()

    d = tree.describe()
    T, N, P = pb.T, pb.N, tlk.get_pattern_count()
    left, right, root = np.array(d["left"], dtype=np.int32), np.array(d["right"], dtype=np.int32), int(d["root"])
    lengths = np.array(d["distance"], dtype=np.float64)
    lengths[root] = 0.0
    states = tlk.pattern_states()  # [taxon in alignment order][pattern]
    ev, U, Ui, _ = subst.eigen_system()
    masks = u.random_masks(np.random.default_rng(4), 5, P)  # over the object's own patterns
    pendant = np.array([0.05, 0.6])
    with Engine(T, P, 4, 4, rescale=0) as e:
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
        want = e.placement_log_likelihoods(masks, pendant, split=0.3)
        got = tlk.placement_log_likelihoods(masks, pendant, split=0.3)
        assert got[0].shape == want[0].shape == (2, 5, N) and got[1].shape == want[1].shape == (2, 5)
        assert np.array_equal(got[0].view(np.uint64), want[0].view(np.uint64))
        assert np.array_equal(got[1], want[1]) and got[1].dtype == np.int32
        assert np.array_equal(got[2].view(np.uint64), want[2].view(np.uint64))
        assert np.all(np.isnan(want[0][:, :, root])) and np.all(np.isfinite(np.delete(want[0], root, axis=2)))
        none, node, best = tlk.placement_log_likelihoods(masks, pendant, split=0.3, want_lnl=False)
        assert none is None and np.array_equal(node, want[1]) and np.array_equal(best.view(np.uint64), want[2].view(np.uint64))
        lnl, nobody, nothing = tlk.placement_log_likelihoods(masks, pendant, split=0.3, want_best=False)
        assert nobody is None and nothing is None and np.array_equal(lnl.view(np.uint64), want[0].view(np.uint64))
        half = tlk.placement_log_likelihoods(masks, pendant)  # split defaults to 0.5
        assert np.array_equal(half[0].view(np.uint64), e.placement_log_likelihoods(masks, pendant)[0].view(np.uint64))
    assert np.array_equal(tree.get_parameters(), p0) and tlk.log_likelihood() == before
    bad = masks.copy()
    bad[0, 0] = 0
    with pytest.raises(pc.PhyamdError):
        tlk.placement_log_likelihoods(bad, pendant)
