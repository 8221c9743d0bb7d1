"""GPU: TreeLikelihoodInterface.PlacementOptimize through the pybind module returns the C ABI's bits: a 9-taxon random tree with
its lengths, sequences and frequencies under HKY + Gamma(4), against an Engine given the object's own patterns, weights, node table
and model; each query's three best edges, all three branches and the pendant length alone, and the object's own state afterwards."""
import numpy as np
import pytest

import placement_util as u
from gpu_util import random_problem
from physher_amd.engine import Engine
from physher_amd.placement import top_candidates
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
    T, P = pb.T, tlk.get_pattern_count()
    left, right, root = np.array(d["left"], dtype=np.int32), np.array(d["right"], dtype=np.int32), int(d["root"])
    lengths = np.array(d["distance"], dtype=np.float64)
    lengths[root] = 0.0
    states = tlk.pattern_states()  # [taxon in alignment order][pattern]
    ev, U, Ui, _ = subst.eigen_system()
    masks = u.random_masks(np.random.default_rng(4), 5, P)  # over the object's own patterns
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
        cands = top_candidates(e.placement_log_likelihoods(masks, [0.1], split=0.3)[0][0], 3)
        assert cands.shape == (15, 2) and root not in cands[:, 1]
        start = np.linspace(0.05, 0.4, len(cands))
        want = e.placement_optimize(masks, cands, start, split=0.3)
        got = tlk.placement_optimize(masks, cands, start, split=0.3)
        assert got[0].shape == want[0].shape == (15, 3) and got[1].shape == got[2].shape == got[3].shape == (15,) and got[3].dtype == np.int32
        for a, b in zip(got[:3], want[:3]):
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
        assert np.array_equal(got[3], want[3]) and np.all(want[3] != 0) and np.all(want[1] >= want[2])
        pend = tlk.placement_optimize(masks, cands, branches=2, max_passes=3)  # the start defaults to 0.1, the split to 0.5
        ref = e.placement_optimize(masks, cands, branches=2, max_passes=3)
        for a, b in zip(pend[:3], ref[:3]):
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
        assert np.array_equal(pend[3], ref[3]) and np.array_equal(ref[0][:, 0], 0.5 * lengths[cands[:, 1]])
    assert np.array_equal(tree.get_parameters(), p0) and tlk.log_likelihood() == before
    bad = cands.copy()
    bad[0, 1] = root
    with pytest.raises(pc.PhyamdError):
        tlk.placement_optimize(masks, bad)
