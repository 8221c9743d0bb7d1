"""GPU: TreeLikelihoodInterface.PairwiseDistances through the pybind module returns the C ABI's bits: the alignment of case A of
tests/test_pair_distance_gpu.py (six taxa, fifty patterns with gaps, written out as sequences by their weights) under GTR + Gamma(4),
against an Engine without a tree given the object's own patterns, weights and model; all pairs and a list, the tables, counting
only, and the object's own state afterwards."""
import numpy as np
import pytest

from gpu_util import random_problem
from physher_amd.engine import Engine

pytestmark = pytest.mark.gpu
NEWICK = "((t0:0.1,t1:0.2):0.05,(t2:0.1,t3:0.15):0.1,(t4:0.3,t5:0.1):0.2);"


def test_case_a_returns_the_c_abis_bits():
    from physher_amd import _phycpp_amd as pc
    pb = random_problem(6, 50, 4, 1, gaps=0.1)
    names = [f"t{i}" for i in range(pb.T)]
    columns = np.repeat(np.arange(pb.P), pb.weights.astype(int))
    seqs = ["".join("ACGT"[s] if s < 4 else "-" for s in pb.tip_states[t, columns]) for t in range(pb.T)]
    rates, freqs = [1.2, 3.1, 0.8, 0.9, 3.4, 1.0], [0.3, 0.2, 0.22, 0.28]
    tree = pc.UnRootedTreeModelInterface(NEWICK, names)
    subst = pc.GTRInterface(rates, freqs)
    site = pc.GammaSiteModelInterface(0.6, 4, None, None)
    tlk = pc.TreeLikelihoodInterface(list(zip(names, seqs)), tree, subst, site, None)
    before = tlk.log_likelihood()
    p0 = tree.get_parameters()

    d = tree.describe()
    T, P = pb.T, tlk.get_pattern_count()
    states = tlk.pattern_states()  # [taxon in alignment order][pattern]
    ev, U, Ui, _ = subst.eigen_system()
    with Engine(T, P, 4, 4, rescale=0) as e:  # no topology, no lengths
        e.set_eigen(ev, U, Ui)
        e.set_frequencies(freqs)
        e.set_category_rates(site.rates(), site.proportions())
        e.set_pattern_weights(tlk.pattern_weights())
        for tip in range(T):
            e.set_tip_states(tip, states[names.index(d["name"][tip])])
        listed = np.array([[3, 1], [0, 5], [0, 2], [4, 2]], dtype=np.int32)
        start = np.array([0.5, 0.02, 0.1, 1.5])
        for pairs, st in ((None, None), (listed, start)):
            want = e.pairwise_distances(pairs, st, lower=1e-6, upper=5.0, tolerance=1e-7, max_iterations=50, want_counts=True)
            got = tlk.pairwise_distances(pairs, st, lower=1e-6, upper=5.0, tolerance=1e-7, max_iterations=50, want_counts=True)
            n = 15 if pairs is None else len(pairs)
            for name, a, b in zip(("distances", "lnl", "d1", "d2", "iterations", "counts"), got, want):
                assert a.shape[0] == n and np.array_equal(a, b), name
            assert np.all(np.isfinite(want[1])) and np.all(want[4] > 0)
            assert np.all(want[5].sum(axis=(1, 2)) == pb.weights.sum())
        only = tlk.pairwise_distances(listed, counts_only=True)
        assert all(x is None for x in only[:5]) and np.array_equal(only[5], want[5])
        plain = tlk.pairwise_distances()
        assert plain[5] is None and plain[0].shape == (15,)
    assert np.array_equal(tree.get_parameters(), p0) and tlk.log_likelihood() == before
    with pytest.raises(pc.PhyamdError):
        tlk.pairwise_distances(np.array([[0, 0]], dtype=np.int32))
