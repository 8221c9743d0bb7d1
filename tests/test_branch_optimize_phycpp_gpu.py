"""GPU: TreeLikelihoodInterface.OptimizeBranchLengths through the pybind module returns the C ABI's bits: nine taxa of the golden
alignment gtr_g4_t16 under GTR + Gamma(4) on a tree of their own (tests/test_nni_phycpp_gpu.py's), against an Engine given the
object's own patterns, weights, node table and model -- two items, with and without a mask -- and the object's own state
afterwards."""
import os

import numpy as np
import pytest

from golden_util import GOLDEN, read_fasta, read_spec
from physher_amd.engine import Engine
from test_nni_phycpp_gpu import NEWICK

pytestmark = pytest.mark.gpu


def test_nine_taxa_return_the_c_abis_bits():
    from physher_amd import _phycpp_amd as pc
    case = "gtr_g4_t16"
    spec = read_spec(case)
    names, seqs = read_fasta(os.path.join(GOLDEN, case, "aln.fa"))
    names, seqs = names[:9], seqs[:9]
    tree = pc.UnRootedTreeModelInterface(NEWICK, names)
    subst = pc.GTRInterface([float(x) for x in spec["rates"].split(",")], [float(x) for x in spec["freqs"].split(",")])
    site = pc.GammaSiteModelInterface(float(spec["alpha"]), 4, None, None)
    tlk = pc.TreeLikelihoodInterface(list(zip(names, seqs)), tree, subst, site, None)
    before = tlk.log_likelihood()
    p0 = tree.get_parameters()

    d = tree.describe()
    T, N, P = 9, 17, tlk.get_pattern_count()
    left, right, root = np.array(d["left"], dtype=np.int32), np.array(d["right"], dtype=np.int32), int(d["root"])
    lengths = np.array(d["distance"], dtype=np.float64)
    lengths[root] = 0.0
    states = tlk.pattern_states()  # [taxon in alignment order][pattern]
    ev, U, Ui, _ = subst.eigen_system()
    trees = (np.tile(left, (2, 1)), np.tile(right, (2, 1)), np.full(2, root, dtype=np.int32))
    start = np.stack([lengths, lengths * np.random.default_rng(9).uniform(0.5, 2.0, size=N)])
    mask = np.ones((2, N), dtype=np.uint8)
    mask[0, [2, int(right[root])]] = 0
    kw = dict(lower=1e-6, upper=5.0, tolerance=1e-7, max_iterations=50, lnl_tolerance=1e-5, max_passes=20)
    with Engine(T, P, 4, 4, rescale=0) as e:
        e.set_topology(left, right, root)
        e.set_branch_lengths(lengths)
        e.set_eigen(ev, U, Ui)
        e.set_frequencies([float(x) for x in spec["freqs"].split(",")])
        e.set_category_rates(site.rates(), site.proportions())
        e.set_pattern_weights(tlk.pattern_weights())
        for tip in range(T):
            e.set_tip_states(tip, states[names.index(d["name"][tip])])
        own = e.log_likelihood()
        assert abs(own - before) <= 1e-10 * abs(before)  # the two sides hold the same problem
        for m in (None, mask):
            want = e.optimize_branch_lengths(trees, start, m, **kw)
            got = tlk.optimize_branch_lengths(*trees, start, m, **kw)
            for name, a, b in zip(("lengths", "lnl", "initial_lnl", "passes"), got, want):
                assert a.shape == b.shape and np.array_equal(a, b), name
            assert np.all(want[3] > 0) and np.all(want[1] >= want[2]) and abs(want[2][0] - own) <= 1e-10 * abs(own)
    assert np.array_equal(tree.get_parameters(), p0) and tlk.log_likelihood() == before
    with pytest.raises(pc.PhyamdError):
        tlk.optimize_branch_lengths(*trees, start[:, :-1])
