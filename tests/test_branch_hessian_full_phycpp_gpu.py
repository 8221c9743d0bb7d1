"""GPU: TreeLikelihoodInterface.BranchHessian through the pybind module returns the C ABI's bits: nine taxa of the golden alignment
gtr_g4_t16 under GTR + Gamma(4) on a tree of their own, against an Engine given the object's own patterns, weights, node table and
model."""
import os

import numpy as np
import pytest

from golden_util import GOLDEN, read_fasta, read_spec
from physher_amd.engine import Engine

pytestmark = pytest.mark.gpu

NEWICK = "(((t0:0.05,t3:0.08):0.03,(t5:0.02,(t1:0.07,t8:0.04):0.06):0.05):0.04,((t2:0.09,t7:0.03):0.02,(t4:0.06,t6:0.01):0.07):0.05);"


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
        want_lnl, want_g, want_H = e.branch_hessian()
    got_lnl, got_g, got_H = tlk.branch_hessian()
    assert got_H.shape == (N, N) and np.asarray(got_g).shape == (N,)
    assert got_lnl == want_lnl
    assert np.array_equal(np.asarray(got_g).view(np.uint64), want_g.view(np.uint64))
    assert np.array_equal(np.ascontiguousarray(got_H).view(np.uint64), want_H.view(np.uint64))
    assert np.array_equal(got_H, got_H.T) and not got_H[root].any()
    only_H = tlk.branch_hessian(False)
    assert only_H[1] is None and np.array_equal(only_H[2], got_H)
    after = tlk.log_likelihood()
    assert np.array_equal(tree.get_parameters(), p0) and abs(after - before) <= 1e-10 * abs(before)
