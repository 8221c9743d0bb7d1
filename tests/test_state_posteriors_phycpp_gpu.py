"""GPU: TreeLikelihoodInterface.StatePosteriors / SiteRatePosteriors through the pybind module return the C ABI's bits: nine taxa
of the golden alignment gtr_g4_t16 under GTR + Gamma(4) on a tree of their own, against an Engine given the object's own patterns,
weights, node table and model, for every node and for a list."""
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
        want_R, want_mean = e.site_rate_posteriors()
        got_R, got_mean = tlk.site_rate_posteriors()
        assert got_R.shape == (P, 4) and np.array_equal(got_R.view(np.uint64), want_R.view(np.uint64))
        assert np.array_equal(np.asarray(got_mean).view(np.uint64), want_mean.view(np.uint64))
        for nodes in (None, np.array([3, 12, 3, 0, root], dtype=np.int32)):
            want_post, want_states = e.state_posteriors(nodes)
            got_post, got_states = tlk.state_posteriors(nodes)
            count = N if nodes is None else len(nodes)
            assert got_post.shape == want_post.shape == (count, P, 4) and got_states.shape == (count, P) and got_states.dtype == np.uint8
            assert np.array_equal(got_post.view(np.uint64), want_post.view(np.uint64)) and np.array_equal(got_states, want_states)
            assert np.abs(want_post.sum(axis=2) - 1.0).max() <= 1e-12
        only_states = tlk.state_posteriors(None, False, True)
        assert only_states[0] is None and np.array_equal(only_states[1], e.state_posteriors()[1])
    after = tlk.log_likelihood()
    assert np.array_equal(tree.get_parameters(), p0) and abs(after - before) <= 1e-10 * abs(before)
    with pytest.raises(pc.PhyamdError):
        tlk.state_posteriors(np.array([3, N], dtype=np.int32))
