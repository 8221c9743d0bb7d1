"""GPU: TreeLikelihoodInterface.PatternLogLikelihoodsTrees through the pybind module returns the C ABI's bits at 16 taxa x 238
patterns x 4 categories: the golden alignment gtr_g4_t16 cut to the prefix that has 238 patterns, against an Engine given the object's
own patterns, weights, node table and model -- the NNI neighbourhood of the tree model's tree and that tree itself, with and
without replicates and rows -- and the object's own state afterwards."""
import os

import numpy as np
import pytest

from golden_util import GOLDEN, read_fasta, read_spec
from physher_amd import resampling
from physher_amd.engine import Engine

pytestmark = pytest.mark.gpu


class _Tree:
    pass


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_sixteen_taxa_return_the_c_abis_bits():
    from physher_amd import _phycpp_amd as pc
    from test_tree_batch_gpu import Items, _nni_neighbourhood
    case = "gtr_g4_t16"
    spec = read_spec(case)
    names, seqs = read_fasta(os.path.join(GOLDEN, case, "aln.fa"))
    columns = list(zip(*seqs))
    sites = max(L for L in range(1, len(columns) + 1) if len(set(columns[:L])) == 238)
    with open(os.path.join(GOLDEN, case, "tree.nwk")) as f:
        tree = pc.UnRootedTreeModelInterface(f.read().strip(), names)
    freqs = [float(x) for x in spec["freqs"].split(",")]
    subst = pc.GTRInterface([float(x) for x in spec["rates"].split(",")], freqs)
    site = pc.GammaSiteModelInterface(float(spec["alpha"]), 4, None, None)
    tlk = pc.TreeLikelihoodInterface([(n, s[:sites]) for n, s in zip(names, seqs)], tree, subst, site, None)
    before = tlk.log_likelihood()
    p0 = tree.get_parameters()

    d = tree.describe()
    T, N, P = 16, 31, tlk.get_pattern_count()
    assert P == 238
    own = _Tree()
    own.T, own.N = T, N
    own.left, own.right, own.root = np.array(d["left"], dtype=np.int32), np.array(d["right"], dtype=np.int32), int(d["root"])
    own.branch_lengths = np.array(d["distance"], dtype=np.float64)
    own.branch_lengths[own.root] = 0.0
    items = Items(_nni_neighbourhood(own) + [(own.left, own.right, own.root, own.branch_lengths)])
    W = resampling.bootstrap_weights(tlk.pattern_weights(), 5, np.random.default_rng(16))
    states = tlk.pattern_states()  # [taxon in alignment order][pattern]
    ev, U, Ui, _ = subst.eigen_system()
    with Engine(T, P, 4, 4, rescale=0) as e:
        e.set_topology(own.left, own.right, own.root)
        e.set_branch_lengths(own.branch_lengths)
        e.set_eigen(ev, U, Ui)
        e.set_frequencies(freqs)
        e.set_category_rates(site.rates(), site.proportions())
        e.set_pattern_weights(tlk.pattern_weights())
        for tip in range(T):
            e.set_tip_states(tip, states[names.index(d["name"][tip])])
        assert abs(e.log_likelihood() - before) <= 1e-10 * abs(before)  # the two sides hold the same problem
        want = e.pattern_log_likelihoods_trees(*items.args(), replicate_weights=W)
    got = tlk.pattern_log_likelihoods_trees(*items.args(), replicate_weights=W)
    assert got[0].shape == (len(items),) and got[1].shape == (len(items), P) and got[2].shape == (5, len(items))
    for a, b in zip(got, want):
        assert np.array_equal(_bits(a), _bits(b))
    assert abs(got[0][-1] - before) <= 1e-10 * abs(before)  # the tree model's own tree
    lnl, rows, rep = tlk.pattern_log_likelihoods_trees(*items.args(), want_patterns=False)
    assert rows is None and rep is None and np.array_equal(_bits(lnl), _bits(want[0]))
    assert np.array_equal(tree.get_parameters(), p0) and tlk.log_likelihood() == before
    with pytest.raises(pc.PhyamdError):
        tlk.pattern_log_likelihoods_trees(*items.args(), replicate_weights=W[:, :-1])
    bad = W.copy()
    bad[2, 7] = -1.0
    with pytest.raises(pc.PhyamdError):
        tlk.pattern_log_likelihoods_trees(*items.args(), replicate_weights=bad)
