"""GPU: TreeLikelihoodInterface.LogLikelihoodTrees / GradientTrees through the pybind module at 16 taxa x 238 patterns x 4
categories: the NNI neighbourhood of the tree model's tree and that tree itself against the CPU oracle with the branch epilogue
applied (lnL 1e-10 relative, gradient 1e-9 * max(1, max|g|)), the object's own state afterwards, and the refused node-height
request of a time tree."""
import os

import numpy as np
import pytest

from golden_util import GOLDEN, load, read_fasta, read_spec
from test_phycpp_gpu import _fluA
from test_tree_batch_gpu import Items, _nni_neighbourhood, _oracle

pytestmark = pytest.mark.gpu


def _t16_p238(pc):
    """the tree, model and tree likelihood of the golden case gtr_g4_t16 on the longest prefix of its alignment that has 238 site
    patterns (each further site adds one pattern or none, so the count is reached exactly), and the oracle Problem of the same
    data: the object's own patterns and weights by tip id, the case's model and tree"""
    from oracle import phyoracle as po
    case = "gtr_g4_t16"
    gold, spec = load(case), read_spec(case)
    names, seqs = read_fasta(os.path.join(GOLDEN, case, "aln.fa"))
    columns = list(zip(*seqs))
    sites = max(L for L in range(1, len(columns) + 1) if len(set(columns[:L])) == 238)
    with open(os.path.join(GOLDEN, case, "tree.nwk")) as f:
        tree = pc.UnRootedTreeModelInterface(f.read().strip(), names)
    subst = pc.GTRInterface([float(x) for x in spec["rates"].split(",")], list(map(float, gold["frequencies"])))
    site = pc.GammaSiteModelInterface(float(spec["alpha"]), int(spec["categories"]), None, None)
    tlk = pc.TreeLikelihoodInterface([(n, s[:sites]) for n, s in zip(names, seqs)], tree, subst, site, None)
    states = tlk.pattern_states()[gold["mapping"][: gold["tip_count"]]]  # tip id -> sequence index
    pb = po.Problem(gold["left"], gold["right"], gold["root"], tlk.pattern_weights(), gold["eval"], gold["evec"], gold["ivec"],
                    gold["frequencies"], gold["cat_rates"], gold["cat_proportions"], gold["distance"], tip_states=states,
                    tip_partials=po.state_partials("nucleotide", 4, states), rescale=2)
    assert pb.weights.sum() == sites
    return gold, tree, tlk, pb


def test_trees_against_the_oracle():
    from oracle import phyoracle as po
    from physher_amd import _phycpp_amd as pc
    gold, tree, tlk, pb = _t16_p238(pc)
    assert (pb.T, pb.P, pb.C) == (16, 238, 4) and tlk.get_pattern_count() == 238
    tlk.request_gradient([pc.TreeLikelihoodGradientFlags.TREE_HEIGHT])
    p0 = tree.get_parameters()
    before = tlk.log_likelihood()
    items = Items(_nni_neighbourhood(pb) + [(pb.left, pb.right, pb.root, pb.branch_lengths)])
    lnl, g = tlk.gradient_trees(*items.args())
    assert lnl.shape == (len(items),) and g.shape == (len(items), pb.N)
    lo = tlk.log_likelihood_trees(*items.args())
    assert np.array_equal(lo, lnl)
    for b in range(len(items)):
        ref = _oracle(pb, items, b)
        want = po.branch_gradient_from_cat(ref["cat_grad"], gold["cat_rates_without_mu"], gold["cat_proportions"])
        print(f"item {b}: lnL {lnl[b]!r} oracle {ref['lnl']!r}  max|dg| {np.abs(g[b] - want).max():.3e}")
        assert abs(lnl[b] - ref["lnl"]) <= 1e-10 * abs(ref["lnl"]), b
        assert np.abs(g[b] - want).max() <= 1e-9 * max(1.0, np.abs(want).max()), b
    assert abs(lnl[-1] - before) <= 1e-10 * abs(before)  # the tree model's own tree
    assert np.array_equal(tree.get_parameters(), p0) and tlk.log_likelihood() == before
    with pytest.raises(pc.PhyamdError):
        tlk.gradient_trees(items.left[:, :-1], items.right[:, :-1], items.roots, items.bl[:, :-1])


def test_node_height_request_is_refused():
    from physher_amd import _phycpp_amd as pc
    from physher_amd import synth
    tree, clock, tlk = _fluA(pc, include_jacobian=False)
    tlk.request_gradient([pc.TreeLikelihoodGradientFlags.TREE_HEIGHT])
    t = synth.random_tree(69, np.random.default_rng(1), shape="caterpillar")
    args = (t.left[None, :], t.right[None, :], np.array([t.root], dtype=np.int32), t.length[None, :])
    before = tlk.log_likelihood()
    with pytest.raises(pc.PhyamdError):
        tlk.gradient_trees(*args)
    assert np.isfinite(tlk.log_likelihood_trees(*args)[0])  # lnL alone differentiates nothing
    assert tlk.log_likelihood() == before
