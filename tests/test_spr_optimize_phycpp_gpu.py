"""GPU: TreeLikelihoodInterface.SPROptimize through the pybind module returns the C ABI's bits: test_spr_optimize_gpu's case
t8_random_p65 -- its tree, lengths, sequences and frequencies -- under HKY, against an Engine given the object's own patterns, weights, node
table and model, for every prune node and for a list, and the object's own state afterwards."""
import numpy as np
import pytest

import spr_optimize_util as t
from physher_amd.engine import Engine

pytestmark = pytest.mark.gpu


def _newick(pb, names, n):
    if n < pb.T:
        return f"{names[n]}:{float(pb.branch_lengths[n])!r}"
    inner = f"({_newick(pb, names, int(pb.left[n]))},{_newick(pb, names, int(pb.right[n]))})"
    return inner + (";" if n == pb.root else f":{float(pb.branch_lengths[n])!r}")


def test_eight_taxa_return_the_c_abis_bits():
    from physher_amd import _phycpp_amd as pc
    pb, _ = t.problem("t8_random_p65")
    names = [f"t{i}" for i in range(pb.T)]
    seqs = ["".join("ACGT"[x] for x in pb.tip_states[i]) for i in range(pb.T)]
    tree = pc.UnRootedTreeModelInterface(_newick(pb, names, pb.root), names)
    freqs = [float(x) for x in pb.freqs]
    subst = pc.HKYInterface(2.0, freqs)
    site = pc.ConstantSiteModelInterface(None)
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
    with Engine(T, P, 4, 1, rescale=0) as e:
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
        for prune in (None, np.array([3, 12, 3, 0], dtype=np.int32)):
            want = e.spr_optimize(prune)
            got = tlk.spr_optimize(prune)
            rows = N if prune is None else len(prune)
            assert got[0].shape == want[0].shape == (rows, N, 3) and got[3].shape == want[3].shape == (rows, N)
            for a, c in zip(got[:3], want[:3]):
                assert np.array_equal(a.view(np.uint64), c.view(np.uint64))
            assert np.array_equal(got[3], want[3])
            assert np.any(np.isfinite(want[1])) and np.any(np.isnan(want[1])) and np.any(want[3] > 0)
        few = tlk.spr_optimize(np.array([3], dtype=np.int32), max_passes=1, upper=0.5)
        assert np.all(np.abs(few[3]) <= 1) and np.nanmax(few[0]) <= 0.5
    assert np.array_equal(tree.get_parameters(), p0) and tlk.log_likelihood() == before
    with pytest.raises(pc.PhyamdError):
        tlk.spr_optimize(np.array([3, N], dtype=np.int32))
