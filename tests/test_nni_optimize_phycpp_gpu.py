"""GPU: TreeLikelihoodInterface.NNIOptimize through the pybind module returns the C ABI's bits: nine taxa of the golden alignment
gtr_g4_t16 under GTR + Gamma(4) on a tree of their own (tests/test_nni_phycpp_gpu.py's), against an Engine given the object's own
patterns, weights, node table and model, with and without start lengths, and the object's own state afterwards."""
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
    cand = [v for v in range(T, N) if v != root]
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
        start = lengths[None, :] * np.random.default_rng(9).uniform(0.5, 2.0, size=(3, N))
        for sl in (None, start):
            want = e.nni_optimize(sl, lower=1e-6, upper=5.0, tolerance=1e-7, max_iterations=50)
            got = tlk.nni_optimize(sl, lower=1e-6, upper=5.0, tolerance=1e-7, max_iterations=50)
            for name, a, b in zip(("lengths", "lnl", "d1", "d2", "iterations"), got, want):
                assert a.shape == (3, N) and np.array_equal(a, b, equal_nan=True), name
            assert np.all(np.isfinite(want[1][:, cand])) and np.all(want[4][:, cand] > 0)
            # row 0 is the engine's tree with one branch optimised (a branch shorter than `lower` is first moved there)
            inside = [v for v in cand if lengths[v] >= 1e-6]
            assert np.all(want[1][0, inside] >= own - 1e-10 * abs(own))
    assert np.array_equal(tree.get_parameters(), p0) and tlk.log_likelihood() == before
    with pytest.raises(pc.PhyamdError):
        tlk.nni_optimize(start[:, :-1])
