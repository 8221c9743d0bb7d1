"""GPU: TreeLikelihoodInterface.SPROptimizeGeneral through the pybind module returns the C ABI's bits on
t9_random_p130_c8_sets of tests/test_spr_general_gpu.py: that case's tree, lengths and 20-state cells, the patterns written out as
sequences by their weights (a sequence has no letter for an ambiguity set: the case's set cells are written as unknown, like its
gaps; the engine's sets are covered through the C ABI there) under a general 20-state model + Gamma(8), against an Engine given the
object's own patterns, weights, node table and model; all rows and a prune list, and the object's own state afterwards."""
import numpy as np
import pytest

from physher_amd.engine import Engine
from spr_optimize_general_util import problem
from test_spr_optimize_phycpp_gpu import _newick

pytestmark = pytest.mark.gpu
LETTERS = "ARNDCQEGHILKMFPSTWYV"


def test_nine_taxa_return_the_c_abis_bits():
    from physher_amd import _phycpp_amd as pc
    pb = problem("t9_random_p130_c8_sets")[0]
    part = np.asarray(pb.tip_partials)  # [T][P][20] 0/1: one member is a state, anything else is written as unknown
    letter = lambda row: LETTERS[int(np.argmax(row))] if row.sum() == 1 else "-"

    names = [f"t{i}" for i in range(pb.T)]
    columns = np.repeat(np.arange(pb.P), pb.weights.astype(int))
    seqs = ["".join(letter(part[t, k]) for k in columns) for t in range(pb.T)]
    rng = np.random.default_rng(3)
    freqs = list(rng.dirichlet(np.full(20, 5.0)))
    rates = list(rng.uniform(0.5, 3.0, size=190))
    dt = pc.GeneralDataTypeInterface(list(LETTERS))
    tree = pc.UnRootedTreeModelInterface(_newick(pb, names, pb.root), names)
    subst = pc.GeneralSubstitutionModelInterface(dt, rates, freqs, list(range(190)), True)
    site = pc.GammaSiteModelInterface(0.6, 8, None, None)
    tlk = pc.TreeLikelihoodInterface(list(zip(names, seqs)), tree, subst, site, None)
    before = tlk.log_likelihood()
    p0 = tree.get_parameters()

    d = tree.describe()
    T, N, P = pb.T, pb.N, tlk.get_pattern_count()
    left, right, root = np.array(d["left"], dtype=np.int32), np.array(d["right"], dtype=np.int32), int(d["root"])
    lengths = np.array(d["distance"], dtype=np.float64)
    lengths[root] = 0.0
    states = tlk.pattern_states()  # [taxon in alignment order][pattern]
    assert np.any(states >= 20) and P > 112  # unknown cells; the last workgroup's first tile
    same = lambda a, b: np.array_equal(a.view(np.uint64), b.view(np.uint64))
    with Engine(T, P, 20, 8, rescale=0) as e:
        e.set_topology(left, right, root)
        e.set_branch_lengths(lengths)
        e.set_eigen(*subst.eigen_system()[:3])
        e.set_frequencies(freqs)
        e.set_category_rates(site.rates(), site.proportions())
        e.set_pattern_weights(tlk.pattern_weights())
        for tip in range(T):
            e.set_tip_states(tip, states[names.index(d["name"][tip])])
        own = e.log_likelihood()
        assert abs(own - before) <= 1e-10 * abs(before)  # the two sides hold the same problem
        prune = np.array([5, 0, root, 9, 5], dtype=np.int32)
        for pr in (None, prune):
            want = e.spr_optimize_general(pr)
            got = tlk.spr_optimize_general(pr)
            rows = N if pr is None else len(pr)
            assert got[0].shape == (rows, N, 3) and got[1].shape == got[2].shape == got[3].shape == (rows, N) and got[3].dtype == np.int32
            assert same(got[0], want[0]) and same(got[1], want[1]) and same(got[2], want[2]) and np.array_equal(got[3], want[3])
            assert np.any(np.isfinite(want[1])) and np.any(np.isnan(want[1])) and np.any(want[3] > 0)
        want = e.spr_optimize_general(prune, lower=0.01, upper=2.0, tolerance=1e-6, max_iterations=7, lnl_tolerance=1e-3, max_passes=2)  # the arguments arrive in order
        got = tlk.spr_optimize_general(prune, lower=0.01, upper=2.0, tolerance=1e-6, max_iterations=7, lnl_tolerance=1e-3, max_passes=2)
        assert same(got[0], want[0]) and same(got[1], want[1]) and same(got[2], want[2]) and np.array_equal(got[3], want[3])
        assert np.all(np.abs(want[3]) <= 2) and np.nanmax(want[0]) <= 2.0 and np.nanmin(want[0]) >= 0.01
    assert np.array_equal(tree.get_parameters(), p0) and abs(tlk.log_likelihood() - before) <= 1e-10 * abs(before)
    with pytest.raises(pc.PhyamdError):
        tlk.spr_optimize_general(np.array([N], dtype=np.int32))
    with pytest.raises(pc.PhyamdError):  # the 4-state call keeps refusing 20 states
        tlk.spr_optimize()
