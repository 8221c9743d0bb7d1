"""GPU: the substitution-parameter gradient at repeated and nearly repeated eigenvalues.

dP/dtheta = U (B o F) U^-1 with F_ab = (e^{l_a t} - e^{l_b t}) / (l_a - l_b).  The two 4-state routes of phyamd_parameter_gradient
(k_eigen_weights: the walk; k_parameter_matrices: the level kernels) formed that quotient as written, with an exact l_a != l_b
test, as the reference does (substmodel.c:478).  An eigen solver returns a repeated eigenvalue split by an ulp, the test is then
true and the quotient is rounding noise: predicted from CPU arithmetic alone (tests/test_parameter_matrix_oracle.py) to be wrong by
tens of percent at K80 and F81 parameter values and by 1e-8 to 1e-3 near JC69.  Both kernels now call exp_divided_difference
(phyamd_device.inc: e^{hi t} (1 - e^{-(hi - lo) t}) / (hi - lo) with expm1), as the 20 / 60 / 61-state route does.

Every case is held against the oracle, whose parameter_matrix tests/test_parameter_matrix_oracle.py pins on a formula without an
eigen system: the parameter gradient at 1e-9 * max(1, |ref|inf), the per-category gradient and lnL of the same call at the
tolerances of DESIGN.md section 4.  The six models of tests/degenerate_eigen_util.py (two of them controls with separated
eigenvalues), 24 x 130 x 4 and 9 x 65 x 2, plain and RESCALE_ALWAYS, on the walk and on the level kernels (asserted from the
profile).  With the parent commit's library the k80, f81 and gtr_near_jc69 cases fail on both routes (PHYAMD_LIB selects a library).
"""
import functools
import os

import numpy as np
import pytest

import degenerate_eigen_util as du
import invalidation_util as iu
from golden_util import GOLDEN, load, read_fasta, read_spec
from gpu_util import engine_from_problem, random_problem
from oracle import phyoracle as po
from physher_amd.engine import RESCALE_ALWAYS, RESCALE_NEVER

pytestmark = pytest.mark.gpu

SHAPES = {"t24": (24, 130, 4), "t9": (9, 65, 2)}


@functools.lru_cache(maxsize=None)
def _case(name, shape, rescale):
    """the problem, its dQ and everything the oracle says, once per module"""
    pb = du.problem(name, *SHAPES[shape], rescale=rescale)
    dQ = du.random_dq(4, 3, seed=11)
    lnl, pg = po.parameter_gradient(pb, dQ)
    ref = pb.gradient()
    assert ref["rescaled"] == bool(rescale) and lnl == ref["lnl"]
    return pb, dQ, pg, ref


def _check(e, pg_ref, ref, what):
    lnl, cg, pg = e.parameter_gradient()
    pscale, gscale = max(1.0, np.abs(pg_ref).max()), max(1.0, np.abs(ref["cat_grad"]).max())
    print(f"{what}: parameter gradient {pg!r} (oracle {pg_ref!r}) off by {np.abs(pg - pg_ref).max() / (1e-9 * pscale):.3e} of the bound; "
          f"gradient {np.abs(cg - ref['cat_grad']).max() / (1e-9 * gscale):.3e}; lnL {abs(lnl - ref['lnl']) / (1e-10 * abs(ref['lnl'])):.3e}")
    assert np.abs(pg - pg_ref).max() <= 1e-9 * pscale
    assert np.abs(cg - ref["cat_grad"]).max() <= 1e-9 * gscale
    assert abs(lnl - ref["lnl"]) <= 1e-10 * abs(ref["lnl"])
    return pg


@pytest.mark.parametrize("route", ["walk", "levels"])
@pytest.mark.parametrize("rescale", [0, 1])
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("name", du.MODELS)
def test_parameter_gradient_four_states(name, shape, rescale, route):
    pb, dQ, pg_ref, ref = _case(name, shape, rescale)
    with engine_from_problem(pb, rescale=RESCALE_ALWAYS if rescale else RESCALE_NEVER) as e:
        e.set_profiling(True)
        if route == "levels":
            e.set_keep_partials(True)
        e.set_rate_matrix_derivatives(dQ)
        pg = _check(e, pg_ref, ref, f"{name} {shape} rescale={rescale} {route}")
        p = e.profile()
        print(f"{p['lower_launches']} post-order and {p['upper_launches']} pre-order launches; {iu.levels(pb)} levels")
        assert iu.levels(pb) >= 4
        if route == "walk":  # k_upper4_walk in its PARAMS form, fed by k_eigen_weights
            assert p["upper_launches"] in (1, 2), "the pre-order pass did not run a tree walk"
        else:  # one launch per level, fed by k_parameter_matrices
            assert p["upper_launches"] >= 4, "the pre-order pass did not run the level kernels"
        assert np.array_equal(e.parameter_gradient()[2], pg)  # nothing changed: the same bits


def test_twenty_states_with_a_nineteenfold_eigenvalue():
    """the general route (k_param_outer_gen), which had the expm1 form before and shares exp_divided_difference now: equal
    exchangeabilities at 20 states"""
    pb = random_problem(12, 40, 2, seed=1220, S=20, gaps=0.03)
    pb.eval, pb.evec, pb.ivec, pb.freqs = (np.ascontiguousarray(a) for a in du.equal_exchangeabilities(20, 3))
    gaps = np.diff(np.sort(pb.eval))
    print("eigenvalue gaps", gaps)
    assert np.count_nonzero(gaps < 1e-13) == 18
    dQ = du.random_dq(20, 3, seed=12)
    _, pg_ref = po.parameter_gradient(pb, dQ)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        e.set_rate_matrix_derivatives(dQ)
        _check(e, pg_ref, pb.gradient(), "20 states, equal exchangeabilities")


def test_gtr_at_the_f81_start_through_the_phycpp_classes():
    """alignment + newick + GTRInterface(all rates 1, empirical frequencies) in, the substitution block of the gradient out: held
    against the oracle at the host library's own eigen system and dQ/dtheta (tests/test_subst_gradient_oracle.py pins that
    yardstick on differences of lnL), 1e-9 * max(1, |ref|inf)"""
    from physher_amd import _phycpp_amd as pc
    from test_subst_gradient_oracle import DEGENERATE_CASE, DEGENERATE_POINTS, degenerate_reference
    _, rates, freqs = DEGENERATE_POINTS["f81_start"]
    pb, m, want = degenerate_reference("f81_start")
    gold = load(DEGENERATE_CASE)
    names, seqs = read_fasta(os.path.join(GOLDEN, DEGENERATE_CASE, "aln.fa"))
    with open(os.path.join(GOLDEN, DEGENERATE_CASE, "tree.nwk")) as f:
        tree = pc.UnRootedTreeModelInterface(f.read().strip(), names)
    subst = pc.GTRInterface(list(rates), list(freqs))
    spec = read_spec(DEGENERATE_CASE)
    assert spec.get("sitedist", "gamma") == "gamma" and "pinv" not in spec and "mu" not in spec
    site = pc.GammaSiteModelInterface(float(spec["alpha"]), int(spec["categories"]), None, None)
    assert pb.C == int(spec["categories"]) and gold["pattern_count"] == pb.P
    tlk = pc.TreeLikelihoodInterface(list(zip(names, seqs)), tree, subst, site, None, use_tip_states=spec["tipstates"] == "1")
    lnl = tlk.log_likelihood()
    ref_lnl = pb.log_likelihood()["lnl"]
    tlk.request_gradient([pc.TreeLikelihoodGradientFlags.SUBSTITUTION_MODEL])
    g = tlk.gradient()
    scale = max(1.0, np.abs(want).max())
    print(f"lnL {lnl!r} (oracle {ref_lnl!r}); substitution block {g!r} (oracle {want!r}) off by {np.abs(g - want).max() / (1e-9 * scale):.3e} of the bound")
    assert abs(lnl - ref_lnl) <= 1e-10 * abs(ref_lnl)
    assert g.shape == want.shape and np.abs(g - want).max() <= 1e-9 * scale
