"""CPU: pin the substitution-model gradient (calculate_dlnl_dQ) before the GPU path is trusted with it.

Two pieces are checked against `gradient_all` of the compiled reference (tests/golden/*, flags TREE|SITE|SUBSTITUTION_MODEL,
i.e. constrained-value derivatives: 5 GTR rates / kappa, then the 4 frequencies as free coordinates):
  * the host library's dQ/dtheta (physher_amd/csrc/host/models.cpp, product code, no GPU needed), and
  * the oracle's numpy restatement of the branch sum and of the root-frequency term (oracle/phyoracle.py).
"""
import numpy as np
import pytest

from golden_util import UNROOTED_CASES, load, oracle_problem, read_spec
from oracle import phyoracle as po
from physher_amd import _phycpp_amd as pc


def subst_cases():
    out = []
    for c in UNROOTED_CASES:
        spec = read_spec(c)
        if spec["datatype"] == "nucleotide" and spec["model"] in ("gtr", "hky"):
            out.append(c)
    return out


def model_from_spec(spec, freqs):
    if spec["model"] == "hky":
        return pc.HKYInterface(float(spec["rates"]), list(freqs))
    return pc.GTRInterface([float(x) for x in spec["rates"].split(",")], list(freqs))


def reference_tail(gold):
    """[rates..., frequencies...] of gradient_all; the tree block is node_count long, then the site-model block."""
    assert gold["gradient_all_flags"] & 4
    n_rates = {"gtr": 5, "hky": 1}[gold["_model"]]
    return gold["gradient_all"][-(n_rates + 4):], n_rates


@pytest.mark.parametrize("case", subst_cases())
def test_parameter_gradient_matches_reference(case):
    gold = load(case)
    spec = read_spec(case)
    gold["_model"] = spec["model"]
    ref, n_rates = reference_tail(gold)
    m = model_from_spec(spec, gold["frequencies"])
    dQ = m.rate_matrix_derivatives()
    assert dQ.shape == (n_rates + 4, 4, 4)
    np.testing.assert_allclose(dQ.sum(axis=2), 0.0, atol=1e-13)  # rows of Q sum to 0 for every parameter value
    pb = oracle_problem(case, gold)
    lnl, g = po.parameter_gradient(pb, dQ)
    assert abs(lnl - gold["lnl"]) <= 1e-9 * abs(gold["lnl"])
    g[n_rates:] += po.root_frequency_term(pb)
    # the reference accumulates per-pattern sums in a different order and its HKY P(t) is closed-form
    np.testing.assert_allclose(g, ref, rtol=2e-8, atol=1e-7)


def test_rate_matrix_derivatives_are_derivatives():
    """dQ/dtheta against central differences of the host Q, all model families including a 6-rate simplex GTR."""
    f = np.array([0.3, 0.2, 0.15, 0.35])
    r5 = np.array([1.2, 3.1, 0.7, 0.9, 2.8])
    r6 = np.array([0.1, 0.3, 0.05, 0.15, 0.25, 0.15])
    dt = pc.GeneralDataTypeInterface(["A", "C", "G", "T"])
    makers = {
        "hky": lambda r, fr: pc.HKYInterface(float(r[0]), list(fr)),
        "gtr5": lambda r, fr: pc.GTRInterface(list(r), list(fr)),
        "gtr6": lambda r, fr: pc.GTRInterface(list(r), list(fr)),
        "general": lambda r, fr: pc.GeneralSubstitutionModelInterface(dt, list(r), list(fr), [0, 1, 0, 2, 1, 0], True),
        "general_raw": lambda r, fr: pc.GeneralSubstitutionModelInterface(dt, list(r), list(fr), [0, 1, 0, 2, 1, 0], False),
    }
    rates = {"hky": np.array([2.5]), "gtr5": r5, "gtr6": r6, "general": np.array([1.0, 2.0, 0.5]), "general_raw": np.array([1.0, 2.0, 0.5])}
    h = 1e-6
    for name, make in makers.items():
        r = rates[name]
        dQ = make(r, f).rate_matrix_derivatives()
        assert dQ.shape[0] == len(r) + 4
        Qof = lambda rr, ff: make(rr, ff).eigen_system()[3]
        for i in range(len(r)):
            e = np.zeros(len(r))
            e[i] = h
            fd = (Qof(r + e, f) - Qof(r - e, f)) / (2 * h)
            np.testing.assert_allclose(dQ[i], fd, atol=2e-9, err_msg=f"{name} rate {i}")
        for i in range(4):  # frequencies move as free coordinates (the reference's grad_wrt_reparam = false convention)
            e = np.zeros(4)
            e[i] = h
            fd = (Qof(r, f + e) - Qof(r, f - e)) / (2 * h)
            np.testing.assert_allclose(dQ[len(r) + i], fd, atol=2e-9, err_msg=f"{name} freq {i}")
    assert pc.JC69Interface().rate_matrix_derivatives().shape[0] == 0


# Parameter points at which the rate matrix has a repeated or nearly repeated eigenvalue.  "GTR with all rates 1 and empirical
# frequencies", where a GTR fit usually starts, is F81: one threefold eigenvalue.  K80 has a double one.  The host library's eigen
# solver returns them split by an ulp or so, and the reference's divided difference (e^{l_a t} - e^{l_b t}) / (l_a - l_b) with its
# exact l_a == l_b test (substmodel.c:478) is then rounding noise: tens of percent of dP/dtheta.
DEGENERATE_POINTS = {
    "f81_start": ("gtr", [1.0, 1.0, 1.0, 1.0, 1.0], [0.1, 0.2, 0.3, 0.4]),
    "k80": ("hky", [2.0], [0.25, 0.25, 0.25, 0.25]),
    "near_jc69": ("gtr", [1.0 + 1.0e-9, 1.0 + 2.5e-9, 1.0 + 1.7e-9, 1.0 + 2.2e-9, 1.0 + 1.3e-9], [0.25, 0.25, 0.25, 0.25]),
}
DEGENERATE_CASE = "gtr_g4_t16"  # the data and tree of a fixture; the model is the point's


def make_model(kind, rates, freqs):
    return pc.HKYInterface(float(rates[0]), list(freqs)) if kind == "hky" else pc.GTRInterface(list(rates), list(freqs))


def degenerate_problem(point, gold=None, rates=None, freqs=None):
    """(oracle problem, model) at a point of DEGENERATE_POINTS, or at other parameter values of its model"""
    kind, r0, f0 = DEGENERATE_POINTS[point]
    gold = gold or load(DEGENERATE_CASE)
    m = make_model(kind, r0 if rates is None else rates, f0 if freqs is None else freqs)
    ev, U, Ui, _ = m.eigen_system()
    g = dict(gold)
    g.update(eval=ev, evec=U, ivec=Ui, frequencies=np.array(f0 if freqs is None else freqs, dtype=np.float64))
    return oracle_problem(DEGENERATE_CASE, g), m


def degenerate_reference(point):
    """the oracle's gradient in [rates..., frequencies...] at a point: the branch sum with the host library's own dQ/dtheta plus the
    root-frequency term"""
    pb, m = degenerate_problem(point)
    n_rates = len(DEGENERATE_POINTS[point][1])
    _, grad = po.parameter_gradient(pb, m.rate_matrix_derivatives())
    grad[n_rates:] += po.root_frequency_term(pb)
    return pb, m, grad


@pytest.mark.parametrize("point", list(DEGENERATE_POINTS))
def test_oracle_parameter_gradient_at_repeated_eigenvalues(point):
    """The yardstick is a central difference of the oracle's lnL in each free parameter at two step sizes, h and h / 2, with one
    Richardson step, (4 D(h / 2) - D(h)) / 3.  |D(h / 2) - D(h)| is the yardstick's own error before that step; the bound is ten
    times it plus 1e-9 * max(1, |g|inf).  lnL needs no dP/dtheta, so the difference knows nothing of the divided difference."""
    kind, r0, f0 = DEGENERATE_POINTS[point]
    r0, f0 = np.array(r0), np.array(f0)
    gold = load(DEGENERATE_CASE)
    pb, m, grad = degenerate_reference(point)
    ev = m.eigen_system()[0]
    print(f"{point}: eigenvalues {ev!r}, smallest gap {np.diff(np.sort(ev)).min():.3e}")
    assert np.diff(np.sort(ev)).min() < 1e-8

    def lnl_of(r, f):
        return degenerate_problem(point, gold, r, f)[0].log_likelihood()["lnl"]

    h = 1e-4
    scale = 1e-9 * max(1.0, np.abs(grad).max())
    for i in range(len(r0) + 4):
        def central(step):
            e = np.zeros(len(r0) + 4)
            e[i] = step
            return (lnl_of(r0 + e[:len(r0)], f0 + e[len(r0):]) - lnl_of(r0 - e[:len(r0)], f0 - e[len(r0):])) / (2 * step)
        coarse, fine = central(h), central(h / 2)
        want, spread = (4 * fine - coarse) / 3, abs(fine - coarse)
        print(f"{point} parameter {i}: gradient {grad[i]!r} yardstick {want!r} spread {spread:.3e} bound {10 * spread + scale:.3e} off by {abs(grad[i] - want):.3e}")
        assert abs(grad[i] - want) <= 10 * spread + scale, (point, i, grad[i], want, spread)


def test_oracle_parameter_gradient_is_a_derivative():
    """The oracle restatement against central differences of the oracle's own lnL (GTR rates and frequencies)."""
    case = "gtr_g4_t16"
    gold = load(case)
    spec = read_spec(case)
    r0 = np.array([float(x) for x in spec["rates"].split(",")])
    f0 = gold["frequencies"].copy()

    def lnl_of(r, f):
        m = pc.GTRInterface(list(r), list(f))
        ev, U, Ui, _ = m.eigen_system()
        g = dict(gold)
        g.update(eval=ev, evec=U, ivec=Ui, frequencies=f)
        return oracle_problem(case, g).log_likelihood()["lnl"]

    m = pc.GTRInterface(list(r0), list(f0))
    ev, U, Ui, _ = m.eigen_system()
    g = dict(gold)
    g.update(eval=ev, evec=U, ivec=Ui)
    pb = oracle_problem(case, g)
    _, grad = po.parameter_gradient(pb, m.rate_matrix_derivatives())
    grad[5:] += po.root_frequency_term(pb)
    h = 1e-5
    for i in range(5):
        e = np.zeros(5)
        e[i] = h
        fd = (lnl_of(r0 + e, f0) - lnl_of(r0 - e, f0)) / (2 * h)
        assert abs(grad[i] - fd) < 1e-5 * max(1.0, abs(fd)), (i, grad[i], fd)
    for i in range(4):
        e = np.zeros(4)
        e[i] = h
        fd = (lnl_of(r0, f0 + e) - lnl_of(r0, f0 - e)) / (2 * h)
        assert abs(grad[5 + i] - fd) < 1e-5 * max(1.0, abs(fd)), (i, grad[5 + i], fd)
