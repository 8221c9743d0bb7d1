"""The restatement of every branch's d lnL/dt and d2 lnL/dt2 (tests/hessian_util.py, what phyamd_branch_hessian_diagonal is checked
against on the GPU), pinned on the CPU: against five-point differences of the oracle's lnL in each branch length, and against the
compiled reference's own single-branch values at the current lengths (tests/golden/<case>/branch_trials.json)."""
import copy
import json
import os

import numpy as np
import pytest

from golden_util import GOLDEN, load, oracle_problem
from gpu_util import random_problem
from hessian_util import branch_hessian_diagonal


def _differences(pb, n):
    """five-point first and second differences of the oracle's lnL in t_n"""
    t = pb.branch_lengths[n]
    h = min(3e-4, 0.1 * t)
    f = []
    for dt in (-2 * h, -h, 0.0, h, 2 * h):
        q = copy.copy(pb)
        q.branch_lengths = pb.branch_lengths.copy()
        q.branch_lengths[n] = t + dt
        f.append(q.log_likelihood()["lnl"])
    d1 = (f[0] - 8 * f[1] + 8 * f[3] - f[4]) / (12 * h)
    d2 = (-f[0] + 16 * f[1] - 30 * f[2] + 16 * f[3] - f[4]) / (12 * h * h)
    return d1, d2


@pytest.mark.parametrize("C,pinv", [(1, None), (2, None), (4, None), (5, None), (4, 0.2)])
@pytest.mark.parametrize("rescale", [0, 1])
def test_restatement_matches_differences_of_lnl(C, pinv, rescale):
    pb = random_problem(T=8, P=60, C=C, seed=5 + C, gaps=0.05, pinv=pinv, rescale=rescale)
    lnl, d1, d2 = branch_hessian_diagonal(pb)
    assert lnl == pytest.approx(pb.log_likelihood()["lnl"], rel=1e-12)
    assert d1[pb.root] == 0.0 and d2[pb.root] == 0.0
    for n in range(pb.N):
        if n == pb.root:
            continue
        f1, f2 = _differences(pb, n)
        assert abs(d1[n] - f1) <= 1e-6 * max(1.0, abs(d1[n])), (n, d1[n], f1)
        assert abs(d2[n] - f2) <= 1e-5 * max(1.0, abs(d2[n])), (n, d2[n], f2)


def test_restatement_under_forced_rescaling_is_the_unscaled_one():
    """deep caterpillar: the rescaled partials differ from the plain ones by per-pattern factors that cancel"""
    plain = random_problem(T=40, P=80, C=4, seed=11, shape="caterpillar", gaps=0.02)
    scaled = copy.copy(plain)
    scaled.rescale = 1
    a, b = branch_hessian_diagonal(plain), branch_hessian_diagonal(scaled)
    assert b[0] == pytest.approx(a[0], rel=1e-12)
    np.testing.assert_allclose(b[1], a[1], rtol=1e-10, atol=1e-8)
    np.testing.assert_allclose(b[2], a[2], rtol=1e-10, atol=1e-6)


@pytest.mark.parametrize("case", ["gtr_g4_t16", "gtr_g4_t24_gaps_tipstates", "wag_g4_t12", "mg94_t8"])
def test_restatement_matches_reference_fixture(case):
    """the compiled reference's d1, d2 of single branches (d2lnldt2_uppper) at the tree's own lengths (trial factor 1.0)"""
    pb = oracle_problem(case, load(case))
    with open(os.path.join(GOLDEN, case, "branch_trials.json")) as f:
        trials = [t for t in json.load(f)["trials"] if t["length"] == pb.branch_lengths[t["node"]]]
    assert len(trials) == 4
    lnl, d1, d2 = branch_hessian_diagonal(pb)
    for tr in trials:
        n = tr["node"]
        assert abs(lnl - tr["lnl"]) <= 1e-10 * abs(tr["lnl"]), tr
        assert abs(d1[n] - tr["d1"]) <= 1e-8 * max(1.0, abs(tr["d1"])), (tr, d1[n])
        assert abs(d2[n] - tr["d2"]) <= 1e-7 * max(1.0, abs(tr["d2"])), (tr, d2[n])
