"""CPU: the definition behind phyamd_state_posteriors, from the oracle alone (tests/state_posteriors_util.py).  J[n][k][j] is the
site likelihood with node n held in state j, so sum_j J[n][k][j] = L_k at every node, rescaled or not; and the cases of
tests/test_state_posteriors_gpu.py leave no cell out of the comparison of states: the oracle's top-two posterior gap is at least
1e-6 everywhere (a condition on the inputs, re-checked here whenever a seed or a shape changes)."""
import numpy as np
import pytest

from state_posteriors_util import CASES, GAP, case, oracle_state_posteriors


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_sum_over_states_is_the_site_likelihood(name):
    pb = case(name)[0]
    J, plk = oracle_state_posteriors(pb)
    L = J.sum(axis=2)
    # (per-pattern factors of a rescaled evaluation are common to the nodes: the same L at every node)
    assert np.abs(L / L[pb.root][None, :] - 1.0).max() <= 1e-12 * pb.S
    assert np.abs(L[pb.root] / np.exp(plk) - 1.0).max() <= 1e-12


@pytest.mark.parametrize("name", sorted(CASES))
def test_no_cell_is_left_out_of_the_comparison_of_states(name):
    gap = case(name)[3]
    print(f"{name}: smallest top-two gap {gap.min():.3e}")
    assert np.count_nonzero(gap < GAP) == 0


def test_folded_uppers_leave_no_cell_out_either():
    pb = case("gaps")[0]
    J, _ = oracle_state_posteriors(pb, fold=True)
    top = np.sort(J / J.sum(axis=2, keepdims=True), axis=2)
    assert (top[:, :, -1] - top[:, :, -2]).min() >= GAP
