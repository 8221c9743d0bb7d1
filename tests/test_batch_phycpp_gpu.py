"""GPU: TreeLikelihoodInterface.LogLikelihoodBatch / GradientBatch through the pybind module against a loop of SetParameters +
LogLikelihood / Gradient on a second, identical object (1e-9 relative): an unrooted tree, a reparameterized time tree with a strict
clock (Jacobian on and off, BRANCH_MODEL requested), the tree model's parameters afterwards, and the refused SITE_MODEL request."""
import numpy as np
import pytest

from test_phycpp_gpu import _build, _fluA

pytestmark = pytest.mark.gpu


def _loop(tree, tlk, params):
    p0 = tree.get_parameters()
    lnl, g = [], []
    for p in params:
        tree.set_parameters(p)
        lnl.append(tlk.log_likelihood())
        g.append(tlk.gradient())
    tree.set_parameters(p0)
    return np.array(lnl), np.array(g)


def _close(a, b):
    return np.abs(a - b).max() <= 1e-9 * max(1.0, np.abs(b).max())


def test_unrooted_tree():
    from physher_amd import _phycpp_amd as pc
    _, tree, _, _, tlk = _build("gtr_g4_t16", pc)
    _, tree2, _, _, tlk2 = _build("gtr_g4_t16", pc)
    for t in (tlk, tlk2):
        t.request_gradient([pc.TreeLikelihoodGradientFlags.TREE_HEIGHT])
    p0 = tree.get_parameters()
    rng = np.random.default_rng(3)
    params = p0[None, :] * rng.uniform(0.6, 1.5, size=(7, len(p0)))
    params[0] = p0
    ref_lnl, ref_g = _loop(tree2, tlk2, params)
    lnl, g = tlk.gradient_batch(params)
    assert g.shape == (7, tlk.gradient_length)
    assert np.abs(lnl - ref_lnl).max() <= 1e-9 * np.abs(ref_lnl).max() and _close(g, ref_g)
    assert np.abs(tlk.log_likelihood_batch(params) - ref_lnl).max() <= 1e-9 * np.abs(ref_lnl).max()
    assert np.array_equal(tree.get_parameters(), p0)  # the tree model holds its previous parameters
    assert abs(tlk.log_likelihood() - ref_lnl[0]) <= 1e-12 * abs(ref_lnl[0])
    tlk.set_reference_compatibility(True)  # the reference's folded arithmetic: the same call, the engine's ordinary path or not
    tlk2.set_reference_compatibility(True)
    ref_lnl, ref_g = _loop(tree2, tlk2, params[:3])
    lnl, g = tlk.gradient_batch(params[:3])
    assert np.abs(lnl - ref_lnl).max() <= 1e-9 * np.abs(ref_lnl).max() and _close(g, ref_g)


@pytest.mark.parametrize("jacobian", [False, True])
def test_time_tree_with_strict_clock(jacobian):
    from physher_amd import _phycpp_amd as pc
    F = pc.TreeLikelihoodGradientFlags
    tree, clock, tlk = _fluA(pc, include_jacobian=jacobian)
    tree2, clock2, tlk2 = _fluA(pc, include_jacobian=jacobian)
    for t in (tlk, tlk2):
        t.request_gradient([F.TREE_HEIGHT, F.BRANCH_MODEL])
    p0 = tree.get_parameters()
    root = int(np.argmax(p0))  # the root height among the ratios
    rng = np.random.default_rng(11)
    params = p0[None, :] * rng.uniform(0.85, 1.0, size=(5, len(p0)))
    params[:, root] = p0[root] * rng.uniform(1.0, 1.1, size=5)
    params[0] = p0
    ref_lnl, ref_g = _loop(tree2, tlk2, params)
    lnl, g = tlk.gradient_batch(params)
    assert g.shape == (5, 69)
    assert np.abs(lnl - ref_lnl).max() <= 1e-9 * np.abs(ref_lnl).max() and _close(g, ref_g)
    assert np.abs(tlk.log_likelihood_batch(params) - ref_lnl).max() <= 1e-9 * np.abs(ref_lnl).max()
    assert np.array_equal(tree.get_parameters(), p0)
    assert _close(tlk.gradient(), ref_g[0])
    tlk.request_gradient([F.TREE_HEIGHT])  # without the clock's block
    tlk2.request_gradient([F.TREE_HEIGHT])
    _, ref_g = _loop(tree2, tlk2, params[:2])
    _, g = tlk.gradient_batch(params[:2])
    assert g.shape == (2, 68) and _close(g, ref_g)


def test_site_model_request_is_refused():
    from physher_amd import _phycpp_amd as pc
    F = pc.TreeLikelihoodGradientFlags
    _, tree, _, _, tlk = _build("gtr_g4_t16", pc)
    tlk.request_gradient([F.TREE_HEIGHT, F.SITE_MODEL])
    p0 = tree.get_parameters()
    with pytest.raises(pc.PhyamdError):
        tlk.gradient_batch(p0[None, :])
    assert np.array_equal(tree.get_parameters(), p0)
    assert np.isfinite(tlk.log_likelihood_batch(p0[None, :])[0])  # lnL alone asks for no gradient block
