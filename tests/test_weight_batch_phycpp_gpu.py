"""GPU: TreeLikelihoodInterface.GradientWeights through the pybind module against one object per item whose pattern weights ARE the
item's -- built from the alignment with every pattern's column repeated as often as the item's weight says -- evaluated with
SetParameters + LogLikelihood / Gradient (1e-9 relative, as tests/test_batch_phycpp_gpu.py): with the tree model's current
parameters (one walk serves every item) and with a parameter vector per item; this object's own state afterwards; refusals."""
import numpy as np
import pytest

import test_phycpp_gpu
from physher_amd import resampling
from test_phycpp_gpu import GOLDEN, _build, read_fasta

pytestmark = pytest.mark.gpu
CASE = "gtr_g4_t16"


def _close(a, b):
    return np.abs(a - b).max() <= 1e-9 * max(1.0, np.abs(b).max())


def _site_of_pattern(pc, tlk, names, seqs):
    """a site of the alignment for every pattern of tlk, in its pattern order (a site's column is encoded by compressing it alone)"""
    index = {tuple(col): k for k, col in enumerate(tlk.pattern_states().T.tolist())}
    site = np.full(tlk.get_pattern_count(), -1)
    for i in range(len(seqs[0])):
        states, _ = pc.compress_patterns("nucleotide", names, [s[i] for s in seqs])
        k = index[tuple(states[:, 0].tolist())]
        if site[k] < 0:
            site[k] = i
    assert np.all(site >= 0)
    return site


def _reference(pc, monkeypatch, names, seqs, site, weights, params):
    """lnL and gradient of an object on the alignment that holds pattern k's column weights[k] times"""
    cols = np.repeat(site, weights.astype(int))
    resampled = ["".join(s[i] for i in cols) for s in seqs]
    monkeypatch.setattr(test_phycpp_gpu, "read_fasta", lambda path: (names, resampled))
    _, tree, _, _, tlk = _build(CASE, pc)
    monkeypatch.undo()
    assert tlk.get_pattern_count() == np.count_nonzero(weights)
    tlk.request_gradient([pc.TreeLikelihoodGradientFlags.TREE_HEIGHT])
    if params is not None:
        tree.set_parameters(params)
    return tlk.log_likelihood(), tlk.gradient()


@pytest.mark.parametrize("with_parameters", [False, True])
def test_gradient_weights_equals_one_object_per_item(monkeypatch, with_parameters):
    import os
    from physher_amd import _phycpp_amd as pc
    names, seqs = read_fasta(os.path.join(GOLDEN, CASE, "aln.fa"))
    _, tree, _, _, tlk = _build(CASE, pc)
    tlk.request_gradient([pc.TreeLikelihoodGradientFlags.TREE_HEIGHT])
    own = tlk.pattern_weights()
    site = _site_of_pattern(pc, tlk, names, seqs)
    W = resampling.bootstrap_weights(own, 3, np.random.default_rng(4))
    W[0] = own
    assert (W == 0).any()
    p0 = tree.get_parameters()
    params = None
    if with_parameters:
        params = p0[None, :] * np.random.default_rng(3).uniform(0.6, 1.5, size=(3, len(p0)))
    lnl0, g0 = tlk.log_likelihood(), tlk.gradient()
    lnl, g = tlk.gradient_weights(W, params)
    assert g.shape == (3, tlk.gradient_length)
    for b in range(3):
        ref_lnl, ref_g = _reference(pc, monkeypatch, names, seqs, site, W[b], None if params is None else params[b])
        print(f"item {b}: lnL {lnl[b]!r} reference {ref_lnl!r}  max|dg| {np.abs(g[b] - ref_g).max():.3e}")
        assert abs(lnl[b] - ref_lnl) <= 1e-9 * abs(ref_lnl) and _close(g[b], ref_g)
    if not with_parameters:  # item 0 carries the object's own weights
        assert abs(lnl[0] - lnl0) <= 1e-9 * abs(lnl0) and _close(g[0], g0)
    assert np.array_equal(tree.get_parameters(), p0)  # the tree model holds its previous parameters
    assert np.array_equal(tlk.pattern_weights(), own)
    assert abs(tlk.log_likelihood() - lnl0) <= 1e-12 * abs(lnl0) and _close(tlk.gradient(), g0)


def test_refusals():
    from physher_amd import _phycpp_amd as pc
    F = pc.TreeLikelihoodGradientFlags
    _, tree, _, _, tlk = _build(CASE, pc)
    own = tlk.pattern_weights()
    tlk.request_gradient([F.TREE_HEIGHT, F.SITE_MODEL])
    with pytest.raises(pc.PhyamdError):
        tlk.gradient_weights(own[None, :])
    tlk.request_gradient([F.TREE_HEIGHT])
    with pytest.raises(pc.PhyamdError):
        tlk.gradient_weights(own[None, :-1])
    bad = own[None, :].copy()
    bad[0, 3] = -1.0
    with pytest.raises(pc.PhyamdError):
        tlk.gradient_weights(bad)
    assert np.isfinite(tlk.gradient_weights(own[None, :])[0][0])
