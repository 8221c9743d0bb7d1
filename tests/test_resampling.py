"""CPU-only: physher_amd.resampling -- the weight rows of bootstrap and jackknife replicates for Engine.gradient_batch_weights."""
import numpy as np
import pytest

from physher_amd import resampling


def _weights(P, seed):
    return np.random.default_rng(seed).integers(1, 6, size=P).astype(np.float64)


@pytest.mark.parametrize("P,count", [(1, 3), (17, 1), (238, 64)])
def test_bootstrap_rows_are_site_counts_that_sum_to_the_alignment(P, count):
    w = _weights(P, P)
    rows = resampling.bootstrap_weights(w, count, np.random.default_rng(5))
    assert rows.shape == (count, P) and rows.dtype == np.float64
    assert np.all(rows >= 0) and np.array_equal(rows, np.rint(rows))
    assert np.array_equal(rows.sum(axis=1), np.full(count, w.sum()))
    again = resampling.bootstrap_weights(w, count, np.random.default_rng(5))
    assert np.array_equal(rows, again)  # the generator is the only source of randomness


def test_bootstrap_draws_follow_the_weights():
    """a pattern's mean draw count is its weight (multinomial with p_k = w_k / sum w): 4000 replicates, within 6 standard errors;
    a pattern of weight 0 is never drawn"""
    w = np.array([0.0, 1.0, 2.0, 5.0, 12.0])
    rows = resampling.bootstrap_weights(w, 4000, np.random.default_rng(1))
    n, p = w.sum(), w / w.sum()
    se = np.sqrt(n * p * (1 - p) / 4000)
    assert np.all(np.abs(rows.mean(axis=0) - w) <= 6 * se)
    assert np.all(rows[:, 0] == 0)
    assert rows.min() == 0  # (pattern 1 is missing from about e^-1 of the replicates: the rows contain zeros)


def test_jackknife_row_k_removes_one_site_of_pattern_k():
    w = _weights(23, 2)
    w[4] = 1.0  # its replicate drops the pattern
    rows = resampling.jackknife_weights(w)
    assert rows.shape == (23, 23)
    assert np.array_equal(rows, w[None, :] - np.eye(23))
    assert rows[4, 4] == 0.0
    w[7] = 0.0  # no site to remove
    assert np.array_equal(resampling.jackknife_weights(w)[7], w)


@pytest.mark.parametrize("n", [0, 1, 10, 40])
def test_jackknife_n_removes_exactly_n_sites(n):
    w = _weights(40, 9)  # (at least 40 sites)
    row = resampling.jackknife_n_weights(w, n, np.random.default_rng(n))
    assert row.shape == w.shape and row.dtype == np.float64
    assert np.all(row >= 0) and np.all(row <= w) and np.array_equal(row, np.rint(row))
    assert row.sum() == w.sum() - n


def test_jackknife_n_can_empty_the_alignment_and_no_more():
    w = np.array([2.0, 0.0, 3.0])
    assert np.array_equal(resampling.jackknife_n_weights(w, 5, np.random.default_rng(0)), np.zeros(3))
    with pytest.raises(ValueError):
        resampling.jackknife_n_weights(w, 6, np.random.default_rng(0))


@pytest.mark.parametrize("bad", [[1.0, -1.0], [1.5, 2.0], [np.nan, 1.0], []])
def test_weights_that_are_not_site_counts_are_refused(bad):
    with pytest.raises(ValueError):
        resampling.bootstrap_weights(bad, 2, np.random.default_rng(0))
    with pytest.raises(ValueError):
        resampling.jackknife_weights(bad)
