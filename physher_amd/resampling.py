"""Resampled pattern-weight vectors for Engine.gradient_batch_weights.  Host-only NumPy: no computation on the device.

A replicate of an alignment -- a bootstrap or jackknife sample of its sites -- is a weight vector over the alignment's own site
patterns: the patterns, and with them every partial and matrix of the engine, stay as they are.  The functions here return such
vectors as rows [count, P]; a pattern a replicate does not contain has weight 0, which the engine treats as a dropped pattern.
"""
from __future__ import annotations

import numpy as np


def _site_counts(weights):
    w = np.ascontiguousarray(weights, dtype=np.float64)
    if w.ndim != 1 or w.size < 1:
        raise ValueError(f"weights must be one-dimensional and not empty (got shape {w.shape})")
    counts = np.rint(w)
    if not np.all(np.isfinite(w)) or np.any(w < 0) or np.any(counts != w):
        raise ValueError("weights must be whole, non-negative site counts per pattern")
    return counts.astype(np.int64)


def bootstrap_weights(weights, count, rng):
    """`count` bootstrap replicates of an alignment with pattern weights `weights` (whole site counts): [count, P] float64.

    A replicate draws sum(w) sites with replacement, a site being of pattern k with probability w_k / sum(w); its row holds how
    often each pattern was drawn -- multinomial counts, which sum to sum(w).

    The reference's SitePattern_bootstrap (phyresampling.c:131-141) draws the same way but then keeps each drawn pattern's ORIGINAL
    weight instead of its draw count, so its replicates are subsets of the alignment rather than resamples of it.  The textbook
    counts are returned here.

    rng: a numpy.random.Generator."""
    counts = _site_counts(weights)
    sites = int(counts.sum())
    if sites < 1:
        raise ValueError("the alignment has no sites")
    if count < 1:
        raise ValueError(f"count must be >= 1 (got {count})")
    return rng.multinomial(sites, counts / sites, size=int(count)).astype(np.float64)


def jackknife_weights(weights):
    """The delete-one-site replicates, one per pattern: [P, P] float64, row k = w - e_k (SitePattern_jackknife, phyresampling.c:158-189,
    for index k; where w_k = 1 the pattern leaves the replicate, weight 0).  A pattern of weight 0 has no site to remove: its row
    is w itself."""
    counts = _site_counts(weights)
    rows = np.tile(counts.astype(np.float64), (counts.size, 1))
    k = np.flatnonzero(counts > 0)
    rows[k, k] -= 1.0
    return rows


def jackknife_n_weights(weights, n, rng):
    """One delete-n replicate: n distinct sites chosen uniformly among the sum(w) sites are removed (SitePattern_jackknife_n,
    phyresampling.c:191-213): [P] float64, never below 0, summing to sum(w) - n.

    rng: a numpy.random.Generator."""
    counts = _site_counts(weights)
    sites = int(counts.sum())
    if n < 0 or n > sites:
        raise ValueError(f"n must be in 0..{sites} (got {n})")
    removed = rng.multivariate_hypergeometric(counts, int(n)) if n > 0 else np.zeros_like(counts)
    return (counts - removed).astype(np.float64)
