"""NumPy helpers around Engine.placement_log_likelihoods: the masks it takes and what a placement tool makes of its result.

A query's masks are 4-bit numbers over the engine's own patterns, bit s = state s (nucleotides in the order A, C, G, T), 15 a gap.
lnl [..., N] holds a query's log-likelihood on the branch above every node, NaN in the root's column."""
import numpy as np


def masks_from_states(states, state_count=4):
    """State codes [...] -> masks [...] uint8 by the engine's own tip encoding (Engine.set_tip_states): code s < state_count is the
    single state s, every other code (a gap, an unknown) is all states."""
    if state_count != 4:
        raise ValueError("placement masks are 4-bit: 4 states")
    states = np.asarray(states)
    if states.dtype.kind not in "iu":
        raise ValueError(f"state codes are integers (got {states.dtype})")
    single = (states >= 0) & (states < 4)
    return np.where(single, np.left_shift(1, np.where(single, states, 0)), 15).astype(np.uint8)


def likelihood_weight_ratios(lnl):
    """The likelihood weight ratio of every edge (EPA / pplacer's LWR): exp(lnl) normalised over the edges of each query, a softmax
    over the last axis.  NaN entries (the root's column) and -inf entries (underflow) get 0; a row without any finite entry is all
    0.  Stable: the row's largest lnL is taken off before exp."""
    lnl = np.asarray(lnl, dtype=np.float64)
    usable = np.isfinite(lnl)
    if np.any(lnl[~usable] == np.inf):
        raise ValueError("a log-likelihood of +inf has no weight ratio")
    top = np.max(np.where(usable, lnl, -np.inf), axis=-1, keepdims=True)
    top = np.where(np.isfinite(top), top, 0.0)
    w = np.where(usable, np.exp(np.where(usable, lnl, top) - top), 0.0)
    total = w.sum(axis=-1, keepdims=True)
    return np.divide(w, total, out=np.zeros_like(w), where=total > 0)
