"""NumPy helpers around Engine.placement_log_likelihoods, Engine.placement_log_likelihoods_general, Engine.placement_optimize and
Engine.placement_optimize_general: the masks and class codes they take, the candidates the optimising calls take from the scoring
calls' results, and what a placement tool makes of a result.

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


AMINO_ACIDS = "ACDEFGHIKLMNPQRSTVWY"  # the engine's state order (physher_amd.synth.AA)
PROTEIN_SETS = (("B", "DN"), ("Z", "EQ"), ("J", "IL"))  # the three standard ambiguity letters and their members


def codes_from_protein(sequences, alphabet=AMINO_ACIDS):
    """Protein sequences (strings of one length, or an array of single letters [queries, P]) -> (codes [queries, P] uint8, sets
    [3] uint64) as Engine.placement_log_likelihoods_general takes them: a letter of `alphabet` is its state 0..19; B, Z and J are
    the sets 21, 22 and 23 (D or N, E or Q, I or L; bit s of sets[q] = state s is a member); X, '-', '?' and every other symbol
    are unknown (20).  Lower case is read as upper case.  The columns are the caller's: they have to be the engine's patterns."""
    if len(alphabet) != 20 or len(set(alphabet.upper())) != 20 or set(alphabet.upper()) & {"B", "Z", "J"}:
        raise ValueError("the alphabet is 20 different letters, none of them B, Z or J")
    table = np.full(256, 20, dtype=np.uint8)
    for s, ch in enumerate(alphabet.upper()):
        table[ord(ch)] = table[ord(ch.lower())] = s
    sets = np.zeros(len(PROTEIN_SETS), dtype=np.uint64)
    for q, (letter, members) in enumerate(PROTEIN_SETS):
        table[ord(letter)] = table[ord(letter.lower())] = 21 + q
        sets[q] = sum(1 << alphabet.upper().index(m) for m in members)
    rows = [np.frombuffer(s.encode("latin-1"), dtype=np.uint8) if isinstance(s, str) else np.frombuffer("".join(s).encode("latin-1"), dtype=np.uint8) for s in sequences]
    if not rows or any(len(r) != len(rows[0]) for r in rows):
        raise ValueError("the sequences are one or more rows of one length")
    return table[np.stack(rows)], sets


def top_candidates(lnl_or_best, k):
    """One pendant length's scores [Q, N] (lnl[i] of Engine.placement_log_likelihoods or, for 20 states,
    Engine.placement_log_likelihoods_general) -> the candidates [count, 2] int32 of Engine.placement_optimize and
    Engine.placement_optimize_general: per query its k best edges as (query, node) rows, query after query, the best edge first.  Ties go
    to the smaller node id; a column of NaN (the root's) is never chosen and neither is a NaN entry; a query with fewer than k
    usable edges gets as many as it has.  A one-dimensional argument is best_node [Q] of one length: every query's one edge."""
    a = np.asarray(lnl_or_best)
    if a.ndim == 1:
        if a.dtype.kind not in "iu":
            raise ValueError(f"a one-dimensional argument is best_node: integers (got {a.dtype})")
        return np.stack([np.arange(len(a)), a], axis=1).astype(np.int32)
    if a.ndim != 2:
        raise ValueError(f"scores are [queries, nodes] (got {a.shape})")
    if k < 1:
        raise ValueError(f"k must be >= 1 (got {k})")
    score = np.where(np.isnan(a), -np.inf, a.astype(np.float64))
    order = np.argsort(-score, axis=1, kind="stable")[:, :k]  # (stable: among equal scores the smaller node id comes first)
    usable = ~np.isnan(np.take_along_axis(a, order, axis=1))
    query = np.broadcast_to(np.arange(a.shape[0])[:, None], order.shape)
    return np.stack([query[usable], order[usable]], axis=1).astype(np.int32)


def likelihood_weight_ratios(lnl, queries=None):
    """The likelihood weight ratio of every edge (EPA / pplacer's LWR): exp(lnl) normalised over the edges of each query, a softmax
    over the last axis.  NaN entries (the root's column) and -inf entries (underflow) get 0; a row without any finite entry is all
    0.  Stable: the row's largest lnL is taken off before exp.
    queries: lnl [count] is laid out sparsely, as Engine.placement_optimize and Engine.placement_optimize_general return it --
    queries [count] holds each entry's query
    (candidates[:, 0]), in any order -- and the result [count] is normalised over the entries of each query."""
    if queries is not None:
        lnl, queries = np.asarray(lnl, dtype=np.float64), np.asarray(queries)
        if lnl.ndim != 1 or queries.shape != lnl.shape:
            raise ValueError(f"sparse scores and their queries are both [count] (got {lnl.shape} and {queries.shape})")
        ids, row = np.unique(queries, return_inverse=True)
        column = np.zeros(len(lnl), dtype=np.int64)
        for r in range(len(ids)):
            at = np.nonzero(row == r)[0]
            column[at] = np.arange(len(at))
        dense = np.full((len(ids), int(column.max()) + 1 if len(lnl) else 0), np.nan)
        dense[row, column] = lnl
        return likelihood_weight_ratios(dense)[row, column]
    lnl = np.asarray(lnl, dtype=np.float64)
    usable = np.isfinite(lnl)
    if np.any(lnl[~usable] == np.inf):
        raise ValueError("a log-likelihood of +inf has no weight ratio")
    top = np.max(np.where(usable, lnl, -np.inf), axis=-1, keepdims=True)
    top = np.where(np.isfinite(top), top, 0.0)
    w = np.where(usable, np.exp(np.where(usable, lnl, top) - top), 0.0)
    total = w.sum(axis=-1, keepdims=True)
    return np.divide(w, total, out=np.zeros_like(w), where=total > 0)
