"""Helpers for the tests of phyamd_placement_log_likelihoods.  No engine, no GPU.

An edge is a non-root node n of a problem's tree (the branch above it, of length t_n).  Placing a query on n with the split sigma and
the pendant length l is, by definition, the tree with T + 1 tips in which a new internal node z takes n's place under n's parent, z
has the children n (branch sigma t_n) and the query (branch l), and z's own branch is (1 - sigma) t_n: augmented_problem builds exactly
that as a problem of the CPU oracle, which knows nothing of any shortcut.  table_route is the NumPy restatement of the call's route:
the oracle's lower and upper partials of the BASE tree, per (length, edge, pattern) the 16 subset sums of y = sum_c w_c P(l r_c)^T E_c,
the table of w_k log F[m], and a gather-and-add over the patterns.  pruned_base maps a tree with one tip removed (SPR_move's pruning)
onto a base problem, for the cross-check with phyamd_spr_log_likelihoods."""
import numpy as np

import pair_distance_util as pu
from oracle import phyoracle as po


def parents(pb):
    parent = np.full(pb.N, -1, dtype=np.int64)
    for v in range(pb.T, pb.N):
        parent[pb.left[v]] = parent[pb.right[v]] = v
    return parent


def edges(pb):
    return [n for n in range(pb.N) if n != pb.root]


def random_masks(rng, Q, P, gaps=0.1, ambiguous=0.1):
    """[Q][P] query masks: single states, a share of gaps (15) and a share of other ambiguity sets (any of 1..14)"""
    m = np.left_shift(1, rng.integers(0, 4, size=(Q, P)))
    r = rng.random((Q, P))
    m = np.where(r < gaps, 15, m)
    m = np.where((r >= gaps) & (r < gaps + ambiguous), rng.integers(1, 15, size=(Q, P)), m)
    return m.astype(np.uint8)


def augmented_problem(pb, n, mask_row, sigma, pendant):
    """the T + 1 tip problem of (edge n, query mask_row [P], sigma, pendant), straight from the definition.  Ids: the old tips keep
    theirs, the query is tip T, an old internal node i becomes i + 1 and z is the last node"""
    assert n != pb.root
    T, N = pb.T, pb.N
    new = lambda i: int(i) if i < T else int(i) + 1
    z, query = 2 * T, T
    left, right = np.full(N + 2, -1, dtype=np.int32), np.full(N + 2, -1, dtype=np.int32)
    bl = np.zeros(N + 2)
    for v in range(N):
        bl[new(v)] = pb.branch_lengths[v]
        if v >= T:
            left[new(v)] = z if pb.left[v] == n else new(pb.left[v])
            right[new(v)] = z if pb.right[v] == n else new(pb.right[v])
    left[z], right[z] = new(n), query
    bl[new(n)], bl[z], bl[query] = sigma * pb.branch_lengths[n], (1.0 - sigma) * pb.branch_lengths[n], pendant
    bl[new(pb.root)] = pb.branch_lengths[pb.root]
    masks = np.concatenate([pu.problem_masks(pb), np.asarray(mask_row, dtype=np.uint8)[None, :]])
    return po.Problem(left, right, new(pb.root), pb.weights, pb.eval, pb.evec, pb.ivec, pb.freqs, pb.cat_rates, pb.cat_props, bl,
                      tip_partials=pu.partials_from_masks(masks))


def oracle_lnl(pb, n, mask_row, sigma, pendant):
    return augmented_problem(pb, n, mask_row, sigma, pendant).log_likelihood()["lnl"]


def oracle_all(pb, masks, pendants, sigma):
    """[L][Q][N]: every (length, query, edge) by the oracle, NaN in the root's column"""
    out = np.full((len(pendants), len(masks), pb.N), np.nan)
    for i, l in enumerate(pendants):
        for q, row in enumerate(masks):
            for n in edges(pb):
                out[i, q, n] = oracle_lnl(pb, n, row, sigma, l)
    return out


def _p(pb, t):
    return np.abs(po.p_t(pb.S, pb.eval, pb.evec, pb.ivec, t))


def tables(pb, pendants, sigma):
    """[L][N][P][16]: w_k log F[m] of every (length, edge, pattern, mask) from the oracle's partials of the base tree; the root's
    rows and the column of mask 0 are 0"""
    r = pb.gradient(want_partials=True)
    lower, upper = r["lower"], r["upper"]  # [N][C][P][S]; L = sum_c w_c sum_i pi_i upper_i (P_n lower)_i
    subset = pu.partials_from_masks(np.arange(16))  # [16][4]
    out = np.zeros((len(pendants), pb.N, pb.P, 16))
    for n in edges(pb):
        E = np.empty((pb.C, pb.P, 4))
        for c in range(pb.C):
            t = pb.branch_lengths[n] * pb.cat_rates[c]
            lo, hi = _p(pb, sigma * t), _p(pb, (1.0 - sigma) * t)
            E[c] = ((pb.freqs * upper[n, c]) @ hi) * (lower[n, c] @ lo.T)  # [P_hi^T (pi o U)] o (P_lo p_n)
        for i, l in enumerate(pendants):
            y = np.zeros((pb.P, 4))
            for c in range(pb.C):
                y += pb.cat_props[c] * (E[c] @ _p(pb, l * pb.cat_rates[c]))  # w_c P(l r_c)^T E_c
            F = y @ subset.T  # [P][16]
            with np.errstate(divide="ignore"):
                out[i, n, :, 1:] = pb.weights[:, None] * np.log(F[:, 1:])
    return out


def table_route(pb, masks, pendants, sigma):
    """[L][Q][N]: the gather over the tables, NaN in the root's column"""
    tab = tables(pb, pendants, sigma)
    masks = np.asarray(masks)
    out = np.full((len(pendants), len(masks), pb.N), np.nan)
    k = np.arange(pb.P)
    for i in range(len(pendants)):
        for n in edges(pb):
            out[i, :, n] = tab[i, n][k[None, :], masks].sum(axis=1)
    return out


def pruned_base(pb, x):
    """tip x pruned as SPR_move prunes it: its parent u goes with it and its sibling s takes u's place with t_s + t_u.  Returns (the
    base problem with T - 1 tips, new_id [N]: the base's id of every node that stays, -1 for x and u, the query's masks [P], t_x)"""
    parent = parents(pb)
    u = int(parent[x])
    assert x < pb.T and u != pb.root
    s = int(pb.right[u] if pb.left[u] == x else pb.left[u])
    g = int(parent[u])
    T = pb.T - 1
    new_id = np.full(pb.N, -1, dtype=np.int64)
    new_id[[t for t in range(pb.T) if t != x]] = np.arange(T)
    new_id[[v for v in range(pb.T, pb.N) if v != u]] = T + np.arange(T - 1)
    left, right = np.full(2 * T - 1, -1, dtype=np.int32), np.full(2 * T - 1, -1, dtype=np.int32)
    bl = np.zeros(2 * T - 1)
    for v in range(pb.N):
        if new_id[v] < 0:
            continue
        bl[new_id[v]] = pb.branch_lengths[v]
        if v >= pb.T:
            kids = [s if k == u else int(k) for k in (pb.left[v], pb.right[v])]
            left[new_id[v]], right[new_id[v]] = new_id[kids[0]], new_id[kids[1]]
    assert g >= 0
    bl[new_id[s]] = pb.branch_lengths[s] + pb.branch_lengths[u]
    masks = pu.problem_masks(pb)
    keep = [t for t in range(pb.T) if t != x]
    base = po.Problem(left, right, int(new_id[pb.root]), pb.weights, pb.eval, pb.evec, pb.ivec, pb.freqs, pb.cat_rates, pb.cat_props, bl,
                      tip_partials=pu.partials_from_masks(masks[keep]))
    return base, new_id, masks[x], float(pb.branch_lengths[x])
