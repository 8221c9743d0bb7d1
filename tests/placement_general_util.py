"""Helpers for the tests of phyamd_placement_log_likelihoods_general.  No engine, no GPU.

placement_util.py for 20 states, with class codes in the place of 4-bit masks: a query cell is a state (0..19), unknown (20) or
21 + q for the CALL's set q (a member word, bit s = state s).  augmented_problem is the T + 1 tip problem of the CPU oracle built
from the definition -- the reference tips enter as the 0/1 partials the engine holds for them (pair_distance_general_util's
codes_from_problem and member_matrix), the query as member_matrix(sets)[codes] -- and knows nothing of any shortcut.  table_route
is the NumPy restatement of the call's route: the oracle's lower and upper partials of the BASE tree, per (length, edge, pattern)
the 32 class sums of y = sum_c w_c P(l r_c)^T E_c, the table of w_k log F[class], and a gather-and-add over the patterns."""
import numpy as np

import pair_distance_general_util as gu
from oracle import phyoracle as po
from placement_util import edges, parents  # noqa: F401  (the same trees)

S, CLASSES, UNKNOWN, MAX_SETS = gu.S, gu.CLASSES, gu.UNKNOWN, gu.CLASSES - gu.S - 1


def random_sets(rng, count):
    """`count` different member words of 2..19 members"""
    sets = []
    while len(sets) < count:
        m = rng.random(S) < 0.3
        w = int(m.astype(np.int64) @ (1 << np.arange(S, dtype=np.int64)))
        if 2 <= m.sum() <= S - 1 and w not in sets:
            sets.append(w)
    return np.array(sets, dtype=np.uint64)


def random_codes(rng, Q, P, set_count=0, unknown=0.1, in_sets=0.15):
    """[Q][P] query codes: single states, a share of unknown cells (20) and a share of cells of the call's sets (21 + q)"""
    c = rng.integers(0, S, size=(Q, P))
    r = rng.random((Q, P))
    c = np.where(r < unknown, UNKNOWN, c)
    if set_count:
        c = np.where((r >= unknown) & (r < unknown + in_sets), S + 1 + rng.integers(0, set_count, size=(Q, P)), c)
    return c.astype(np.uint8)


def reference_partials(pb):
    """[T][P][20]: the 0/1 vectors of the reference tips as the engine holds them"""
    codes, members = gu.codes_from_problem(pb)
    return gu.member_matrix(members)[codes]


def query_partials(code_row, sets):
    return gu.member_matrix(gu.class_members(list(sets)))[np.asarray(code_row)]


def augmented_problem(pb, n, code_row, sets, sigma, pendant, reference=None):
    """the T + 1 tip problem of (edge n, query code_row [P] over `sets`, sigma, pendant), straight from the definition.  Ids: the
    old tips keep theirs, the query is tip T, an old internal node i becomes i + 1 and z is the last node.  reference: the value
    of reference_partials(pb), for callers that build many problems on one base"""
    assert n != pb.root and pb.S == S
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
    part = np.concatenate([reference_partials(pb) if reference is None else reference, query_partials(code_row, sets)[None]])
    return po.Problem(left, right, new(pb.root), pb.weights, pb.eval, pb.evec, pb.ivec, pb.freqs, pb.cat_rates, pb.cat_props, bl, tip_partials=part)


def oracle_lnl(pb, n, code_row, sets, sigma, pendant, reference=None):
    return augmented_problem(pb, n, code_row, sets, sigma, pendant, reference).log_likelihood()["lnl"]


def oracle_all(pb, codes, sets, pendants, sigma):
    """[L][Q][N]: every (length, query, edge) by the oracle, NaN in the root's column"""
    out = np.full((len(pendants), len(codes), pb.N), np.nan)
    reference = reference_partials(pb)
    for i, l in enumerate(pendants):
        for q, row in enumerate(codes):
            for n in edges(pb):
                out[i, q, n] = oracle_lnl(pb, n, row, sets, sigma, l, reference)
    return out


def _p(pb, t):
    return np.abs(po.p_t(pb.S, pb.eval, pb.evec, pb.ivec, t))


def class_likelihoods(pb, sets, pendants, sigma):
    """[L][N][P][32]: F[class] = sum_c w_c sum_z (sum_{j in class} P(l r_c)[z][j]) E_c,z of every (length, edge, pattern) from the
    oracle's partials of the base tree; the root's rows and the classes no set stands for are 0"""
    r = pb.gradient(want_partials=True)
    lower, upper = r["lower"], r["upper"]  # [N][C][P][S]; L = sum_c w_c sum_i pi_i upper_i (P_n lower)_i
    members = gu.member_matrix(gu.class_members(list(sets)))  # [32][20]
    out = np.zeros((len(pendants), pb.N, pb.P, CLASSES))
    for n in edges(pb):
        E = np.empty((pb.C, pb.P, S))
        for c in range(pb.C):
            t = pb.branch_lengths[n] * pb.cat_rates[c]
            lo, hi = _p(pb, sigma * t), _p(pb, (1.0 - sigma) * t)
            E[c] = ((pb.freqs * upper[n, c]) @ hi) * (lower[n, c] @ lo.T)  # [P_hi^T (pi o u_n)] o (P_lo p_n)
        for i, l in enumerate(pendants):
            y = np.zeros((pb.P, S))
            for c in range(pb.C):
                y += pb.cat_props[c] * (E[c] @ _p(pb, l * pb.cat_rates[c]))  # w_c P(l r_c)^T E_c
            out[i, n] = y @ members.T
    return out


def tables(pb, sets, pendants, sigma):
    """[L][N][P][32]: w_k log F[class]; the root's rows, patterns of weight 0 and the classes no set stands for are 0"""
    F = class_likelihoods(pb, sets, pendants, sigma)
    live = np.zeros(CLASSES, dtype=bool)
    live[:S + 1 + len(sets)] = True
    out = np.zeros_like(F)
    for n in edges(pb):
        with np.errstate(divide="ignore"):
            out[:, n][..., live] = np.where(pb.weights[:, None] != 0, pb.weights[:, None] * np.log(F[:, n][..., live]), 0.0)
    return out


def table_route(pb, codes, sets, pendants, sigma):
    """[L][Q][N]: the gather over the tables, NaN in the root's column"""
    tab = tables(pb, sets, pendants, sigma)
    codes = np.asarray(codes)
    assert codes.max() <= S + len(sets)
    out = np.full((len(pendants), len(codes), pb.N), np.nan)
    k = np.arange(pb.P)
    for i in range(len(pendants)):
        for n in edges(pb):
            out[i, :, n] = tab[i, n][k[None, :], codes].sum(axis=1)
    return out
