"""Shared by the invalidation tests: other trees over the same tips, explicit transition matrices, and a NumPy pruning pass that
takes any matrix per node.  Every helper is pinned on the CPU oracle alone in tests/test_invalidation_util.py.  No engine, no GPU."""
import numpy as np

from oracle import phyoracle as po
from physher_amd import synth


def replace(pb, **kw):
    """pb with some fields replaced"""
    f = dict(left=pb.left, right=pb.right, root=pb.root, weights=pb.weights, eval_=pb.eval, evec=pb.evec, ivec=pb.ivec, freqs=pb.freqs,
             cat_rates=pb.cat_rates, cat_props=pb.cat_props, branch_lengths=pb.branch_lengths.copy(), tip_states=pb.tip_states,
             tip_partials=pb.tip_partials, rescale=pb.rescale)
    f.update(kw)
    return po.Problem(f["left"], f["right"], f["root"], f["weights"], f["eval_"], f["evec"], f["ivec"], f["freqs"], f["cat_rates"], f["cat_props"],
                      f["branch_lengths"], tip_states=f["tip_states"], tip_partials=f["tip_partials"], rescale=f["rescale"])


def parents(pb):
    parent = -np.ones(pb.N, dtype=np.int64)
    for n in range(pb.T, pb.N):
        parent[pb.left[n]] = parent[pb.right[n]] = n
    return parent


def levels(pb):
    """the number of levels of internal nodes: the longest chain of internal nodes from a cherry to the root"""
    def height(n):
        return 0 if n < pb.T else 1 + max(height(pb.left[n]), height(pb.right[n]))
    return height(pb.root)


def relabel(pb, perm):
    """the same problem with its node ids permuted, new = perm[old]: perm keeps the tips 0..T-1 and permutes the internal ids
    T..2T-2, so the root need not be the last id.  left, right, root and branch_lengths follow"""
    perm = np.asarray(perm)
    assert np.array_equal(perm[:pb.T], np.arange(pb.T)) and np.array_equal(np.sort(perm[pb.T:]), np.arange(pb.T, pb.N))
    left, right, bl = -np.ones(pb.N, dtype=np.int32), -np.ones(pb.N, dtype=np.int32), np.zeros(pb.N)
    for n in range(pb.N):
        bl[perm[n]] = pb.branch_lengths[n]
        if n >= pb.T:
            left[perm[n]], right[perm[n]] = perm[pb.left[n]], perm[pb.right[n]]
    return replace(pb, left=left, right=right, root=int(perm[pb.root]), branch_lengths=bl)


def rearranged(pb, v, k, t):
    """NNI arrangement k of the internal node v (not the root), with the length of v set to t: (left, right, branch_lengths) of a
    whole tree.  k = 0: the tree itself; k = 1: left[v] changes places with v's sibling; k = 2: right[v] does"""
    left, right, bl = pb.left.copy(), pb.right.copy(), pb.branch_lengths.copy()
    bl[v] = t
    if k > 0:
        u = parents(pb)[v]
        of_u = left if left[u] != v else right  # the array that holds u's slot of the sibling
        of_v = left if k == 1 else right       # k = 1: a = left[v] changes places with the sibling; k = 2: b = right[v]
        of_u[u], of_v[v] = of_v[v], of_u[u]
    return left, right, bl


def neighbour(pb, edge, which):
    """the NNI neighbour of pb's tree across the branch above the internal node `edge`: which = 1 or 2 (rearranged's k)"""
    assert which in (1, 2) and pb.T <= edge < pb.N and edge != pb.root
    left, right, bl = rearranged(pb, edge, which, pb.branch_lengths[edge])
    return replace(pb, left=left, right=right, branch_lengths=bl)


def other_tree(pb, shape, seed):
    """another tree over the same tips (synth.random_tree of that shape), with branch lengths in the range of pb's own"""
    bl = pb.branch_lengths[np.arange(pb.N) != pb.root]
    tree = synth.random_tree(pb.T, np.random.default_rng(seed), shape=shape, bl_low=bl.min(), bl_high=bl.max())
    return replace(pb, left=tree.left, right=tree.right, root=tree.root, branch_lengths=tree.length)


def matrices_at(pb, lengths):
    """[N][C][S][S]: P(lengths[n] r_c) of pb's eigen system for every node (the root's entry too: it is ignored).  An engine
    given these for a set of nodes is the oracle's problem with those nodes' lengths replaced"""
    out = np.empty((pb.N, pb.C, pb.S, pb.S))
    for n in range(pb.N):
        for c in range(pb.C):
            out[n, c] = po.p_t(pb.S, pb.eval, pb.evec, pb.ivec, lengths[n] * pb.cat_rates[c])
    return out


def rate_matrix(pb):
    """Q = U diag(lambda) U^-1"""
    return pb.evec @ np.diag(pb.eval) @ pb.ivec


def tip_vectors(pb):
    """[T][P][S] 0/1 tip partials of a problem (a code >= S is a gap: all ones)"""
    if pb.tip_partials is not None:
        return np.asarray(pb.tip_partials, dtype=np.float64)
    tp = np.zeros((pb.T, pb.P, pb.S))
    for t in range(pb.T):
        s = pb.tip_states[t]
        known = s < pb.S
        tp[t, np.nonzero(known)[0], s[known]] = 1.0
        tp[t, ~known] = 1.0
    return tp


def prune(pb, mats, Q):
    """Post-order pruning and the pre-order pass of pb's tree and data with ANY matrix per node and category, mats [N][C][S][S]
    (the root's is not read), in float64 and without rescaling:
        p_n = (P_l p_l) * (P_r p_r);   L_k = sum_c w_c pi . p_root[c, k];   lnL = sum_k weight_k log L_k
        u_n = P_s p_s under the root, else (P_a u_a) * (P_s p_s) with parent a and sibling s
        g[n][c] = sum_k weight_k / L_k  sum_i pi_i u_n[c, k, i] (Q P_n p_n)[c, k, i]
    -- the header's convention: per category, without w_c r_c, the root's row 0.  Returns dict(lnl, pattern_lk [P], cat_grad [N][C])."""
    lower = np.zeros((pb.N, pb.C, pb.P, pb.S))
    lower[:pb.T] = tip_vectors(pb)[:, None]
    msg = np.zeros_like(lower)  # P_n p_n

    order, stack = [], [pb.root]
    while stack:  # parents before children
        n = stack.pop()
        order.append(n)
        if n >= pb.T:
            stack += [pb.left[n], pb.right[n]]
    for n in reversed(order):
        if n >= pb.T:
            lower[n] = msg[pb.left[n]] * msg[pb.right[n]]
        if n != pb.root:
            msg[n] = np.einsum("cij,ckj->cki", mats[n], lower[n])
    like = np.einsum("c,cki,i->k", pb.cat_props, lower[pb.root], pb.freqs)
    pattern_lk = np.log(like)
    upper = np.zeros_like(lower)
    g = np.zeros((pb.N, pb.C))
    for a in order:
        if a < pb.T:
            continue
        for n, s in ((pb.left[a], pb.right[a]), (pb.right[a], pb.left[a])):
            upper[n] = msg[s] if a == pb.root else np.einsum("cij,ckj->cki", mats[a], upper[a]) * msg[s]
            g[n] = np.einsum("i,cki,ij,ckj,k->c", pb.freqs, upper[n], Q, msg[n], pb.weights / like)
    return dict(lnl=float(pattern_lk @ pb.weights), pattern_lk=pattern_lk, cat_grad=g)


def reversible_matrices(pb, seed):
    """[N][C][S][S]: every node's P(t_n r_c) from a random reversible model of its own (all reversible with respect to pb's
    frequencies): matrices that are no exponential of one common Q"""
    from golden_util import reversible_eigen
    rng = np.random.default_rng(seed)
    out = np.empty((pb.N, pb.C, pb.S, pb.S))
    for n in range(pb.N):
        r = rng.uniform(0.5, 3.0, size=(pb.S, pb.S))
        ev, U, Ui = reversible_eigen(0.5 * (r + r.T), pb.freqs)
        for c in range(pb.C):
            out[n, c] = po.p_t(pb.S, ev, U, Ui, pb.branch_lengths[n] * pb.cat_rates[c])
    return out
