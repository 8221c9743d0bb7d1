"""Two NumPy restatements of the full branch-length Hessian of lnL (phyamd_branch_hessian): _singleTreeLikelihood_ddlogP
(treelikelihood.c:532-690) for every pair of branches, as calculate_hessian (hessian.c:14-25) asks for them.

(a) brute_force: per pair (a, b) the tree is pruned again with P_a and P_b replaced by their derivatives -- the definition;
(b) message_form: from the oracle's lower and upper partials, one tangent per (branch, ancestor) carried up the tree -- what the
    device kernels compute (physher_amd/csrc/phyamd_bhess.inc)."""
import numpy as np

from oracle import phyoracle as po


def _matrices(pb):
    """P [N][C][S][S] (substmodel.c:552: |exp(Q t r)|), Q [S][S]"""
    Pm = np.zeros((pb.N, pb.C, pb.S, pb.S))
    for n in range(pb.N):
        for c in range(pb.C):
            Pm[n, c] = np.abs(po.p_t(pb.S, pb.eval, pb.evec, pb.ivec, pb.branch_lengths[n] * pb.cat_rates[c]))
    return Pm, pb.evec @ np.diag(pb.eval) @ pb.ivec


def _tip_partials(pb):
    """[T][P][S] 0/1"""
    if pb.tip_partials is not None:
        return np.asarray(pb.tip_partials, dtype=np.float64)
    tp = np.ones((pb.T, pb.P, pb.S))
    for t in range(pb.T):
        known = pb.tip_states[t] < pb.S
        tp[t, known] = 0.0
        tp[t, np.nonzero(known)[0], pb.tip_states[t][known]] = 1.0
    return tp


def _post_order(pb):
    order, stack = [], [pb.root]
    while stack:
        n = stack.pop()
        order.append(n)
        if n >= pb.T:
            stack += [int(pb.left[n]), int(pb.right[n])]
    return order[::-1]


def _site_likelihoods(pb, tips, mats, order):
    """L_k [P] by pruning with the matrices mats [N][C][S][S]"""
    part = {}
    for n in order:
        if n < pb.T:
            part[n] = np.broadcast_to(tips[n], (pb.C, pb.P, pb.S))
        else:
            l, r = int(pb.left[n]), int(pb.right[n])
            part[n] = np.einsum("cij,ckj->cki", mats[l], part[l]) * np.einsum("cij,ckj->cki", mats[r], part[r])
    return np.einsum("c,cki,i->k", pb.cat_props, part[pb.root], pb.freqs)


def brute_force(pb):
    """(lnL, g [N], H [N][N]):  g[a] = sum_k w_k L_a,k / L_k,  H[a][b] = sum_k w_k (L_ab,k / L_k - L_a,k L_b,k / L_k^2) with L_a the
    site likelihood with P_{a,c} replaced by r_c Q P_{a,c}, L_ab with both replaced (a = b: by r_c^2 Q Q P_{a,c}).  Root row and
    column 0."""
    Pm, Q = _matrices(pb)
    r = pb.cat_rates[:, None, None]
    d1 = np.einsum("ij,ncjk->ncik", Q, Pm) * r
    d2 = np.einsum("ij,ncjk->ncik", Q, d1) * r
    tips, order = _tip_partials(pb), _post_order(pb)
    L = _site_likelihoods(pb, tips, Pm, order)
    nodes = [n for n in range(pb.N) if n != pb.root]
    La = {}
    g, H = np.zeros(pb.N), np.zeros((pb.N, pb.N))
    for a in nodes:
        m = Pm.copy()
        m[a] = d1[a]
        La[a] = _site_likelihoods(pb, tips, m, order)
        g[a] = np.sum(pb.weights * La[a] / L)
    for i, a in enumerate(nodes):
        for b in nodes[i:]:
            m = Pm.copy()
            if a == b:
                m[a] = d2[a]
            else:
                m[a], m[b] = d1[a], d1[b]
            Lab = _site_likelihoods(pb, tips, m, order)
            H[a, b] = H[b, a] = np.sum(pb.weights * (Lab / L - La[a] * La[b] / L ** 2))
    return float(np.sum(pb.weights * np.log(L))), g, H


def message_form(pb):
    """(lnL, g [N], H [N][N]) from the oracle's partials: with msg(n) = P_n p_n, A_m = P_m^T (pi o u_m) (the root: pi),
    T_a^(par a) = r_c Q P_a p_a and T_a^(par m) = P_m (T_a^(m) o msg(other child of m)),
        a below b != root:        L_ab = sum_c w_c r_c sum_i (pi o u_b)_i (Q P_b (T_a^(b) o msg(other child of b)))_i
        a, b on two sides of m:   L_ab = sum_c w_c sum_i (A_m)_i (T_a^(m))_i (T_b^(m))_i
        a = b:                    L_aa = sum_c w_c r_c^2 sum_i (pi o u_a)_i (Q Q P_a p_a)_i"""
    res = pb.gradient(want_partials=True)
    lower, upper = res["lower"], res["upper"]  # [N][C][P][S]
    Pm, Q = _matrices(pb)
    w, r, pi = pb.cat_props, pb.cat_rates, pb.freqs
    parent = np.full(pb.N, -1)
    for n in range(pb.T, pb.N):
        parent[pb.left[n]] = parent[pb.right[n]] = n
    msg = np.einsum("ncij,nckj->ncki", Pm, lower)
    L = np.einsum("c,cki,i->k", w, lower[pb.root], pi)
    nodes = [n for n in range(pb.N) if n != pb.root]
    La = np.zeros((pb.N, pb.P))
    first = np.zeros((pb.N, pb.N))  # sum_k w_k L_ab,k / L_k
    T = {}  # (a, m) -> T_a^(m) [C][P][S], m every ancestor of a
    for a in nodes:
        t = np.einsum("ij,ckj->cki", Q, msg[a]) * r[:, None, None]
        fu = upper[a] * pi
        La[a] = np.einsum("c,cki,cki->k", w, fu, t)
        Laa = np.einsum("c,cki,cki->k", w * r * r, fu, np.einsum("ij,jl,ckl->cki", Q, Q, msg[a]))
        first[a, a] = np.sum(pb.weights * Laa / L)
        cur, m = a, int(parent[a])
        T[a, m] = t
        while m != pb.root:
            sib = int(pb.right[m]) if int(pb.left[m]) == cur else int(pb.left[m])
            x = t * msg[sib]
            px = np.einsum("cij,ckj->cki", Pm[m], x)
            Lam = np.einsum("c,cki,cki->k", w * r, upper[m] * pi, np.einsum("ij,ckj->cki", Q, px))
            first[a, m] = first[m, a] = np.sum(pb.weights * Lam / L)
            t, cur, m = px, m, int(parent[m])
            T[a, m] = t
    below = {n: [n] for n in range(pb.N)}
    for n in _post_order(pb):
        if n >= pb.T:
            below[n] = [n] + below[int(pb.left[n])] + below[int(pb.right[n])]
    for m in range(pb.T, pb.N):
        Am = np.broadcast_to(pi, (pb.C, pb.P, pb.S)) if m == pb.root else np.einsum("cij,cki->ckj", Pm[m], upper[m] * pi)
        for a in below[int(pb.left[m])]:
            wa = np.einsum("c,cki,cki->cki", w, Am, T[a, m])
            for b in below[int(pb.right[m])]:
                first[a, b] = first[b, a] = np.sum(pb.weights * np.einsum("cki,cki->k", wa, T[b, m]) / L)
    G = La / L
    outer = np.triu(np.einsum("k,ak,bk->ab", pb.weights, G, G))  # (one triangle, mirrored: a BLAS product need not be symmetric in its bits)
    H = first - (outer + np.triu(outer, 1).T)
    H[pb.root, :] = 0.0
    H[:, pb.root] = 0.0
    return res["lnl"], G @ pb.weights, H
