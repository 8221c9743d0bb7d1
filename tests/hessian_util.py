"""NumPy restatement of every branch's first and second derivative of lnL (phyamd_branch_hessian_diagonal), built from the oracle's
partials: _singleTreeLikelihood_d2logP / d2lnldt2_uppper (treelikelihood.c:469-530, 2267-2335) for all branches."""
import numpy as np

from oracle import phyoracle as po


def branch_hessian_diagonal(pb):
    """(lnL, d1 [N], d2 [N]) of an oracle Problem: for every node n != root and pattern k, with u, p the upper and lower partials
    that meet on n's branch and P_c = exp(Q t_n r_c),
        L_k   = sum_c w_c sum_i pi_i u_i (P_c p)_i
        L'_k  = sum_c w_c r_c sum_i pi_i u_i (Q P_c p)_i
        L''_k = sum_c w_c r_c^2 sum_i pi_i u_i (Q Q P_c p)_i
    d1 = sum_k w_k L'_k / L_k, d2 = sum_k w_k (L''_k / L_k - (L'_k / L_k)^2).  The partials may be rescaled: the scale factors are
    per pattern and cancel in both ratios.  Root row 0."""
    r = pb.gradient(want_partials=True)
    lower, upper = r["lower"], r["upper"]  # [N][C][P][S]
    Q = pb.evec @ np.diag(pb.eval) @ pb.ivec
    d1, d2 = np.zeros(pb.N), np.zeros(pb.N)
    for n in range(pb.N):
        if n == pb.root:
            continue
        L, A, B = np.zeros(pb.P), np.zeros(pb.P), np.zeros(pb.P)
        for c in range(pb.C):
            Pm = np.abs(po.p_t(pb.S, pb.eval, pb.evec, pb.ivec, pb.branch_lengths[n] * pb.cat_rates[c]))  # substmodel.c:552
            b = lower[n, c] @ Pm.T  # [P][S]: P p
            qb = b @ Q.T
            fu = upper[n, c] * pb.freqs
            w, rc = pb.cat_props[c], pb.cat_rates[c]
            L += w * np.sum(fu * b, axis=1)
            A += w * rc * np.sum(fu * qb, axis=1)
            B += w * rc * rc * np.sum(fu * (qb @ Q.T), axis=1)
        d1[n] = np.sum(pb.weights * A / L)
        d2[n] = np.sum(pb.weights * (B / L - (A / L) ** 2))
    return r["lnl"], d1, d2
