"""Shared by the state-posterior tests: the cases, and NumPy contractions of the CPU oracle's own lower and upper partials
    n != root: J[n][k][j] = sum_c w_c p_n[c,k,j] sum_i pi_i u_n[c,k,i] P_{n,c}[i][j];   root: J[k][j] = sum_c w_c pi_j p_root[c,k,j]
    R[k][c] = w_c pi . p_root[c,k] / sum_c' (the same)
(asr.c:28-134, ppsites.c:17-43).  No engine, no GPU."""
import functools

import numpy as np

from gpu_util import random_problem
from physher_amd._lib import RESCALE_ALWAYS, RESCALE_AUTO

GAP = 1e-6  # states are compared wherever the oracle's top-two posterior gap is at least this


def ambiguous(pb, seed=1):
    """tip partials instead of tip states: gaps all ones, one cell in twenty a two-state ambiguity code"""
    rng = np.random.default_rng(seed)
    tp = np.zeros((pb.T, pb.P, pb.S))
    for t in range(pb.T):
        s = pb.tip_states[t]
        for k in range(pb.P):
            if s[k] >= pb.S:
                tp[t, k] = 1.0
            else:
                tp[t, k, s[k]] = 1.0
                if rng.random() < 0.05:
                    tp[t, k, (s[k] + 1 + rng.integers(pb.S - 1)) % pb.S] = 1.0
    pb.tip_partials, pb.tip_states = tp, None
    return pb


# name -> (problem factory, engine rescaling policy, tip mode); the smallest top-two posterior gap over all cells of all nodes
CASES = {
    "gaps": (lambda: random_problem(12, 200, 4, seed=5, gaps=0.1), RESCALE_AUTO, "states"),  # 3.8e-3
    "one_category": (lambda: random_problem(9, 130, 1, seed=5), RESCALE_AUTO, "states"),  # 0.11: P not a multiple of 64, C = 1
    "larger_tree": (lambda: random_problem(37, 238, 4, seed=5, gaps=0.03), RESCALE_AUTO, "states"),  # 3.3e-3
    "aa": (lambda: random_problem(6, 70, 2, seed=5, S=20), RESCALE_AUTO, "states"),  # 0.14
    "rescaled": (lambda: random_problem(40, 100, 4, seed=5, shape="caterpillar", bl=(0.5, 1.5), rescale=1), RESCALE_ALWAYS, "states"),  # 4.7e-5
    "codon": (lambda: random_problem(8, 300, 2, seed=5, S=61, gaps=0.03), RESCALE_AUTO, "states"),  # 2.5e-2: the size of the 61-state cases of tests/test_branch_hessian_gpu.py
    "ambiguity_codes": (lambda: ambiguous(random_problem(12, 200, 4, seed=5, gaps=0.1)), RESCALE_AUTO, "partials"),  # 3.8e-3
    "pinv": (lambda: random_problem(12, 200, 4, seed=5, gaps=0.1, pinv=0.2), RESCALE_AUTO, "states"),  # 2.1e-3
}


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


def oracle_state_posteriors(pb, fold=False):
    """(J [N][P][S], pattern lnL [P]) from the oracle's lower and upper partials.  fold: the uppers of the reference's
    include_root_freqs arithmetic (pi multiplied in at the root's children), contracted without pi"""
    from oracle import phyoracle as po
    q = pb
    if fold:
        q = po.Problem(pb.left, pb.right, pb.root, pb.weights, pb.eval, pb.evec, pb.ivec, pb.freqs, pb.cat_rates, pb.cat_props, pb.branch_lengths,
                       tip_states=pb.tip_states, tip_partials=pb.tip_partials, rescale=pb.rescale, fold_root_freqs=1)
    r = q.gradient(want_partials=True)
    lower, upper = r["lower"], r["upper"]
    tips = tip_vectors(pb)
    J = np.zeros((pb.N, pb.P, pb.S))
    for n in range(pb.N):
        for c in range(pb.C):
            p = tips[n] if n < pb.T else lower[n, c]
            if n == pb.root:
                J[n] += pb.cat_props[c] * pb.freqs[None, :] * p
                continue
            Pm = np.abs(po.p_t(pb.S, pb.eval, pb.evec, pb.ivec, pb.branch_lengths[n] * pb.cat_rates[c]))
            u = upper[n, c] if fold else upper[n, c] * pb.freqs[None, :]
            J[n] += pb.cat_props[c] * p * (u @ Pm)
    return J, r["pattern_lk"]


def oracle_site_rates(pb):
    r = pb.log_likelihood(want_lower=True)
    num = np.einsum("c,cki,i->kc", pb.cat_props, r["lower"][pb.root], pb.freqs)
    R = num / num.sum(axis=1, keepdims=True)
    return R, R @ pb.cat_rates


@functools.lru_cache(maxsize=None)
def case(name):
    """(problem, oracle posteriors [N][P][S], oracle states, top-two gap per cell, policy, tip mode): computed once per module"""
    make, policy, tip_mode = CASES[name]
    pb = make()
    J, _ = oracle_state_posteriors(pb)
    post = J / J.sum(axis=2, keepdims=True)
    top = np.sort(post, axis=2)
    for a in (post, top):
        a.setflags(write=False)
    return pb, post, post.argmax(axis=2), top[:, :, -1] - top[:, :, -2], policy, tip_mode
