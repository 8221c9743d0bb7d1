"""Eigen systems with repeated and nearly repeated eigenvalues, as a caller's eigen solver hands them to set_eigen, and the
yardstick of dP/dtheta that needs no eigen system at all.

Six 4-state models through tests/golden_util.reversible_eigen (numpy's symmetric solver).  Two are controls with well separated
eigenvalues (a random GTR, HKY); JC69 has a threefold eigenvalue that the solver happens to return as equal doubles; K80 and F81
have a double one that it returns split by an ulp or two; a GTR within 1e-9 of JC69 has three eigenvalues about 1e-9 apart.  "GTR
with all rates 1 and empirical frequencies", where a GTR fit usually starts, is the F81 entry.
"""
import numpy as np
import scipy.linalg

from golden_util import reversible_eigen

F81_FREQS = np.array([0.1, 0.2, 0.3, 0.4])
MODELS = ("gtr_random", "jc69", "k80", "f81", "hky", "gtr_near_jc69")
# the smallest gap between two eigenvalues that each entry must show (lower, upper): what makes it the case it is named for
GAPS = {"gtr_random": (1e-2, 1.0), "jc69": (0.0, 1e-15), "k80": (0.0, 1e-14), "f81": (0.0, 1e-14), "hky": (1e-2, 1.0), "gtr_near_jc69": (1e-11, 1e-8)}


def _kappa(k):
    r = np.ones((4, 4))
    r[0, 2] = r[2, 0] = r[1, 3] = r[3, 1] = k
    return r


def model(name):
    """(symmetric exchangeabilities [4][4], frequencies [4])"""
    rng = np.random.default_rng(77)
    if name == "gtr_random":
        r = rng.uniform(0.5, 3.0, size=(4, 4))
        return 0.5 * (r + r.T), rng.dirichlet(np.full(4, 5.0))
    if name == "jc69":
        return np.ones((4, 4)), np.full(4, 0.25)
    if name == "k80":
        return _kappa(2.0), np.full(4, 0.25)
    if name == "f81":
        return np.ones((4, 4)), F81_FREQS.copy()
    if name == "hky":
        return _kappa(3.0), F81_FREQS.copy()
    if name == "gtr_near_jc69":
        r = 1.0 + 1e-9 * rng.uniform(1.0, 3.0, size=(4, 4))
        return 0.5 * (r + r.T), np.full(4, 0.25)
    raise ValueError(name)


def eigen(name):
    """(eval, evec, ivec) as reversible_eigen returns them"""
    return reversible_eigen(*model(name))


def smallest_gap(ev):
    return float(np.diff(np.sort(np.asarray(ev))).min())


def rate_matrix(ev, U, Ui):
    return (U * ev[None, :]) @ Ui


def random_dq(S, count, seed):
    """rows sum to zero like any dQ/dtheta"""
    dQ = np.random.default_rng(seed).normal(size=(count, S, S))
    return dQ - dQ.sum(axis=2, keepdims=True) * np.eye(S)[None]


def problem(name, T, P, C, rescale=0, seed=0):
    """An oracle Problem on a model of MODELS: gpu_util.random_problem's tree (0.01 to 0.1; 0.3 to 0.9 when rescaled, as the suite's
    forced-rescaling cases have), data, gaps, weights and category rates, with the model's own frequencies and eigen system"""
    from gpu_util import random_problem
    pb = random_problem(T, P, C, seed=7000 + seed + T + P, gaps=0.03, bl=(0.3, 0.9) if rescale else (0.01, 0.1), rescale=rescale)
    _, freqs = model(name)
    pb.eval, pb.evec, pb.ivec = (np.ascontiguousarray(a) for a in eigen(name))
    pb.freqs = np.ascontiguousarray(freqs)
    return pb


def equal_exchangeabilities(S, seed):
    """(eval, evec, ivec, freqs): all exchangeabilities 1 and random frequencies, F81 at S states: one (S - 1)-fold eigenvalue"""
    freqs = np.random.default_rng(seed).dirichlet(np.full(S, 5.0))
    return reversible_eigen(np.ones((S, S)), freqs) + (freqs,)


def block_expm_derivative(Q, dQ, t):
    """dP/dtheta of P = exp(Q t) in the direction dQ: the upper right block of exp([[Q t, dQ t], [0, Q t]]) (Van Loan 1978).  No
    eigen system, no divided difference: repeated eigenvalues are nothing special to it."""
    S = len(Q)
    M = np.zeros((2 * S, 2 * S))
    M[:S, :S] = M[S:, S:] = Q * t
    M[:S, S:] = dQ * t
    return scipy.linalg.expm(M)[:S, S:]
