"""Problems at the edges of the branch-length range -- exactly 0, 1e-12..1e-6, 20..100 -- that the oracle is still a yardstick for.

The rule: the data are evolved ON the extreme tree.  Zeroing branches under data that were evolved on the old lengths makes site
likelihoods hang on the 1e-17 off-diagonals of |U diag(1) U^-1| = P(0), where the oracle disagrees with itself (a mathematically
identical eigen system with its eigenvalues in reverse order moves a per-pattern lnL by up to 45).  So edge_problem sets the
lengths first, then calls synth.evolve on that tree (a zero-length branch gets no substitution there), then adds gaps.

The gate: eigen_reversed(pb) is the same problem to the oracle in another rounding.  tests/test_edge_inputs_util.py asserts, for
every case the GPU files use, that the two oracles agree within one tenth of each GPU tolerance (gate_shares <= 0.1), so that a
GPU tolerance is at least ten times the yardstick's own rounding sensitivity.  No engine, no GPU in this file.
"""
import copy
import functools

import numpy as np

from golden_util import reversible_eigen
from invalidation_util import parents, rearranged
from oracle import phyoracle as po
from physher_amd import synth

FAMILIES = ("zero_internal", "polytomy", "zero_tips", "tiny_internal", "long",
            "zero_internal+long", "zero_tips+zero_internal", "tiny_internal+long", "zero_tips+polytomy+long")
# name: (S, T, P, C) -- 4 states: two full 64-pattern blocks and a ragged one, and the smallest tree with every node kind; the
# smallest 20- and 61-state shapes with more than one level and a ragged pattern tile
SHAPES = {"4s_t24": (4, 24, 130, 4), "4s_t9": (4, 9, 65, 2), "20s": (20, 12, 40, 2), "61s": (61, 6, 17, 1)}
GAPS = 0.03
NNI_FAMILIES = ("zero_internal", "polytomy", "tiny_internal", "long")
NNI_CENTRALS = ("own", 0.0, 30.0)
BATCH_FACTORS = (1.0, 0.5, 2.0)

# DESIGN.md section 4
TOL_LNL, TOL_PATTERN, TOL_PARTIAL, TOL_GRADIENT = 1e-10, 1e-11, 1e-9, 1e-9


def internal_branches(tree_or_pb):
    """internal nodes other than the root, by id"""
    left = tree_or_pb.left
    n_nodes = len(left)
    return [n for n in range((n_nodes + 1) // 2, n_nodes) if n != tree_or_pb.root]


def cherry_left_tips(tree_or_pb):
    left, right = tree_or_pb.left, tree_or_pb.right
    T = (len(left) + 1) // 2
    return [int(left[n]) for n in range(T, len(left)) if left[n] < T and right[n] < T]


def apply_family(tree, family, rng):
    """new lengths [N] for the tree: each '+'-joined part takes its branches from those no earlier part has touched"""
    bl = np.array(tree.length, dtype=np.float64, copy=True)
    N = len(bl)
    touched = np.zeros(N, dtype=bool)
    touched[tree.root] = True
    inner = internal_branches(tree)

    def half_of_the_inner():
        free = [n for n in inner if not touched[n]]
        return sorted(int(n) for n in rng.choice(free, size=(len(free) + 1) // 2, replace=False))

    for part in family.split("+"):
        if part == "zero_internal":
            nodes, values = half_of_the_inner(), 0.0
        elif part == "polytomy":
            nodes, values = [n for n in inner if not touched[n]], 0.0
        elif part == "zero_tips":
            nodes, values = cherry_left_tips(tree), 0.0
        elif part == "tiny_internal":
            nodes = half_of_the_inner()
            values = 10.0 ** rng.uniform(-12.0, -6.0, size=len(nodes))
        elif part == "long":
            free = [n for n in range(N) if not touched[n]]
            nodes = sorted(int(n) for n in rng.choice(free, size=min(len(free), max(1, (N - 1) // 4)), replace=False))
            values = rng.uniform(20.0, 100.0, size=len(nodes))
        else:
            raise ValueError(part)
        bl[nodes] = values
        touched[nodes] = True
    return bl


def edge_problem(S, T, P, C, family, seed, gaps=GAPS, rescale=0):
    """An oracle Problem with random_problem's model (frequencies, symmetric rates, reversible_eigen, category rates, integer
    weights) on a synth.random_tree at (0.01, 0.1) with the family's lengths applied, and tip states evolved on THAT tree."""
    rng = np.random.default_rng(seed)
    tree = synth.random_tree(T, rng, bl_low=0.01, bl_high=0.1)
    tree.length = apply_family(tree, family, rng)
    states = synth.evolve(tree, P, S, rng)
    if gaps > 0:
        states = np.where(rng.random(states.shape) < gaps, S + 13, states).astype(np.uint8)
    weights = rng.integers(1, 5, size=P).astype(np.float64)
    freqs = rng.dirichlet(np.full(S, 5.0))
    r = rng.uniform(0.5, 3.0, size=(S, S))
    ev, U, Ui = reversible_eigen(0.5 * (r + r.T), freqs)
    rates = np.sort(rng.gamma(0.5, 2.0, size=C)) + 0.05
    props = np.full(C, 1.0 / C)
    rates = rates / (rates * props).sum()
    return po.Problem(tree.left, tree.right, tree.root, weights, ev, U, Ui, freqs, rates, props, tree.length, tip_states=states, rescale=rescale)


def with_fields(pb, **kw):
    q = copy.copy(pb)
    for k, v in kw.items():
        setattr(q, k, np.ascontiguousarray(v) if isinstance(v, np.ndarray) else v)
    return q


def eigen_reversed(pb):
    """the same problem with eval, the columns of evec and the rows of ivec reversed"""
    return with_fields(pb, eval=pb.eval[::-1].copy(), evec=pb.evec[:, ::-1].copy(), ivec=pb.ivec[::-1, :].copy())


# Seeds are chosen for the gate (the oracle against itself; no engine has a say): the first seed of the case's own sequence, in
# steps of 1000, at which every gate of tests/test_edge_inputs_util.py holds.  All but these took their first.
# ("4s_t9", "zero_internal"): at central length 0 one NNI entry's d1 differed by 0.157 of its bound.  zero_tips+polytomy+long: no
# ordinary branch stood t = 0 and t = 1e-10 (the only ordinary branches left are tips on a polytomy, and some pattern needed a
# substitution on each of them) until these seeds.
SEED_STEPS = {("4s_t24", "zero_tips+polytomy+long"): 5, ("4s_t9", "zero_internal"): 1, ("20s", "zero_tips+polytomy+long"): 3,
              ("4s_t9", "zero_tips+polytomy+long"): 4}


def seed_of(shape, family):
    return 9000 + 37 * list(SHAPES).index(shape) + FAMILIES.index(family) + 1000 * SEED_STEPS.get((shape, family), 0)


@functools.lru_cache(maxsize=None)
def case(shape, family, rescale=0):
    S, T, P, C = SHAPES[shape]
    return edge_problem(S, T, P, C, family, seed_of(shape, family), rescale=rescale)


def scaled(pb, factor):
    """every positive length multiplied by factor: zeros stay zero, so the item stays consistent with the data"""
    return with_fields(pb, branch_lengths=pb.branch_lengths * factor)


# ---------------------------------------------------------------------------------------------------------
# errors as shares of the tolerances of DESIGN.md section 4: <= 1 passes a GPU comparison, <= 0.1 the gate
# ---------------------------------------------------------------------------------------------------------
def share_lnl(got, ref):
    return abs(got - ref) / (TOL_LNL * abs(ref))


def share_pattern(got, ref):
    """per-pattern lnL as the suite holds it everywhere (assert_allclose, rtol = atol = 1e-11)"""
    return float(np.max(np.abs(got - ref) / (TOL_PATTERN + TOL_PATTERN * np.abs(ref))))


def share_gradient(got, ref):
    """1e-9 * max(1, |ref|inf): gradients, second derivatives, parameter gradients"""
    return float(np.max(np.abs(np.asarray(got) - np.asarray(ref))) / (TOL_GRADIENT * max(1.0, float(np.max(np.abs(ref))))))


def per_pattern_unit(a):
    """partials [C][P][S] divided by each pattern's largest entry over categories and states: rescaling factors are per pattern, so
    this is what a rescaled engine and the oracle have in common"""
    return a / np.max(np.abs(a), axis=(0, 2), keepdims=True)


def share_partials(got, ref, floor=0.0, own_units=True):
    """1e-9 relative, entry by entry, in units of each pattern's largest entry; entries of the reference at or below floor (in those
    units) are held to an ABSOLUTE 1e-9 * floor instead: see PARTIAL_FLOOR.  own_units: got is brought to its own units
    (per_pattern_unit: a rescaled engine against the oracle); False: to the reference's, so that the scale is compared as well"""
    r = per_pattern_unit(ref)
    g = per_pattern_unit(got) if own_units else got / np.max(np.abs(ref), axis=(0, 2), keepdims=True)
    bound = TOL_PARTIAL * np.maximum(np.abs(r), floor)
    diff = np.abs(g - r)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.max(np.where(diff == 0.0, 0.0, diff / bound)))  # (an exact zero of the reference is matched only by a zero)


# The entry-by-entry relative bound on partials (floor 0, as the rest of the suite holds them) passes the gate on the `long` family
# alone.  Everywhere else the gate DROPS it: an entry that is 0 in exact arithmetic -- a state the data below a zero-length branch
# exclude -- is a sum of the 1e-17 off-diagonals of |U diag(1) U^-1| in the oracle and in any engine, and an entry of 1e-12 below a
# tiny branch is formed from off-diagonals that are themselves only good to 1e-17 absolute; the oracle and its eigen-reversed copy
# differ there by 1e-6 to 100 % (shares of 5 to 3e8 of the bound).  What the oracle does keep is an ABSOLUTE error per pattern:
# over all 72 cases it differs from its reversed self by at most 1.3e-13 of the pattern's largest entry, whatever the entry's
# size.  So for those families an entry below PARTIAL_FLOOR of its pattern's largest is held to 1e-9 * PARTIAL_FLOOR of that
# largest entry (1e-11: 77 times the oracle's own 1.3e-13, so the gate's tenth holds with room), and an entry above it to the
# relative 1e-9 as everywhere.
PARTIAL_FLOOR = 1e-2


def partial_floor(family):
    return 0.0 if family == "long" else PARTIAL_FLOOR


def gate_core(pb, floor):
    """shares of the GPU tolerances by which the oracle differs from its eigen-reversed self: lnL, per-pattern lnL, the per-category
    gradient, lower and upper partials of every node"""
    a, b = pb.gradient(want_partials=True), eigen_reversed(pb).gradient(want_partials=True)
    out = dict(lnl=share_lnl(b["lnl"], a["lnl"]), pattern=share_pattern(b["pattern_lk"], a["pattern_lk"]),
               gradient=share_gradient(b["cat_grad"], a["cat_grad"]))
    out["lower"] = max(share_partials(b["lower"][n], a["lower"][n], floor) for n in range(pb.T, pb.N))
    out["upper"] = max(share_partials(b["upper"][n], a["upper"][n], floor) for n in range(pb.N) if n != pb.root)
    g = np.abs(po.branch_gradient_from_cat(a["cat_grad"], pb.cat_rates, pb.cat_props)).max()
    out["exp rounding"] = g * 2.0 ** -52 / (TOL_LNL * abs(a["lnl"]))  # (exp_rounding_shares, for every branch at once)
    return out


def nni_candidates(pb):
    return internal_branches(pb)


def nni_central(pb, central):
    """[3][N] trial lengths, or None for the engine's own"""
    return None if central == "own" else np.full((3, pb.N), float(central))


def nni_problem(pb, v, k, t):
    left, right, bl = rearranged(pb, v, k, t)
    return with_fields(pb, left=left, right=right, branch_lengths=bl)


def nni_oracle(pb, central):
    """(lnl [3][N], d1 [3][N]) of every entry by the oracle on the rearranged tree (NaN elsewhere)"""
    lnl, d1 = np.full((3, pb.N), np.nan), np.full((3, pb.N), np.nan)
    for v in nni_candidates(pb):
        t = pb.branch_lengths[v] if central == "own" else float(central)
        for k in range(3):
            r = nni_problem(pb, v, k, t).gradient()
            lnl[k, v] = r["lnl"]
            d1[k, v] = po.branch_gradient_from_cat(r["cat_grad"], pb.cat_rates, pb.cat_props)[v]
    return lnl, d1


def gate_nni(pb, central):
    (la, da), (lb, db) = nni_oracle(pb, central), nni_oracle(eigen_reversed(pb), central)
    cand = nni_candidates(pb)
    out = dict(lnl=float(np.max(np.abs(lb[:, cand] - la[:, cand]) / (TOL_LNL * np.abs(la[:, cand])))), d1=share_gradient(db[:, cand], da[:, cand]))
    if central != 0.0:  # (e^0 is 1 in every implementation)
        out["exp rounding"] = float(np.max(np.abs(da[:, cand])) * 2.0 ** -52 / (TOL_LNL * np.min(np.abs(la[:, cand]))))
    return out


# ---------------------------------------------------------------------------------------------------------
# single-branch trials, second derivatives, the substitution-parameter gradient
# ---------------------------------------------------------------------------------------------------------
def ordinary(pb, n):
    return n != pb.root and 0.01 <= pb.branch_lengths[n] <= 0.1


TRIAL_LENGTHS = (0.0, 1e-10, 50.0)
TRIAL_ON_ZERO = 0.05


def oracle_branch(pb, n, t):
    """(lnL, d1, d2, |per-category gradient|inf, |d2|inf) with branch n at length t"""
    from hessian_util import branch_hessian_diagonal
    q = with_fields(pb, branch_lengths=np.where(np.arange(pb.N) == n, t, pb.branch_lengths))
    lnl, d1, d2 = branch_hessian_diagonal(q)
    return lnl, d1[n], d2[n], float(np.abs(q.gradient()["cat_grad"]).max()), float(np.abs(d2).max())


def exp_rounding_shares(lnl, d1, d2, gmax):
    """What eigen reversal cannot show, because both copies share it: e^{lambda t r} is stored to an ulp of 1, 2^-52 or so, in the
    oracle and in any engine (whose exp may be an ulp off besides), and with |lambda r| near 1 that is the same as moving t by
    2^-52.  lnL then moves by |d1| 2^-52 and d1 by |d2| 2^-52: as shares of the lnL and of the d1 tolerance.  Where a pattern needs
    a substitution on a branch of length 1e-10 its likelihood is q t, d1 is 1e10, d2 is -1e20 and these shares are 20 and 2000:
    such a trial measures the rounding of exp, not the engine (an MI355X run showed 32 and 420 on two of them)."""
    return abs(d1) * 2.0 ** -52 / (TOL_LNL * abs(lnl)), abs(d2) * 2.0 ** -52 / (TOL_GRADIENT * max(1.0, gmax))


def gate_branch(pb, n, t):
    ref = oracle_branch(pb, n, t)
    return max(share_branch(oracle_branch(eigen_reversed(pb), n, t), ref) + (exp_rounding_shares(*ref[:4]) if t > 0.0 else ()))


@functools.lru_cache(maxsize=None)
def branch_trials(shape, family):
    """[(node, t)]: t in TRIAL_LENGTHS on one branch of ordinary length, and TRIAL_ON_ZERO on the first and the last zero-length
    branch where the case has any.  Shrinking a branch to 0 under data that were evolved with it at 0.01 to 0.1 is the very thing the
    module's rule forbids: where a pattern needs a substitution on that branch (its two ends then lie between zero-length branches
    that hold different states) the trial hangs on P(0)'s off-diagonals, d1 is 1e15 and the oracle disagrees with itself.  So the
    branch is CHOSEN BY THE GATE: the first ordinary branch, internal nodes before tips, at which the oracle and its eigen-reversed
    copy agree within a tenth of the tolerances at all three lengths and the rounding of exp stays below a tenth as well
    (exp_rounding_shares; tests/test_edge_inputs_util.py asserts that one exists in every case, and asserts the gate for it again)."""
    pb = case(shape, family)
    out = []
    for n in [n for n in internal_branches(pb) if ordinary(pb, n)] + [n for n in range(pb.T) if ordinary(pb, n)]:
        if all(gate_branch(pb, n, t) <= 0.1 for t in TRIAL_LENGTHS):
            out = [(n, t) for t in TRIAL_LENGTHS]
            break
    zero = [n for n in range(pb.N) if n != pb.root and pb.branch_lengths[n] == 0.0]
    for n in dict.fromkeys(zero[:1] + zero[-1:]):
        out.append((n, TRIAL_ON_ZERO))
    return out


def share_branch(got, ref):
    """(lnL, d1, d2) of one trial against oracle_branch's row"""
    return (share_lnl(got[0], ref[0]), abs(got[1] - ref[1]) / (TOL_GRADIENT * max(1.0, ref[3])), abs(got[2] - ref[2]) / (TOL_GRADIENT * max(1.0, ref[4])))


POSTERIOR_FAMILIES = ("zero_tips+zero_internal", "long")


def posteriors(pb):
    """what state_posteriors / site_rate_posteriors return, from tests/state_posteriors_util.py's restatements: post [N][P][S], the most
    probable states, the top-two gap per cell, R [P][C] and the mean rate [P]"""
    from state_posteriors_util import oracle_site_rates, oracle_state_posteriors
    J, _ = oracle_state_posteriors(pb)
    post = J / J.sum(axis=2, keepdims=True)
    top = np.sort(post, axis=2)
    R, mean = oracle_site_rates(pb)
    return dict(post=post, states=post.argmax(axis=2), gap=top[:, :, -1] - top[:, :, -2], R=R, mean=mean)


def zero_tip_parents(pb):
    """[(tip, its parent, the patterns at which the tip is observed)] for every zero-length tip"""
    par = parents(pb)
    return [(t, int(par[t]), pb.tip_states[t] < pb.S) for t in range(pb.T) if pb.branch_lengths[t] == 0.0]


def beyond_exp_case(shape="20s"):
    """the shape's `long` case with its first tip's branch at 700: (l_a - l_b) t r passes 709, the largest argument of exp, in the
    fastest category -- e^{l_b t} expm1((l_a - l_b) t) is then 0 * inf where e^{hi t} (1 - e^{-(hi - lo) t}) is just e^{hi t}"""
    pb = case(shape, "long")
    bl = pb.branch_lengths.copy()
    bl[0] = 700.0
    pb = with_fields(pb, branch_lengths=bl)
    assert (pb.eval.max() - pb.eval.min()) * 700.0 * pb.cat_rates.max() > 710.0
    return pb


def random_dq(S, count, seed):
    """rows sum to zero like any dQ/dtheta"""
    dQ = np.random.default_rng(seed).normal(size=(count, S, S))
    return dQ - dQ.sum(axis=2, keepdims=True) * np.eye(S)[None]
