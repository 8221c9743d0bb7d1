"""What phyamd_get_pass_profile must report for each row of the rule that chooses a 4-state pass's kernel (lower_kernel,
upper_kernel, stream_lower_form in phyamd_shard.inc; the launchers in phyamd_launch.inc), the problems the rows run on, and the
oracle comparison every row makes.  The expected profiles below are written from the text of that rule, never from a run."""
import functools

import numpy as np

import state_posteriors_util as spu
import stream_pairs_util as sp
import upper_park_util as upk
from golden_util import reversible_eigen
from oracle import phyoracle as po
from physher_amd import synth

LEVELS, WALK, STREAM = 0, 1, 2        # *_family
REFERENCE, CARRIED, EXP2 = 0, 1, 2    # lower_form (LowerForm)
STREAM_WAVES = 4                      # phyamd_walk4s.inc
CATS_ALL = (1, 2, 3, 4, 5, 8, 9, 16)  # G = 4, 2, 1, 1, then by_waves(C) = 8, 8, 16, 16
LOWER_KEYS = ("lower_family", "lower_form", "lower_scale", "lower_ambiguous", "lower_incremental", "lower_waves", "lower_ppt")
UPPER_KEYS = ("upper_family", "upper_scale", "upper_ambiguous", "upper_waves", "upper_tf", "upper_fold", "upper_compat", "upper_params", "upper_catblk",
              "upper_pair_ops")
NO_LOWER = dict.fromkeys(LOWER_KEYS, -1)
NO_UPPER = dict.fromkeys(UPPER_KEYS, -1)


def walk_waves(C):
    """the wave bound by_waves picks for the level kernels and the table-gather walks: their workgroup holds C * G waves,
    G = max(1, 4 / C) pattern groups (phyamd_create)"""
    w = C * max(1, 4 // C)
    return 4 if w <= 4 else 8 if w <= 8 else 16


# ---- expected profiles: one function per launcher --------------------------------------------------------------------------

def lower_stream(form, scaling, ambiguous=0):
    """launch_lower_stream.  stream_variant(form, scaling): CarriedExp2 -> SCALE 2; else the reference's rescaling or none"""
    assert form != CARRIED or not scaling
    assert form != EXP2 or scaling
    scale = 2 if form == EXP2 else 1 if scaling else 0
    return dict(lower_family=STREAM, lower_form=form, lower_scale=scale, lower_ambiguous=ambiguous, lower_incremental=0, lower_waves=STREAM_WAVES, lower_ppt=0)


def lower_walk(C, scaling, ppt):
    """launch_lower_walk -> launch_lower_walk_ppt; launch_lower leaves Reference.  Rescaled: one pattern per thread"""
    assert ppt == 1 or not scaling
    return dict(lower_family=WALK, lower_form=REFERENCE, lower_scale=int(scaling), lower_ambiguous=0, lower_incremental=0, lower_waves=walk_waves(C), lower_ppt=ppt)


def lower_levels(C, scaling, incremental=0):
    """launch_lower_levels"""
    return dict(lower_family=LEVELS, lower_form=REFERENCE, lower_scale=int(scaling), lower_ambiguous=0, lower_incremental=incremental, lower_waves=walk_waves(C),
                lower_ppt=0)


def upper_stream(form, scaling, ambiguous=0, fold=0, pair_ops=0):
    """launch_upper_stream reads the stored lowers of `form`: SCALE and TF from stream_variant; the pair ops' descriptor set is
    read by the plain, unambiguous TF instantiation alone"""
    scale = 2 if form == EXP2 else 1 if scaling else 0
    tf = int(form != REFERENCE)
    assert pair_ops == 0 or (tf and scale == 0 and not ambiguous)
    return dict(upper_family=STREAM, upper_scale=scale, upper_ambiguous=ambiguous, upper_waves=STREAM_WAVES, upper_tf=tf, upper_fold=fold, upper_compat=0,
                upper_params=0, upper_catblk=0, upper_pair_ops=pair_ops)


def upper_walk(C, scaling, fold=0, compat=0, params=0):
    """launch_upper_walk_v, or launch_upper_walk_params (CATBLK: the unscaled form with a wave bound of 4)"""
    assert not (params and (fold or compat)) and (not compat or scaling)
    catblk = int(params and not scaling and walk_waves(C) == 4)
    return dict(upper_family=WALK, upper_scale=int(scaling), upper_ambiguous=0, upper_waves=walk_waves(C), upper_tf=0, upper_fold=fold, upper_compat=compat,
                upper_params=params, upper_catblk=catblk, upper_pair_ops=0)


def upper_levels(C, scaling, fold=0, compat=0, params=0):
    """launch_upper_levels"""
    assert not compat or scaling
    return dict(upper_family=LEVELS, upper_scale=int(scaling), upper_ambiguous=0, upper_waves=walk_waves(C), upper_tf=0, upper_fold=fold, upper_compat=compat,
                upper_params=params, upper_catblk=0, upper_pair_ops=0)


def profile(lower, upper):
    return {**lower, **upper}


def lower_part(p):
    return {key: p[key] for key in LOWER_KEYS}


def upper_part(p):
    return {key: p[key] for key in UPPER_KEYS}


# ---- problems --------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def pair_tree_name():
    """the smallest random tree among stream_pairs_util's cases whose streamed pre-order schedule has a pair op and a park"""
    names = [n for n in sp.ALL if n.startswith("random")]
    names.sort(key=lambda n: sp.make_tree(n).tip_count)
    for n in names:
        if sp.reach(n)["count"] > 0 and upk.named_stats(n)[1]["parks"] > 0:
            return n
    raise AssertionError("no random tree of stream_pairs_util has a pair op and a park")


def pair_ops():
    return sp.reach(pair_tree_name())["count"]


def problem_on(tree, P, C, seed, gaps, rescale=0):
    """gpu_util.random_problem's recipe on a given tree"""
    rng = np.random.default_rng(seed)
    states = synth.evolve(tree, P, 4, rng)
    if gaps > 0:
        states = np.where(rng.random(states.shape) < gaps, 4 + 13, states).astype(np.uint8)
    weights = rng.integers(1, 5, size=P).astype(np.float64)
    freqs = rng.dirichlet(np.full(4, 5.0))
    r = rng.uniform(0.5, 3.0, size=(4, 4))
    r = 0.5 * (r + r.T)
    ev, U, Ui = reversible_eigen(r, freqs)
    rates = np.sort(rng.gamma(0.5, 2.0, size=C)) + 0.05
    props = np.full(C, 1.0 / C)
    rates = rates / (rates * props).sum()
    return po.Problem(tree.left, tree.right, tree.root, weights, ev, U, Ui, freqs, rates, props, tree.length, tip_states=states, rescale=rescale)


def clone(pb, **changes):
    kw = dict(left=pb.left, right=pb.right, root=pb.root, weights=pb.weights, eval_=pb.eval, evec=pb.evec, ivec=pb.ivec, freqs=pb.freqs, cat_rates=pb.cat_rates,
              cat_props=pb.cat_props, branch_lengths=pb.branch_lengths, tip_states=pb.tip_states, tip_partials=pb.tip_partials, rescale=pb.rescale,
              compat_scaled_gradient=pb.compat_scaled_gradient, fold_root_freqs=pb.fold_root_freqs)
    kw.update(changes)
    return po.Problem(**kw)


@functools.lru_cache(maxsize=None)
def unscaled_problem(P, C):
    """the unscaled rows: P = 321 is two streamed workgroups (4 blocks of 64 each) and a ragged last wave; 3 % gaps"""
    return problem_on(sp.make_tree(pair_tree_name()), P, C, seed=1000 + P + C, gaps=0.03)


@functools.lru_cache(maxsize=None)
def rescaled_problem(shape, C):
    """the rescaled rows: 64 taxa in a caterpillar or 60 in a random tree, lengths in (0.5, 1.5), 130 patterns.  Where the oracle's own
    scale factors are all zero the tree is lengthened, eight taxa at a time, until some are not (the tests assert that they are).
    Longer branches would not do it: a saturated branch leaves every partial near the stationary frequencies"""
    from gpu_util import random_problem
    T0 = {"caterpillar": 64, "random": 60}[shape]
    for T in range(T0, T0 + 161, 8):
        pb = random_problem(T, 130, C, seed=7000 + T0 + C, shape=shape, gaps=0.03, bl=(0.5, 1.5), rescale=1)
        if rescales(pb):
            break
    return pb


def rescales(pb):
    """the oracle's own word that a rescaled evaluation of pb rescales: a non-zero scale factor at some node for some pattern"""
    r = clone(pb, rescale=1).log_likelihood(want_lower=True)
    return bool(r["rescaled"] and np.any(r["scaling"][pb.T:] != 0.0))


def one_hot(pb):
    """pb on tip partials: a state's unit vector, all ones for a gap"""
    tp = np.zeros((pb.T, pb.P, 4))
    for t in range(pb.T):
        s = pb.tip_states[t]
        known = s < 4
        tp[t, np.flatnonzero(known), s[known]] = 1.0
        tp[t, ~known] = 1.0
    return clone(pb, tip_partials=tp, tip_states=None)


def ambiguous(pb, seed=1):
    """pb on tip partials with masks of two states (state_posteriors_util.ambiguous: one cell in twenty) and of three (every
    third of those)"""
    q = spu.ambiguous(clone(pb), seed)
    tp = q.tip_partials
    two = np.argwhere(tp.sum(axis=2) == 2)
    assert len(two) >= 6
    for t, k in two[::3]:
        tp[t, k, int(np.flatnonzero(tp[t, k] == 0)[0])] = 1.0
    sizes = set(np.unique(tp.sum(axis=2)).astype(int))
    assert {1, 2, 3} <= sizes <= {1, 2, 3, 4}, sizes
    return q


def new_lengths(pb, seed=3):
    rng = np.random.default_rng(seed)
    return pb.branch_lengths * rng.uniform(0.6, 1.6, size=pb.N)


def rate_matrix_derivatives(count=3, seed=7):
    rng = np.random.default_rng(seed)
    dQ = rng.normal(size=(count, 4, 4))
    dQ -= dQ.sum(axis=2, keepdims=True) * np.eye(4)[None]  # rows sum to zero like any dQ/dtheta
    return dQ


# ---- the oracle comparison (the suite's bounds) -------------------------------------------------------------------------------

_ORACLE = {}


def oracle(pb, fold=0, compat=0):
    """pb.gradient() under the two flags, computed once per problem object and left unchanged"""
    key = (id(pb), fold, compat)
    if key not in _ORACLE:
        r = clone(pb, fold_root_freqs=fold, compat_scaled_gradient=compat).gradient()
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _ORACLE[key] = (pb, r)  # (pb: the key is its id)
    return _ORACLE[key][1]


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


def check_lnl(e, lnl, ref):
    assert abs(lnl - ref["lnl"]) <= 1e-10 * abs(ref["lnl"]), (lnl, ref["lnl"])
    np.testing.assert_allclose(e.pattern_log_likelihoods(), ref["pattern_lk"], rtol=1e-11, atol=1e-11)


def check_gradient(e, flags, ref, want):
    """gradient(flags) twice: the whole profile after each, the oracle's numbers, the same bits again"""
    lnl, cg = e.gradient(flags)
    got = e.pass_profile()
    assert got == want, {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert e.rescaling == ref["rescaled"]
    check_lnl(e, lnl, ref)
    assert np.all(np.isfinite(ref["cat_grad"]))
    err = np.abs(cg - ref["cat_grad"]).max()
    print(f"lnL off by {abs(lnl - ref['lnl']) / abs(ref['lnl']):.2e} (relative), gradient by {err:.2e} of {1e-9 * max(1.0, np.abs(ref['cat_grad']).max()):.2e}")
    assert err <= 1e-9 * max(1.0, np.abs(ref["cat_grad"]).max())
    lnl2, cg2 = e.gradient(flags)
    assert same_bits(lnl, lnl2) and same_bits(cg, cg2)
    assert e.pass_profile()["upper_family"] == want["upper_family"]
    return lnl, cg
