"""GPU: every evaluation of the engine at the edges of the branch-length range -- lengths of exactly 0 (polytomies written as
zero-length internal branches, identical sequences), of 1e-12 to 1e-6 (an optimiser on its lower bound) and of 20 to 100 (a
saturated outgroup) -- against the CPU oracle at the tolerances of DESIGN.md section 4: lnL 1e-10 relative, per-pattern lnL 1e-11,
partials 1e-9 relative, gradients and second derivatives 1e-9 * max(1, |ref|inf).

The cases are tests/edge_inputs_util.py's: nine families of lengths on four shapes, the data evolved on the extreme tree itself so
that the oracle stays a yardstick, and tests/test_edge_inputs_util.py (CPU) asserts for every comparison made here that the oracle
agrees with its eigen-reversed self within a tenth of the tolerance.  One call was dropped by that gate: the entry-by-entry
relative bound on partials holds on the `long` family alone; elsewhere entries below 1e-2 of their pattern's largest are held to an
absolute 1e-11 of it (edge_inputs_util.PARTIAL_FLOOR has the reason and the figures).  The branch that branch_log_likelihood
shrinks to 0 is chosen by the same gate (edge_inputs_util.branch_trials).

Every code path that forms P(t), Q P or Q Q P on its own is reached: k_transition_matrices, the batched walk's copy, the NNI trial
lengths, the exponential sums of nni_optimize, the path walk of branch_log_likelihood, the tangents of the branch Hessian, and the
rescaling exponents of partials that are a tip's indicator.  Each test prints its errors as shares of the tolerances.
"""
import functools

import numpy as np
import pytest

import edge_inputs_util as eu
import invalidation_util as iu
from full_hessian_util import brute_force
from gpu_util import engine_from_problem
from hessian_util import branch_hessian_diagonal
from nni_optimize_util import evaluate as nni_evaluate
from oracle import phyoracle as po
from physher_amd.engine import GRAD_FOLD_ROOT_FREQS, RESCALE_ALWAYS, RESCALE_NEVER
from state_posteriors_util import GAP

pytestmark = pytest.mark.gpu

CORE = [(s, f, r) for s in eu.SHAPES for f in eu.FAMILIES for r in (0, 1)]
FOUR = [s for s in eu.SHAPES if eu.SHAPES[s][0] == 4]
HESS = [s for s in eu.SHAPES if eu.SHAPES[s][0] in (4, 20)]


def _policy(rescale):
    return RESCALE_ALWAYS if rescale else RESCALE_NEVER


def _report(what, shares):
    print(f"SHARES {what}: " + ", ".join(f"{k} {v:.2e}" for k, v in shares.items()))
    for k, v in shares.items():
        assert v <= 1.0, (what, k, v)


@functools.lru_cache(maxsize=None)
def _oracle(shape, family, rescale):
    pb = eu.case(shape, family, rescale)
    ref = pb.gradient(want_partials=True)
    assert ref["rescaled"] == bool(rescale) and np.isfinite(ref["lnl"])
    folded = eu.with_fields(pb, fold_root_freqs=1).gradient() if pb.S == 4 else None
    return pb, ref, folded


def _gradient_shares(e, ref, flags=0):
    """log_likelihood() (on a new engine: the post-order pass alone), then lnL, per-pattern lnL and the per-category gradient of one
    gradient() call; a second call of either returns the same bits"""
    first = e.log_likelihood()
    launches = [e.profile()["lower_launches"]]  # (a profiling engine: the post-order launches of this call, 0 when nothing was pending)
    assert e.log_likelihood() == first
    lnl, cg = e.gradient(flags)
    launches.append(e.profile()["upper_launches"])
    plk = e.pattern_log_likelihoods()
    lnl2, cg2 = e.gradient(flags)
    assert lnl2 == lnl and np.array_equal(cg2, cg)
    return dict(log_likelihood=eu.share_lnl(first, ref["lnl"]), lnl=eu.share_lnl(lnl, ref["lnl"]), pattern=eu.share_pattern(plk, ref["pattern_lk"]),
                gradient=eu.share_gradient(cg, ref["cat_grad"])), launches


# ---------------------------------------------------------------------------------------------------------
# log_likelihood, pattern_log_likelihoods, gradient: the walks, the level kernels and their partials, plain and rescaled
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,family,rescale", CORE)
def test_core_evaluations(shape, family, rescale):
    pb, ref, folded = _oracle(shape, family, rescale)
    what = f"{shape} {family} rescale={rescale}"
    levels = iu.levels(pb)
    with engine_from_problem(pb, rescale=_policy(rescale)) as e:  # the default engine: the tree walks
        e.set_profiling(True)
        shares, (lower, upper) = _gradient_shares(e, ref)
        print(f"{what}: {lower} post-order and {upper} pre-order launches on {levels} levels")
        if pb.S == 4:  # (as tests/test_invalidation_gpu.py tells the walks from the level kernels: 1 or 2 launches, not one per level)
            assert levels >= 4 and lower in (1, 2) and upper in (1, 2), (levels, lower, upper)
            shares.update({"folded " + k: v for k, v in _gradient_shares(e, folded, GRAD_FOLD_ROOT_FREQS)[0].items()})
        else:  # the post-order walk exists at 20 states unscaled; the pre-order pass is always the level kernels'
            assert e.general_profile()["lower_family"] == (1 if pb.S == 20 and not rescale else 0)
        assert e.rescaling == bool(rescale)
        _report(what + " walks", shares)
    with engine_from_problem(pb, rescale=_policy(rescale)) as e:  # keeping partials: the level kernels
        e.set_profiling(True)
        e.set_keep_partials(True)
        shares, (lower, upper) = _gradient_shares(e, ref)
        print(f"{what}: {lower} post-order and {upper} pre-order launches on {levels} levels, keeping partials")
        if pb.S == 4:
            assert lower >= 3 and upper >= 3, (levels, lower, upper)
            shares.update({"folded " + k: v for k, v in _gradient_shares(e, folded, GRAD_FOLD_ROOT_FREQS)[0].items()})
            e.gradient()  # (the uppers read back below are the plain form's)
        else:
            assert e.general_profile()["lower_family"] == 0
        floor = eu.partial_floor(family)
        shares["lower"] = max(eu.share_partials(e.partials(n), ref["lower"][n], floor, own_units=bool(rescale)) for n in range(pb.T, pb.N))
        shares["upper"] = max(eu.share_partials(e.partials(n, upper=True), ref["upper"][n], floor, own_units=bool(rescale))
                              for n in range(pb.N) if n != pb.root)
        _report(what + " levels", shares)


# ---------------------------------------------------------------------------------------------------------
# branch derivatives
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rescale", [0, 1])
@pytest.mark.parametrize("family", eu.FAMILIES)
@pytest.mark.parametrize("shape", HESS)
def test_branch_hessian_diagonal(shape, family, rescale):
    pb, ref, _ = _oracle(shape, family, rescale)
    _, r1, r2 = branch_hessian_diagonal(pb)
    with engine_from_problem(pb, rescale=_policy(rescale)) as e:
        lnl, d1, d2 = e.branch_hessian_diagonal()
        assert d1[pb.root] == 0.0 and d2[pb.root] == 0.0
        _report(f"{shape} {family} rescale={rescale} hessian diagonal", dict(lnl=eu.share_lnl(lnl, ref["lnl"]), d1=eu.share_gradient(d1, r1), d2=eu.share_gradient(d2, r2)))


@pytest.mark.parametrize("family", eu.FAMILIES)
def test_branch_hessian(family):
    """the full Hessian on the 9-taxon shape against the brute-force restatement (tests/full_hessian_util.py)"""
    pb = eu.case("4s_t9", family)
    lr, gr, Hr = brute_force(pb)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        lnl, g, H = e.branch_hessian()
    assert not H[pb.root].any() and not H[:, pb.root].any()
    _report(f"4s_t9 {family} full hessian", dict(lnl=eu.share_lnl(lnl, lr), g=eu.share_gradient(g, gr), H=eu.share_gradient(H, Hr)))


@functools.lru_cache(maxsize=None)
def _trials(shape, family):
    pb = eu.case(shape, family)
    return [(n, t, eu.oracle_branch(pb, n, t)) for n, t in eu.branch_trials(shape, family)]


@pytest.mark.parametrize("route", ["resident", "path"])
@pytest.mark.parametrize("family", eu.FAMILIES)
@pytest.mark.parametrize("shape", HESS)
def test_branch_log_likelihood(shape, family, route):
    """t in {0, 1e-10, 50} on a branch of ordinary length, an ordinary t on a zero-length branch: from the resident uppers of a
    keep-partials gradient, and on a default engine, where the call walks the path from the branch to the root itself"""
    pb = eu.case(shape, family)
    shares = {}
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        if route == "resident":
            e.set_keep_partials(True)
        e.gradient()
        for n, t, ref in _trials(shape, family):
            if route == "resident":
                e.partials(n, upper=True)  # (resident: readable)
            s = eu.share_branch(e.branch_log_likelihood(n, t), ref)
            shares.update({f"node {n} t={t:g} lnl": s[0], f"node {n} t={t:g} d1": s[1], f"node {n} t={t:g} d2": s[2]})
    _report(f"{shape} {family} branch trials, {route}", shares)


@pytest.mark.parametrize("family", eu.FAMILIES)
@pytest.mark.parametrize("shape,route", [(s, r) for s in eu.SHAPES for r in (("walk", "levels") if eu.SHAPES[s][0] == 4 else ("levels",))])
def test_parameter_gradient(shape, route, family):
    """a random dQ against the oracle, whose dP/dtheta tests/test_parameter_matrix_oracle.py pins: 4 states on the walk and on the
    level kernels (asserted from the profile); 20 and 61 states have the one route, on stored partials"""
    pb, ref, _ = _oracle(shape, family, 0)
    dQ = eu.random_dq(pb.S, 2, seed=5)
    _, pg_ref = po.parameter_gradient(pb, dQ)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        e.set_profiling(True)
        if route == "levels":
            e.set_keep_partials(True)
        e.set_rate_matrix_derivatives(dQ)
        lnl, cg, pg = e.parameter_gradient()
        if pb.S == 4:
            up = e.profile()["upper_launches"]
            assert (up in (1, 2)) if route == "walk" else up >= 3, up
        assert np.all(np.isfinite(pg))
        _report(f"{shape} {family} parameter gradient, {route}",
                dict(lnl=eu.share_lnl(lnl, ref["lnl"]), gradient=eu.share_gradient(cg, ref["cat_grad"]), parameters=eu.share_gradient(pg, pg_ref)))


def test_parameter_gradient_beyond_the_range_of_exp():
    """20 states with one branch at 700.  k_param_outer_gen formed F_ab as e^{l_b t} expm1((l_a - l_b) t) / (l_a - l_b): with
    (l_a - l_b) t r above 709 that is 0 * inf, and the whole parameter gradient was NaN.  exp_divided_difference puts the larger
    eigenvalue in front (phyamd_device.inc), where nothing overflows.  Found by reading the kernel while moving the 4-state
    routes to its form."""
    pb = eu.beyond_exp_case()
    ref = pb.gradient()
    dQ = eu.random_dq(pb.S, 2, seed=5)
    _, pg_ref = po.parameter_gradient(pb, dQ)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        e.set_rate_matrix_derivatives(dQ)
        lnl, cg, pg = e.parameter_gradient()
    print("parameter gradient", pg, "oracle", pg_ref)
    assert np.all(np.isfinite(pg))
    _report("20s long, one branch at 700", dict(lnl=eu.share_lnl(lnl, ref["lnl"]), gradient=eu.share_gradient(cg, ref["cat_grad"]),
                                                 parameters=eu.share_gradient(pg, pg_ref)))


# ---------------------------------------------------------------------------------------------------------
# batched and topology calls (4 states)
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", eu.FAMILIES)
@pytest.mark.parametrize("shape", FOUR)
def test_gradient_batches(shape, family):
    """three items: the case's lengths, and every positive length halved and doubled (zeros stay zero)"""
    pb = eu.case(shape, family)
    items = [eu.scaled(pb, f) for f in eu.BATCH_FACTORS]
    refs = [q.gradient() for q in items]
    bl = np.stack([q.branch_lengths for q in items])
    shares = {}
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        lnl, g = e.gradient_batch(bl)
        assert e.batch_profile()["items_fast"] == 3
        left, right, roots = np.stack([pb.left] * 3), np.stack([pb.right] * 3), np.full(3, pb.root, dtype=np.int32)
        tl, tg = e.gradient_batch_trees(left, right, roots, bl)
        assert e.batch_profile()["items_fast"] == 3
        for i, f in enumerate(eu.BATCH_FACTORS):
            shares[f"x{f:g} lnl"], shares[f"x{f:g} gradient"] = eu.share_lnl(lnl[i], refs[i]["lnl"]), eu.share_gradient(g[i], refs[i]["cat_grad"])
            shares[f"trees x{f:g} lnl"], shares[f"trees x{f:g} gradient"] = eu.share_lnl(tl[i], refs[i]["lnl"]), eu.share_gradient(tg[i], refs[i]["cat_grad"])
    _report(f"{shape} {family} batches", shares)


@functools.lru_cache(maxsize=None)
def _nni_reference(shape, family, central):
    return eu.nni_oracle(eu.case(shape, family), central)


@pytest.mark.parametrize("central", eu.NNI_CENTRALS)
@pytest.mark.parametrize("family", eu.NNI_FAMILIES)
@pytest.mark.parametrize("shape", FOUR)
def test_nni_log_likelihoods(shape, family, central):
    """every entry: lnL and d1 against the oracle on the rearranged tree, d2 against a second engine's Hessian diagonal on that
    tree (as tests/test_nni_gpu.py does); at the engine's own lengths, and with every central edge at 0 and at 30"""
    pb = eu.case(shape, family)
    cand = eu.nni_candidates(pb)
    rl, r1 = _nni_reference(shape, family, central)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e, engine_from_problem(pb, rescale=RESCALE_NEVER) as second:
        lnl, d1, d2 = e.nni_log_likelihoods(eu.nni_central(pb, central))
        assert e.nni_profile()["candidates"] == len(cand) and not e.rescaling
        r2 = np.full((3, pb.N), np.nan)
        for v in cand:
            t = pb.branch_lengths[v] if central == "own" else float(central)
            for k in range(3):
                q = eu.nni_problem(pb, v, k, t)
                second.set_topology(q.left, q.right, q.root)
                second.set_branch_lengths(q.branch_lengths)
                r2[k, v] = second.branch_hessian_diagonal()[2][v]
    non = [n for n in range(pb.N) if n not in cand]
    assert all(np.all(np.isnan(a[:, non])) and np.all(np.isfinite(a[:, cand])) for a in (lnl, d1, d2))
    shares = dict(lnl=float(np.max(np.abs(lnl[:, cand] - rl[:, cand]) / (eu.TOL_LNL * np.abs(rl[:, cand])))),
                  d1=eu.share_gradient(d1[:, cand], r1[:, cand]), d2=eu.share_gradient(d2[:, cand], r2[:, cand]))
    zero = [v for v in cand if central == 0.0 or (central == "own" and pb.branch_lengths[v] == 0.0)]
    if zero:  # a zero-length central edge joins four subtrees in one point: its three arrangements are one tree
        shares["arrangements of a zero-length edge"] = float(np.max(np.abs(lnl[1:, zero] - lnl[0, zero]) / (eu.TOL_LNL * np.abs(lnl[0, zero]))))
    assert zero or family in ("tiny_internal", "long") or central == 30.0
    _report(f"{shape} {family} nni central={central}", shares)


@pytest.mark.parametrize("shape", FOUR)
def test_nni_optimize_stays_on_the_lower_bound(shape):
    """row 0 of a zero-length candidate at which the oracle's d1 is negative on the lower bound: the rule's first evaluation closes
    the bracket there, so the call returns `lower` itself, d1 <= 0, and the oracle's lnL at `lower`"""
    pb = eu.case(shape, "zero_internal")
    lower = 1e-8
    zero = [v for v in eu.nni_candidates(pb) if pb.branch_lengths[v] == 0.0]
    refs = {v: nni_evaluate(pb, v, 0, lower) for v in zero}
    gscale = max(1.0, max(abs(r[1]) for r in refs.values()))
    held = [v for v in zero if refs[v][1] <= -1e-6 * gscale]  # (clear of the bound by 1000 times the d1 tolerance)
    print(f"{shape}: zero-length candidates {zero}, d1 at the lower bound {[refs[v][1] for v in zero]}")
    assert held
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        lengths, lnl, d1, d2, it = e.nni_optimize(lower=lower)
    shares = {}
    for v in held:
        assert lengths[0, v] == lower and d1[0, v] <= 0.0 and it[0, v] >= 1, (v, lengths[0, v], d1[0, v], it[0, v])
        shares[f"node {v} lnl"] = eu.share_lnl(lnl[0, v], refs[v][0])
        shares[f"node {v} d1"] = abs(d1[0, v] - refs[v][1]) / (eu.TOL_GRADIENT * gscale)
    _report(f"{shape} zero_internal nni_optimize", shares)


# ---------------------------------------------------------------------------------------------------------
# posteriors and shards
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", eu.POSTERIOR_FAMILIES)
@pytest.mark.parametrize("shape", list(eu.SHAPES))
def test_posteriors(shape, family):
    pb = eu.case(shape, family)
    ref = eu.posteriors(pb)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        post, states = e.state_posteriors()
        R, mean = e.site_rate_posteriors()
    sure = ref["gap"] >= GAP
    assert np.array_equal(states[sure], ref["states"][sure])
    shares = dict(states=np.abs(post - ref["post"]).max() / 1e-9, rates=np.abs(R - ref["R"]).max() / 1e-9,
                  mean_rate=np.abs(mean - ref["mean"]).max() / (1e-9 * max(1.0, np.abs(ref["mean"]).max())))
    for tip, parent, seen in eu.zero_tip_parents(pb):  # the node above a zero-length tip IS the tip
        ind = np.eye(pb.S)[pb.tip_states[tip][seen]]
        shares["indicator above a zero-length tip"] = max(shares.get("indicator above a zero-length tip", 0.0), np.abs(post[parent][seen] - ind).max() / 1e-9)
        assert np.array_equal(states[parent][seen], pb.tip_states[tip][seen])
    assert ("indicator above a zero-length tip" in shares) == ("zero_tips" in family)
    _report(f"{shape} {family} posteriors", shares)


def test_two_shards_return_the_one_engine_bits():
    pb, ref, _ = _oracle("4s_t24", "zero_internal+long", 0)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        one = e.gradient()
        _report("4s_t24 zero_internal+long one engine", _gradient_shares(e, ref)[0])
    with engine_from_problem(pb, rescale=RESCALE_NEVER, devices=[0, 0]) as e:
        assert e.shard_count == 2
        two = e.gradient()
    assert two[0] == one[0] and np.array_equal(two[1], one[1])
