"""GPU: phyamd_nni_log_likelihoods_general -- lnL and its first two derivatives in the central branch for every NNI neighbour of a
20-state engine's tree, from the resident partials and one launch over the edges -- entry by entry against the CPU oracle alone,
which knows nothing of the shortcut.  Entry (k, v) at trial length t: the rearranged tree is built in numpy
(invalidation_util.rearranged), and the reference is hessian_util.branch_hessian_diagonal of that oracle problem: its lnL and its
rows v of d1 and d2.  Tolerances are the suite's for these quantities (tests/test_nni_gpu.py, tests/test_general_tiles_gpu.py): lnL
1e-10 relative, d1 and d2 1e-9 * max(1, |ref|).  Then the call against the same engine's own evaluations, bit for bit across calls,
the engine afterwards, underflow in band and every refusal."""
import copy
import functools

import numpy as np
import pytest

import pair_distance_general_util as gu
from gpu_util import engine_from_problem, random_problem
from hessian_util import branch_hessian_diagonal
from invalidation_util import parents as _parents, rearranged as _rearranged
from physher_amd.engine import GRAD_FOLD_ROOT_FREQS, RESCALE_ALWAYS, RESCALE_AUTO, RESCALE_NEVER, Engine, EngineError
from test_batch_gpu import _bits, _deep
from test_tree_batch_gpu import _relabel

pytestmark = pytest.mark.gpu
EINVAL, EUNSUPPORTED = -1, -4
NAME = "phyamd_nni_log_likelihoods_general"
TILE, BLOCK = 16, 128  # patterns of a wave's tile and of a workgroup

# (T, shape, P, C, gaps, pinv, engine tip sets, relabelled): the smallest shapes where the kernel can go wrong
CASES = {
    "t3_p5_c1": (3, "random", 5, 1, 0.0, None, 0, False),
    "t4_caterpillar_p16_c4": (4, "caterpillar", 16, 4, 0.0, None, 0, False),
    "t4_balanced_p17_c2": (4, "balanced", 17, 2, 0.0, None, 0, False),
    "t9_random_p130_c8_sets": (9, "random", 130, 8, 0.08, None, 3, False),
    "t9_caterpillar_p70_c4_pinv": (9, "caterpillar", 70, 4, 0.0, 0.25, 0, False),
    "t9_relabelled_p64_c1": (9, "random", 64, 1, 0.0, None, 0, True),
    "t17_random_p200_c4": (17, "random", 200, 4, 0.0, None, 0, False),
}


def _candidates(pb):
    return [v for v in range(pb.T, pb.N) if v != pb.root]


def _trial_lengths(pb, seed):
    """random trial lengths in [0.5 t_v, 2 t_v], different per k"""
    return pb.branch_lengths[None, :] * np.random.default_rng(seed).uniform(0.5, 2.0, size=(3, pb.N))


def _reference(pb, central):
    """(lnl, d1, d2) [3][N] of the oracle for every entry: NaN at tips and the root"""
    out = np.full((3, 3, pb.N), np.nan)
    base = None
    for v in _candidates(pb):
        for k in range(3):
            if k == 0 and central is None:  # the engine's tree at its own lengths: one problem for every candidate
                if base is None:
                    base = branch_hessian_diagonal(pb)
                r = base
            else:
                q = copy.copy(pb)
                q.left, q.right, q.branch_lengths = _rearranged(pb, v, k, pb.branch_lengths[v] if central is None else central[k, v])
                r = branch_hessian_diagonal(q)
            out[:, k, v] = r[0], r[1][v], r[2][v]
    return out


@functools.lru_cache(maxsize=None)
def _case(name):
    """(problem, tip mode, trial lengths, the oracle's entries at the engine's own lengths, ... at the trial lengths), computed once"""
    T, shape, P, C, gaps, pinv, tip_sets, relabel = CASES[name]
    pb = random_problem(T, P, C, seed=7 * T + P + C, S=20, shape=shape, gaps=gaps, pinv=pinv)
    if relabel:
        tree, _ = _relabel((pb.left, pb.right, pb.root, pb.branch_lengths), np.random.default_rng(3), pb.T)
        pb.left, pb.right, pb.root, pb.branch_lengths = tree[0], tree[1], tree[2], tree[3]
    if tip_sets:
        gu.with_sets(pb, tip_sets, 0.1, 7 * T + P + C + 1)
    central = _trial_lengths(pb, 5)
    if name == "t17_random_p200_c4":  # one entry at t = 0 and one at t = 10
        cand = _candidates(pb)
        central[1, cand[2]] = 0.0
        central[2, cand[5]] = 10.0
    own, trial = _reference(pb, None), _reference(pb, central)
    for a in (central, own, trial):
        a.setflags(write=False)
    return pb, ("partials" if tip_sets else "states"), central, own, trial


def _check(got, ref, pb, what):
    cand = _candidates(pb)
    non = [n for n in range(pb.N) if n not in cand]
    for a in got:
        assert a.shape == (3, pb.N) and np.all(np.isnan(a[:, non])) and np.all(np.isfinite(a[:, cand])), what
    lnl, d1, d2 = (a[:, cand] for a in got)
    rl, r1, r2 = (a[:, cand] for a in ref)
    err = [np.abs(lnl - rl) / np.abs(rl), np.abs(d1 - r1) / np.maximum(1.0, np.abs(r1)), np.abs(d2 - r2) / np.maximum(1.0, np.abs(r2))]
    print(f"{what}: {lnl.size} entries, worst lnL {err[0].max():.3e} d1 {err[1].max():.3e} d2 {err[2].max():.3e}")
    assert err[0].max() <= 1e-10, (what, np.unravel_index(np.argmax(err[0]), err[0].shape))
    assert err[1].max() <= 1e-9, (what, np.unravel_index(np.argmax(err[1]), err[1].shape))
    assert err[2].max() <= 1e-9, (what, np.unravel_index(np.argmax(err[2]), err[2].shape))


@pytest.mark.parametrize("case", sorted(CASES))
def test_every_entry_matches_the_oracle(case):
    pb, tip_mode, central, own, trial = _case(case)
    parent, cand = _parents(pb), _candidates(pb)
    tip = lambda n: n < pb.T
    sibling = lambda v: pb.left[parent[v]] if pb.left[parent[v]] != v else pb.right[parent[v]]
    if case == "t3_p5_c1":  # one candidate: its parent is the root, its sibling and children are tips; less than one tile
        (v,) = cand
        assert parent[v] == pb.root and tip(sibling(v)) and tip(pb.left[v]) and tip(pb.right[v]) and pb.P < TILE
    if case == "t4_caterpillar_p16_c4":  # exactly one tile; a candidate whose parent is not the root; a tip sibling
        assert pb.P == TILE and any(parent[v] != pb.root for v in cand) and any(tip(sibling(v)) for v in cand)
    if case == "t4_balanced_p17_c2":  # both candidates under the root, each the other's stored sibling; a ragged second tile
        assert len(cand) == 2 and all(parent[v] == pb.root for v in cand) and sibling(cand[0]) == cand[1] and TILE < pb.P < 2 * TILE
    if case == "t9_random_p130_c8_sets":  # a workgroup's patterns and a bit, the most categories, unknown cells and engine sets
        codes = gu.codes_from_problem(pb)[0]
        assert BLOCK < pb.P < BLOCK + TILE and pb.C == 8 and np.any(codes == 20) and np.any(codes > 20)
    if case == "t9_caterpillar_p70_c4_pinv":  # a zero-rate category
        assert pb.cat_rates[0] == 0.0 and pb.cat_props[0] == 0.25
        assert any(not tip(pb.left[v]) or not tip(pb.right[v]) for v in cand)  # a stored child
    if case == "t9_relabelled_p64_c1":  # internal ids permuted, the root not 2T-2
        assert pb.root != pb.N - 1
    if case == "t17_random_p200_c4":
        assert np.count_nonzero(central[:, cand] == 0.0) == 1 and np.count_nonzero(central[:, cand] == 10.0) == 1
        assert any(not tip(sibling(v)) and parent[v] != pb.root for v in cand)  # a stored sibling below a stored parent
    assert len(set(pb.weights)) > 1  # weights that are not uniform
    with engine_from_problem(pb, rescale=RESCALE_AUTO, tip_mode=tip_mode) as e:
        _check(e.nni_log_likelihoods_general(), own, pb, case + " own lengths")
        prof = e.nni_profile()
        assert prof["candidates"] == pb.T - 2 and prof["scratch_bytes"] > 0 and not e.rescaling, prof
        _check(e.nni_log_likelihoods_general(central), trial, pb, case + " trial lengths")


def test_row_zero_is_the_engines_own_evaluation():
    pb, tip_mode, _, _, _ = _case("t17_random_p200_c4")
    cand = _candidates(pb)
    with engine_from_problem(pb, rescale=RESCALE_AUTO, tip_mode=tip_mode) as e:
        lnl, d1, d2 = e.nni_log_likelihoods_general()
        own = e.log_likelihood()
        _, h1, h2 = e.branch_hessian_diagonal()
    print(f"row 0: lnL {np.abs(lnl[0, cand] - own).max() / abs(own):.3e} d1 {np.abs(d1[0, cand] - h1[cand]).max():.3e} d2 {np.abs(d2[0, cand] - h2[cand]).max():.3e}")
    assert np.abs(lnl[0, cand] - own).max() <= 1e-12 * abs(own)
    assert np.all(np.abs(d1[0, cand] - h1[cand]) <= 1e-9 * np.maximum(1.0, np.abs(h1[cand])))
    assert np.all(np.abs(d2[0, cand] - h2[cand]) <= 1e-9 * np.maximum(1.0, np.abs(h2[cand])))


def test_folded_uppers_are_used_as_they_are():
    """after a PHYAMD_GRAD_FOLD_ROOT_FREQS keep-partials gradient the resident uppers carry pi and the call leaves pi out.  That
    arithmetic is the likelihood's for uniform frequencies only (include/physher_amd.h), so the problem has them: every entry
    against the oracle at the same tolerances, under and beside the root"""
    from golden_util import reversible_eigen
    from oracle import phyoracle as po
    src = random_problem(9, 70, 2, seed=41, S=20, gaps=0.05)
    rng = np.random.default_rng(42)
    r = rng.uniform(0.5, 3.0, size=(20, 20))
    freqs = np.full(20, 1.0 / 20)
    ev, U, Ui = reversible_eigen(0.5 * (r + r.T), freqs)
    pb = po.Problem(src.left, src.right, src.root, src.weights, ev, U, Ui, freqs, src.cat_rates, src.cat_props, src.branch_lengths, tip_states=src.tip_states)
    parent = _parents(pb)
    assert any(parent[v] == pb.root for v in _candidates(pb)) and any(parent[v] != pb.root for v in _candidates(pb))
    central = _trial_lengths(pb, 5)
    ref = _reference(pb, central)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        e.set_keep_partials(True)
        e.gradient(GRAD_FOLD_ROOT_FREQS)
        _check(e.nni_log_likelihoods_general(central), ref, pb, "folded uppers")
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        _check(e.nni_log_likelihoods_general(central), ref, pb, "plain uppers")


def _same(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def test_bits_do_not_depend_on_the_call_the_scratch_or_the_other_entries():
    pb, tip_mode, central, _, _ = _case("t9_random_p130_c8_sets")
    cand = _candidates(pb)
    with engine_from_problem(pb, rescale=RESCALE_AUTO, tip_mode=tip_mode) as e:
        first = e.nni_log_likelihoods_general(central)
        assert _same(first, e.nni_log_likelihoods_general(central))
        e.pairwise_distances_general(counts_only=True, want_counts=True)  # (another call in the same scratch)
        assert _same(first, e.nni_log_likelihoods_general(central))
        lo, n1, n2 = e.nni_log_likelihoods_general(central, want_derivatives=False)
        assert n1 is None and n2 is None and np.array_equal(_bits(lo), _bits(first[0]))
        # an entry's bits are its own: every other entry's trial length changed
        k, v = 1, cand[3]
        other = np.array(_trial_lengths(pb, 6))
        other[k, v] = central[k, v]
        moved = e.nni_log_likelihoods_general(other)
        assert all(_bits(a[k, v]) == _bits(b[k, v]) for a, b in zip(moved, first))
        assert not np.array_equal(_bits(moved[0][:, cand]), _bits(first[0][:, cand]))
        assert not e.rescaling
    with engine_from_problem(pb, rescale=RESCALE_AUTO, tip_mode=tip_mode) as e:  # a scratch that held nothing before
        assert _same(first, e.nni_log_likelihoods_general(central))


def test_the_engine_afterwards_is_a_keep_partials_engine_with_the_same_bits():
    """the engine after the call against a fresh engine with set_keep_partials(True) that never made the call: the same bits from
    every later evaluation, also after a change of a length; topology, lengths and models stay"""
    pb, tip_mode, central, _, _ = _case("t9_random_p130_c8_sets")
    ref = pb.gradient()
    with engine_from_problem(pb, rescale=RESCALE_AUTO, tip_mode=tip_mode) as a, engine_from_problem(pb, rescale=RESCALE_AUTO, tip_mode=tip_mode) as b:
        first = a.nni_log_likelihoods_general(central)
        assert not a.rescaling
        b.set_keep_partials(True)
        b.gradient()
        at = a.branch_log_likelihood(0, float(pb.branch_lengths[0]))[0]  # read from the resident partials of a keep-partials engine
        assert abs(at - ref["lnl"]) <= 1e-10 * abs(ref["lnl"])
        for step in range(2):
            la, ga = a.gradient()
            lb, gb = b.gradient()
            assert _bits(np.array([la, a.log_likelihood()])).tolist() == _bits(np.array([lb, b.log_likelihood()])).tolist(), step
            assert np.array_equal(_bits(ga), _bits(gb)), step
            if step == 0:
                assert abs(la - ref["lnl"]) <= 1e-10 * abs(ref["lnl"])
                assert np.abs(ga - ref["cat_grad"]).max() <= 1e-9 * max(1.0, np.abs(ref["cat_grad"]).max())
                assert _same(a.nni_log_likelihoods_general(central), first)  # a call on an engine already in that state changes nothing
                a.set_branch_length(3, 0.37)
                b.set_branch_length(3, 0.37)
        moved = a.nni_log_likelihoods_general(central)  # a pending change is evaluated by the call
        assert not np.array_equal(_bits(moved[0]), _bits(first[0]))
        assert _bits(np.array([a.log_likelihood()])).tolist() == _bits(np.array([b.log_likelihood()])).tolist()
        assert not a.rescaling


# ---- underflow --------------------------------------------------------------------------------------------------------------------

def _underflow_case():
    """the recipe of underflow_case in tests/test_placement_general_gpu.py: a caterpillar so deep that the oracle's rescaled
    evaluation puts one pattern's log10 site likelihood below -330, past the smallest subnormal number"""
    for T in range(240, 400, 10):
        pb = _deep(T, 6, 2, seed=11, S=20)
        site = np.asarray(pb.log_likelihood()["pattern_lk"]) / np.log(10.0)  # (the oracle rescales: exact past the underflow)
        if site.min() < -330.0:
            return pb, site
    raise AssertionError("no depth puts a pattern's site likelihood below 1e-330")


def test_underflow_is_reported_in_band():
    pb, site = _underflow_case()
    assert site.min() < -330.0 and pb.weights[int(np.argmin(site))] > 0
    cand = _candidates(pb)
    non = [n for n in range(pb.N) if n not in cand]
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        lnl, d1, d2 = e.nni_log_likelihoods_general()  # returns: no error
        assert not e.rescaling
    assert not np.any(np.isfinite(lnl[:, cand]))
    assert np.all(np.isnan(d1[:, cand])) and np.all(np.isnan(d2[:, cand]))
    assert all(np.all(np.isnan(a[:, non])) for a in (lnl, d1, d2))


# ---- refusals ---------------------------------------------------------------------------------------------------------------------

def _refused(e, code=EUNSUPPORTED, **kw):
    with pytest.raises(EngineError) as err:
        e.nni_log_likelihoods_general(**kw)
    assert err.value.code == code, err.value
    print(err.value)
    assert NAME in str(err.value)
    return str(err.value)


def _still_usable(e, pb):
    ref = pb.log_likelihood()["lnl"]
    assert abs(e.log_likelihood() - ref) <= 1e-10 * abs(ref)


def _protein(T=8, P=100, C=2, seed=3, **kw):
    return random_problem(T, P, C, seed=seed, S=20, **kw)


def test_four_states_are_sent_to_the_four_state_call():
    pb = random_problem(8, 100, 2, seed=3)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        msg = _refused(e)
        assert "20 states" in msg and "use phyamd_nni_log_likelihoods)" in msg
        _still_usable(e, pb)


@pytest.mark.parametrize("S", [60, 61])
def test_codon_state_counts_are_not_built(S):
    pb = random_problem(5, 40, 1, seed=S, S=S)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        msg = _refused(e)
        assert "not built" in msg and str(S) in msg
        _still_usable(e, pb)


def test_nine_categories_are_refused():
    pb = _protein(C=9, seed=9)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        assert "categories" in _refused(e)
        _still_usable(e, pb)


def test_flags_are_refused():
    pb = _protein()
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        assert "flags" in _refused(e, flags=1)
        _still_usable(e, pb)
        e.nni_log_likelihoods_general()


def test_a_missing_eigen_system_is_refused():
    pb = _protein()
    with Engine(pb.T, pb.P, 20, pb.C, rescale=RESCALE_NEVER) as e:
        e.set_topology(pb.left, pb.right, pb.root)
        e.set_branch_lengths(pb.branch_lengths)
        e.set_frequencies(pb.freqs)
        e.set_category_rates(pb.cat_rates, pb.cat_props)
        e.set_pattern_weights(pb.weights)
        for t in range(pb.T):
            e.set_tip_states(t, pb.tip_states[t])
        assert "eigen" in _refused(e, code=EINVAL)


def test_a_rescaling_engine_is_refused():
    pb = _protein(T=20, P=60, C=2, seed=12, gaps=0.03, rescale=1)
    with engine_from_problem(pb, rescale=RESCALE_ALWAYS) as e:
        assert "rescal" in _refused(e)
        _still_usable(e, pb)


def test_an_engine_that_switches_to_rescaling_during_the_call_is_refused():
    pb = _deep(600, 20, 2, seed=5, S=20)
    with engine_from_problem(pb, rescale=RESCALE_AUTO) as e:
        assert not e.rescaling
        msg = _refused(e)
        assert "rescal" in msg and "PHYAMD_RESCALE_AUTO" in msg
        assert e.rescaling
        _still_usable(e, pb)


def test_a_tiled_engine_is_refused():
    pb = _protein(T=20, P=2000, C=2, seed=13, gaps=0.03)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        e.gradient()
        base = e.profile()["device_bytes"]
    cap = None
    for frac in np.arange(0.9, 0.1, -0.05):  # (the search of tests/test_nni_gpu.py for a cap that tiles)
        try:
            with engine_from_problem(pb, rescale=RESCALE_NEVER, max_device_bytes=int(frac * base)) as e:
                if e.profile()["tiles"] >= 2:
                    cap = int(frac * base)
                    break
        except EngineError:
            pass
    assert cap is not None, "no cap puts this problem into tiles"
    with engine_from_problem(pb, rescale=RESCALE_NEVER, max_device_bytes=cap) as e:
        assert e.profile()["tiles"] > 1
        assert "tiled" in _refused(e)
        _still_usable(e, pb)


def test_explicit_matrices_are_refused():
    pb = _protein()
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        e.gradient()
        e.set_node_matrices(2, e.node_matrices(2))
        assert "explicit matrices" in _refused(e)
        _still_usable(e, pb)


def test_a_sharded_handle_is_refused():
    pb = _protein(P=200)
    with engine_from_problem(pb, rescale=RESCALE_NEVER, devices=[0, 0]) as e:
        assert e.shard_count == 2
        assert "shard" in _refused(e)
        _still_usable(e, pb)


def test_a_bad_trial_length_counts_only_at_a_candidate():
    pb = _protein()
    central = _trial_lengths(pb, 1)
    v = _candidates(pb)[1]
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        want = e.nni_log_likelihoods_general(central)
        for bad in (-0.01, np.nan):
            broken = central.copy()
            broken[2, v] = bad
            msg = _refused(e, code=EINVAL, central_lengths=broken)
            assert "central_lengths" in msg and f"[{v}]" in msg, msg
        ignored = central.copy()
        ignored[:, 0] = -1.0             # a tip
        ignored[1, pb.root] = np.nan     # the root
        assert _same(want, e.nni_log_likelihoods_general(ignored))
