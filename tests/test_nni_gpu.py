"""GPU: phyamd_nni_log_likelihoods -- lnL and its first two derivatives in the central branch for every NNI neighbour of the engine's
tree, from one post-order walk, one pre-order walk and one launch over the edges -- entry by entry against references that know
nothing of the shortcut.  Entry (k, v): the rearranged tree is built in numpy (the two child slots exchanged, the length of v set);
lnl is the CPU oracle's log-likelihood of that tree, d1 the oracle's per-category gradient through branch_gradient_from_cat at row
v, d2 phyamd_branch_hessian_diagonal's row v on a second engine given the rearranged tree through set_topology (and, on one case,
a central difference of the oracle's d1 in t_v).  Tolerances are the suite's for single evaluations
(tests/test_branch_hessian_gpu.py, tests/test_tree_batch_gpu.py): lnL 1e-10 relative, d1 and d2 1e-9 * max(1, |ref|).  Then the
call against the same engine's own evaluations, bit for bit across calls, under a memory cap, through every refusal, with
underflowing partials and on a sharded handle."""
import copy

import numpy as np
import pytest

from gpu_util import engine_from_problem, random_problem
from invalidation_util import parents as _parents, rearranged as _rearranged  # (the NNI neighbours are built there)
from oracle.phyoracle import branch_gradient_from_cat
from physher_amd.engine import GRAD_FOLD_ROOT_FREQS, RESCALE_ALWAYS, RESCALE_AUTO, RESCALE_NEVER, EngineError
from test_batch_gpu import _ambiguous_partials, _bits, _deep
from test_tree_batch_gpu import _relabel

pytestmark = pytest.mark.gpu
EINVAL, EUNSUPPORTED = -1, -4


def _candidates(pb):
    return [v for v in range(pb.T, pb.N) if v != pb.root]


def _reference(pb, ref_engine, v, k, t):
    """(lnl, d1, d2) of entry (k, v) at trial length t"""
    left, right, bl = _rearranged(pb, v, k, t)
    q = copy.copy(pb)
    q.left, q.right, q.branch_lengths = left, right, bl
    r = q.gradient()
    d1 = branch_gradient_from_cat(r["cat_grad"], pb.cat_rates, pb.cat_props)[v]
    ref_engine.set_topology(left, right, pb.root)
    ref_engine.set_branch_lengths(bl)
    _, _, h2 = ref_engine.branch_hessian_diagonal()
    return r["lnl"], d1, h2[v]


def _trial_lengths(pb, seed):
    """random trial lengths in [0.5 t_v, 2 t_v], different per k"""
    return pb.branch_lengths[None, :] * np.random.default_rng(seed).uniform(0.5, 2.0, size=(3, pb.N))


def _check_entries(pb, e, ref_engine, central, entries, what):
    lnl, d1, d2 = e.nni_log_likelihoods(central)
    assert e.nni_profile()["candidates"] == pb.T - 2 and not e.rescaling
    worst = np.zeros(3)
    base = None  # (k = 0 at the engine's own lengths: one tree for every candidate)
    for k, v in entries:
        t = pb.branch_lengths[v] if central is None else central[k, v]
        if k == 0 and central is None:
            if base is None:
                q = copy.copy(pb)
                r = q.gradient()
                ref_engine.set_topology(pb.left, pb.right, pb.root)
                ref_engine.set_branch_lengths(pb.branch_lengths)
                base = (r["lnl"], branch_gradient_from_cat(r["cat_grad"], pb.cat_rates, pb.cat_props), ref_engine.branch_hessian_diagonal()[2])
            rl, r1, r2 = base[0], base[1][v], base[2][v]
        else:
            rl, r1, r2 = _reference(pb, ref_engine, v, k, t)
        err = np.array([abs(lnl[k, v] - rl) / abs(rl), abs(d1[k, v] - r1) / max(1.0, abs(r1)), abs(d2[k, v] - r2) / max(1.0, abs(r2))])
        worst = np.maximum(worst, err)
        assert err[0] <= 1e-10, (what, k, v, lnl[k, v], rl)
        assert err[1] <= 1e-9, (what, k, v, d1[k, v], r1)
        assert err[2] <= 1e-9, (what, k, v, d2[k, v], r2)
    print(f"{what}: {len(entries)} entries, worst lnL {worst[0]:.3e} d1 {worst[1]:.3e} d2 {worst[2]:.3e}")
    non = [n for n in range(pb.N) if n < pb.T or n == pb.root]
    assert np.all(np.isnan(lnl[:, non])) and np.all(np.isnan(d1[:, non])) and np.all(np.isnan(d2[:, non]))
    cand = _candidates(pb)
    assert np.all(np.isfinite(lnl[:, cand])) and np.all(np.isfinite(d1[:, cand])) and np.all(np.isfinite(d2[:, cand]))
    return lnl, d1, d2


def _relabelled(pb, seed):
    """the problem's tree with its internal ids permuted, the root somewhere below 2T-2"""
    tree, _ = _relabel((pb.left, pb.right, pb.root, pb.branch_lengths), np.random.default_rng(seed), pb.T)
    pb.left, pb.right, pb.root, pb.branch_lengths = tree[0], tree[1], tree[2], tree[3]
    assert pb.root != pb.N - 1
    return pb


# (T, P, C, shape, relabel, gaps, pinv, ambiguity codes)
CASES = {
    "t3": (3, 1, 1, "random", False, 0.0, None, False),
    "t4_caterpillar": (4, 63, 2, "caterpillar", False, 0.0, None, False),
    "t4_balanced": (4, 65, 2, "balanced", False, 0.0, None, False),
    "t37_gaps_pinv": (37, 238, 4, "random", False, 0.05, 0.25, False),
    "t37_c8": (37, 700, 8, "random", False, 0.0, None, False),
    "t37_ambiguity": (37, 238, 4, "random", False, 0.05, None, True),
}
for _shape in ("caterpillar", "balanced", "random", "relabelled"):
    for _P in (64, 65):
        CASES[f"t8_{_shape}_p{_P}"] = (8, _P, 1, "random" if _shape == "relabelled" else _shape, _shape == "relabelled", 0.0, None, False)


def _problem(case):
    T, P, C, shape, relabel, gaps, pinv, ambig = CASES[case]
    pb = random_problem(T, P, C, seed=11 * T + P + C, shape=shape, gaps=gaps, pinv=pinv)
    if relabel:
        _relabelled(pb, 3)
    if ambig:
        _ambiguous_partials(pb, 3)
    return pb, ("partials" if ambig else "states")


@pytest.mark.parametrize("case", sorted(CASES))
def test_every_entry_matches_the_references(case):
    pb, tip_mode = _problem(case)
    parent = _parents(pb)
    if case == "t3":  # one candidate: its parent is the root, its sibling and children are tips
        (v,) = _candidates(pb)
        assert parent[v] == pb.root and max(pb.left[v], pb.right[v]) < pb.T
    if case == "t4_caterpillar":  # a candidate whose parent is not the root
        assert any(parent[v] != pb.root for v in _candidates(pb))
    if case == "t4_balanced":  # both candidates under the root, each the other's sibling
        assert all(parent[v] == pb.root for v in _candidates(pb)) and len(_candidates(pb)) == 2
    entries = [(k, v) for v in _candidates(pb) for k in range(3)]
    with engine_from_problem(pb, rescale=RESCALE_AUTO, tip_mode=tip_mode) as e, engine_from_problem(pb, rescale=RESCALE_AUTO, tip_mode=tip_mode) as ref:
        _check_entries(pb, e, ref, None, entries, case + " own lengths")
        _check_entries(pb, e, ref, _trial_lengths(pb, 5), entries, case + " trial lengths")


def test_two_hundred_taxa():
    """every candidate for k = 0; a fixed seeded sample of 24 candidates for k = 1, 2"""
    pb = random_problem(200, 63, 4, seed=200, gaps=0.02)
    parent, cand = _parents(pb), _candidates(pb)
    under_root = [v for v in cand if parent[v] == pb.root]
    cherries = [v for v in cand if pb.left[v] < pb.T and pb.right[v] < pb.T]
    rng = np.random.default_rng(24)
    sample = {under_root[0], cherries[0]}
    for v in rng.permutation(cand):
        if len(sample) == 24:
            break
        sample.add(int(v))
    sample = sorted(sample)
    assert len(sample) == 24
    assert any(parent[v] == pb.root for v in sample) and any(pb.left[v] < pb.T and pb.right[v] < pb.T for v in sample)
    entries = [(0, v) for v in cand] + [(k, v) for v in sample for k in (1, 2)]
    with engine_from_problem(pb, rescale=RESCALE_AUTO) as e, engine_from_problem(pb, rescale=RESCALE_AUTO) as ref:
        _check_entries(pb, e, ref, None, entries, "t200 own lengths")
        _check_entries(pb, e, ref, _trial_lengths(pb, 6), entries, "t200 trial lengths")


def test_d2_is_the_derivative_of_the_oracles_d1():
    """the definition, cross-checked without any engine: a central difference of the oracle's d1 in t_v, step 1e-4 * max(t_v, 0.01),
    agreement 1e-5 relative"""
    pb = random_problem(8, 65, 2, seed=81, gaps=0.03)
    central = _trial_lengths(pb, 7)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        _, _, d2 = e.nni_log_likelihoods(central)
    for v in _candidates(pb):
        for k in range(3):
            t = central[k, v]
            h = 1e-4 * max(t, 0.01)
            g = []
            for tt in (t - h, t + h):
                q = copy.copy(pb)
                q.left, q.right, q.branch_lengths = _rearranged(pb, v, k, tt)
                g.append(branch_gradient_from_cat(q.gradient()["cat_grad"], pb.cat_rates, pb.cat_props)[v])
            fd = (g[1] - g[0]) / (2 * h)
            print(f"({k}, {v}): d2 {d2[k, v]!r} central difference {fd!r}")
            assert abs(d2[k, v] - fd) <= 1e-5 * abs(fd), (k, v, d2[k, v], fd)


def test_row_zero_is_the_engines_own_evaluation():
    pb = random_problem(37, 238, 4, seed=17, gaps=0.05)
    with engine_from_problem(pb, rescale=RESCALE_AUTO) as e:
        lnl, d1, d2 = e.nni_log_likelihoods()
        own = e.log_likelihood()
        _, h1, h2 = e.branch_hessian_diagonal()
    cand = _candidates(pb)
    non = [n for n in range(pb.N) if n not in cand]
    print(f"row 0: lnL {np.abs(lnl[0, cand] - own).max() / abs(own):.3e} d1 {np.abs(d1[0, cand] - h1[cand]).max():.3e} d2 {np.abs(d2[0, cand] - h2[cand]).max():.3e}")
    assert np.abs(lnl[0, cand] - own).max() <= 1e-10 * abs(own)
    assert np.all(np.abs(d1[0, cand] - h1[cand]) <= 1e-9 * np.maximum(1.0, np.abs(h1[cand])))
    assert np.all(np.abs(d2[0, cand] - h2[cand]) <= 1e-9 * np.maximum(1.0, np.abs(h2[cand])))
    for a in (lnl, d1, d2):
        assert a.shape == (3, pb.N) and np.all(np.isnan(a[:, non])) and np.all(np.isfinite(a[:, cand]))


def test_two_tips_have_no_candidate():
    pb = random_problem(2, 65, 2, seed=2)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        lnl, d1, d2 = e.nni_log_likelihoods()
        assert e.nni_profile()["candidates"] == 0
        assert np.all(np.isnan(lnl)) and np.all(np.isnan(d1)) and np.all(np.isnan(d2))
        ref = pb.log_likelihood()["lnl"]
        assert abs(e.log_likelihood() - ref) <= 1e-10 * abs(ref)


def _same(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def test_bit_for_bit_across_calls_and_the_engine_is_untouched():
    pb = random_problem(37, 700, 4, seed=31, gaps=0.05)
    central = _trial_lengths(pb, 9)
    bl = pb.branch_lengths[None, :] * np.random.default_rng(4).uniform(0.5, 1.8, size=(5, pb.N))
    other = random_problem(37, 700, 4, seed=32)  # (another tree, for the tree batch)
    trees = (other.left[None, :], other.right[None, :], np.array([other.root], dtype=np.int32), other.branch_lengths[None, :])
    with engine_from_problem(pb, rescale=RESCALE_AUTO) as e, engine_from_problem(pb, rescale=RESCALE_AUTO) as fresh:
        before = (e.log_likelihood(), e.gradient(), e.gradient_batch(bl))
        first = e.nni_log_likelihoods(central)
        second = e.nni_log_likelihoods(central)
        assert _same(first, second)
        e.gradient_batch(bl)  # (both batch kinds run in the same scratch, with other op lists and fewer upper slots)
        e.gradient_batch_trees(*trees)
        third = e.nni_log_likelihoods(central)
        assert _same(first, third)
        lo, n1, n2 = e.nni_log_likelihoods(central, want_derivatives=False)
        assert n1 is None and n2 is None and np.array_equal(_bits(lo), _bits(first[0]))
        after = (e.log_likelihood(), e.gradient(), e.gradient_batch(bl))
        assert _bits(before[0]) == _bits(after[0])
        assert _bits(before[1][0]) == _bits(after[1][0]) and np.array_equal(_bits(before[1][1]), _bits(after[1][1]))
        assert _same(before[2], after[2])
        # an engine that never made the call takes the same path from here on
        node = 5 if pb.root != 5 else 6
        for eng in (e, fresh):
            eng.set_branch_length(node, 0.37)
        a, b = e.gradient(), fresh.gradient()
        assert _bits(a[0]) == _bits(b[0]) and np.array_equal(_bits(a[1]), _bits(b[1]))
        assert not e.rescaling
    with engine_from_problem(pb, rescale=RESCALE_AUTO) as e:  # a scratch that held nothing before
        assert _same(first, e.nni_log_likelihoods(central))


def test_under_a_memory_cap():
    pb = random_problem(37, 700, 4, seed=99, gaps=0.05)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        e.gradient()
        e.branch_hessian_diagonal()
        held = e.profile()["device_bytes"]  # (what the engine holds besides the batch scratch)
        want = e.nni_log_likelihoods()
        scratch = e.nni_profile()["scratch_bytes"]
        assert scratch > 0 and e.profile()["device_bytes"] >= held + scratch
    roomy = None
    for extra in (1.1, 1.25, 1.5, 2.0, 3.0, 4.0):  # the smallest of these caps that leaves room for the scratch
        cap = int(held + extra * scratch)
        with engine_from_problem(pb, rescale=RESCALE_NEVER, max_device_bytes=cap) as e:
            e.gradient()
            e.branch_hessian_diagonal()  # (the engine's own buffers are made first: the room is what is left beside them)
            assert e.profile()["tiles"] == 1
            try:
                got = e.nni_log_likelihoods()
            except EngineError as err:
                assert err.code == EUNSUPPORTED and "scratch" in str(err), err
                continue
            roomy = cap
            print(f"cap = held + {extra} x scratch = {cap}: the call runs; device_bytes {e.profile()['device_bytes']}")
            assert e.profile()["device_bytes"] <= cap
            assert _same(want, got)
            break
    assert roomy is not None, "no cap left room for the scratch"
    with engine_from_problem(pb, rescale=RESCALE_NEVER, max_device_bytes=roomy) as e, \
            engine_from_problem(pb, rescale=RESCALE_NEVER, max_device_bytes=roomy) as fresh:
        assert _same(want, e.nni_log_likelihoods())  # made first, before the engine's own buffers
        a, b = e.gradient(), fresh.gradient()
        assert _bits(a[0]) == _bits(b[0]) and np.array_equal(_bits(a[1]), _bits(b[1]))
        ha, hb = e.branch_hessian_diagonal(), fresh.branch_hessian_diagonal()
        assert _same(ha[1:], hb[1:]) and _bits(ha[0]) == _bits(hb[0])
        assert e.profile()["device_bytes"] <= roomy
        assert _same(want, e.nni_log_likelihoods())
        assert e.profile()["device_bytes"] <= roomy
    tight = int(held + scratch / 4)
    with engine_from_problem(pb, rescale=RESCALE_NEVER, max_device_bytes=tight) as e:
        assert e.profile()["tiles"] == 1
        with pytest.raises(EngineError) as err:
            e.nni_log_likelihoods()
        print(err.value)
        assert err.value.code == EUNSUPPORTED and "scratch" in str(err.value)
        _still_usable(e, pb)
        assert e.profile()["device_bytes"] <= tight


def _refused(e, code=EUNSUPPORTED, **kw):
    with pytest.raises(EngineError) as err:
        e.nni_log_likelihoods(**kw)
    assert err.value.code == code, err.value
    print(err.value)
    return str(err.value)


def _still_usable(e, pb):
    ref = pb.log_likelihood()["lnl"]
    assert abs(e.log_likelihood() - ref) <= 1e-10 * abs(ref)


def test_twenty_states_are_refused():
    pb = random_problem(10, 200, 2, seed=20, S=20, gaps=0.03)
    with engine_from_problem(pb, rescale=RESCALE_AUTO) as e:
        assert "4 states" in _refused(e)
        _still_usable(e, pb)


def test_nine_categories_are_refused():
    pb = random_problem(8, 100, 9, seed=9)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        assert "categories" in _refused(e)
        _still_usable(e, pb)


def test_a_rescaling_engine_is_refused():
    pb = random_problem(37, 238, 4, seed=12, gaps=0.03, rescale=1)
    with engine_from_problem(pb, rescale=RESCALE_ALWAYS) as e:
        assert "rescal" in _refused(e)
        _still_usable(e, pb)


def test_an_auto_engine_that_has_switched_is_refused():
    pb = _deep(800, 100, 4, seed=5)
    with engine_from_problem(pb, rescale=RESCALE_AUTO) as e:
        e.log_likelihood()
        assert e.rescaling
        assert "rescal" in _refused(e)
        _still_usable(e, pb)


def test_a_tiled_engine_is_refused():
    pb = random_problem(40, 2000, 4, seed=13, gaps=0.03)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        e.gradient()
        base = e.profile()["device_bytes"]
    cap = None
    for frac in np.arange(0.9, 0.1, -0.05):  # (the search of tests/test_tree_batch_gpu.py for a cap that tiles)
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


def test_an_empty_tip_mask_is_refused():
    pb = random_problem(8, 100, 2, seed=23)
    tp = np.zeros((pb.T, pb.P, 4))
    for t in range(pb.T):
        tp[t, np.arange(pb.P), pb.tip_states[t]] = 1.0
    tp[3, 40] = 0.0  # no state is compatible with this cell
    pb.tip_partials, pb.tip_states = tp, None
    with engine_from_problem(pb, rescale=RESCALE_NEVER, tip_mode="partials") as e:
        assert "empty state mask" in _refused(e)
        e.log_likelihood()


def test_explicit_matrices_are_refused():
    pb = random_problem(8, 100, 2, seed=3)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        e.gradient()
        e.set_node_matrices(2, e.node_matrices(2))
        assert "explicit matrices" in _refused(e)
        _still_usable(e, pb)


def test_flags_are_refused():
    pb = random_problem(8, 100, 2, seed=3)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        assert "flags" in _refused(e, flags=GRAD_FOLD_ROOT_FREQS)
        _still_usable(e, pb)
        e.nni_log_likelihoods()


def test_a_negative_trial_length_counts_only_at_a_candidate():
    pb = random_problem(8, 100, 2, seed=3)
    central = _trial_lengths(pb, 1)
    v = _candidates(pb)[1]
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        want = e.nni_log_likelihoods(central)
        for bad in (-0.01, np.nan, np.inf):
            broken = central.copy()
            broken[2, v] = bad
            msg = _refused(e, code=EINVAL, central_lengths=broken)
            assert "central_lengths" in msg and f"[{v}]" in msg, msg
        ignored = central.copy()
        ignored[:, 0] = -1.0       # a tip
        ignored[1, pb.root] = np.nan  # the root
        assert _same(want, e.nni_log_likelihoods(ignored))


@pytest.mark.parametrize("rescale", [RESCALE_NEVER, RESCALE_AUTO])
def test_underflow_is_reported_in_band(rescale):
    pb = _deep(800, 100, 4, seed=5)
    cand = _candidates(pb)
    with engine_from_problem(pb, rescale=rescale) as e:
        lnl, d1, d2 = e.nni_log_likelihoods()
        assert not e.rescaling  # never a switch to rescaling
        assert not np.any(np.isfinite(lnl[:, cand]))
        assert np.all(np.isnan(d1)) and np.all(np.isnan(d2))


def test_shards_agree_with_one_engine():
    pb = random_problem(37, 700, 4, seed=21, gaps=0.05)
    central = _trial_lengths(pb, 2)
    cand = _candidates(pb)
    with engine_from_problem(pb, rescale=RESCALE_AUTO) as e:
        one = e.nni_log_likelihoods(central)
    with engine_from_problem(pb, rescale=RESCALE_AUTO, devices=[0, 0]) as e:
        assert e.shard_count == 2
        two = e.nni_log_likelihoods(central)
        lo, _, _ = e.nni_log_likelihoods(central, want_derivatives=False)
    print(f"two shards: lnL {np.abs(two[0][:, cand] - one[0][:, cand]).max():.3e} d1 {np.abs(two[1][:, cand] - one[1][:, cand]).max():.3e} "
          f"d2 {np.abs(two[2][:, cand] - one[2][:, cand]).max():.3e}")
    assert np.all(np.abs(two[0][:, cand] - one[0][:, cand]) <= 1e-10 * np.abs(one[0][:, cand]))
    assert np.array_equal(_bits(lo), _bits(two[0]))
    for a, b in ((two[1], one[1]), (two[2], one[2])):
        assert np.all(np.abs(a[:, cand] - b[:, cand]) <= 1e-9 * np.maximum(1.0, np.abs(b[:, cand])))
    non = [n for n in range(pb.N) if n not in cand]
    assert all(np.all(np.isnan(a[:, non])) for a in two)
