"""GPU: phyamd_branch_hessian -- lnL, the branch gradient and the full branch-length Hessian from the partials a keep-partials
gradient leaves resident (phyamd_bhess.inc: the tangent walk, the cousin tiles and the outer-product tiles on the fp64 matrix
pipe) -- against the two NumPy restatements (tests/full_hessian_util.py, pinned on the CPU against each other and against
differences of the oracle's analytic gradient), against the Hessian diagonal's call, and across pattern chunks, shards, scratch
histories and later evaluations."""
import numpy as np
import pytest
import torch

from full_hessian_util import brute_force, message_form
from golden_util import reversible_eigen
from gpu_util import engine_from_problem, random_problem
from oracle import phyoracle as po
from physher_amd.engine import GRAD_FOLD_ROOT_FREQS, RESCALE_ALWAYS, RESCALE_NEVER, EngineError

pytestmark = pytest.mark.gpu
EINVAL, EUNSUPPORTED = -1, -4


def _check(got, ref, what, rel=1e-9):
    (lnl, g, H), (lr, gr, Hr) = got, ref
    dg, dH = np.abs(g - gr).max() / max(1.0, np.abs(gr).max()), np.abs(H - Hr).max() / max(1.0, np.abs(Hr).max())
    print(f"{what}: lnL {abs(lnl - lr) / abs(lr):.2e}, g {dg:.2e}, H {dH:.2e}")
    assert abs(lnl - lr) <= 1e-10 * abs(lr), (lnl, lr)
    assert dg <= rel, dg
    assert dH <= rel, dH


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same_bits(x, y):
    return x[0] == y[0] and np.array_equal(_bits(x[1]), _bits(y[1])) and np.array_equal(_bits(x[2]), _bits(y[2]))


_big_cache = []


def _big():
    """T = 40, P = 700, C = 4: the problem, restatement (b) of it (the brute force is too slow here) and one engine's result"""
    if not _big_cache:
        pb = random_problem(40, 700, 4, seed=71, gaps=0.05)
        with engine_from_problem(pb) as e:
            got = e.branch_hessian()
            diag = e.branch_hessian_diagonal()
            again = e.branch_hessian()
            prof = e.hessian_profile()
        _big_cache.append((pb, message_form(pb), got, diag, again, prof))
    return _big_cache[0]


@pytest.mark.parametrize("T,shape", [(9, "random"), (13, "caterpillar")])
@pytest.mark.parametrize("C,pinv", [(1, None), (2, None), (4, None), (5, None), (8, None), (4, 0.25)])
def test_matches_brute_force(T, shape, C, pinv):
    """node counts 17 and 25: the pair tiles have edges; P = 150: the last block of 64 masks lanes; every kind of pair -- two
    tips of a cherry, node and ancestor at depth >= 3, cousins under an inner node, the root's two children"""
    pb = random_problem(T, 150, C, seed=60 + T + C, shape=shape, gaps=0.05, pinv=pinv)
    ref = brute_force(pb)
    with engine_from_problem(pb) as e:
        got = e.branch_hessian()
        prof = e.hessian_profile()
    _check(got, ref, f"T={T} {shape} C={C} pinv={pinv}")
    _, g, H = got
    assert np.array_equal(_bits(H), _bits(H.T))
    assert not H[pb.root].any() and not H[:, pb.root].any() and g[pb.root] == 0.0
    assert prof["pairs"] == (pb.N - 1) * pb.N // 2 and prof["chunks"] == 1 and prof["scratch_bytes"] > 0


def test_tip_partials_with_ambiguity_codes():
    pb = random_problem(9, 150, 4, seed=77, gaps=0.05)
    rng = np.random.default_rng(1)
    tp = np.zeros((pb.T, pb.P, 4))
    for t in range(pb.T):
        s = pb.tip_states[t]
        for k in range(pb.P):
            if s[k] >= 4:
                tp[t, k] = 1.0
            else:
                tp[t, k, s[k]] = 1.0
                if rng.random() < 0.1:  # a two-state ambiguity code (R, Y, ...)
                    tp[t, k, (s[k] + 1 + rng.integers(3)) % 4] = 1.0
    pb.tip_partials, pb.tip_states = tp, None
    ref = brute_force(pb)
    with engine_from_problem(pb, tip_mode="partials") as e:
        _check(e.branch_hessian(), ref, "ambiguity codes")


def test_forty_taxa_match_the_message_form():
    pb, ref, got, _, _, prof = _big()
    _check(got, ref, "T=40 P=700 C=4")
    assert prof["pairs"] == (pb.N - 1) * pb.N // 2 and prof["chunks"] == 1


def test_diagonal_gradient_symmetry_root_and_repeat():
    pb, _, (lnl, g, H), (l2, d1, d2), again, _ = _big()
    assert lnl == l2
    assert np.abs(np.diag(H) - d2).max() <= 1e-9 * max(1.0, np.abs(d2).max())
    assert np.abs(g - d1).max() <= 1e-9 * max(1.0, np.abs(d1).max())
    assert np.array_equal(_bits(H), _bits(H.T))
    assert not H[pb.root].any() and not H[:, pb.root].any() and g[pb.root] == 0.0
    assert _same_bits((lnl, g, H), again)  # two calls, the second after another call's pre-order pass: identical bits


def test_want_gradient_false():
    pb, _, got, _, _, _ = _big()
    with engine_from_problem(pb) as e:
        lnl, g, H = e.branch_hessian(want_gradient=False)
    assert g is None and lnl == got[0] and np.array_equal(_bits(H), _bits(got[2]))


def test_scratch_history_does_not_change_the_bits():
    """an engine whose batch scratch was first used (and filled) by nni_log_likelihoods returns the bits of a fresh one"""
    pb, _, got, _, _, _ = _big()
    with engine_from_problem(pb) as e:
        e.nni_log_likelihoods()
        assert _same_bits(e.branch_hessian(), got)
        e.nni_log_likelihoods()
        assert _same_bits(e.branch_hessian(), got)


def test_pattern_chunks_under_a_cap():
    """a cap that leaves room for part of the tangents only: the call runs in two or more chunks of whole blocks, stays within the
    cap and matches the uncapped call.  T = 30 caterpillar x 2000 patterns: the tangents (sum of depths = 870 slots, 228 MB) are some
    ten times the engine's own partials, so chunking comes long before the engine tiles its patterns -- a cap that does tile
    them must have the call refused"""
    pb = random_problem(30, 2000, 4, seed=81, shape="caterpillar", gaps=0.03)
    with engine_from_problem(pb) as whole:
        ref = whole.branch_hessian()
        assert whole.hessian_profile()["chunks"] == 1
        base = whole.profile()["device_bytes"]
    for frac in np.arange(0.9, 0.1, -0.05):
        cap = int(frac * base)
        with engine_from_problem(pb, max_device_bytes=cap) as e:
            if e.profile()["tiles"] >= 2:
                with pytest.raises(EngineError) as err:
                    e.branch_hessian()
                assert err.value.code == EUNSUPPORTED
                pytest.fail("the cap tiled the engine's patterns before it chunked the call")
            got = e.branch_hessian()
            chunks = e.hessian_profile()["chunks"]
            assert e.profile()["tiles"] == 1 and e.profile()["device_bytes"] <= cap
            if chunks >= 2:
                print(f"cap {frac:.2f} of {base} bytes: {chunks} chunks")
                _check(got, ref, "chunked")
                assert np.array_equal(_bits(got[2]), _bits(got[2].T))
                assert _same_bits(e.branch_hessian(), got)
                return
    pytest.fail("no cap put the call into chunks")


@pytest.mark.parametrize("shards", [2, 4])
def test_sharded_handles(shards):
    pb, ref, _, _, _, _ = _big()
    have = max(1, torch.cuda.device_count())
    with engine_from_problem(pb, devices=[i % have for i in range(shards)]) as e:
        got = e.branch_hessian()
        assert e.hessian_profile()["pairs"] == (pb.N - 1) * pb.N // 2
    _check(got, ref, f"{shards} shards")
    assert np.array_equal(_bits(got[2]), _bits(got[2].T))


def test_the_engine_is_left_as_a_keep_partials_gradient_leaves_it():
    pb = random_problem(20, 300, 4, seed=34, gaps=0.03)
    dQ = np.random.default_rng(3).normal(size=(2, 4, 4))
    node = int(pb.left[pb.root])

    def run(e):
        return [e.log_likelihood(), *e.gradient(), *e.parameter_gradient(), *e.branch_log_likelihood(node, 0.7 * pb.branch_lengths[node])]

    with engine_from_problem(pb) as a, engine_from_problem(pb) as b:
        a.set_rate_matrix_derivatives(dQ)
        b.set_rate_matrix_derivatives(dQ)
        a.branch_hessian()
        b.set_keep_partials(True)
        b.gradient()
        ra, rb = run(a), run(b)
        a.branch_hessian()
        ra2, rb2 = run(a), run(b)
    for x, y in zip(ra + ra2, rb + rb2):
        assert np.array_equal(_bits(np.asarray(x, dtype=np.float64)), _bits(np.asarray(y, dtype=np.float64)))


def test_folded_uppers():
    """uppers a PHYAMD_GRAD_FOLD_ROOT_FREQS keep-partials gradient left are used as they are.  Uniform frequencies: only there do
    the folded uppers equal pi o u (the reference's include_root_freqs arithmetic carries pi through P, which commutes with a
    constant pi only), so only there is the Hessian formed from them the Hessian"""
    base = random_problem(12, 150, 4, seed=91, gaps=0.05)
    r = np.random.default_rng(5).uniform(0.5, 3.0, size=(4, 4))
    freqs = np.full(4, 0.25)
    ev, U, Ui = reversible_eigen(0.5 * (r + r.T), freqs)
    pb = po.Problem(base.left, base.right, base.root, base.weights, ev, U, Ui, freqs, base.cat_rates, base.cat_props, base.branch_lengths,
                    tip_states=base.tip_states)
    ref = brute_force(pb)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        plain = e.branch_hessian()
        _check(plain, ref, "uniform frequencies")
        e.update_all_nodes()
        e.gradient(flags=GRAD_FOLD_ROOT_FREQS)
        folded = e.branch_hessian()
        _check(folded, ref, "folded uppers")


def test_refusals():
    def refused(e, code, **kw):
        with pytest.raises(EngineError) as err:
            e.branch_hessian(**kw)
        assert err.value.code == code, (err.value.code, str(err.value))
        assert "phyamd_branch_hessian" in str(err.value)

    with engine_from_problem(random_problem(8, 100, 2, seed=36, S=20)) as e:
        refused(e, EUNSUPPORTED)
    with engine_from_problem(random_problem(8, 100, 9, seed=36)) as e:
        refused(e, EUNSUPPORTED)
    pb = random_problem(8, 100, 2, seed=36)
    with engine_from_problem(pb, rescale=RESCALE_ALWAYS) as e:
        refused(e, EUNSUPPORTED)
    with engine_from_problem(pb) as e:
        refused(e, EINVAL, flags=1)
        e.branch_hessian()
        mats = np.stack([np.abs(po.p_t(4, pb.eval, pb.evec, pb.ivec, pb.branch_lengths[3] * r)) for r in pb.cat_rates])
        e.set_node_matrices(3, mats)
        refused(e, EUNSUPPORTED)


def test_underflow_without_rescaling_is_reported_in_band():
    deep = random_problem(900, 64, 4, seed=13, bl=(0.5, 1.5))
    with engine_from_problem(deep, rescale=RESCALE_NEVER) as e:
        lnl, g, H = e.branch_hessian()
    assert np.isinf(lnl) and lnl < 0 and np.all(np.isnan(g)) and np.all(np.isnan(H))
