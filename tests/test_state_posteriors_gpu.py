"""GPU: phyamd_state_posteriors -- the marginal posterior of the state at every node per pattern and its argmax (asr_marginal,
asr.c:28-134) -- and phyamd_site_rate_posteriors (SingleTreeLikelihood_posterior_sites, ppsites.c:17-43) against NumPy
contractions of the CPU oracle's own lower and upper partials (tests/state_posteriors_util.py):
    n != root: J[n][k][j] = sum_c w_c p_n[c,k,j] sum_i pi_i u_n[c,k,i] P_{n,c}[i][j];   root: J[k][j] = sum_c w_c pi_j p_root[c,k,j]
    posterior = J / sum_j J,  state = the smallest j with the largest J;   R[k][c] = w_c pi . p_root[c,k] / sum_c' (the same).
Posteriors: 1e-9 * max(1, |ref|) = 1e-9, the bound tests/test_branch_hessian_gpu.py and tests/test_nni_gpu.py put on d1 / d2, which
are formed from the same two partials, for every state count.  States: equal at every cell whose oracle top-two gap is at least
1e-6; no cell of the cases below is left out (smallest gaps, from the oracle alone, beside each case)."""
import numpy as np
import pytest

from gpu_util import engine_from_problem, random_problem
from physher_amd.engine import GRAD_FOLD_ROOT_FREQS, RESCALE_ALWAYS, RESCALE_NEVER, EngineError
from state_posteriors_util import CASES, GAP, oracle_site_rates, oracle_state_posteriors, tip_vectors
from state_posteriors_util import case as _case

pytestmark = pytest.mark.gpu
EINVAL, EUNSUPPORTED = -1, -4
TOL = 1e-9


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint8)


def _check(got_post, got_states, post, states, gap, what, nodes=None):
    if nodes is not None:
        post, states, gap = post[nodes], states[nodes], gap[nodes]
    err = np.abs(got_post - post).max()
    sure = gap >= GAP
    print(f"{what}: max |posterior - oracle| = {err:.3e}; smallest top-two gap {gap.min():.3e}; cells left out {np.count_nonzero(~sure)}")
    assert err <= TOL * max(1.0, np.abs(post).max()), (what, err)
    assert np.all(sure), (what, "the oracle's gap is below 1e-6 at", np.argwhere(~sure)[:5])
    assert got_states.dtype == np.uint8 and np.array_equal(got_states[sure], states[sure]), (what, np.argwhere(got_states != states)[:5])


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_node_matches_the_oracle(name):
    pb, post, states, gap, policy, tip_mode = _case(name)
    with engine_from_problem(pb, rescale=policy, tip_mode=tip_mode) as e:
        got_post, got_states = e.state_posteriors()
        assert got_post.shape == (pb.N, pb.P, pb.S) and got_states.shape == (pb.N, pb.P)
        assert e.rescaling == (policy == RESCALE_ALWAYS)
        _check(got_post, got_states, post, states, gap, name)
        assert np.abs(got_post.sum(axis=2) - 1.0).max() <= 1e-12
        only_post, none = e.state_posteriors(want_states=False)
        none2, only_states = e.state_posteriors(want_posteriors=False)
        assert none is None and none2 is None
        assert np.array_equal(_bits(only_post), _bits(got_post)) and np.array_equal(only_states, got_states)


@pytest.mark.parametrize("name", ["gaps", "ambiguity_codes", "aa"])
def test_tips_and_the_root(name):
    pb, post, states, gap, policy, tip_mode = _case(name)
    tips = tip_vectors(pb)
    with engine_from_problem(pb, rescale=policy, tip_mode=tip_mode) as e:
        got_post, got_states = e.state_posteriors(nodes=list(range(pb.T)) + [pb.root])
    observed = tips.sum(axis=2) == 1
    assert observed.any() and (~observed).any() or name == "aa"
    # an observed cell: one-hot, exactly, and its code
    assert np.array_equal(got_post[:pb.T][observed], tips[observed])
    assert np.array_equal(got_states[:pb.T][observed], tips[observed].argmax(axis=1))
    # a gap or an ambiguity code: the oracle's posterior (zero outside the code's states)
    _check(got_post[:pb.T], got_states[:pb.T], post, states, gap, name + " tips", nodes=np.arange(pb.T))
    assert np.all(got_post[:pb.T][tips == 0] == 0.0)
    # the root row: pi o p_root
    r = pb.log_likelihood(want_lower=True)
    Jr = np.einsum("c,ckj,j->kj", pb.cat_props, r["lower"][pb.root], pb.freqs)
    assert np.abs(got_post[pb.T] - Jr / Jr.sum(axis=1, keepdims=True)).max() <= TOL


def test_rows_do_not_depend_on_the_list_or_the_chunks():
    pb, post, states, gap, policy, tip_mode = _case("larger_tree")
    rng = np.random.default_rng(3)
    nodes = np.concatenate([rng.permutation(pb.N), [pb.root, 0, 5, 5, pb.N - 1]]).astype(np.int32)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        full_post, full_states = e.state_posteriors()
        held = e.profile()["device_bytes"]
        got_post, got_states = e.state_posteriors(nodes)
        assert np.array_equal(_bits(got_post), _bits(full_post[nodes])) and np.array_equal(got_states, full_states[nodes])
        one_post, one_states = e.state_posteriors([7])
        assert np.array_equal(_bits(one_post[0]), _bits(full_post[7])) and np.array_equal(one_states[0], full_states[7])
    # a cap that leaves room for a few rows of staging beside the engine: the rows run in several chunks
    staging = pb.N * (pb.P * (4 * 8 + 1) + 32)  # per row: [P][4] doubles, [P] bytes, the row's descriptor
    assert held > staging
    cap = held - staging // 2  # what the engine holds without any staging, and room for less than half of the rows
    with engine_from_problem(pb, rescale=RESCALE_NEVER, max_device_bytes=cap) as e:
        e.set_keep_partials(True)
        e.gradient()
        assert e.profile()["tiles"] == 1
        before = e.profile()["device_bytes"]
        assert before + staging > cap, "the cap does not force chunks"
        got_post, got_states = e.state_posteriors()
        assert e.profile()["device_bytes"] <= cap
        assert np.array_equal(_bits(got_post), _bits(full_post)) and np.array_equal(got_states, full_states)
        got_post, got_states = e.state_posteriors(nodes)
        assert np.array_equal(_bits(got_post), _bits(full_post[nodes])) and np.array_equal(got_states, full_states[nodes])
        # one output only, after a call that left the other's staging as large as the room: that staging does not take this call's room
        for kw in (dict(want_posteriors=False), dict(want_states=False), dict(want_posteriors=False), dict()):
            got_post, got_states = e.state_posteriors(**kw)
            assert e.profile()["device_bytes"] <= cap, kw
            assert got_post is None or np.array_equal(_bits(got_post), _bits(full_post)), kw
            assert got_states is None or np.array_equal(got_states, full_states), kw
            if not kw:  # ... nor the site-rate call's, nor that call's the next state call's
                R, mean = e.site_rate_posteriors()
                assert e.profile()["device_bytes"] <= cap and np.abs(R.sum(axis=1) - 1.0).max() <= 1e-12
                assert np.array_equal(e.state_posteriors(want_posteriors=False)[1], full_states)
        e.gradient()
        assert e.profile()["device_bytes"] <= cap


@pytest.mark.parametrize("name", ["larger_tree", "aa", "rescaled"])
def test_the_engine_afterwards_is_a_keep_partials_engine_that_ran_a_gradient(name):
    pb, _, _, _, policy, tip_mode = _case(name)
    with engine_from_problem(pb, rescale=policy, tip_mode=tip_mode) as a, engine_from_problem(pb, rescale=policy, tip_mode=tip_mode) as b:
        first = a.state_posteriors()
        b.set_keep_partials(True)
        b.gradient()
        for step in range(2):
            la, ga = a.gradient()
            lb, gb = b.gradient()
            assert _bits(np.array([la, a.log_likelihood()])).tolist() == _bits(np.array([lb, b.log_likelihood()])).tolist(), (name, step)
            assert np.array_equal(_bits(ga), _bits(gb)), (name, step)
            if step == 0:
                second = a.state_posteriors()
                assert np.array_equal(_bits(first[0]), _bits(second[0])) and np.array_equal(first[1], second[1])
                a.set_branch_length(3, 0.37)
                b.set_branch_length(3, 0.37)
        # a pending change is evaluated by the call
        a.set_branch_lengths(1.3 * pb.branch_lengths)
        b.set_branch_lengths(1.3 * pb.branch_lengths)
        third = a.state_posteriors()
        assert not np.array_equal(_bits(third[0]), _bits(first[0]))
        assert _bits(np.array([a.log_likelihood()])).tolist() == _bits(np.array([b.log_likelihood()])).tolist()


def test_folded_uppers():
    """after a PHYAMD_GRAD_FOLD_ROOT_FREQS keep-partials gradient the resident uppers carry pi (exact for uniform frequencies only:
    the reference's include_root_freqs arithmetic); the call drops pi and matches the oracle's uppers of that arithmetic (smallest top-two gap there: 2.7e-3)"""
    pb = _case("gaps")[0]
    J, _ = oracle_state_posteriors(pb, fold=True)
    post = J / J.sum(axis=2, keepdims=True)
    top = np.sort(post, axis=2)
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        e.set_keep_partials(True)
        e.gradient(flags=GRAD_FOLD_ROOT_FREQS)
        got_post, got_states = e.state_posteriors()
        _check(got_post, got_states, post, post.argmax(axis=2), top[:, :, -1] - top[:, :, -2], "folded uppers")
        assert not np.array_equal(_bits(got_post), _bits(np.ascontiguousarray(_case("gaps")[1])))
        e.update_all_nodes()  # the uppers are dropped: the call runs the flags-0 gradient
        got_post, got_states = e.state_posteriors()
        _check(got_post, got_states, *_case("gaps")[1:4], "after the folded uppers were dropped")


def test_rescaled_and_unscaled_engines_agree():
    pb, post, states, gap, _, _ = _case("larger_tree")
    with engine_from_problem(pb, rescale=RESCALE_ALWAYS) as a, engine_from_problem(pb, rescale=RESCALE_NEVER) as b:
        pa, sa = a.state_posteriors()
        pc, sc = b.state_posteriors()
        assert a.rescaling and not b.rescaling
        assert np.abs(pa - pc).max() <= TOL and np.array_equal(sa, sc)
        _check(pa, sa, post, states, gap, "RESCALE_ALWAYS")
        Ra, ma = a.site_rate_posteriors()
        Rb, mb = b.site_rate_posteriors()
        assert np.abs(Ra - Rb).max() <= TOL and np.abs(ma - mb).max() <= TOL * max(1.0, np.abs(mb).max())


@pytest.mark.parametrize("name", sorted(CASES))
def test_site_rates_match_the_oracle(name):
    pb, _, _, _, policy, tip_mode = _case(name)
    R, mean = oracle_site_rates(pb)
    with engine_from_problem(pb, rescale=policy, tip_mode=tip_mode) as e:
        got_R, got_mean = e.site_rate_posteriors()
        assert got_R.shape == (pb.P, pb.C) and got_mean.shape == (pb.P,)
        err = np.abs(got_R - R).max(), np.abs(got_mean - mean).max()
        print(f"{name}: max |R - oracle| = {err[0]:.3e}, max |mean rate - oracle| = {err[1]:.3e}")
        assert err[0] <= TOL and err[1] <= TOL * max(1.0, np.abs(mean).max())
        assert np.abs(got_R.sum(axis=1) - 1.0).max() <= 1e-12
        if pb.C == 1:
            assert np.all(got_R == 1.0) and np.all(got_mean == pb.cat_rates[0])
        again = e.site_rate_posteriors()
        assert np.array_equal(_bits(again[0]), _bits(got_R)) and np.array_equal(_bits(again[1]), _bits(got_mean))
        e.state_posteriors(nodes=[pb.root])  # (the keep-partials evaluation leaves the same root partial)
        after = e.site_rate_posteriors()
        assert np.abs(after[0] - R).max() <= TOL


@pytest.mark.parametrize("name", ["larger_tree", "aa"])
def test_two_shards_return_the_one_engine_bits(name):
    pb, _, _, _, policy, tip_mode = _case(name)
    with engine_from_problem(pb, rescale=policy, tip_mode=tip_mode) as one, engine_from_problem(pb, rescale=policy, tip_mode=tip_mode, devices=[0, 0]) as two:
        assert two.shard_count == 2
        nodes = np.array([pb.root, 1, pb.N - 1, pb.T, 1], dtype=np.int32)
        for nd in (None, nodes):
            a, b = one.state_posteriors(nd), two.state_posteriors(nd)
            assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[1], b[1])
        a, b = one.site_rate_posteriors(), two.site_rate_posteriors()
        assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))


def _refused(call, code):
    with pytest.raises(EngineError) as err:
        call()
    print(err.value)
    assert err.value.code == code, err.value
    return str(err.value)


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
        assert "tile" in _refused(e.state_posteriors, EUNSUPPORTED)
        assert "tile" in _refused(e.site_rate_posteriors, EUNSUPPORTED)
        ref = pb.log_likelihood()["lnl"]
        assert abs(e.log_likelihood() - ref) <= 1e-10 * abs(ref)


def test_bad_arguments_are_refused():
    import ctypes
    pb = _case("one_category")[0]
    with engine_from_problem(pb) as e:
        lib, h = e._lib, e._h
        post = np.empty((pb.N, pb.P, pb.S))
        states = np.empty((pb.N, pb.P), dtype=np.uint8)
        pp, sp = post.ctypes.data_as(ctypes.c_void_p), states.ctypes.data_as(ctypes.c_void_p)
        assert lib.phyamd_state_posteriors(h, 1, pb.N, None, pp, sp) == EINVAL and b"flags" in lib.phyamd_last_error()
        assert lib.phyamd_state_posteriors(h, 0, pb.N, None, None, None) == EINVAL and b"both null" in lib.phyamd_last_error()
        assert lib.phyamd_state_posteriors(h, 0, 0, None, pp, sp) == EINVAL and b"count" in lib.phyamd_last_error()
        assert "count" in _refused(lambda: e._check(lib.phyamd_state_posteriors(h, 0, pb.N - 1, None, pp, sp)), EINVAL)
        msg = _refused(lambda: e.state_posteriors([3, 4, pb.N, 5]), EINVAL)
        assert "nodes[2]" in msg and str(pb.N) in msg
        assert "nodes[0]" in _refused(lambda: e.state_posteriors([-1]), EINVAL)
        with pytest.raises(ValueError):
            e.state_posteriors(want_posteriors=False, want_states=False)
        assert lib.phyamd_site_rate_posteriors(h, None, None) == EINVAL
        ref = pb.log_likelihood()["lnl"]
        assert abs(e.log_likelihood() - ref) <= 1e-10 * abs(ref)  # still usable
    with pytest.raises(EngineError) as err:  # not ready: as check_ready reports
        from physher_amd.engine import Engine
        with Engine(pb.T, pb.P, pb.S, pb.C) as e:
            e.state_posteriors()
    assert err.value.code == EINVAL


def test_a_likelihood_that_is_not_finite_is_reported_in_band():
    """a deep caterpillar without rescaling underflows: lnL = -inf, every posterior NaN, every state 255"""
    pb = random_problem(700, 70, 2, seed=8, shape="caterpillar", bl=(0.5, 1.5))
    with engine_from_problem(pb, rescale=RESCALE_NEVER) as e:
        post, states = e.state_posteriors(nodes=[0, pb.root, pb.T + 3])
        assert not np.isfinite(e.log_likelihood())
        assert np.all(np.isnan(post)) and np.all(states == 255)


@pytest.mark.parametrize("name", ["larger_tree", "aa"])
def test_site_rates_leave_the_engine_as_it_was(name):
    """an engine that is not rescaling: lnL and gradients after the call are bit for bit those of an engine that never made it"""
    pb, _, _, _, policy, tip_mode = _case(name)
    with engine_from_problem(pb, rescale=policy, tip_mode=tip_mode) as a, engine_from_problem(pb, rescale=policy, tip_mode=tip_mode) as b:
        a.site_rate_posteriors()
        for step in range(2):
            la, ga = a.gradient()
            lb, gb = b.gradient()
            assert _bits(np.array([la, a.log_likelihood()])).tolist() == _bits(np.array([lb, b.log_likelihood()])).tolist(), (name, step)
            assert np.array_equal(_bits(ga), _bits(gb)), (name, step)
            a.site_rate_posteriors()
            a.set_branch_length(3, 0.37)
            b.set_branch_length(3, 0.37)
