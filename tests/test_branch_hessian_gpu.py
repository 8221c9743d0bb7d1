"""GPU: phyamd_branch_hessian_diagonal -- lnL, every branch's d lnL/dt and d2 lnL/dt2 from one post-order and one pre-order pass
(the level kernel's HESS form) -- against the NumPy restatement (tests/hessian_util.py, pinned on the CPU against differences of
the oracle's lnL and the reference's own values), against the single-branch evaluation row by row, and across pattern tiles,
shards, the device-resident form and later evaluations."""
import json
import os

import numpy as np
import pytest
import torch

from golden_util import GOLDEN, load, oracle_problem, read_spec
from gpu_util import engine_from_problem, random_problem
from hessian_util import branch_hessian_diagonal
from physher_amd.engine import RESCALE_ALWAYS, RESCALE_AUTO, RESCALE_NEVER, EngineError

pytestmark = pytest.mark.gpu
EINVAL, EUNSUPPORTED = -1, -4


def _check(lnl, d1, d2, ref, rel=1e-9):
    lr, r1, r2 = ref
    assert abs(lnl - lr) <= 1e-10 * abs(lr), (lnl, lr)
    assert np.abs(d1 - r1).max() <= rel * max(1.0, np.abs(r1).max()), np.abs(d1 - r1).max()
    assert np.abs(d2 - r2).max() <= rel * max(1.0, np.abs(r2).max()), np.abs(d2 - r2).max()


def _deep(T, P, C, seed, **kw):
    """a caterpillar deep enough (T >= 700) that the partials underflow without rescaling"""
    return random_problem(T, P, C, seed=seed, shape="caterpillar", bl=(0.5, 1.5), rescale=1, **kw)


@pytest.mark.parametrize("shape", ["random", "caterpillar"])
@pytest.mark.parametrize("C,pinv", [(1, None), (2, None), (4, None), (5, None), (4, 0.25)])
@pytest.mark.parametrize("rescale", [RESCALE_NEVER, RESCALE_ALWAYS])
def test_matches_restatement(shape, C, pinv, rescale):
    pb = random_problem(37, 700, C, seed=40 + C, shape=shape, gaps=0.05, pinv=pinv, rescale=1 if rescale == RESCALE_ALWAYS else 0)
    ref = branch_hessian_diagonal(pb)
    with engine_from_problem(pb, rescale=rescale) as e:
        lnl, d1, d2 = e.branch_hessian_diagonal()
        _check(lnl, d1, d2, ref)
        assert d1[pb.root] == 0.0 and d2[pb.root] == 0.0


@pytest.mark.parametrize("S", [20, 61])
@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("rescale", [RESCALE_NEVER, RESCALE_ALWAYS])
def test_generic_states_match_restatement(S, C, rescale):
    """20 / 61 states: the HESS form of k_upper_gen (20 states: unfused for the call) against the restatement, and rows equal to
    the single-branch evaluation"""
    T = 12 if S == 20 else 8
    pb = random_problem(T, 300, C, seed=50 + S + C, S=S, gaps=0.03, rescale=1 if rescale == RESCALE_ALWAYS else 0)
    ref = branch_hessian_diagonal(pb)
    with engine_from_problem(pb, rescale=rescale) as e:
        lnl, d1, d2 = e.branch_hessian_diagonal()
        _check(lnl, d1, d2, ref)
        for n in range(pb.N):
            if n == pb.root:
                continue
            _, b1, b2 = e.branch_log_likelihood(n, pb.branch_lengths[n])
            assert abs(d1[n] - b1) <= 1e-9 * max(1.0, abs(b1)) and abs(d2[n] - b2) <= 1e-9 * max(1.0, abs(b2)), (n, d1[n], b1, d2[n], b2)


@pytest.mark.parametrize("C", [2, 4])
def test_tip_partials_with_ambiguity_codes(C):
    pb = random_problem(24, 500, C, seed=77, gaps=0.05)
    rng = np.random.default_rng(1)
    tp = np.zeros((pb.T, pb.P, 4))
    for t in range(pb.T):
        s = pb.tip_states[t]
        for k in range(pb.P):
            if s[k] >= 4:
                tp[t, k] = 1.0
            else:
                tp[t, k, s[k]] = 1.0
                if rng.random() < 0.05:  # a two-state ambiguity code (R, Y, ...)
                    tp[t, k, (s[k] + 1 + rng.integers(3)) % 4] = 1.0
    pb.tip_partials, pb.tip_states = tp, None
    ref = branch_hessian_diagonal(pb)
    with engine_from_problem(pb, tip_mode="partials") as e:
        _check(*e.branch_hessian_diagonal(), ref)


@pytest.mark.parametrize("case", ["gtr_g4_t16", "gtr_g4_t24_gaps_tipstates", "wag_g4_t12", "mg94_t8"])
def test_matches_reference_fixture(case):
    gold = load(case)
    spec = read_spec(case)
    pb = oracle_problem(case, gold)
    with open(os.path.join(GOLDEN, case, "branch_trials.json")) as f:
        trials = [t for t in json.load(f)["trials"] if t["length"] == pb.branch_lengths[t["node"]]]
    assert len(trials) == 4
    with engine_from_problem(pb, tip_mode="states" if spec["tipstates"] == "1" else "partials") as e:
        lnl, d1, d2 = e.branch_hessian_diagonal()
    for tr in trials:
        n = tr["node"]
        assert abs(lnl - tr["lnl"]) <= 1e-10 * abs(tr["lnl"]), tr
        assert abs(d1[n] - tr["d1"]) <= 1e-8 * max(1.0, abs(tr["d1"])), (tr, d1[n])
        assert abs(d2[n] - tr["d2"]) <= 1e-7 * max(1.0, abs(tr["d2"])), (tr, d2[n])


@pytest.mark.parametrize("C,rescale,deep", [(4, RESCALE_NEVER, False), (5, RESCALE_ALWAYS, True), (4, RESCALE_AUTO, True), (1, RESCALE_AUTO, False)])
def test_rows_equal_single_branch_evaluation(C, rescale, deep):
    pb = _deep(800, 100, C, seed=5) if deep else random_problem(40, 400, C, seed=6, gaps=0.03)
    with engine_from_problem(pb, rescale=rescale) as e:
        lnl, d1, d2 = e.branch_hessian_diagonal()
        if deep:
            assert e.rescaling
        for n in range(0, pb.N, 1 if pb.N < 100 else 23):  # (deep trees: a path walk per branch, a sample of them)
            if n == pb.root:
                continue
            l, b1, b2 = e.branch_log_likelihood(n, pb.branch_lengths[n])
            assert abs(l - lnl) <= 1e-10 * abs(lnl)
            assert abs(d1[n] - b1) <= 1e-9 * max(1.0, abs(b1)), (n, d1[n], b1)
            assert abs(d2[n] - b2) <= 1e-9 * max(1.0, abs(b2)), (n, d2[n], b2)


def _tiled_cap(pb, rescale):
    with engine_from_problem(pb, rescale=rescale) as whole:
        whole.branch_hessian_diagonal()
        base = whole.profile()["device_bytes"]
    for frac in np.arange(0.9, 0.1, -0.05):
        try:
            with engine_from_problem(pb, rescale=rescale, max_device_bytes=int(frac * base)) as e:
                if e.profile()["tiles"] >= 2:
                    return int(frac * base)
        except EngineError:
            pass
    pytest.fail("no cap puts this problem into tiles")


@pytest.mark.parametrize("C,rescale,deep", [(4, RESCALE_NEVER, False), (2, RESCALE_ALWAYS, True), (4, RESCALE_AUTO, True)])
def test_tiled_equals_untiled_and_single_branch_rows(C, rescale, deep):
    """a cap that forces two or more tiles: the per-tile sums added in tile order equal the untiled call; on deep trees the
    categories' exponents differ between tiles"""
    pb = _deep(800, 2000, C, seed=21) if deep else random_problem(40, 2000, C, seed=22, gaps=0.03)
    cap = _tiled_cap(pb, rescale)
    with engine_from_problem(pb, rescale=rescale) as one, engine_from_problem(pb, rescale=rescale, max_device_bytes=cap) as tiled:
        assert tiled.profile()["tiles"] >= 2
        ref = one.branch_hessian_diagonal()
        got = tiled.branch_hessian_diagonal()
        assert one.rescaling == deep and tiled.rescaling == deep
        assert tiled.profile()["device_bytes"] <= cap
        _check(*got, ref)
        for n in range(0, pb.N, 7 if pb.N < 100 else 41):
            if n == pb.root:
                continue
            _, b1, b2 = one.branch_log_likelihood(n, pb.branch_lengths[n])
            assert abs(got[1][n] - b1) <= 1e-9 * max(1.0, abs(b1)) and abs(got[2][n] - b2) <= 1e-9 * max(1.0, abs(b2))


@pytest.mark.parametrize("S,rescale", [(4, RESCALE_NEVER), (4, RESCALE_ALWAYS), (20, RESCALE_NEVER), (61, RESCALE_ALWAYS)])
def test_shard_count_does_not_change_the_bits(S, rescale):
    pb = random_problem(30 if S == 4 else 8, 5000 if S == 4 else 1500, 4 if S == 4 else 2, seed=31, S=S, gaps=0.03,
                        bl=(0.3, 0.9) if rescale == RESCALE_ALWAYS else (0.01, 0.1))
    have = max(1, torch.cuda.device_count())
    out = []
    for n in (1, 2, 4):
        kw = {"devices": [i % have for i in range(n)]} if n > 1 else {}
        with engine_from_problem(pb, rescale=rescale, **kw) as e:
            out.append(e.branch_hessian_diagonal())
    for lnl, d1, d2 in out[1:]:
        assert lnl == out[0][0]
        assert np.array_equal(d1, out[0][1]) and np.array_equal(d2, out[0][2])


def test_device_form_equals_host_form():
    pb = random_problem(30, 900, 4, seed=32, gaps=0.03)
    with engine_from_problem(pb, device=0) as e:
        lnl, d1, d2 = e.branch_hessian_diagonal()
        buf = torch.full((1 + 2 * pb.N,), -1.0, dtype=torch.float64, device="cuda:0")
        e.branch_hessian_diagonal_device(buf.data_ptr())
        e.synchronize()
        v = buf.cpu().numpy()
    assert v[0] == lnl and np.array_equal(v[1:1 + pb.N], d1) and np.array_equal(v[1 + pb.N:], d2)


@pytest.mark.parametrize("S,rescale,deep", [(4, RESCALE_NEVER, False), (4, RESCALE_AUTO, False), (4, RESCALE_AUTO, True), (4, RESCALE_ALWAYS, True),
                                             (20, RESCALE_AUTO, False), (61, RESCALE_NEVER, False)])
def test_no_sticky_state(S, rescale, deep):
    """after the call lnL, the gradient and the parameter gradient are bit for bit those of an engine that never made it, and the
    single-branch evaluation gives the same values"""
    pb = _deep(800, 300, 4, seed=33) if deep else random_problem(40 if S == 4 else 10, 800 if S == 4 else 200, 4 if S == 4 else 2, seed=34, S=S, gaps=0.03)
    dQ = np.random.default_rng(3).normal(size=(2, S, S))
    node = int(pb.left[pb.root])

    def run(e):
        return [e.log_likelihood(), *e.gradient(), *e.parameter_gradient(), *e.branch_log_likelihood(node, 0.7 * pb.branch_lengths[node])]

    with engine_from_problem(pb, rescale=rescale) as a, engine_from_problem(pb, rescale=rescale) as b:
        a.set_rate_matrix_derivatives(dQ)
        b.set_rate_matrix_derivatives(dQ)
        a.branch_hessian_diagonal()
        ra, rb = run(a), run(b)
        a.branch_hessian_diagonal()
        ra2, rb2 = run(a), run(b)
    for x, y in zip(ra + ra2, rb + rb2):
        assert np.array_equal(np.asarray(x), np.asarray(y))


@pytest.mark.parametrize("S,C,rescale", [(4, 4, RESCALE_NEVER), (4, 2, RESCALE_ALWAYS), (20, 2, RESCALE_NEVER)])
def test_no_sticky_state_tiled(S, C, rescale):
    """the same on engines that process their patterns in tiles (run_tiled, mode 3)"""
    pb = random_problem(30 if S == 4 else 10, 3000 if S == 4 else 1500, C, seed=37, S=S, gaps=0.03, bl=(0.3, 0.9) if rescale == RESCALE_ALWAYS else (0.01, 0.1))
    cap = _tiled_cap(pb, rescale)

    def run(e):
        return [e.log_likelihood(), *e.gradient(), e.root_invariant_term()]

    with engine_from_problem(pb, rescale=rescale, max_device_bytes=cap) as a, engine_from_problem(pb, rescale=rescale, max_device_bytes=cap) as b:
        assert a.profile()["tiles"] >= 2
        a.branch_hessian_diagonal()
        ra, rb = run(a), run(b)
        a.branch_hessian_diagonal()
        ra2, rb2 = run(a), run(b)
    for x, y in zip(ra + ra2, rb + rb2):
        assert np.array_equal(np.asarray(x), np.asarray(y))


def test_refusals_and_nan():
    pb = random_problem(20, 300, 2, seed=35)
    with engine_from_problem(pb) as e:
        for flags in (1, 2, 4):
            with pytest.raises(EngineError) as err:
                e.branch_hessian_diagonal(flags=flags)
            assert err.value.code == EINVAL
    pb9 = random_problem(8, 100, 9, seed=36)
    with engine_from_problem(pb9) as e:  # 4 states: one workgroup holds every category's exchange, at most 8
        with pytest.raises(EngineError) as err:
            e.branch_hessian_diagonal()
        assert err.value.code == EUNSUPPORTED
    deep = random_problem(900, 64, 4, seed=13, bl=(0.5, 1.5))
    with engine_from_problem(deep, rescale=RESCALE_NEVER) as e:  # lnL underflows to -inf: every derivative NaN
        lnl, d1, d2 = e.branch_hessian_diagonal()
        assert np.isinf(lnl) and lnl < 0 and np.all(np.isnan(d1)) and np.all(np.isnan(d2))
