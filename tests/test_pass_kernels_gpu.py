"""Every row of the rule that chooses the kernel of a 4-state pass (lower_kernel / upper_kernel, phyamd_shard.inc), reached the way
a caller reaches it.  Each case runs the call sequence, asserts the WHOLE profile phyamd_get_pass_profile reports for the pass
under test -- the expected values are written down in pass_kernel_util.py from the text of the rule and the launchers -- and then
compares with the oracle at the suite's bounds: lnL 1e-10 relative, the per-category gradient 1e-9 * max(1, max |ref|), per-pattern
lnL rtol = atol = 1e-11, and a second identical call returns the same bits.

Three rows are not what a first reading of the rule suggests; the code decides, and the rows assert what it says:
  * ambiguity codes keep the pre-order walk off the pair ops' descriptor set (launch_upper_stream: pairs = ... && !amb);
  * under rescaling a first call with PHYAMD_GRAD_FOLD_ROOT_FREQS asks for the reference's form before its post-order pass
    (run_gradient), so the power-of-two form never meets the FOLD flag: that call is a row of the reference's rescaling;
  * a changed branch after a pass that left Carried / CarriedExp2 lowers recomputes every node in the reference's form (run_lower);
    the incremental level pass is the one after the NEXT changed branch.
"""
import numpy as np
import pytest

import pass_kernel_util as k
from gpu_util import engine_from_problem
from oracle import phyoracle as po
from physher_amd import _lib
from physher_amd.engine import GRAD_COMPAT_SCALED, GRAD_FOLD_ROOT_FREQS, RESCALE_ALWAYS, RESCALE_AUTO, RESCALE_NEVER, EngineError

pytestmark = pytest.mark.gpu

P_UNSCALED = 321
SHAPES = ("caterpillar", "random")


def _rescaled_cases(ambiguous_at):
    """(C, tips, shape): every C on both trees with tip states; ambiguous tips on the random tree at the given C"""
    return [(C, "states", shape) for shape in SHAPES for C in k.CATS_ALL] + [(C, "ambiguous", "random") for C in ambiguous_at]


def _engine(pb, rescale, **kw):
    return engine_from_problem(pb, rescale=rescale, tip_mode="states" if pb.tip_partials is None else "partials", **kw)


def _tips(pb, tips):
    return pb if tips == "states" else k.ambiguous(pb)


def _expect(e, want):
    got = e.pass_profile()
    assert got == want, {key: (got[key], want[key]) for key in want if got[key] != want[key]}


def test_the_profile_before_any_pass_and_its_refusals():
    pb = k.unscaled_problem(63, 2)
    with _engine(pb, RESCALE_NEVER) as e:
        _expect(e, k.profile(k.NO_LOWER, k.NO_UPPER))
        lnl = e.log_likelihood()
        _expect(e, k.profile(k.lower_stream(k.CARRIED, False), k.NO_UPPER))
        k.check_lnl(e, lnl, k.oracle(pb))
        assert e._lib.phyamd_get_pass_profile(e._h, None) == _lib.EINVAL
        msg = e._lib.phyamd_last_error()
        assert b"phyamd_get_pass_profile" in msg and b"null out" in msg, msg
    from gpu_util import random_problem
    aa = random_problem(5, 20, 1, seed=3, S=20)
    with engine_from_problem(aa, rescale=RESCALE_NEVER) as e:
        e.log_likelihood()
        with pytest.raises(EngineError) as err:
            e.pass_profile()
        assert err.value.code == _lib.EUNSUPPORTED and "phyamd_get_pass_profile" in str(err.value) and "20 states" in str(err.value)


def test_a_tiled_engine_and_a_sharded_handle_report_a_profile():
    """the last tile's, the first shard's: both run the default row"""
    pb = k.unscaled_problem(2000, 2)
    ref = k.oracle(pb)
    with _engine(pb, RESCALE_NEVER) as e:
        e.gradient()
        held = e.profile()["device_bytes"]
    with _engine(pb, RESCALE_NEVER, max_device_bytes=int(0.45 * held)) as e:
        lnl, cg = e.gradient()
        assert e.profile()["tiles"] >= 2
        p = e.pass_profile()
        assert (p["lower_family"], p["lower_form"], p["upper_family"], p["upper_tf"]) == (k.STREAM, k.CARRIED, k.STREAM, 1), p
        assert abs(lnl - ref["lnl"]) <= 1e-10 * abs(ref["lnl"]) and np.abs(cg - ref["cat_grad"]).max() <= 1e-9 * max(1.0, np.abs(ref["cat_grad"]).max())
    with _engine(pb, RESCALE_NEVER, devices=[0, 0]) as e:
        lnl, cg = e.gradient()
        _expect(e, k.profile(k.lower_stream(k.CARRIED, False), k.upper_stream(k.CARRIED, False, pair_ops=k.pair_ops())))
        assert abs(lnl - ref["lnl"]) <= 1e-10 * abs(ref["lnl"]) and np.abs(cg - ref["cat_grad"]).max() <= 1e-9 * max(1.0, np.abs(ref["cat_grad"]).max())


# ---- the unscaled streamed walks ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P,C", [(P_UNSCALED, C) for C in k.CATS_ALL] + [(63, 4)])
def test_s_plain(P, C):
    """S-plain, the default row: Stream / Carried, the pre-order walk on the descriptor set with the pair ops"""
    pb = k.unscaled_problem(P, C)
    assert k.pair_ops() > 0
    with _engine(pb, RESCALE_NEVER) as e:
        want = k.profile(k.lower_stream(k.CARRIED, False), k.upper_stream(k.CARRIED, False, pair_ops=k.pair_ops()))
        lnl, _ = k.check_gradient(e, 0, k.oracle(pb), want)
        assert want["upper_pair_ops"] > 0 and e.pass_profile() == want
        assert k.same_bits(e.log_likelihood(), lnl)


@pytest.mark.parametrize("C", [1, 4, 8])
def test_s_ambig(C):
    """S-ambig: masks of two and three states -> the AMBIG instantiations of both walks, which read no pair ops"""
    pb = k.ambiguous(k.unscaled_problem(P_UNSCALED, C))
    with _engine(pb, RESCALE_NEVER) as e:
        want = k.profile(k.lower_stream(k.CARRIED, False, ambiguous=1), k.upper_stream(k.CARRIED, False, ambiguous=1))
        k.check_gradient(e, 0, k.oracle(pb), want)


@pytest.mark.parametrize("C", [1, 4, 8])
def test_s_fold(C):
    """S-fold: S-plain, then the FOLD flag on the same stored lowers (no post-order pass in between)"""
    pb = k.unscaled_problem(P_UNSCALED, C)
    with _engine(pb, RESCALE_NEVER) as e:
        lower = k.lower_stream(k.CARRIED, False)
        k.check_gradient(e, 0, k.oracle(pb), k.profile(lower, k.upper_stream(k.CARRIED, False, pair_ops=k.pair_ops())))
        k.check_gradient(e, GRAD_FOLD_ROOT_FREQS, k.oracle(pb, fold=1), k.profile(lower, k.upper_stream(k.CARRIED, False, fold=1, pair_ops=k.pair_ops())))


@pytest.mark.parametrize("tips", ["states", "ambiguous"])
@pytest.mark.parametrize("C", [1, 4, 8])
def test_s_ref(C, tips):
    """S-ref: a reader of stored partials turns the reference's form on for good: the plain, non-TF streamed walks"""
    pb = _tips(k.unscaled_problem(P_UNSCALED, C), tips)
    amb = int(tips == "ambiguous")
    with _engine(pb, RESCALE_NEVER) as e:
        e.gradient()
        _expect(e, k.profile(k.lower_stream(k.CARRIED, False, amb), k.upper_stream(k.CARRIED, False, amb, pair_ops=0 if amb else k.pair_ops())))
        e.partials(pb.root)  # (the root is stored in every schedule)
        moved = k.clone(pb, branch_lengths=k.new_lengths(pb))
        e.set_branch_lengths(moved.branch_lengths)
        want = k.profile(k.lower_stream(k.REFERENCE, False, amb), k.upper_stream(k.REFERENCE, False, amb))
        k.check_gradient(e, 0, k.oracle(moved), want)


# ---- rescaled problems ---------------------------------------------------------------------------------------------------------

def _rescaled(shape, C, tips="states"):
    pb = k.rescaled_problem(shape, C)
    assert k.rescales(pb), "the oracle never rescales this problem"
    return _tips(pb, tips)


@pytest.mark.parametrize("C,tips,shape", _rescaled_cases((1, 4, 8)))
def test_s_exp2(C, tips, shape):
    """S-exp2: a fresh rescaling engine's gradient() runs both streamed walks on powers of two per category, whatever C"""
    pb = _rescaled(shape, C, tips)
    amb = int(tips == "ambiguous")
    with _engine(pb, RESCALE_ALWAYS) as e:
        k.check_gradient(e, 0, k.oracle(pb), k.profile(k.lower_stream(k.EXP2, True, amb), k.upper_stream(k.EXP2, True, amb)))


def _reference_rescaling(C, amb=0, fold=0):
    """the reference's rescaling form on both passes: the streamed walks while the C category waves fit one workgroup
    (stream_shape_fits: C <= STREAM_WAVES), else the table-gather walks at one pattern per thread"""
    if C <= k.STREAM_WAVES:
        return k.profile(k.lower_stream(k.REFERENCE, True, amb), k.upper_stream(k.REFERENCE, True, amb, fold=fold))
    return k.profile(k.lower_walk(C, True, ppt=1), k.upper_walk(C, True, fold=fold))


@pytest.mark.parametrize("C,tips,shape", _rescaled_cases((2, 4, 9)))
def test_s_scale1_and_w_scale_after_a_reader(C, tips, shape):
    """S-scale1 (C <= 4) and W-scale (C > 4, waves 8 / 8 / 16 / 16), first route: a single-branch evaluation first, then new
    lengths and gradient()"""
    pb = _rescaled(shape, C, tips)
    amb = int(tips == "ambiguous")
    ref = k.oracle(pb)
    with _engine(pb, RESCALE_ALWAYS) as e:
        node = pb.T + 1 if pb.T + 1 != pb.root else pb.T
        lt, _, _ = e.branch_log_likelihood(node, pb.branch_lengths[node])
        assert abs(lt - ref["lnl"]) <= 1e-10 * abs(ref["lnl"])
        got = e.pass_profile()
        want = _reference_rescaling(C, amb)
        assert k.lower_part(got) == k.lower_part(want), got
        moved = k.clone(pb, branch_lengths=k.new_lengths(pb))
        e.set_branch_lengths(moved.branch_lengths)
        k.check_gradient(e, 0, k.oracle(moved), want)


@pytest.mark.parametrize("C,tips,shape", _rescaled_cases((2, 4, 9)))
def test_s_scale1_and_w_scale_from_a_first_fold_call(C, tips, shape):
    """second route (also the FOLD half of S-exp2): a fresh rescaling engine whose first call carries the FOLD flag"""
    pb = _rescaled(shape, C, tips)
    amb = int(tips == "ambiguous")
    with _engine(pb, RESCALE_ALWAYS) as e:
        k.check_gradient(e, GRAD_FOLD_ROOT_FREQS, k.oracle(pb, fold=1), _reference_rescaling(C, amb, fold=1))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("C", [2, 4, 5, 16])
def test_w_compat(C, shape):
    """W-compat: the reference's per-category arithmetic under rescaling is the table-gather pre-order walk's"""
    pb = _rescaled(shape, C)
    with _engine(pb, RESCALE_ALWAYS) as e:
        want = k.profile(_reference_rescaling(C), k.upper_walk(C, True, compat=1))
        k.check_gradient(e, GRAD_COMPAT_SCALED, k.oracle(pb, compat=1), want)


# ---- the table-gather walks as fallbacks ------------------------------------------------------------------------------------

EMPTY_TIP, EMPTY_PATTERN = 3, 40


@pytest.mark.parametrize("C", [1, 4, 5])
@pytest.mark.parametrize("policy", [RESCALE_NEVER, RESCALE_ALWAYS, RESCALE_AUTO])
def test_w_empty(policy, C):
    """W-empty: one tip cell with an empty state mask.  Known only once the mask words are built, it sends both passes to the
    table-gather walks: unscaled at two patterns per thread (321 patterns are at most six workgroups, far fewer than the card
    holds at once: launch_lower_walk, g <= slots1), rescaled at one.  RESCALE_AUTO: lnL = -inf switches rescaling on, the evaluation
    runs again.

    The pattern's site likelihood is 0 under every policy: the pattern is -inf and lnL is -inf.  The reference's rescaling divides the
    node's all-zero partials by their maximum 0 and leaves NaN for both (SingleTreeLikelihood_scalePartials,
    treelikelihood.c:1790-1836), as the oracle does; k_lower4_walk and k_lower4 do not rescale by a zero maximum."""
    full = k.one_hot(k.unscaled_problem(P_UNSCALED, C))
    tp = full.tip_partials.copy()
    tp[EMPTY_TIP, EMPTY_PATTERN] = 0.0
    scaling = policy != RESCALE_NEVER
    pb = k.clone(full, tip_partials=tp, rescale={RESCALE_NEVER: 0, RESCALE_ALWAYS: 1, RESCALE_AUTO: 2}[policy])
    ref = k.oracle(pb)
    others = np.arange(pb.P) != EMPTY_PATTERN
    with _engine(pb, policy) as e:
        lnl, cg = e.gradient()
        assert e.rescaling == scaling == ref["rescaled"]
        _expect(e, k.profile(k.lower_walk(C, scaling, ppt=1 if scaling else 2), k.upper_walk(C, scaling)))
        plk = e.pattern_log_likelihoods()
        print("lnL", lnl, "oracle", ref["lnl"], "; the pattern:", plk[EMPTY_PATTERN], "oracle", ref["pattern_lk"][EMPTY_PATTERN])
        np.testing.assert_allclose(plk[others], ref["pattern_lk"][others], rtol=1e-11, atol=1e-11)
        assert not np.isfinite(ref["pattern_lk"][EMPTY_PATTERN]) and not np.isfinite(ref["lnl"])
        assert plk[EMPTY_PATTERN] == -np.inf and lnl == -np.inf
        finite = np.isfinite(ref["cat_grad"])
        finite[pb.root] = False  # (the root's row: zeros here, whatever the oracle leaves there)
        rest = np.ones_like(finite)
        rest[pb.root] = False
        assert np.array_equal(np.isfinite(cg)[rest], finite[rest])
        if finite.any():
            assert np.abs(cg[finite] - ref["cat_grad"][finite]).max() <= 1e-9 * max(1.0, np.abs(ref["cat_grad"][finite]).max())
        lnl2, cg2 = e.gradient()
        assert k.same_bits(lnl, lnl2) and k.same_bits(cg, cg2)
        # the tip set back: the mask words are rebuilt, the streamed walks again
        e.set_tip_partials(EMPTY_TIP, full.tip_partials[EMPTY_TIP])
        back = k.clone(full, rescale=int(scaling))
        if scaling:
            want = k.profile(k.lower_stream(k.EXP2, True), k.upper_stream(k.EXP2, True))
        else:
            want = k.profile(k.lower_stream(k.CARRIED, False), k.upper_stream(k.CARRIED, False, pair_ops=k.pair_ops()))
        k.check_gradient(e, 0, k.oracle(back), want)


@pytest.mark.parametrize("C", [4, 5])
@pytest.mark.parametrize("policy", [RESCALE_NEVER, RESCALE_ALWAYS])
def test_an_empty_tip_mask_in_the_level_kernels(policy, C):
    """the same tip cell with resident partials (L-keep): k_lower4's rescaling leaves a zero maximum alone as well"""
    full = k.one_hot(k.unscaled_problem(P_UNSCALED, C))
    tp = full.tip_partials.copy()
    tp[EMPTY_TIP, EMPTY_PATTERN] = 0.0
    scaling = policy == RESCALE_ALWAYS
    pb = k.clone(full, tip_partials=tp, rescale=int(scaling))
    ref = k.oracle(pb)
    others = np.arange(pb.P) != EMPTY_PATTERN
    with _engine(pb, policy) as e:
        e.set_keep_partials(True)
        lnl, cg = e.gradient()
        _expect(e, k.profile(k.lower_levels(C, scaling), k.upper_levels(C, scaling)))
        plk = e.pattern_log_likelihoods()
        print("lnL", lnl, "oracle", ref["lnl"], "; the pattern:", plk[EMPTY_PATTERN], "oracle", ref["pattern_lk"][EMPTY_PATTERN])
        np.testing.assert_allclose(plk[others], ref["pattern_lk"][others], rtol=1e-11, atol=1e-11)
        assert plk[EMPTY_PATTERN] == -np.inf and lnl == -np.inf
        rest = np.arange(pb.N) != pb.root
        assert not np.isfinite(ref["cat_grad"][rest]).any() and not np.isfinite(cg[rest]).any()
        assert k.same_bits(lnl, e.log_likelihood())


def _parameter_gradient(e, pb, dQ, flags, want, skip=()):
    _, og = po.parameter_gradient(pb, dQ, skip_nodes=skip)
    ref = k.oracle(pb, compat=int(bool(flags & GRAD_COMPAT_SCALED)))
    lnl, cg, pg = e.parameter_gradient(flags)
    _expect(e, want)
    k.check_lnl(e, lnl, ref)
    print("parameter gradient off by", np.abs(pg - og).max(), "of", 1e-9 * max(1.0, np.abs(og).max()))
    assert np.abs(pg - og).max() <= 1e-9 * max(1.0, np.abs(og).max())
    assert np.abs(cg - ref["cat_grad"]).max() <= 1e-9 * max(1.0, np.abs(ref["cat_grad"]).max())
    lnl2, cg2, pg2 = e.parameter_gradient(flags)
    assert k.same_bits(lnl, lnl2) and k.same_bits(cg, cg2) and k.same_bits(pg, pg2)


def _params_problem(rescale, C):
    return _rescaled("random", C) if rescale == RESCALE_ALWAYS else k.unscaled_problem(P_UNSCALED, C)


def _params_lower(rescale, C):
    """the parameter gradient reads the stored lowers in the reference's form (run_gradient: require_reference_form)"""
    return k.lower_part(_reference_rescaling(C)) if rescale == RESCALE_ALWAYS else k.lower_stream(k.REFERENCE, False)


@pytest.mark.parametrize("rescale", [RESCALE_NEVER, RESCALE_ALWAYS])
@pytest.mark.parametrize("C", [1, 4, 8])
def test_w_params(C, rescale):
    """W-params: the substitution-parameter sums in the table-gather pre-order walk (CATBLK: unscaled with a wave bound of 4)"""
    pb = _params_problem(rescale, C)
    scaling = rescale == RESCALE_ALWAYS
    dQ = k.rate_matrix_derivatives()
    with _engine(pb, rescale) as e:
        e.set_rate_matrix_derivatives(dQ)
        want = k.profile(_params_lower(rescale, C), k.upper_walk(C, scaling, params=1))
        assert want["upper_catblk"] == int(not scaling and C <= 4)
        _parameter_gradient(e, pb, dQ, 0, want)


@pytest.mark.parametrize("rescale,flags", [(RESCALE_NEVER, 0), (RESCALE_ALWAYS, 0), (RESCALE_ALWAYS, GRAD_COMPAT_SCALED)])
@pytest.mark.parametrize("C", [1, 4, 8])
def test_l_params(C, rescale, flags):
    """L-params: explicit matrices on one node (they have no eigen system), or the compat flag under rescaling (the level kernels'
    arithmetic), send the parameter sums to the level kernels.  The explicit matrices are the node's own P(t r_c): the oracle's
    problem is unchanged but for that node's parameter terms, which are zero (k_parameter_matrices)"""
    pb = _params_problem(rescale, C)
    scaling = rescale == RESCALE_ALWAYS
    compat = int(bool(flags & GRAD_COMPAT_SCALED))
    dQ = k.rate_matrix_derivatives()
    node = 2
    with _engine(pb, rescale) as e:
        e.set_rate_matrix_derivatives(dQ)
        skip = ()
        if not compat:
            e.set_node_matrices(node, np.stack([po.p_t(4, pb.eval, pb.evec, pb.ivec, pb.branch_lengths[node] * r) for r in pb.cat_rates]))
            skip = (node,)
        want = k.profile(_params_lower(rescale, C), k.upper_levels(C, scaling, compat=compat, params=1))
        _parameter_gradient(e, pb, dQ, flags, want, skip)


# ---- the level kernels -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rescale,C", [(RESCALE_NEVER, 4), (RESCALE_NEVER, 8), (RESCALE_ALWAYS, 4), (RESCALE_ALWAYS, 5)])
def test_l_incr(rescale, C):
    """L-incr: changed single branches after gradient().  The first one finds Carried / CarriedExp2 lowers, which an incremental
    update cannot read: every node is recomputed in the reference's form (a full pass of the walks).  The second one is the
    incremental pass of the level kernels.  The pre-order half of the profile stays the gradient's"""
    scaling = rescale == RESCALE_ALWAYS
    pb = _rescaled("random", C) if scaling else k.unscaled_problem(P_UNSCALED, C)
    with _engine(pb, rescale) as e:
        e.gradient()
        form = k.EXP2 if scaling else k.CARRIED
        upper = k.upper_stream(form, scaling, pair_ops=0 if scaling else k.pair_ops())
        _expect(e, k.profile(k.lower_stream(form, scaling), upper))
        bl = pb.branch_lengths.copy()
        full = k.lower_part(_reference_rescaling(C)) if scaling else k.lower_stream(k.REFERENCE, False)
        for node, factor, lower in ((pb.T + 2, 1.7, full), (5, 0.6, k.lower_levels(C, scaling, incremental=1))):
            assert node != pb.root
            bl[node] *= factor
            e.set_branch_length(node, bl[node])
            lnl = e.log_likelihood()
            _expect(e, k.profile(lower, upper))
            k.check_lnl(e, lnl, k.clone(pb, branch_lengths=bl).log_likelihood())
            assert k.same_bits(lnl, e.log_likelihood())
        # and the gradient on top of the incrementally updated lowers, which are the reference's
        after = k.upper_part(_reference_rescaling(C)) if scaling else k.upper_stream(k.REFERENCE, False)
        k.check_gradient(e, 0, k.oracle(k.clone(pb, branch_lengths=bl)), k.profile(k.lower_levels(C, scaling, incremental=1), after))


@pytest.mark.parametrize("rescale,C", [(RESCALE_NEVER, 4), (RESCALE_NEVER, 16), (RESCALE_ALWAYS, 4), (RESCALE_ALWAYS, 9)])
def test_l_keep(rescale, C):
    """L-keep: resident partials have no walk lists: both passes are the level kernels'"""
    scaling = rescale == RESCALE_ALWAYS
    pb = _rescaled("caterpillar", C) if scaling else k.unscaled_problem(P_UNSCALED, C)
    with _engine(pb, rescale) as e:
        e.set_keep_partials(True)
        k.check_gradient(e, 0, k.oracle(pb), k.profile(k.lower_levels(C, scaling), k.upper_levels(C, scaling)))


# ---- a memory cap ------------------------------------------------------------------------------------------------------------

def test_w_cap():
    """W-cap: a cap without room for a streamed walk's mask words or table blocks sends it to the table-gather walks
    (lower_stream_capped / upper_stream_capped).  The tile plan reserves more than a plain gradient allocates and knows nothing of
    the mask words, so the caps worth trying are the first ones it accepts untiled: that threshold is found by bisection, then
    128 caps follow it, one mask-word plane apart.  Every cap under which the engine evaluates untiled gives the oracle's numbers;
    the family is reported, not asserted -- the plan's slack may always leave the room"""
    C = 4
    pb = k.unscaled_problem(P_UNSCALED, C)
    ref = k.oracle(pb)
    tol = 1e-9 * max(1.0, np.abs(ref["cat_grad"]).max())
    with _engine(pb, RESCALE_NEVER) as e:
        e.gradient()
        held = e.profile()["device_bytes"]
    plane = (pb.P + 63) // 64 * 64 * 4  # one dword per pattern of the padded blocks

    def untiled(cap):
        try:
            with _engine(pb, RESCALE_NEVER, max_device_bytes=cap) as e:
                return e.profile()["tiles"] == 1
        except EngineError as err:
            assert err.code == _lib.ENOMEM, err
            return False

    lo, hi = plane, 8 * held
    assert not untiled(lo) and untiled(hi)
    while hi - lo > plane:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if untiled(mid) else (mid, hi)
    accepted, on_walk, refused, families = 0, 0, 0, set()
    for cap in range(hi, hi + 128 * plane, plane):
        try:
            with _engine(pb, RESCALE_NEVER, max_device_bytes=cap) as e:
                assert e.profile()["tiles"] == 1
                lnl, cg = e.gradient()
                p = e.pass_profile()
                accepted += 1
                families.add((p["lower_family"], p["upper_family"]))
                on_walk += int(k.WALK in (p["lower_family"], p["upper_family"]))
                assert e.profile()["device_bytes"] <= cap
                assert abs(lnl - ref["lnl"]) <= 1e-10 * abs(ref["lnl"]), (cap, p)
                np.testing.assert_allclose(e.pattern_log_likelihoods(), ref["pattern_lk"], rtol=1e-11, atol=1e-11)
                assert np.abs(cg - ref["cat_grad"]).max() <= tol, (cap, p)
                lnl2, cg2 = e.gradient()
                assert k.same_bits(lnl, lnl2) and k.same_bits(cg, cg2)
        except EngineError as err:
            assert err.code == _lib.ENOMEM, err
            refused += 1
    print(f"W-cap: an uncapped engine holds {held} bytes, the first untiled cap is {hi}; of 128 caps from there {accepted} evaluated, {on_walk} of them on the "
          f"table-gather walks for either pass (families seen: {sorted(families)}), {refused} ran out of memory")
    assert accepted >= 1
