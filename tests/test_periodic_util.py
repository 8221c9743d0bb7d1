"""CPU-only: the periodic alignment of tests/periodic_util.py on the oracle alone.  A problem of P patterns whose column j is
column j mod K of a K-pattern problem, and that K-pattern problem with the weights summed per residue class, have the same lnL and
gradient to rounding, and per-pattern lnL and every lower and upper partial of the big one at j are bit for bit the small one's at
j mod K.  This is what tests/test_general_tiles_gpu.py rests on.

Bounds: lnL is a sum of P terms of one sign (w_j log L_j < 0), added in two orders: the two sums differ by at most P * 2^-53 relative,
1e-13 at P = 871.  A gradient row is such a sum of terms of either sign; 1e-12 * max(1, |g|_inf) allows the same P * 2^-53 on a row whose
terms' magnitudes add up to ten times the largest row."""
import numpy as np
import pytest

from gpu_util import random_problem
from hessian_util import branch_hessian_diagonal
from periodic_util import K, assert_periodic_bits, choose_gen_tiles, expand, level_tiles, node_levels, periodic_pair

P = 3 * K + 100  # 871 = 54 * 16 + 7


@pytest.mark.parametrize("S,T,C", [(20, 9, 2), (61, 6, 1)])
@pytest.mark.parametrize("rescale", [0, 1])
def test_periodic_problem_equals_its_period(S, T, C, rescale):
    period = random_problem(T, K, C, seed=S + T + rescale, S=S, gaps=0.05, bl=(0.3, 0.9) if rescale else (0.01, 0.1), rescale=rescale)
    big, small = periodic_pair(period, P, seed=5)
    assert big.P == P and small.P == K
    assert np.all((big.weights >= 1) & (big.weights <= 4)) and not np.array_equal(big.weights[:K], big.weights[K:2 * K])
    assert small.weights.sum() == big.weights.sum()
    for t in range(T):
        assert np.array_equal(big.tip_states[t], expand(period.tip_states[t], P, 0))
    rb, rs = big.gradient(want_partials=True), small.gradient(want_partials=True)
    assert rb["rescaled"] == rs["rescaled"] == bool(rescale)
    assert abs(rb["lnl"] - rs["lnl"]) <= 1e-13 * abs(rs["lnl"])
    assert np.abs(rb["cat_grad"] - rs["cat_grad"]).max() <= 1e-12 * max(1.0, np.abs(rs["cat_grad"]).max())
    assert np.array_equal(rb["pattern_lk"], expand(rs["pattern_lk"], P, 0))
    assert np.array_equal(rb["lower"], expand(rs["lower"], P, 2))
    others = [n for n in range(big.N) if n != big.root]  # (the root has no upper: its rows are not written)
    assert np.array_equal(rb["upper"][others], expand(rs["upper"][others], P, 2))
    assert_periodic_bits(rb["pattern_lk"], 0)
    assert_periodic_bits(rb["lower"], 2)


def test_hessian_restatement_on_the_period():
    period = random_problem(7, K, 2, seed=3, S=20, gaps=0.05)
    big, small = periodic_pair(period, P, seed=6)
    (lb, b1, b2), (ls, s1, s2) = branch_hessian_diagonal(big), branch_hessian_diagonal(small)
    assert abs(lb - ls) <= 1e-13 * abs(ls)
    assert np.abs(b1 - s1).max() <= 1e-12 * max(1.0, np.abs(s1).max()) and np.abs(b2 - s2).max() <= 1e-12 * max(1.0, np.abs(s2).max())


def test_assert_periodic_bits_sees_one_changed_entry():
    a = np.tile(np.arange(K, dtype=np.float64), 4)[:P].reshape(1, P, 1) * np.ones((2, 1, 3))
    assert_periodic_bits(a, 1)
    a[1, 700, 2] = np.nextafter(a[1, 700, 2], np.inf)
    with pytest.raises(AssertionError, match="positions 443 and 700"):
        assert_periodic_bits(a, 1)


def test_tile_chooser_restatement():
    """one round of workgroups is the cheapest schedule: 1 tile while work x ceil(P / 128) fits the slots, more beyond"""
    assert choose_gen_tiles(16411, 3, 512, 20) == 1  # 3 x 129 = 387 workgroups
    assert choose_gen_tiles(16411, 4, 512, 20) == 2  # 516 workgroups: two rounds of one tile cost 6, one round of two tiles 4
    assert choose_gen_tiles(16411, 128, 512, 20) >= 4
    pb = random_problem(64, 8, 4, seed=1, S=20)
    height, depth, parent = node_levels(pb)
    assert height[pb.root] == height.max() and depth[pb.root] == 0 and parent[pb.root] == -1
    for slots in (256, 512, 1024):
        for by in (height, depth):
            tiles = set(level_tiles(pb, 16411, slots, by).values())
            assert min(tiles) < max(tiles) and max(tiles) >= 2, (slots, tiles)  # several tile counts in one pass
