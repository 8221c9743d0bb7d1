"""A periodic alignment: the oracle's cost of K patterns for an engine of P >> K patterns.

Column j of the big problem is column j mod K of an oracle Problem of K patterns; its weight w_j is an integer 1..4 drawn per j (not
periodic: a weight read from the wrong pattern shows).  The oracle runs on the K patterns with W_k = sum of w_j over j = k mod K
(small integers: exact in fp64), and its lnL, gradient and every other sum over patterns are those of the big problem to rounding
(another order of the same terms).  Per-pattern results of the big problem at position j are the oracle's at j mod K: a pattern's
column goes through the same products wherever it stands.  K = 257 is odd and shares no factor with 16 (a tile) or 128 (a
workgroup's patterns), so over the periods every column lands in every lane of a tile and every tile of a workgroup.

Also here: the restatement of the tile chooser of the 20 / 60 / 61-state level kernels (choose_gen_tiles, phyamd_launch.inc) over
the levels of a tree, by which a test picks a node per tile count and a pattern count is sized."""
import numpy as np

from oracle import phyoracle as po

K = 257
GEN_TILES_MAX, GEN_WAVES = 8, 8  # phyamd_general.inc


def _with(pb, tip_states, tip_partials, weights):
    return po.Problem(pb.left, pb.right, pb.root, weights, pb.eval, pb.evec, pb.ivec, pb.freqs, pb.cat_rates, pb.cat_props, pb.branch_lengths,
                      tip_states=tip_states, tip_partials=tip_partials, rescale=pb.rescale, compat_scaled_gradient=pb.compat_scaled_gradient,
                      fold_root_freqs=pb.fold_root_freqs)


def periodic_pair(period, P, seed):
    """(big, small) from an oracle Problem `period` of K patterns: `big` has P patterns, column j = column j mod K of `period`,
    weights independent integers 1..4; `small` is `period` with the weights summed over each residue class."""
    k = period.P
    assert P > k
    idx = np.arange(P) % k
    w = np.random.default_rng(seed).integers(1, 5, size=P).astype(np.float64)
    W = np.bincount(idx, weights=w, minlength=k)
    assert np.all(W == np.round(W)) and W.sum() == w.sum()  # sums of small integers: exact
    states = None if period.tip_states is None else period.tip_states[:, idx]
    partials = None if period.tip_partials is None else period.tip_partials[:, idx]
    return _with(period, states, partials, w), _with(period, period.tip_states, period.tip_partials, W)


def expand(a, P, axis):
    """an array with K entries along `axis` -> P entries, position j from j mod K"""
    return np.take(a, np.arange(P) % a.shape[axis], axis=axis)


def assert_periodic_bits(a, axis, k=K):
    """positions j and j + k along `axis` hold the same bits (NaNs would fail: there are none to expect)"""
    a = np.moveaxis(np.asarray(a), axis, 0)
    assert a.shape[0] > k
    same = a[:-k] == a[k:]
    if not same.all():
        j = int(np.argwhere(same.reshape(same.shape[0], -1).all(axis=1) == 0)[0, 0])
        rel = np.abs(a[j] - a[j + k]).max() / max(np.abs(a[j]).max(), 1e-300)
        raise AssertionError(f"positions {j} and {j + k} differ (relative {rel:.3e}); {int((~same).sum())} entries differ in all")


# ---- which tile count each level of a tree gets -------------------------------------------------------------------------------

def choose_gen_tiles(P, work, slots, S):
    """choose_gen_tiles(P, 8 waves, work = ops x categories, slots, gen_stage_cost(S)) of phyamd_launch.inc"""
    stage = 2.0 if S == 20 else 0.6
    total = (P + 15) // 16
    best, best_cost = 1, 0.0
    for q in range(1, GEN_TILES_MAX + 1):
        wgs = work * ((total + GEN_WAVES * q - 1) // (GEN_WAVES * q))
        cost = float((wgs + slots - 1) // slots) * (stage + q)
        if q == 1 or cost < best_cost * (1.0 - 1e-9):
            best, best_cost = q, cost
    return best


def node_levels(pb):
    """(height, depth, parent) of every node of a Problem's tree when every internal node is stored (keep-partials, rescaled, 60 /
    61 states): the post-order pass launches the internal nodes of height h = 1, 2, ... together, the pre-order pass those of
    depth d = 0, 1, ... (build_schedule)."""
    N, T = pb.N, pb.T
    parent = np.full(N, -1)
    depth = np.zeros(N, dtype=int)
    order, stack = [], [pb.root]
    while stack:
        n = stack.pop()
        order.append(n)
        if n >= T:
            for ch in (int(pb.left[n]), int(pb.right[n])):
                parent[ch], depth[ch] = n, depth[n] + 1
                stack.append(ch)
    height = np.zeros(N, dtype=int)
    for n in reversed(order):
        if n >= T:
            height[n] = 1 + max(height[pb.left[n]], height[pb.right[n]])
    return height, depth, parent


def level_tiles(pb, P, slots, by):
    """{level: tiles per wave} of a pass over every internal node, levels keyed by `by` (height: post-order, depth: pre-order)"""
    out = {}
    for lv in sorted(set(int(by[n]) for n in range(pb.T, pb.N))):
        cnt = sum(1 for n in range(pb.T, pb.N) if by[n] == lv)
        out[lv] = choose_gen_tiles(P, cnt * pb.C, slots, pb.S)
    return out
