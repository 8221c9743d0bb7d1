"""NumPy helpers over the tables of Engine.pairwise_distances: counts[..., mi, mj] is the summed weight of the patterns where the
pair's first taxon has state mask mi and its second mask mj (4-bit masks, bit s = state s; nucleotides in the order A, C, G, T).

The count-based distances follow the reference's pattern forms (distancematrix.c): only cells where both masks are a single state
count -- the reference's `n1 < 4 && n2 < 4` -- and 1000.0 is returned where the reference returns it.  (The reference sums the
weights of the counted cells into an int; these helpers sum them as they are, which is the same for whole-number weights.)"""
import numpy as np

SINGLE = np.array([1, 2, 4, 8])  # the masks of the single states 0..3
_TRANSITION = np.zeros((4, 4), dtype=bool)
_TRANSITION[0, 2] = _TRANSITION[2, 0] = _TRANSITION[1, 3] = _TRANSITION[3, 1] = True  # A <-> G, C <-> T


def square(values, T):
    """The all-pairs vector (0,1), (0,2), ..., (T-2,T-1) as a symmetric [T, T] matrix with a zero diagonal."""
    values = np.asarray(values)
    if values.shape != (T * (T - 1) // 2,):
        raise ValueError(f"all pairs of {T} taxa are {T * (T - 1) // 2} values (got {values.shape})")
    m = np.zeros((T, T), dtype=values.dtype)
    iu = np.triu_indices(T, 1)  # row-major: the call's order
    m[iu] = values
    m.T[iu] = values
    return m


def state_counts(counts):
    """[..., 4, 4]: the cells where both masks are a single state, by state"""
    counts = np.asarray(counts, dtype=np.float64)
    if counts.shape[-2:] != (16, 16):
        raise ValueError(f"counts must be [..., 16, 16] (got {counts.shape})")
    return counts[..., SINGLE[:, None], SINGLE[None, :]]


def _differences(counts):
    n4 = state_counts(counts)
    n = n4.sum(axis=(-2, -1))
    same = np.trace(n4, axis1=-2, axis2=-1)
    return n - same, n


def p_distance(counts):
    """The uncorrected distance d / n of _distance_raw_patterns: the weight of the cells that differ over the weight of the cells
    compared; 1000.0 where nothing was compared."""
    d, n = _differences(counts)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(n == 0, 1000.0, d / n)


def jc69(counts):
    """The JC69 distance -3/4 log(1 - 4/3 p) of _distance_jc69_patterns, p the uncorrected distance; 1000.0 where p >= 0.75.  Where
    nothing was compared p is 0 / 0 and the result NaN, as in the reference."""
    d, n = _differences(counts)
    with np.errstate(divide="ignore", invalid="ignore"):
        p = d / n
        return np.where(p >= 0.75, 1000.0, -0.75 * np.log(1.0 - (4.0 / 3.0) * p))


def k2p(counts):
    """Kimura's two-parameter distance by the textbook formula -1/2 log(1 - 2 P - Q) - 1/4 log(1 - 2 Q), P and Q the proportions of
    transitions (A <-> G, C <-> T) and transversions among the cells compared.  The reference's expression
    (_distance_k2p_patterns) has 2 * transitions - transversions in its first term where the formula has
    2 * transitions + transversions; this helper does NOT reproduce that.  NaN where nothing was compared or a logarithm's argument is
    not positive."""
    n4 = state_counts(counts)
    n = n4.sum(axis=(-2, -1))
    ts = (n4 * _TRANSITION).sum(axis=(-2, -1))
    tv = n - np.trace(n4, axis1=-2, axis2=-1) - ts
    with np.errstate(divide="ignore", invalid="ignore"):
        P, Q = ts / n, tv / n
        return -0.5 * np.log(1.0 - 2.0 * P - Q) - 0.25 * np.log(1.0 - 2.0 * Q)


# --- the 32 x 32 class tables of Engine.pairwise_distances_general (20 states) ---
# counts[..., ci, cj] is the summed weight of the patterns where the pair's first taxon has class ci and its second class cj: classes
# 0..19 are the states, 20 is unknown and 21 + q an ambiguity set whose number is the engine's own (class_members says what it
# holds).  The count-based distances look at single states only -- the reference's `n1 < state_count && n2 < state_count` -- so
# they need the leading 20 x 20 block and no class_members.
def state_counts_general(counts):
    """[..., 20, 20]: the cells where both classes are a single state, by state"""
    counts = np.asarray(counts, dtype=np.float64)
    if counts.shape[-2:] != (32, 32):
        raise ValueError(f"counts must be [..., 32, 32] (got {counts.shape})")
    return counts[..., :20, :20]


def _differences_general(counts):
    n20 = state_counts_general(counts)
    n = n20.sum(axis=(-2, -1))
    same = np.trace(n20, axis1=-2, axis2=-1)
    return n - same, n


def p_distance_general(counts):
    """p_distance over the class tables: d / n of the cells where both classes are states; 1000.0 where nothing was compared."""
    d, n = _differences_general(counts)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(n == 0, 1000.0, d / n)


def kimura_protein(counts):
    """Kimura's protein distance -log(1 - p - 0.2 p^2) of _distance_aa_kimura_patterns, p = d / n over the cells where both codes
    are states.  As in the reference: NaN where nothing was compared (0 / 0) or the logarithm's argument is negative, inf where it is
    0."""
    d, n = _differences_general(counts)
    with np.errstate(divide="ignore", invalid="ignore"):
        p = d / n
        return -np.log(1.0 - p - 0.2 * p * p)
