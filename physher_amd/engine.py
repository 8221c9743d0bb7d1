"""numpy-facing wrapper over the C ABI (include/physher_amd.h).  No computation happens in Python."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import (GRAD_COMPAT_SCALED, GRAD_FOLD_ROOT_FREQS, RESCALE_ALWAYS, RESCALE_AUTO, RESCALE_NEVER,  # noqa: F401
                   EngineError)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class Engine:
    """One tree-likelihood instance on one GPU (the device analogue of physher's SingleTreeLikelihood)."""

    def __init__(self, tip_count, pattern_count, state_count=4, category_count=1, device=-1, rescale=RESCALE_AUTO,
                 max_device_bytes=0, stream=None, devices=None):
        """devices: list of HIP device ordinals -> the patterns are sharded over them inside this process
        (phyamd_create_sharded; the same ordinal may repeat); None -> one engine on `device`."""
        self._lib = _lib.load()
        self.T, self.P, self.S, self.C = int(tip_count), int(pattern_count), int(state_count), int(category_count)
        self.N = 2 * self.T - 1
        self._lengths = self._stored_lengths = None  # what set_branch_lengths / set_branch_length last sent, and store()'s copy
        cfg = _lib.Config(self.T, self.P, self.S, self.C, device, rescale, max_device_bytes, stream)
        h = C.c_void_p()
        self._h = None
        if devices is None:
            self._check(self._lib.phyamd_create(C.byref(cfg), C.byref(h)))
        else:
            ids = np.ascontiguousarray(devices, dtype=np.int32)
            self._check(self._lib.phyamd_create_sharded(C.byref(cfg), len(ids), _ptr(ids), C.byref(h)))
        self._h = h

    @property
    def shard_count(self):
        return self._lib.phyamd_shard_count(self._h)

    def _check(self, rc):
        if rc != 0:
            raise EngineError(rc, self._lib.phyamd_last_error().decode())

    def close(self):
        if self._h is not None:
            self._lib.phyamd_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # --- data
    def set_tip_states(self, tip, states):
        a = np.ascontiguousarray(states, dtype=np.uint8)
        assert a.shape == (self.P,)
        self._check(self._lib.phyamd_set_tip_states(self._h, tip, _ptr(a)))

    def set_tip_partials(self, tip, partials):
        a = _f64(partials)
        assert a.shape == (self.P, self.S)
        self._check(self._lib.phyamd_set_tip_partials(self._h, tip, _ptr(a)))

    def set_pattern_weights(self, w):
        a = _f64(w)
        assert a.shape == (self.P,)
        self._check(self._lib.phyamd_set_pattern_weights(self._h, _ptr(a)))

    def set_topology(self, left, right, root):
        l = np.ascontiguousarray(left, dtype=np.int32)
        r = np.ascontiguousarray(right, dtype=np.int32)
        assert l.shape == (self.N,) and r.shape == (self.N,)
        self._check(self._lib.phyamd_set_topology(self._h, _ptr(l), _ptr(r), int(root)))

    def set_branch_lengths(self, bl):
        a = _f64(bl)
        assert a.shape == (self.N,)
        self._check(self._lib.phyamd_set_branch_lengths(self._h, _ptr(a)))
        self._lengths = a.copy()  # (optimize_branch_lengths' default start)

    def set_branch_length(self, node, length):
        """One branch; the next evaluation only recomputes the path from `node` to the root."""
        self._check(self._lib.phyamd_set_branch_length(self._h, int(node), float(length)))
        if self._lengths is not None:
            self._lengths[int(node)] = float(length)

    def update_all_nodes(self):
        self._check(self._lib.phyamd_update_all_nodes(self._h))

    def set_eigen(self, eval_, evec, ivec):
        a, b, c = _f64(eval_), _f64(evec), _f64(ivec)
        assert a.shape == (self.S,) and b.shape == (self.S, self.S) and c.shape == (self.S, self.S)
        self._check(self._lib.phyamd_set_eigen(self._h, _ptr(a), _ptr(b), _ptr(c)))

    def set_frequencies(self, f):
        a = _f64(f)
        assert a.shape == (self.S,)
        self._check(self._lib.phyamd_set_frequencies(self._h, _ptr(a)))

    def set_category_rates(self, rates, props):
        a, b = _f64(rates), _f64(props)
        assert a.shape == (self.C,) and b.shape == (self.C,)
        self._check(self._lib.phyamd_set_category_rates(self._h, _ptr(a), _ptr(b)))

    def set_node_matrices(self, node, mats):
        a = _f64(mats)
        assert a.shape == (self.C, self.S, self.S)
        self._check(self._lib.phyamd_set_node_matrices(self._h, node, _ptr(a)))

    def set_matrices(self, mats):
        """explicit P(t) of every node at once: [N][C][S][S] by node id (the root's entry is ignored)"""
        a = _f64(mats)
        assert a.shape == (self.N, self.C, self.S, self.S)
        self._check(self._lib.phyamd_set_matrices(self._h, _ptr(a)))

    def set_rate_matrix(self, Q):
        a = _f64(Q)
        assert a.shape == (self.S, self.S)
        self._check(self._lib.phyamd_set_rate_matrix(self._h, _ptr(a)))

    # --- evaluation
    def log_likelihood(self):
        v = C.c_double()
        self._check(self._lib.phyamd_log_likelihood(self._h, C.byref(v)))
        return v.value

    def gradient(self, flags=0):
        """Returns (lnL, cat_gradient [N][C])."""
        v = C.c_double()
        g = np.empty((self.N, self.C))
        self._check(self._lib.phyamd_gradient(self._h, flags, C.byref(v), _ptr(g)))
        return v.value, g

    def branch_gradient(self, flags=0, rates_without_mu=None):
        v = C.c_double()
        g = np.empty(self.N)
        r = None if rates_without_mu is None else _f64(rates_without_mu)
        self._check(self._lib.phyamd_branch_gradient(self._h, flags, None if r is None else _ptr(r), C.byref(v), _ptr(g)))
        return v.value, g

    def log_likelihood_device(self, device_ptr):
        """post-order pass only; lnL -> device_ptr[0] on the engine's stream"""
        self._check(self._lib.phyamd_log_likelihood_device(self._h, C.c_void_p(device_ptr)))

    def gradient_device(self, device_ptr, flags=0):
        self._check(self._lib.phyamd_gradient_device(self._h, flags, C.c_void_p(device_ptr)))

    def root_invariant_term(self):
        v = C.c_double()
        self._check(self._lib.phyamd_root_invariant_term(self._h, C.byref(v)))
        return v.value

    # --- substitution-model gradient (calculate_dlnl_dQ, treelikelihood.c:2337-2583)
    def set_rate_matrix_derivatives(self, dQ):
        """dQ [count][S][S]: d(normalised Q)/d(parameter); an empty array clears."""
        dQ = np.ascontiguousarray(dQ, dtype=np.float64).reshape(-1, self.S, self.S)
        self._np = dQ.shape[0]
        self._check(self._lib.phyamd_set_rate_matrix_derivatives(self._h, self._np, _ptr(dQ)))

    def parameter_gradient(self, flags=0):
        """(lnL, cat_gradient [N][C], parameter_gradient [count]) from one post-order + one pre-order pass."""
        lnl = C.c_double()
        g = np.empty((self.N, self.C))
        pg = np.empty(getattr(self, "_np", 0))
        self._check(self._lib.phyamd_parameter_gradient(self._h, flags, C.byref(lnl), _ptr(g), _ptr(pg)))
        return lnl.value, g, pg

    def parameter_gradient_device(self, device_ptr, flags=0):
        """[lnL | cat gradient | parameter gradient | root frequency term] -> device buffer (1 + N*C + count + S doubles)."""
        self._check(self._lib.phyamd_parameter_gradient_device(self._h, flags, C.c_void_p(device_ptr)))

    def root_frequency_term(self):
        a = np.empty(self.S)
        self._check(self._lib.phyamd_root_frequency_term(self._h, _ptr(a)))
        return a

    def branch_log_likelihood(self, node, length):
        """(lnL, d lnL/dt, d2 lnL/dt2) of one branch at a trial length, from the resident upper/lower partials
        (needs set_keep_partials(True) and a gradient() call for the current parameters)."""
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        self._check(self._lib.phyamd_branch_log_likelihood(self._h, int(node), float(length), C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def branch_hessian_diagonal(self, flags=0):
        """(lnL, d1 [N], d2 [N]): every branch's d lnL/dt and d2 lnL/dt2 at its current length from one post-order and one
        pre-order pass (row n = branch_log_likelihood(n, t_n)[1:]; root row 0)."""
        v = C.c_double()
        d1, d2 = np.empty(self.N), np.empty(self.N)
        self._check(self._lib.phyamd_branch_hessian_diagonal(self._h, flags, C.byref(v), _ptr(d1), _ptr(d2)))
        return v.value, d1, d2

    def branch_hessian_diagonal_device(self, device_ptr, flags=0):
        """[lnL | d1[N] | d2[N]] -> device_ptr on the engine's stream (sums over this engine's patterns)"""
        self._check(self._lib.phyamd_branch_hessian_diagonal_device(self._h, flags, C.c_void_p(device_ptr)))

    def gradient_batch(self, branch_lengths, flags=0, want_gradient=True):
        """lnL and the per-category branch gradient for B branch-length vectors [B, N] at once: (lnl [B], g [B, N, C] or None).
        Item b is what set_branch_lengths(branch_lengths[b]) + gradient(flags) returns; the engine's own lengths stay."""
        bl = _f64(branch_lengths)
        if bl.ndim != 2 or bl.shape[1] != self.N or bl.shape[0] < 1:
            raise ValueError(f"branch_lengths must be [B >= 1, {self.N}] (got {bl.shape})")
        count = bl.shape[0]
        lnl = np.empty(count)
        g = np.empty((count, self.N, self.C)) if want_gradient else None
        self._check(self._lib.phyamd_gradient_batch(self._h, flags, count, _ptr(bl), _ptr(lnl), None if g is None else _ptr(g)))
        return lnl, g

    def gradient_batch_trees(self, left, right, roots, branch_lengths, flags=0, want_gradient=True):
        """lnL and the per-category branch gradient of B trees on this engine's data and models at once: left, right [B, N] and
        roots [B] in set_topology's convention per item, branch_lengths [B, N] by the item's node ids -> (lnl [B], g [B, N, C] by
        the item's node ids, or None).  Item b is what a fresh engine returns from set_topology + set_branch_lengths +
        gradient(flags); this engine's own tree, lengths and partials stay.  No item-by-item fallback: EngineError otherwise."""
        l = np.ascontiguousarray(left, dtype=np.int32)
        r = np.ascontiguousarray(right, dtype=np.int32)
        ro = np.ascontiguousarray(roots, dtype=np.int32)
        bl = _f64(branch_lengths)
        if l.ndim != 2 or l.shape[1] != self.N or l.shape[0] < 1:
            raise ValueError(f"left: [B >= 1, {self.N}], got {l.shape}")
        count = l.shape[0]
        if r.shape != l.shape or bl.shape != l.shape or ro.shape != (count,):
            raise ValueError(f"right, branch_lengths: {l.shape} and roots: ({count},), got {r.shape}, {bl.shape}, {ro.shape}")
        lnl = np.empty(count)
        g = np.empty((count, self.N, self.C)) if want_gradient else None
        self._check(self._lib.phyamd_gradient_batch_trees(self._h, flags, count, _ptr(l), _ptr(r), _ptr(ro), _ptr(bl), _ptr(lnl),
                                                          None if g is None else _ptr(g)))
        return lnl, g

    def batch_profile(self):
        """Of the last gradient_batch / gradient_batch_trees: items_fast / items_sequential, chunks, scratch_bytes, ms."""
        p = _lib.BatchProfile()
        self._check(self._lib.phyamd_get_batch_profile(self._h, C.byref(p)))
        return {k: getattr(p, k) for k, _ in p._fields_}

    def nni_log_likelihoods(self, central_lengths=None, want_derivatives=True, flags=0):
        """Every NNI neighbour of this engine's tree at once: (lnl, d1, d2), each [3, N] (d1, d2 None without want_derivatives).
        Column v is an internal node other than the root, with parent u, sibling s and children a = left[v], b = right[v]; row 0 is
        the engine's tree, row 1 has a and s exchanged, row 2 b and s.  central_lengths [3, N]: the trial length of branch v per row
        (None: its own length; entries at tips and the root are ignored).  d1, d2: the derivatives of that lnL in the length of v,
        as branch_hessian_diagonal defines them.  Tips' and the root's columns are NaN.  The engine's tree, lengths and partials
        stay.  No fallback: EngineError where gradient_batch_trees refuses."""
        cl = None
        if central_lengths is not None:
            cl = _f64(central_lengths)
            if cl.shape != (3, self.N):
                raise ValueError(f"central_lengths must be [3, {self.N}] (got {cl.shape})")
        lnl = np.empty((3, self.N))
        d1 = np.empty((3, self.N)) if want_derivatives else None
        d2 = np.empty((3, self.N)) if want_derivatives else None
        self._check(self._lib.phyamd_nni_log_likelihoods(self._h, flags, None if cl is None else _ptr(cl), _ptr(lnl),
                                                         None if d1 is None else _ptr(d1), None if d2 is None else _ptr(d2)))
        return lnl, d1, d2

    def nni_log_likelihoods_general(self, central_lengths=None, want_derivatives=True, flags=0):
        """nni_log_likelihoods for an engine of 20 states: (lnl, d1, d2), each [3, N], in that method's rows and columns and by its
        definition -- entry (k, v) is this engine's own log_likelihood and rows v of branch_hessian_diagonal on the rearranged tree
        with the length of v set to central_lengths[k, v] (None: its own).  The four messages round every edge are read from the
        resident partials: afterwards the engine is one with set_keep_partials(True) that has run gradient(); its tree, lengths and
        models stay.  An entry whose lnL is not finite has NaN d1 and d2.  No fallback: EngineError for a state count other than 20,
        more than 8 categories, flags, tiled patterns, explicit matrices, a rescaling or a sharded engine."""
        cl = None
        if central_lengths is not None:
            cl = _f64(central_lengths)
            if cl.shape != (3, self.N):
                raise ValueError(f"central_lengths must be [3, {self.N}] (got {cl.shape})")
        lnl = np.empty((3, self.N))
        d1 = np.empty((3, self.N)) if want_derivatives else None
        d2 = np.empty((3, self.N)) if want_derivatives else None
        self._check(self._lib.phyamd_nni_log_likelihoods_general(self._h, flags, None if cl is None else _ptr(cl), _ptr(lnl),
                                                                 None if d1 is None else _ptr(d1), None if d2 is None else _ptr(d2)))
        return lnl, d1, d2

    def nni_profile(self):
        """Of the last nni_log_likelihoods or nni_log_likelihoods_general: candidates (edges scored), scratch_bytes, ms."""
        p = _lib.NniProfile()
        self._check(self._lib.phyamd_get_nni_profile(self._h, C.byref(p)))
        return {k: getattr(p, k) for k, _ in p._fields_}

    def nni_optimize(self, start_lengths=None, lower=1e-8, upper=10.0, tolerance=1e-8, max_iterations=100, want_derivatives=True,
                     want_iterations=True, flags=0):
        """The central branch of every NNI neighbour optimised on the device: (lengths, lnl, d1, d2, iterations), each [3, N] in
        nni_log_likelihoods' rows and columns (NaN, iterations 0, at tips and the root; d1, d2 / iterations None when not wanted).
        Per entry the length of v in [lower, upper] that maximises its lnL, by a safeguarded Newton iteration from start_lengths
        [3, N] (None: the branch's own length): d1 > 0 moves the bracket's low end to t, else its high end; the Newton step is
        taken when d2 < 0 and it stays inside the bracket, else the bracket is halved; the entry stops on a step <= tolerance.
        iterations: the steps proposed, negated where max_iterations ran out or lnL was not finite.  lnl, d1, d2 are those of
        nni_log_likelihoods at the returned lengths.  The engine's tree, lengths and partials stay.  No fallback: EngineError
        where nni_log_likelihoods refuses, and on a sharded engine."""
        return self._nni_optimize(self._lib.phyamd_nni_optimize, start_lengths, lower, upper, tolerance, max_iterations, want_derivatives, want_iterations, flags)

    def nni_optimize_general(self, start_lengths=None, lower=1e-8, upper=10.0, tolerance=1e-8, max_iterations=100, want_derivatives=True,
                             want_iterations=True, flags=0):
        """nni_optimize for an engine of 20 states: (lengths, lnl, d1, d2, iterations), each [3, N], in that method's rows and
        columns, by its rule and with its sign convention for iterations.  lnl, d1, d2 are those of nni_log_likelihoods_general at
        the returned lengths.  The four messages round every edge are read from the resident partials: afterwards the engine is
        one with set_keep_partials(True) that has run gradient(); its tree, lengths and models stay.  An entry whose lnL is not
        finite at an iterate ends there with NaN d1 and d2 and a negative count.  No fallback: EngineError for a state count other
        than 20, more than 8 categories, flags, tiled patterns, explicit matrices, a rescaling or a sharded engine."""
        return self._nni_optimize(self._lib.phyamd_nni_optimize_general, start_lengths, lower, upper, tolerance, max_iterations, want_derivatives, want_iterations,
                                  flags)

    def _nni_optimize(self, call, start_lengths, lower, upper, tolerance, max_iterations, want_derivatives, want_iterations, flags):
        sl = None
        if start_lengths is not None:
            sl = _f64(start_lengths)
            if sl.shape != (3, self.N):
                raise ValueError(f"start_lengths must be [3, {self.N}] (got {sl.shape})")
        lengths, lnl = np.empty((3, self.N)), np.empty((3, self.N))
        d1 = np.empty((3, self.N)) if want_derivatives else None
        d2 = np.empty((3, self.N)) if want_derivatives else None
        it = np.empty((3, self.N), dtype=np.int32) if want_iterations else None
        self._check(call(self._h, flags, None if sl is None else _ptr(sl), lower, upper, tolerance, max_iterations, _ptr(lengths), _ptr(lnl),
                         None if d1 is None else _ptr(d1), None if d2 is None else _ptr(d2), None if it is None else _ptr(it)))
        return lengths, lnl, d1, d2, it

    def nni_optimize_profile(self):
        """Of the last nni_optimize or nni_optimize_general: candidates, chunks (of candidates), scratch_bytes, iterations (over all entries), ms."""
        p = _lib.NniOptimizeProfile()
        self._check(self._lib.phyamd_get_nni_optimize_profile(self._h, C.byref(p)))
        return {k: getattr(p, k) for k, _ in p._fields_}

    def optimize_branch_lengths(self, trees=None, lengths=None, optimise=None, lower=1e-8, upper=10.0, tolerance=1e-8, max_iterations=100,
                                lnl_tolerance=1e-6, max_passes=50, want_initial=True, want_passes=True, flags=0):
        """Every branch length of B trees optimised on the device, one branch at a time, pass after pass: (lengths [B, N], lnl [B],
        initial_lnl [B], passes [B]; the last two None when not wanted).  trees: (left [B, N], right [B, N], roots [B]) as
        gradient_batch_trees takes them, or None: every item is this engine's tree.  lengths [B, N] by the item's node ids is the
        start; None with trees None: one item on the lengths last given to set_branch_lengths.  optimise [B, N]: non-zero where
        the node's branch is visited (None: every node but the root).  A pass visits the nodes in post-order; a visit moves its
        branch by nni_optimize's safeguarded Newton rule in [lower, upper] and keeps the move when lnL did not fall.  An item stops
        when a pass gains no more than lnl_tolerance (passes > 0) or after max_passes (passes = -max_passes); a lnL that is not
        finite ends it in band with passes negative.  The engine's tree, lengths and partials stay.  No fallback: EngineError where
        gradient_batch_trees refuses, and on a sharded engine."""
        if lengths is None:
            if trees is not None or self._lengths is None:
                raise ValueError("lengths=None needs trees=None and an engine whose set_branch_lengths has been called")
            lengths = self._lengths[None, :]
        bl = _f64(lengths)
        if bl.ndim != 2 or bl.shape[1] != self.N or bl.shape[0] < 1:
            raise ValueError(f"lengths must be [B >= 1, {self.N}] (got {bl.shape})")
        count = bl.shape[0]
        l = r = ro = None
        if trees is not None:
            l, r, ro = (np.ascontiguousarray(x, dtype=np.int32) for x in trees)
            if l.shape != bl.shape or r.shape != bl.shape or ro.shape != (count,):
                raise ValueError(f"trees: left, right {bl.shape} and roots ({count},), got {l.shape}, {r.shape}, {ro.shape}")
        m = None
        if optimise is not None:
            m = np.ascontiguousarray(np.asarray(optimise) != 0, dtype=np.uint8)
            if m.shape != bl.shape:
                raise ValueError(f"optimise must be {bl.shape} (got {m.shape})")
        out, lnl = np.empty((count, self.N)), np.empty(count)
        lnl0 = np.empty(count) if want_initial else None
        passes = np.empty(count, dtype=np.int32) if want_passes else None
        opt = lambda a: None if a is None else _ptr(a)
        self._check(self._lib.phyamd_optimize_branch_lengths(self._h, flags, count, opt(l), opt(r), opt(ro), _ptr(bl), opt(m), lower, upper, tolerance,
                                                             max_iterations, lnl_tolerance, max_passes, _ptr(out), _ptr(lnl), opt(lnl0), opt(passes)))
        return out, lnl, lnl0, passes

    def branch_optimize_profile(self):
        """Of the last optimize_branch_lengths: items, chunks (of items), passes (the most a chunk ran), visits and iterations
        (over all items), scratch_bytes, ms."""
        p = _lib.BranchOptimizeProfile()
        self._check(self._lib.phyamd_get_branch_optimize_profile(self._h, C.byref(p)))
        return {k: getattr(p, k) for k, _ in p._fields_}

    def spr_log_likelihoods(self, prune=None, flags=0):
        """Every SPR regraft of the prune nodes' subtrees at once: lnl [count, N].  Row i prunes node prune[i] (None: every node, row
        i is node i); column w regrafts it onto the edge above w: with u the prune node's parent and s its sibling, s takes u's
        place under u's parent with length t_s + t_u, u takes w's place under w's parent and gets w where s was, and both halves
        of the graft edge get 0.5 t_w.  NaN where w is the root, u, s, the prune node or one of its descendants, and in the whole
        row of the root and of its children (re-root to reach those moves).  lnL only, at that fixed assignment: spr_optimize
        optimises the three branches at the graft point of every candidate.
        The engine's tree, lengths and partials stay.  No fallback: EngineError where gradient_batch_trees refuses."""
        return self._spr_log_likelihoods(self._lib.phyamd_spr_log_likelihoods, prune, flags)

    def spr_log_likelihoods_general(self, prune=None, flags=0):
        """spr_log_likelihoods for an engine of 20 states: lnl [count, N] in that method's rows and columns, by its move and its
        candidate rule; an entry is the engine's own log_likelihood() of the rearranged tree.  The messages and uppers that
        pruning changes are walked per row from the resident lower partials: afterwards the engine is one with
        set_keep_partials(True) that has run gradient(); its tree, lengths and models stay.  A candidate whose lnL is not finite
        reports it in band.  No fallback: EngineError for a state count other than 20, more than 8 categories, flags, tiled
        patterns, explicit matrices, a rescaling or a sharded engine, and a row whose scratch does not fit the memory cap."""
        return self._spr_log_likelihoods(self._lib.phyamd_spr_log_likelihoods_general, prune, flags)

    def _spr_log_likelihoods(self, call, prune, flags):
        pr = None
        if prune is not None:
            pr = np.ascontiguousarray(prune, dtype=np.int32)
            if pr.ndim != 1:
                raise ValueError(f"prune must be one-dimensional (got {pr.shape})")
        count = self.N if pr is None else len(pr)
        lnl = np.empty((count, self.N))
        self._check(call(self._h, flags, count, None if pr is None else _ptr(pr), _ptr(lnl)))
        return lnl

    def spr_profile(self):
        """Of the last spr_log_likelihoods or spr_log_likelihoods_general: prunes (rows), chunks, candidates, scratch_bytes, ms."""
        p = _lib.SprProfile()
        self._check(self._lib.phyamd_get_spr_profile(self._h, C.byref(p)))
        return {k: getattr(p, k) for k, _ in p._fields_}

    def spr_optimize(self, prune=None, lower=1e-8, upper=10.0, tolerance=1e-8, max_iterations=100, lnl_tolerance=1e-6, max_passes=50,
                     want_initial_lnl=True, want_passes=True, flags=0):
        """The three branches that meet at the graft point of every SPR regraft optimised on the device: (lengths [count, N, 3],
        lnl [count, N], initial_lnl [count, N], passes [count, N]; the last two None when not wanted), in spr_log_likelihoods' rows,
        columns and rearranged trees.  lengths holds (t_p, t_w, t_u) of the prune node, the target node and the prune node's
        parent, from the start (t_p, 0.5 t_w, 0.5 t_w).  An entry is what optimize_branch_lengths returns for its rearranged tree
        with only those three nodes marked: a pass visits the parent's left child, its right child, then the parent; a visit moves
        its branch by nni_optimize's safeguarded Newton rule in [lower, upper] and keeps the move when lnL did not fall; the entry
        stops when a pass gains no more than lnl_tolerance (passes > 0) or after max_passes (passes = -max_passes); a lnL that is
        not finite ends it in band with passes negative.  NaN (passes 0) wherever spr_log_likelihoods has NaN.  The engine's tree,
        lengths and partials stay.  No fallback: EngineError where spr_log_likelihoods refuses, and on a sharded engine."""
        return self._spr_optimize(self._lib.phyamd_spr_optimize, prune, lower, upper, tolerance, max_iterations, lnl_tolerance, max_passes, want_initial_lnl,
                                  want_passes, flags)

    def spr_optimize_general(self, prune=None, lower=1e-8, upper=10.0, tolerance=1e-8, max_iterations=100, lnl_tolerance=1e-6, max_passes=50,
                             want_initial_lnl=True, want_passes=True, flags=0):
        """spr_optimize for an engine of 20 states: the same tuple, in spr_log_likelihoods_general's rows, columns and rearranged
        trees, by spr_optimize's start, pass order, visit rule and stop test; all three branches are always visited.  The two
        branches a visit holds enter through the engine's own matrix arithmetic, the visited one through the eigen sum.  The rows
        are walked from the resident lower partials: afterwards the engine is one with set_keep_partials(True) that has run
        gradient(); its tree, lengths and models stay.  A lnL that is not finite ends an entry in band with passes negative.  No
        fallback: EngineError for a state count other than 20, more than 8 categories, flags, tiled patterns, explicit matrices, a
        rescaling or a sharded engine, and a row whose scratch does not fit the memory cap."""
        return self._spr_optimize(self._lib.phyamd_spr_optimize_general, prune, lower, upper, tolerance, max_iterations, lnl_tolerance, max_passes,
                                  want_initial_lnl, want_passes, flags)

    def _spr_optimize(self, call, prune, lower, upper, tolerance, max_iterations, lnl_tolerance, max_passes, want_initial_lnl, want_passes, flags):
        pr = None
        if prune is not None:
            pr = np.ascontiguousarray(prune, dtype=np.int32)
            if pr.ndim != 1:
                raise ValueError(f"prune must be one-dimensional (got {pr.shape})")
        count = self.N if pr is None else len(pr)
        lengths, lnl = np.empty((count, self.N, 3)), np.empty((count, self.N))
        lnl0 = np.empty((count, self.N)) if want_initial_lnl else None
        passes = np.empty((count, self.N), dtype=np.int32) if want_passes else None
        opt = lambda a: None if a is None else _ptr(a)
        self._check(call(self._h, flags, count, opt(pr), lower, upper, tolerance, max_iterations, lnl_tolerance, max_passes, _ptr(lengths), _ptr(lnl), opt(lnl0),
                         opt(passes)))
        return lengths, lnl, lnl0, passes

    def spr_optimize_profile(self):
        """Of the last spr_optimize or spr_optimize_general: prunes (rows), chunks (of rows), candidates, visits and iterations (over all candidates),
        scratch_bytes, ms."""
        p = _lib.SprOptimizeProfile()
        self._check(self._lib.phyamd_get_spr_optimize_profile(self._h, C.byref(p)))
        return {k: getattr(p, k) for k, _ in p._fields_}

    def pairwise_distances(self, pairs=None, start=None, lower=1e-8, upper=10.0, tolerance=1e-8, max_iterations=100, want_derivatives=True,
                           want_iterations=True, want_counts=False, counts_only=False, flags=0):
        """The maximum-likelihood distance of pairs of taxa under the engine's own model, on the device, before any topology exists:
        (distances [count], lnl [count], d1 [count], d2 [count], iterations [count] int32, counts [count, 16, 16]); what is not
        wanted is None.  pairs [count, 2] holds (i, j), i the side that carries pi (None: all i < j, row-major: distances.square
        makes the matrix).  Per pair the length in [lower, upper] that maximises the two-tip likelihood, by nni_optimize's
        safeguarded Newton rule from start[p] (None: 0.1); lnl, d1 and d2 there; iterations negative where max_iterations ran out
        or lnL was not finite.  Identical rows end at lower, saturated pairs at upper.  counts[p, mi, mj] is the summed weight of
        the patterns where taxon i has state mask mi and taxon j mask mj (bit s = state s): the sufficient statistic of the ML
        distance and of physher_amd.distances' p-distance, JC69 and K2P.  counts_only: only the tables -- no model needed, the
        bounds ignored.  Needs tip data and weights (and for distances the eigen system, frequencies and rates), no topology and
        no lengths; works on a rescaling engine and with any number of categories.  The engine is unchanged.  EngineError on
        engines that are not 4-state, tiled or sharded, and where a tip cell has an empty mask."""
        return self._pair_distances(self._lib.phyamd_pairwise_distances, 16, pairs, start, lower, upper, tolerance, max_iterations, want_derivatives, want_iterations,
                                    want_counts, counts_only, flags)

    def _pair_distances(self, call, classes, pairs, start, lower, upper, tolerance, max_iterations, want_derivatives, want_iterations, want_counts, counts_only, flags,
                        *more):
        """the arrays of the two distance calls: counts is [count, classes, classes]; more: the pointers behind counts"""
        pr = None
        if pairs is not None:
            pr = np.ascontiguousarray(pairs, dtype=np.int32)
            if pr.ndim != 2 or pr.shape[1] != 2:
                raise ValueError(f"pairs must be [count, 2] (got {pr.shape})")
        count = self.T * (self.T - 1) // 2 if pr is None else len(pr)
        st = None
        if start is not None:
            st = np.ascontiguousarray(start, dtype=np.float64)
            if st.shape != (count,):
                raise ValueError(f"start must be [{count}] (got {st.shape})")
        solve = not counts_only
        dist = np.empty(count) if solve else None
        lnl = np.empty(count) if solve else None
        d1 = np.empty(count) if solve and want_derivatives else None
        d2 = np.empty(count) if solve and want_derivatives else None
        it = np.empty(count, dtype=np.int32) if solve and want_iterations else None
        counts = np.empty((count, classes, classes)) if want_counts or counts_only else None
        opt = lambda a: None if a is None else _ptr(a)
        self._check(call(self._h, flags, count, opt(pr), opt(st), lower, upper, tolerance, max_iterations, opt(dist), opt(lnl), opt(d1), opt(d2), opt(it), opt(counts),
                         *more))
        return dist, lnl, d1, d2, it, counts

    def pairwise_distances_general(self, pairs=None, start=None, lower=1e-8, upper=10.0, tolerance=1e-8, max_iterations=100, want_derivatives=True,
                                   want_iterations=True, want_counts=False, counts_only=False, want_class_members=False, flags=0):
        """pairwise_distances for an engine of 20 states (proteins): (distances, lnl, d1, d2, iterations, counts [count, 32, 32],
        class_members [32] uint64); what is not wanted is None.  The same pairs, rule, start, bounds and outputs, with the tables
        over tip classes: counts[p, ci, cj] is the summed weight of the patterns where taxon i has class ci and taxon j class cj.
        A class is a state (0..19), unknown (20) or one of the engine's ambiguity sets (21 + q, numbered in the order in which
        set_tip_partials first met them): class_members[c] has bit s set where state s is a member of class c and is 0 for a
        class no set stands for, so it is what gives counts its meaning (physher_amd.distances: state_counts_general,
        p_distance_general, kimura_protein).  EngineError on engines that are not 20-state, tiled or sharded, and with more than
        11 recorded sets or a set without a member."""
        members = np.zeros(32, dtype=np.uint64) if want_class_members else None
        out = self._pair_distances(self._lib.phyamd_pairwise_distances_general, 32, pairs, start, lower, upper, tolerance, max_iterations, want_derivatives,
                                   want_iterations, want_counts, counts_only, flags, None if members is None else _ptr(members))
        return out + (members,)

    def distance_profile(self):
        """Of the last pairwise_distances or pairwise_distances_general: pairs, chunks (of pairs), segments (of the pattern axis),
        scratch_bytes, iterations (over all pairs), ms."""
        p = _lib.DistanceProfile()
        self._check(self._lib.phyamd_get_distance_profile(self._h, C.byref(p)))
        return {k: getattr(p, k) for k, _ in p._fields_}

    def placement_log_likelihoods(self, masks, pendant, split=0.5, want_lnl=True, want_best=True, flags=0):
        """Query sequences that are not among the engine's taxa, each placed on every edge of the engine's tree, on the device:
        (lnl [lengths, queries, N], best_node [lengths, queries] int32, best_lnl [lengths, queries]); what is not wanted is None.
        masks [queries, P] uint8 holds a 4-bit state mask 1..15 per query and pattern (bit s = state s, 15 a gap:
        physher_amd.placement.masks_from_states) OVER THE ENGINE'S OWN PATTERNS -- compress the reference and the queries jointly,
        or not at all.  pendant [lengths] > 0.  Column n places the query on the branch above node n: a new node takes n's place
        under n's parent, with the children n (branch split * t_n) and the query (branch pendant[i]), on a branch of
        (1 - split) * t_n; NaN in the root's column.  best_node is the smallest node id with the largest lnL, formed on the device:
        with want_lnl=False only the best edges come back.  lnL only, at those lengths; -inf in band where it underflows.
        The engine's tree, lengths and partials stay.  No fallback: EngineError where nni_log_likelihoods refuses, and on a sharded
        handle."""
        m = np.ascontiguousarray(masks, dtype=np.uint8)
        if m.ndim != 2 or m.shape[1] != self.P:
            raise ValueError(f"masks must be [queries, {self.P}] (got {m.shape})")
        pd = np.ascontiguousarray(np.atleast_1d(pendant), dtype=np.float64)
        if pd.ndim != 1:
            raise ValueError(f"pendant must be one-dimensional (got {pd.shape})")
        Q, L = m.shape[0], len(pd)
        lnl = np.empty((L, Q, self.N)) if want_lnl else None
        node = np.empty((L, Q), dtype=np.int32) if want_best else None
        best = np.empty((L, Q)) if want_best else None
        opt = lambda a: None if a is None else _ptr(a)
        self._check(self._lib.phyamd_placement_log_likelihoods(self._h, flags, Q, _ptr(m), L, _ptr(pd), split, opt(lnl), opt(node), opt(best)))
        return lnl, node, best

    def placement_log_likelihoods_general(self, codes, pendant, split=0.5, sets=(), want_lnl=True, want_best=True, flags=0):
        """placement_log_likelihoods for an engine of 20 states (proteins): the same definition, columns and outputs -- (lnl
        [lengths, queries, N], best_node [lengths, queries] int32, best_lnl [lengths, queries]); what is not wanted is None.
        codes [queries, P] uint8 holds a class code per query and pattern OVER THE ENGINE'S OWN PATTERNS: 0..19 a state, 20
        unknown, 21 + q the set sets[q] of THIS call (an integer with bit s set where state s is a member; at most 11 sets;
        physher_amd.placement.codes_from_protein makes both).  The engine is afterwards one with set_keep_partials(True) that has
        run the flags-0 gradient; its tree, lengths and models stay.  -inf in band where a lnL underflows.  No fallback: EngineError
        on engines that are not 20-state, have more than 8 categories, are rescaling, tiled or sharded, or hold explicit node
        matrices."""
        m = np.ascontiguousarray(codes, dtype=np.uint8)
        if m.ndim != 2 or m.shape[1] != self.P:
            raise ValueError(f"codes must be [queries, {self.P}] (got {m.shape})")
        pd = np.ascontiguousarray(np.atleast_1d(pendant), dtype=np.float64)
        if pd.ndim != 1:
            raise ValueError(f"pendant must be one-dimensional (got {pd.shape})")
        st = np.ascontiguousarray(sets, dtype=np.uint64)
        if st.ndim != 1:
            raise ValueError(f"sets must be one-dimensional (got {st.shape})")
        Q, L = m.shape[0], len(pd)
        lnl = np.empty((L, Q, self.N)) if want_lnl else None
        node = np.empty((L, Q), dtype=np.int32) if want_best else None
        best = np.empty((L, Q)) if want_best else None
        opt = lambda a: None if a is None else _ptr(a)
        self._check(self._lib.phyamd_placement_log_likelihoods_general(self._h, flags, Q, _ptr(m), len(st), _ptr(st) if len(st) else None, L, _ptr(pd), split, opt(lnl),
                                                                       opt(node), opt(best)))
        return lnl, node, best

    def placement_profile(self):
        """Of the last placement_log_likelihoods or placement_log_likelihoods_general: queries, lengths, edges, edge_chunks, query_chunks (per edge chunk), scratch_bytes,
        ms."""
        p = _lib.PlacementProfile()
        self._check(self._lib.phyamd_get_placement_profile(self._h, C.byref(p)))
        return {k: getattr(p, k) for k, _ in p._fields_}

    def placement_optimize(self, masks, candidates, pendant_start=None, split=0.5, branches=7, lower=1e-8, upper=10.0, tolerance=1e-8, max_iterations=100,
                           lnl_tolerance=1e-6, max_passes=50, want_initial_lnl=True, want_passes=True, flags=0):
        """The three branches around chosen placements optimised on the device: (lengths [count, 3], lnl [count], initial_lnl
        [count], passes [count] int32; the last two None when not wanted).  masks [queries, P] as placement_log_likelihoods takes
        them; candidates [count, 2] int32 holds (query, node) pairs (physher_amd.placement.top_candidates picks each query's best
        edges from a placement_log_likelihoods result; duplicates allowed).  lengths holds (distal, pendant, proximal): the branch
        of node n below the insertion point, the query's and the new node's, from the start (split * t_n, pendant_start[i] or 0.1,
        (1 - split) * t_n).  An entry is what optimize_branch_lengths returns for the placed tree with the branches of `branches`
        marked (bit 0 distal, bit 1 pendant, bit 2 proximal; 7: all three, 2: the pendant length alone): a pass visits them in
        that order by spr_optimize's rule and stop test; a branch that is not marked comes back as its start.  A lnL that is not
        finite ends an entry in band with passes negative.  The engine's tree, lengths and partials stay.  No fallback:
        EngineError where placement_log_likelihoods refuses."""
        m = np.ascontiguousarray(masks, dtype=np.uint8)
        if m.ndim != 2 or m.shape[1] != self.P:
            raise ValueError(f"masks must be [queries, {self.P}] (got {m.shape})")
        cd = np.ascontiguousarray(candidates, dtype=np.int32)
        if cd.ndim != 2 or cd.shape[1] != 2:
            raise ValueError(f"candidates must be [count, 2] (got {cd.shape})")
        count = len(cd)
        st = None
        if pendant_start is not None:
            st = np.ascontiguousarray(pendant_start, dtype=np.float64)
            if st.shape != (count,):
                raise ValueError(f"pendant_start must be [{count}] (got {st.shape})")
        lengths, lnl = np.empty((count, 3)), np.empty(count)
        lnl0 = np.empty(count) if want_initial_lnl else None
        passes = np.empty(count, dtype=np.int32) if want_passes else None
        opt = lambda a: None if a is None else _ptr(a)
        self._check(self._lib.phyamd_placement_optimize(self._h, flags, m.shape[0], _ptr(m), count, _ptr(cd), opt(st), split, branches, lower, upper, tolerance,
                                                        max_iterations, lnl_tolerance, max_passes, _ptr(lengths), _ptr(lnl), opt(lnl0), opt(passes)))
        return lengths, lnl, lnl0, passes

    def placement_optimize_general(self, codes, candidates, sets=None, pendant_start=None, split=0.5, branches=7, lower=1e-8, upper=10.0, tolerance=1e-8,
                                   max_iterations=100, lnl_tolerance=1e-6, max_passes=50, want_initial_lnl=True, want_passes=True, flags=0):
        """placement_optimize for an engine of 20 states (proteins): the same rule, arguments and outputs -- (lengths [count, 3],
        lnl [count], initial_lnl [count], passes [count] int32; the last two None when not wanted) -- with class codes for the
        queries.  codes [queries, P] uint8 and sets are placement_log_likelihoods_general's: 0..19 a state, 20 unknown, 21 + q the
        set sets[q] of THIS call (at most 11).  candidates [count, 2] int32 holds (query, node) pairs
        (physher_amd.placement.top_candidates picks them from a placement_log_likelihoods_general result;
        physher_amd.placement.likelihood_weight_ratios(lnl, queries) takes the sparse result).  The engine is afterwards one with
        set_keep_partials(True) that has run the flags-0 gradient; its tree, lengths and models stay.  A lnL that is not finite ends
        an entry in band with passes negative.  No fallback: EngineError where placement_log_likelihoods_general refuses."""
        m = np.ascontiguousarray(codes, dtype=np.uint8)
        if m.ndim != 2 or m.shape[1] != self.P:
            raise ValueError(f"codes must be [queries, {self.P}] (got {m.shape})")
        cd = np.ascontiguousarray(candidates, dtype=np.int32)
        if cd.ndim != 2 or cd.shape[1] != 2:
            raise ValueError(f"candidates must be [count, 2] (got {cd.shape})")
        sw = np.ascontiguousarray(() if sets is None else sets, dtype=np.uint64)
        if sw.ndim != 1:
            raise ValueError(f"sets must be one-dimensional (got {sw.shape})")
        count = len(cd)
        st = None
        if pendant_start is not None:
            st = np.ascontiguousarray(pendant_start, dtype=np.float64)
            if st.shape != (count,):
                raise ValueError(f"pendant_start must be [{count}] (got {st.shape})")
        lengths, lnl = np.empty((count, 3)), np.empty(count)
        lnl0 = np.empty(count) if want_initial_lnl else None
        passes = np.empty(count, dtype=np.int32) if want_passes else None
        opt = lambda a: None if a is None else _ptr(a)
        self._check(self._lib.phyamd_placement_optimize_general(self._h, flags, m.shape[0], _ptr(m), len(sw), _ptr(sw) if len(sw) else None, count, _ptr(cd), opt(st), split,
                                                                branches, lower, upper, tolerance, max_iterations, lnl_tolerance, max_passes, _ptr(lengths), _ptr(lnl),
                                                                opt(lnl0), opt(passes)))
        return lengths, lnl, lnl0, passes

    def placement_optimize_profile(self):
        """Of the last placement_optimize or placement_optimize_general: candidates, edges (distinct among them), chunks (of candidates), visits and iterations
        (over all candidates), scratch_bytes, ms."""
        p = _lib.PlacementOptimizeProfile()
        self._check(self._lib.phyamd_get_placement_optimize_profile(self._h, C.byref(p)))
        return {k: getattr(p, k) for k, _ in p._fields_}

    def state_posteriors(self, nodes=None, want_posteriors=True, want_states=True):
        """Marginal ancestral reconstruction on the device: (posteriors [count, P, S] float64, states [count, P] uint8), either None
        when not wanted.  Row i is node nodes[i] (None: every node, row i is node i; tips and the root included, duplicates
        allowed): the posterior of its state per pattern given all the data, and the most probable state (the smallest on a
        tie).  An observed tip cell is one-hot; a gap cell holds the imputed state.  Evaluates whatever is pending; the engine
        is afterwards one with set_keep_partials(True) that has run gradient().  NaN / 255 where lnL is not finite."""
        if not (want_posteriors or want_states):
            raise ValueError("want_posteriors and want_states are both False")
        nd = None
        if nodes is not None:
            nd = np.ascontiguousarray(nodes, dtype=np.int32)
            if nd.ndim != 1:
                raise ValueError(f"nodes must be one-dimensional (got {nd.shape})")
        count = self.N if nd is None else len(nd)
        post = np.empty((count, self.P, self.S)) if want_posteriors else None
        states = np.empty((count, self.P), dtype=np.uint8) if want_states else None
        self._check(self._lib.phyamd_state_posteriors(self._h, 0, count, None if nd is None else _ptr(nd),
                                                      None if post is None else _ptr(post), None if states is None else _ptr(states)))
        return post, states

    def site_rate_posteriors(self):
        """(R [P, C], mean_rate [P]): the posterior of each pattern's rate category and its mean rate (sum_c R[k, c] r_c)."""
        R = np.empty((self.P, self.C))
        mean = np.empty(self.P)
        self._check(self._lib.phyamd_site_rate_posteriors(self._h, _ptr(R), _ptr(mean)))
        return R, mean

    def branch_hessian(self, flags=0, want_gradient=True):
        """(lnL, g [N] or None, H [N, N]): the full branch-length Hessian of lnL, H[a, b] = d2 lnL / dt_a dt_b for every pair of
        branches (symmetric; the root's row and column 0; diag(H) is branch_hessian_diagonal's d2), and g[a] = d lnL / dt_a.
        4 states, at most 8 categories, an engine that is not rescaling.  Evaluates whatever is pending; the engine is afterwards
        one with set_keep_partials(True) that has run gradient().  All NaN where lnL is not finite."""
        v = C.c_double()
        g = np.empty(self.N) if want_gradient else None
        H = np.empty((self.N, self.N))
        self._check(self._lib.phyamd_branch_hessian(self._h, flags, C.byref(v), None if g is None else _ptr(g), _ptr(H)))
        return v.value, g, H

    def hessian_profile(self):
        """Of the last branch_hessian: chunks (of patterns), pairs (unordered, a <= b), scratch_bytes, ms."""
        p = _lib.HessianProfile()
        self._check(self._lib.phyamd_get_hessian_profile(self._h, C.byref(p)))
        return {k: getattr(p, k) for k, _ in p._fields_}

    def general_profile(self):
        """How the 20 / 60 / 61-state kernels of the last post-order and the last pre-order pass were launched: lower_family (0: one
        launch per level, 1: the walk, -1: none yet), lower_slots / upper_slots (resident workgroups the launches were sized by),
        lower_levels / upper_levels, the fewest and the most tiles per wave over those levels (lower_tiles_min / _max, upper_tiles_min
        / _max), walk_units and walk_workgroups, upper_hess (1: the pass of branch_hessian_diagonal).  EngineError at 4 states."""
        p = _lib.GeneralProfile()
        self._check(self._lib.phyamd_get_general_profile(self._h, C.byref(p)))
        return {k: getattr(p, k) for k, _ in p._fields_}

    def pass_profile(self):
        """Which 4-state kernel the last post-order and the last pre-order pass launched, every field -1 before the first pass of
        its kind: lower_family / upper_family (0: the level kernels, 1: the table-gather walks, 2: the streamed walks), lower_form
        (0: Reference, 1: Carried, 2: CarriedExp2), lower_scale / upper_scale (0: none, 1: the reference's, 2: powers of two),
        lower_ambiguous / upper_ambiguous, lower_incremental, lower_waves / upper_waves, lower_ppt, upper_tf, upper_fold,
        upper_compat, upper_params, upper_catblk, upper_pair_ops.  EngineError at 20 / 60 / 61 states."""
        p = _lib.PassProfile()
        self._check(self._lib.phyamd_get_pass_profile(self._h, C.byref(p)))
        return {k: getattr(p, k) for k, _ in p._fields_}

    def gradient_batch_weights(self, weights, branch_lengths=None, flags=0, want_gradient=True):
        """lnL and the per-category branch gradient for B pattern-weight vectors [B, P] at once -- bootstrap or jackknife replicates
        (physher_amd.resampling), RELL reweighting, site minibatches: (lnl [B], g [B, N, C] or None).  Item b is what
        set_pattern_weights(weights[b]), set_branch_lengths(branch_lengths[b]) if branch_lengths [B, N] is given, and
        gradient(flags) return; the engine's own weights and lengths stay.  Weights are finite and >= 0; a zero drops the pattern.
        Without branch_lengths one walk of the tree serves every item."""
        w = _f64(weights)
        if w.ndim != 2 or w.shape[1] != self.P or w.shape[0] < 1:
            raise ValueError(f"weights must be [B >= 1, {self.P}] (got {w.shape})")
        count = w.shape[0]
        bl = None
        if branch_lengths is not None:
            bl = _f64(branch_lengths)
            if bl.shape != (count, self.N):
                raise ValueError(f"branch_lengths must be [{count}, {self.N}] (got {bl.shape})")
        lnl = np.empty(count)
        g = np.empty((count, self.N, self.C)) if want_gradient else None
        self._check(self._lib.phyamd_gradient_batch_weights(self._h, flags, count, _ptr(w), None if bl is None else _ptr(bl), _ptr(lnl),
                                                            None if g is None else _ptr(g)))
        return lnl, g

    def weight_batch_profile(self):
        """Of the last gradient_batch_weights: items_fast / items_sequential, item_chunks, pattern_chunks, walks, scratch_bytes, ms."""
        p = _lib.WeightBatchProfile()
        self._check(self._lib.phyamd_get_weight_batch_profile(self._h, C.byref(p)))
        return {k: getattr(p, k) for k, _ in p._fields_}

    def pattern_log_likelihoods_trees(self, left, right, roots, branch_lengths, replicate_weights=None, want_patterns=True, flags=0):
        """The per-pattern log-likelihoods of B trees on this engine's data and models at once, and RELL replicates of them:
        (lnl [B], pattern_lnl [B, P] or None, replicate_lnl [R, B] or None).  left, right [B, N], roots [B] and branch_lengths
        [B, N] as gradient_batch_trees takes them; left = right = roots = None: every item is this engine's tree.  Row b is what
        pattern_log_likelihoods() returns after set_topology + set_branch_lengths + log_likelihood on item b, lnl[b] its sum under
        the engine's weights, replicate_lnl[r, b] its sum under replicate_weights[r] ([R, P], finite and >= 0:
        physher_amd.resampling).  An item whose lnL is not finite has an all-NaN replicate column.  This engine's own tree, lengths,
        weights and partials stay.  No item-by-item fallback: EngineError where gradient_batch_trees refuses."""
        bl = _f64(branch_lengths)
        if bl.ndim != 2 or bl.shape[1] != self.N or bl.shape[0] < 1:
            raise ValueError(f"branch_lengths must be [B >= 1, {self.N}] (got {bl.shape})")
        count = bl.shape[0]
        given = [x is not None for x in (left, right, roots)]
        l = r = ro = None
        if all(given):
            l = np.ascontiguousarray(left, dtype=np.int32)
            r = np.ascontiguousarray(right, dtype=np.int32)
            ro = np.ascontiguousarray(roots, dtype=np.int32)
            if l.shape != bl.shape or r.shape != bl.shape or ro.shape != (count,):
                raise ValueError(f"left, right: {bl.shape} and roots: ({count},), got {l.shape}, {r.shape}, {ro.shape}")
        elif any(given):
            raise ValueError("left, right and roots are given together, or all three are None (the engine's tree)")
        w = None
        if replicate_weights is not None:
            w = _f64(replicate_weights)
            if w.ndim != 2 or w.shape[1] != self.P or w.shape[0] < 1:
                raise ValueError(f"replicate_weights must be [R >= 1, {self.P}] (got {w.shape})")
        lnl = np.empty(count)
        rows = np.empty((count, self.P)) if want_patterns else None
        rep = np.empty((w.shape[0], count)) if w is not None else None
        opt = lambda a: None if a is None else _ptr(a)
        self._check(self._lib.phyamd_pattern_log_likelihoods_trees(self._h, flags, count, opt(l), opt(r), opt(ro), _ptr(bl), _ptr(lnl), opt(rows),
                                                                   0 if w is None else w.shape[0], opt(w), opt(rep)))
        return lnl, rows, rep

    def site_lnl_profile(self):
        """Of the last pattern_log_likelihoods_trees: items, chunks (of items), replicate_chunks (per chunk of items), lower_slots (the
        most partials an item parked per pattern and category), scratch_bytes, ms."""
        p = _lib.SiteLnlProfile()
        self._check(self._lib.phyamd_get_site_lnl_profile(self._h, C.byref(p)))
        return {k: getattr(p, k) for k, _ in p._fields_}

    def store(self):
        """Remember the current (evaluated) state: parameters, lnL and partials (MCMC store)."""
        self._check(self._lib.phyamd_store(self._h))
        self._stored_lengths = None if self._lengths is None else self._lengths.copy()

    def restore(self):
        """Back to the stored state without recomputing the tree (MCMC reject)."""
        self._check(self._lib.phyamd_restore(self._h))
        self._lengths = None if self._stored_lengths is None else self._stored_lengths.copy()

    def synchronize(self):
        self._check(self._lib.phyamd_synchronize(self._h))

    # --- inspection
    def pattern_log_likelihoods(self):
        a = np.empty(self.P)
        self._check(self._lib.phyamd_get_pattern_log_likelihoods(self._h, _ptr(a)))
        return a

    def partials(self, node, upper=False):
        a = np.empty((self.C, self.P, self.S))
        self._check(self._lib.phyamd_get_partials(self._h, node, int(upper), _ptr(a)))
        return a

    def node_matrices(self, node, derivative=False):
        a = np.empty((self.C, self.S, self.S))
        self._check(self._lib.phyamd_get_node_matrices(self._h, node, int(derivative), _ptr(a)))
        return a

    @property
    def rescaling(self):
        return bool(self._lib.phyamd_is_rescaling(self._h))

    def set_rescaling(self, policy):
        self._check(self._lib.phyamd_set_rescaling(self._h, int(policy)))

    def set_keep_partials(self, on=True):
        self._check(self._lib.phyamd_set_keep_partials(self._h, int(on)))

    def set_reduction_levels(self, levels):
        """3 (default): this engine sums its pattern blocks over eight bisection segments; an engine holding 1 / 2^k of a larger
        pattern list cut by sharding.shard_range runs with 3 - k (see include/physher_amd.h)."""
        self._check(self._lib.phyamd_set_reduction_levels(self._h, int(levels)))

    def set_profiling(self, on=True):
        self._check(self._lib.phyamd_set_profiling(self._h, int(on)))

    def profile(self):
        p = _lib.Profile()
        self._check(self._lib.phyamd_get_profile(self._h, C.byref(p)))
        return {k: getattr(p, k) for k, _ in p._fields_}
