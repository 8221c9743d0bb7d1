/*
 * physher_amd.h -- C ABI of the MI355X (gfx950) tree-likelihood engine.
 *
 * This is the drop-in boundary for physher's Felsenstein-pruning hot path.  Every entry point is
 * plain C (pointers + sizes, no C++/torch types) and replaces one piece of what
 * `struct _SingleTreeLikelihood` and its five kernel function pointers do on the CPU in the
 * reference (src/phyc/treelikelihood.h:46-124).  The reference-side binding a maintainer would add
 * is shown in INTEGRATION.md.
 *
 * Conventions shared with the reference:
 *   - node ids: tips 0..T-1, internal nodes T..2T-2, children before parents not required
 *     (src/phyc/tree.c:183-224); the root may be any internal node.
 *   - host-side array layouts are the reference's: partials [C][P][S] (state fastest,
 *     treelikelihood.c:1028), matrices [C][S][S] row-major P[parent state][child state]
 *     (substmodel.c:547-555), tip states uint8, code >= S = unknown/gap (sitepattern.h:68-82).
 *   - numerical trouble is reported in-band like the reference does: NaN/inf lnL and an all-NaN
 *     gradient (treelikelihood.c:327-332, 1489-1519).  API misuse and device errors return a
 *     negative PHYAMD_E* code; phyamd_last_error() holds the message.  Nothing here calls exit().
 *
 * All functions are single-caller per engine (the reference's objects are not thread-safe either,
 * SURVEY.md section 8b); different engines may be used from different threads.
 */
#ifndef PHYSHER_AMD_H
#define PHYSHER_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct phyamd_engine phyamd_engine;

enum {
	PHYAMD_OK = 0,
	PHYAMD_EINVAL = -1,   /* bad argument / call order */
	PHYAMD_EDEVICE = -2,  /* HIP runtime error (message in phyamd_last_error) */
	PHYAMD_ENOMEM = -3,   /* device memory exhausted */
	PHYAMD_EUNSUPPORTED = -4
};

/* rescaling policy: SingleTreeLikelihood_use_rescaling + the lazy switch of treelikelihood.c:1496-1519 */
enum { PHYAMD_RESCALE_NEVER = 0, PHYAMD_RESCALE_ALWAYS = 1, PHYAMD_RESCALE_AUTO = 2 };

/* gradient flags */
enum {
	/* Multiply the root frequencies into the upper partials of the root's children and drop them from
	 * the final state sum: the reference's `include_root_freqs = true` mode (treelikelihood.c:241,
	 * 2147-2153), which it uses when no substitution-model gradient is requested.  That mode is only
	 * exact for uniform frequencies; the default (0) is the reference's `include_root_freqs = false`
	 * arithmetic (treelikelihood.c:2715-2751), exact for every reversible model. */
	PHYAMD_GRAD_FOLD_ROOT_FREQS = 1,
	/* Under rescaling divide each category's derivative by that category's own site likelihood, as
	 * treelikelihood.c:2851-2870 does, instead of by the mixture likelihood. */
	PHYAMD_GRAD_COMPAT_SCALED = 2
};

typedef struct {
	int32_t tip_count;      /* T */
	int32_t pattern_count;  /* P (this engine's shard of the compressed patterns) */
	int32_t state_count;    /* S: 4 (nucleotides), 20 (amino acids), 60 / 61 (codons); others -> PHYAMD_EUNSUPPORTED */
	int32_t category_count; /* C */
	int32_t device;         /* HIP device ordinal; -1 = current device */
	int32_t rescale;        /* PHYAMD_RESCALE_* (all state counts) */
	int64_t max_device_bytes; /* 0 = 92 % of the device memory that is free when the engine is created.  Below the (estimated)
	                             working set of all patterns the engine processes them in
	                             tiles through ONE set of partial arrays: tip data, weights and per-pattern lnL of all tiles
	                             stay resident, per-tile sums are added in tile order (phyamd_profile.tiles tells how many).
	                             lnL, gradients and parameter gradients work as usual; calls that need resident partials
	                             (phyamd_get_partials, phyamd_set_keep_partials, phyamd_store, phyamd_branch_log_likelihood)
	                             return PHYAMD_EUNSUPPORTED, and every evaluation recomputes every
	                             tile.  PHYAMD_ENOMEM if even a 256-pattern tile does not fit. */
	void *stream;           /* hipStream_t to run on, NULL = engine-owned stream */
} phyamd_config;

/* --- life cycle: new_SingleTreeLikelihood / free_SingleTreeLikelihood (treelikelihood.c:1007-1185) --- */
int phyamd_create(const phyamd_config *cfg, phyamd_engine **out);
/* The same engine with its site patterns sharded over `device_count` GPUs of this node, inside ONE process: shard s
 * is a complete engine on device_ids[s] (NULL: devices 0 .. device_count-1) that owns the contiguous pattern range
 * [s P / n, (s+1) P / n); tree, branch lengths, eigen system and rates are replicated to every shard, per-pattern arguments
 * (tip data, weights, per-pattern lnL, partials) are sliced, and every evaluation runs on all shards at once (one host thread per
 * shard) and returns the per-shard sums added in shard order -- lnL, the [node][category] gradient, parameter sums, root terms:
 * the "single all-reduce of the per-block lnL and gradient vector", done on the host where the caller wants the 64 KB anyway.
 * Every other call of this header works on the handle unchanged, except the *_device evaluations (their output lives on one
 * device: PHYAMD_EUNSUPPORTED for device_count > 1; the one-process-per-GPU form of the same sharding -- bench.py under
 * torchrun -- is what uses them, with one RCCL all-reduce).  cfg->device is ignored, cfg->stream must be NULL,
 * cfg->max_device_bytes applies per shard.  The same device may be listed more than once. */
int phyamd_create_sharded(const phyamd_config *cfg, int32_t device_count, const int32_t *device_ids, phyamd_engine **out);
/* number of shards behind a handle (1 for phyamd_create) */
int phyamd_shard_count(phyamd_engine *e);
void phyamd_destroy(phyamd_engine *e);
const char *phyamd_last_error(void);
/* version of this ABI (bumped on any signature change) */
int phyamd_abi_version(void);

/* --- data: sp->patterns / sp->weights / tlk->partials of tips (sitepattern.h:68-82, treelikelihood.c:1106-1117) --- */
/* states[P] codes of one tip ("tipstates": true semantics; code >= S => all ones). */
int phyamd_set_tip_states(phyamd_engine *e, int tip, const uint8_t *states);
/* partials[P][S] of one tip ("tipstates": false semantics), replicated over categories like treelikelihood.c:1111-1114.
 * Built for the 0/1 vectors every data type of the reference produces (datatype.c:212-240, datatype.h:26-66): one state,
 * all states, or a set of states (nucleotide ambiguity codes; named sets of a general data type -- at most 255 - S
 * distinct sets per engine for 20 / 60 / 61 states); other values are refused with PHYAMD_EUNSUPPORTED. */
int phyamd_set_tip_partials(phyamd_engine *e, int tip, const double *partials);
int phyamd_set_pattern_weights(phyamd_engine *e, const double *weights /* [P] */);

/* new_SitePattern (sitepattern.c:186-251) on the device: de-duplicates the columns of an alignment and returns them in the
 * reference's order -- the iteration order of its chained hash table (hashtable.c: 193 buckets, growth through the prime
 * table at load 0.65, chains prepended and reversed by growth), rebuilt from per-column hashes and first-occurrence ranks
 * with radix sorts instead of T*L sequential insertions.  Engine-independent and synchronous.
 *   rows[taxon_count]: host pointers to site_count bytes each (state codes; or raw one-byte symbols when symbol_codes is
 *   given: symbol_codes[256] maps a symbol to its state code, datatype.c:55-89);
 *   patterns: host buffer of taxon_count * site_count bytes, filled as [taxon][pattern] with *pattern_count columns;
 *   weights: host buffer of site_count doubles.
 * PHYAMD_EUNSUPPORTED if two different columns collide in both 32-bit hashes (nothing is folded: compress on the host). */
int phyamd_compress_patterns(int device /* -1: current */, int32_t taxon_count, int64_t site_count, const uint8_t *const *rows,
                             const uint8_t *symbol_codes /* [256] or NULL */, int32_t *pattern_count, uint8_t *patterns, double *weights);

/* --- tree: Tree/Node ids, Node_left/right (tree.c:183-224) ---
 * Tips are 0..T-1, internal ids T..2T-2 in any order, any internal node may be the root.  May be called again on an engine that
 * has evaluated: every partial is dropped, the schedule is rebuilt, a stored state (phyamd_store) is forgotten.  Branch lengths go
 * by node id and stay: the engine keeps the vector of the last phyamd_set_branch_lengths / phyamd_set_branch_length as the caller
 * sent it, the entry at the root's id included, so after a call that moves the root to another id the old root's id has the length
 * that was sent for it (not 0), and the new root's entry is the one ignored.  Explicit node matrices stay with their ids too.
 * A refused call (PHYAMD_EINVAL: not a binary tree over these ids) leaves the engine on the tree it had. */
int phyamd_set_topology(phyamd_engine *e, const int32_t *left, const int32_t *right /* [2T-1], -1 for tips */, int root);
/* branch length per node id, already multiplied by the clock rate for time trees
 * (treelikelihood.c:1652-1663); the root entry is ignored, and kept for a later change of root (phyamd_set_topology). */
int phyamd_set_branch_lengths(phyamd_engine *e, const double *lengths /* [2T-1] */);

/* One branch: Node_set_distance + update_nodes[node] = true (treelikelihood.c:73-92).  The next evaluation recomputes only
 * the stored partials on the path from `node` to the root (_calculate_partials' dirty walk, treelikelihood.c:1645-1734)
 * instead of the whole tree; every other setter (and phyamd_set_branch_lengths) implies a full recomputation. */
int phyamd_set_branch_length(phyamd_engine *e, int node, double length);
/* SingleTreeLikelihood_update_all_nodes (treelikelihood.c:1737-1771): force the next evaluation to recompute every node. */
int phyamd_update_all_nodes(phyamd_engine *e);

/* MCMC store / restore (_singleTreeLikelihood_store, _treelikelihood_handle_restore: treelikelihood.c:116-161; the
 * current/stored index pairs of allocate_storage, :947-1005).  phyamd_store evaluates anything pending and remembers the
 * engine's state: branch lengths, eigen system, frequencies, category rates and proportions, lnL, and the stored partials --
 * the first call gives every stored node a second slot (lower-partial memory doubles); evaluations after a store never
 * write the slot the stored state lives in.  phyamd_restore brings that state back without recomputing the tree: nodes
 * point at their stored slots again and only the root is re-integrated on the next evaluation.  The caller does NOT send
 * the old parameters again after a restore.  Not covered: topology, tip data, pattern weights, explicit node matrices
 * (changing the first three drops the stored state; restore then returns PHYAMD_EINVAL).  If slots were reassigned in between
 * (phyamd_set_keep_partials, the lazy rescaling switch) the restored parameters are simply recomputed in full. */
int phyamd_store(phyamd_engine *e);
int phyamd_restore(phyamd_engine *e);

/* --- models: SubstitutionModel eigen system + frequencies, SiteModel rates/proportions --- */
/* eval[S], evec[S][S], ivec[S][S]: m->eigendcmp after update_eigen_system (substmodel.c:1092-1115);
 * P(t) = |evec diag(exp(eval t)) ivec| is formed on the device (substmodel.c:518-557). */
int phyamd_set_eigen(phyamd_engine *e, const double *eval, const double *evec, const double *ivec);
int phyamd_set_frequencies(phyamd_engine *e, const double *freqs /* [S] */);
/* sm->get_rate(c) (includes mu) and sm->get_proportions (sitemodel.c:544-549) */
int phyamd_set_category_rates(phyamd_engine *e, const double *rates /* [C] */, const double *proportions /* [C] */);
/* Optional: explicit matrices [C][S][S] for one node (closed-form models: jc69.c:73-79, hky.c:230-273).
 * Cleared by phyamd_set_eigen. */
int phyamd_set_node_matrices(phyamd_engine *e, int node, const double *matrices);
/* The same for every node at once: matrices [2T-1][C][S][S] by node id (the root's entry is ignored), one upload.  What
 * _calculate_partials does per node with m->p_t (treelikelihood.c:1671-1691) when the caller wants the model's own closed-form
 * arithmetic bit for bit. */
int phyamd_set_matrices(phyamd_engine *e, const double *matrices);
/* Rate matrix Q [S][S] (rows sum to 0, normalised like substmodel.c:1135-1143).  The gradient kernels use
 * (dP/dt) p = Q (P p) instead of a second matrix per branch (the reference's dp_dt, substmodel.c:695-723, is the
 * same product).  phyamd_set_eigen derives Q itself; only explicit-matrix users need this call. */
int phyamd_set_rate_matrix(phyamd_engine *e, const double *Q);

/* --- evaluation --- */
/* lnL = sum_k w_k log L_k: _calculate_simple (treelikelihood.c:1454-1526). */
int phyamd_log_likelihood(phyamd_engine *e, double *lnl);
/* lnL and the per-category branch gradient g[node][c] = sum_k w_k (dL_kc/dt_node) / L_k:
 * update_upper_partials + gradient_cat_branch_lengths (treelikelihood.c:2129-2161, 2793-2941).
 * cat_gradient [2T-1][C]; the root row is 0.  NaN/inf lnL => all-NaN gradient. */
int phyamd_gradient(phyamd_engine *e, int flags, double *lnl, double *cat_gradient);
/* Same, then the epilogue gradient_branch_length_from_cat_inplace (treelikelihood.c:3129-3143):
 * branch_gradient[node] = sum_c g[node][c] w_c r_c  (r_c WITHOUT mu: pass them here).  [2T-1]. */
int phyamd_branch_gradient(phyamd_engine *e, int flags, const double *rates_without_mu /* [C] or NULL */, double *lnl,
                           double *branch_gradient);
/* lnL alone, left on the device (device_out[0]) on the engine's stream: the post-order pass without a host round trip
 * (with PHYAMD_RESCALE_AUTO an unscaled engine still reads lnL back once to test for +-inf, treelikelihood.c:1496-1519). */
int phyamd_log_likelihood_device(phyamd_engine *e, double *device_out);
/* Device-resident result for multi-GPU sharding: writes [lnL, g[0][0..C-1], g[1][..], ...]
 * (1 + (2T-1)*C doubles) to `device_out` on the engine's stream, no host synchronisation. */
int phyamd_gradient_device(phyamd_engine *e, int flags, double *device_out);
/* After an evaluation (rescaled or not): sum_k (w_k / L_k) sum_i pi_i ( p_root[cat 0] - mean of p_root[cat >= 1] ), the only part
 * of the +I site-model gradient that needs O(P) data (gradient_pinv_sitemodel / gradient_pinv_W_sitemodel,
 * treelikelihood.c:2943-3008); the rest of that gradient is O(N C) host arithmetic on phyamd_gradient's output. */
int phyamd_root_invariant_term(phyamd_engine *e, double *out);

/* --- substitution-model gradient: calculate_dlnl_dQ (treelikelihood.c:2337-2583) --- */
#define PHYAMD_MAX_PARAMETERS 2048 /* a 61-state symmetric model has 1830 rates + 61 frequencies */
/* dQ [count][S][S]: derivative of the (normalised) rate matrix with respect to each parameter, what the reference's
 * m->dQ holds after _gtr_dQdp / _hky_dQdp / _general_dQdp (gtr.c:256-326, hky.c:493-541, gensubst.c:216-279).  The engine
 * forms dP/dtheta = U ((U^-1 dQ U) o F(t)) U^-1 per branch and category itself (dPdp_with_dQdp, substmodel.c:469-489).
 * Needs phyamd_set_eigen; count = 0 clears. */
int phyamd_set_rate_matrix_derivatives(phyamd_engine *e, int count, const double *dQ);
/* One post-order + one pre-order pass giving lnL, the per-category branch gradient (cat_gradient may be NULL) and
 *   parameter_gradient[th] = sum_k (w_k / L_k) sum_branches sum_c w_c sum_i pi_i u_i (dP_th p)_i
 * i.e. the branch sum of calculate_dlnl_dQ for all parameters at once (the reference re-walks the tree per parameter).
 * For a frequency parameter add dpi_f/dtheta * phyamd_root_frequency_term()[f] (treelikelihood.c:2370-2401).
 * Works with rescaling; PHYAMD_GRAD_FOLD_ROOT_FREQS is refused (the reference clears include_root_freqs here).
 * 4 states: fused into the pre-order pass.  20 / 60 / 61 states (general K-state matrices of discrete-trait models,
 * dPdp_with_dQdp_general, gensubst.c:284-323): separate kernels on the stored partials -- the first call switches the
 * engine to phyamd_set_keep_partials(1). */
int phyamd_parameter_gradient(phyamd_engine *e, int flags, double *lnl, double *cat_gradient, double *parameter_gradient);
/* Device-resident form for multi-GPU sharding, like phyamd_gradient_device: writes
 * [lnL | g[node][cat] | parameter_gradient[count] | root frequency term[S]]  (1 + (2T-1)*C + count + S doubles, all of them
 * sums over this engine's patterns) to `device_out` on the engine's stream, no host synchronisation. */
int phyamd_parameter_gradient_device(phyamd_engine *e, int flags, double *device_out);
/* After an evaluation: out[f] = sum_k w_k (sum_c w_c p_root[c][k][f]) / (sum_i pi_i sum_c w_c p_root[c][k][i]), f < S:
 * d lnL / d pi_f through the root frequencies alone. */
int phyamd_root_frequency_term(phyamd_engine *e, double *out /* [S] */);
/* The optimiser's fast path (_calculate_uppper / dlnldt_uppper / d2lnldt2_uppper, treelikelihood.c:2196-2335, 2592-2686):
 * lnL and its first two derivatives with respect to the length of ONE branch, evaluated at a TRIAL length from the upper
 * and lower partials that meet on the branch -- O(patterns) work per trial instead of a tree sweep.  Every state count,
 * rescaled evaluations included (their stored partials are anchored on the per-pattern lnL they belong to).
 * The upper partial comes from the last phyamd_gradient if phyamd_set_keep_partials(1) left it resident; otherwise pending
 * changes are evaluated first (single changed branches: only their paths to the root) and the one upper the branch needs is
 * rebuilt by a walk down its path from the root (node_upper / update_upper of the reference, treelikelihood.c:1737-1771) and
 * kept until partials change again -- so the reference's loop "trials of one branch, accept (phyamd_set_branch_length), next
 * branch" (optimizer.c:116-150) costs a path per branch, not a sweep.  Any of lnl / d1 / d2 may be NULL.  The engine's branch
 * lengths are not changed by this call. */
int phyamd_branch_log_likelihood(phyamd_engine *e, int node, double length, double *lnl, double *d1, double *d2);
/* lnL, and for every node n != root the exact first and second derivative of lnL in t_n:
 *   d1[n] = sum_k w_k L'_k / L_k,   d2[n] = sum_k w_k (L''_k / L_k - (L'_k / L_k)^2),
 *   L'_k = sum_c w_c r_c sum_i pi_i u_i (Q P_c p)_i,   L''_k = sum_c w_c r_c^2 sum_i pi_i u_i (Q Q P_c p)_i
 * with r_c the category rates the matrices were built with (P_c = exp(Q t r_c)), u the branch's upper partial and p its lower.
 * This is _singleTreeLikelihood_d2logP / d2lnldt2_uppper (treelikelihood.c:469-530, 2267-2335) for all branches at once: row n
 * is what phyamd_branch_log_likelihood(e, n, t_n, ...) returns as d1 and d2, from ONE post-order and ONE pre-order pass instead
 * of a path walk per branch -- the diagonal physher's Laplace approximations (laplace.c:102, 207, 347, 489, 579, 717), its
 * Hessian (hessian.c:14-25) and Newton-type branch optimisers ask for.  Root row 0 (no row is zeroed for unrooted trees: that
 * rule is the caller's epilogue, as for phyamd_gradient).  [2T-1] each; d1 may be NULL.  flags: 0 (others reserved, refused).
 * NaN/inf lnL => all-NaN d1, d2.  Branch lengths are not changed, and later evaluations give what they would have given
 * without this call.  Every state count, rescaling policy, tiled patterns and shards.  Needs the eigen system; refused with
 * PHYAMD_EUNSUPPORTED: explicit node matrices (Q P, Q Q P are the derivatives of exp(Q t r) only), more than 8 categories with
 * 4 states, a zero frequency with 20 / 60 / 61 states. */
int phyamd_branch_hessian_diagonal(phyamd_engine *e, int flags, double *lnl, double *d1, double *d2);
/* device-resident form for sharding: [lnL | d1[2T-1] | d2[2T-1]], sums over this engine's patterns, no host sync */
int phyamd_branch_hessian_diagonal_device(phyamd_engine *e, int flags, double *device_out);
/* lnL and the per-category branch gradient for `count` branch-length vectors on the engine's tree, data and models.
 * branch_lengths [count][2T-1] by node id (root entries ignored); lnl [count]; cat_gradient [count][2T-1][C], root rows 0,
 * or NULL for lnL only (post-order work only).  Item b equals what phyamd_set_branch_lengths(item b) + phyamd_gradient(flags)
 * returns.  The engine's own branch lengths are unchanged afterwards.  NaN/inf lnL of an item => that item's gradient all NaN.
 * The call is defined as "evaluate the items one by one through the ordinary path, then put the engine's lengths back", so it
 * works on every engine configuration; where the conditions below hold the items run together instead -- one launch walks every
 * item's tree, a workgroup per (item, 64 patterns), with no floating-point atomics: an item's result does not depend on `count`,
 * on its position in the batch or on how the batch was cut into chunks, bit for bit.  That fast path takes: 4 states, at most 8
 * categories, an engine that is not rescaling (PHYAMD_RESCALE_NEVER: an underflowing item reports -inf / NaN in-band like a
 * single evaluation; PHYAMD_RESCALE_AUTO: an item whose lnL is not finite is evaluated again one by one, which may switch the
 * engine to rescaling as any evaluation does), untiled patterns and at most 8192 of them per shard (above that one evaluation
 * fills the card and the loop is faster), no tip cell with an empty state mask, flags 0 or
 * PHYAMD_GRAD_FOLD_ROOT_FREQS, and scratch for at least one item within the memory cap (a batch that does not fit as a whole
 * runs in chunks of items).  After a batch whose items all took it, later evaluations return what they would have returned
 * without the call.  Sharded handles run the batch on every shard's patterns and add the per-item results in shard order.
 * PHYAMD_EINVAL: count < 1, null pointers; PHYAMD_EUNSUPPORTED: explicit node matrices (they cannot follow per-item lengths). */
int phyamd_gradient_batch(phyamd_engine *e, int flags, int32_t count, const double *branch_lengths, double *lnl, double *cat_gradient);
/* lnL and the per-category branch gradient of `count` trees on the engine's tip data, weights and models.
 * left, right [count][2T-1] and roots [count]: each item in phyamd_set_topology's convention (tips 0..T-1 are the engine's
 * tips, internal ids T..2T-2 in any order, any internal node may be the root); branch_lengths [count][2T-1] by the ITEM's node
 * ids (root entry ignored); lnl [count]; cat_gradient [count][2T-1][C] by the item's node ids, the item's root row 0, or NULL
 * for lnL only.  Item b equals what a fresh engine with the same data and models returns from phyamd_set_topology(item b),
 * phyamd_set_branch_lengths(item b) and phyamd_gradient(flags) / phyamd_log_likelihood.  The engine itself -- its topology,
 * lengths, partials -- is unchanged: later evaluations return the bits they would have returned without the call.  An item's
 * result does not depend on `count`, its position, the other items or the chunks the batch ran in, bit for bit; an item whose
 * arrays equal the engine's own returns the bits of phyamd_gradient_batch for the same lengths (same op builder, same kernel).
 * There is NO item-by-item fallback (a loop over phyamd_set_topology rebuilds the schedule and discards the partials per item):
 * PHYAMD_EUNSUPPORTED, naming the condition, unless 4 states, at most 8 categories, an engine that is not rescaling now
 * (PHYAMD_RESCALE_ALWAYS, or PHYAMD_RESCALE_AUTO after its switch, is refused), untiled patterns (any number), no tip cell with
 * an empty state mask, no explicit node matrices, flags 0 or PHYAMD_GRAD_FOLD_ROOT_FREQS, and scratch for at least one item
 * within the memory cap (a batch that does not fit as a whole runs in chunks of items).  An item whose lnL is not finite
 * reports it in-band with an all-NaN gradient, under PHYAMD_RESCALE_NEVER and _AUTO alike: the engine is never switched to
 * rescaling.  Every item is validated on the host before anything is launched (tips -1 / -1; two distinct children in range;
 * one parent per node; a parentless internal root; all nodes reached): PHYAMD_EINVAL with the item's index in the message; also
 * for count < 1 or a null pointer other than cat_gradient.  Needs data, models, weights and a topology of the engine's own.
 * Sharded handles run the batch on every shard's patterns and add the per-item results in shard order. */
int phyamd_gradient_batch_trees(phyamd_engine *e, int flags, int32_t count, const int32_t *left, const int32_t *right,
                                const int32_t *roots, const double *branch_lengths, double *lnl, double *cat_gradient);
/* of the last batch call of either kind (a batch of trees: items_fast = count, items_sequential = 0): items that ran together /
 * one by one, chunks the fast path was cut into, bytes of batch scratch the
 * engine holds (kept for the next call and counted in phyamd_profile.device_bytes, but released whenever an array of the engine
 * itself needs the room: under max_device_bytes the engine behaves as one that never made the call), wall time of the call */
typedef struct { int32_t items_fast, items_sequential, chunks; int64_t scratch_bytes; double ms; } phyamd_batch_profile;
int phyamd_get_batch_profile(phyamd_engine *e, phyamd_batch_profile *out);   /* of the last batch call */
/* lnL, and its first and second derivative in the central branch, of every NNI neighbour of the engine's tree: ONE post-order
 * and ONE pre-order walk of the engine's tree, then every edge's three arrangements in one launch -- O(T) work for the whole
 * neighbourhood, where phyamd_gradient_batch_trees walks each of the 2 (T - 2) neighbours from the tips.
 * A CANDIDATE is every internal node v other than the root; u its parent, s its sibling, a = left[v], b = right[v].  Every
 * subtree keeps its own branch length; the length of v is central_lengths[k][v], or the engine's t_v when central_lengths is
 * NULL.  Row k of lnl, d1, d2 ([3][2T-1] each) at column v:
 *   k = 0  the engine's tree
 *   k = 1  a and s exchanged: v gets children (s, b), u gets a where s was
 *   k = 2  b and s exchanged: v gets children (a, s), u gets b where s was
 * lnl[k][v] is the rearranged tree's log-likelihood: the lnl of the phyamd_gradient_batch_trees item whose arrays are the engine's
 * with the two child slots exchanged and branch_lengths[v] set to the trial length.  d1[k][v], d2[k][v] are its first and second
 * derivative in the length of v, by phyamd_branch_hessian_diagonal's definitions (d1 = that item's sum_c g[v][c] w_c r_c).
 * Columns of tips and of the root are NaN in all three outputs: no such rearrangement exists (two tips: everything is NaN).
 * Entries of central_lengths at those columns are ignored.  d1 and d2 may be NULL (both NULL: their work is skipped; the lnl
 * bits are the same).  When u is the root, k = 1 and k = 2 are, for a reversible model, the same unrooted topology with the
 * lengths of a, b and s redistributed; they are computed like every other entry.  The unrooted NNI ACROSS the root edge (a child
 * of one root child exchanged with a child of the other) is not among the candidates: a caller re-roots the tree to reach it.
 * The engine -- its topology, lengths, partials -- is unchanged: later evaluations return the bits they would have returned
 * without the call, two calls return identical bits, and the result does not depend on what the batch scratch held before.
 * An entry whose lnL is not finite reports it in band with NaN d1 and d2, under PHYAMD_RESCALE_NEVER and _AUTO alike: the engine
 * is never switched to rescaling.  There is no fallback path: PHYAMD_EUNSUPPORTED, naming the condition, under
 * phyamd_gradient_batch_trees' conditions (not 4 states, more than 8 categories, an engine that is rescaling now, tiled patterns, a
 * tip cell with an empty state mask, explicit node matrices, scratch -- every internal node's lower and upper partial, held in
 * the batch scratch and released like it -- that does not fit the memory cap) and for flags other than 0.  PHYAMD_EINVAL: null
 * engine or lnl, no eigen system, a negative or non-finite trial length of a candidate.  Sharded handles run on every shard's
 * patterns and add the three arrays in shard order. */
int phyamd_nni_log_likelihoods(phyamd_engine *e, int flags, const double *central_lengths /* [3][2T-1] or NULL */,
                               double *lnl /* [3][2T-1] */, double *d1 /* [3][2T-1] or NULL */, double *d2 /* [3][2T-1] or NULL */);
/* of the last phyamd_nni_log_likelihoods: candidate edges scored (T - 2), bytes of batch scratch the engine holds (see
 * phyamd_batch_profile), wall time of the call */
typedef struct { int32_t candidates; int64_t scratch_bytes; double ms; } phyamd_nni_profile;
int phyamd_get_nni_profile(phyamd_engine *e, phyamd_nni_profile *out);
/* The central branch of every NNI neighbour optimised in one call: for every entry (k, v) of phyamd_nni_log_likelihoods -- the same
 * candidates v, the same arrangements k = 0, 1, 2, NaN in the columns of tips and of the root (iterations: 0) -- the length of v in
 * [lower, upper] that maximises the entry's lnL, found on the device by ONE walk of the engine's tree and then, per entry, an
 * iteration that repeats no walk, no matrix launch and no host round trip (the four messages that meet on the edge do not depend
 * on the length).  THE RULE, per entry: t = clamp(start, lower, upper), a = lower, b = upper, where start is start_lengths[k][v] or,
 * with start_lengths NULL, the engine's t_v.  Each iteration evaluates d1(t) and d2(t); if d1 > 0 then a = t, else b = t; it
 * proposes t' = t - d1 / d2 when d2 < 0 and a < t' < b, otherwise t' = (a + b) / 2; it stops when |t' - t| <= tolerance, and t* = t'.
 * iterations[k][v] is the number of proposals made.  After max_iterations proposals without that the entry stops all the same:
 * t* is the last proposal and the count is stored negated.  lengths[k][v] = t*; lnl, d1 and d2 are evaluated at t* and are, by
 * definition, what phyamd_nni_log_likelihoods returns for the entry at central_lengths[k][v] = t* (here they are formed from the
 * eigen system without the reference's fabs on P(t): a rounding difference).  A lnL that is not finite at an iterate ends the entry
 * in band: lengths holds that iterate, lnl the value that is not finite, d1 and d2 NaN and iterations a negative count; the engine
 * is never switched to rescaling.  d1, d2 and iterations may be NULL.
 * The engine -- its topology, lengths, partials -- is unchanged and later evaluations return the bits they would have returned
 * without the call; two calls return identical bits, and an entry's bits do not depend on the other candidates, on the chunks
 * the entries ran in or on which optional outputs are asked for.  The scratch is the batch scratch's: the walk's item of
 * phyamd_nni_log_likelihoods and per entry C x 4 doubles per pattern; candidates that do not fit the memory cap together run in
 * chunks.  There is no fallback path: PHYAMD_EUNSUPPORTED, naming the condition, under phyamd_gradient_batch_trees' conditions (not
 * 4 states, more than 8 categories, an engine that is rescaling now, tiled patterns, a tip cell with an empty state mask, explicit
 * node matrices), when the scratch of the walk and one candidate does not fit the memory cap, for flags other than 0, and on a
 * handle sharded over several devices (every iteration would need a sum across the shards).  PHYAMD_EINVAL: null engine, lengths
 * or lnl, no eigen system, bounds that are not 0 <= lower < upper < inf, a tolerance that is not finite and positive,
 * max_iterations outside 1..1000, a negative or non-finite start length of a candidate. */
int phyamd_nni_optimize(phyamd_engine *e, int flags, const double *start_lengths /* [3][2T-1] or NULL: the engine's t_v */,
                        double lower, double upper, double tolerance, int32_t max_iterations,
                        double *lengths /* [3][2T-1] */, double *lnl /* [3][2T-1] */, double *d1 /* [3][2T-1] or NULL */,
                        double *d2 /* [3][2T-1] or NULL */, int32_t *iterations /* [3][2T-1] or NULL */);
/* of the last phyamd_nni_optimize: candidate edges, chunks of candidates they ran in, bytes of batch scratch the engine holds (see
 * phyamd_batch_profile), proposals made over all entries, wall time of the call */
typedef struct { int32_t candidates, chunks; int64_t scratch_bytes, iterations; double ms; } phyamd_nni_optimize_profile;
int phyamd_get_nni_optimize_profile(phyamd_engine *e, phyamd_nni_optimize_profile *out);
/* lnL of every SPR regraft of chosen subtrees of the engine's tree: per prune node ONE post-order and ONE pre-order walk of the
 * tree without it, then every target edge in one launch -- O(T) work per prune node and O(T^2) for the whole neighbourhood, where
 * phyamd_gradient_batch_trees walks each of the O(T^2) rearranged trees from the tips.
 * Row i of lnl ([count][2T-1]) belongs to the prune node p = prune[i]; prune == NULL: count must be 2T-1 and row i is node i.
 * Column w is the target edge, named by the node below it.  With u = parent(p), s = sibling(p), g = parent(u), x = parent(w),
 * lnl[i][w] is the log-likelihood of the tree obtained from the engine's arrays by (node ids kept)
 *   g's child slot that held u now holds s, with t'_s = t_s + t_u;
 *   x's child slot that held w now holds u;
 *   u keeps p in its slot and gets w in the slot s had, with t'_u = t'_w = 0.5 t_w;
 * everything else -- the root, t_p -- unchanged: the graft edge is halved and the sibling's branch absorbs the parent's.  It is
 * the lnl of the phyamd_gradient_batch_trees item with those arrays.  Column w is a CANDIDATE unless w is the root, u, s, p or a
 * descendant of p; every other column is NaN.  A row is all NaN when p is the root or a child of the root (no error, so that
 * prune == NULL works uniformly): a caller re-roots the tree to reach those moves, as for the NNI across the root edge above.
 * Duplicates in prune are allowed.  There are no derivatives and no trial lengths in this call: the lengths are a fixed, arbitrary
 * assignment.  phyamd_spr_optimize (at the end of this header) optimises the three branches at the graft point of every candidate.
 * The remaining contract is phyamd_nni_log_likelihoods': the engine -- its topology, lengths, partials -- is unchanged and later
 * evaluations return the bits they would have returned without the call; two calls return identical bits, and a row does not
 * depend on what the batch scratch held before, on count, on its position in prune or on the chunks the rows ran in; a
 * candidate whose lnL is not finite reports it in band, under PHYAMD_RESCALE_NEVER and _AUTO alike, and the engine is never
 * switched to rescaling.  There is no fallback path: PHYAMD_EUNSUPPORTED, naming the condition, under
 * phyamd_gradient_batch_trees' conditions (not 4 states, more than 8 categories, an engine that is rescaling now, tiled patterns,
 * a tip cell with an empty state mask, explicit node matrices), for flags other than 0, and when the scratch of one row -- every
 * internal node's lower and upper partial, held in the batch scratch and released like it -- does not fit the memory cap (rows
 * that do not fit as a whole run in chunks of rows).  PHYAMD_EINVAL: null engine or lnl, count < 1, prune == NULL with another
 * count than 2T-1, an id outside 0..2T-2 (with its index in the message), no eigen system (the half-length matrices come from
 * it).  Sharded handles run on every shard's patterns and add the arrays in shard order. */
int phyamd_spr_log_likelihoods(phyamd_engine *e, int flags, int32_t count, const int32_t *prune /* [count] or NULL */,
                               double *lnl /* [count][2T-1] */);
/* of the last phyamd_spr_log_likelihoods or phyamd_spr_log_likelihoods_general: rows asked for, chunks of rows they ran in, candidates scored, bytes of batch scratch
 * the engine holds (see phyamd_batch_profile), wall time of the call.  Sharded handles: candidates and scratch_bytes are summed
 * over the shards */
typedef struct { int32_t prunes, chunks; int64_t candidates, scratch_bytes; double ms; } phyamd_spr_profile;
int phyamd_get_spr_profile(phyamd_engine *e, phyamd_spr_profile *out);
/* The marginal posterior of the state at a node, per site pattern, and its argmax -- the reconstructed ancestral sequence:
 * asr_marginal / _marginal_reconstruction (asr.c:28-134) for `count` nodes at once, on the device, from the lower and the upper
 * partial that meet on each node's branch (the pair phyamd_branch_log_likelihood reads).  With p_n the lower partial of node n (a
 * tip: its 0/1 mask), u_n its upper partial in phyamd_get_partials' convention, P_{n,c} the matrices of its branch as the engine
 * holds them (explicit node matrices included), pi the frequencies and w_c the proportions, per pattern k and state j
 *   n != root:  J[n][k][j] = sum_c w_c p_n[c][k][j] sum_i pi_i u_n[c][k][i] P_{n,c}[i][j]
 *   n == root:  J[n][k][j] = sum_c w_c pi_j p_root[c][k][j]
 *   posteriors[n][k][j] = J[n][k][j] / sum_j' J[n][k][j'],   states[n][k] = the smallest j with the largest J (asr.c:73-86)
 * -- the site likelihood with node n held in state j: sum_j J[n][k][j] = L_k at every node, so a per-pattern factor of a rescaled
 * evaluation cancels in the quotient and the call serves every rescaling policy.  Every state count.
 * nodes [count]: any ids in 0..2T-2, duplicates allowed; NULL: count must be 2T-1 and row i is node i.  Tips are rows like any
 * other: one-hot where the tip is observed, the imputed state where it has a gap or an ambiguity code.  posteriors
 * [count][P][S] and states [count][P]: either may be NULL (not both).  flags: 0 (others reserved, refused).
 * The call evaluates whatever is pending and needs every partial resident: if phyamd_set_keep_partials is off it is turned on
 * (as phyamd_parameter_gradient does for 20 / 60 / 61 states), and if no resident upper partials belong to the current inputs the
 * flags-0 gradient runs.  Afterwards the engine is an engine with phyamd_set_keep_partials(1) that has run phyamd_gradient,
 * and nothing else about it has changed: later evaluations return the bits such an engine returns.  Upper partials that a
 * PHYAMD_GRAD_FOLD_ROOT_FREQS keep-partials gradient left resident are used as they are (pi is inside them).
 * A NaN / inf lnL of the evaluation is reported in band: NaN posteriors, state 255.  A row depends on its node and the engine's
 * inputs only -- not on count, its position, or the chunks the rows ran in (the staging of a chunk is sized to the memory cap, at
 * least one row), bit for bit; two calls return identical bits.  Sharded handles: every shard fills its own pattern range, so a
 * pattern's bits do not depend on the shard count.
 * PHYAMD_EUNSUPPORTED: tiled patterns.  PHYAMD_EINVAL: null engine, flags other than 0,
 * both outputs NULL, count < 1, nodes == NULL with another count than 2T-1, an id outside 0..2T-2 (with its index in the
 * message); an engine that is not ready (data, models, weights, topology) reports what is missing. */
int phyamd_state_posteriors(phyamd_engine *e, int flags, int32_t count, const int32_t *nodes /* [count] or NULL */,
                            double *posteriors /* [count][P][S] or NULL */, uint8_t *states /* [count][P] or NULL */);
/* The posterior of the rate category of each site pattern and its mean rate: SingleTreeLikelihood_posterior_sites
 * (ppsites.c:17-43, 100),
 *   posteriors[k][c] = w_c sum_i pi_i p_root[c][k][i] / sum_c' (the same),   mean_rates[k] = sum_c posteriors[k][c] r_c
 * with r_c the engine's category rates.  The quotient is taken over the categories' own sum instead of exp(lnL_k): identical
 * without rescaling, and the only one of the two defined with it.  Every state count and rescaling policy; an invariant class is
 * a category like any other.  Whatever is pending is evaluated by a post-order pass; the call reads the root's stored partial, as
 * phyamd_root_frequency_term does, and leaves the engine as that pass leaves it: later evaluations return the bits they would
 * have returned without the call (a rescaling engine's stored partials are settled in the reference's form first, as by
 * phyamd_root_frequency_term).  mean_rates may be NULL.  PHYAMD_EUNSUPPORTED: tiled patterns.  Sharded handles: every shard
 * fills its own pattern range. */
int phyamd_site_rate_posteriors(phyamd_engine *e, double *posteriors /* [P][C] */, double *mean_rates /* [P] or NULL */);
/* The full branch-length Hessian of lnL, every pair of branches in one call: _singleTreeLikelihood_ddlogP
 * (treelikelihood.c:532-690), which calculate_hessian (hessian.c:14-25) evaluates pair by pair with a pruning pass each.  Here it is
 * formed from the lower and upper partials a keep-partials gradient leaves resident, with O(T^2) node operations.  With p_n the
 * lower partial of node n (a tip: its 0/1 mask), u_n its upper partial in phyamd_get_partials' convention, P_{n,c} = exp(Q t_n r_c),
 * pi the frequencies, w_c the proportions, r_c the category rates, w_k the pattern weights and L_k the site likelihood, for nodes
 * a, b other than the root
 *   gradient[a]   = sum_k w_k L_a,k / L_k                                (d lnL / d t_a: phyamd_branch_gradient's entry)
 *   hessian[a][b] = sum_k w_k (L_ab,k / L_k - L_a,k L_b,k / L_k^2)        (d2 lnL / d t_a d t_b; symmetric, both triangles written)
 * where L_a,k is the site likelihood with P_{a,c} replaced by r_c Q P_{a,c} and L_ab,k the one with both P_{a,c} and P_{b,c}
 * replaced (a = b: the one replacement by r_c^2 Q Q P_{a,c}, so hessian[a][a] is phyamd_branch_hessian_diagonal's d2[a]).  The
 * root's row and column are 0; for an unrooted tree the caller also zeroes the row and column of the root's child whose length
 * is not a parameter, as for phyamd_gradient.  With msg(n) = P_n p_n, A_m = P_m^T (pi o u_m) (the root: pi),
 * T_a^(par a) = r_c Q P_a p_a and T_a^(par m) = P_m (T_a^(m) o msg(other child of m)) the terms are
 *   a below b:               L_ab,k = sum_c w_c r_c sum_i (pi o u_b)_i (Q P_b (T_a^(b) o msg(other child of b)))_i
 *   a, b on two sides of m:  L_ab,k = sum_c w_c sum_i (A_m)_i (T_a^(m))_i (T_b^(m))_i
 * hessian [2T-1][2T-1] row-major by node id; gradient [2T-1] or NULL; flags: 0 (others reserved, refused).
 * The call evaluates whatever is pending and needs every partial resident, like phyamd_state_posteriors: if
 * phyamd_set_keep_partials is off it is turned on, and if no resident upper partials belong to the current inputs the flags-0
 * gradient runs.  Afterwards the engine is an engine with phyamd_set_keep_partials(1) that has run phyamd_gradient, and nothing
 * else about it has changed.  Upper partials that a PHYAMD_GRAD_FOLD_ROOT_FREQS keep-partials gradient left resident are used as
 * they are.  *lnl: the log likelihood of that evaluation; if it is NaN or +-inf, gradient and hessian are all NaN (in band:
 * PHYAMD_RESCALE_NEVER on an underflowing tree reports -inf this way).
 * Sums over patterns use no floating-point atomics: they are formed over blocks of 64 patterns and added in block order, so two
 * calls return identical bits whatever the scratch held before.  The scratch (a tangent per (branch, ancestor): sum_a depth(a) C
 * P 4 doubles, and a row of P doubles per branch) lives in the batch scratch and is counted and released like it; under
 * max_device_bytes the patterns run in chunks of whole blocks whose sums are added in chunk order (PHYAMD_ENOMEM if not one
 * block fits): the bits may depend on the cap and on nothing else.  Sharded handles: every shard runs its own patterns, and lnl,
 * gradient and hessian are added over the shards like phyamd_gradient's sums.
 * PHYAMD_EUNSUPPORTED, with the condition in the message: state counts other than 4, more than 8 categories, explicit node
 * matrices (Q P is the derivative of exp(Q t r) only), tiled patterns, and an engine that is rescaling when the partials are read
 * (PHYAMD_RESCALE_ALWAYS, or PHYAMD_RESCALE_AUTO after its switch, including a switch made by the evaluation this call
 * triggered): the terms multiply partials of different nodes, and a rescaled evaluation's partials do not share units.
 * PHYAMD_EINVAL, naming the function and the argument: null engine, lnl or hessian; flags other than 0; no eigen system; an
 * engine that is not ready. */
int phyamd_branch_hessian(phyamd_engine *e, int flags, double *lnl, double *gradient /* [2T-1] or NULL */, double *hessian /* [2T-1][2T-1] */);
/* The last phyamd_branch_hessian: pairs = the unordered pairs a <= b scored, (2T-2)(2T-1)/2; chunks = the pattern chunks the call
 * ran in (sharded: the most of any shard); scratch_bytes = the batch scratch held afterwards, summed over the shards */
typedef struct { int32_t chunks; int64_t pairs, scratch_bytes; double ms; } phyamd_hessian_profile;
int phyamd_get_hessian_profile(phyamd_engine *e, phyamd_hessian_profile *out);
/* How the 20 / 60 / 61-state kernels of the last post-order pass and of the last pre-order pass were launched (read-only
 * bookkeeping of the launchers; a pass that found its results current and launched nothing leaves the record as it was).
 * lower_family: 0 = k_lower_gen, one launch per tree level; 1 = k_lower_gen_walk, one launch whose workgroups draw (pattern
 * group, category) units from a counter; -1 = no post-order pass has run.  *_slots: the workgroups the card holds at one time for
 * that pass's kernel, as the occupancy query answered (what the tile chooser and the walk's launch are sized by).  *_levels: tree
 * levels launched (an incremental pass: only those with a node to recompute); *_tiles_min / _max: the fewest and the most
 * 16-pattern tiles per wave over those levels (0: none launched; the walk has neither levels nor tiles: 0).  walk_units / walk_workgroups: the
 * walk's work units and the workgroups launched for them (0 unless lower_family is 1).  The pre-order pass is the gradient's, the
 * parameter gradient's or phyamd_branch_hessian_diagonal's (upper_hess = 1: k_upper_gen's HESS form); upper_levels = 0: none has
 * run.  Sharded handles: the first shard's.  PHYAMD_EUNSUPPORTED on a 4-state engine, with the condition in the message. */
typedef struct { int32_t lower_family, lower_slots, lower_levels, lower_tiles_min, lower_tiles_max, walk_units, walk_workgroups;
                 int32_t upper_hess, upper_slots, upper_levels, upper_tiles_min, upper_tiles_max; } phyamd_general_profile;
int phyamd_get_general_profile(phyamd_engine *e, phyamd_general_profile *out);
/* Which 4-state kernel the last post-order pass and the last pre-order pass of an evaluation launched (read-only bookkeeping of
 * the launchers, written where the instantiation is picked; a pass that found its results current and launched nothing leaves
 * the record as it was, and so does the pass of phyamd_branch_hessian_diagonal).  Every field is -1 before the first pass of
 * its kind.  *_family: 0 = the level kernels (k_lower4 / k_upper4, one launch per tree level), 1 = the table-gather tree walks
 * (k_lower4_walk / k_upper4_walk), 2 = the streamed tree walks (k_lower4_stream / k_upper4_stream).  lower_form: what the pass
 * left in the stored lowers, 0 = the reference's p_n, 1 = t_n = P_n p_n, 2 = t_n rescaled by powers of two per category.
 * *_scale: 0 = no rescaling, 1 = the reference's, 2 = powers of two.  *_ambiguous: the streamed walks' form for tip data with
 * partial ambiguity codes.  lower_incremental: the pass recomputed only the nodes above changed branches.  *_waves: the wave
 * bound the kernel was compiled for, 4 / 8 / 16 (the streamed walks: 4, the most waves their workgroup holds).  lower_ppt: patterns per
 * thread of k_lower4_walk, 1 or 2 (0: another kernel).  upper_tf: the pass read stored lowers of form 1 or 2.  upper_fold /
 * upper_compat: PHYAMD_GRAD_FOLD_ROOT_FREQS / the PHYAMD_GRAD_COMPAT_SCALED arithmetic.  upper_params: the pass also formed the
 * substitution-parameter sums; upper_catblk: ... in k_upper4_walk's form of four pattern groups of one category per workgroup.
 * upper_pair_ops: the pair ops (phyamd_stream_pairs) of the descriptor set the streamed walk read, 0 where it read a set
 * without them.  Sharded handles: the first shard's; pattern tiles: the last tile's.  PHYAMD_EUNSUPPORTED on a 20 / 60 /
 * 61-state engine, with the condition in the message. */
typedef struct { int32_t lower_family, lower_form, lower_scale, lower_ambiguous, lower_incremental, lower_waves, lower_ppt;
                 int32_t upper_family, upper_scale, upper_ambiguous, upper_waves, upper_tf, upper_fold, upper_compat, upper_params, upper_catblk,
                         upper_pair_ops; } phyamd_pass_profile;
int phyamd_get_pass_profile(phyamd_engine *e, phyamd_pass_profile *out);
/* lnL and the per-category branch gradient for `count` pattern-weight vectors on the engine's tree, data and models: the batch
 * axis of resampling -- bootstrap and jackknife replicates of one alignment (phyresampling.c:105-260 builds a SitePattern and a
 * likelihood object per replicate), RELL reweighting, site minibatches (a weight vector with zeros).  weights [count][P], any
 * finite doubles >= 0 (a zero weight does what dropping the pattern does, its site likelihood being finite); branch_lengths [count][2T-1] by node id (root entries
 * ignored), or NULL: every item on the engine's own lengths; lnl [count]; cat_gradient [count][2T-1][C], root rows 0, or NULL
 * for lnL only.  Item b equals what phyamd_set_pattern_weights(weights[b]), phyamd_set_branch_lengths(branch_lengths[b]) if
 * lengths are given, and phyamd_gradient(flags) / phyamd_log_likelihood return.  NaN/inf lnL of an item => that item's gradient
 * all NaN.  Afterwards the engine's own weights and lengths are back and later evaluations return the bits they would have
 * returned without the call.  Like phyamd_gradient_batch the call is defined as "evaluate the items one by one through the
 * ordinary path, then put the engine's weights and lengths back" and so works on every engine configuration; under that call's
 * conditions -- 4 states, at most 8 categories, an engine that is not rescaling, untiled patterns, no tip cell with an empty state
 * mask, flags 0 or PHYAMD_GRAD_FOLD_ROOT_FREQS, scratch within the memory cap -- the items run together, with no floating-point
 * atomics, on one of two paths:
 *   with branch_lengths: phyamd_gradient_batch's walk with a weight row per item, under its bound of 8192 patterns per shard.  An
 *     item's bits do not depend on `count`, its position or the chunks the batch ran in, and an item whose weights equal the
 *     engine's own returns the bits of phyamd_gradient_batch for the same lengths.  PHYAMD_RESCALE_AUTO: an item whose lnL is
 *     not finite is evaluated again through the ordinary path, which may switch the engine to rescaling; _NEVER: in band.
 *   branch_lengths == NULL: partials and matrices do not depend on the weights, so ONE walk of the tree serves every item.  It
 *     leaves the unweighted per-pattern terms (log L_k, and every (branch, category)'s gradient term over L_k) as rows, and item
 *     b's results are the products of its weight row with them, formed on the matrix pipe over segments of 4096 patterns that
 *     are added in segment order.  Any number of untiled patterns; explicit node matrices are used as the engine holds them.  An
 *     item's bits do not depend on `count`, its position, the chunks of items or what the scratch held before; the lnL-only form
 *     returns the same lnL bits.  If the rows do not fit the memory cap the patterns run in chunks of whole blocks of 64 whose
 *     sums are added in chunk order (PHYAMD_ENOMEM if not one block fits): the bits may then depend on the cap.
 *     PHYAMD_RESCALE_AUTO: if any pattern's log L_k is not finite the whole call goes item by item, which may switch the engine
 *     to rescaling; _NEVER: in band.
 * The scratch lives in the batch scratch and is counted and released like it.  Sharded handles: every shard takes its own
 * pattern columns of `weights`, and the per-item results are added in shard order.
 * PHYAMD_EINVAL, naming the function and the argument: null engine, weights or lnl; count < 1; a negative or non-finite weight
 * (with the item's index in the message); an engine that is not ready (data, models, weights and a topology of its own, and
 * lengths unless the call brings them).  PHYAMD_EUNSUPPORTED: explicit node matrices together with branch_lengths. */
int phyamd_gradient_batch_weights(phyamd_engine *e, int flags, int32_t count, const double *weights /* [count][P] */,
                                  const double *branch_lengths /* [count][2T-1] or NULL */, double *lnl /* [count] */,
                                  double *cat_gradient /* [count][2T-1][C] or NULL */);
/* of the last phyamd_gradient_batch_weights: items that ran together / one by one; chunks of items and of patterns the fast path
 * was cut into; walks = tree walks of the fast path (with branch_lengths: the items walked; without: the pattern chunks, one
 * walk each, whatever the item count); bytes of batch scratch the engine holds (see phyamd_batch_profile); wall time of the call.
 * Sharded handles: the fewest items_fast, the most of the other counts, scratch_bytes summed over the shards */
typedef struct { int32_t items_fast, items_sequential, item_chunks, pattern_chunks, walks;
                 int64_t scratch_bytes; double ms; } phyamd_weight_batch_profile;
int phyamd_get_weight_batch_profile(phyamd_engine *e, phyamd_weight_batch_profile *out);
/* The per-pattern log-likelihoods of `count` trees on the engine's tip data, weights and models, their weighted sums, and RELL
 * replicates of them: what model comparison consumes -- the site log-likelihoods behind CPO, WAIC and PSIS-LOO (logmcmc.c logs
 * them per sample, cpo.c:17-75 reads them back), and pattern_lnl [trees][P] times weights [replicates][P]^T behind RELL bootstrap
 * support and the KH / SH / AU topology tests (phyresampling.c:105-260 builds a SitePattern and a likelihood object per replicate).
 * left, right [count][2T-1] and roots [count]: each item in phyamd_set_topology's convention (tips 0..T-1 are the engine's tips,
 * internal ids T..2T-2 in any order, any internal node may be the root), or all three NULL: every item is the engine's tree;
 * branch_lengths [count][2T-1] by the ITEM's node ids (root entry ignored).
 *   pattern_lnl[b][k] ([count][P], or NULL) = log L_k of item b: the quantity phyamd_get_pattern_log_likelihoods returns after
 *     phyamd_set_topology(item b), phyamd_set_branch_lengths(item b) and phyamd_log_likelihood;
 *   lnl[b] = sum_k w_k pattern_lnl[b][k] with the engine's weights, over blocks of 64 patterns added in block order;
 *   replicate_lnl[r][b] ([replicate_count][count]) = sum_k replicate_weights[r][k] pattern_lnl[b][k], replicate_weights
 *     [replicate_count][P] any finite doubles >= 0: formed on the matrix pipe over segments of 4096 patterns that are added in
 *     segment order.  replicate_count 0 with both pointers NULL: no replicates.
 * One post-order pass per item that stores only the partials a later op still reads -- at most floor(log2 T) - 1 per pattern and
 * category, none for a caterpillar (phyamd_post_order_slots) -- so far more items fit a chunk than in phyamd_gradient_batch_trees'
 * lnL-only form; the [count][P] matrix is never resident: each chunk of items is walked, read back and multiplied with every chunk
 * of replicates before the next.  No floating-point atomics.  The engine itself -- its topology, lengths, weights, partials -- is
 * unchanged: later evaluations return the bits they would have returned without the call.  An item's lnl, its pattern_lnl row and
 * its replicate_lnl column depend on its own arrays, the engine's inputs and (the column) the replicate rows only: not on `count`,
 * its position, the chunks of items or of replicates, what the scratch held, or which optional outputs were asked for, bit for
 * bit; two calls return identical bits.
 * There is NO item-by-item fallback: PHYAMD_EUNSUPPORTED, naming the condition, under phyamd_gradient_batch_trees' conditions (not
 * 4 states, more than 8 categories, an engine that is rescaling now, tiled patterns, a tip cell with an empty state mask, explicit
 * node matrices, scratch for one item that does not fit the memory cap) and for flags other than 0.  An item whose lnL is not
 * finite reports it in band -- its row as computed, its replicate_lnl column all NaN -- under PHYAMD_RESCALE_NEVER and _AUTO
 * alike: the engine is never switched to rescaling.  PHYAMD_EINVAL, naming the function and the argument: a null engine,
 * branch_lengths or lnl; count < 1; only some of left / right / roots null; replicate_count < 0; replicates without replicate_lnl
 * or the reverse; a negative or non-finite replicate weight (with the replicate's index); an invalid item (validated on the host
 * before anything is launched, with the item's index); an engine that is not ready (data, models, weights and a topology of its
 * own).  The scratch lives in the batch scratch and is counted and released like it.  Sharded handles: every shard fills its own
 * pattern columns of pattern_lnl and takes its own columns of replicate_weights; lnl and replicate_lnl are added in shard order. */
int phyamd_pattern_log_likelihoods_trees(phyamd_engine *e, int flags, int32_t count, const int32_t *left, const int32_t *right,
                                         const int32_t *roots, const double *branch_lengths, double *lnl /* [count] */,
                                         double *pattern_lnl /* [count][P] or NULL */, int32_t replicate_count,
                                         const double *replicate_weights /* [replicate_count][P] or NULL */,
                                         double *replicate_lnl /* [replicate_count][count] or NULL */);
/* of the last phyamd_pattern_log_likelihoods_trees: its items; the chunks of items it ran in and the chunks of replicates each of
 * them was multiplied with; the most partials any item parked per pattern and category; bytes of batch scratch the engine holds
 * (see phyamd_batch_profile); wall time of the call.  Sharded handles: the most of each count, scratch_bytes summed */
typedef struct { int32_t items, chunks, replicate_chunks, lower_slots; int64_t scratch_bytes; double ms; } phyamd_site_lnl_profile;
int phyamd_get_site_lnl_profile(phyamd_engine *e, phyamd_site_lnl_profile *out);
int phyamd_synchronize(phyamd_engine *e);

/* --- inspection (parity tests, debugging) --- */
int phyamd_get_pattern_log_likelihoods(phyamd_engine *e, double *out /* [P] */);
/* lower (upper=0) or upper (upper=1) partials of a node after the last evaluation, reference layout
 * [C][P][S]. Upper partials exist only after phyamd_gradient with keep_partials enabled. */
int phyamd_get_partials(phyamd_engine *e, int node, int upper, double *out);
/* P(t_n r_c) of a node, or with derivative = 1 its derivative in the argument t_n r_c (substmodel.c:695-723: WITHOUT the factor
 * r_c), as the next evaluation uses them.  A node with explicit matrices (phyamd_set_node_matrices, phyamd_set_matrices): what
 * was set, and Q P for the derivative -- the only one the engine defines for such a node (the branch term of its gradient), Q
 * from phyamd_set_rate_matrix / phyamd_set_eigen; PHYAMD_EINVAL without a Q. */
int phyamd_get_node_matrices(phyamd_engine *e, int node, int derivative, double *out /* [C][S][S] */);
/* The post-order walk of a tree as the streamed 4-state kernel runs it, from the host schedule alone (no device, no engine): the
 * ops in launch order -- the cut subtrees' chunks, then the top part -- eight ints each: chunk | node | left | right | where the
 * left child's partial comes from | the right child's (-1: not a stored child, 0: memory, 1: the op in front, 2: the wave's first
 * park slot, 3: its second) | bit 0 / 1: the result is kept in the first / second slot | bit 0 / 1: the left / right child is the
 * root of a cut subtree (written by another workgroup).  second_slot = 0: the schedule of PHYAMD_LOWER_PARK2=0.  Returns the
 * number of ops (at most `capacity` of them are written) or a negative PHYAMD_E* code. */
int phyamd_post_order_parks(int32_t tip_count, const int32_t *left /* [2T-1] */, const int32_t *right, int32_t root, int32_t second_slot,
                            int32_t *out /* [capacity][8] */, int32_t capacity);
/* The pre-order walk of a tree as one of its 4-state kernels runs it, from the host schedule alone (no device, no engine): the ops
 * in launch order -- the top part, then the cut subtrees' chunks -- PHYAMD_PRE_ORDER_COLUMNS ints each.
 *   form 0: the chunked list as k_upper4_walk reads it (one LDS park slot per wave);
 *   form 1: the same list after the streamed walk's rewrites, as k_upper4_stream reads its descriptors (two LDS slots, the op in
 *           front's registers instead of a slot it would only just have stored, children swapped so that the carried one is left);
 *   form 2: the one unchunked list, as k_upper4_walk's parameter form reads it (no LDS slot: every park has an HBM slot).
 * Columns: 0 chunk | 1 node | 2 left | 3 right | 4, 5 kind of the left / right child (0 tip, 1 stored, 2 DEEP: two fringe or tip
 * halves, an op of its own, 3 cherry, 4 cherry + tip) | 6, 7 kinds of a DEEP left child's halves, 8, 9 of a DEEP right child's
 * (-1: the child is not DEEP) | 10 where the node's own upper comes from (0: nowhere, the root; 1: the registers of the op in
 * front; 2 / 3: the wave's first / second LDS slot; 4: HBM) | 11 its HBM slot (-1: none) | 12 where the left child's upper goes
 * (0: nowhere, a tip or fringe child; 1: to the next op in registers; 2 / 3: LDS slot; 4: HBM) | 13 the HBM slot it is stored to
 * (-1: not stored) | 14, 15 the same for the right child | 16 form 1: the HBM slot prefetched for the next op (-1: none) |
 * 17 bit 0 / 1: the left / right child is the root of a cut subtree (its op opens another chunk) | 18 the carried child (0: none,
 * 1: left, 2: right; forms 0 and 2: as scheduled, even where a cut sent it through HBM) | 19 the number of branch terms the op
 * produces | 20-29 their nodes, in the order of the op's result rows (-1: unused).
 * *hbm_slots (may be NULL): the upper slots the list needs.  Returns the number of ops (at most `capacity` of them are written)
 * or a negative PHYAMD_E* code. */
#define PHYAMD_PRE_ORDER_COLUMNS 30
int phyamd_pre_order_schedule(int32_t tip_count, const int32_t *left /* [2T-1] */, const int32_t *right, int32_t root, int32_t form,
                              int32_t *out /* [capacity][PHYAMD_PRE_ORDER_COLUMNS] */, int32_t capacity, int32_t *hbm_slots);
/* The post-order pass of a tree as phyamd_pattern_log_likelihoods_trees runs it, from the host schedule alone (no device, no
 * engine): the internal nodes' ops in order, the larger subtree first and ties by left / right, six ints each: node | left | right |
 * where the left child's partial comes from | the right child's (-1: a tip, -2: the op in front's registers, >= 0: a slot, free
 * again once read) | where the result goes (-2: handed on in registers, >= 0: a slot, -1: the root's).  *slots (may be NULL): the
 * slots the list uses, at most max(0, floor(log2 T) - 1).  Returns the number of ops (at most `capacity` of them are written) or a
 * negative PHYAMD_E* code. */
int phyamd_post_order_slots(int32_t tip_count, const int32_t *left /* [2T-1] */, const int32_t *right, int32_t root,
                            int32_t *out /* [capacity][6] */, int32_t capacity, int32_t *slots);
/* The stored nodes that the streamed 4-state walks of a tree do not store (PHYAMD_STREAM_ELIDE, on by default), from the host
 * schedule alone (no device, no engine): a stored node with one stored child and one child that is a tip or a cherry, which the
 * post-order walk hands to its parent in registers and the pre-order walk forms again from the stored child.  Children before
 * parents, eight ints each: node | its parent | its stored child | its other child | that child's kind (0 tip, 3 cherry) | how
 * the post-order walk hands the node to its parent (1: the op in front, 2: the wave's first park slot) | the side the node has in
 * its parent's streamed pre-order op (0 left, 1 right) | the post-order chunk of the node's and its parent's ops.  Returns the
 * number of such nodes (at most `capacity` of them are written) or a negative PHYAMD_E* code. */
int phyamd_stream_elisions(int32_t tip_count, const int32_t *left /* [2T-1] */, const int32_t *right, int32_t root,
                           int32_t *out /* [capacity][8] */, int32_t capacity);
/* The pair ops of the streamed pre-order walk of a tree (PHYAMD_STREAM_PAIRS, on by default), from the host schedule alone (no
 * device, no engine): the plain pass runs the op of a DEEP child inside its parent's op where that child is walked first, the op's
 * other child is stored or a tip, and the parent's table block has room for the child's tips.  One record of
 * PHYAMD_STREAM_PAIR_COLUMNS ints per op of the streamed list (phyamd_pre_order_schedule, form 1, with PHYAMD_STREAM_ELIDE's kinds):
 * 0 chunk | 1 node | 2 what the rule decided (0: fused with its DEEP child's op; 1: no DEEP child; 2: no DEEP child whose op is the
 * next of the chunk and takes its upper in registers; 3: the other child is neither stored nor a tip; 4: a tip beside a DEEP child
 * of five or six tips; 5: the op runs inside the pair in front; -1: pairs = 0) | 3 the DEEP child looked at | 4 the other child |
 * 5 its kind in the descriptor (0 tip, 1 stored, 2 DEEP, 3 cherry, 4 cherry + tip, 5 / 6 stored and formed beside a tip / cherry) |
 * 6 the DEEP child's tips | 7 fused: 1 = the op behind the pair is the other child's and takes its upper in registers | 8 where the
 * op's own upper comes from in the pair set (0 root, 1 registers, 2 / 3 LDS slot, 4 HBM) | 9 where its right child's upper goes
 * (0 nowhere or registers, 2 / 3 LDS slot, 4 HBM) | 10 the HBM slot it requests for the next op (-1: none) | 11 the op that runs
 * next (-1: the chunk ends) | 12 whether it requests both pieces of that op's table block | 13 a digest of the op's rows in the
 * tables every other pass reads (the same with pairs = 0 and 1) | 14 a digest of its descriptor in the pair set | 16-31 fused: the
 * node of each of the sixteen result lanes' branch terms (-1: none) | 32-47 and its slab position.  Returns the number of ops (at
 * most `capacity` of them are written) or a negative PHYAMD_E* code. */
#define PHYAMD_STREAM_PAIR_COLUMNS 48
int phyamd_stream_pairs(int32_t tip_count, const int32_t *left /* [2T-1] */, const int32_t *right, int32_t root, int32_t pairs,
                        int32_t *out /* [capacity][PHYAMD_STREAM_PAIR_COLUMNS] */, int32_t capacity);
/* The elided nodes (phyamd_stream_elisions) whose own op of the streamed pre-order walk takes its stored child's plane from its
 * parent's op in registers instead of requesting it again (PHYAMD_STREAM_KEEP, on by default), from the host schedule alone (no
 * device, no engine).  The parent's op is handed that plane to form the elided node's message; where the node's op is the very
 * next op of the chunk and the stored child sits there on the side the node had in its parent's op, the parent's op requests
 * nothing for that side.  One record of PHYAMD_STREAM_KEEP_COLUMNS ints per elided node, in phyamd_stream_elisions' order:
 * 0 node | 1 its parent | 2 the side it has in its parent's op (0 left, 1 right) | 3 what the rule decided (0: kept; 1: the node's
 * op is not the next op of its parent's chunk -- its upper is parked or the other child is walked first; 2: its stored child sits
 * on the other side there; 3: its op opens a chunk, whose prologue fetches its operands; 4: keep = 0) | 4 whether the parent's op
 * requests a plane for that side in the descriptor set of the rescaled and ambiguity-code passes (1) or not (0) | 5 the same in
 * the plain pass's set (phyamd_stream_pairs).  Returns the number of elided nodes (at most `capacity` of them are written) or a
 * negative PHYAMD_E* code. */
#define PHYAMD_STREAM_KEEP_COLUMNS 6
int phyamd_stream_keeps(int32_t tip_count, const int32_t *left /* [2T-1] */, const int32_t *right, int32_t root, int32_t keep,
                        int32_t *out /* [capacity][PHYAMD_STREAM_KEEP_COLUMNS] */, int32_t capacity);
int phyamd_is_rescaling(phyamd_engine *e);
/* SingleTreeLikelihood_use_rescaling (treelikelihood.c:1410-1423) after construction: PHYAMD_RESCALE_ALWAYS / _NEVER switch
 * at once (the next evaluation recomputes every node), PHYAMD_RESCALE_AUTO keeps the current state and re-arms the lazy switch. */
int phyamd_set_rescaling(phyamd_engine *e, int policy);
/* keep every node's upper partials resident after a gradient call (costs memory; off by default) */
int phyamd_set_keep_partials(phyamd_engine *e, int on);

/* --- measurement --- */
typedef struct {
	double matrices_ms, lower_ms, upper_ms, reduce_ms; /* HIP-event time per kernel family, last evaluation */
	int32_t lower_launches, upper_launches;
	int64_t device_bytes; /* resident device memory of this engine */
	int32_t tiles;         /* pattern tiles per evaluation */
} phyamd_profile;
/* Sums over patterns (lnL, gradient rows of the default 4-state path) are formed over the engine's blocks of 64 patterns in an
 * order fixed by the pattern range alone: the block range is bisected `levels` times (default 3: eight segments), each segment
 * summed in block order, the segments added pairwise.  An engine that holds one half / quarter / eighth of a larger pattern list
 * cut by the same bisection (physher_amd/sharding.py::shard_range, phyamd_create_sharded with 2 / 4 / 8 devices) runs with
 * 2 / 1 / 0 levels; adding the shards' results pairwise then gives bit for bit the one-engine result.  Replaces nothing in the
 * reference (its sums are sequential, treelikelihood.c:1482-1487); SURVEY 8e "deterministic alternative". */
int phyamd_set_reduction_levels(phyamd_engine *e, int levels);
int phyamd_set_profiling(phyamd_engine *e, int on);
int phyamd_get_profile(phyamd_engine *e, phyamd_profile *out);

/* --- all branch lengths of a batch of trees --- */
/* Every branch length of `count` trees optimised on the device, one branch at a time, pass after pass: the sweep a hill-climb runs
 * between topology rounds, for many trees at once.  left, right [count][2T-1] and roots [count] are the items, each in
 * phyamd_gradient_batch_trees' convention, or all three NULL: every item is the engine's tree.  branch_lengths [count][2T-1], by the
 * ITEM's node ids, is the start.  optimise [count][2T-1] marks the nodes whose branches are visited (non-zero), or NULL: every node
 * but the root; the root's own entry is ignored.
 * THE RULE.  The state of an item is its lengths t, a copy of the start.  Entries of the root and of nodes that are not visited
 * are never changed and come back in `lengths` bit for bit.
 *   A pass visits the nodes n with n != root and optimise[n] != 0 in the post-order of the item's tree: the left subtree, the right
 * subtree, then the node.
 *   A visit of n: f(t) = (lnL, d1, d2) of the item's tree with t_n = t and every other length as it stands now, d1 and d2 by
 * phyamd_branch_hessian_diagonal's definitions.  t0 = clamp(t_n, lower, upper).  t' comes from phyamd_nni_optimize's rule started at
 * t0: t = t0, a = lower, b = upper; each iteration evaluates d1(t) and d2(t); if d1 > 0 then a = t, else b = t; it proposes
 * t' = t - d1 / d2 when d2 < 0 and a < t' < b, otherwise t' = (a + b) / 2; it stops when |t' - t| <= tolerance or after
 * max_iterations proposals.  The visit accepts t_n = t' when lnL(t') is finite and lnL(t') >= lnL(t0); otherwise t_n = t0.  So lnL
 * never falls from visit to visit.
 *   A lnL that is not finite at an iterate (one of the t whose d1 and d2 the iteration evaluates, t0 among them) ends the item in
 * band: lengths is the state before that visit, lnl the value that is not finite, passes the negated index of the pass (from 1).
 * The engine is never switched to rescaling, under PHYAMD_RESCALE_NEVER and _AUTO alike.
 *   After pass p: lnl_p is lnL at the current lengths (lnl_0 that of the start, which initial_lnl reports).  The item stops when
 * lnl_p - lnl_(p-1) <= lnl_tolerance, with passes = p; after max_passes passes without that, with passes = -max_passes.  With
 * nothing to visit passes = 0 and lnl = initial_lnl.
 *   The root's two children are not special: for a reversible model only their sum matters, and a caller who wants the
 * reference's convention sends one of them with optimise = 0.
 * lnl and the derivatives of a visit are formed from the eigen system like phyamd_nni_optimize's (without the reference's fabs on
 * P(t): a rounding difference); initial_lnl is phyamd_gradient_batch_trees' lnl of the start.  initial_lnl and passes may be NULL.
 * The engine -- its topology, lengths, partials -- is unchanged and later evaluations return the bits they would have returned
 * without the call; two calls return identical bits; an item's bits do not depend on `count`, its position, the other items, the
 * chunks the items ran in, the optional outputs or what the batch scratch held.  The scratch is the batch scratch's: per item the
 * lnL-only walk's of phyamd_gradient_batch_trees and a partial per node; items that do not fit the memory cap together run in chunks.
 * Every item is validated on the host before anything is launched, with its index in the message.  There is no fallback path:
 * PHYAMD_EUNSUPPORTED, naming the condition, under phyamd_gradient_batch_trees' conditions (not 4 states, more than 8 categories, an
 * engine that is rescaling now, tiled patterns, a tip cell with an empty state mask, explicit node matrices, scratch of one item
 * that does not fit the memory cap), for flags other than 0, and on a handle sharded over several devices (every iteration would
 * need a sum across the shards).  PHYAMD_EINVAL: null engine, branch_lengths, lengths or lnl; only some of left / right / roots
 * null; count < 1; no eigen system; bounds that are not 0 <= lower < upper < inf; a tolerance that is not finite and positive;
 * max_iterations outside 1..1000; an lnl_tolerance that is negative or not finite; max_passes outside 1..1000; an invalid tree; a
 * negative or non-finite start length of a visited node. */
int phyamd_optimize_branch_lengths(phyamd_engine *e, int flags, int32_t count,
                                   const int32_t *left, const int32_t *right, const int32_t *roots, /* [count][2T-1], [count]; or all NULL */
                                   const double *branch_lengths /* [count][2T-1] */, const uint8_t *optimise /* [count][2T-1] or NULL */,
                                   double lower, double upper, double tolerance, int32_t max_iterations,
                                   double lnl_tolerance, int32_t max_passes,
                                   double *lengths /* [count][2T-1] */, double *lnl /* [count] */,
                                   double *initial_lnl /* [count] or NULL */, int32_t *passes /* [count] or NULL */);
/* of the last phyamd_optimize_branch_lengths: items, chunks of items they ran in, the most passes a chunk ran, visits made and
 * proposals made over all items, bytes of batch scratch the engine holds (see phyamd_batch_profile), wall time of the call */
typedef struct { int32_t items, chunks, passes; int64_t visits, iterations, scratch_bytes; double ms; } phyamd_branch_optimize_profile;
int phyamd_get_branch_optimize_profile(phyamd_engine *e, phyamd_branch_optimize_profile *out);
/* One pass of phyamd_optimize_branch_lengths over a tree as the device runs it, from the host schedule alone (no device, no
 * engine): a depth-first tour that, on entering an internal node, forms what meets each child's branch from above (O), and on
 * leaving it forms the node's lower partial (p) again and visits it.  The ops in launch order, six ints each:
 *   0 the index of the visit the op belongs to (an op that is no visit runs in front of that visit) |
 *   1 kind: 0 forms O of a node, 1 forms p of an internal node, 2 is the visit of a node |
 *   2 the node |
 *   3, 4 operands -- kind 0: the node's parent, whose O and matrix are read (-3: the parent is the root, which has no O), and its
 *        sibling, whose message is read; kind 1: the node's left and right child, whose messages are read; kind 2: the plane of
 *        the node's O and of its p (-1: a tip, whose p is its data) |
 *   5 the plane written: node for O of a node, 2T-1 + (node - T) for p of an internal node, -1 for a visit.
 * A message of a node reads its matrix and, for an internal node, its p.  Every node but the root is visited once, in post-order
 * (left subtree, right subtree, node); a visit changes the node's length, that is its matrix.  Returns the number of ops,
 * 5 T - 6 (at most `capacity` of them are written), or a negative PHYAMD_E* code. */
int phyamd_branch_sweep_schedule(int32_t tip_count, const int32_t *left /* [2T-1] */, const int32_t *right, int32_t root,
                                 int32_t *out /* [capacity][6] */, int32_t capacity);

/* --- the three graft branches of every SPR regraft --- */
/* The three branches that meet at the graft point of every SPR regraft optimised in one call: what a likelihood SPR search
 * compares (the reference's optimize_tripod after every SPR_move, spropt.c:1538-1623).  Rows, columns and the move are
 * phyamd_spr_log_likelihoods': row i is the prune node p = prune[i] (prune == NULL: count must be 2T-1 and row i is node i), column
 * w the target edge, u = parent(p) the new central node, and the candidates and their rearranged trees are the same.  Per cell
 * lengths holds (t_p, t_w, t_u), lnl the log-likelihood there, initial_lnl that of the start and passes the pass count; every
 * cell that is no candidate is NaN in lengths, lnl and initial_lnl and 0 in passes, and a row whose p is the root or a child of the
 * root is all NaN.  initial_lnl and passes may be NULL.
 * THE RULE.  Entry (p, w) is, by definition, what phyamd_optimize_branch_lengths returns for ONE item whose tree is the rearranged
 * tree of the entry, whose branch_lengths are that tree's -- t'_s = t_s + t_u, t'_u = t'_w = 0.5 t_w, everything else the
 * engine's -- and whose optimise marks p, w and u only.  Spelled out: the state is (t_p, t_w, t_u), at the start
 * (t_p, 0.5 t_w, 0.5 t_w) of the engine's lengths.
 *   A pass visits u's left child, u's right child, then u; in the rearranged tree p keeps its slot and w has the slot s had.
 *   A visit of branch z: f(t) = (lnL, d1, d2) of the rearranged tree with t_z = t and the other two lengths as they stand now, d1 and
 * d2 by phyamd_branch_hessian_diagonal's definitions.  t0 = clamp(t_z, lower, upper).  t' comes from phyamd_nni_optimize's rule
 * started at t0: t = t0, a = lower, b = upper; each iteration evaluates d1(t) and d2(t); if d1 > 0 then a = t, else b = t; it
 * proposes t' = t - d1 / d2 when d2 < 0 and a < t' < b, otherwise t' = (a + b) / 2; it stops when |t' - t| <= tolerance or after
 * max_iterations proposals.  The visit accepts t_z = t' when lnL(t') is finite and lnL(t') >= lnL(t0); otherwise t_z = t0.  So lnL
 * never falls from visit to visit.
 *   lnl_0 is lnL at the start, which initial_lnl reports: phyamd_spr_log_likelihoods' entry up to rounding.  After pass k, lnl_k is
 * lnL at the current lengths.  The entry stops after pass k when lnl_k - lnl_(k-1) <= lnl_tolerance, with passes = k; after
 * max_passes passes without that, with passes = -max_passes.
 *   A lnL that is not finite at an iterate (one of the t whose d1 and d2 the iteration evaluates, t0 among them) ends the entry in
 * band: lengths is the state before that visit, lnl the value that is not finite, passes the negated index of the pass (from 1).
 * The engine is never switched to rescaling, under PHYAMD_RESCALE_NEVER and _AUTO alike.
 * lnL and the derivatives are formed from the eigen system like phyamd_nni_optimize's (without the reference's fabs on P(t): a
 * rounding difference; a category of rate zero behaves as it does there).  Everything happens on the device after the SPR call's
 * one walk per row: the three messages that meet at u -- p's lower, w's lower and w's upper in the pruned tree -- depend on none of
 * the three lengths, so an entry's whole iteration runs in one workgroup without a further walk, matrix launch or host round trip.
 * The engine -- its topology, lengths, partials -- is unchanged and later evaluations return the bits they would have returned
 * without the call; two calls return identical bits; an entry's bits do not depend on count, the row's position in prune, the other
 * rows or candidates, the chunks the rows ran in, the optional outputs or what the batch scratch held.  The scratch is the batch
 * scratch's: per row phyamd_spr_log_likelihoods' and per candidate 2 x C x 4 doubles per pattern; rows that do not fit the memory
 * cap together run in chunks of rows.  There is no fallback path: PHYAMD_EUNSUPPORTED, naming the condition, under
 * phyamd_gradient_batch_trees' conditions (not 4 states, more than 8 categories, an engine that is rescaling now, tiled patterns, a
 * tip cell with an empty state mask, explicit node matrices), for flags other than 0, on a handle sharded over several devices
 * (every iteration would need a sum across the shards), and when the scratch of one row does not fit the memory cap.
 * PHYAMD_EINVAL: null engine, lengths or lnl; count < 1; prune == NULL with another count than 2T-1; an id outside 0..2T-2 (with its
 * index in the message); no eigen system; bounds that are not 0 <= lower < upper < inf; a tolerance that is not finite and
 * positive; max_iterations outside 1..1000; an lnl_tolerance that is negative or not finite; max_passes outside 1..1000. */
int phyamd_spr_optimize(phyamd_engine *e, int flags, int32_t count, const int32_t *prune /* [count] or NULL */,
                        double lower, double upper, double tolerance, int32_t max_iterations,
                        double lnl_tolerance, int32_t max_passes,
                        double *lengths /* [count][2T-1][3]: t_p, t_w, t_u */, double *lnl /* [count][2T-1] */,
                        double *initial_lnl /* [count][2T-1] or NULL */, int32_t *passes /* [count][2T-1] or NULL */);
/* of the last phyamd_spr_optimize or phyamd_spr_optimize_general: rows asked for, chunks of rows they ran in, candidates optimised, visits made and proposals made
 * over all of them, bytes of batch scratch the engine holds (see phyamd_batch_profile), wall time of the call */
typedef struct { int32_t prunes, chunks; int64_t candidates, visits, iterations, scratch_bytes; double ms; } phyamd_spr_optimize_profile;
int phyamd_get_spr_optimize_profile(phyamd_engine *e, phyamd_spr_optimize_profile *out);

/* --- the maximum-likelihood distance of pairs of taxa --- */
/* The ML distance of `count` pairs of taxa under the engine's own model (eigen system, frequencies, category rates and proportions,
 * ambiguity masks), before any topology exists: what a distance method (NJ, UPGMA) builds a starting tree from, where the
 * reference's closed forms (distancematrix.c: uncorrected, JC69, K2P) ignore the model.  pairs [count][2] holds (i, j), i != j, both
 * in 0..T-1; pairs == NULL: count must be T(T-1)/2 and the entries are (0,1), (0,2), ..., (T-2,T-1).  i is the side that carries
 * pi; nothing assumes reversibility.
 * For a pair and a length t, pattern k has L_k(t) = sum_c w_c sum_a (V^T (pi o m_i))_a (V^-1 m_j)_a exp(lambda_a r_c t) with m_i, m_j
 * the two 0/1 state masks: the two-tip tree of phyamd_log_likelihood with one branch of length t.  L_k depends on k only through
 * the pair of masks, so with the weighted table N[mi][mj] = sum_k w_k [mask_i[k] = mi][mask_j[k] = mj] (16 x 16, masks as 4-bit
 * numbers, bit s = state s), S_n[a](t) = sum_c w_c (lambda_a r_c)^n exp(lambda_a r_c t) and G[mi][mj][a] = (V^T (pi o mi))_a (V^-1 mj)_a:
 *   F_n[mi][mj] = sum_a G[mi][mj][a] S_n[a],  lnL = sum N log F_0,  d1 = sum N F_1 / F_0,  d2 = sum N (F_2 / F_0 - (F_1 / F_0)^2),
 * the sums over the bins with N > 0.  f(t) = (lnL, d1, d2).
 * THE RULE, per pair, is phyamd_nni_optimize's (see there) on this f: start is start[p] or, with start NULL, 0.1.  distances[p] = t*;
 * lnl, d1 and d2 are evaluated at t*; iterations has phyamd_nni_optimize's sign convention; a lnL that is not finite at an iterate
 * ends the pair in band exactly as there.  Identical rows end at lower and saturated pairs at upper: results, not errors.  lnl, d1,
 * d2 and iterations may be NULL.  counts [count][16][16], if given, receives the tables N (counts[p][mi][mj]): the sufficient
 * statistic of every count-based distance as well (physher_amd/distances.py: p-distance, JC69, K2P).  With distances == NULL and
 * counts given the call ONLY COUNTS: it needs no eigen system, frequencies or rates, and ignores start, the bounds, the tolerance and
 * max_iterations.
 * The call needs tip data for every tip and the pattern weights, and for distances the eigen system, the frequencies and the
 * category rates and proportions.  It needs no topology and no branch lengths and reads no partials: it works before
 * phyamd_set_topology, on an engine that is rescaling, and with any number of categories.  The tables are formed on the matrix pipe
 * over segments of 4096 patterns added in order, a pair's whole iteration runs in one workgroup, and nothing is added with atomics:
 * the engine is unchanged and later evaluations return the bits they would have returned without the call; two calls return identical
 * bits; a pair's bits do not depend on the other pairs, on its position in the list, on the chunks the pairs ran in or on which
 * optional outputs are asked for.  The scratch is the batch scratch's, per pair 2 KB per segment and 2 KB; pairs that do not fit the
 * memory cap together run in chunks.  PHYAMD_EUNSUPPORTED, naming the condition: not 4 states, tiled patterns, a tip cell with an
 * empty state mask, a handle sharded over several devices (the tables would add up across the shards: not built), flags other than
 * 0, scratch of one pair that does not fit the memory cap.  PHYAMD_EINVAL: null engine; neither distances nor counts; lnl, d1, d2 or
 * iterations without distances; count < 1, or another count than T(T-1)/2 with pairs NULL; an index outside 0..T-1 or i == j; a tip
 * without data; no pattern weights; for distances a missing eigen system, frequencies or rates, and phyamd_nni_optimize's conditions
 * on the bounds, the tolerance, max_iterations and the start values. */
int phyamd_pairwise_distances(phyamd_engine *e, int flags, int32_t count, const int32_t *pairs /* [count][2] or NULL: all i<j, row-major */,
                              const double *start /* [count] or NULL: 0.1 */, double lower, double upper, double tolerance, int32_t max_iterations,
                              double *distances /* [count] or NULL */, double *lnl /* [count] or NULL */, double *d1, double *d2 /* or NULL */,
                              int32_t *iterations /* or NULL */, double *counts /* [count][16][16] or NULL */);
/* of the last phyamd_pairwise_distances: pairs asked for, chunks of pairs they ran in, segments of the pattern axis, bytes of batch
 * scratch the engine holds (see phyamd_batch_profile), proposals made over all pairs, wall time of the call */
typedef struct { int32_t pairs, chunks, segments; int64_t scratch_bytes, iterations; double ms; } phyamd_distance_profile;
int phyamd_get_distance_profile(phyamd_engine *e, phyamd_distance_profile *out);
/* phyamd_pairwise_distances for an engine of 20 states (proteins under WAG / LG + Gamma: the classical use of ML distances, where the
 * reference has Kimura's -log(1 - p - 0.2 p^2) alone): the same pairs, the same likelihood, THE SAME RULE word for word (start 0.1,
 * the sign convention of iterations, a lnL that is not finite ends the pair in band, identical rows end at lower and saturated pairs
 * at upper as results) and the same outputs, with the tables over tip CLASSES instead of masks.  A tip cell's class is the code the
 * engine stores for it: 0..19 the state; 20 unknown (all states: a state code >= 20, or partials that are all 1); 21 + q the
 * engine's ambiguity set q, the sets numbered in the order in which phyamd_set_tip_partials first met them on this engine.  With m_c
 * the 0/1 vector of class c, L_k(t) = sum_c w_c sum_a (V^T (pi o m_ci))_a (V^-1 m_cj)_a exp(lambda_a r_c t),
 * N[ci][cj] = sum_k w_k [class_i[k] = ci][class_j[k] = cj] (32 x 32), S_n[a] as above for a < 20, G[ci][cj][a] = (V^T (pi o m_ci))_a
 * (V^-1 m_cj)_a, and F_n, lnL, d1 and d2 as above over the bins with N > 0; the bins of class 20 are computed like every other bin.
 * counts [count][32][32], if given, receives the tables (counts[p][ci][cj]).  class_members [32], if given, receives one bit per
 * member state of each class: 1 << c for a state, 2^20 - 1 for class 20, the set's members for 21 + q, 0 for a class no set stands
 * for.  The numbering of the sets is the engine's own, so class_members is what gives counts its meaning (physher_amd/distances.py:
 * state_counts_general, p_distance_general, kimura_protein).  With distances == NULL and counts given the call only counts, as above.
 * What the call needs and what it leaves alone are phyamd_pairwise_distances': no topology, no lengths, no partials; a rescaling
 * engine and any number of categories; segments of 4096 patterns added in order, no atomics, the engine unchanged, identical bits
 * from two calls, a pair's bits independent of the other pairs, its position, the grouping of pairs into waves, the chunks and the
 * optional outputs.  The scratch is the batch scratch's, per pair 8 KB per segment and 8 KB.  PHYAMD_EUNSUPPORTED, naming the
 * condition: a state count other than 20 (4: use phyamd_pairwise_distances; 60 / 61: 64 x 64 tables are not built), more than 11
 * ambiguity sets recorded on the engine (a class is below 32), a recorded set with no member (tip partials that are all 0), tiled
 * patterns, a handle sharded over several devices, flags other than 0, scratch of one pair that does not fit the memory cap.
 * PHYAMD_EINVAL: as for phyamd_pairwise_distances.  phyamd_get_distance_profile reports the last distance call of either kind. */
int phyamd_pairwise_distances_general(phyamd_engine *e, int flags, int32_t count, const int32_t *pairs /* [count][2] or NULL: all i<j, row-major */,
                                      const double *start /* [count] or NULL: 0.1 */, double lower, double upper, double tolerance, int32_t max_iterations,
                                      double *distances /* [count] or NULL */, double *lnl, double *d1, double *d2 /* [count] or NULL */,
                                      int32_t *iterations /* or NULL */, double *counts /* [count][32][32] or NULL */,
                                      uint64_t *class_members /* [32] or NULL */);

/* --- query sequences placed on every edge of the engine's tree --- */
/* lnL of `queries` sequences that are NOT among the engine's taxa, each placed on every edge of the engine's tree, in one call:
 * phylogenetic placement (EPA / pplacer style: reads scored on a fixed reference tree) and stepwise addition (a tree grown one taxon
 * at a time).
 * THE DEFINITION.  An edge is a non-root node n of the engine's tree, meaning the branch above it with length t_n.  Placing query x
 * on n with the split sigma in [0, 1] and the pendant length l > 0 is the tree with T + 1 tips in which a new internal node z takes
 * n's place under n's parent; z has the children n and x; n's branch becomes sigma t_n, z's branch (1 - sigma) t_n and x's branch l;
 * every other length, the models and the pattern weights are the engine's.  lnl[i][q][n] is the log-likelihood of that tree
 * (phyamd_log_likelihood's) under pendant[i].  Both children of the root are edges by this same definition; the root's column holds
 * NaN.  sigma = 0.5 and l = t_x is the reference's SPR_move of x onto n (phyamd_spr_log_likelihoods on the tree that holds x).
 * masks [queries][P] holds per query and pattern a 4-bit state mask 1..15 (bit s = state s; 15: a gap; phyamd_set_tip_states' tip
 * encoding).  THE MASKS REFER TO THE ENGINE'S OWN PATTERNS: the caller compresses the reference alignment and the queries jointly
 * (a column of the joint alignment is a pattern, and the engine's weights count the joint columns), or not at all.
 * best_node [lengths][queries], if given, receives per (length, query) the smallest node id with the largest lnL (a later edge
 * replaces an earlier one only when its lnL is strictly larger; the root is never chosen) and best_lnl, if given, that lnL.  They
 * are formed on the device: with lnl == NULL only 2 lengths queries numbers come back instead of [lengths][queries][2T-1].
 * The tree side is independent of the query: one walk of the engine's tree (phyamd_nni_log_likelihoods') leaves what every edge
 * contributes, and a query enters a pattern only through its mask, so per (pendant length, edge, pattern) the 16 possible weighted
 * log site likelihoods are tabulated once and a (query, edge) score is a gather-and-add over the patterns: no walk, matrix, exp or log
 * per query.  The patterns are added in order inside fixed segments of 4096 and the segments in order; nothing is added with
 * atomics: the engine's tree, lengths and partials are unchanged and later evaluations return the bits they would have returned
 * without the call; two calls return identical bits; a (length, query, edge) result does not depend on the other queries, on their
 * order, or on the chunks of edges and queries the call ran in under the memory cap.  An lnL that underflows is -inf in band (the
 * call does not rescale).
 * PHYAMD_EINVAL: null lnl and best_node; best_lnl without best_node; null masks or pendant; queries < 1 or lengths < 1; a split
 * outside [0, 1] or not finite; a pendant length that is not finite or not > 0; null engine; a mask byte of 0 or above 15 (the query
 * and the pattern are named); no eigen system; an engine that is not ready to evaluate.  PHYAMD_EUNSUPPORTED, naming the
 * condition: a handle sharded over several devices, flags other than 0, not 4 states, more than 8 categories, an engine that is
 * rescaling, tiled patterns, a tip cell with an empty state mask, explicit node matrices, scratch of one query on one edge that
 * does not fit the memory cap.  The argument checks come before the handle's state is looked at. */
int phyamd_placement_log_likelihoods(phyamd_engine *e, int flags, int32_t queries,
                                     const uint8_t *masks /* [queries][P]: 4-bit state masks 1..15 over the engine's patterns */, int32_t lengths,
                                     const double *pendant /* [lengths] */, double split,
                                     double *lnl /* [lengths][queries][2T-1] or NULL; NaN in the root's column */,
                                     int32_t *best_node /* [lengths][queries] or NULL */, double *best_lnl /* [lengths][queries] or NULL */);
/* of the last phyamd_placement_log_likelihoods: queries and pendant lengths asked for, edges of the tree (2T-2), chunks of edges the
 * tables were built in, chunks of queries scored against each, bytes of batch scratch the engine holds (see phyamd_batch_profile),
 * wall time of the call */
typedef struct { int32_t queries, lengths, edges, edge_chunks, query_chunks; int64_t scratch_bytes; double ms; } phyamd_placement_profile;
int phyamd_get_placement_profile(phyamd_engine *e, phyamd_placement_profile *out);

/* --- the three branches around chosen placements --- */
/* The three branches that meet at the insertion point of `count` chosen placements optimised in one call: what a placement tool
 * (EPA-ng's branch triplet, pplacer, RAxML-EPA) or a stepwise addition runs on the few best edges per query after
 * phyamd_placement_log_likelihoods has scored all of them, and where its likelihood weight ratios and pendant lengths come from.
 * queries and masks are phyamd_placement_log_likelihoods'.  Candidate i is the query q = candidates[i][0] on the edge
 * n = candidates[i][1], a non-root node.  Per candidate lengths holds (distal t_n, pendant t_x, proximal t_z), lnl the
 * log-likelihood there, initial_lnl that of the start and passes the pass count.  initial_lnl and passes may be NULL.  Duplicates
 * among the candidates are allowed.
 * THE RULE.  The tree of candidate i is the placed tree of phyamd_placement_log_likelihoods' definition: T + 1 tips, a new node z in
 * n's place with the left child n and the right child x (the query).  The start is t_n = split t_n (distal),
 * t_x = pendant_start[i] (pendant; pendant_start NULL: 0.1) and t_z = (1 - split) t_n (proximal), t_n on the right sides the engine's.
 * Entry i is, by definition, what phyamd_optimize_branch_lengths returns for ONE item with that tree and those start lengths whose
 * optimise marks the nodes chosen by `branches`: bit 0 n (distal), bit 1 x (pendant), bit 2 z (proximal).  A pass visits the marked
 * ones in the order n, x, z (z's left child, its right child, z).  The visit, its safeguarded Newton iteration and its acceptance,
 * the stop test after a pass (passes = k, or -max_passes), the end in band at an lnL that is not finite (lengths the state before
 * that visit, lnl the value, passes the negated pass index) and how lnL and the derivatives are formed are phyamd_spr_optimize's
 * (see there), with (t_n, t_x, t_z) for its (t_w, t_p, t_u).  A branch that is not marked is never clamped or changed and comes back
 * as its start value, bit for bit.  initial_lnl is lnL at the start: phyamd_placement_log_likelihoods' entry at that pendant length
 * and split, up to rounding.  branches = 7 is the EPA-ng / optimize_tripod form; branches = 2 optimises the pendant length alone.
 * Everything happens on the device after phyamd_placement_log_likelihoods' one walk of the engine's tree: the three messages that
 * meet at z -- the query's mask vector, n's lower partial and what n's edge sees from above -- depend on none of the three lengths
 * and only the first on the query, so the third is formed once per distinct edge, and a candidate's whole iteration runs in one
 * workgroup without a further walk, matrix launch or host round trip.  The engine -- its topology, lengths, partials -- is unchanged
 * and later evaluations return the bits they would have returned without the call; two calls return identical bits; a candidate's
 * bits do not depend on count, its position, the other candidates or queries, the chunks the candidates ran in, the optional
 * outputs or what the batch scratch held.  Nothing is added with atomics.  The engine is never switched to rescaling.  The scratch
 * is the batch scratch's: phyamd_nni_log_likelihoods' walk, per candidate C x 4 doubles per padded pattern and per distinct edge of
 * a chunk as much again; candidates that do not fit the memory cap together run in chunks.  There is no fallback path:
 * PHYAMD_EUNSUPPORTED, naming the condition, under phyamd_placement_log_likelihoods' conditions (not 4 states, more than 8
 * categories, an engine that is rescaling, tiled patterns, a tip cell with an empty state mask, explicit node matrices, a handle
 * sharded over several devices, flags other than 0) and when the scratch of one candidate does not fit the memory cap.
 * PHYAMD_EINVAL, naming the function and the argument: null masks, candidates, lengths or lnl; queries < 1 or count < 1; a
 * candidate's query outside 0..queries-1 (with its index); branches outside 1..7; a split outside [0, 1]; a start that is not finite
 * and > 0; phyamd_spr_optimize's conditions on the bounds, tolerances and counts; null engine; a candidate's node outside 0..2T-2
 * or equal to the root (with its index); a mask byte of 0 or above 15 (the query and the pattern are named); no eigen system.  The
 * argument checks come before the handle is looked at. */
int phyamd_placement_optimize(phyamd_engine *e, int flags, int32_t queries,
                              const uint8_t *masks /* [queries][P], 1..15, as phyamd_placement_log_likelihoods */,
                              int32_t count, const int32_t *candidates /* [count][2]: (query, node) */,
                              const double *pendant_start /* [count] or NULL: 0.1 */, double split,
                              int32_t branches /* bit 0: distal (n's), bit 1: pendant (the query's), bit 2: proximal (z's); 1..7 */,
                              double lower, double upper, double tolerance, int32_t max_iterations,
                              double lnl_tolerance, int32_t max_passes,
                              double *lengths /* [count][3]: distal, pendant, proximal */, double *lnl /* [count] */,
                              double *initial_lnl /* [count] or NULL */, int32_t *passes /* [count] or NULL */);
/* of the last phyamd_placement_optimize or phyamd_placement_optimize_general: candidates asked for, distinct edges among them, chunks of candidates they ran in, visits
 * made and proposals made over all of them, bytes of batch scratch the engine holds (see phyamd_batch_profile), wall time of the
 * call */
typedef struct { int32_t candidates, edges, chunks; int64_t visits, iterations, scratch_bytes; double ms; } phyamd_placement_optimize_profile;
int phyamd_get_placement_optimize_profile(phyamd_engine *e, phyamd_placement_optimize_profile *out);

/* --- query sequences placed on every edge, 20 states --- */
/* phyamd_placement_log_likelihoods for an engine of 20 states (proteins): its definition word for word -- the edge n, the new node z
 * in n's place with the children n (branch sigma t_n) and the query (branch pendant[i]), z's branch (1 - sigma) t_n, NaN in the
 * root's column, best_node the smallest node id with the largest lnL -- with another vector for the query.  A cell of codes
 * [queries][P] is a CLASS code: 0..19 a state, 20 unknown (all states), 21 + q the CALLER's set sets[q] (bit s = state s is a
 * member; set_count <= 11, so every code is below 32).  The sets are the call's own and not the numbering phyamd_set_tip_partials
 * records for the engine's tips: a query is not an engine tip.  THE CODES REFER TO THE ENGINE'S OWN PATTERNS, as in the 4-state call.
 * The tree side is read from resident partials: THE ENGINE IS AFTERWARDS ONE WITH phyamd_set_keep_partials(1) THAT HAS RUN THE
 * FLAGS-0 GRADIENT (as after phyamd_state_posteriors); its topology, lengths and models are unchanged, a call on an engine already
 * in that state changes nothing, and later evaluations return the bits they would have returned.  Per edge the upper partial (the
 * message at the top of n's branch) and the node's own partial meet the split matrices, and a query enters a pattern only through
 * its class, so per (pendant length, edge, pattern) the 32 possible weighted log site likelihoods are tabulated once -- three
 * 20-wide products per (edge, category, 16 patterns) on the fp64 matrix cores, the categories added in category order -- and a
 * (query, edge) score is a gather-and-add over the patterns: in order inside fixed segments of 4096, the segments in order, no
 * atomics.  Two calls return identical bits; a (length, query, edge) result does not depend on the other queries, on their order,
 * on whether lnl is asked for, or on the chunks of edges and queries the call ran in under the memory cap.  An lnL that underflows
 * is -inf in band and reaches only the queries whose cells select the underflowed entries (the call does not rescale).
 * PHYAMD_EINVAL, naming the function and the argument: phyamd_placement_log_likelihoods' argument conditions (codes for masks);
 * set_count outside 0..11; null sets with set_count > 0; a set word of 0 or with bits at or above 2^20; a code above 20 + set_count
 * (the query and the pattern are named); no eigen system; an engine that is not ready to evaluate.  PHYAMD_EUNSUPPORTED, naming
 * the condition: a state count other than 20 (4: use phyamd_placement_log_likelihoods; 60 / 61: not built), more than 8 categories,
 * an engine that is rescaling -- also when PHYAMD_RESCALE_AUTO switched it on during the call's own evaluation --, tiled patterns,
 * explicit node matrices, a handle sharded over several devices, flags other than 0, scratch of one query on one edge that does
 * not fit the memory cap.  The argument checks come before the handle's state is looked at.  phyamd_get_placement_profile reports
 * the last placement call of either kind. */
int phyamd_placement_log_likelihoods_general(phyamd_engine *e, int flags, int32_t queries,
                                             const uint8_t *codes /* [queries][P]: class codes over the engine's patterns */,
                                             int32_t set_count, const uint64_t *sets /* [set_count] member words, or NULL with set_count 0 */,
                                             int32_t lengths, const double *pendant /* [lengths] */, double split,
                                             double *lnl /* [lengths][queries][2T-1] or NULL; NaN in the root's column */,
                                             int32_t *best_node /* [lengths][queries] or NULL */, double *best_lnl /* [lengths][queries] or NULL */);

/* --- the three branches around chosen placements, 20 states --- */
/* phyamd_placement_optimize for an engine of 20 states (proteins): the second half of the pair that
 * phyamd_placement_log_likelihoods_general opens -- the distal, pendant and proximal branch of `count` chosen (query, edge)
 * placements optimised in one call.  queries, codes, set_count and sets are phyamd_placement_log_likelihoods_general's: a cell of
 * codes [queries][P] is a CLASS code over the engine's own patterns, 0..19 a state, 20 unknown (all states), 21 + q the CALLER's set
 * sets[q] (bit s = state s is a member; set_count <= 11).  Candidate i is the query q = candidates[i][0] on the edge
 * n = candidates[i][1], a non-root node.  Per candidate lengths holds (distal t_n, pendant t_x, proximal t_z), lnl the
 * log-likelihood there, initial_lnl that of the start and passes the pass count.  initial_lnl and passes may be NULL.  Duplicates
 * among the candidates are allowed.
 * THE RULE, in full (it is phyamd_placement_optimize's, word for word; that call defines it through
 * phyamd_optimize_branch_lengths, which does not exist for 20 states).  The tree of candidate i is the placed tree: T + 1 tips, a
 * new node z in n's place with the left child n and the right child x (the query), everything else the engine's.  The model is the
 * engine's eigen system, P(t r_c) = |V e^(lambda t r_c) V^-1| elementwise, and the query's vector at a pattern is the 0/1 member
 * vector of its class code.  The start is t_n = split t_n (distal), t_x = pendant_start[i] (pendant; pendant_start NULL: 0.1) and
 * t_z = (1 - split) t_n (proximal), t_n on the right sides the engine's.  initial_lnl is lnL of the placed tree at the start, the
 * lengths as they are given (not clamped): phyamd_placement_log_likelihoods_general's entry at that pendant length and split, up
 * to rounding.  `branches` marks the branches that are optimised: bit 0 n (distal), bit 1 x (pendant), bit 2 z (proximal).  A PASS
 * visits the marked ones in the order n, x, z (z's left child, its right child, z).  A VISIT of a branch holds the other two
 * lengths where they stand, clamps the branch's length to t_0 in [lower, upper] and runs phyamd_nni_optimize's safeguarded Newton
 * iteration on lnL(t) of the placed tree: with the bracket [lo, hi] = [lower, upper] and t = t_0, evaluate lnL, d1 = dlnL/dt and
 * d2 = d2lnL/dt2 at t; lo = t if d1 > 0, else hi = t; the proposal is t - d1 / d2 if d2 < 0 and it lies strictly inside
 * (lo, hi), else the midpoint (lo + hi) / 2; the iteration ends when the proposal moves by no more than `tolerance` or after
 * max_iterations proposals, and the last proposal is the visit's candidate length t_1.  The visit keeps t_1 if lnL(t_1) is
 * finite and not below lnL(t_0), else it leaves t_0 (the clamped length).  After a pass the STOP TEST: if lnL after the pass
 * minus lnL after the previous pass (the first pass: initial_lnl) is <= lnl_tolerance, the entry ends with passes = k, the
 * number of passes made; else after max_passes passes it ends with passes = -max_passes.  lnl is lnL at the lengths returned.
 * An lnL that is NOT FINITE at an iterate of a visit (some pattern's site likelihood is not in (0, inf): underflow, the call
 * does not rescale) ends the entry IN BAND: lengths are the state before that visit, lnl is the value that is not finite (-inf or
 * NaN) and passes is the negated index of the pass, counted from 1.  A branch that is not marked is never clamped or changed and
 * comes back as its start value, bit for bit.
 * The tree side is read from resident partials, exactly as in phyamd_placement_log_likelihoods_general: THE ENGINE IS AFTERWARDS ONE
 * WITH phyamd_set_keep_partials(1) THAT HAS RUN THE FLAGS-0 GRADIENT; its topology, lengths and models are unchanged, and later
 * evaluations return the bits they would have returned.  The three messages that meet at z -- the query's class vector, n's own
 * partial and pi times the upper partial at the top of n's branch -- depend on none of the three lengths, so a candidate's whole
 * rule runs in one workgroup without a walk, a matrix launch or a host round trip per visit: per visit the coefficients
 * K[c][e] of lnL's exponential sum sum_c sum_e K[c][e] exp(lambda_e r_c t) are formed per pattern with three 20-wide products on
 * the fp64 matrix cores (the query enters through tables over its 32 classes) and every iterate is a fixed-order sum over them.
 * Two calls return identical bits; a candidate's bits depend on the engine's inputs, its query's codes, the sets, its edge and its
 * start, and not on count, its position, the other candidates or queries, the chunks the candidates ran in, the optional outputs
 * or what the batch scratch held.  Nothing is added with atomics.  The engine is never switched to rescaling by the solve.  The
 * scratch is the batch scratch's: per candidate C x 20 doubles per padded pattern and per distinct internal edge of a chunk as
 * much again; candidates that do not fit the memory cap together run in chunks.
 * PHYAMD_EINVAL, naming the function and the argument: null codes, candidates, lengths or lnl; queries < 1 or count < 1; a
 * candidate's query outside 0..queries-1 (with its index); branches outside 1..7; a split outside [0, 1]; a start that is not finite
 * and > 0; bounds that are not 0 <= lower < upper < inf; a tolerance that is not finite and > 0; max_iterations or max_passes
 * outside 1..1000; an lnl_tolerance that is not finite and >= 0; set_count outside 0..11; null sets with set_count > 0; a set word
 * of 0 or with bits at or above 2^20; null engine; a candidate's node outside 0..2T-2 or equal to the root (with its index); a
 * code above 20 + set_count (the query and the pattern are named); no eigen system; an engine that is not ready to evaluate.  The
 * argument checks come before the handle's state is looked at.  There is no fallback path: PHYAMD_EUNSUPPORTED, naming the
 * condition: a state count other than 20 (4: use phyamd_placement_optimize; 60 / 61: not built), more than 8 categories, an engine
 * that is rescaling -- also when PHYAMD_RESCALE_AUTO switched it on during the call's own evaluation --, tiled patterns, explicit
 * node matrices, a handle sharded over several devices, flags other than 0, scratch of one candidate that does not fit the memory
 * cap.  phyamd_get_placement_optimize_profile reports the last call of either kind. */
int phyamd_placement_optimize_general(phyamd_engine *e, int flags, int32_t queries,
                                      const uint8_t *codes /* [queries][P] class codes, as phyamd_placement_log_likelihoods_general */,
                                      int32_t set_count, const uint64_t *sets /* [set_count] member words, or NULL with set_count 0 */,
                                      int32_t count, const int32_t *candidates /* [count][2]: (query, node) */,
                                      const double *pendant_start /* [count] or NULL: 0.1 */, double split,
                                      int32_t branches /* bit 0: distal (n's), bit 1: pendant (the query's), bit 2: proximal (z's); 1..7 */,
                                      double lower, double upper, double tolerance, int32_t max_iterations,
                                      double lnl_tolerance, int32_t max_passes,
                                      double *lengths /* [count][3]: distal, pendant, proximal */, double *lnl /* [count] */,
                                      double *initial_lnl /* [count] or NULL */, int32_t *passes /* [count] or NULL */);

/* --- every NNI neighbour of the engine's tree, 20 states --- */
/* phyamd_nni_log_likelihoods for an engine of 20 states (proteins): lnL, and its first and second derivative in the central
 * branch, of every NNI neighbour of the engine's tree in one call -- O(T) work for the whole neighbourhood, where the loop it
 * replaces (phyamd_set_topology + phyamd_set_branch_length + phyamd_branch_hessian_diagonal on a second engine) walks the tree
 * twice from the tips per entry.
 * THE DEFINITION, in full (it is phyamd_nni_log_likelihoods', word for word).  A CANDIDATE is every internal node v other than the
 * root; u its parent, s its sibling, a = left[v], b = right[v].  Every subtree keeps its own branch length; the length of v is
 * central_lengths[k][v], or the engine's t_v when central_lengths is NULL.  Row k of lnl, d1, d2 ([3][2T-1] each) at column v:
 *   k = 0  the engine's tree
 *   k = 1  a and s exchanged: v gets children (s, b), u gets a where s was
 *   k = 2  b and s exchanged: v gets children (a, s), u gets b where s was
 * Entry (k, v) is what the engine itself returns for the rearranged tree with t_v set to the trial length: lnl[k][v] is
 * phyamd_log_likelihood, d1[k][v] and d2[k][v] are rows v of phyamd_branch_hessian_diagonal's first and second derivative.  (The
 * central branch's transition matrix enters as V e^(lambda t r_c) V^-1 without the reference's elementwise |.|: a rounding
 * difference, as in phyamd_nni_optimize.)  A trial length of 0 is legal.  Columns of tips and of the root are NaN in all three
 * outputs (two tips: everything is NaN); entries of central_lengths at those columns are ignored.  d1 and d2 may be NULL (both NULL:
 * their sums are skipped; the lnl bits are the same).  When u is the root, k = 1 and k = 2 are, for a reversible model, the same
 * unrooted topology with the lengths of a, b and s redistributed; they are computed like every other entry.  An entry whose lnL
 * is not finite (some pattern's site likelihood is not in (0, inf): underflow, the call does not rescale) reports it in band with
 * NaN d1 and d2.
 * The tree side is read from resident partials, exactly as in phyamd_placement_log_likelihoods_general: THE ENGINE IS AFTERWARDS ONE
 * WITH phyamd_set_keep_partials(1) THAT HAS RUN THE FLAGS-0 GRADIENT; its topology, lengths and models are unchanged, and later
 * evaluations return the bits such an engine returns without the call.  Upper partials that a PHYAMD_GRAD_FOLD_ROOT_FREQS
 * keep-partials gradient left resident are used as they are (pi is inside them).  The three arrangements round an edge differ in
 * four messages only, and all four are resident: a stored lower partial is the message P_x p_x itself (a tip: a column, the row sums
 * or a set's columns of its branch matrix), and the parent's is P_u times the upper partial at the top of u's branch (ones at the
 * root).  With F = pi o A_u o m_o and p = m_x o m_y for (o; x, y) = (s; a, b), (a; s, b), (b; a, s) the site likelihood in the central
 * length t is sum_c sum_e K[c][e] exp(lambda_e r_c t), K[c][e] = w_c (V^T F)_e (V^-1 p)_e, so nothing is walked, no trial matrix is
 * formed and the derivatives cost no further product: seven 20-wide products on the fp64 matrix cores per (candidate, category,
 * 16 patterns).  Two calls return identical bits; an entry's bits depend on the engine's inputs and on its own trial length alone
 * -- not on the other entries' lengths, the optional outputs or what the batch scratch held.  Nothing is added with atomics: sums
 * over patterns are formed over blocks of 128 patterns and added in block order.  The engine is never switched to rescaling by the
 * call's own kernels.  The scratch is the batch scratch's: 64 bytes and nine doubles per block per candidate.
 * PHYAMD_EINVAL: null engine or lnl (checked before the handle's state is looked at), no eigen system, a negative or non-finite
 * trial length of a candidate (named), an engine that is not ready to evaluate.  There is no fallback path: PHYAMD_EUNSUPPORTED,
 * naming the function and the condition: a state count other than 20 (4: use phyamd_nni_log_likelihoods; 60 / 61: not built),
 * more than 8 categories, flags other than 0, tiled patterns, explicit node matrices, an engine that is rescaling -- also when
 * PHYAMD_RESCALE_AUTO switched it on during the call's own evaluation --, a handle sharded over several devices, scratch that does
 * not fit the memory cap.  phyamd_get_nni_profile reports the last call of either kind. */
int phyamd_nni_log_likelihoods_general(phyamd_engine *e, int flags, const double *central_lengths /* [3][2T-1] or NULL */,
                                       double *lnl /* [3][2T-1] */, double *d1 /* [3][2T-1] or NULL */, double *d2 /* [3][2T-1] or NULL */);
/* phyamd_nni_optimize for an engine of 20 states (proteins): the central branch of every NNI neighbour of the engine's tree
 * optimised in one call.  A tree search judges an NNI move at its best central length, not at the old one; the routes this replaces
 * are one phyamd_nni_log_likelihoods_general call per Newton round with the rule on the host, or a second engine looped over all
 * 3 (T - 2) entries.
 * THE DEFINITION, in full (it is phyamd_nni_optimize's, word for word).  A CANDIDATE is every internal node v other than the root; u
 * its parent, s its sibling, a = left[v], b = right[v].  Every subtree keeps its own branch length.  Row k of every output
 * ([3][2T-1] each) at column v:
 *   k = 0  the engine's tree
 *   k = 1  a and s exchanged: v gets children (s, b), u gets a where s was
 *   k = 2  b and s exchanged: v gets children (a, s), u gets b where s was
 * and entry (k, v) is the length of v in [lower, upper] that maximises the lnL of that tree, found by THE RULE: t = clamp(start,
 * lower, upper), a = lower, b = upper, where start is start_lengths[k][v] or, with start_lengths NULL, the engine's t_v.  Each
 * iteration evaluates d1(t) and d2(t), the first and second derivative of the entry's lnL in the length of v
 * (phyamd_branch_hessian_diagonal's definitions, row v); if d1 > 0 then a = t, else b = t; it proposes t' = t - d1 / d2 when d2 < 0
 * and a < t' < b, otherwise t' = (a + b) / 2; it stops when |t' - t| <= tolerance, and t* = t'.  iterations[k][v] is the number of
 * proposals made.  After max_iterations proposals without that the entry stops all the same: t* is the last proposal and the count
 * is stored negated.  lengths[k][v] = t*; lnl, d1 and d2 are evaluated at t* and are what phyamd_nni_log_likelihoods_general
 * returns for the entry at central_lengths[k][v] = t*, up to the order of the sum over patterns.  (The central branch's transition
 * matrix enters as V e^(lambda t r_c) V^-1 without the reference's elementwise |.|: a rounding difference.)  A lnL that is not
 * finite at an iterate (some pattern's site likelihood is not in (0, inf): underflow, the call does not rescale) ends the entry in
 * band: lengths holds that iterate, lnl the value that is not finite, d1 and d2 NaN and iterations a negative count.  Columns of
 * tips and of the root hold NaN in the double outputs and 0 in iterations (two tips: everywhere); entries of start_lengths at those
 * columns are not read.  d1, d2 and iterations may be NULL.  When u is the root, k = 1 and k = 2 are, for a reversible model, the
 * same unrooted topology with the lengths of a, b and s redistributed; they are computed like every other entry.
 * The tree side is read from resident partials, exactly as in phyamd_nni_log_likelihoods_general: THE ENGINE IS AFTERWARDS ONE WITH
 * phyamd_set_keep_partials(1) THAT HAS RUN THE FLAGS-0 GRADIENT; its topology, lengths and models are unchanged, and later
 * evaluations return the bits such an engine returns without the call.  Upper partials that a PHYAMD_GRAD_FOLD_ROOT_FREQS
 * keep-partials gradient left resident are used as they are (pi is inside them).  The four messages that meet on a candidate edge
 * do not depend on the central length, so an entry's site likelihood is sum_c sum_e K[c][e] exp(lambda_e r_c t) with
 * K[c][e] = w_c (V^T F)_e (V^-1 p)_e (F and p: see phyamd_nni_log_likelihoods_general).  K is formed once per entry -- seven
 * 20-wide products on the fp64 matrix cores per (candidate, category, 16 patterns) -- and kept in the batch scratch; then one
 * workgroup runs the entry's whole rule, and an iteration costs C x 20 exponentials and a pass over K: nothing is walked, no trial
 * matrix is formed, and no iteration costs a walk, a launch or a host round trip.  Two calls return identical bits; an entry's
 * bits depend on the engine's inputs and on its own start alone -- not on the other entries, the chunks the candidates ran in, the
 * optional outputs or what the batch scratch held.  Nothing is added with atomics: sums over patterns are formed in a fixed order
 * inside the entry's workgroup.  The engine is never switched to rescaling by the call's own kernels.  The scratch is the batch
 * scratch's: per candidate 3 x C x 20 doubles per (padded) pattern and its three entries' results; candidates that do not fit the
 * memory cap together run in chunks.
 * PHYAMD_EINVAL: null engine, lengths or lnl (checked before the handle's state is looked at), no eigen system, bounds that are not
 * 0 <= lower < upper < inf, a tolerance that is not finite and positive, max_iterations outside 1..1000, a negative or non-finite
 * start length of a candidate (named), an engine that is not ready to evaluate.  There is no fallback path: PHYAMD_EUNSUPPORTED,
 * naming the function and the condition: a state count other than 20 (4: use phyamd_nni_optimize; 60 / 61: not built), more than 8
 * categories, flags other than 0, tiled patterns, explicit node matrices, an engine that is rescaling -- also when
 * PHYAMD_RESCALE_AUTO switched it on during the call's own evaluation --, a handle sharded over several devices, scratch of one
 * candidate that does not fit the memory cap.  phyamd_get_nni_optimize_profile reports the last call of either kind. */
int phyamd_nni_optimize_general(phyamd_engine *e, int flags, const double *start_lengths /* [3][2T-1] or NULL: the engine's t_v */,
                                double lower, double upper, double tolerance, int32_t max_iterations,
                                double *lengths /* [3][2T-1] */, double *lnl /* [3][2T-1] */, double *d1 /* [3][2T-1] or NULL */,
                                double *d2 /* [3][2T-1] or NULL */, int32_t *iterations /* [3][2T-1] or NULL */);
/* phyamd_spr_log_likelihoods for an engine of 20 states (proteins): lnL of every SPR regraft of chosen subtrees of the engine's tree
 * in one call.  The route this replaces is a second engine looped over the O(T^2) rearranged trees, each walked from the tips.
 * THE DEFINITION, in full (it is phyamd_spr_log_likelihoods', word for word).  Row i of lnl ([count][2T-1]) belongs to the prune node
 * p = prune[i]; prune == NULL: count must be 2T-1 and row i is node i.  Column w is the target edge, named by the node below it.
 * With u = parent(p), s = sibling(p), g = parent(u), x = parent(w), lnl[i][w] is the log-likelihood of the tree obtained from the
 * engine's arrays by (node ids kept)
 *   g's child slot that held u now holds s, with t'_s = t_s + t_u;
 *   x's child slot that held w now holds u;
 *   u keeps p in its slot and gets w in the slot s had, with t'_u = t'_w = 0.5 t_w;
 * everything else -- the root, t_p -- unchanged.  Entry (i, w) is what the engine itself returns from phyamd_log_likelihood for that
 * tree (the sibling's branch enters as P(t_u r_c) P(t_s r_c), not as the matrix of the summed length: a rounding difference).
 * Column w is a CANDIDATE unless w is the root, u, s, p or a descendant of p; every other column is NaN.  A row is all NaN when p is
 * the root or a child of the root (no error, so that prune == NULL works uniformly).  Duplicates in prune are allowed.  A candidate
 * whose lnL is not finite (some pattern's site likelihood is not in (0, inf): underflow, the call does not rescale) reports it in
 * band.
 * The tree side is read from resident partials, exactly as in phyamd_nni_log_likelihoods_general: THE ENGINE IS AFTERWARDS ONE WITH
 * phyamd_set_keep_partials(1) THAT HAS RUN THE FLAGS-0 GRADIENT; its topology, lengths and models are unchanged, and later
 * evaluations return the bits such an engine returns without the call.  Only LOWER partials are read -- a stored lower is the
 * message P_n p_n itself -- so the result is the likelihood's whether or not a PHYAMD_GRAD_FOLD_ROOT_FREQS gradient left pi inside
 * the resident uppers.  Per row, the messages on the path from u to the root are formed anew (the first is P_u m_s: no merged matrix),
 * then the pruned tree's upper of every internal node outside p's subtree, parent before child; per candidate, category and 16
 * patterns three 20-wide products on the fp64 matrix cores give sum_i pi_i U_i (H_w ((H_w p'_w) o m_p))_i with H_w = P(0.5 t_w r_c).
 * Two calls return identical bits; a row's bits depend on the engine's inputs and on p alone -- not on count, the row's position
 * in prune, the chunk it ran in or what the batch scratch held.  Nothing is added with atomics: sums over patterns are formed over
 * blocks of 128 patterns and added in block order.  The engine is never switched to rescaling by the call's own kernels.  The
 * scratch is the batch scratch's, counted and released like it: per row (T - 1 + D) x C x 20 x Pp x 8 bytes of partials -- the
 * upper of every internal node and D path messages, D the depth of the deepest internal node, Pp the patterns rounded up to 16 --,
 * 64 (T - 1 + D) + 4 bytes of ops, and per node 64 bytes of candidate, 4 of index, 8 of result and 8 per block of 128 patterns;
 * beside the rows, half the engine's lengths with their matrices and images.  Rows that do not fit the memory cap together run in
 * chunks of rows.
 * PHYAMD_EINVAL: null engine or lnl (checked before the handle's state is looked at), count < 1, prune == NULL with another count
 * than 2T-1, an id outside 0..2T-2 (with its index in the message), no eigen system, an engine that is not ready to evaluate.
 * There is no fallback path: PHYAMD_EUNSUPPORTED, naming the function and the condition: a state count other than 20 (4: use
 * phyamd_spr_log_likelihoods; 60 / 61: not built), more than 8 categories, flags other than 0, tiled patterns, explicit node
 * matrices, an engine that is rescaling -- also when PHYAMD_RESCALE_AUTO switched it on during the call's own evaluation --, a
 * handle sharded over several devices, scratch of one row that does not fit the memory cap.  phyamd_get_spr_profile reports the
 * last call of either kind. */
int phyamd_spr_log_likelihoods_general(phyamd_engine *e, int flags, int32_t count, const int32_t *prune /* [count] or NULL */,
                                       double *lnl /* [count][2T-1] */);
/* phyamd_spr_optimize for an engine of 20 states (proteins): the three branches that meet at the graft point of every SPR regraft
 * of chosen subtrees optimised in one call -- what a likelihood SPR search compares after it has scored the regrafts.  The route this
 * replaces is a second engine looped over the O(T^2) rearranged trees with the rule on the host through
 * phyamd_branch_log_likelihood: one walk and one host round trip per iterate.
 * THE DEFINITION, in full.  Rows, columns, candidates and the rearranged tree are phyamd_spr_log_likelihoods_general's: row i belongs
 * to the prune node p = prune[i] (prune == NULL: count must be 2T-1 and row i is node i), column w is the target edge, named by the
 * node below it; with u = parent(p), s = sibling(p), g = parent(u), x = parent(w) the rearranged tree is (node ids kept)
 *   g's child slot that held u now holds s, with t'_s = t_s + t_u;
 *   x's child slot that held w now holds u;
 *   u keeps p in its slot and gets w in the slot s had;
 * everything else unchanged.  Column w is a CANDIDATE unless w is the root, u, s, p or a descendant of p.  Per cell lengths holds
 * (t_p, t_w, t_u), lnl the log-likelihood there, initial_lnl that of the start and passes the pass count; a cell that is no candidate
 * is NaN in lengths, lnl and initial_lnl and 0 in passes, and a row whose p is the root or a child of the root is all NaN.
 * Duplicates in prune are allowed.  initial_lnl and passes may be NULL.
 * THE RULE.  The state is (t_p, t_w, t_u), at the start (t_p, 0.5 t_w, 0.5 t_w) of the engine's lengths.  lnl_0 is lnL of the
 * rearranged tree at the start with the lengths as they are given (not clamped), which initial_lnl reports: up to rounding
 * phyamd_spr_log_likelihoods_general's entry.
 *   A pass visits u's left child, u's right child, then u; in the rearranged tree p keeps its slot and w has the slot s had.  All
 * three branches are always visited.
 *   A visit of branch z: f(t) = (lnL, d1, d2) of the rearranged tree with t_z = t and the other two lengths as they stand now, d1 and
 * d2 the first and second derivative of lnL in t_z.  t0 = clamp(t_z, lower, upper).  t' comes from phyamd_nni_optimize's rule started
 * at t0: t = t0, a = lower, b = upper; each iteration evaluates d1(t) and d2(t); if d1 > 0 then a = t, else b = t; it proposes
 * t' = t - d1 / d2 when d2 < 0 and a < t' < b, otherwise t' = (a + b) / 2; it stops when |t' - t| <= tolerance or after
 * max_iterations proposals.  The visit accepts t_z = t' when lnL(t') is finite and lnL(t') >= lnL(t0); otherwise t_z = t0.  So lnL
 * never falls from visit to visit.
 *   After pass k, lnl_k is lnL at the current lengths.  The entry stops after pass k when lnl_k - lnl_(k-1) <= lnl_tolerance, with
 * passes = k; after max_passes passes without that, with passes = -max_passes.
 *   A lnL that is not finite at an iterate (one of the t whose d1 and d2 the iteration evaluates, t0 among them; some pattern's site
 * likelihood is not in (0, inf): underflow, the call does not rescale) ends the entry in band: lengths is the state before that
 * visit, lnl the value that is not finite, passes the negated index of the pass (from 1).
 * THE MODEL.  The two branches a visit holds enter as P(t r_c) = |V e^(lambda t r_c) V^-1| elementwise, the engine's own matrix
 * arithmetic; the visited branch enters through the eigen sum sum_c sum_e K[c][e] exp(lambda_e r_c t) without the |.| (a rounding
 * difference); the sibling's merged branch enters as P(t_u r_c) P(t_s r_c), not as the matrix of the summed length (a rounding
 * difference, as in phyamd_spr_log_likelihoods_general).
 * The tree side is read from resident partials, exactly as in phyamd_spr_log_likelihoods_general: THE ENGINE IS AFTERWARDS ONE WITH
 * phyamd_set_keep_partials(1) THAT HAS RUN THE FLAGS-0 GRADIENT; its topology, lengths and models are unchanged, and later
 * evaluations return the bits such an engine returns without the call.  Only LOWER partials are read, so a
 * PHYAMD_GRAD_FOLD_ROOT_FREQS gradient changes nothing.  After the scoring call's walk per row, three vectors meet at u and none
 * depends on the three lengths: A, p's own partial; B, w's own partial in the pruned tree; F = pi o U, U the scoring call's
 * (x is the root ? 1 : P_x u'_x) o m'_y.  With K = w_c (V^T F)_e (V^-1 [(P(t_w) B) o (P(t_p) A)])_e for u,
 * w_c (V^T [(P(t_u)^T F) o (P(t_p) A)])_e (V^-1 B)_e for w and the same with A and B exchanged for p, one workgroup runs an entry's
 * whole rule: a visit forms K with four 20-wide products on the fp64 matrix cores per (category, 16 patterns), an iterate costs
 * C x 20 exponentials and a pass over K, and nothing is walked, launched or sent to the host per visit.  Two calls return identical
 * bits; an entry's bits depend on the engine's inputs and on (p, w) alone -- not on count, the row's position in prune, the other
 * rows, the chunks the rows ran in, the optional outputs or what the batch scratch held.  Nothing is added with atomics.  The engine
 * is never switched to rescaling by the call's own kernels.
 * The scratch is the batch scratch's, counted and released like it.  With npd = C x 20 x Pp doubles (Pp the patterns rounded up to
 * 16), D the depth of the deepest internal node and N = 2T-1: per row 8 npd (T - 1 + 2 D + 2 N) bytes -- the scoring call's T - 1
 * uppers and D path messages, D own partials of path nodes, and pi o U and K of at most N candidates -- and 64 (T - 1 + D) + 4 bytes of
 * ops, 56 D of own-partial records, and per node 64 + 32 bytes of candidate records, 4 of index, 24 of start and 40 + 16 + 40 + 12 of
 * results; beside the rows 8 npd (T - 1) bytes, every internal node's own partial, and 56 (T - 1) of records.  Rows that do not fit
 * the memory cap together run in chunks of rows, with the same bits.
 * PHYAMD_EINVAL (the arguments are checked before the handle's state is looked at): null engine, lengths or lnl; count < 1; prune ==
 * NULL with another count than 2T-1; an id outside 0..2T-2 (with its index in the message); no eigen system; bounds that are not
 * 0 <= lower < upper < inf; a tolerance that is not finite and positive; max_iterations outside 1..1000; an lnl_tolerance that is
 * negative or not finite; max_passes outside 1..1000; an engine that is not ready to evaluate.  There is no fallback path:
 * PHYAMD_EUNSUPPORTED, naming the function and the condition: a state count other than 20 (4: use phyamd_spr_optimize; 60 / 61: not
 * built), more than 8 categories, flags other than 0, tiled patterns, explicit node matrices, an engine that is rescaling -- also
 * when PHYAMD_RESCALE_AUTO switched it on during the call's own evaluation --, a handle sharded over several devices, scratch of one
 * row that does not fit the memory cap.  phyamd_get_spr_optimize_profile reports the last call of either kind. */
int phyamd_spr_optimize_general(phyamd_engine *e, int flags, int32_t count, const int32_t *prune /* [count] or NULL */,
                                double lower, double upper, double tolerance, int32_t max_iterations,
                                double lnl_tolerance, int32_t max_passes,
                                double *lengths /* [count][2T-1][3]: t_p, t_w, t_u */, double *lnl /* [count][2T-1] */,
                                double *initial_lnl /* [count][2T-1] or NULL */, int32_t *passes /* [count][2T-1] or NULL */);

#ifdef __cplusplus
}
#endif
#endif
