// phyamd_queries.inc -- the whole-tree query calls on one shard: batches of branch-length vectors, of pattern weights and of trees, NNI and SPR scores, pairwise distances,
// per-pattern posteriors, the full branch Hessian, and the per-pattern lnL of a batch of trees with its RELL replicates.  They read what the engine holds and write only their own scratch
// (part of phyamd_engine.hip: one translation unit, internal linkage)

// ---- what the calls share ------------------------------------------------------------------------------------------------------

// the in-band rule for an evaluation whose lnL is NaN / inf (treelikelihood.c:327-332): everything derived from it is NaN, a
// most probable state 255.  (Per entry, one lnL each: nni_mask_derivatives)
bool not_finite(double lnl) { return std::isnan(lnl) || std::isinf(lnl); }
void mask_if_not_finite(double lnl, double *values, size_t n) {
	if (values && not_finite(lnl)) std::fill(values, values + n, NAN);
}
void mask_states_if_not_finite(double lnl, uint8_t *states, size_t n) {
	if (states && not_finite(lnl)) std::fill(states, states + n, (uint8_t)255);
}

// ready but for the lengths, which the call brings itself
int check_ready_but_lengths(Shard *e) {
	const bool had = e->have_lengths;
	e->have_lengths = true;
	const int rc = check_ready(e);
	e->have_lengths = had;
	return rc;
}

// every partial resident: the engine becomes one with phyamd_set_keep_partials(1) that has run the flags-0 gradient
int require_resident_partials(Shard *e, const char *call) {
	int rc;
	if (!e->keep_partials && (rc = shard_set_keep_partials(e, 1))) return rc;
	if ((!uppers_resident(e) || !lowers_current(e)) && (rc = eval_gradient(e, 0))) return rc;
	if ((rc = require_reference_form(e))) return rc;  // (stored partials: the partials themselves, in the reference's form)
	if (!uppers_resident(e) || e->sched.core_index[e->root] < 0) return fail(PHYAMD_EDEVICE, "%s: the gradient left no resident partials", call);
	return PHYAMD_OK;
}

// The preconditions of the 20-state calls that read the resident partials (the two placement calls, phyamd_place_calls.inc, and
// phyamd_nni_log_likelihoods_general), in two halves: a call may check its own arguments against the engine in between.  The first
// reads the engine's inputs; the second makes every partial resident (require_resident_partials: the engine is afterwards a
// keep-partials engine that has run the flags-0 gradient).  A call words what is its own
struct GeneralQueryCall {
	const char *name;
	const char *built;                  // what "is / are" built for 20 states only
	const char *use_4_state_call;       // the call an engine of 4 states is sent to
	const char *not_built;              // what 60 / 61 states would need and "is / are" not built
	const char *explicit_why;           // why explicit node matrices are refused: "which ..."
	const char *eigen_use;              // what "is / are" formed from the eigen system
	const char *what_does_not_rescale;  // "tables do", "solve does"
};
int check_general_query_inputs(Shard *e, const GeneralQueryCall &call, int flags) {
	const char *name = call.name;
	if (e->S == 4) return fail(PHYAMD_EUNSUPPORTED, "%s: %s built for 20 states (the engine has 4: use %s)", name, call.built, call.use_4_state_call);
	if (e->S != PLACE_GEN_STATES) return fail(PHYAMD_EUNSUPPORTED, "%s: %s built for 20 states (the engine has %d: %s not built)", name, call.built, e->S, call.not_built);
	if (e->C > BATCH_MAX_CATEGORIES) return fail(PHYAMD_EUNSUPPORTED, "%s: %d rate categories (at most %d categories)", name, e->C, BATCH_MAX_CATEGORIES);
	if (flags != 0) return fail(PHYAMD_EUNSUPPORTED, "%s: flags %d (no flags are defined: pass 0)", name, flags);
	if (e->tiles > 1) return fail(PHYAMD_EUNSUPPORTED, "%s: the patterns are tiled and the call needs every partial of all patterns resident", name);
	if (std::any_of(e->explicit_host.begin(), e->explicit_host.end(), [](uint8_t x) { return x != 0; }))
		return fail(PHYAMD_EUNSUPPORTED, "%s: a node has explicit matrices, %s", name, call.explicit_why);
	if (!e->have_eigen) return fail(PHYAMD_EINVAL, "%s needs the eigen system (phyamd_set_eigen): %s formed from it", name, call.eigen_use);
	return check_ready(e);
}
int check_general_query_resident(Shard *e, const GeneralQueryCall &call) {
	static const char *const rescaling = "%s: the engine is rescaling%s and the %s not rescale (underflow is otherwise -inf in band)";
	if (e->scaling_on) return fail(PHYAMD_EUNSUPPORTED, rescaling, call.name, "", call.what_does_not_rescale);
	if (int rc = require_resident_partials(e, call.name)) return rc;
	if (e->scaling_on)
		return fail(PHYAMD_EUNSUPPORTED, rescaling, call.name, " (PHYAMD_RESCALE_AUTO switched it on during the call's own evaluation)", call.what_does_not_rescale);
	if (e->tiles > 1) return fail(PHYAMD_EUNSUPPORTED, "%s: the patterns are tiled and the call needs every partial of all patterns resident", call.name);
	return PHYAMD_OK;
}

// transition matrices of `items` branch-length vectors [items][N] on the device -> mats [items][N][C][16]; roots: per item, or null:
// the engine's
void launch_batch_matrices(Shard *e, int items, const double *lengths, const int32_t *roots, double *mats) {
	const size_t total = (size_t)items * e->N * e->C * 16;
	hipLaunchKernelGGL(k_batch_matrices, dim3((unsigned)std::min<size_t>((total + 255) / 256, 4096)), dim3(256), 0, e->stream, e->C, e->N, items, e->d_model, e->d_rates, lengths,
	                   e->root, roots, mats);
}

size_t batch_scratch_bytes(const Shard *e) { return (size_t)e->batch_mem.bytes; }

// the frame of a call that keeps a profile: the device bound, the body run on `prof` (what the entry point knows beforehand), and
// the profile stored -- also of a call that failed -- with the scratch the call leaves and its wall time
template <typename Prof, typename Body>
int profiled_call(Shard *e, Prof Shard::*slot, Prof prof, Body body) {
	const auto t0 = std::chrono::steady_clock::now();
	int rc;
	if ((rc = bind_device(e))) return rc;
	rc = body(prof);
	prof.scratch_bytes = (int64_t)batch_scratch_bytes(e);
	prof.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
	e->*slot = prof;
	return rc;
}

// ---- a batch of branch-length vectors (phyamd_gradient_batch) ----------------------------------------------------------------

// (the op lists: build_batch_ops, phyamd_tree_schedule.h)

// the engine's own lists (a batch of branch-length vectors), built once per topology
int ensure_engine_batch_ops(Shard *e) {
	if (e->batch_left == e->left && e->batch_right == e->right && e->batch_root == e->root && !e->batch_ops.empty() && e->d_batch_ops.get()) return PHYAMD_OK;
	e->batch_left = e->left;
	e->batch_right = e->right;
	e->batch_root = e->root;
	e->batch_ops.clear();
	e->batch_upper_slots = build_batch_ops(e->T, e->left.data(), e->right.data(), e->root, &e->batch_ops);
	int rc;
	if ((rc = e->d_batch_ops.ensure(e->batch_ops.size()))) {
		e->batch_ops.clear();
		return rc;
	}
	HIP_TRY(hipMemcpyAsync(e->d_batch_ops, e->batch_ops.data(), sizeof(BatchOp) * e->batch_ops.size(), hipMemcpyHostToDevice, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream));
	return PHYAMD_OK;
}

size_t nni_candidates(const Shard *e) { return (size_t)std::max(0, e->T - 2); }

// What a call needs of the batch scratch per item (ScratchPlan).  The batched walk's arrays are the common base: an item's lengths,
// matrices and result rows, its stored lowers and per-block lnL, and with the pre-order pass (grad) so many parked uppers (slots)
// and the gradient slab; trees: the items walk their own op lists from their own roots
ScratchPlan batch_plan(Shard *e, bool grad, int slots, bool trees) {
	const size_t D = sizeof(double), N = (size_t)e->N, C = (size_t)e->C, nblk = ((size_t)e->P + WAVE - 1) / WAVE, plane = nblk * WAVE * 4;
	ScratchPlan p;
	p.add(e->d_batch_len, D * N);
	p.add(e->d_batch_mats, D * N * C * 16);
	p.add(e->d_batch_out, D * (grad ? 1 + N * C : 1));
	p.add(e->d_batch_lower, D * (size_t)(e->T - 1) * C * plane);
	p.add(e->d_batch_lnl, D * nblk);
	if (grad) {
		p.add(e->d_batch_upper, D * (size_t)slots * C * plane);
		p.add(e->d_batch_slab, D * nblk * C * N);
	}
	if (trees) {
		p.add(e->d_batch_item_ops, sizeof(BatchOp) * 2 * (size_t)(e->T - 1));
		p.add(e->d_batch_roots, sizeof(int32_t));
	}
	return p;
}

// what phyamd_nni_log_likelihoods and phyamd_nni_optimize share (launch_nni_walk): ONE item with every upper parked (slots = T - 1),
// and whatever the item count the op lists, the candidates and their index by node, and the caller's [3][N] lengths
ScratchPlan nni_base_plan(Shard *e) {
	const size_t N = (size_t)e->N, cands = std::max<size_t>(nni_candidates(e), 1);
	ScratchPlan p = batch_plan(e, true, e->T - 1, false);
	p.add(e->d_nni_ops, 0, sizeof(BatchOp) * 2 * (size_t)(e->T - 1));
	p.add(e->d_nni_cands, 0, sizeof(NniCand) * cands);
	p.add(e->d_nni_cand_of, 0, sizeof(int32_t) * N);
	p.add(e->d_nni_len, 0, sizeof(double) * 3 * N);
	return p;
}

// phyamd_nni_log_likelihoods: the walk's, and the trial matrices, the slab and the result
ScratchPlan nni_plan(Shard *e) {
	const size_t D = sizeof(double), N = (size_t)e->N, C = (size_t)e->C, nblk = ((size_t)e->P + WAVE - 1) / WAVE, cands = std::max<size_t>(nni_candidates(e), 1);
	ScratchPlan p = nni_base_plan(e);
	p.add(e->d_nni_mats, 0, D * 3 * N * C * 16);
	p.add(e->d_nni_slab, 0, D * cands * nblk * 9);
	p.add(e->d_nni_out, 0, D * 9 * N);
	return p;
}

// phyamd_spr_log_likelihoods: an item is a ROW -- every upper parked, its own op lists, its candidates, their index by cell, the
// slab and the result.  The two length vectors and their matrices are allocated once but counted for every row when a chunk is
// sized: an over-count of 16 N (1 + 16 C) bytes per row beyond the first, which the capped tests' chunk counts are pinned to
ScratchPlan spr_plan(Shard *e) {
	const size_t D = sizeof(double), N = (size_t)e->N, C = (size_t)e->C, nblk = ((size_t)e->P + WAVE - 1) / WAVE;
	ScratchPlan p = batch_plan(e, true, e->T - 1, true);
	p.add(e->d_spr_cands, sizeof(SprCand) * N);
	p.add(e->d_spr_cand_of, sizeof(int32_t) * N);
	p.add(e->d_spr_slab, D * N * nblk);
	p.add(e->d_spr_out, D * N);
	p.add(e->d_spr_len, D * 2 * N, 0, true);
	p.add(e->d_spr_mats, D * 2 * N * C * 16, 0, true);
	return p;
}

void release_batch_scratch(Shard *e) {
	e->batch_mem.release_all();
	e->batch_held = ScratchPlan{};
	e->batch_items = 0;
}

// items of `plan` the scratch holds now (none once the group has been released to make room)
size_t batch_items_held(const Shard *e, const ScratchPlan &plan) { return plan.held(e->batch_items) ? e->batch_items : 0; }

constexpr int BATCH_MAX_CHUNK = 65535;  // gridDim.y

// items of a batch (count items of `plan`) whose scratch fits beside the engine (scratch_room).  What the scratch holds already is
// kept unless more items would fit.
size_t batch_items_that_fit(const Shard *e, size_t count, const ScratchPlan &plan) {
	const size_t want = std::min<size_t>(count, BATCH_MAX_CHUNK), have = batch_items_held(e, plan);
	if (have >= want) return want;
	const double fit = plan.items_in(scratch_room(e, (double)batch_scratch_bytes(e), EngineRoom::MayGrow));
	if (fit <= (double)have) return have;
	return (size_t)std::min((double)want, fit);
}

int allocate_batch_scratch(Shard *e, size_t items, const ScratchPlan &plan) {
	release_batch_scratch(e);  // (the arrays grow together: all are freed before any is allocated again)
	if (int rc = plan.allocate(items)) {
		release_batch_scratch(e);
		return rc;
	}
	e->batch_held = plan;
	e->batch_items = items;
	e->nni_lists_valid = false;  // (freed above with everything else)
	return PHYAMD_OK;
}

int ensure_batch_scratch(Shard *e, size_t items, const ScratchPlan &plan) {
	if (batch_items_held(e, plan) >= items) return PHYAMD_OK;
	if (e->cfg.max_device_bytes <= 0 && e->batch_items > 0 && e->batch_held.held(e->batch_items)) {
		// without a cap the scratch keeps what the previous call needed as well -- the held plan's entries that this one lacks, and
		// of an array both name the larger size: calls of several kinds, or of trees that park in fewer and in more slots, may
		// alternate without an allocation each (under a cap every call gets exactly its own)
		ScratchPlan both = plan;
		both.merge(e->batch_held);
		if (allocate_batch_scratch(e, items, both) == PHYAMD_OK) return PHYAMD_OK;
		(void)hipGetLastError();  // (the attempt's out-of-memory is not the call's: a later hipGetLastError() of the call would report it)
	}
	return allocate_batch_scratch(e, items, plan);
}

// `rows` rows of `width` doubles, src_stride apart on the host, to rows dst_stride apart on the device
int upload_rows(Shard *e, double *dst, size_t dst_stride, const double *src, size_t src_stride, size_t width, size_t rows) {
	if (dst_stride == width && src_stride == width) HIP_TRY(hipMemcpyAsync(dst, src, sizeof(double) * width * rows, hipMemcpyHostToDevice, e->stream));
	else HIP_TRY(hipMemcpy2DAsync(dst, sizeof(double) * dst_stride, src, sizeof(double) * src_stride, sizeof(double) * width, rows, hipMemcpyHostToDevice, e->stream));
	return PHYAMD_OK;
}

// the batched walk's arguments on the engine's inputs and the batch scratch: every block of the patterns, the engine's weight row for
// every item.  ops: post-order then pre-order list (item_stride: BatchArgs'); slots: an item's upper slots; mats: [item][N][C][16]
BatchArgs batch_args(Shard *e, const BatchOp *ops, int item_stride, int slots, bool grad, const double *mats) {
	BatchArgs a{};
	a.lower_ops = ops, a.upper_ops = ops + (e->T - 1), a.item_stride = item_stride;
	a.T = e->T, a.N = e->N, a.P = e->P, a.C = e->C, a.nblk = (e->P + WAVE - 1) / WAVE, a.upper_slots = slots, a.grad = grad ? 1 : 0;
	a.tipmask = e->d_tipmask, a.freqs = e->d_freqs, a.props = e->d_props, a.weights = e->d_weights, a.Q = e->d_Q, a.mats = mats;
	a.lower = e->d_batch_lower, a.upper = e->d_batch_upper, a.lnl_part = e->d_batch_lnl, a.slab = e->d_batch_slab;
	return a;
}

// one chunk of `items` items through the batched walk: lengths [items][N] (host) -> out [items][rows] (host), rows = 1 or 1 + N C.
// trees: the items walk their own op lists from their own roots, already in d_batch_item_ops and d_batch_roots; else the
// engine's.  slots: the upper slots an item of this chunk has in d_batch_upper (at least what its list parks in).  weights: a row
// of pattern weights per item (host, rows weight_stride apart; phyamd_gradient_batch_weights), or null: the engine's for every item
int run_batch_chunk(Shard *e, int flags, int items, const double *lengths, bool grad, int slots, bool trees, double *out, const double *weights = nullptr,
                    size_t weight_stride = 0) {
	const int nblk = (e->P + WAVE - 1) / WAVE, rows = grad ? 1 + e->N * e->C : 1, nops = e->T - 1;
	const BatchOp *ops = trees ? e->d_batch_item_ops.get() : e->d_batch_ops.get();
	const int32_t *roots = trees ? e->d_batch_roots.get() : nullptr;
	HIP_TRY(hipMemcpyAsync(e->d_batch_len, lengths, sizeof(double) * (size_t)items * e->N, hipMemcpyHostToDevice, e->stream));
	launch_batch_matrices(e, items, e->d_batch_len, roots, e->d_batch_mats);
	int rc;
	if (weights && (rc = upload_rows(e, e->d_reweight_w, (size_t)e->P, weights, weight_stride, (size_t)e->P, (size_t)items))) return rc;
	BatchArgs a = batch_args(e, ops, trees ? 2 * nops : 0, slots, grad, e->d_batch_mats);
	if (weights) a.weights = e->d_reweight_w, a.weight_stride = (size_t)e->P;
	const dim3 grid(nblk, items), block(WAVE, e->C);
	if (flags & PHYAMD_GRAD_FOLD_ROOT_FREQS) hipLaunchKernelGGL(k_batch_walk4<true>, grid, block, 0, e->stream, a);
	else hipLaunchKernelGGL(k_batch_walk4<false>, grid, block, 0, e->stream, a);
	hipLaunchKernelGGL(k_batch_finish, dim3((unsigned)(((size_t)items * rows + 255) / 256)), dim3(256), 0, e->stream, items, e->N, e->C, nblk, e->root, roots, rows,
	                   e->d_batch_lnl, e->d_batch_slab, e->d_batch_out);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(out, e->d_batch_out, sizeof(double) * (size_t)items * rows, hipMemcpyDeviceToHost, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream));
	return PHYAMD_OK;
}

// an item's row of the batched walk [lnl | gradient [N C]] into the caller's arrays, a lnL that is not finite in band
void store_batch_item(const double *row, size_t ncat, double *lnl, double *cat_gradient) {
	*lnl = row[0];
	if (!cat_gradient) return;
	std::copy(row + 1, row + 1 + ncat, cat_gradient);
	mask_if_not_finite(row[0], cat_gradient, ncat);
}

// the definition of the call: item by item through the ordinary path (the caller puts the engine's lengths back, and its weights
// where the item brings its own; either may be null: the engine's)
int batch_item_sequential(Shard *e, int flags, const double *lengths, double *lnl, double *cat_gradient, const double *weights = nullptr) {
	int rc;
	if (weights && (rc = shard_set_pattern_weights(e, weights))) return rc;
	if (lengths && (rc = shard_set_branch_lengths(e, lengths))) return rc;
	return cat_gradient ? shard_gradient(e, flags, lnl, cat_gradient) : shard_log_likelihood(e, lnl);
}

// the items of a batch, each through the batched walk or the ordinary path; prof: how many went which way.  weights: null, or a
// row of pattern weights per item, weight_stride apart (phyamd_gradient_batch_weights with lengths: `name` and `walked`, the items
// the batched walk was launched for)
int run_batch(Shard *e, int flags, int32_t count, const double *branch_lengths, double *lnl, double *cat_gradient, phyamd_batch_profile &prof,
              const char *name = "phyamd_gradient_batch", const double *weights = nullptr, size_t weight_stride = 0, int32_t *walked = nullptr) {
	int rc;
	if ((rc = check_ready_but_lengths(e))) return rc;
	for (int n = 0; n < e->N; n++)
		if (n != e->root && e->explicit_host[n])
			return fail(PHYAMD_EUNSUPPORTED, "%s: node %d has explicit matrices, which cannot follow per-item branch lengths", name, n);
	if (cat_gradient && !e->have_Q) return fail(PHYAMD_EINVAL, "the gradient needs the rate matrix: phyamd_set_eigen or phyamd_set_rate_matrix");
	const bool grad = cat_gradient != nullptr;
	const size_t N = (size_t)e->N, ncat = N * e->C, rows = grad ? 1 + ncat : 1;
	std::vector<uint8_t> redo(count, 1);  // items the sequential path (still) has to evaluate
	if ((rc = ensure_engine_batch_ops(e))) return rc;
	ScratchPlan plan = batch_plan(e, grad, e->batch_upper_slots, false);
	if (weights) plan.add(e->d_reweight_w, sizeof(double) * (size_t)e->P);
	const auto row = [&](size_t b) { return weights ? weights + b * weight_stride : nullptr; };
	std::vector<double> lengths, out;
	for (size_t first = 0; first < (size_t)count && batch_fast_path(e, flags, 1);) {
		// (every chunk asks again: an item that went through the ordinary path may have taken the scratch's room)
		const size_t chunk = batch_items_that_fit(e, (size_t)count - first, plan);
		if (!batch_fast_path(e, flags, chunk)) break;
		if ((rc = ensure_batch_scratch(e, chunk, plan))) return rc;
		const size_t items = std::min(chunk, (size_t)count - first);
		lengths.assign(branch_lengths + first * N, branch_lengths + (first + items) * N);
		out.resize(items * rows);
		for (size_t b = 0; b < items; b++) lengths[b * N + e->root] = 0.0;  // (ignored, as phyamd_set_branch_lengths does)
		if ((rc = run_batch_chunk(e, flags, (int)items, lengths.data(), grad, e->batch_upper_slots, false, out.data(), row(first), weight_stride))) return rc;
		prof.chunks++;
		if (walked) *walked += (int32_t)items;
		for (size_t b = 0; b < items; b++) {
			const double l = out[b * rows];
			if (not_finite(l) && e->cfg.rescale == PHYAMD_RESCALE_AUTO) {
				// the lazy switch's case (treelikelihood.c:1496-1519): this item goes through the ordinary path right away, and
				// if that turns rescaling on, so does the rest of the batch
				if ((rc = batch_item_sequential(e, flags, branch_lengths + (first + b) * N, lnl + first + b, grad ? cat_gradient + (first + b) * ncat : nullptr, row(first + b))))
					return rc;
				redo[first + b] = 0;
				prof.items_sequential++;
				continue;
			}
			store_batch_item(&out[b * rows], ncat, lnl + first + b, grad ? cat_gradient + (first + b) * ncat : nullptr);
			redo[first + b] = 0;
			prof.items_fast++;
		}
		first += items;
	}
	for (int b = 0; b < count; b++) {
		if (!redo[b]) continue;
		if ((rc = batch_item_sequential(e, flags, branch_lengths + (size_t)b * N, lnl + b, grad ? cat_gradient + (size_t)b * ncat : nullptr, row((size_t)b)))) return rc;
		prof.items_sequential++;
	}
	return PHYAMD_OK;
}

int shard_gradient_batch(Shard *e, int flags, int32_t count, const double *branch_lengths, double *lnl, double *cat_gradient) {
	CHECK_ENGINE(e);
	return profiled_call(e, &Shard::batch_prof, phyamd_batch_profile{}, [&](phyamd_batch_profile &prof) {
		const std::vector<double> lengths = e->lengths_sent;
		const bool had_lengths = e->have_lengths;
		int rc = run_batch(e, flags, count, branch_lengths, lnl, cat_gradient, prof);
		if (prof.items_sequential > 0 || rc) {  // the ordinary path has set items' lengths: the engine's own go back
			const std::string why = g_last_error;
			if (had_lengths) {
				const int rc2 = shard_set_branch_lengths(e, lengths.data());
				if (!rc) rc = rc2;
				else g_last_error = why;
			} else
				e->have_lengths = false;
		}
		return rc;
	});
}

// ---- a batch of pattern-weight vectors (phyamd_gradient_batch_weights) ---------------------------------------------------------

// The scratch of the shared-lengths path (phyamd_reweight.inc) for pattern chunks of nblk blocks.  An item is a REPLICATE: its
// weight row over the chunk's patterns, its result row and its segment sums.  Whatever the replicate count: the walk's arrays of
// ONE item (stored lowers, parked uppers), the rows R and the mark of a log L_k that is not finite.  The op lists and the matrices
// are the engine's own and count with the engine
ScratchPlan reweight_plan(Shard *e, bool grad, size_t nblk) {
	const size_t D = sizeof(double), N = (size_t)e->N, C = (size_t)e->C, Pc = nblk * WAVE, rows = grad ? 1 + N * C : 1;
	const size_t segments = (Pc + REWEIGHT_SEGMENT - 1) / REWEIGHT_SEGMENT;
	ScratchPlan p;
	p.add(e->d_batch_lower, 0, D * (size_t)(e->T - 1) * C * Pc * 4);
	if (grad) p.add(e->d_batch_upper, 0, D * (size_t)e->batch_upper_slots * C * Pc * 4);
	p.add(e->d_batch_lnl, 0, D);
	p.add(e->d_reweight_R, 0, D * rows * Pc);
	p.add(e->d_reweight_w, D * Pc);
	p.add(e->d_batch_out, D * rows);
	p.add(e->d_reweight_part, D * segments * rows);
	return p;
}

constexpr size_t REWEIGHT_MAX_CHUNK = (size_t)1 << 20;  // replicates per chunk: gridDim.y of k_reweight_mfma is a sixteenth

// the product W R^T of `reps` weight rows (host, weight_stride apart, `width` patterns wide) with the `rows` rows of d_reweight_R
// (Pc wide): the weights go up into rows padded to Pc and k_reweight_mfma leaves the segment sums in d_reweight_part.  *r: the
// product's arguments for the caller's finish kernel (out: where k_reweight_finish puts the results, or null)
int launch_reweight_product(Shard *e, const double *weights, size_t weight_stride, size_t width, size_t reps, size_t rows, size_t Pc, double *out, ReweightArgs *r) {
	if (width < Pc) HIP_TRY(hipMemsetAsync(e->d_reweight_w, 0, sizeof(double) * reps * Pc, e->stream));  // (a garbage NaN times R's 0 is a NaN)
	if (int rc = upload_rows(e, e->d_reweight_w, Pc, weights, weight_stride, width, reps)) return rc;
	*r = ReweightArgs{e->d_reweight_w, e->d_reweight_R, e->d_reweight_part, out, (int)reps, (int)rows, (int)Pc, (int)((Pc + REWEIGHT_SEGMENT - 1) / REWEIGHT_SEGMENT), e->N, e->C};
	hipLaunchKernelGGL(k_reweight_mfma, dim3((unsigned)((rows + 15) / 16), (unsigned)((reps + 15) / 16), (unsigned)r->segments), dim3(WAVE), 0, e->stream, *r);
	return PHYAMD_OK;
}

// every replicate on the engine's own lengths: ONE walk per pattern chunk leaves R, and the replicates are products with it.
// *sequential: the engine does not take the batched walk, or (PHYAMD_RESCALE_AUTO) a pattern's log L_k is not finite: nothing has
// been stored and the caller evaluates the replicates one by one
int run_reweight(Shard *e, int flags, int32_t count, const double *weights, size_t weight_stride, double *lnl, double *cat_gradient,
                 phyamd_weight_batch_profile &prof, bool *sequential) {
	static const char *const name = "phyamd_gradient_batch_weights";
	int rc;
	*sequential = false;
	if ((rc = check_ready(e))) return rc;
	if (cat_gradient && !e->have_Q) return fail(PHYAMD_EINVAL, "the gradient needs the rate matrix: phyamd_set_eigen or phyamd_set_rate_matrix");
	if (batch_walk_refusal(e, flags)) {
		*sequential = true;
		return PHYAMD_OK;
	}
	if ((rc = ensure_engine_batch_ops(e)) || (rc = update_matrices(e))) return rc;
	const bool grad = cat_gradient != nullptr, lazy = e->cfg.rescale == PHYAMD_RESCALE_AUTO;
	const int N = e->N, C = e->C, P = e->P;
	const size_t ncat = (size_t)N * C, rows = grad ? 1 + ncat : 1, nblk_all = ((size_t)P + WAVE - 1) / WAVE;
	// the pattern chunk: every block if one replicate fits beside it, else the most blocks that leave room for one
	const double room = scratch_room(e, (double)batch_scratch_bytes(e), EngineRoom::MayGrow);
	const auto fit = [&](size_t nb) { return reweight_plan(e, grad, nb).items_in(room); };
	size_t nblk = nblk_all;
	if (fit(nblk) < 1.0) {
		if (fit(1) < 1.0) {
			const ScratchPlan one = reweight_plan(e, grad, 1);
			return fail(PHYAMD_ENOMEM, "%s: the scratch of one block of 64 patterns (%.0f bytes, and %.0f per replicate) does not fit the memory budget", name,
			            (double)one.fixed_bytes(), (double)one.item_bytes());
		}
		size_t lo = 1, hi = nblk_all;  // fit(lo) >= 1 > fit(hi)
		while (hi - lo > 1) {
			const size_t mid = lo + (hi - lo) / 2;
			(fit(mid) >= 1.0 ? lo : hi) = mid;
		}
		nblk = lo;
	}
	const ScratchPlan plan = reweight_plan(e, grad, nblk);
	const size_t chunk = (size_t)std::min((double)std::min<size_t>((size_t)count, REWEIGHT_MAX_CHUNK), fit(nblk));
	if (!plan.held(chunk) && e->cfg.max_device_bytes > 0) release_batch_scratch(e);  // (under a cap a call gets exactly its own scratch)
	if ((rc = plan.allocate(chunk))) return rc;

	const BatchOp *ops = e->d_batch_ops.get();
	std::vector<double> total((size_t)count * rows), out;
	double *const mark = lazy ? e->d_batch_lnl.get() : nullptr;
	for (size_t b0 = 0; b0 < nblk_all; b0 += nblk) {
		const size_t nb = std::min(nblk, nblk_all - b0), Pc = nb * WAVE, k0 = b0 * WAVE, width = std::min(Pc, (size_t)P - k0);
		BatchArgs a = batch_args(e, ops, 0, e->batch_upper_slots, grad, e->d_mats);
		a.nblk = (int)nb, a.lnl_part = a.slab = nullptr;  // the terms form: the chunk's blocks, rows of R instead of sums
		a.k0 = (int)k0, a.Pc = (int)Pc, a.R = e->d_reweight_R, a.not_finite = mark;
		if (mark) HIP_TRY(hipMemsetAsync(mark, 0, sizeof(double), e->stream));
		const dim3 grid((unsigned)nb), block(WAVE, C);
		if (flags & PHYAMD_GRAD_FOLD_ROOT_FREQS) hipLaunchKernelGGL(k_reweight_terms4<true>, grid, block, 0, e->stream, a);
		else hipLaunchKernelGGL(k_reweight_terms4<false>, grid, block, 0, e->stream, a);
		HIP_TRY(hipGetLastError());
		prof.walks++;
		prof.pattern_chunks++;
		for (size_t first = 0; first < (size_t)count; first += chunk) {
			const size_t items = std::min(chunk, (size_t)count - first);
			ReweightArgs r;
			if ((rc = launch_reweight_product(e, weights + first * weight_stride + k0, weight_stride, width, items, rows, Pc, e->d_batch_out, &r))) return rc;
			hipLaunchKernelGGL(k_reweight_finish, dim3((unsigned)((items * rows + 255) / 256)), dim3(256), 0, e->stream, r);
			HIP_TRY(hipGetLastError());
			out.resize(items * rows);
			double marked = 0.0;
			HIP_TRY(hipMemcpyAsync(out.data(), e->d_batch_out, sizeof(double) * items * rows, hipMemcpyDeviceToHost, e->stream));
			if (mark) HIP_TRY(hipMemcpyAsync(&marked, mark, sizeof(double), hipMemcpyDeviceToHost, e->stream));
			HIP_TRY(hipStreamSynchronize(e->stream));
			if (marked != 0.0) {  // the lazy switch's case: the ordinary path decides, replicate by replicate
				*sequential = true;
				return PHYAMD_OK;
			}
			if (b0 == 0) prof.item_chunks++;
			double *const t = total.data() + first * rows;
			for (size_t i = 0; i < items * rows; i++) t[i] = b0 == 0 ? out[i] : t[i] + out[i];  // (the pattern chunks in chunk order)
		}
	}
	for (size_t b = 0; b < (size_t)count; b++) store_batch_item(&total[b * rows], ncat, lnl + b, grad ? cat_gradient + b * ncat : nullptr);
	prof.items_fast = count;
	return PHYAMD_OK;
}

// weights: row b at weights + b * weight_stride, this shard's P patterns of it (the group layer passes the handle's pattern count
// and a pointer advanced to this shard's range)
int shard_gradient_batch_weights(Shard *e, int flags, int32_t count, const double *weights, size_t weight_stride, const double *branch_lengths, double *lnl,
                                 double *cat_gradient) {
	static const char *const name = "phyamd_gradient_batch_weights";
	if (!e) return fail(PHYAMD_EINVAL, "%s: null engine", name);
	return profiled_call(e, &Shard::weight_prof, phyamd_weight_batch_profile{}, [&](phyamd_weight_batch_profile &prof) {
		const std::vector<double> lengths = e->lengths_sent, own = e->weights_host;
		const bool had_lengths = e->have_lengths, had_weights = e->have_weights;
		const uint64_t epoch = e->weights_epoch;
		const size_t ncat = (size_t)e->N * e->C;
		int rc;
		if (branch_lengths) {
			phyamd_batch_profile walk{};
			rc = run_batch(e, flags, count, branch_lengths, lnl, cat_gradient, walk, name, weights, weight_stride, &prof.walks);
			prof.items_fast = walk.items_fast, prof.items_sequential = walk.items_sequential, prof.item_chunks = walk.chunks;
		} else {
			bool sequential = false;
			rc = run_reweight(e, flags, count, weights, weight_stride, lnl, cat_gradient, prof, &sequential);
			for (int b = 0; b < count && sequential && !rc; b++)
				if (!(rc = batch_item_sequential(e, flags, nullptr, lnl + b, cat_gradient ? cat_gradient + (size_t)b * ncat : nullptr, weights + (size_t)b * weight_stride)))
					prof.items_sequential++;
		}
		// the ordinary path has set items' weights and lengths: the engine's own go back, whichever way the call ends
		const bool failed = rc != PHYAMD_OK;
		const std::string why = g_last_error;
		if (e->weights_epoch != epoch) {
			const int rc2 = had_weights ? shard_set_pattern_weights(e, own.data()) : PHYAMD_OK;
			if (!had_weights) e->have_weights = false;
			if (!rc) rc = rc2;
		}
		if (branch_lengths && (prof.items_sequential > 0 || rc)) {
			const int rc2 = had_lengths ? shard_set_branch_lengths(e, lengths.data()) : PHYAMD_OK;
			if (!had_lengths) e->have_lengths = false;
			if (!rc) rc = rc2;
		}
		if (failed) g_last_error = why;
		return rc;
	});
}

// ---- a batch of trees (phyamd_gradient_batch_trees) ---------------------------------------------------------------------------

// The items of a batch of trees in chunks of what the scratch holds.  item_ops(left, right, root, ops): an item's op list appended
// to ops (null: nothing is built), the slots it parks in; plan_of(slots): the scratch of a chunk whose items park in that many.
// Every item's tree is validated before anything is launched.  Per chunk the scratch is ensured, the items' op lists and roots go
// up (d_batch_item_ops, d_batch_roots; not waited for) and body runs on items [first, first + items), the slots of the deepest-
// parking one, their lengths [items][N] with the roots' entries zeroed (host), and the times before and after the lists were built
template <typename ItemOps, typename PlanOf, typename Body>
int for_tree_chunks(Shard *e, const char *name, int flags, int32_t count, const int32_t *left, const int32_t *right, const int32_t *roots, const double *branch_lengths,
                    ItemOps item_ops, PlanOf plan_of, Body body) {
	const size_t N = (size_t)e->N;
	std::vector<int> slots(count);  // per item: the slots its list parks in
	{
		std::vector<int32_t> parents;
		for (int32_t b = 0; b < count; b++) {  // every item, before anything is launched
			const int32_t *l = left + (size_t)b * N, *r = right + (size_t)b * N;
			const std::string err = validate_tree(TreeRef{e->T, l, r, roots[b]}, parents, name, b);
			if (!err.empty()) return fail(PHYAMD_EINVAL, "%s", err.c_str());
			slots[b] = item_ops(l, r, roots[b], nullptr);
		}
	}
	std::vector<double> lengths;
	std::vector<BatchOp> ops;
	int rc;
	for (size_t first = 0; first < (size_t)count;) {
		// the chunk and its slot count settle each other: fewer items never need more slots
		size_t items = std::min<size_t>((size_t)count - first, BATCH_MAX_CHUNK);
		int chunk_slots = 0;
		ScratchPlan plan;
		for (;;) {
			chunk_slots = *std::max_element(slots.begin() + first, slots.begin() + first + items);
			plan = plan_of(chunk_slots);
			const size_t fit = batch_items_that_fit(e, items, plan);
			if (const char *why = tree_batch_refusal(e, flags, fit)) return fail(PHYAMD_EUNSUPPORTED, "%s: %s", name, why);
			if (fit >= items) break;
			items = fit;
		}
		if ((rc = ensure_batch_scratch(e, items, plan))) return rc;
		lengths.assign(branch_lengths + first * N, branch_lengths + (first + items) * N);
		for (size_t b = 0; b < items; b++) lengths[b * N + roots[first + b]] = 0.0;  // (ignored, as phyamd_set_branch_lengths does)
		const auto t0 = std::chrono::steady_clock::now();
		ops.clear();
		for (size_t b = first; b < first + items; b++) item_ops(left + b * N, right + b * N, roots[b], &ops);
		const auto t1 = std::chrono::steady_clock::now();
		HIP_TRY(hipMemcpyAsync(e->d_batch_item_ops, ops.data(), sizeof(BatchOp) * ops.size(), hipMemcpyHostToDevice, e->stream));
		HIP_TRY(hipMemcpyAsync(e->d_batch_roots, roots + first, sizeof(int32_t) * items, hipMemcpyHostToDevice, e->stream));
		if ((rc = body(first, items, chunk_slots, lengths.data(), t0, t1))) return rc;  // (ends with the stream waited for: ops and lengths are reused)
		first += items;
	}
	return PHYAMD_OK;
}

// the items of a batch of trees through the batched walk: per chunk the upper slots of its deepest-parking item, three launches
int run_tree_batch(Shard *e, int flags, int32_t count, const int32_t *left, const int32_t *right, const int32_t *roots, const double *branch_lengths, double *lnl,
                   double *cat_gradient, phyamd_batch_profile &prof) {
	static const char *const name = "phyamd_gradient_batch_trees";
	int rc;
	if ((rc = check_ready_but_lengths(e))) return rc;
	const bool grad = cat_gradient != nullptr;
	if (const char *why = tree_batch_refusal(e, flags, 1)) return fail(PHYAMD_EUNSUPPORTED, "%s: %s", name, why);
	if (grad && !e->have_Q) return fail(PHYAMD_EINVAL, "the gradient needs the rate matrix: phyamd_set_eigen or phyamd_set_rate_matrix");
	const size_t ncat = (size_t)e->N * e->C, rows = grad ? 1 + ncat : 1;
	std::vector<double> out;
	// (an item's upper slots are its pre-order list's: without the gradient nothing is parked)
	const auto item_ops = [&](const int32_t *l, const int32_t *r, int32_t root, std::vector<BatchOp> *ops) { return ops || grad ? build_batch_ops(e->T, l, r, root, ops) : 1; };
	const auto plan_of = [&](int slots) { return batch_plan(e, grad, slots, true); };
	const auto chunk = [&](size_t first, size_t items, int slots, const double *lengths, auto t0, auto t1) -> int {
		HIP_TRY(hipStreamSynchronize(e->stream));  // (the lists' upload, timed on its own)
		const auto t2 = std::chrono::steady_clock::now();
		out.resize(items * rows);
		if (int rc = run_batch_chunk(e, flags, (int)items, lengths, grad, slots, true, out.data())) return rc;
		if (e->batch_trace) {
			const auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
			std::fprintf(stderr, "phyamd_gradient_batch_trees: chunk %d items %zu slots %d build_ms %.6f upload_ms %.6f\n", prof.chunks, items, slots, ms(t0, t1),
			             ms(t1, t2));
		}
		prof.chunks++;
		for (size_t b = 0; b < items; b++) {
			// (a lnL that is not finite is in band whatever the rescaling mode: the engine is never switched)
			store_batch_item(&out[b * rows], ncat, lnl + first + b, grad ? cat_gradient + (first + b) * ncat : nullptr);
			prof.items_fast++;
		}
		return PHYAMD_OK;
	};
	return for_tree_chunks(e, name, flags, count, left, right, roots, branch_lengths, item_ops, plan_of, chunk);
}

// reads the engine's inputs and writes only the batch scratch: nothing in Shard::state changes
int shard_gradient_batch_trees(Shard *e, int flags, int32_t count, const int32_t *left, const int32_t *right, const int32_t *roots, const double *branch_lengths,
                               double *lnl, double *cat_gradient) {
	CHECK_ENGINE(e);
	return profiled_call(e, &Shard::batch_prof, phyamd_batch_profile{}, [&](phyamd_batch_profile &prof) { return run_tree_batch(e, flags, count, left, right, roots, branch_lengths, lnl, cat_gradient, prof); });
}

// ---- every NNI neighbour of the engine's tree (phyamd_nni_log_likelihoods) -----------------------------------------------------

// the engine's tree's op lists with every upper parked, its candidate edges and their index by node, into the scratch
int upload_nni_lists(Shard *e) {
	if (e->nni_lists_valid && e->d_nni_ops.get()) return PHYAMD_OK;
	const int T = e->T, N = e->N;
	std::vector<BatchOp> ops;
	build_batch_ops(T, e->left.data(), e->right.data(), e->root, &ops, true);
	std::vector<NniCand> cands;
	std::vector<int32_t> cand_of(N, -1);
	for (int v = T; v < N; v++) {
		if (v == e->root) continue;
		const int u = e->sched.parent[v];
		cand_of[v] = (int32_t)cands.size();
		cands.push_back(NniCand{v, u == e->root ? BATCH_ROOT : u, e->left[u] == v ? e->right[u] : e->left[u], e->left[v], e->right[v], {0, 0, 0}});
	}
	HIP_TRY(hipMemcpyAsync(e->d_nni_ops, ops.data(), sizeof(BatchOp) * ops.size(), hipMemcpyHostToDevice, e->stream));
	if (!cands.empty()) HIP_TRY(hipMemcpyAsync(e->d_nni_cands, cands.data(), sizeof(NniCand) * cands.size(), hipMemcpyHostToDevice, e->stream));
	HIP_TRY(hipMemcpyAsync(e->d_nni_cand_of, cand_of.data(), sizeof(int32_t) * N, hipMemcpyHostToDevice, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream));  // (stack-lifetime buffers)
	e->nni_lists_valid = true;
	return PHYAMD_OK;
}

// a call on the NNI candidates of the walked tree: its name, its [3][N] lengths' argument, what one is called, what the eigen system forms
struct NniWalkCall {
	const char *name, *argument, *noun, *formed;
};

// the call's checks, and its lengths [3][N]: a candidate's own three where the caller gives them (own, or null), every other entry
// the engine's (ignored: no arrangement reads that matrix)
int check_nni_walk(Shard *e, const NniWalkCall &call, int flags, const double *own, std::vector<double> &lengths) {
	int rc;
	if ((rc = check_ready(e))) return rc;
	if (flags != 0) return fail(PHYAMD_EUNSUPPORTED, "%s: flags %d (no flags are defined: pass 0)", call.name, flags);
	if (const char *why = tree_batch_refusal(e, 0, 1)) return fail(PHYAMD_EUNSUPPORTED, "%s: %s", call.name, why);
	if (!e->have_eigen || !e->have_Q) return fail(PHYAMD_EINVAL, "%s needs the eigen system (phyamd_set_eigen): %s formed from it", call.name, call.formed);
	const int T = e->T, N = e->N;
	lengths.resize((size_t)3 * N);
	for (int k = 0; k < 3; k++) std::copy(e->lengths.begin(), e->lengths.end(), lengths.begin() + (size_t)k * N);
	for (int v = T; v < N && own; v++) {
		if (v == e->root) continue;
		for (int k = 0; k < 3; k++) {
			const double t = own[(size_t)k * N + v];
			if (!std::isfinite(t) || t < 0.0) return fail(PHYAMD_EINVAL, "%s: %s[%d][%d] = %g: a %s is finite and not negative", call.name, call.argument, k, v, t, call.noun);
			lengths[(size_t)k * N + v] = t;
		}
	}
	return PHYAMD_OK;
}

// the scratch of `plan` (nni_base_plan's and the caller's own), the lists, the lengths [3][N] (host) into d_nni_len, the matrices
// of the engine's lengths -- and with `trial` those of the three length vectors, into d_nni_mats -- and ONE item through
// the batched walk with every upper parked.  The caller waits for the stream before `lengths` goes
int launch_nni_walk(Shard *e, const ScratchPlan &plan, const std::vector<double> &lengths, bool trial) {
	int rc;
	if ((rc = ensure_batch_scratch(e, 1, plan)) || (rc = upload_nni_lists(e))) return rc;
	HIP_TRY(hipMemcpyAsync(e->d_nni_len, lengths.data(), sizeof(double) * lengths.size(), hipMemcpyHostToDevice, e->stream));
	launch_batch_matrices(e, 1, e->d_lengths, nullptr, e->d_batch_mats);  // the walk's item: the engine's lengths
	if (trial) launch_batch_matrices(e, 3, e->d_nni_len, nullptr, e->d_nni_mats);
	const BatchArgs walk = batch_args(e, e->d_nni_ops.get(), 0, e->T - 1, true, e->d_batch_mats);
	hipLaunchKernelGGL(k_batch_walk4<false>, dim3(walk.nblk, 1), dim3(WAVE, e->C), 0, e->stream, walk);
	return PHYAMD_OK;
}

// out [3 terms][3][N] (host): one walk of the engine's tree with every upper parked, the trial matrices, every edge's three
// arrangements in one launch.  Reads the engine's inputs and writes only the batch scratch: nothing in Shard::state changes
int run_nni(Shard *e, int flags, const double *central_lengths, bool deriv, double *out, phyamd_nni_profile &prof) {
	static const NniWalkCall call{"phyamd_nni_log_likelihoods", "central_lengths", "trial length", "the trial matrices, d1 and d2 are"};
	int rc;
	std::vector<double> trial;
	if ((rc = check_nni_walk(e, call, flags, central_lengths, trial))) return rc;
	const int T = e->T, N = e->N, C = e->C;
	const size_t cands = nni_candidates(e);
	prof.candidates = (int32_t)cands;
	std::fill(out, out + (size_t)9 * N, NAN);
	if (cands == 0) return PHYAMD_OK;  // two tips: no internal edge
	const ScratchPlan plan = nni_plan(e);
	if (batch_items_that_fit(e, 1, plan) < 1)
		return fail(PHYAMD_EUNSUPPORTED, "phyamd_nni_log_likelihoods: the scratch (%zu bytes: every internal node's lower and upper partial) does not fit the memory budget",
		            plan.item_bytes() + plan.fixed_bytes());
	if ((rc = launch_nni_walk(e, plan, trial, true))) return rc;
	const int nblk = (e->P + WAVE - 1) / WAVE;
	for (size_t first = 0; first < cands; first += BATCH_MAX_CHUNK) {  // (gridDim.y)
		const size_t n = std::min<size_t>(cands - first, BATCH_MAX_CHUNK);
		const NniArgs a{e->d_nni_cands.get() + first, T, N, e->P, C, nblk, deriv ? 1 : 0, e->d_tipmask, e->d_freqs, e->d_props, e->d_rates, e->d_weights, e->d_Q,
		                e->d_batch_mats, e->d_nni_mats, e->d_batch_lower, e->d_batch_upper, e->d_nni_slab + first * nblk * 9};
		hipLaunchKernelGGL(k_nni4, dim3(nblk, (unsigned)n), dim3(WAVE, C), 0, e->stream, a);
	}
	hipLaunchKernelGGL(k_nni_finish, dim3((unsigned)(((size_t)9 * N + 255) / 256)), dim3(256), 0, e->stream, N, nblk, e->d_nni_cand_of.get(), e->d_nni_slab.get(),
	                   e->d_nni_out.get());
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(out, e->d_nni_out, sizeof(double) * (size_t)9 * N, hipMemcpyDeviceToHost, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream));  // (also covers `trial`)
	return PHYAMD_OK;
}

// mask_if_not_finite per entry: every entry has a lnL of its own; out: [lnl | d1 | d2]
void nni_mask_derivatives(size_t entries, double *out) {
	for (size_t i = 0; i < entries; i++)
		if (not_finite(out[i])) out[entries + i] = out[2 * entries + i] = NAN;
}

// out [3 terms][3][N] on the host; deriv: d1 and d2 as well (else those rows are NaN at tips and the root, 0 elsewhere)
int shard_nni_log_likelihoods(Shard *e, int flags, const double *central_lengths, bool deriv, double *out) {
	CHECK_ENGINE(e);
	return profiled_call(e, &Shard::nni_prof, phyamd_nni_profile{}, [&](phyamd_nni_profile &prof) {
		const int rc = run_nni(e, flags, central_lengths, deriv, out, prof);
		if (!rc) nni_mask_derivatives((size_t)3 * e->N, out);
		return rc;
	});
}

// ---- every NNI neighbour of a 20-state engine's tree (phyamd_nni_log_likelihoods_general) ---------------------------------------

// nothing is walked and nothing scales with an item count: the candidates and their index by node, the caller's [3][N] lengths, the
// images of V^T and V^-1, the slab (blocks of CLASSNNI_BLOCK patterns) and the result
ScratchPlan nni_gen_plan(Shard *e, size_t nblk) {
	const size_t D = sizeof(double), N = (size_t)e->N, cands = std::max<size_t>(nni_candidates(e), 1);
	ScratchPlan p;
	p.add(e->d_nnig_cands, 0, sizeof(ClassNniCand) * cands);
	p.add(e->d_nnig_eig, 0, D * 2 * MatImage<2, 5>::SIZE);
	p.add(e->d_nni_cand_of, 0, sizeof(int32_t) * N);
	p.add(e->d_nni_len, 0, D * 3 * N);
	p.add(e->d_nni_slab, 0, D * cands * nblk * 9);
	p.add(e->d_nni_out, 0, D * 9 * N);
	return p;
}

// the candidate edges of the engine's tree with the resident partials of their four messages, in node order, and their index by
// node, into d_nnig_cands and d_nni_cand_of (the caller waits for the stream before the two vectors go).  What the two 20-state NNI
// calls share
int upload_classnni_records(Shard *e, const char *name, std::vector<ClassNniCand> &records, std::vector<int32_t> &cand_of) {
	const int T = e->T, N = e->N, root = e->root;
	const size_t npd = node_partial_doubles(e);
	const auto lower_of = [&](int n) { return n < T ? (const double *)nullptr : e->d_lower + (size_t)e->sched.core_index[n] * npd; };
	records.clear();
	cand_of.assign(N, -1);
	for (int v = T; v < N; v++) {
		if (v == root) continue;
		const int u = e->sched.parent[v], s = e->left[u] == v ? e->right[u] : e->left[u], a = e->left[v], b = e->right[v];
		for (const int n : {a, b, s})
			if (n >= T && e->sched.core_index[n] < 0) return fail(PHYAMD_EDEVICE, "%s: node %d has no resident lower partial", name, n);
		if (u != root && (e->sched.upper_slot[u] < 0 || !e->d_upper)) return fail(PHYAMD_EDEVICE, "%s: node %d has no resident upper partial", name, u);
		cand_of[v] = (int32_t)records.size();
		records.push_back(ClassNniCand{u == root ? nullptr : e->d_upper + (size_t)e->sched.upper_slot[u] * npd, lower_of(a), lower_of(b), lower_of(s), v, u, a, b, s, {0, 0, 0}});
	}
	e->nni_lists_valid = false;  // (d_nni_cand_of holds this call's index, which is the 4-state lists' too, but their ops and candidates are not here)
	HIP_TRY(hipMemcpyAsync(e->d_nnig_cands, records.data(), sizeof(ClassNniCand) * records.size(), hipMemcpyHostToDevice, e->stream));
	HIP_TRY(hipMemcpyAsync(e->d_nni_cand_of, cand_of.data(), sizeof(int32_t) * N, hipMemcpyHostToDevice, e->stream));
	return PHYAMD_OK;
}

// the images of V^T and V^-1 into d_nnig_eig
void launch_classnni_eigen_images(Shard *e) {
	const double *evec = e->d_model.get() + PLACE_GEN_STATES, *ivec = evec + PLACE_GEN_STATES * PLACE_GEN_STATES;  // d_model: eval [20] | evec [20][20] | ivec [20][20]
	hipLaunchKernelGGL(k_classplace_transposed_images, dim3(1), dim3(256), 0, e->stream, evec, e->d_nnig_eig.get());
	build_matrix_images(e, 1, ivec, e->d_nnig_eig.get() + MatImage<2, 5>::SIZE);
}

// out [3 terms][3][N] (host): the four messages round every candidate edge read from the resident partials, every edge's three
// arrangements in one launch.  Writes only the batch scratch beyond the evaluation that made the partials resident
int run_nni_general(Shard *e, int flags, const double *central_lengths, bool deriv, double *out, phyamd_nni_profile &prof) {
	static const GeneralQueryCall call{"phyamd_nni_log_likelihoods_general", "the kernel is", "phyamd_nni_log_likelihoods", "64-wide products are",
	                                   "which have no exponential sum in the central length", "the likelihood in the central length is", "coefficients do"};
	int rc;
	if ((rc = check_general_query_inputs(e, call, flags))) return rc;
	const int T = e->T, N = e->N, C = e->C, P = e->P, root = e->root;
	std::vector<double> trial((size_t)3 * N);  // a candidate's own three where the caller gives them, every other entry the engine's (not read)
	for (int k = 0; k < 3; k++) std::copy(e->lengths.begin(), e->lengths.end(), trial.begin() + (size_t)k * N);
	for (int v = T; v < N && central_lengths; v++) {
		if (v == root) continue;
		for (int k = 0; k < 3; k++) {
			const double t = central_lengths[(size_t)k * N + v];
			if (!std::isfinite(t) || t < 0.0) return fail(PHYAMD_EINVAL, "%s: central_lengths[%d][%d] = %g: a trial length is finite and not negative", call.name, k, v, t);
			trial[(size_t)k * N + v] = t;
		}
	}
	if ((rc = check_general_query_resident(e, call))) return rc;
	const size_t cands = nni_candidates(e);
	prof.candidates = (int32_t)cands;
	std::fill(out, out + (size_t)9 * N, NAN);
	if (cands == 0) return PHYAMD_OK;  // two tips: no internal edge
	const int nblk = (P + CLASSNNI_BLOCK - 1) / CLASSNNI_BLOCK;
	const ScratchPlan plan = nni_gen_plan(e, (size_t)nblk);
	if (batch_items_that_fit(e, 1, plan) < 1)
		return fail(PHYAMD_EUNSUPPORTED, "%s: the scratch (%zu bytes: the candidates, the slab and the result) does not fit the memory budget", call.name,
		            plan.item_bytes() + plan.fixed_bytes());
	if ((rc = ensure_batch_scratch(e, 1, plan))) return rc;
	std::vector<ClassNniCand> records;
	std::vector<int32_t> cand_of;
	if ((rc = upload_classnni_records(e, call.name, records, cand_of))) return rc;
	HIP_TRY(hipMemcpyAsync(e->d_nni_len, trial.data(), sizeof(double) * trial.size(), hipMemcpyHostToDevice, e->stream));
	launch_classnni_eigen_images(e);
	for (size_t first = 0; first < cands; first += BATCH_MAX_CHUNK) {  // (gridDim.y)
		const size_t n = std::min<size_t>(cands - first, BATCH_MAX_CHUNK);
		const ClassNniArgs a{e->d_nnig_cands.get() + first, N, P, e->Pp, C, e->upper_fold ? 1 : 0, deriv ? 1 : 0, e->d_tipmask, e->d_tipsets, e->d_freqs, e->d_props, e->d_rates,
		                     e->d_weights, e->d_model, e->d_imgs, e->d_nnig_eig, e->d_nni_len, e->d_nni_slab + first * nblk * 9};
		hipLaunchKernelGGL(k_classnni, dim3((unsigned)nblk, (unsigned)n), dim3(GenGeo<2>::WAVES * 64), 0, e->stream, a);
	}
	hipLaunchKernelGGL(k_nni_finish, dim3((unsigned)(((size_t)9 * N + 255) / 256)), dim3(256), 0, e->stream, N, nblk, e->d_nni_cand_of.get(), e->d_nni_slab.get(),
	                   e->d_nni_out.get());
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(out, e->d_nni_out, sizeof(double) * (size_t)9 * N, hipMemcpyDeviceToHost, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream));  // (also covers the records, the index and `trial`)
	return PHYAMD_OK;
}

// out [3 terms][3][N] on the host; deriv: d1 and d2 as well (else those rows are NaN at tips and the root, 0 elsewhere)
int shard_nni_general(Shard *e, int flags, const double *central_lengths, bool deriv, double *out) {
	CHECK_ENGINE(e);
	return profiled_call(e, &Shard::nni_prof, phyamd_nni_profile{}, [&](phyamd_nni_profile &prof) {
		const int rc = run_nni_general(e, flags, central_lengths, deriv, out, prof);
		if (!rc) nni_mask_derivatives((size_t)3 * e->N, out);
		return rc;
	});
}

// ---- the optimised central branch of every NNI neighbour (phyamd_nni_optimize) ------------------------------------------------

// the walk's (nni_base_plan: its [3][N] lengths are the start lengths), and for the `chunk` candidates that run at once the
// coefficients and the results of their three entries (sizes: d_cbopt_K, d_cbopt_out, d_cbopt_iter)
ScratchPlan cbopt_plan(Shard *e, size_t chunk) {
	const size_t D = sizeof(double), C = (size_t)e->C, nblk = ((size_t)e->P + WAVE - 1) / WAVE;
	ScratchPlan p = nni_base_plan(e);
	p.add(e->d_cbopt_K, 0, chunk * D * 3 * C * 4 * nblk * WAVE);
	p.add(e->d_cbopt_out, 0, chunk * D * 3 * 4);
	p.add(e->d_cbopt_iter, 0, chunk * sizeof(int32_t) * 3);
	return p;
}

// the candidates of a chunk under plan_of(chunk), whose fixed bytes grow with the chunk: all of them (at most gridDim.y's) if the
// scratch holds as much or has room for it, else what fits beside the part that does not grow (0: not even one)
template <typename PlanOf>
size_t candidates_that_fit(Shard *e, size_t cands, PlanOf plan_of) {
	const size_t want = std::min<size_t>(cands, BATCH_MAX_CHUNK);
	if (batch_items_held(e, plan_of(want)) >= 1) return want;
	const ScratchPlan none = plan_of(0), one = plan_of(1);
	const double walk = (double)(none.fixed_bytes() + none.item_bytes()), per = (double)(one.fixed_bytes() - none.fixed_bytes());
	const double fit = std::floor((scratch_room(e, (double)batch_scratch_bytes(e), EngineRoom::MayGrow) - walk) / per);
	return fit < 1.0 ? 0 : (size_t)std::min((double)want, fit);
}
size_t cbopt_chunk(Shard *e, size_t cands) {
	return candidates_that_fit(e, cands, [e](size_t chunk) { return cbopt_plan(e, chunk); });
}

struct NniOptimizeArgs {
	const double *start;
	double lower, upper, tolerance;
	int32_t max_iterations;
	double *lengths, *lnl, *d1, *d2;
	int32_t *iterations;
};

// one walk of the engine's tree with every upper parked, then chunk by chunk the candidates' coefficients and their iterations.
// Reads the engine's inputs and writes only the batch scratch: nothing in Shard::state changes
int run_nni_optimize(Shard *e, int flags, const NniOptimizeArgs &o, phyamd_nni_optimize_profile &prof) {
	static const NniWalkCall call{"phyamd_nni_optimize", "start_lengths", "start length", "the likelihood in the central length is"};
	int rc;
	std::vector<double> start;
	if ((rc = check_nni_walk(e, call, flags, o.start, start))) return rc;
	const int T = e->T, N = e->N, C = e->C;
	const size_t cands = nni_candidates(e), entries = (size_t)3 * N;
	prof.candidates = (int32_t)cands;
	std::fill(o.lengths, o.lengths + entries, NAN);
	std::fill(o.lnl, o.lnl + entries, NAN);
	if (o.d1) std::fill(o.d1, o.d1 + entries, NAN);
	if (o.d2) std::fill(o.d2, o.d2 + entries, NAN);
	if (o.iterations) std::fill(o.iterations, o.iterations + entries, 0);
	if (cands == 0) return PHYAMD_OK;  // two tips: no internal edge
	const size_t chunk = cbopt_chunk(e, cands);
	if (chunk < 1) {
		const ScratchPlan one = cbopt_plan(e, 1);
		return fail(PHYAMD_EUNSUPPORTED, "%s: the scratch of one candidate (%zu bytes: every internal node's lower and upper partial, and its entries' coefficients) does not fit the memory budget",
		            call.name, one.fixed_bytes() + one.item_bytes());
	}
	if ((rc = launch_nni_walk(e, cbopt_plan(e, chunk), start, false))) return rc;
	const int nblk = (e->P + WAVE - 1) / WAVE;
	HIP_TRY(hipGetLastError());
	// (the candidates' nodes in d_nni_cands' order: upload_nni_lists')
	std::vector<int> node;
	for (int v = T; v < N; v++)
		if (v != e->root) node.push_back(v);
	std::vector<double> out;
	std::vector<int32_t> iter;
	for (size_t first = 0; first < cands; first += chunk) {
		const size_t n = std::min(chunk, cands - first);
		const CboptCoeffArgs ca{e->d_nni_cands.get() + first, T, N, e->P, C, nblk, e->d_tipmask, e->d_freqs, e->d_props, e->d_model, e->d_batch_mats, e->d_batch_lower,
		                        e->d_batch_upper, e->d_cbopt_K};
		hipLaunchKernelGGL(k_cbopt_coeff4, dim3(nblk, (unsigned)n), dim3(WAVE, C), 0, e->stream, ca);
		const CboptSolveArgs sa{e->d_nni_cands.get() + first, N, e->P, C, nblk * WAVE, o.max_iterations, o.lower, o.upper, o.tolerance, e->d_model, e->d_rates, e->d_weights,
		                        e->d_nni_len, e->d_cbopt_K, e->d_cbopt_out, e->d_cbopt_iter};
		hipLaunchKernelGGL(k_cbopt_solve4, dim3((unsigned)(3 * n)), dim3(CBOPT_THREADS), 0, e->stream, sa);
		HIP_TRY(hipGetLastError());
		out.resize(n * 12);
		iter.resize(n * 3);
		HIP_TRY(hipMemcpyAsync(out.data(), e->d_cbopt_out, sizeof(double) * out.size(), hipMemcpyDeviceToHost, e->stream));
		HIP_TRY(hipMemcpyAsync(iter.data(), e->d_cbopt_iter, sizeof(int32_t) * iter.size(), hipMemcpyDeviceToHost, e->stream));
		HIP_TRY(hipStreamSynchronize(e->stream));  // (also covers `start`)
		prof.chunks++;
		for (size_t i = 0; i < n; i++)
			for (int k = 0; k < 3; k++) {
				const double *r = &out[(i * 3 + k) * 4];
				const size_t at = (size_t)k * N + node[first + i];
				o.lengths[at] = r[0];
				o.lnl[at] = r[1];
				if (o.d1) o.d1[at] = r[2];
				if (o.d2) o.d2[at] = r[3];
				if (o.iterations) o.iterations[at] = iter[i * 3 + k];
				prof.iterations += std::abs(iter[i * 3 + k]);
			}
	}
	return PHYAMD_OK;
}

int shard_nni_optimize(Shard *e, int flags, const NniOptimizeArgs &o) {
	CHECK_ENGINE(e);
	return profiled_call(e, &Shard::cbopt_prof, phyamd_nni_optimize_profile{}, [&](phyamd_nni_optimize_profile &prof) { return run_nni_optimize(e, flags, o, prof); });
}

// ---- the optimised central branch of every NNI neighbour of a 20-state engine's tree (phyamd_nni_optimize_general) ---------------

// nothing is walked: the candidates, their index by node, the images of V^T and V^-1 and the caller's [3][N] start lengths, and for
// the `chunk` candidates that run at once the coefficients and the results of their three entries
ScratchPlan classcb_plan(Shard *e, size_t chunk) {
	const size_t D = sizeof(double), N = (size_t)e->N, C = (size_t)e->C, cands = std::max<size_t>(nni_candidates(e), 1);
	ScratchPlan p;
	p.add(e->d_nnig_cands, 0, sizeof(ClassNniCand) * cands);
	p.add(e->d_nnig_eig, 0, D * 2 * MatImage<2, 5>::SIZE);
	p.add(e->d_nni_cand_of, 0, sizeof(int32_t) * N);
	p.add(e->d_nni_len, 0, D * 3 * N);
	p.add(e->d_classcb_K, 0, chunk * D * 3 * C * PLACE_GEN_STATES * (size_t)e->Pp);
	p.add(e->d_classcb_out, 0, chunk * D * 3 * 4);
	p.add(e->d_classcb_iter, 0, chunk * sizeof(int32_t) * 3);
	return p;
}

// the four messages round every candidate edge read from the resident partials, then chunk by chunk the candidates' coefficients
// and their iterations.  Writes only the batch scratch beyond the evaluation that made the partials resident
int run_nni_optimize_general(Shard *e, int flags, const NniOptimizeArgs &o, phyamd_nni_optimize_profile &prof) {
	static const GeneralQueryCall call{"phyamd_nni_optimize_general", "the kernels are", "phyamd_nni_optimize", "64-wide products are",
	                                   "which have no exponential sum in the central length", "the likelihood in the central length is", "coefficients do"};
	int rc;
	if ((rc = check_general_query_inputs(e, call, flags))) return rc;
	const int T = e->T, N = e->N, C = e->C, P = e->P, root = e->root;
	std::vector<double> start((size_t)3 * N);  // a candidate's own three where the caller gives them, every other entry the engine's (not read)
	for (int k = 0; k < 3; k++) std::copy(e->lengths.begin(), e->lengths.end(), start.begin() + (size_t)k * N);
	for (int v = T; v < N && o.start; v++) {
		if (v == root) continue;
		for (int k = 0; k < 3; k++) {
			const double t = o.start[(size_t)k * N + v];
			if (!std::isfinite(t) || t < 0.0) return fail(PHYAMD_EINVAL, "%s: start_lengths[%d][%d] = %g: a start length is finite and not negative", call.name, k, v, t);
			start[(size_t)k * N + v] = t;
		}
	}
	if ((rc = check_general_query_resident(e, call))) return rc;
	const size_t cands = nni_candidates(e), entries = (size_t)3 * N;
	prof.candidates = (int32_t)cands;
	std::fill(o.lengths, o.lengths + entries, NAN);
	std::fill(o.lnl, o.lnl + entries, NAN);
	if (o.d1) std::fill(o.d1, o.d1 + entries, NAN);
	if (o.d2) std::fill(o.d2, o.d2 + entries, NAN);
	if (o.iterations) std::fill(o.iterations, o.iterations + entries, 0);
	if (cands == 0) return PHYAMD_OK;  // two tips: no internal edge
	const size_t chunk = candidates_that_fit(e, cands, [e](size_t n) { return classcb_plan(e, n); });
	if (chunk < 1) {
		const ScratchPlan one = classcb_plan(e, 1);
		return fail(PHYAMD_EUNSUPPORTED, "%s: the scratch of one candidate (%zu bytes: the candidates, and its entries' coefficients) does not fit the memory budget", call.name,
		            one.fixed_bytes() + one.item_bytes());
	}
	if ((rc = ensure_batch_scratch(e, 1, classcb_plan(e, chunk)))) return rc;
	std::vector<ClassNniCand> records;
	std::vector<int32_t> cand_of;
	if ((rc = upload_classnni_records(e, call.name, records, cand_of))) return rc;
	HIP_TRY(hipMemcpyAsync(e->d_nni_len, start.data(), sizeof(double) * start.size(), hipMemcpyHostToDevice, e->stream));
	launch_classnni_eigen_images(e);
	const int nblk = (P + CLASSNNI_BLOCK - 1) / CLASSNNI_BLOCK;
	std::vector<double> out;
	std::vector<int32_t> iter;
	for (size_t first = 0; first < cands; first += chunk) {
		const size_t n = std::min(chunk, cands - first);
		const ClassCbCoeffArgs ca{e->d_nnig_cands.get() + first, P, e->Pp, C, e->upper_fold ? 1 : 0, e->d_tipmask, e->d_tipsets, e->d_freqs, e->d_props, e->d_imgs, e->d_nnig_eig,
		                          e->d_classcb_K};
		hipLaunchKernelGGL(k_classcb_coeff, dim3((unsigned)nblk, (unsigned)n), dim3(GenGeo<2>::WAVES * 64), 0, e->stream, ca);
		const ClassCbSolveArgs sa{e->d_nnig_cands.get() + first, N, P, e->Pp, C, o.max_iterations, o.lower, o.upper, o.tolerance, e->d_model, e->d_rates, e->d_weights,
		                          e->d_nni_len, e->d_classcb_K, e->d_classcb_out, e->d_classcb_iter};
		hipLaunchKernelGGL(k_classcb_solve, dim3((unsigned)(3 * n)), dim3(CLASSOPT_THREADS), 0, e->stream, sa);
		HIP_TRY(hipGetLastError());
		out.resize(n * 12);
		iter.resize(n * 3);
		HIP_TRY(hipMemcpyAsync(out.data(), e->d_classcb_out, sizeof(double) * out.size(), hipMemcpyDeviceToHost, e->stream));
		HIP_TRY(hipMemcpyAsync(iter.data(), e->d_classcb_iter, sizeof(int32_t) * iter.size(), hipMemcpyDeviceToHost, e->stream));
		HIP_TRY(hipStreamSynchronize(e->stream));  // (also covers the records, the index and `start`)
		prof.chunks++;
		for (size_t i = 0; i < n; i++)
			for (int k = 0; k < 3; k++) {
				const double *r = &out[(i * 3 + k) * 4];
				const size_t at = (size_t)k * N + records[first + i].v;
				o.lengths[at] = r[0];
				o.lnl[at] = r[1];
				if (o.d1) o.d1[at] = r[2];
				if (o.d2) o.d2[at] = r[3];
				if (o.iterations) o.iterations[at] = iter[i * 3 + k];
				prof.iterations += std::abs(iter[i * 3 + k]);
			}
	}
	return PHYAMD_OK;
}

int shard_nni_optimize_general(Shard *e, int flags, const NniOptimizeArgs &o) {
	CHECK_ENGINE(e);
	return profiled_call(e, &Shard::cbopt_prof, phyamd_nni_optimize_profile{}, [&](phyamd_nni_optimize_profile &prof) { return run_nni_optimize_general(e, flags, o, prof); });
}

// ---- all branch lengths of a batch of trees (phyamd_optimize_branch_lengths) -----------------------------------------------------

// per item: the lnL-only walk's of a batch of trees (batch_plan: lengths, matrices, lnL, every internal lower, op lists, root), a
// plane O_n per node, the visited branch's coefficients, the tour's ops and visit slots, the mask, lnL before and now, the status
ScratchPlan blopt_plan(Shard *e) {
	const size_t D = sizeof(double), N = (size_t)e->N, C = (size_t)e->C, nblk = ((size_t)e->P + WAVE - 1) / WAVE, plane = nblk * WAVE * 4;
	ScratchPlan p = batch_plan(e, false, 1, true);
	p.add(e->d_blopt_O, D * N * C * plane);
	p.add(e->d_blopt_K, D * C * plane);
	p.add(e->d_blopt_ops, sizeof(BloptOp) * 3 * (size_t)(e->T - 1));
	p.add(e->d_blopt_visits, sizeof(BloptVisit) * 2 * (size_t)(e->T - 1));
	p.add(e->d_blopt_mask, N);
	p.add(e->d_blopt_lnl, D * 2);
	p.add(e->d_blopt_status, sizeof(int32_t) * BLOPT_STATUS);
	return p;
}

struct BranchOptimizeArgs {
	int32_t count;
	const int32_t *left, *right, *roots;
	const double *start;
	const uint8_t *optimise;
	double lower, upper, tolerance;
	int32_t max_iterations;
	double lnl_tolerance;
	int32_t max_passes;
	double *lengths, *lnl, *initial_lnl;
	int32_t *passes;
};

// the items in chunks of what the scratch holds (for_tree_chunks); per chunk the lnL-only walk of the tree batch, then pass after
// pass every visit slot's two launches, enqueued without a wait; the status words come back once per pass.  Reads the engine's
// inputs and writes only the batch scratch: nothing in Shard::state changes
int run_branch_optimize(Shard *e, int flags, const BranchOptimizeArgs &o, phyamd_branch_optimize_profile &prof) {
	static const char *const name = "phyamd_optimize_branch_lengths";
	int rc;
	if ((rc = check_ready_but_lengths(e))) return fail(rc, "%s: the engine is not ready: %s", name, std::string(g_last_error).c_str());
	if (flags != 0) return fail(PHYAMD_EUNSUPPORTED, "%s: flags %d (no flags are defined: pass 0)", name, flags);
	if (const char *why = tree_batch_refusal(e, 0, 1)) return fail(PHYAMD_EUNSUPPORTED, "%s: %s", name, why);
	if (!e->have_eigen) return fail(PHYAMD_EINVAL, "%s needs the eigen system (phyamd_set_eigen): the likelihood in a branch length is formed from it", name);
	const int T = e->T, C = e->C, nblk = (e->P + WAVE - 1) / WAVE, nvisits = 2 * (T - 1), nops = 3 * (T - 1);
	const size_t N = (size_t)e->N, count = (size_t)o.count;
	const int32_t *left = o.left, *right = o.right, *roots = o.roots;
	std::vector<int32_t> own_left, own_right, own_roots;
	if (!left) {  // every item is the engine's tree
		for (size_t b = 0; b < count; b++) {
			own_left.insert(own_left.end(), e->left.begin(), e->left.end());
			own_right.insert(own_right.end(), e->right.begin(), e->right.end());
		}
		own_roots.assign(count, e->root);
		left = own_left.data(), right = own_right.data(), roots = own_roots.data();
	}
	// every item before anything is launched: its tree, then the start lengths of the nodes it visits
	std::vector<uint8_t> mask(count * N, 1);
	{
		std::vector<int32_t> parents;
		for (size_t b = 0; b < count; b++) {
			const std::string err = validate_tree(TreeRef{T, left + b * N, right + b * N, roots[b]}, parents, name, (int)b);
			if (!err.empty()) return fail(PHYAMD_EINVAL, "%s", err.c_str());
			for (size_t n = 0; n < N; n++) {
				uint8_t &m = mask[b * N + n];
				m = (int32_t)n != roots[b] && (!o.optimise || o.optimise[b * N + n]) ? 1 : 0;
				const double t = o.start[b * N + n];
				if (m && (!std::isfinite(t) || t < 0.0))
					return fail(PHYAMD_EINVAL, "%s: item %zu: branch_lengths[%zu] = %g: the start length of a visited node is finite and not negative", name, b, n, t);
			}
		}
	}
	std::copy(o.start, o.start + count * N, o.lengths);
	std::vector<SweepOp> sweep;
	std::vector<BloptOp> ops;
	std::vector<BloptVisit> visits;
	std::vector<double> out, lnl2, len;
	std::vector<int32_t> status;
	const auto item_ops = [&](const int32_t *l, const int32_t *r, int32_t root, std::vector<BatchOp> *list) { return list ? build_batch_ops(T, l, r, root, list) : 1; };
	const auto plan_of = [&](int) { return blopt_plan(e); };
	const auto chunk = [&](size_t first, size_t items, int, const double *lengths, auto, auto) -> int {
		// the tours, and which items have anything to visit
		ops.assign(items * nops, BloptOp{});
		visits.assign(items * nvisits, BloptVisit{});
		status.assign(items * BLOPT_STATUS, 0);
		for (size_t b = 0; b < items; b++) {
			sweep.clear();
			build_branch_sweep(T, left + (first + b) * N, right + (first + b) * N, roots[first + b], &sweep);
			BloptOp *io = &ops[b * nops];
			BloptVisit *iv = &visits[b * nvisits];
			int32_t at = 0;
			for (const SweepOp &s : sweep) {
				if (s.kind != SWEEP_VISIT) {
					io[at++] = BloptOp{s.kind, s.node, s.a, s.b, {0, 0, 0, 0}};
					continue;
				}
				iv[s.visit] = BloptVisit{s.node, s.visit ? iv[s.visit - 1].end : 0, at, s.visit + 1 == nvisits ? 1 : 0, {0, 0, 0, 0}};
			}
			const uint8_t *m = &mask[(first + b) * N];
			if (!std::any_of(m, m + N, [](uint8_t x) { return x != 0; })) status[b * BLOPT_STATUS + BLOPT_DONE] = 1;  // (passes: 0)
		}
		HIP_TRY(hipMemcpyAsync(e->d_blopt_ops, ops.data(), sizeof(BloptOp) * ops.size(), hipMemcpyHostToDevice, e->stream));
		HIP_TRY(hipMemcpyAsync(e->d_blopt_visits, visits.data(), sizeof(BloptVisit) * visits.size(), hipMemcpyHostToDevice, e->stream));
		HIP_TRY(hipMemcpyAsync(e->d_blopt_mask, &mask[first * N], items * N, hipMemcpyHostToDevice, e->stream));
		HIP_TRY(hipMemcpyAsync(e->d_blopt_status, status.data(), sizeof(int32_t) * status.size(), hipMemcpyHostToDevice, e->stream));
		// the start state: the tree batch's lnL-only walk leaves the items' lengths, matrices and every internal lower resident
		out.resize(items);
		if (int rc = run_batch_chunk(e, 0, (int)items, lengths, false, 1, true, out.data())) return rc;
		lnl2.resize(items * 2);
		for (size_t b = 0; b < items; b++) lnl2[2 * b] = lnl2[2 * b + 1] = out[b];
		HIP_TRY(hipMemcpyAsync(e->d_blopt_lnl, lnl2.data(), sizeof(double) * lnl2.size(), hipMemcpyHostToDevice, e->stream));
		BloptStepArgs sa{};
		sa.ops = e->d_blopt_ops, sa.visits = e->d_blopt_visits, sa.ops_stride = nops, sa.visits_stride = nvisits;
		sa.T = T, sa.N = e->N, sa.P = e->P, sa.C = C, sa.nblk = nblk;
		sa.tipmask = e->d_tipmask, sa.freqs = e->d_freqs, sa.props = e->d_props, sa.model = e->d_model, sa.optimise = e->d_blopt_mask, sa.status = e->d_blopt_status;
		sa.mats = e->d_batch_mats, sa.lower = e->d_batch_lower, sa.O = e->d_blopt_O, sa.K = e->d_blopt_K;
		BloptSolveArgs so{};
		so.visits = e->d_blopt_visits, so.visits_stride = nvisits, so.max_passes = o.max_passes;
		so.N = e->N, so.P = e->P, so.C = C, so.Pp = nblk * WAVE, so.max_iterations = o.max_iterations;
		so.lower = o.lower, so.upper = o.upper, so.tolerance = o.tolerance, so.lnl_tolerance = o.lnl_tolerance;
		so.model = e->d_model, so.rates = e->d_rates, so.weights = e->d_weights, so.optimise = e->d_blopt_mask, so.K = e->d_blopt_K;
		so.lengths = e->d_batch_len, so.mats = e->d_batch_mats, so.lnl = e->d_blopt_lnl, so.status = e->d_blopt_status;
		const auto all_done = [&] {
			for (size_t b = 0; b < items; b++)
				if (!status[b * BLOPT_STATUS + BLOPT_DONE]) return false;
			return true;
		};
		int32_t pass = 0;
		while (!all_done()) {  // (ends after max_passes: the last pass's stop test ends every item)
			if (++pass > o.max_passes) return fail(PHYAMD_EDEVICE, "%s: an item of chunk %d is not done after %d passes", name, prof.chunks, o.max_passes);
			for (int i = 0; i < nvisits; i++) {
				sa.step = so.step = i;
				so.pass = pass;
				hipLaunchKernelGGL(k_blopt_step4, dim3((unsigned)nblk, (unsigned)items), dim3(WAVE, C), 0, e->stream, sa);
				hipLaunchKernelGGL(k_blopt_solve4, dim3((unsigned)items), dim3(CBOPT_THREADS), 0, e->stream, so);
			}
			HIP_TRY(hipGetLastError());
			HIP_TRY(hipMemcpyAsync(status.data(), e->d_blopt_status, sizeof(int32_t) * status.size(), hipMemcpyDeviceToHost, e->stream));
			HIP_TRY(hipStreamSynchronize(e->stream));
		}
		prof.passes = std::max(prof.passes, pass);
		len.resize(items * N);
		HIP_TRY(hipMemcpyAsync(len.data(), e->d_batch_len, sizeof(double) * len.size(), hipMemcpyDeviceToHost, e->stream));
		HIP_TRY(hipMemcpyAsync(lnl2.data(), e->d_blopt_lnl, sizeof(double) * lnl2.size(), hipMemcpyDeviceToHost, e->stream));
		HIP_TRY(hipStreamSynchronize(e->stream));
		prof.chunks++;
		for (size_t b = 0; b < items; b++) {
			const size_t at = first + b;
			for (size_t n = 0; n < N; n++)  // (the root's entry and those of nodes that are not visited stay the caller's)
				if (mask[at * N + n]) o.lengths[at * N + n] = len[b * N + n];
			o.lnl[at] = lnl2[2 * b + 1];
			if (o.initial_lnl) o.initial_lnl[at] = out[b];
			if (o.passes) o.passes[at] = status[b * BLOPT_STATUS + BLOPT_PASSES];
			prof.visits += status[b * BLOPT_STATUS + BLOPT_VISITS];
			prof.iterations += status[b * BLOPT_STATUS + BLOPT_ITERATIONS];
		}
		return PHYAMD_OK;
	};
	return for_tree_chunks(e, name, 0, o.count, left, right, roots, o.start, item_ops, plan_of, chunk);
}

int shard_branch_optimize(Shard *e, int flags, const BranchOptimizeArgs &o) {
	CHECK_ENGINE(e);
	phyamd_branch_optimize_profile known{};
	known.items = o.count;
	return profiled_call(e, &Shard::blopt_prof, known, [&](phyamd_branch_optimize_profile &prof) { return run_branch_optimize(e, flags, o, prof); });
}

// ---- every SPR regraft of chosen subtrees (phyamd_spr_log_likelihoods) ---------------------------------------------------------

// the engine's tree's park_all op lists, where each internal node's op is in them, and every node's depth-first interval
void ensure_spr_lists(Shard *e) {
	if (!e->state.spr_lists_dirty) return;
	const int T = e->T, N = e->N, nops = T - 1;
	e->spr_ops.clear();
	build_batch_ops(T, e->left.data(), e->right.data(), e->root, &e->spr_ops, true);
	e->spr_lower_at.assign(N, -1);
	e->spr_upper_at.assign(N, -1);
	for (int i = 0; i < nops; i++) e->spr_lower_at[e->spr_ops[i].node] = i, e->spr_upper_at[e->spr_ops[nops + i].node] = i;
	e->spr_tin.assign(N, 0);
	e->spr_tout.assign(N, 0);
	int32_t clock = 0;
	std::vector<std::pair<int, bool>> stack{{e->root, false}};
	while (!stack.empty()) {
		const auto [n, done] = stack.back();
		stack.pop_back();
		if (done) {
			e->spr_tout[n] = clock;
			continue;
		}
		e->spr_tin[n] = clock++;
		stack.push_back({n, true});
		if (n >= T) stack.push_back({e->right[n], false}), stack.push_back({e->left[n], false});
	}
	spr_lists_rebuilt(e);
}

// row p (not the root, not a child of it) into a chunk's lists: its op lists -- the engine's with p a ghost in its parent's two
// ops, and nothing parked in p's subtree -- appended to `ops`, its candidates to `cands`, their indices into cand_of [N]
void build_spr_row(const Shard *e, int row, int p, std::vector<BatchOp> *ops, std::vector<SprCand> *cands, int32_t *cand_of) {
	const int T = e->T, N = e->N, nops = T - 1;
	const int u = e->sched.parent[p], s = e->left[u] == p ? e->right[u] : e->left[u];
	const auto below_p = [&](int n) { return e->spr_tin[p] <= e->spr_tin[n] && e->spr_tin[n] < e->spr_tout[p]; };
	const size_t first = ops->size();
	ops->insert(ops->end(), e->spr_ops.begin(), e->spr_ops.end());
	BatchOp &up = (*ops)[first + e->spr_lower_at[u]], &down = (*ops)[first + nops + e->spr_upper_at[u]];
	if (up.left == p) up.left = BATCH_GHOST, up.carry = up.carry == 1 ? 0 : up.carry;
	else up.right = BATCH_GHOST, up.carry = up.carry == 2 ? 0 : up.carry;
	if (down.left == p) down.left = BATCH_GHOST, down.dst_left = BATCH_NONE;
	else down.right = BATCH_GHOST, down.dst_right = BATCH_NONE;
	for (int i = 0; i < nops; i++) {
		BatchOp &op = (*ops)[first + nops + i];
		if (below_p(op.node)) op.dst_left = op.dst_right = BATCH_NONE;
	}
	for (int w = 0; w < N; w++) {
		cand_of[w] = -1;
		if (w == e->root || w == u || w == s || below_p(w)) continue;
		const int x = e->sched.parent[w];
		cand_of[w] = (int32_t)cands->size();
		cands->push_back(SprCand{row, w, x == e->root ? BATCH_ROOT : x, e->left[x] == w ? e->right[x] : e->left[x], p, e->left[u] == p ? 1 : 0, {0, 0}});
	}
}

// the prune list of an SPR call (`name`), 4 or 20 states: null with the node count, or ids; live: the indices of the rows that have
// candidates -- p is neither the root nor a child of it
int check_prune_list(const Shard *e, const char *name, int32_t count, const int32_t *prune, std::vector<int32_t> &live) {
	const int N = e->N;
	if (!prune && count != N) return fail(PHYAMD_EINVAL, "%s: prune is null, so count must be the node count %d (got %d)", name, N, count);
	for (int32_t i = 0; i < count; i++) {
		const int p = prune ? prune[i] : i;
		if (p < 0 || p >= N) return fail(PHYAMD_EINVAL, "%s: prune[%d] = %d is not a node id (0..%d)", name, i, p, N - 1);
		if (p != e->root && e->sched.parent[p] != e->root) live.push_back(i);
	}
	return PHYAMD_OK;
}

// what phyamd_spr_log_likelihoods and phyamd_spr_optimize (`name`) check alike
int check_spr_call(Shard *e, const char *name, const char *eigen_use, int flags, int32_t count, const int32_t *prune, std::vector<int32_t> &live) {
	int rc;
	if ((rc = check_ready(e))) return rc;
	if (flags != 0) return fail(PHYAMD_EUNSUPPORTED, "%s: flags %d (no flags are defined: pass 0)", name, flags);
	if (const char *why = tree_batch_refusal(e, 0, 1)) return fail(PHYAMD_EUNSUPPORTED, "%s: %s", name, why);
	if (!e->have_eigen) return fail(PHYAMD_EINVAL, "%s needs the eigen system (phyamd_set_eigen): %s", name, eigen_use);
	return check_prune_list(e, name, count, prune, live);
}

// the live rows in chunks of what the scratch holds of `plan`; per chunk the rows' lists built and sent, the matrices of the
// engine's lengths (and, halves: of half of them behind) and k_spr_walk4, then body(first, rows, cands, mats) -- which ends with
// the stream synchronised, since the next chunk builds the lists anew.  row_holds: what a row's scratch is, for the refusal
template <typename Body>
int for_spr_row_chunks(Shard *e, const char *name, const char *row_holds, const ScratchPlan &plan, const std::vector<int32_t> &live, const int32_t *prune, bool halves,
                       Body body) {
	const int T = e->T, N = e->N, C = e->C, nblk = (e->P + WAVE - 1) / WAVE;
	int rc;
	ensure_spr_lists(e);
	std::vector<double> lengths((size_t)2 * N);
	for (int n = 0; n < N; n++) lengths[n] = e->lengths[n], lengths[N + n] = 0.5 * e->lengths[n];
	std::vector<BatchOp> ops;
	std::vector<SprCand> cands;
	std::vector<int32_t> cand_of;
	for (size_t first = 0; first < live.size();) {
		const size_t rows = std::min(batch_items_that_fit(e, live.size() - first, plan), live.size() - first);
		if (rows < 1) return fail(PHYAMD_EUNSUPPORTED, "%s: the scratch of one row (%zu bytes: %s) does not fit the memory budget", name, plan.item_bytes(), row_holds);
		if ((rc = ensure_batch_scratch(e, rows, plan))) return rc;
		ops.clear();
		cands.clear();
		cand_of.resize(rows * N);
		for (size_t r = 0; r < rows; r++) {
			const int32_t i = live[first + r];
			build_spr_row(e, (int)r, prune ? prune[i] : i, &ops, &cands, cand_of.data() + r * N);
		}
		HIP_TRY(hipMemcpyAsync(e->d_batch_item_ops, ops.data(), sizeof(BatchOp) * ops.size(), hipMemcpyHostToDevice, e->stream));
		HIP_TRY(hipMemcpyAsync(e->d_spr_cands, cands.data(), sizeof(SprCand) * cands.size(), hipMemcpyHostToDevice, e->stream));
		HIP_TRY(hipMemcpyAsync(e->d_spr_cand_of, cand_of.data(), sizeof(int32_t) * cand_of.size(), hipMemcpyHostToDevice, e->stream));
		HIP_TRY(hipMemcpyAsync(e->d_spr_len, lengths.data(), sizeof(double) * lengths.size(), hipMemcpyHostToDevice, e->stream));
		launch_batch_matrices(e, halves ? 2 : 1, e->d_spr_len, nullptr, e->d_spr_mats);  // the engine's lengths, then their halves
		const double *mats = e->d_spr_mats.get();
		const SprWalkArgs walk{e->d_batch_item_ops.get(), T, N, e->P, C, nblk, e->d_tipmask, mats, e->d_batch_lower, e->d_batch_upper};
		hipLaunchKernelGGL(k_spr_walk4, dim3(nblk, (unsigned)rows), dim3(WAVE, C), 0, e->stream, walk);
		if ((rc = body(first, rows, cands, mats))) return rc;
		first += rows;
	}
	return PHYAMD_OK;
}

// lnl [count][N] (host).  Reads the engine's inputs and writes only the batch scratch: nothing in Shard::state changes but the
// record that the host lists are the tree's
int run_spr(Shard *e, int flags, int32_t count, const int32_t *prune, double *lnl, phyamd_spr_profile &prof) {
	static const char *const name = "phyamd_spr_log_likelihoods";
	int rc;
	std::vector<int32_t> live;
	if ((rc = check_spr_call(e, name, "the half-length matrices are formed from it", flags, count, prune, live))) return rc;
	const int T = e->T, N = e->N, C = e->C, nblk = (e->P + WAVE - 1) / WAVE;
	std::fill(lnl, lnl + (size_t)count * N, NAN);
	prof.prunes = count;
	if (live.empty()) return PHYAMD_OK;
	std::vector<double> out;
	return for_spr_row_chunks(e, name, "every internal node's lower and upper partial", spr_plan(e), live, prune, true,
	                          [&](size_t first, size_t rows, const std::vector<SprCand> &cands, const double *mats) -> int {
		const double *half = mats + (size_t)N * C * 16;
		for (size_t c0 = 0; c0 < cands.size(); c0 += BATCH_MAX_CHUNK) {  // (gridDim.y)
			const size_t n = std::min<size_t>(cands.size() - c0, BATCH_MAX_CHUNK);
			const SprArgs a{e->d_spr_cands.get() + c0, T, N, e->P, C, nblk, e->d_tipmask, e->d_freqs, e->d_props, e->d_weights, mats, half, e->d_batch_lower, e->d_batch_upper,
			                e->d_spr_slab.get() + c0 * nblk};
			hipLaunchKernelGGL(k_spr4, dim3(nblk, (unsigned)n), dim3(WAVE, C), 0, e->stream, a);
		}
		const size_t cells = rows * N;
		hipLaunchKernelGGL(k_spr_finish, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, e->stream, cells, nblk, e->d_spr_cand_of.get(), e->d_spr_slab.get(),
		                   e->d_spr_out.get());
		HIP_TRY(hipGetLastError());
		out.resize(cells);
		HIP_TRY(hipMemcpyAsync(out.data(), e->d_spr_out, sizeof(double) * cells, hipMemcpyDeviceToHost, e->stream));
		HIP_TRY(hipStreamSynchronize(e->stream));  // (also covers the lists, which the next chunk builds anew)
		for (size_t r = 0; r < rows; r++) std::copy(out.begin() + r * N, out.begin() + (r + 1) * N, lnl + (size_t)live[first + r] * N);
		prof.chunks++;
		prof.candidates += (int64_t)cands.size();
		return PHYAMD_OK;
	});
}

int shard_spr_log_likelihoods(Shard *e, int flags, int32_t count, const int32_t *prune, double *lnl) {
	CHECK_ENGINE(e);
	return profiled_call(e, &Shard::spr_prof, phyamd_spr_profile{}, [&](phyamd_spr_profile &prof) { return run_spr(e, flags, count, prune, lnl, prof); });
}

// ---- every SPR regraft of chosen subtrees of a 20-state engine's tree (phyamd_spr_log_likelihoods_general) -----------------------

// an item is a ROW: its planes [C][20][Pp] -- the pruned tree's upper of every internal node by node, then `slots` path messages --,
// its ops and their count, its candidates, their index by cell, the slab (blocks of CLASSSPR_BLOCK patterns) and the result; whatever
// the row count: half the engine's lengths, their matrices and images
ScratchPlan spr_gen_plan(Shard *e, size_t slots, size_t nblk) {
	const size_t D = sizeof(double), N = (size_t)e->N, C = (size_t)e->C, ops = (size_t)(e->T - 1) + slots, matrix = (size_t)PLACE_GEN_STATES * PLACE_GEN_STATES;
	ScratchPlan p;
	p.add(e->d_sprg_work, D * ops * node_partial_doubles(e));
	p.add(e->d_sprg_ops, sizeof(ClassSprOp) * ops);
	p.add(e->d_sprg_nops, sizeof(int32_t));
	p.add(e->d_sprg_cands, sizeof(ClassSprCand) * N);
	p.add(e->d_spr_cand_of, sizeof(int32_t) * N);
	p.add(e->d_spr_slab, D * N * nblk);
	p.add(e->d_spr_out, D * N);
	p.add(e->d_placeg_len, 0, D * N);
	p.add(e->d_placeg_zero, 0, N);
	p.add(e->d_placeg_mats, 0, D * N * C * matrix);
	p.add(e->d_placeg_dmats, 0, D * N * C * matrix);
	p.add(e->d_placeg_imgs, 0, D * N * C * MatImage<2, 5>::SIZE);
	return p;
}

// row p (not the root, not a child of it) into a chunk's lists: its path ops and pre-order ops into ops[0..], their count returned;
// its candidates appended to `cands`, their indices into cand_of [N].  work: the row's planes; path: [N] nulls, and nulls again afterwards
int build_spr_gen_row(const Shard *e, int p, double *work, std::vector<const double *> &path, ClassSprOp *ops, std::vector<ClassSprCand> *cands, int32_t *cand_of) {
	const int T = e->T, N = e->N, nops = T - 1, root = e->root;
	const size_t npd = node_partial_doubles(e);
	const int u = e->sched.parent[p], s = e->left[u] == p ? e->right[u] : e->left[u];
	const auto below_p = [&](int n) { return e->spr_tin[p] <= e->spr_tin[n] && e->spr_tin[n] < e->spr_tout[p]; };
	const auto upper_of = [&](int n) { return work + (size_t)(n - T) * npd; };
	const auto message = [&](int n) {  // the pruned tree's message of n: a path message, the resident lower, or null for a tip
		return path[n] ? path[n] : n < T ? (const double *)nullptr : e->d_lower + (size_t)e->sched.core_index[n] * npd;
	};
	int count = 0, slot = 0;
	std::vector<int> on_path;
	const auto path_op = [&](int node, const double *ma, int a, const double *mb, int b) {
		double *dst = work + (size_t)(nops + slot++) * npd;
		ops[count++] = ClassSprOp{nullptr, ma, mb, dst, nullptr, node, a, b, 1, {0, 0}};
		path[node] = dst;
		on_path.push_back(node);
	};
	path_op(u, message(s), s, nullptr, -1);  // m'(slot of u) = P_u m_s
	for (int child = u, n = e->sched.parent[u]; n != root; child = n, n = e->sched.parent[n]) {
		const int sib = e->left[n] == child ? e->right[n] : e->left[n];
		path_op(n, path[child], child, message(sib), sib);
	}
	for (int i = 0; i < nops; i++) {
		const int x = e->spr_ops[nops + i].node;
		if (x == p || below_p(x)) continue;
		const int l = e->left[x], r = e->right[x];
		double *dl = l >= T && l != p ? upper_of(l) : nullptr, *dr = r >= T && r != p ? upper_of(r) : nullptr;
		if (!dl && !dr) continue;
		ops[count++] = ClassSprOp{x == root ? nullptr : upper_of(x), l == p ? nullptr : message(l), r == p ? nullptr : message(r), dl, dr, x, l == p ? -1 : l, r == p ? -1 : r, 0, {0, 0}};
	}
	const double *mp = p < T ? nullptr : e->d_lower + (size_t)e->sched.core_index[p] * npd;
	for (int w = 0; w < N; w++) {
		cand_of[w] = -1;
		if (w == root || w == u || w == s || below_p(w)) continue;
		const int x = e->sched.parent[w], y = e->left[x] == w ? e->right[x] : e->left[x];
		const int l = w < T ? -1 : e->left[w], r = w < T ? -1 : e->right[w];
		cand_of[w] = (int32_t)cands->size();
		cands->push_back(ClassSprCand{x == root ? nullptr : upper_of(x), message(y), w < T ? nullptr : message(l), w < T ? nullptr : message(r), mp, w, x, y, l, r, p});
	}
	for (const int n : on_path) path[n] = nullptr;
	return count;
}

// the preconditions of the two 20-state SPR calls up to the prune list, and every partial resident
int check_spr_general_call(Shard *e, const GeneralQueryCall &call, int flags, int32_t count, const int32_t *prune, std::vector<int32_t> &live) {
	int rc;
	if ((rc = check_general_query_inputs(e, call, flags))) {
		if (g_last_error.find(call.name) != std::string::npos) return rc;
		const std::string why = g_last_error;  // (an engine that is not ready: check_ready's words, which name no call)
		return fail(rc, "%s: %s", call.name, why.c_str());
	}
	if ((rc = check_prune_list(e, call.name, count, prune, live))) return rc;
	return check_general_query_resident(e, call);
}

// a chunk of rows of the two 20-state SPR calls, walked: the rows live[first .. first + rows), a row's planes `stride` apart in
// d_sprg_work (T - 1 uppers, then `slots` path messages), the rows' candidates one after the other and their index by cell
struct SprGenChunk {
	size_t first, rows, slots, stride;
	int nblk;
	const std::vector<ClassSprCand> *cands;
	const std::vector<int32_t> *cand_of;  // [rows][N]
};

// the live rows in chunks of what the scratch holds of plan_of(slots, nblk); per chunk the rows' lists built (build_spr_gen_row) and
// sent, halves: the matrices and images of half the engine's lengths, and k_classspr_walk, then body(chunk) -- which ends with the
// stream synchronised, since the next chunk builds the lists anew.  row_holds: what a row's scratch is, for the refusal
template <typename PlanOf, typename Body>
int for_spr_gen_row_chunks(Shard *e, const char *name, const char *row_holds, const std::vector<int32_t> &live, const int32_t *prune, bool halves, const PlanOf &plan_of,
                           const Body &body) {
	const int T = e->T, N = e->N, C = e->C, P = e->P, nops = T - 1;
	int rc;
	for (int n = T; n < N; n++)
		if (n != e->root && e->sched.core_index[n] < 0) return fail(PHYAMD_EDEVICE, "%s: node %d has no resident lower partial", name, n);
	ensure_spr_lists(e);
	std::vector<int32_t> depth(N, 0);
	size_t slots = 1;  // the depth of the deepest internal node: a row whose u lies at depth d forms d path messages
	for (int i = 0; i < nops; i++) {
		const int x = e->spr_ops[nops + i].node;
		depth[e->left[x]] = depth[e->right[x]] = depth[x] + 1;
		slots = std::max(slots, (size_t)depth[x]);
	}
	const int nblk = (P + CLASSSPR_BLOCK - 1) / CLASSSPR_BLOCK;
	const size_t npd = node_partial_doubles(e), stride = (size_t)nops + slots;
	const ScratchPlan plan = plan_of(slots, (size_t)nblk);
	std::vector<double> half(N);
	for (int n = 0; n < N; n++) half[n] = 0.5 * e->lengths[n];
	std::vector<ClassSprOp> ops;
	std::vector<int32_t> op_counts, cand_of;
	std::vector<ClassSprCand> cands;
	std::vector<const double *> path(N, nullptr);
	for (size_t first = 0; first < live.size();) {
		const size_t rows = std::min(batch_items_that_fit(e, live.size() - first, plan), live.size() - first);
		if (rows < 1) return fail(PHYAMD_EUNSUPPORTED, "%s: the scratch of one row (%zu bytes: %s) does not fit the memory budget", name, plan.item_bytes(), row_holds);
		if ((rc = ensure_batch_scratch(e, rows, plan))) return rc;
		ops.assign(rows * stride, ClassSprOp{});
		op_counts.resize(rows);
		cands.clear();
		cand_of.resize(rows * N);
		for (size_t r = 0; r < rows; r++) {
			const int32_t i = live[first + r];
			op_counts[r] = build_spr_gen_row(e, prune ? prune[i] : i, e->d_sprg_work.get() + r * stride * npd, path, ops.data() + r * stride, &cands, cand_of.data() + r * N);
		}
		HIP_TRY(hipMemcpyAsync(e->d_sprg_ops, ops.data(), sizeof(ClassSprOp) * ops.size(), hipMemcpyHostToDevice, e->stream));
		HIP_TRY(hipMemcpyAsync(e->d_sprg_nops, op_counts.data(), sizeof(int32_t) * rows, hipMemcpyHostToDevice, e->stream));
		HIP_TRY(hipMemcpyAsync(e->d_sprg_cands, cands.data(), sizeof(ClassSprCand) * cands.size(), hipMemcpyHostToDevice, e->stream));
		HIP_TRY(hipMemcpyAsync(e->d_spr_cand_of, cand_of.data(), sizeof(int32_t) * cand_of.size(), hipMemcpyHostToDevice, e->stream));
		if (halves) {  // half the engine's lengths: their matrices through the engine's own matrix kernel, and the images
			HIP_TRY(hipMemcpyAsync(e->d_placeg_len, half.data(), sizeof(double) * N, hipMemcpyHostToDevice, e->stream));
			HIP_TRY(hipMemsetAsync(e->d_placeg_zero, 0, N, e->stream));
			const size_t total = (size_t)N * C * PLACE_GEN_STATES * PLACE_GEN_STATES;
			hipLaunchKernelGGL(k_transition_matrices, dim3((unsigned)std::min<size_t>((total + 255) / 256, 4096)), dim3(256), 0, e->stream, PLACE_GEN_STATES, C, N, e->d_model.get(),
			                   e->d_rates.get(), e->d_placeg_len.get(), e->d_placeg_zero.get(), -1, e->d_placeg_mats.get(), e->d_placeg_dmats.get());
			build_matrix_images(e, N * C, e->d_placeg_mats, e->d_placeg_imgs);
		}
		const ClassSprWalkArgs walk{e->d_sprg_ops.get(), e->d_sprg_nops.get(), (int)stride, P, e->Pp, C, e->d_tipmask, e->d_tipsets, e->d_imgs};
		hipLaunchKernelGGL(k_classspr_walk, dim3((unsigned)nblk, (unsigned)rows), dim3(GenGeo<2>::WAVES * 64), 0, e->stream, walk);
		if ((rc = body(SprGenChunk{first, rows, slots, stride, nblk, &cands, &cand_of}))) return rc;
		first += rows;
	}
	return PHYAMD_OK;
}

// lnl [count][N] (host): every row walked from the resident lowers into its own planes, every candidate of the chunk in one launch.
// Writes only the batch scratch beyond the evaluation that made the partials resident
int run_spr_general(Shard *e, int flags, int32_t count, const int32_t *prune, double *lnl, phyamd_spr_profile &prof) {
	static const GeneralQueryCall call{"phyamd_spr_log_likelihoods_general", "the kernels are", "phyamd_spr_log_likelihoods", "64-wide products are",
	                                   "which have no half-length counterpart", "the half-length matrices are", "kernels do"};
	int rc;
	std::vector<int32_t> live;
	if ((rc = check_spr_general_call(e, call, flags, count, prune, live))) return rc;
	const int N = e->N, C = e->C, P = e->P;
	std::fill(lnl, lnl + (size_t)count * N, NAN);
	prof.prunes = count;
	if (live.empty()) return PHYAMD_OK;
	std::vector<double> out;
	return for_spr_gen_row_chunks(
	    e, call.name, "the pruned tree's upper of every internal node and the path messages", live, prune, true,
	    [e](size_t slots, size_t nblk) { return spr_gen_plan(e, slots, nblk); },
	    [&](const SprGenChunk &k) -> int {
		    const std::vector<ClassSprCand> &cands = *k.cands;
		    const int nblk = k.nblk;
		    for (size_t c0 = 0; c0 < cands.size(); c0 += BATCH_MAX_CHUNK) {  // (gridDim.y)
			    const size_t n = std::min<size_t>(cands.size() - c0, BATCH_MAX_CHUNK);
			    const ClassSprArgs a{e->d_sprg_cands.get() + c0, P, e->Pp, C, e->d_tipmask, e->d_tipsets, e->d_freqs, e->d_props, e->d_weights, e->d_imgs, e->d_placeg_imgs,
			                         e->d_spr_slab.get() + c0 * nblk};
			    hipLaunchKernelGGL(k_classspr, dim3((unsigned)nblk, (unsigned)n), dim3(GenGeo<2>::WAVES * 64), 0, e->stream, a);
		    }
		    const size_t cells = k.rows * N;
		    hipLaunchKernelGGL(k_spr_finish, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, e->stream, cells, nblk, e->d_spr_cand_of.get(), e->d_spr_slab.get(),
		                       e->d_spr_out.get());
		    HIP_TRY(hipGetLastError());
		    out.resize(cells);
		    HIP_TRY(hipMemcpyAsync(out.data(), e->d_spr_out, sizeof(double) * cells, hipMemcpyDeviceToHost, e->stream));
		    HIP_TRY(hipStreamSynchronize(e->stream));  // (also covers the lists, which the next chunk builds anew)
		    for (size_t r = 0; r < k.rows; r++) std::copy(out.begin() + r * N, out.begin() + (r + 1) * N, lnl + (size_t)live[k.first + r] * N);
		    prof.chunks++;
		    prof.candidates += (int64_t)cands.size();
		    return PHYAMD_OK;
	    });
}

int shard_spr_general(Shard *e, int flags, int32_t count, const int32_t *prune, double *lnl) {
	CHECK_ENGINE(e);
	return profiled_call(e, &Shard::spr_prof, phyamd_spr_profile{}, [&](phyamd_spr_profile &prof) { return run_spr_general(e, flags, count, prune, lnl, prof); });
}

// ---- the three graft branches of every SPR regraft, optimised (phyamd_spr_optimize) ----------------------------------------------

// the SPR row's, and per row for its (at most N) candidates: pi o U, the visited branch's coefficients, the results and status
// words, and the cells they are scattered into
ScratchPlan tripod_plan(Shard *e) {
	const size_t D = sizeof(double), N = (size_t)e->N, C = (size_t)e->C, nblk = ((size_t)e->P + WAVE - 1) / WAVE, plane = nblk * WAVE * 4;
	ScratchPlan p = spr_plan(e);
	p.add(e->d_tripod_fU, D * N * C * plane);
	p.add(e->d_tripod_K, D * N * C * plane);
	p.add(e->d_tripod_res, D * N * 5);
	p.add(e->d_tripod_status, sizeof(int32_t) * N * TRIPOD_STATUS);
	p.add(e->d_tripod_out, D * N * 5);
	p.add(e->d_tripod_counts, sizeof(int32_t) * N * 3);
	return p;
}

struct SprOptimizeArgs {
	int32_t count;
	const int32_t *prune;
	double lower, upper, tolerance;
	int32_t max_iterations;
	double lnl_tolerance;
	int32_t max_passes;
	double *lengths, *lnl, *initial_lnl;
	int32_t *passes;
};

// lengths [count][N][3], lnl, initial_lnl, passes [count][N] (host): the SPR call's rows and walk, then per chunk of rows pi o U of
// every candidate and one workgroup per candidate that runs its whole rule.  Reads the engine's inputs and writes only the batch
// scratch: nothing in Shard::state changes but the record that the host lists are the tree's
int run_spr_optimize(Shard *e, int flags, const SprOptimizeArgs &o, phyamd_spr_optimize_profile &prof) {
	static const char *const name = "phyamd_spr_optimize";
	int rc;
	std::vector<int32_t> live;
	if ((rc = check_ready(e))) return fail(rc, "%s: the engine is not ready: %s", name, std::string(g_last_error).c_str());
	if ((rc = check_spr_call(e, name, "the likelihood in a branch length is formed from it", flags, o.count, o.prune, live))) return rc;
	const int T = e->T, N = e->N, C = e->C, nblk = (e->P + WAVE - 1) / WAVE;
	const size_t all = (size_t)o.count * N;
	std::fill(o.lengths, o.lengths + all * 3, NAN);
	std::fill(o.lnl, o.lnl + all, NAN);
	if (o.initial_lnl) std::fill(o.initial_lnl, o.initial_lnl + all, NAN);
	if (o.passes) std::fill(o.passes, o.passes + all, 0);
	prof.prunes = o.count;
	if (live.empty()) return PHYAMD_OK;
	std::vector<double> out;
	std::vector<int32_t> counts;
	return for_spr_row_chunks(e, name, "every internal node's lower and upper partial, and two planes per candidate", tripod_plan(e), live, o.prune, false,
	                          [&](size_t first, size_t rows, const std::vector<SprCand> &cands, const double *mats) -> int {
		const size_t plane = (size_t)nblk * WAVE * 4;
		for (size_t c0 = 0; c0 < cands.size(); c0 += BATCH_MAX_CHUNK) {  // (gridDim.y)
			const size_t n = std::min<size_t>(cands.size() - c0, BATCH_MAX_CHUNK);
			const TripodUpperArgs a{e->d_spr_cands.get() + c0, T, N, e->P, C, nblk, e->d_tipmask, e->d_freqs, mats, e->d_batch_lower, e->d_batch_upper,
			                        e->d_tripod_fU.get() + c0 * C * plane};
			hipLaunchKernelGGL(k_tripod_upper4, dim3(nblk, (unsigned)n), dim3(WAVE, C), 0, e->stream, a);
		}
		TripodSolveArgs s{};
		s.cands = e->d_spr_cands, s.T = T, s.P = e->P, s.C = C, s.nblk = nblk, s.max_iterations = o.max_iterations, s.max_passes = o.max_passes;
		s.lower = o.lower, s.upper = o.upper, s.tolerance = o.tolerance, s.lnl_tolerance = o.lnl_tolerance;
		s.tipmask = e->d_tipmask, s.props = e->d_props, s.model = e->d_model, s.rates = e->d_rates, s.weights = e->d_weights;
		s.lengths = e->d_spr_len, s.row_lower = e->d_batch_lower, s.fU = e->d_tripod_fU, s.K = e->d_tripod_K, s.out = e->d_tripod_res, s.status = e->d_tripod_status;
		if (!cands.empty()) hipLaunchKernelGGL(k_tripod_solve4, dim3((unsigned)cands.size()), dim3(CBOPT_THREADS), 0, e->stream, s);
		const size_t cells = rows * N;
		hipLaunchKernelGGL(k_tripod_finish, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, e->stream, cells, e->d_spr_cand_of.get(), e->d_tripod_res.get(),
		                   e->d_tripod_status.get(), e->d_tripod_out.get(), e->d_tripod_counts.get());
		HIP_TRY(hipGetLastError());
		out.resize(cells * 5);
		counts.resize(cells * 3);
		HIP_TRY(hipMemcpyAsync(out.data(), e->d_tripod_out, sizeof(double) * out.size(), hipMemcpyDeviceToHost, e->stream));
		HIP_TRY(hipMemcpyAsync(counts.data(), e->d_tripod_counts, sizeof(int32_t) * counts.size(), hipMemcpyDeviceToHost, e->stream));
		HIP_TRY(hipStreamSynchronize(e->stream));  // (also covers the lists, which the next chunk builds anew)
		for (size_t r = 0; r < rows; r++)
			for (size_t w = 0; w < (size_t)N; w++) {
				const size_t from = r * N + w, to = (size_t)live[first + r] * N + w;
				const double *v = &out[from * 5];
				std::copy(v, v + 3, o.lengths + to * 3);
				o.lnl[to] = v[3];
				if (o.initial_lnl) o.initial_lnl[to] = v[4];
				if (o.passes) o.passes[to] = counts[from * 3];
				prof.visits += counts[from * 3 + 1];
				prof.iterations += counts[from * 3 + 2];
			}
		prof.chunks++;
		prof.candidates += (int64_t)cands.size();
		return PHYAMD_OK;
	});
}

int shard_spr_optimize(Shard *e, int flags, const SprOptimizeArgs &o) {
	CHECK_ENGINE(e);
	return profiled_call(e, &Shard::tripod_prof, phyamd_spr_optimize_profile{}, [&](phyamd_spr_optimize_profile &prof) { return run_spr_optimize(e, flags, o, prof); });
}

// ---- the three graft branches of every SPR regraft of a 20-state engine's tree, optimised (phyamd_spr_optimize_general) --------------

// (phyamd_place_calls.inc, behind this file: what k_classplace_own forms a node's own partial from, and its launch)
int place_own_of(Shard *e, const char *name, int node, double *out, PlaceGenOwn *own);

// an item is a ROW: the scoring call's planes, ops, candidates and index by cell (spr_gen_plan's, without the slab, the result and
// the half lengths); `slots` own partials of the path nodes above u and their records; and per candidate (at most N): its record,
// its start, pi o U and the coefficients of the branch being visited -- a node's partial each --, the result and the status words;
// per cell the scattered results and counts.  Whatever the row count: every internal node's own partial and its record.
//   bytes = rows * [8 npd (T - 1 + 2 slots + 2 N) + lists] + 8 npd (T - 1) + records,   npd = C * 20 * Pp
ScratchPlan classgraft_plan(Shard *e, size_t slots) {
	const size_t D = sizeof(double), N = (size_t)e->N, internal = (size_t)(e->T - 1), ops = internal + slots, npd = node_partial_doubles(e);
	ScratchPlan p;
	p.add(e->d_sprg_work, D * ops * npd);
	p.add(e->d_sprg_ops, sizeof(ClassSprOp) * ops);
	p.add(e->d_sprg_nops, sizeof(int32_t));
	p.add(e->d_sprg_cands, sizeof(ClassSprCand) * N);
	p.add(e->d_spr_cand_of, sizeof(int32_t) * N);
	p.add(e->d_graft_own, D * slots * npd, D * internal * npd);
	p.add(e->d_placeg_owns, sizeof(PlaceGenOwn) * slots, sizeof(PlaceGenOwn) * internal);
	p.add(e->d_graft_cands, sizeof(ClassGraftCand) * N);
	p.add(e->d_qopt_start, D * N * 3);
	p.add(e->d_graft_F, D * N * npd);
	p.add(e->d_graft_K, D * N * npd);
	p.add(e->d_tripod_res, D * N * 5);
	p.add(e->d_tripod_status, sizeof(int32_t) * N * TRIPOD_STATUS);
	p.add(e->d_tripod_out, D * N * 5);
	p.add(e->d_tripod_counts, sizeof(int32_t) * N * 3);
	return p;
}

// lengths [count][N][3], lnl, initial_lnl, passes [count][N] (host): the 20-state scoring call's rows and walk, then per chunk of rows
// the own partials, pi o U of every candidate and one workgroup per candidate that runs its whole rule.  Writes only the batch
// scratch beyond the evaluation that made the partials resident
int run_spr_optimize_general(Shard *e, int flags, const SprOptimizeArgs &o, phyamd_spr_optimize_profile &prof) {
	static const GeneralQueryCall call{"phyamd_spr_optimize_general", "the kernels are", "phyamd_spr_optimize", "64-wide products are",
	                                   "which the solve cannot form at another length", "the likelihood in a branch length is", "solve does"};
	int rc;
	std::vector<int32_t> live;
	if ((rc = check_spr_general_call(e, call, flags, o.count, o.prune, live))) return rc;
	const int T = e->T, N = e->N, C = e->C, P = e->P, root = e->root, nops = T - 1;
	const size_t all = (size_t)o.count * N, npd = node_partial_doubles(e);
	std::fill(o.lengths, o.lengths + all * 3, NAN);
	std::fill(o.lnl, o.lnl + all, NAN);
	if (o.initial_lnl) std::fill(o.initial_lnl, o.initial_lnl + all, NAN);
	if (o.passes) std::fill(o.passes, o.passes + all, 0);
	prof.prunes = o.count;
	if (live.empty()) return PHYAMD_OK;
	std::vector<PlaceGenOwn> owns;
	std::vector<ClassGraftCand> cands;
	std::vector<double> start, out;
	std::vector<int32_t> counts;
	std::vector<const double *> own_on_path(N, nullptr);
	return for_spr_gen_row_chunks(
	    e, call.name, "the pruned tree's upper of every internal node, the path messages and own partials, and two planes per candidate", live, o.prune, false,
	    [e](size_t slots, size_t) { return classgraft_plan(e, slots); },
	    [&](const SprGenChunk &k) -> int {
		    const std::vector<ClassSprCand> &scands = *k.cands;
		    double *const own_all = e->d_graft_own.get(), *const own_rows = own_all + (size_t)nops * npd;
		    const auto own_of = [&](int n) { return n < T ? (const double *)nullptr : own_all + (size_t)(n - T) * npd; };
		    owns.clear(), cands.clear(), start.clear();
		    for (int n = T; n < N; n++) {  // every internal node's own partial in the engine's tree (the root's is not read)
			    if (n == root) continue;
			    PlaceGenOwn own;
			    if (int rc = place_own_of(e, call.name, n, own_all + (size_t)(n - T) * npd, &own)) return rc;
			    owns.push_back(own);
		    }
		    for (size_t r = 0; r < k.rows; r++) {
			    const int32_t i = live[k.first + r];
			    const int p = o.prune ? o.prune[i] : i, u = e->sched.parent[p];
			    // the path nodes above u: their own partial is the path message of the child below them times the other child's message
			    const double *work = e->d_sprg_work.get() + r * k.stride * npd;
			    std::vector<int> on_path;
			    size_t slot = 0;
			    for (int child = u, n = e->sched.parent[u]; n != root; child = n, n = e->sched.parent[n], slot++) {
				    double *dst = own_rows + (r * k.slots + slot) * npd;
				    PlaceGenOwn own;
				    if (int rc = place_own_of(e, call.name, n, dst, &own)) return rc;
				    const double *msg = work + ((size_t)nops + slot) * npd;  // build_spr_gen_row: the message of the path's slot-th node
				    if (e->left[n] == child) own.src_l = msg, own.row_l = nullptr;
				    else own.src_r = msg, own.row_r = nullptr;
				    owns.push_back(own);
				    own_on_path[n] = dst;
				    on_path.push_back(n);
			    }
			    for (int w = 0; w < N; w++) {
				    const int32_t ci = (*k.cand_of)[r * N + w];
				    if (ci < 0) continue;
				    if ((size_t)ci != cands.size() || scands[ci].w != w || scands[ci].p != p) return fail(PHYAMD_EDEVICE, "%s: the candidate lists are out of order", call.name);
				    cands.push_back(ClassGraftCand{own_of(p), own_on_path[w] ? own_on_path[w] : own_of(w), p, w, e->left[u] == p ? 1 : 0, 0});
				    start.push_back(e->lengths[p]);
				    start.push_back(0.5 * e->lengths[w]);
				    start.push_back(0.5 * e->lengths[w]);
			    }
			    for (const int n : on_path) own_on_path[n] = nullptr;
		    }
		    if (!owns.empty()) {
			    HIP_TRY(hipMemcpyAsync(e->d_placeg_owns, owns.data(), sizeof(PlaceGenOwn) * owns.size(), hipMemcpyHostToDevice, e->stream));
			    hipLaunchKernelGGL(k_classplace_own, dim3((unsigned)((P + 255) / 256), (unsigned)owns.size(), (unsigned)C), dim3(256), 0, e->stream, e->d_placeg_owns.get(), P, e->Pp,
			                       e->d_tipsets.get());
		    }
		    HIP_TRY(hipMemcpyAsync(e->d_graft_cands, cands.data(), sizeof(ClassGraftCand) * cands.size(), hipMemcpyHostToDevice, e->stream));
		    HIP_TRY(hipMemcpyAsync(e->d_qopt_start, start.data(), sizeof(double) * start.size(), hipMemcpyHostToDevice, e->stream));
		    for (size_t c0 = 0; c0 < cands.size(); c0 += BATCH_MAX_CHUNK) {  // (gridDim.y)
			    const size_t n = std::min<size_t>(cands.size() - c0, BATCH_MAX_CHUNK);
			    const ClassGraftUpperArgs a{e->d_sprg_cands.get() + c0, P, e->Pp, C, e->d_tipmask, e->d_tipsets, e->d_freqs, e->d_imgs, e->d_graft_F.get() + c0 * npd};
			    hipLaunchKernelGGL(k_classgraft_upper, dim3((unsigned)k.nblk, (unsigned)n), dim3(GenGeo<2>::WAVES * 64), 0, e->stream, a);
		    }
		    ClassGraftArgs s{};
		    s.cands = e->d_graft_cands, s.P = P, s.Pp = e->Pp, s.C = C, s.max_iterations = o.max_iterations, s.max_passes = o.max_passes;
		    s.lower = o.lower, s.upper = o.upper, s.tolerance = o.tolerance, s.lnl_tolerance = o.lnl_tolerance;
		    s.tipcode = e->d_tipmask, s.tipsets = e->d_tipsets, s.props = e->d_props, s.model = e->d_model, s.rates = e->d_rates, s.weights = e->d_weights;
		    s.start = e->d_qopt_start, s.F = e->d_graft_F, s.K = e->d_graft_K, s.out = e->d_tripod_res, s.status = e->d_tripod_status;
		    if (!cands.empty()) hipLaunchKernelGGL(k_classgraft_solve, dim3((unsigned)cands.size()), dim3(CLASSOPT_THREADS), 0, e->stream, s);
		    const size_t cells = k.rows * N;
		    hipLaunchKernelGGL(k_tripod_finish, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, e->stream, cells, e->d_spr_cand_of.get(), e->d_tripod_res.get(),
		                       e->d_tripod_status.get(), e->d_tripod_out.get(), e->d_tripod_counts.get());
		    HIP_TRY(hipGetLastError());
		    out.resize(cells * 5);
		    counts.resize(cells * 3);
		    HIP_TRY(hipMemcpyAsync(out.data(), e->d_tripod_out, sizeof(double) * out.size(), hipMemcpyDeviceToHost, e->stream));
		    HIP_TRY(hipMemcpyAsync(counts.data(), e->d_tripod_counts, sizeof(int32_t) * counts.size(), hipMemcpyDeviceToHost, e->stream));
		    HIP_TRY(hipStreamSynchronize(e->stream));  // (also covers the lists, which the next chunk builds anew)
		    for (size_t r = 0; r < k.rows; r++)
			    for (size_t w = 0; w < (size_t)N; w++) {
				    const size_t from = r * N + w, to = (size_t)live[k.first + r] * N + w;
				    const double *v = &out[from * 5];
				    std::copy(v, v + 3, o.lengths + to * 3);
				    o.lnl[to] = v[3];
				    if (o.initial_lnl) o.initial_lnl[to] = v[4];
				    if (o.passes) o.passes[to] = counts[from * 3];
				    prof.visits += counts[from * 3 + 1];
				    prof.iterations += counts[from * 3 + 2];
			    }
		    prof.chunks++;
		    prof.candidates += (int64_t)cands.size();
		    return PHYAMD_OK;
	    });
}

int shard_spr_optimize_general(Shard *e, int flags, const SprOptimizeArgs &o) {
	CHECK_ENGINE(e);
	return profiled_call(e, &Shard::tripod_prof, phyamd_spr_optimize_profile{}, [&](phyamd_spr_optimize_profile &prof) { return run_spr_optimize_general(e, flags, o, prof); });
}

// ---- the ML distance of pairs of taxa (phyamd_pairwise_distances) ---------------------------------------------------------------

// an item is a PAIR: its two taxa and its group record, its table's segment sums and the table (`bins` doubles each: 256 mask pairs at
// 4 states, 1024 class pairs at 20), its start and its results.  Nothing whatever the pair count: the call walks no tree and reads
// the engine's tip data, weights and model where they are
ScratchPlan pairdist_plan(Shard *e, size_t segments, size_t bins = 256) {
	const size_t D = sizeof(double);
	ScratchPlan p;
	p.add(e->d_pairdist_pairs, sizeof(int32_t) * 2);
	p.add(e->d_pairdist_groups, sizeof(int32_t) * 2);
	p.add(e->d_pairdist_part, D * segments * bins);
	p.add(e->d_pairdist_counts, D * bins);
	p.add(e->d_pairdist_start, D);
	p.add(e->d_pairdist_out, D * 4);
	p.add(e->d_pairdist_iter, sizeof(int32_t));
	return p;
}

constexpr size_t PAIRDIST_MAX_CHUNK = (size_t)1 << 20;  // pairs per chunk: gridDim.x of k_pairdist_solve4, 2 GB of tables
constexpr size_t PAIRDIST_GEN_MAX_CHUNK = (size_t)1 << 18;  // the same 2 GB of the larger tables (k_pairdist_finish runs four blocks per pair)

struct PairDistanceArgs {
	int32_t count;
	const int32_t *pairs;  // [count][2], validated (phyamd_pairwise_distances); null: all i < j, row-major
	const double *start;
	double lower, upper, tolerance;
	int32_t max_iterations;
	double *distances, *lnl, *d1, *d2;
	int32_t *iterations;
	double *counts;
	uint64_t *class_members;  // phyamd_pairwise_distances_general only
};

// what the two distance calls differ in, beside their kernels: the table's bins, the partners of a wave of the counting kernel and
// the pairs of a chunk
struct PairDistanceKind {
	size_t bins, partners, max_chunk;
};

// the checks the two distance calls share, after the state count's
int check_pairwise_distances(Shard *e, const char *name, int flags, bool solve) {
	if (e->tiles > 1) return fail(PHYAMD_EUNSUPPORTED, "%s: the patterns are tiled and the call needs the tip data of all patterns resident", name);
	if (flags != 0) return fail(PHYAMD_EUNSUPPORTED, "%s: flags %d (no flags are defined: pass 0)", name, flags);
	for (int t = 0; t < e->T; t++)
		if (!e->tip_set[t]) return fail(PHYAMD_EINVAL, "%s: tip %d has no data (phyamd_set_tip_states / phyamd_set_tip_partials)", name, t);
	if (std::any_of(e->tip_empty.begin(), e->tip_empty.end(), [](uint8_t x) { return x != 0; })) return fail(PHYAMD_EUNSUPPORTED, "%s: a tip cell has an empty state mask", name);
	if (!e->have_weights) return fail(PHYAMD_EINVAL, "%s: phyamd_set_pattern_weights has not been called", name);
	if (solve && !e->have_eigen) return fail(PHYAMD_EINVAL, "%s needs the eigen system (phyamd_set_eigen): the likelihood in the distance is formed from it", name);
	if (solve && !e->have_freqs) return fail(PHYAMD_EINVAL, "%s: phyamd_set_frequencies has not been called", name);
	if (solve && !e->have_rates) return fail(PHYAMD_EINVAL, "%s: phyamd_set_category_rates has not been called", name);
	return PHYAMD_OK;
}

// chunk by chunk the pairs' tables on the matrix pipe and, with `distances`, each pair's whole iteration in one workgroup.  Reads
// the engine's tip data, weights and model and writes only the batch scratch: nothing in Shard::state changes.  launch_count(args,
// grid) and launch_solve(args, pairs) launch the call's counting kernel and its iterations
template <class LaunchCount, class LaunchSolve>
int run_pairdist_chunks(Shard *e, const char *name, const PairDistanceArgs &o, phyamd_distance_profile &prof, const PairDistanceKind &kind, const LaunchCount &launch_count,
                        const LaunchSolve &launch_solve) {
	const bool solve = o.distances != nullptr;
	const int T = e->T, P = e->P;
	const size_t count = (size_t)o.count, segments = ((size_t)P + REWEIGHT_SEGMENT - 1) / REWEIGHT_SEGMENT, bins = kind.bins;
	if (segments > 65535) return fail(PHYAMD_EUNSUPPORTED, "%s: %zu segments of %d patterns (at most 65535: gridDim.y)", name, segments, REWEIGHT_SEGMENT);
	prof.pairs = o.count;
	prof.segments = (int32_t)segments;
	std::vector<int32_t> all;
	const int32_t *pairs = o.pairs;
	if (!pairs) {
		all.reserve(count * 2);
		for (int i = 0; i < T; i++)
			for (int j = i + 1; j < T; j++) all.push_back(i), all.push_back(j);
		pairs = all.data();
	}
	const ScratchPlan plan = pairdist_plan(e, segments, bins);
	const size_t want = std::min(count, kind.max_chunk);
	size_t chunk = want;
	if (!plan.held(want)) {
		const double fit = plan.items_in(scratch_room(e, (double)batch_scratch_bytes(e), EngineRoom::MayGrow));
		if (fit < 1.0)
			return fail(PHYAMD_EUNSUPPORTED, "%s: the scratch of one pair (%zu bytes: its table's %zu segment sums, the table and its results) does not fit the memory budget", name,
			            plan.item_bytes(), segments);
		chunk = (size_t)std::min((double)want, fit);
		if (!plan.held(chunk))
			if (int rc = allocate_batch_scratch(e, chunk, plan)) return rc;
	}
	std::vector<int32_t> groups, iter;
	std::vector<double> start, out;
	for (size_t first = 0; first < count; first += chunk) {
		const size_t n = std::min(chunk, count - first);
		const int32_t *pc = pairs + 2 * first;
		groups.clear();  // runs of pairs that share their first taxon, at most kind.partners long
		for (size_t i = 0; i < n;) {
			size_t len = 1;
			while (len < kind.partners && i + len < n && pc[2 * (i + len)] == pc[2 * i]) len++;
			groups.push_back((int32_t)i), groups.push_back((int32_t)len);
			i += len;
		}
		HIP_TRY(hipMemcpyAsync(e->d_pairdist_pairs, pc, sizeof(int32_t) * 2 * n, hipMemcpyHostToDevice, e->stream));
		HIP_TRY(hipMemcpyAsync(e->d_pairdist_groups, groups.data(), sizeof(int32_t) * groups.size(), hipMemcpyHostToDevice, e->stream));
		const PairCountArgs ca{e->d_pairdist_pairs, e->d_pairdist_groups, e->d_tipmask, e->d_weights, e->d_pairdist_part, e->d_pairdist_counts, P, (int)n, (int)segments};
		launch_count(ca, dim3((unsigned)(groups.size() / 2), (unsigned)segments));
		PairCountArgs fa = ca;  // k_pairdist_finish adds records of 256 bins: a table of `bins` is bins / 256 of them
		fa.npairs = (int)(n * (bins / 256));
		hipLaunchKernelGGL(k_pairdist_finish, dim3((unsigned)fa.npairs), dim3(256), 0, e->stream, fa);
		if (solve) {
			start.assign(n, 0.1);
			if (o.start) std::copy(o.start + first, o.start + first + n, start.begin());
			HIP_TRY(hipMemcpyAsync(e->d_pairdist_start, start.data(), sizeof(double) * n, hipMemcpyHostToDevice, e->stream));
			const PairSolveArgs sa{e->d_pairdist_counts, e->d_pairdist_start, e->C, o.max_iterations, o.lower, o.upper, o.tolerance, e->d_model, e->d_freqs, e->d_rates, e->d_props,
			                       e->d_pairdist_out, e->d_pairdist_iter};
			launch_solve(sa, (unsigned)n);
			out.resize(n * 4);
			iter.resize(n);
			HIP_TRY(hipMemcpyAsync(out.data(), e->d_pairdist_out, sizeof(double) * out.size(), hipMemcpyDeviceToHost, e->stream));
			HIP_TRY(hipMemcpyAsync(iter.data(), e->d_pairdist_iter, sizeof(int32_t) * n, hipMemcpyDeviceToHost, e->stream));
		}
		HIP_TRY(hipGetLastError());
		if (o.counts) HIP_TRY(hipMemcpyAsync(o.counts + first * bins, e->d_pairdist_counts, sizeof(double) * n * bins, hipMemcpyDeviceToHost, e->stream));
		HIP_TRY(hipStreamSynchronize(e->stream));  // (also covers the chunk's lists and starts)
		prof.chunks++;
		for (size_t i = 0; i < n && solve; i++) {
			const double *r = &out[i * 4];
			o.distances[first + i] = r[0];
			if (o.lnl) o.lnl[first + i] = r[1];
			if (o.d1) o.d1[first + i] = r[2];
			if (o.d2) o.d2[first + i] = r[3];
			if (o.iterations) o.iterations[first + i] = iter[i];
			prof.iterations += std::abs(iter[i]);
		}
	}
	return PHYAMD_OK;
}

int run_pairwise_distances(Shard *e, int flags, const PairDistanceArgs &o, phyamd_distance_profile &prof) {
	static const char *const name = "phyamd_pairwise_distances";
	if (e->S != 4) return fail(PHYAMD_EUNSUPPORTED, "%s: the mask-pair tables are built for 4 states (the engine has %d)", name, e->S);
	if (int rc = check_pairwise_distances(e, name, flags, o.distances != nullptr)) return rc;
	return run_pairdist_chunks(
	    e, name, o, prof, PairDistanceKind{256, (size_t)PAIRDIST_PARTNERS, PAIRDIST_MAX_CHUNK},
	    [e](const PairCountArgs &ca, dim3 grid) { hipLaunchKernelGGL(k_pairdist_counts4, grid, dim3(WAVE), 0, e->stream, ca); },
	    [e](const PairSolveArgs &sa, unsigned n) { hipLaunchKernelGGL(k_pairdist_solve4, dim3(n), dim3(PAIRDIST_THREADS), 0, e->stream, sa); });
}

// the 20-state call: the classes are the codes of d_tipmask (phyamd_pairdist_gen.inc), so the sets the engine has recorded must leave
// every code below 32; class_members is the host's copy of what the kernel builds its class tables from
int run_pairwise_distances_general(Shard *e, int flags, const PairDistanceArgs &o, phyamd_distance_profile &prof) {
	static const char *const name = "phyamd_pairwise_distances_general";
	if (e->S == 4) return fail(PHYAMD_EUNSUPPORTED, "%s: the class-pair tables are built for 20 states (the engine has 4: use phyamd_pairwise_distances)", name);
	if (e->S != PAIRDIST_GEN_STATES)
		return fail(PHYAMD_EUNSUPPORTED, "%s: the class-pair tables are built for 20 states (the engine has %d: 64 x 64 tables are not built)", name, e->S);
	constexpr size_t max_sets = PAIRDIST_GEN_CLASSES - PAIRDIST_GEN_STATES - 1;
	const size_t sets = e->tipsets_host.size();
	if (sets > max_sets)
		return fail(PHYAMD_EUNSUPPORTED, "%s: the engine has recorded %zu ambiguity sets (at most %zu: a tip cell's class must be below %d)", name, sets, max_sets, PAIRDIST_GEN_CLASSES);
	for (size_t q = 0; q < sets; q++)
		if (e->tipsets_host[q] == 0) return fail(PHYAMD_EUNSUPPORTED, "%s: ambiguity set %zu has no member (a tip cell's partials are all 0)", name, q);
	if (int rc = check_pairwise_distances(e, name, flags, o.distances != nullptr)) return rc;
	const int rc = run_pairdist_chunks(
	    e, name, o, prof, PairDistanceKind{(size_t)PAIRDIST_GEN_BINS, (size_t)PAIRDIST_GEN_PARTNERS, PAIRDIST_GEN_MAX_CHUNK},
	    [e](const PairCountArgs &ca, dim3 grid) { hipLaunchKernelGGL(k_classpair_counts, grid, dim3(WAVE), 0, e->stream, ca); },
	    [e, sets](const PairSolveArgs &sa, unsigned n) {
		    const PairSolveGenArgs ga{sa, e->d_tipsets, (int)sets};
		    hipLaunchKernelGGL(k_classpair_solve, dim3(n), dim3(PAIRDIST_THREADS), 0, e->stream, ga);
	    });
	if (rc) return rc;
	if (o.class_members)
		for (size_t c = 0; c < (size_t)PAIRDIST_GEN_CLASSES; c++)
			o.class_members[c] = c < 20 ? (uint64_t)1 << c : c == 20 ? ((uint64_t)1 << 20) - 1 : c - 21 < sets ? (uint64_t)e->tipsets_host[c - 21] : 0;
	return PHYAMD_OK;
}

int shard_pairwise_distances(Shard *e, int flags, const PairDistanceArgs &o) {
	CHECK_ENGINE(e);
	return profiled_call(e, &Shard::dist_prof, phyamd_distance_profile{}, [&](phyamd_distance_profile &prof) { return run_pairwise_distances(e, flags, o, prof); });
}

int shard_pairwise_distances_general(Shard *e, int flags, const PairDistanceArgs &o) {
	CHECK_ENGINE(e);
	return profiled_call(e, &Shard::dist_prof, phyamd_distance_profile{}, [&](phyamd_distance_profile &prof) { return run_pairwise_distances_general(e, flags, o, prof); });
}

// ---- per-pattern posteriors (phyamd_state_posteriors, phyamd_site_rate_posteriors) ---------------------------------------------

// The staging arrays of the two calls, and rows of a chunk that fit beside the engine.  per_row[a]: bytes a row takes in array a
// for this call, 0: the call does not use the array -- it is released first, so that what an earlier call left never takes this
// call's room.  An array the call uses is kept where it is large enough (DeviceBuffer::reserve frees only an array it regrows),
// so the arrays are counted at the larger of what they hold and what n rows need: n is the most rows that fit the room beside a
// fully resident engine (scratch_room); if arrays kept from a roomier time leave no such n under a cap, they are released and the
// rows sized for empty ones.  At least one row: if even that does not fit, the allocation reports it
constexpr int POST_ARRAYS = 4;
size_t post_rows_that_fit(Shard *e, size_t count, const size_t (&per_row)[POST_ARRAYS]) {
	DeviceBuffer *const arrays[POST_ARRAYS] = {&e->d_post_rows, &e->d_post_out, &e->d_post_lower, &e->d_post_states};
	size_t row_bytes = 0;
	double held = 0.0;
	for (int a = 0; a < POST_ARRAYS; a++) {
		if (per_row[a] == 0) arrays[a]->release();
		row_bytes += per_row[a];
		held += (double)arrays[a]->bytes();
	}
	const double room = scratch_room(e, held, EngineRoom::Resident);
	const size_t n = (size_t)std::min((double)std::min<size_t>(count, BATCH_MAX_CHUNK), std::max(std::floor(room / (double)row_bytes), 1.0));
	if (e->cfg.max_device_bytes <= 0) return n;
	double after = 0.0;  // what the arrays hold once n rows are ensured
	for (int a = 0; a < POST_ARRAYS; a++) after += (double)std::max(arrays[a]->bytes(), n * per_row[a]);
	if (after > room)
		for (DeviceBuffer *a : arrays) a->release();
	return n;
}

// posteriors: row i at posteriors + (i * pattern_stride) * S, this shard's P patterns of it; states: row i at states + i *
// pattern_stride (the group layer passes the handle's pattern count and pointers advanced to this shard's range).  lnl: the log
// likelihood of the evaluation the partials belong to (this shard's patterns)
int shard_state_posteriors(Shard *e, int flags, int32_t count, const int32_t *nodes, size_t pattern_stride, double *posteriors, uint8_t *states, double *lnl) {
	CHECK_ENGINE(e);
	NOT_TILED(e, "phyamd_state_posteriors (every partial resident)");
	if (flags != 0) return fail(PHYAMD_EINVAL, "phyamd_state_posteriors: flags %d (no flags are defined: pass 0)", flags);
	if (!posteriors && !states) return fail(PHYAMD_EINVAL, "phyamd_state_posteriors: posteriors and states are both null");
	if (count < 1) return fail(PHYAMD_EINVAL, "phyamd_state_posteriors: count must be >= 1 (got %d)", count);
	const int N = e->N, C = e->C, S = e->S, P = e->P;
	if (!nodes && count != N) return fail(PHYAMD_EINVAL, "phyamd_state_posteriors: nodes is null, so count must be the node count %d (got %d)", N, count);
	for (int32_t i = 0; nodes && i < count; i++)
		if (nodes[i] < 0 || nodes[i] >= N) return fail(PHYAMD_EINVAL, "phyamd_state_posteriors: nodes[%d] = %d is not a node id (0..%d)", i, nodes[i], N - 1);
	int rc;
	if ((rc = bind_device(e)) || (rc = check_ready(e))) return rc;
	if ((rc = require_resident_partials(e, "phyamd_state_posteriors"))) return rc;
	const size_t npd = node_partial_doubles(e);
	const size_t per_row[POST_ARRAYS] = {sizeof(PostRow), posteriors ? sizeof(double) * P * S : 0, e->generic ? sizeof(double) * npd : 0, states ? (size_t)P : 0};
	const int fold = e->upper_fold ? 1 : 0;
	std::vector<PostRow> rows;
	std::vector<double> host_post;
	std::vector<uint8_t> host_states;
	const bool direct = pattern_stride == (size_t)P;  // one shard: a chunk's rows are contiguous in the caller's arrays
	for (size_t first = 0; first < (size_t)count;) {
		const size_t n = post_rows_that_fit(e, (size_t)count - first, per_row);
		if ((rc = e->d_post_rows.ensure(n)) || (posteriors && (rc = e->d_post_out.ensure(n * P * S))) || (states && (rc = e->d_post_states.ensure(n * P))) ||
		    (e->generic && (rc = e->d_post_lower.ensure(n * npd))))
			return rc;
		rows.resize(n);
		for (size_t r = 0; r < n; r++) {
			const int node = nodes ? nodes[first + r] : (int)(first + r);
			PostRow &d = rows[r];
			d.node = node;
			d.mat = node == e->root ? -1 : node;
			d.tip = node < e->T ? e->d_tipmask + (size_t)node * P : nullptr;
			d.low = nullptr;
			d.up = nullptr;
			if (node != e->root) {
				if (e->sched.upper_slot[node] < 0) return fail(PHYAMD_EDEVICE, "phyamd_state_posteriors: node %d has no resident upper partial", node);
				d.up = e->d_upper + (size_t)e->sched.upper_slot[node] * npd;
			}
			if (node >= e->T) {
				if (e->sched.core_index[node] < 0) return fail(PHYAMD_EDEVICE, "phyamd_state_posteriors: node %d has no resident lower partial", node);
				d.low = e->d_lower + (size_t)e->sched.core_index[node] * npd;
				if (e->generic && node != e->root) {  // a stored array is the message P p: the node's own partial, into this row's temporary
					double *own = e->d_post_lower + r * npd;
					if ((rc = true_lower_gen(e, node, own, nullptr))) return rc;
					d.low = own;
				}
			}
		}
		HIP_TRY(hipMemcpyAsync(e->d_post_rows, rows.data(), sizeof(PostRow) * n, hipMemcpyHostToDevice, e->stream));
		double *post = posteriors ? e->d_post_out.get() : nullptr;
		uint8_t *st = states ? e->d_post_states.get() : nullptr;
		if (e->generic)
			hipLaunchKernelGGL(k_post_gen, dim3((P + 255) / 256, (unsigned)n), dim3(256), 0, e->stream, e->d_post_rows.get(), P, e->Pp, S, C, e->d_mats.get(), e->d_freqs.get(), fold,
			                   e->d_props.get(), e->d_tipsets.get(), post, st);
		else
			hipLaunchKernelGGL(k_post4, dim3((P + WAVE - 1) / WAVE, (unsigned)n), dim3(WAVE, C), sizeof(double) * 4 * C * WAVE, e->stream, e->d_post_rows.get(), P, C,
			                   e->d_mats.get(), e->d_freqs.get(), fold, e->d_props.get(), post, st);
		HIP_TRY(hipGetLastError());
		if (posteriors) {
			double *dst = posteriors + first * pattern_stride * S;
			if (!direct) host_post.resize(n * P * S), dst = host_post.data();
			HIP_TRY(hipMemcpyAsync(dst, post, sizeof(double) * n * P * S, hipMemcpyDeviceToHost, e->stream));
		}
		if (states) {
			uint8_t *dst = states + first * pattern_stride;
			if (!direct) host_states.resize(n * P), dst = host_states.data();
			HIP_TRY(hipMemcpyAsync(dst, st, n * P, hipMemcpyDeviceToHost, e->stream));
		}
		HIP_TRY(hipStreamSynchronize(e->stream));  // (also covers `rows`, which the next chunk builds anew)
		for (size_t r = 0; !direct && r < n; r++) {
			if (posteriors) std::memcpy(posteriors + (first + r) * pattern_stride * S, host_post.data() + r * P * S, sizeof(double) * P * S);
			if (states) std::memcpy(states + (first + r) * pattern_stride, host_states.data() + r * P, (size_t)P);
		}
		first += n;
	}
	HIP_TRY(hipMemcpyAsync(e->h_result, e->d_result, sizeof(double), hipMemcpyDeviceToHost, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream));
	*lnl = e->h_result[0];
	return PHYAMD_OK;
}

// posteriors [P][C] and mean_rates [P] (or null) of this shard's patterns.  Reads the root's stored partial, like
// phyamd_root_frequency_term: whatever is pending is evaluated by a post-order pass, and the engine is afterwards what that pass
// leaves -- the root's array is p_root in every storage convention, only a rescaled evaluation's factors have to be the reference's
int shard_site_rate_posteriors(Shard *e, double *posteriors, double *mean_rates) {
	CHECK_ENGINE(e);
	NOT_TILED(e, "phyamd_site_rate_posteriors (the root partial of every pattern resident)");
	int rc;
	if ((rc = bind_device(e)) || (rc = check_ready(e))) return rc;
	if ((rc = run_lower(e, 1))) return rc;
	if (e->scaling_on && (rc = require_reference_form(e))) return rc;  // (see shard_root_frequency_term: factors common to the categories)
	if (e->sched.core_index[e->root] < 0 || !e->d_lower) return fail(PHYAMD_EDEVICE, "phyamd_site_rate_posteriors: the root partial is not resident");
	const int P = e->P, C = e->C;
	e->d_post_rows.release(), e->d_post_lower.release(), e->d_post_states.release();  // (what a state call left is not this call's: its room is)
	if ((rc = e->d_post_out.ensure((size_t)P * C + P))) return rc;
	const double *root = e->d_lower + (size_t)e->sched.core_index[e->root] * node_partial_doubles(e);
	const size_t cat_stride = e->generic ? (size_t)e->S * e->Pp : (size_t)P * e->S;
	const size_t pat_stride = e->generic ? 1 : (size_t)e->S, state_stride = e->generic ? (size_t)e->Pp : 1;
	double *R = e->d_post_out.get(), *mean = R + (size_t)P * C;
	hipLaunchKernelGGL(k_site_rate_post, dim3((P + 255) / 256), dim3(256), 0, e->stream, P, e->S, C, root, cat_stride, pat_stride, state_stride, e->d_freqs.get(),
	                   e->d_props.get(), e->d_rates.get(), R, mean);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(posteriors, R, sizeof(double) * P * C, hipMemcpyDeviceToHost, e->stream));
	if (mean_rates) HIP_TRY(hipMemcpyAsync(mean_rates, mean, sizeof(double) * P, hipMemcpyDeviceToHost, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream));
	return PHYAMD_OK;
}

// ---- the full branch-length Hessian (phyamd_branch_hessian) --------------------------------------------------------------------

// the lists of the engine's tree: every node's walk to the root (one tangent slot per step), and the work lists of the two tile
// kernels -- per internal node m the 16 x 16 tiles of (node below its left child) x (node below its right child), and the tiles
// of the upper triangle of (branch) x (branch)
struct BhessLists {
	std::vector<BhessStart> starts;
	std::vector<BhessStep> steps;
	std::vector<BhessTile> cousins, outer;
};

void build_bhess_lists(const Shard *e, BhessLists &L) {
	const int N = e->N, root = e->root;
	std::vector<std::vector<std::pair<int32_t, int32_t>>> below((size_t)2 * N);  // [2 m + side]: (node, slot of its tangent at m)
	std::vector<int32_t> branches;
	for (int a = 0; a < N; a++) {
		if (a == root) continue;
		branches.push_back(a);
		BhessStart s{a, (int32_t)L.steps.size(), 0, 0};
		for (int cur = a, m = e->sched.parent[a];; cur = m, m = e->sched.parent[m]) {
			const bool from_left = e->left[m] == cur;
			below[(size_t)2 * m + (from_left ? 0 : 1)].push_back({a, (int32_t)L.steps.size()});
			L.steps.push_back(BhessStep{m, from_left ? e->right[m] : e->left[m], a, 0});
			s.count++;
			if (m == root) break;
		}
		L.starts.push_back(s);
	}
	const auto fill = [](int32_t *rows, int32_t *nodes, const std::pair<int32_t, int32_t> *from, size_t n) {
		for (size_t i = 0; i < 16; i++) rows[i] = from[i < n ? i : 0].second, nodes[i] = i < n ? from[i].first : -1;
	};
	for (int m = e->T; m < N; m++) {
		const auto &l = below[(size_t)2 * m], &r = below[(size_t)2 * m + 1];
		for (size_t i = 0; i < l.size(); i += 16)
			for (size_t j = 0; j < r.size(); j += 16) {
				BhessTile t{};
				t.m = m;
				fill(t.row_a, t.node_a, l.data() + i, std::min<size_t>(16, l.size() - i));
				fill(t.row_b, t.node_b, r.data() + j, std::min<size_t>(16, r.size() - j));
				L.cousins.push_back(t);
			}
	}
	std::vector<std::pair<int32_t, int32_t>> rows;  // (node, its row of G)
	for (int32_t a : branches) rows.push_back({a, a});
	for (size_t i = 0; i < rows.size(); i += 16)
		for (size_t j = i; j < rows.size(); j += 16) {
			BhessTile t{};
			t.m = -1;
			fill(t.row_a, t.node_a, rows.data() + i, std::min<size_t>(16, rows.size() - i));
			fill(t.row_b, t.node_b, rows.data() + j, std::min<size_t>(16, rows.size() - j));
			L.outer.push_back(t);
		}
}

// the call's scratch (ScratchPlan): an item is one block of 64 patterns -- its tangents, its rows of w / L, 1 / L, G and the walk's
// slab, its tiles; whatever the chunk, the sums (the chunk's and the running matrix and gradient, r Q P and r^2 Q Q P) and the lists
ScratchPlan bhess_plan(Shard *e, size_t nsteps, size_t tiles, size_t list_bytes) {
	const size_t D = sizeof(double), N = (size_t)e->N, C = (size_t)e->C;
	ScratchPlan p;
	p.add(e->d_bhess_tan, D * nsteps * C * WAVE * 4);
	p.add(e->d_bhess_rows, D * (2 * WAVE + N * WAVE + nsteps + 2 * N));
	p.add(e->d_bhess_tiles, D * 256 * tiles);
	p.add(e->d_bhess_sums, 0, D * (2 * N * N + 2 * N + 2 * N * C * 16));
	p.add(e->d_bhess_lists, 0, list_bytes);
	return p;
}

// lnl, gradient [N] (or null) and hessian [N][N] of this shard's patterns (host)
int run_branch_hessian(Shard *e, double *lnl, double *gradient, double *hessian, phyamd_hessian_profile &prof) {
	static const char *const name = "phyamd_branch_hessian";
	const int N = e->N, C = e->C, P = e->P;
	int rc;
	if (e->generic) return fail(PHYAMD_EUNSUPPORTED, "%s: %d states (the tangent walk and the pair tiles are built for 4)", name, e->S);
	if (C > BHESS_MAX_CATEGORIES) return fail(PHYAMD_EUNSUPPORTED, "%s: %d categories (a workgroup holds the category waves of one block: at most %d)", name, C, BHESS_MAX_CATEGORIES);
	NOT_TILED(e, "phyamd_branch_hessian (every partial resident)");
	if ((rc = check_ready(e))) return rc;
	if (std::any_of(e->explicit_host.begin(), e->explicit_host.end(), [](uint8_t x) { return x != 0; }))
		return fail(PHYAMD_EUNSUPPORTED, "%s: a node has explicit matrices (Q P is the derivative of exp(Q t r) only)", name);
	if (!e->have_eigen || !e->have_Q) return fail(PHYAMD_EINVAL, "%s needs the eigen system (phyamd_set_eigen): the derivatives of the matrices are formed from it", name);
	static const char *const rescaling = "%s: the engine is rescaling (the terms multiply partials of different nodes, and a rescaled evaluation's partials do not share units)";
	if (e->scaling_on) return fail(PHYAMD_EUNSUPPORTED, rescaling, name);
	if ((rc = require_resident_partials(e, name))) return rc;
	if (e->scaling_on) return fail(PHYAMD_EUNSUPPORTED, rescaling, name);  // (PHYAMD_RESCALE_AUTO: that evaluation switched)

	BhessLists L;
	build_bhess_lists(e, L);
	std::vector<int32_t> lower_of(N), upper_of(N);
	for (int n = 0; n < N; n++) {
		lower_of[n] = n < e->T ? -1 : e->sched.core_index[n];
		upper_of[n] = n == e->root ? 0 : e->sched.upper_slot[n];
		if ((n >= e->T && lower_of[n] < 0) || upper_of[n] < 0) return fail(PHYAMD_EDEVICE, "%s: node %d has no resident partial", name, n);
	}
	const size_t nsteps = L.steps.size(), ntc = L.cousins.size(), nto = L.outer.size(), nn = (size_t)N * N;
	const size_t at_steps = sizeof(BhessStart) * L.starts.size(), at_cousins = at_steps + sizeof(BhessStep) * nsteps, at_outer = at_cousins + sizeof(BhessTile) * ntc,
	             at_lower = at_outer + sizeof(BhessTile) * nto, at_upper = at_lower + sizeof(int32_t) * N, list_bytes = at_upper + sizeof(int32_t) * N;
	const size_t nblk_all = ((size_t)P + WAVE - 1) / WAVE;
	const ScratchPlan plan = bhess_plan(e, nsteps, ntc + nto, list_bytes);
	// the chunk: whole blocks whose scratch fits beside the engine, the whole scratch group counted free
	const double fit = plan.items_in(scratch_room(e, (double)batch_scratch_bytes(e), EngineRoom::MayGrow));
	if (fit < 1.0)
		return fail(PHYAMD_ENOMEM, "%s: the scratch of one block of 64 patterns (%.0f bytes, and %.0f for the matrix and the lists) does not fit the memory budget", name,
		            (double)plan.item_bytes(), (double)plan.fixed_bytes());
	const size_t nblk = (size_t)std::min((double)nblk_all, fit), Pc = nblk * WAVE;
	if (!plan.held(nblk) && e->cfg.max_device_bytes > 0) release_batch_scratch(e);  // (under a cap a call gets exactly its own scratch)
	if ((rc = plan.allocate(nblk))) return rc;

	std::vector<char> lists(list_bytes);
	std::memcpy(lists.data(), L.starts.data(), at_steps);
	std::memcpy(lists.data() + at_steps, L.steps.data(), sizeof(BhessStep) * nsteps);
	if (ntc) std::memcpy(lists.data() + at_cousins, L.cousins.data(), sizeof(BhessTile) * ntc);
	std::memcpy(lists.data() + at_outer, L.outer.data(), sizeof(BhessTile) * nto);
	std::memcpy(lists.data() + at_lower, lower_of.data(), sizeof(int32_t) * N);
	std::memcpy(lists.data() + at_upper, upper_of.data(), sizeof(int32_t) * N);
	HIP_TRY(hipMemcpyAsync(e->d_bhess_lists, lists.data(), list_bytes, hipMemcpyHostToDevice, e->stream));
	const char *dl = e->d_bhess_lists.get();
	const BhessStart *d_starts = reinterpret_cast<const BhessStart *>(dl);
	const BhessStep *d_steps = reinterpret_cast<const BhessStep *>(dl + at_steps);
	const BhessTile *d_cousins = reinterpret_cast<const BhessTile *>(dl + at_cousins), *d_outer = reinterpret_cast<const BhessTile *>(dl + at_outer);
	double *Hc = e->d_bhess_sums.get(), *H = Hc + nn, *gc = H + nn, *g = gc + N, *qp = g + N, *qqp = qp + (size_t)N * C * 16;
	hipLaunchKernelGGL(k_bhess_matrices, dim3((unsigned)(((size_t)N * C * 16 + 255) / 256)), dim3(256), 0, e->stream, N * C, C, e->d_mats.get(), e->d_Q.get(), e->d_rates.get(), qp,
	                   qqp);
	BhessArgs a{};
	a.steps = d_steps;
	a.lower_of = reinterpret_cast<const int32_t *>(dl + at_lower), a.upper_of = reinterpret_cast<const int32_t *>(dl + at_upper);
	a.T = e->T, a.N = N, a.P = P, a.C = C, a.root = e->root, a.fold = e->upper_fold ? 1 : 0;
	a.nsteps = (int)nsteps;
	a.tipmask = e->d_tipmask, a.lower = e->d_lower, a.upper = e->d_upper;
	a.mats = e->d_mats, a.qp = qp, a.qqp = qqp;
	a.freqs = e->d_freqs, a.props = e->d_props, a.weights = e->d_weights;
	a.site = e->d_bhess_rows.get(), a.G = a.site + 2 * Pc, a.slab = a.G + (size_t)N * Pc;
	a.tan = e->d_bhess_tan;
	double *cousin_out = e->d_bhess_tiles.get(), *outer_out = cousin_out + ntc * nblk * 256;
	for (size_t b0 = 0; b0 < nblk_all; b0 += nblk) {
		const size_t nb = std::min(nblk, nblk_all - b0);  // (the last chunk may be shorter: it runs in the same arrays at its own width)
		a.k0 = (int)(b0 * WAVE), a.nblk = (int)nb, a.Pc = (int)(nb * WAVE);
		a.G = a.site + 2 * (size_t)a.Pc, a.slab = a.G + (size_t)N * a.Pc;
		HIP_TRY(hipMemsetAsync(Hc, 0, sizeof(double) * nn, e->stream));
		hipLaunchKernelGGL(k_bhess_site, dim3((unsigned)((a.Pc + 255) / 256)), dim3(256), 0, e->stream, a);
		for (size_t y = 0; y < L.starts.size(); y += BATCH_MAX_CHUNK) {  // (gridDim.y)
			a.starts = d_starts + y;
			hipLaunchKernelGGL(k_bhess_walk, dim3((unsigned)nb, (unsigned)std::min<size_t>(L.starts.size() - y, BATCH_MAX_CHUNK)), dim3(WAVE, C), 0, e->stream, a);
		}
		for (size_t y = 0; y < ntc; y += BATCH_MAX_CHUNK)
			hipLaunchKernelGGL(k_bhess_cousins, dim3((unsigned)nb, (unsigned)std::min<size_t>(ntc - y, BATCH_MAX_CHUNK)), dim3(256), 0, e->stream, a, d_cousins + y,
			                   cousin_out + y * nb * 256);
		for (size_t y = 0; y < nto; y += BATCH_MAX_CHUNK)
			hipLaunchKernelGGL(k_bhess_outer, dim3((unsigned)nb, (unsigned)std::min<size_t>(nto - y, BATCH_MAX_CHUNK)), dim3(WAVE), 0, e->stream, a, d_outer + y,
			                   outer_out + y * nb * 256);
		BhessFinish f{0, N, (int)nb, e->root, (int)nsteps, b0 == 0 ? 1 : 0, nto * 256, d_outer, d_steps, outer_out, Hc, gc, H, g};
		const auto finish = [&] { hipLaunchKernelGGL(k_bhess_finish, dim3((unsigned)((f.count + 255) / 256)), dim3(256), 0, e->stream, f); };
		finish();
		f.mode = 1, f.count = nsteps + N, f.slab = a.slab;
		finish();
		if (ntc) {
			f.mode = 2, f.count = ntc * 256, f.tiles = d_cousins, f.slab = cousin_out;
			finish();
		}
		f.mode = 3, f.count = nn;
		finish();
		HIP_TRY(hipGetLastError());
		prof.chunks++;
	}
	HIP_TRY(hipMemcpyAsync(hessian, H, sizeof(double) * nn, hipMemcpyDeviceToHost, e->stream));
	if (gradient) HIP_TRY(hipMemcpyAsync(gradient, g, sizeof(double) * N, hipMemcpyDeviceToHost, e->stream));
	HIP_TRY(hipMemcpyAsync(e->h_result, e->d_result, sizeof(double), hipMemcpyDeviceToHost, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream));  // (also covers `lists`)
	*lnl = e->h_result[0];
	return PHYAMD_OK;
}

int shard_branch_hessian(Shard *e, int flags, double *lnl, double *gradient, double *hessian) {
	if (!e) return fail(PHYAMD_EINVAL, "phyamd_branch_hessian: null engine");
	if (flags != 0) return fail(PHYAMD_EINVAL, "phyamd_branch_hessian: flags %d (no flags are defined: pass 0)", flags);
	phyamd_hessian_profile known{};
	known.pairs = (int64_t)(e->N - 1) * e->N / 2;
	return profiled_call(e, &Shard::bhess_prof, known, [&](phyamd_hessian_profile &prof) {
		const int rc = run_branch_hessian(e, lnl, gradient, hessian, prof);
		if (!rc) mask_if_not_finite(*lnl, gradient, (size_t)e->N), mask_if_not_finite(*lnl, hessian, (size_t)e->N * e->N);
		return rc;
	});
}

// ---- per-pattern lnL of a batch of trees, and RELL replicates of them (phyamd_pattern_log_likelihoods_trees) --------------------

// (the post-order list with its slot words: site_lnl_ops, phyamd_tree_schedule.h)

constexpr size_t SITE_LNL_MAX_REPLICATES = (size_t)1 << 19;  // replicates per chunk: gridDim.y of k_reweight_mfma is a sixteenth

// What the call needs of the batch scratch per item for replicate chunks of `reps` rows: an item's lengths, matrices, op list and
// root, its `slots` parked partials (in d_batch_lower, where the batched walk keeps all T - 1), its row of log L_k (the product's R),
// its per-block sums and its lnL; and with replicates the product's segment sums and results per (replicate, item).  Whatever the
// item count: the replicate chunk's weight rows
ScratchPlan sitelnl_plan(Shard *e, int slots, size_t reps) {
	const size_t D = sizeof(double), N = (size_t)e->N, C = (size_t)e->C, nblk = ((size_t)e->P + WAVE - 1) / WAVE, Pc = nblk * WAVE;
	const size_t segments = (Pc + REWEIGHT_SEGMENT - 1) / REWEIGHT_SEGMENT;
	ScratchPlan p;
	p.add(e->d_batch_len, D * N);
	p.add(e->d_batch_mats, D * N * C * 16);
	p.add(e->d_batch_out, D);
	p.add(e->d_batch_lower, D * (size_t)slots * C * Pc * 4);
	p.add(e->d_batch_lnl, D * nblk);
	p.add(e->d_batch_item_ops, sizeof(BatchOp) * (size_t)(e->T - 1));
	p.add(e->d_batch_roots, sizeof(int32_t));
	p.add(e->d_reweight_R, D * Pc);
	if (reps > 0) {
		p.add(e->d_reweight_w, 0, D * reps * Pc);
		p.add(e->d_reweight_part, D * segments * reps);
		p.add(e->d_sitelnl_rell, D * reps);
	}
	return p;
}

// the items in chunks of what the scratch holds (for_tree_chunks); per chunk: the lengths go up, matrices, walk and finish are
// launched, the rows come back if they are wanted, and every replicate chunk is multiplied with the rows while they are resident
int run_site_lnl(Shard *e, int flags, int32_t count, const int32_t *left, const int32_t *right, const int32_t *roots, const double *branch_lengths, double *lnl,
                 double *pattern_lnl, size_t pattern_stride, int32_t replicate_count, const double *replicate_weights, size_t weight_stride, double *replicate_lnl,
                 phyamd_site_lnl_profile &prof) {
	static const char *const name = "phyamd_pattern_log_likelihoods_trees";
	int rc;
	if ((rc = check_ready_but_lengths(e))) return fail(rc, "%s: the engine is not ready: %s", name, std::string(g_last_error).c_str());
	if (flags != 0) return fail(PHYAMD_EUNSUPPORTED, "%s: flags %d (no flags are defined: pass 0)", name, flags);
	if (const char *why = tree_batch_refusal(e, 0, 1)) return fail(PHYAMD_EUNSUPPORTED, "%s: %s", name, why);
	const int T = e->T, P = e->P, C = e->C;
	const size_t N = (size_t)e->N, nblk = ((size_t)P + WAVE - 1) / WAVE, Pc = nblk * WAVE, R = (size_t)replicate_count;
	std::vector<int32_t> own_left, own_right, own_roots;
	if (!left) {  // every item is the engine's tree
		for (int32_t b = 0; b < count; b++) {
			own_left.insert(own_left.end(), e->left.begin(), e->left.end());
			own_right.insert(own_right.end(), e->right.begin(), e->right.end());
		}
		own_roots.assign(count, e->root);
		left = own_left.data(), right = own_right.data(), roots = own_roots.data();
	}
	// the replicate chunk: all of them if their weight rows take at most a quarter of the room, else as many as do (at least one)
	size_t reps = 0;
	if (R > 0) {
		const double room = scratch_room(e, (double)batch_scratch_bytes(e), EngineRoom::MayGrow);
		reps = (size_t)std::min((double)std::min(R, SITE_LNL_MAX_REPLICATES), std::max(1.0, std::floor(room / 4 / (double)(sizeof(double) * Pc))));
	}
	std::vector<BatchOp> work;
	std::vector<double> out, rows, rell;
	const auto item_ops = [&](const int32_t *l, const int32_t *r, int32_t root, std::vector<BatchOp> *ops) {
		const int parks = site_lnl_ops(T, l, r, root, work, ops);
		prof.lower_slots = std::max(prof.lower_slots, (int32_t)parks);
		return parks;
	};
	const auto plan_of = [&](int slots) { return sitelnl_plan(e, slots, reps); };
	const auto chunk = [&](size_t first, size_t items, int slots, const double *lengths, auto, auto) -> int {
		HIP_TRY(hipMemcpyAsync(e->d_batch_len, lengths, sizeof(double) * items * N, hipMemcpyHostToDevice, e->stream));
		launch_batch_matrices(e, (int)items, e->d_batch_len, e->d_batch_roots, e->d_batch_mats);
		const SiteLnlArgs a{e->d_batch_item_ops, T, e->N, P, C, (int)nblk, slots, e->d_tipmask, e->d_freqs, e->d_props, e->d_weights, e->d_batch_mats,
		                    e->d_batch_lower, e->d_reweight_R, e->d_batch_lnl};
		hipLaunchKernelGGL(k_sitelnl_walk4, dim3((unsigned)nblk, (unsigned)items), dim3(WAVE, C), 0, e->stream, a);
		hipLaunchKernelGGL(k_batch_finish, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, e->stream, (int)items, e->N, C, (int)nblk, e->root, e->d_batch_roots.get(), 1,
		                   e->d_batch_lnl.get(), (const double *)nullptr, e->d_batch_out.get());
		HIP_TRY(hipGetLastError());
		out.resize(items);
		HIP_TRY(hipMemcpyAsync(out.data(), e->d_batch_out, sizeof(double) * items, hipMemcpyDeviceToHost, e->stream));
		if (pattern_lnl) {
			rows.resize(items * Pc);
			HIP_TRY(hipMemcpyAsync(rows.data(), e->d_reweight_R, sizeof(double) * items * Pc, hipMemcpyDeviceToHost, e->stream));
		}
		HIP_TRY(hipStreamSynchronize(e->stream));  // (also covers the chunk's lists and lengths, reused by the next chunk)
		std::copy(out.begin(), out.end(), lnl + first);
		for (size_t b = 0; b < items && pattern_lnl; b++) std::copy(rows.begin() + b * Pc, rows.begin() + b * Pc + P, pattern_lnl + (first + b) * pattern_stride);
		prof.chunks++;
		for (size_t r0 = 0; r0 < R; r0 += reps) {  // every replicate chunk is multiplied with the rows while they are resident
			const size_t nr = std::min(reps, R - r0);
			ReweightArgs w;
			if (int rc = launch_reweight_product(e, replicate_weights + r0 * weight_stride, weight_stride, (size_t)P, nr, items, Pc, nullptr, &w)) return rc;
			hipLaunchKernelGGL(k_sitelnl_rell_finish, dim3((unsigned)((nr * items + 255) / 256)), dim3(256), 0, e->stream, (int)nr, (int)items, w.segments, e->d_reweight_part.get(),
			                   e->d_sitelnl_rell.get());
			HIP_TRY(hipGetLastError());
			rell.resize(nr * items);
			HIP_TRY(hipMemcpyAsync(rell.data(), e->d_sitelnl_rell, sizeof(double) * nr * items, hipMemcpyDeviceToHost, e->stream));
			HIP_TRY(hipStreamSynchronize(e->stream));
			for (size_t r = 0; r < nr; r++) std::copy(rell.begin() + r * items, rell.begin() + (r + 1) * items, replicate_lnl + (r0 + r) * (size_t)count + first);
			if (first == 0) prof.replicate_chunks++;
		}
		return PHYAMD_OK;
	};
	if ((rc = for_tree_chunks(e, name, 0, count, left, right, roots, branch_lengths, item_ops, plan_of, chunk))) return rc;
	// a lnL that is not finite is in band whatever the rescaling mode (the engine is never switched): its replicates are all NaN
	for (size_t b = 0; b < (size_t)count && R > 0; b++)
		if (not_finite(lnl[b]))
			for (size_t r = 0; r < R; r++) replicate_lnl[r * (size_t)count + b] = NAN;
	return PHYAMD_OK;
}

// reads the engine's inputs and writes only the batch scratch: nothing in Shard::state changes.  pattern_lnl: rows pattern_stride
// apart, replicate_weights: rows weight_stride apart, this shard's P patterns of either (the group layer passes the handle's
// pattern count and pointers advanced to this shard's range)
int shard_pattern_log_likelihoods_trees(Shard *e, int flags, int32_t count, const int32_t *left, const int32_t *right, const int32_t *roots, const double *branch_lengths,
                                        double *lnl, double *pattern_lnl, size_t pattern_stride, int32_t replicate_count, const double *replicate_weights,
                                        size_t weight_stride, double *replicate_lnl) {
	phyamd_site_lnl_profile known{};
	known.items = count;
	return profiled_call(e, &Shard::site_prof, known, [&](phyamd_site_lnl_profile &prof) {
		return run_site_lnl(e, flags, count, left, right, roots, branch_lengths, lnl, pattern_lnl, pattern_stride, replicate_count, replicate_weights, weight_stride,
		                    replicate_lnl, prof);
	});
}
