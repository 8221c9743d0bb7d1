// phyamd_eval.inc -- one evaluation: lower pass with incremental updates and the lazy rescaling switch, gradient passes, pattern tiling
// (part of phyamd_engine.hip: one translation unit, internal linkage)

// the engine's tree under its current options (schedule_options): the callers that change a switch come through here
int rebuild_schedule(Shard *e) {
	int rc;
	const std::string err = build_schedule(TreeRef{e->T, e->left.data(), e->right.data(), e->root}, schedule_options(e), &e->sched);
	if (!err.empty()) return fail(PHYAMD_EINVAL, "%s", err.c_str());
	if ((rc = upload_schedule(e))) return rc;
	if ((rc = ensure_lower_storage(e))) return rc;
	input_changed(e, Input::ScheduleRebuilt);
	return PHYAMD_OK;
}

void record(Shard *e, int i) {
	if (e->profiling) (void)hipEventRecord(e->ev[i], e->stream);
}

// lower pass (+ lazy rescaling).  On return d_result[0] holds lnL on the device.
// need_host_check: 1 = read lnL back and decide the lazy switch here; 2 = (gradient calls) send lnL on its way to the host and let
// the caller decide once its pre-order pass has been LAUNCHED (finish_lazy_check): the device does not idle between the passes
// for a host round trip (~40 us: 2.4 % of an evaluation at 500 taxa x 1e5 patterns).
int run_lower(Shard *e, int need_host_check) {
	int rc;
	if ((rc = bind_device(e))) return rc;
	if ((rc = check_ready(e))) return rc;
	e->check_pending = false;  // (a deferred check of a call that failed half way is dropped: this evaluation makes its own)
	record(e, 0);
	if ((rc = update_matrices(e))) return rc;
	record(e, 1);
	if (e->scaling_on && (rc = ensure_scaling_storage(e))) return rc;
	e->act_level_off = &e->sched.lower_level_off;
	e->act_lower_ops = e->d_lower_ops;
	e->incremental_pass = false;
	bool incremental = !e->state.all_dirty;
	if (incremental && e->lower_form != LowerForm::Reference && !lowers_current(e)) {
		// an incremental update reads stored children in the reference's form: this pass recomputes every node in it
		prefer_reference_form(e);
		incremental = false;
	}
	if (lowers_current(e)) {  // nothing changed: d_result[0] still holds lnL
		record(e, 2);
		e->prof.lower_launches = 0;
		e->prof_pending = e->profiling;
		e->prof_with_upper = false;
		return PHYAMD_OK;
	}
	uppers_dropped(e);  // partials are about to change
	std::vector<uint8_t> dirty;
	if (incremental) {
		// only single branch lengths changed since the stored partials were computed: recompute the core nodes on the paths
		// from those branches to the root, in level order (update_nodes[] semantics, treelikelihood.c:73-114, 1645-1734)
		dirty.assign(e->N, 0);
		// (20 / 60 / 61 states store t_n = P_n p_n: the branch's own node is recomputed too)
		for (int n : e->state.changed)
			for (int a = e->generic && n >= e->T ? n : e->sched.parent[n]; a >= 0 && !dirty[a]; a = e->sched.parent[a])
				if (e->sched.core_index[a] >= 0) dirty[a] = 1;  // fused fringe nodes are recomputed inside their first stored ancestor
		if (e->state.force_root) dirty[e->root] = 1;
	}
	if (e->state.stored_valid && e->stored.epoch == e->schedule_epoch) {
		// nodes about to be written leave the slot the stored state lives in (current_partials_indexes flip, treelikelihood.c:1693-1700)
		bool moved = false;
		for (int n = e->T; n < e->N; n++)
			if (e->sched.core_index[n] >= 0 && (!incremental || dirty[n]) && e->sched.core_index[n] == e->stored.core_index[n]) {
				e->sched.core_index[n] += e->sched.core_index[n] < e->sched.core_count ? e->sched.core_count : -e->sched.core_count;
				moved = true;
			}
		if (moved) {
			refresh_op_cores(e->sched);
			if ((rc = upload_schedule(e))) return rc;
		}
	}
	if (incremental) {
		e->inc_ops.clear();
		e->inc_level_off.assign(1, 0);
		for (size_t lv = 0; lv + 1 < e->sched.lower_level_off.size(); lv++) {
			for (int i = e->sched.lower_level_off[lv]; i < e->sched.lower_level_off[lv + 1]; i++)
				if (dirty[e->sched.lower_ops[i].parent]) e->inc_ops.push_back(e->sched.lower_ops[i]);
			e->inc_level_off.push_back((int)e->inc_ops.size());
		}
		if ((rc = e->d_inc_ops.ensure(e->N))) return rc;
		HIP_TRY(hipMemcpyAsync(e->d_inc_ops, e->inc_ops.data(), e->inc_ops.size() * sizeof(NodeOp), hipMemcpyHostToDevice, e->stream));
		HIP_TRY(hipStreamSynchronize(e->stream));  // inc_ops is reused by the next call
		e->act_level_off = &e->inc_level_off;
		e->act_lower_ops = e->d_inc_ops;
		e->incremental_pass = true;
	}
	for (int attempt = 0; attempt < 2; attempt++) {
		e->lnl_per_block = false;
		if (lower_kernel(e, false) == PassKernel::Stream && (rc = make_stream_buffers(e, true))) return rc;
		if ((rc = launch_lower(e, lower_kernel(e, true)))) return rc;
		if (e->lnl_per_block) {  // the tree walk: per-block sums, added in an order that depends on the pattern range alone
			if ((rc = reduce_block_sums(e, 0, e->d_lnl_part, e->lnl_blocks, 1, 1, nullptr, e->d_result))) return rc;
		} else
			hipLaunchKernelGGL(k_reduce_rows, dim3(1), dim3(64), 0, e->stream, e->d_lnl_part, e->generic ? e->nblk_root : e->lnl_blocks, (const uint8_t *)nullptr,
			                   e->d_result);
		HIP_TRY(hipGetLastError());
		if (e->cfg.rescale != PHYAMD_RESCALE_AUTO || e->scaling_on || !need_host_check) break;
		if (need_host_check == 2) {
			if (!e->ev_check) HIP_TRY(hipEventCreateWithFlags(&e->ev_check, hipEventDisableTiming));
			HIP_TRY(hipMemcpyAsync(e->h_result + 1 + (size_t)e->N * e->C + 2 * PHYAMD_MAX_PARAMETERS, e->d_result, sizeof(double), hipMemcpyDeviceToHost, e->stream));
			HIP_TRY(hipEventRecord(e->ev_check, e->stream));
			e->check_pending = true;
			break;
		}
		// lazy switch (treelikelihood.c:1496-1519): +-inf lnL turns rescaling on for good and recomputes
		HIP_TRY(hipMemcpyAsync(e->h_result, e->d_result, sizeof(double), hipMemcpyDeviceToHost, e->stream));
		HIP_TRY(hipStreamSynchronize(e->stream));
		if (!std::isinf(e->h_result[0])) break;
		e->scaling_on = true;
		if ((rc = rebuild_schedule(e))) return rc;  // the rescaled schedule (20 states: no walk lists), fringe fusion stays
		if ((rc = ensure_scaling_storage(e))) return rc;
		e->act_level_off = &e->sched.lower_level_off;  // and recomputes every node
		e->act_lower_ops = e->d_lower_ops;
		e->incremental_pass = false;
	}
	e->incremental_pass = false;
	lowers_computed(e);
	record(e, 2);
	e->prof_pending = e->profiling;
	e->prof_with_upper = false;
	return PHYAMD_OK;
}

// B_theta = U^-1 dQ_theta U, dP/dtheta matrices and their tip tables (recomputed per call: O(np N C) work)
int update_parameter_matrices(Shard *e) {
	const int S = e->S, np = e->np;
	int rc;
	if ((size_t)np * S * S > e->d_B.size()) {  // (the three grow together: all are freed before any is allocated again)
		e->d_B.release();
		e->d_dpm.release();
		e->d_dptab.release();
	}
	if ((rc = e->d_B.ensure((size_t)np * S * S)) || (rc = e->d_dpm.ensure((size_t)np * e->N * e->C * S * S)) || (rc = e->d_dptab.ensure((size_t)np * e->T * e->C * 64)) ||
	    (rc = e->d_ppart.ensure((size_t)np * e->sched.upper_ops.size() * ((size_t)e->nblk + 1))))
		return rc;
	if (e->state.params_dirty) {
		const std::vector<double> B = eigen_basis_derivatives(e);
		HIP_TRY(hipMemcpyAsync(e->d_B, B.data(), sizeof(double) * B.size(), hipMemcpyHostToDevice, e->stream));
		HIP_TRY(hipStreamSynchronize(e->stream));  // B is a stack-lifetime buffer
		parameter_basis_rebuilt(e);
	}
	const size_t total = (size_t)np * e->N * e->C * S * S;
	hipLaunchKernelGGL(k_parameter_matrices, dim3((unsigned)std::min<size_t>((total + 255) / 256, 4096)), dim3(256), 0, e->stream, S, e->C, e->N, np, e->d_model,
	                   e->d_B, e->d_rates, e->d_lengths, e->d_explicit, e->root, e->d_dpm);
	const int n = np * e->T * e->C * 64;
	hipLaunchKernelGGL(k_parameter_tip_tables, dim3((n + 255) / 256), dim3(256), 0, e->stream, e->T, e->N, e->C, np, e->d_dpm, e->d_dptab);
	HIP_TRY(hipGetLastError());
	return PHYAMD_OK;
}

// substitution-parameter sums of the 20 / 60 / 61-state engines on the stored partials of a keep-partials gradient
// (k_param_den_gen ... k_param_contract_gen); dst: [np] on the device
int launch_parameters_gen(Shard *e, double *dst) {
	const int S = e->S, S2 = S * S, np = e->np, B = e->N - 1;
	int rc;
	if ((rc = e->d_pg_nodes.ensure(B)) || (rc = e->d_pg_core.ensure(e->N)) || (rc = e->d_pg_den.ensure((size_t)B * e->P)) ||
	    (rc = e->d_pg_Gw.ensure(((size_t)B * e->C + 1) * S2)))
		return rc;
	bool grew;
	if ((rc = e->d_pg_B.ensure((size_t)np * S2, &grew))) return rc;
	{  // the schedule may have been rebuilt since the last call: the two index tables are N ints
		std::vector<int> nodes;
		for (int n = 0; n < e->N; n++)
			if (n != e->root) nodes.push_back(n);
		HIP_TRY(hipMemcpyAsync(e->d_pg_nodes, nodes.data(), sizeof(int) * nodes.size(), hipMemcpyHostToDevice, e->stream));
		HIP_TRY(hipMemcpyAsync(e->d_pg_core, e->sched.core_index.data(), sizeof(int) * e->N, hipMemcpyHostToDevice, e->stream));
		HIP_TRY(hipStreamSynchronize(e->stream));
	}
	if (grew || e->state.params_dirty) {
		const std::vector<double> Bm = eigen_basis_derivatives(e);
		HIP_TRY(hipMemcpyAsync(e->d_pg_B, Bm.data(), sizeof(double) * Bm.size(), hipMemcpyHostToDevice, e->stream));
		HIP_TRY(hipStreamSynchronize(e->stream));
		parameter_basis_rebuilt(e);
	}
	{  // the kernels below take every node's partial p_n itself; the post-order pass stores t_n = P_n p_n (k_lower_gen)
		const size_t npd = node_partial_doubles(e);
		if ((rc = e->d_pg_lower.ensure(lower_slots(e) * npd))) return rc;
		for (int n = e->T; n < e->N; n++)
			if (e->sched.core_index[n] >= 0 && (rc = true_lower_gen(e, n, e->d_pg_lower + (size_t)e->sched.core_index[n] * npd, nullptr))) return rc;
	}
	hipLaunchKernelGGL(k_param_den_gen, dim3((e->P + 255) / 256, B), dim3(256), 0, e->stream, e->d_pg_nodes, e->T, e->P, e->Pp, S, e->C, e->d_pg_core, e->d_tipmask,
	                   e->d_tipsets, e->d_pg_lower, e->d_upper, e->d_mats, e->d_freqs, e->d_props, e->d_pg_den);
	const size_t lds = sizeof(double) * 2 * (size_t)std::max(S2, S * (PARAM_CHUNK + 1));
	hipLaunchKernelGGL(k_param_outer_gen, dim3(B, e->C), dim3(256), lds, e->stream, e->d_pg_nodes, e->T, e->P, e->Pp, S, e->C, e->d_pg_core, e->d_tipmask,
	                   e->d_tipsets, e->d_pg_lower, e->d_upper, e->d_model, e->d_freqs, e->d_props, e->d_rates, e->d_lengths, e->d_explicit, e->d_weights,
	                   e->d_pg_den, e->d_pg_Gw);
	double *Gsum = e->d_pg_Gw + (size_t)B * e->C * S2;
	hipLaunchKernelGGL(k_param_sum_gen, dim3((S2 + 255) / 256), dim3(256), 0, e->stream, B * e->C, S2, e->d_pg_Gw, Gsum);
	hipLaunchKernelGGL(k_param_contract_gen, dim3(np), dim3(64), 0, e->stream, S2, e->d_pg_B, Gsum, dst);
	HIP_TRY(hipGetLastError());
	return PHYAMD_OK;
}

// d lnL / d pi_f through the root frequencies, f < S, written to dst (device) on the engine's stream
int launch_root_frequency_term(Shard *e, double *dst) {
	int rc;
	const int nb = (e->P + 255) / 256;
	if ((rc = e->d_rf_part.ensure(((size_t)nb + 1) * e->S))) return rc;
	const double *root = e->d_lower + (size_t)e->sched.core_index[e->root] * node_partial_doubles(e);
	const size_t cat_stride = e->generic ? (size_t)e->S * e->Pp : (size_t)e->P * e->S;
	const size_t pat_stride = e->generic ? 1 : (size_t)e->S, state_stride = e->generic ? (size_t)e->Pp : 1;
	hipLaunchKernelGGL(k_root_frequency_term, dim3(nb), dim3(256), 0, e->stream, e->P, e->S, e->C, root, cat_stride, pat_stride, state_stride, e->d_freqs,
	                   e->d_props, e->d_weights, e->d_rf_part);
	hipLaunchKernelGGL(k_reduce_rows, dim3(e->S), dim3(64), 0, e->stream, e->d_rf_part, nb, (const uint8_t *)nullptr, dst ? dst : e->d_rf_part + (size_t)nb * e->S);
	HIP_TRY(hipGetLastError());
	return PHYAMD_OK;
}

// sum_k (w_k / L_k) sum_i pi_i (p_root[cat 0] - mean of p_root[cat >= 1]) of the resident root partial -> dst (device), in whatever
// form the last post-order pass left it (CarriedExp2: with its per-category exponents)
int launch_root_invariant_term(Shard *e, double *dst) {
	int rc;
	const int nb = (e->P + 255) / 256;
	if ((rc = e->d_inv_part.ensure((size_t)nb + 1))) return rc;
	const double *root = e->d_lower + (size_t)e->sched.core_index[e->root] * node_partial_doubles(e);
	const size_t cat_stride = e->generic ? (size_t)e->S * e->Pp : (size_t)e->P * e->S;
	const size_t pat_stride = e->generic ? 1 : (size_t)e->S, state_stride = e->generic ? (size_t)e->Pp : 1;
	const int *Ec = e->lower_form == LowerForm::CarriedExp2 ? (const int *)e->d_Ec : nullptr;
	hipLaunchKernelGGL(k_root_invariant_term, dim3(nb), dim3(256), 0, e->stream, e->P, e->S, e->C, root, cat_stride, pat_stride, state_stride, e->d_freqs,
	                   e->d_props, e->d_weights, Ec, e->d_inv_part);
	hipLaunchKernelGGL(k_reduce_rows, dim3(1), dim3(64), 0, e->stream, e->d_inv_part, nb, (const uint8_t *)nullptr, dst ? dst : e->d_inv_part + nb);
	HIP_TRY(hipGetLastError());
	return PHYAMD_OK;
}

// the deferred half of the lazy switch (run_lower, need_host_check = 2): true = lnL was +-inf, rescaling is on now and the whole
// evaluation has to run again (once per engine at most: the switch is for good)
int finish_lazy_check(Shard *e, bool *again) {
	int rc;
	*again = false;
	if (!e->check_pending) return PHYAMD_OK;
	e->check_pending = false;
	HIP_TRY(hipEventSynchronize(e->ev_check));
	if (!std::isinf(e->h_result[1 + (size_t)e->N * e->C + 2 * PHYAMD_MAX_PARAMETERS])) return PHYAMD_OK;
	e->scaling_on = true;
	if ((rc = rebuild_schedule(e))) return rc;
	if ((rc = ensure_scaling_storage(e))) return rc;
	*again = true;
	return PHYAMD_OK;
}

int run_gradient(Shard *e, int flags, bool with_params = false) {
	int rc;
	// the streamed walks' own forms serve the plain gradient only: parameter sums, the reference's folded / per-category arithmetic
	// and resident uppers read stored partials with other kernels
	if (with_params || e->keep_partials || (e->scaling_on && (flags & PHYAMD_GRAD_COMPAT_SCALED))) {
		if ((rc = bind_device(e))) return rc;
		if ((rc = require_reference_form(e))) return rc;  // (stored lowers of an earlier call in another form: computed again)
	} else if (e->scaling_on && (flags & PHYAMD_GRAD_FOLD_ROOT_FREQS))
		prefer_reference_form(e);  // (the reference's folded arithmetic under rescaling: its form from the next post-order pass on)
	e->upper_fold = (flags & PHYAMD_GRAD_FOLD_ROOT_FREQS) != 0;
	if (with_params) {
		if (e->np < 1) return fail(PHYAMD_EINVAL, "phyamd_set_rate_matrix_derivatives has not been called");
		if (!e->have_eigen) return fail(PHYAMD_EINVAL, "substitution-parameter gradients need the eigen system (phyamd_set_eigen)");
		if (flags & PHYAMD_GRAD_FOLD_ROOT_FREQS)
			return fail(PHYAMD_EINVAL, "PHYAMD_GRAD_FOLD_ROOT_FREQS cannot be combined with parameter gradients (the reference clears include_root_freqs, treelikelihood.c:291-305)");
	}
	if (with_params && e->generic && !e->keep_partials) {
		// the 20 / 60 / 61-state parameter kernels read every node's lower and upper partial: keep them from here on
		if ((rc = bind_device(e))) return rc;
		e->keep_partials = true;
		if ((rc = rebuild_schedule(e))) return rc;
	}
	if ((rc = run_lower(e, e->tiles == 1 ? 2 : 1))) return rc;
	if ((flags & PHYAMD_GRAD_FOLD_ROOT_FREQS) && e->scaling_on && e->sched.fused) {
		// The reference's folded-frequency arithmetic is inexact for non-uniform pi (DESIGN.md, quirk 1): under rescaling every
		// branch then has its own "site likelihood" as denominator, which the fused fringe does not form.  Reproducing it takes
		// the unfused schedule (every internal node stored) from here on.
		e->fusion_enabled = false;
		if ((rc = rebuild_schedule(e))) return rc;
		if ((rc = run_lower(e, true))) return rc;
	}
	// (a tile's post-order pass decides the lazy switch itself: rescaling may have come on after the requirement above was settled)
	if (e->scaling_on && (flags & PHYAMD_GRAD_COMPAT_SCALED) && (rc = require_reference_form(e))) return rc;
	PassKernel k = upper_kernel(e, flags, with_params, false);
	if ((rc = ensure_upper_storage(e, k))) return rc;
	if (!e->have_Q) return fail(PHYAMD_EINVAL, "the gradient needs the rate matrix: phyamd_set_eigen or phyamd_set_rate_matrix");
	if (k != PassKernel::Levels && (rc = upload_qpi(e))) return rc;  // (the walks' branch terms: diag(pi) Q)
	if (k == PassKernel::Stream && (rc = make_stream_buffers(e, false))) return rc;
	k = upper_kernel(e, flags, with_params, true);
	const bool walk_params = with_params && k == PassKernel::Walk;
	e->grad_blocks = e->nblk;
	e->slab_walk_order = false;
	// (the compat flag changes only the branch terms; parameter sums always use the mixture denominator: level kernels then)
	if (with_params && !e->generic) {
		if (k == PassKernel::Levels && (rc = update_parameter_matrices(e))) return rc;
		if ((rc = launch_upper_params(e, flags, k))) return rc;
	} else if ((rc = launch_upper(e, flags, k)))
		return rc;
	record(e, 3);
	if (e->slab_walk_order) {
		if ((rc = reduce_stream_slab(e, e->d_result + 1))) return rc;
	} else
		hipLaunchKernelGGL(k_reduce_rows, dim3(e->N * e->C), dim3(64), 0, e->stream, e->d_gpart, e->grad_blocks, e->d_row_valid, e->d_result + 1);
	if (walk_params) {
		if ((rc = launch_root_frequency_term(e, e->d_result + 1 + (size_t)e->N * e->C + e->np))) return rc;
	} else if (with_params && e->generic) {
		if ((rc = launch_parameters_gen(e, e->d_result + 1 + (size_t)e->N * e->C))) return rc;
		if ((rc = launch_root_frequency_term(e, e->d_result + 1 + (size_t)e->N * e->C + e->np))) return rc;
	} else if (with_params) {  // [np][ops][nblk] -> [np][ops] -> [np], fixed order
		const int ops = (int)e->sched.upper_ops.size();
		double *stage = e->d_ppart + (size_t)e->np * ops * e->nblk;
		hipLaunchKernelGGL(k_reduce_rows, dim3(e->np * ops), dim3(64), 0, e->stream, e->d_ppart, e->nblk, (const uint8_t *)nullptr, stage);
		hipLaunchKernelGGL(k_reduce_rows, dim3(e->np), dim3(64), 0, e->stream, stage, ops, (const uint8_t *)nullptr, e->d_result + 1 + (size_t)e->N * e->C);
		if ((rc = launch_root_frequency_term(e, e->d_result + 1 + (size_t)e->N * e->C + e->np))) return rc;
	}
	HIP_TRY(hipGetLastError());
	record(e, 4);
	e->prof_with_upper = true;
	uppers_computed(e);
	bool again = false;
	if ((rc = finish_lazy_check(e, &again))) return rc;
	return again ? run_gradient(e, flags, with_params) : PHYAMD_OK;
}

// Every branch's d lnL / dt and d2 lnL / dt2 (phyamd_branch_hessian_diagonal): raw sums [lnL | d1 | d2] over this engine's patterns
// (or tile) to out.  The HESS pass reads the stored lowers in the reference's form; unlike the other readers this call does not
// keep the engine on that form: an engine whose streamed walks store another one recomputes its lowers in that form at the next
// evaluation, so lnL and gradients afterwards are those of an engine that never made the call.
int run_hessian(Shard *e, double *out) {
	int rc;
	if ((rc = bind_device(e))) return rc;
	const bool form_only = e->reference_form_only;
	e->reference_form_only = true;
	// 20 states fuse cherries into their parents' ops, which leaves their tip branches without rows: the unfused schedule for this
	// call, the fused one again afterwards (rebuild_schedule: the next evaluation recomputes every node, as a new engine would)
	const bool unfuse = e->generic && e->sched.fused;
	if (unfuse) {
		e->fusion_enabled = false;
		rc = rebuild_schedule(e);
	}
	if (!rc) rc = run_lower(e, 1);
	if (!rc) rc = require_reference_form(e);
	if (!rc && !(rc = ensure_upper_storage(e, PassKernel::Levels)) && !(rc = ensure_hess_storage(e))) rc = launch_hess(e, out);
	if (unfuse) {
		e->fusion_enabled = true;
		const int rc2 = rebuild_schedule(e);
		if (!rc) rc = rc2;
	}
	uppers_dropped(e);  // (the level pass's uppers: not those a keep-partials gradient leaves)
	if (!form_only) {
		e->reference_form_only = false;
		if (e->lower_form != stream_lower_form(e)) lowers_discarded(e);
	}
	return rc;
}

// [lnL | d1[N] | d2[N]]: a NaN / inf lnL makes every derivative NaN (treelikelihood.c:327-332)
__global__ void k_hess_finish(int n, double *__restrict__ v) {
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const double l = v[0];
	if (isnan(l) || isinf(l)) v[1 + i] = NAN;
}

__global__ void k_accumulate(int n, const double *__restrict__ src, double *__restrict__ dst) {
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) dst[i] += src[i];
}

// One evaluation = every tile in turn through the same partial storage; the per-tile results ([lnL | gradient rows | parameter
// sums | root frequency term]: all of them sums over patterns) are added in tile order (fixed: reproducible).
// mode 0: post-order pass only; 1: + pre-order pass and branch gradient; 2: + substitution-parameter sums; 3: the HESS pass
// ([lnL | d1 | d2] in hess_result instead of d_result)
int run_tiled(Shard *e, int mode, int flags) {
	int rc;
	if ((rc = bind_device(e))) return rc;
	if (mode == 3 && (rc = ensure_hess_storage(e))) return rc;
	const int n = mode == 0 ? 1 : mode == 3 ? 1 + 2 * e->N : 1 + e->N * e->C + (mode == 2 ? e->np + e->S : 0);
	double *result = mode == 3 ? hess_result(e) : e->d_result, *total = mode == 3 ? hess_total(e) : e->d_total;
	HIP_TRY(hipMemsetAsync(total, 0, sizeof(double) * n, e->stream));
	double *inv_total = e->d_total + (size_t)e->N * e->C + 2 * PHYAMD_MAX_PARAMETERS;  // the last entry of the allocation: the +I root term
	HIP_TRY(hipMemsetAsync(inv_total, 0, sizeof(double), e->stream));
	const uint8_t unknown = e->generic ? (uint8_t)e->S : (uint8_t)0xF;
	for (int t = 0; t < e->tiles; t++) {
		const size_t off = (size_t)t * e->P;
		const size_t w = std::min<size_t>((size_t)e->P, (size_t)e->Ptot - off);
		HIP_TRY(hipMemcpy2DAsync(e->d_tipmask, (size_t)e->P, e->d_tip_all + off, (size_t)e->Ptot, w, (size_t)e->T, hipMemcpyDeviceToDevice, e->stream));
		HIP_TRY(hipMemcpyAsync(e->d_weights, e->d_weights_all + off, sizeof(double) * w, hipMemcpyDeviceToDevice, e->stream));
		if (w < (size_t)e->P) {  // ragged last tile: unknown tips of weight 0 (L = 1, log L = 0, no gradient)
			HIP_TRY(hipMemset2DAsync(e->d_tipmask + w, (size_t)e->P, unknown, (size_t)e->P - w, (size_t)e->T, e->stream));
			HIP_TRY(hipMemsetAsync(e->d_weights + w, 0, sizeof(double) * ((size_t)e->P - w), e->stream));
		}
		tile_loaded(e);
		if ((rc = mode == 0 ? run_lower(e, true) : mode == 3 ? run_hessian(e, result) : run_gradient(e, flags, mode == 2))) return rc;
		hipLaunchKernelGGL(k_accumulate, dim3((n + 255) / 256), dim3(256), 0, e->stream, n, result, total);
		if (e->C >= 2) {  // the +I site-model gradient needs this tile's root partial while it is resident (in the form it is in)
			if ((rc = launch_root_invariant_term(e, nullptr))) return rc;
			hipLaunchKernelGGL(k_accumulate, dim3(1), dim3(64), 0, e->stream, 1, e->d_inv_part + (e->P + 255) / 256, inv_total);
		}
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipMemcpyAsync(e->d_plk_all + off, e->d_plk, sizeof(double) * w, hipMemcpyDeviceToDevice, e->stream));
	}
	HIP_TRY(hipMemcpyAsync(result, total, sizeof(double) * n, hipMemcpyDeviceToDevice, e->stream));
	tiled_totals_computed(e, mode == 2);
	return PHYAMD_OK;
}

int eval_lower(Shard *e) { return e->tiles > 1 ? run_tiled(e, 0, 0) : run_lower(e, true); }
// [lnL | d1 | d2] in hess_result(e), the NaN rule applied
int eval_hessian(Shard *e) {
	int rc;
	if ((rc = bind_device(e)) || (rc = ensure_hess_storage(e))) return rc;
	if ((rc = e->tiles > 1 ? run_tiled(e, 3, 0) : run_hessian(e, hess_result(e)))) return rc;
	hipLaunchKernelGGL(k_hess_finish, dim3((2 * e->N + 255) / 256), dim3(256), 0, e->stream, 2 * e->N, hess_result(e));
	HIP_TRY(hipGetLastError());
	return PHYAMD_OK;
}
int eval_gradient(Shard *e, int flags, bool with_params = false) {
	return e->tiles > 1 ? run_tiled(e, with_params ? 2 : 1, flags) : run_gradient(e, flags, with_params);
}

// destination of one tip's pattern codes: the engine's own table, or the all-tiles table
uint8_t *tip_row(Shard *e, int tip) { return e->tiles > 1 ? e->d_tip_all + (size_t)tip * e->Ptot : e->d_tipmask + (size_t)tip * e->P; }

#define NOT_TILED(e, what) \
	if ((e)->tiles > 1) return fail(PHYAMD_EUNSUPPORTED, what " is not available when the patterns are processed in tiles (max_device_bytes)")

void finish_profile(Shard *e, bool with_upper) {
	if (!e->profiling || !e->prof_pending) return;
	e->prof_pending = false;
	(void)hipEventSynchronize(e->ev[with_upper ? 4 : 2]);
	float ms = 0;
	(void)hipEventElapsedTime(&ms, e->ev[0], e->ev[1]);
	e->prof.matrices_ms = ms;
	(void)hipEventElapsedTime(&ms, e->ev[1], e->ev[2]);
	e->prof.lower_ms = ms;
	e->prof.upper_ms = e->prof.reduce_ms = 0;
	if (with_upper) {
		(void)hipEventElapsedTime(&ms, e->ev[2], e->ev[3]);
		e->prof.upper_ms = ms;
		(void)hipEventElapsedTime(&ms, e->ev[3], e->ev[4]);
		e->prof.reduce_ms = ms;
	}
}
