// phyamd_schedule.inc -- the engine's side of its schedule (a Schedule and a StreamTables, built by phyamd_tree_schedule.h): device
// storage, upload, readiness
// (part of phyamd_engine.hip: one translation unit, internal linkage)

int bind_device(Shard *e) {
	HIP_TRY(hipSetDevice(e->device));
	return PHYAMD_OK;
}

size_t node_partial_doubles(const Shard *e) { return (size_t)e->C * e->S * (e->generic ? e->Pp : e->P); }
size_t lower_slots(const Shard *e) { return e->d_lower.size() / node_partial_doubles(e); }  // node partials d_lower holds
size_t upper_slots_held(const Shard *e) { return e->d_upper.size() / node_partial_doubles(e); }

int ensure_lower_storage(Shard *e) {
	const size_t need = (size_t)std::max(1, e->sched.core_count) * (e->two_slots ? 2 : 1);
	if (lower_slots(e) >= need) return PHYAMD_OK;
	e->d_lower.release();
	e->d_lscale.release();  // (sized by d_lower: ensure_scaling_storage)
	return e->d_lower.ensure(need * node_partial_doubles(e));
}

// after slots moved (store / restore): the ops carry slot indices
void refresh_op_cores(Schedule &s) {
	for (std::vector<NodeOp> *ops : {&s.lower_ops, &s.upper_ops, &s.walk_lower_ops, &s.walk_upper_ops, &s.walk_chunk_ops, &s.walk_lower_chunk_ops})
		for (NodeOp &op : *ops) {
			op.core_parent = s.core_index[op.parent];
			op.core_left = s.core_index[op.left];
			op.core_right = s.core_index[op.right];
		}
}

int upload_schedule(Shard *e) {
	// op tables are a few KB: allocated once at the maximum size (N - T ops each)
	int rc;
	if ((rc = e->d_lower_ops.ensure(e->N)) || (rc = e->d_upper_ops.ensure(e->N))) return rc;
	HIP_TRY(hipMemcpyAsync(e->d_lower_ops, e->sched.lower_ops.data(), e->sched.lower_ops.size() * sizeof(NodeOp), hipMemcpyHostToDevice, e->stream));
	HIP_TRY(hipMemcpyAsync(e->d_upper_ops, e->sched.upper_ops.data(), e->sched.upper_ops.size() * sizeof(NodeOp), hipMemcpyHostToDevice, e->stream));
	static_assert(sizeof(DeepDesc) == 6 * sizeof(double), "DeepDesc is laid out in the tail of the tip-message table");
	if (!e->generic)
		HIP_TRY(hipMemcpyAsync(e->d_tiptab + (size_t)e->T * e->C * 64, e->sched.deep_host.data(), e->sched.deep_host.size() * sizeof(DeepDesc), hipMemcpyHostToDevice,
		                       e->stream));
	if (e->sched.walking || e->sched.gen_walking) {
		if ((rc = e->d_walk_lower_ops.ensure(e->N)) || (rc = e->d_walk_upper_ops.ensure(e->N))) return rc;
		HIP_TRY(hipMemcpyAsync(e->d_walk_lower_ops, e->sched.walk_lower_ops.data(), e->sched.walk_lower_ops.size() * sizeof(NodeOp), hipMemcpyHostToDevice, e->stream));
		HIP_TRY(hipMemcpyAsync(e->d_walk_upper_ops, e->sched.walk_upper_ops.data(), e->sched.walk_upper_ops.size() * sizeof(NodeOp), hipMemcpyHostToDevice, e->stream));
	}
	if (e->sched.walking) {
		if ((rc = e->d_walk_chunk_ops.ensure(e->N)) || (rc = e->d_walk_chunk_off.ensure((size_t)e->N + 2))) return rc;
		HIP_TRY(hipMemcpyAsync(e->d_walk_chunk_ops, e->sched.walk_chunk_ops.data(), e->sched.walk_chunk_ops.size() * sizeof(NodeOp), hipMemcpyHostToDevice, e->stream));
		HIP_TRY(hipMemcpyAsync(e->d_walk_chunk_off, e->sched.walk_chunk_off.data(), e->sched.walk_chunk_off.size() * sizeof(int), hipMemcpyHostToDevice, e->stream));
		if ((rc = e->d_walk_lower_chunk_ops.ensure(e->N)) || (rc = e->d_walk_lower_chunk_off.ensure((size_t)e->N + 2))) return rc;
		HIP_TRY(hipMemcpyAsync(e->d_walk_lower_chunk_ops, e->sched.walk_lower_chunk_ops.data(), e->sched.walk_lower_chunk_ops.size() * sizeof(NodeOp), hipMemcpyHostToDevice, e->stream));
		HIP_TRY(hipMemcpyAsync(e->d_walk_lower_chunk_off, e->sched.walk_lower_chunk_off.data(), e->sched.walk_lower_chunk_off.size() * sizeof(int), hipMemcpyHostToDevice, e->stream));
		if (stream_possible(e)) {  // the streamed walks' tables follow the chunked lists (core indices included: store / restore moves them)
			build_stream_tables(e->sched, StreamGeometry{e->P, e->C, (size_t)e->nblk_walk_upper * e->G * WAVE, e->stream_elide_on, e->stream_pairs_on, e->stream_keep_on},
			                    &e->stream_tab);
			// (descriptors and chunks twice: those of the TF forms, then the plain ones behind them -- stream_elide, stream_plain_ops;
			// the descriptors a third time, with the pair ops, at 2 x their count -- stream_pairs)
			if ((rc = e->d_stream_ops.ensure((size_t)3 * e->N)) || (rc = e->d_stream_pair_tab.ensure((size_t)e->N * 16)) || (rc = e->d_stream_chunks.ensure((size_t)2 * e->N + 4)) ||
			    (rc = e->d_stream_row_entries.ensure(std::max((size_t)e->N * 32, e->stream_tab.row_entries.size()))) ||
			    (rc = e->d_stream_site_tab.ensure((size_t)e->N * 16)) || (rc = e->d_stream_qnode.ensure(e->N)) || (rc = e->d_stream_op_tips.ensure((size_t)e->N * 12)) ||
			    (rc = e->d_stream_flag.ensure(1)) || (rc = e->d_stream_op_deep.ensure(e->N)))
				return rc;
			HIP_TRY(hipMemcpyAsync(e->d_stream_op_tips, e->stream_tab.op_tips.data(), e->stream_tab.op_tips.size() * sizeof(int), hipMemcpyHostToDevice, e->stream));
			HIP_TRY(hipMemcpyAsync(e->d_stream_op_deep, e->stream_tab.op_deep.data(), e->stream_tab.op_deep.size() * sizeof(int), hipMemcpyHostToDevice, e->stream));
			HIP_TRY(hipMemcpyAsync(e->d_stream_ops, e->stream_tab.desc.data(), e->stream_tab.desc.size() * sizeof(StreamDesc), hipMemcpyHostToDevice, e->stream));
			HIP_TRY(hipMemcpyAsync(e->d_stream_chunks, e->stream_tab.chunks.data(), e->stream_tab.chunks.size() * sizeof(StreamChunk), hipMemcpyHostToDevice, e->stream));
			if (!e->stream_tab.plain_desc.empty()) {
				HIP_TRY(hipMemcpyAsync(e->d_stream_ops + e->stream_tab.desc.size(), e->stream_tab.plain_desc.data(), e->stream_tab.plain_desc.size() * sizeof(StreamDesc),
				                       hipMemcpyHostToDevice, e->stream));
				HIP_TRY(hipMemcpyAsync(e->d_stream_chunks + e->stream_tab.chunks.size(), e->stream_tab.plain_chunks.data(),
				                       e->stream_tab.plain_chunks.size() * sizeof(StreamChunk), hipMemcpyHostToDevice, e->stream));
			}
			if (!e->stream_tab.pair_desc.empty()) {
				HIP_TRY(hipMemcpyAsync(e->d_stream_ops + 2 * e->stream_tab.desc.size(), e->stream_tab.pair_desc.data(), e->stream_tab.pair_desc.size() * sizeof(StreamDesc),
				                       hipMemcpyHostToDevice, e->stream));
				HIP_TRY(hipMemcpyAsync(e->d_stream_pair_tab, e->stream_tab.pair_tab.data(), e->stream_tab.pair_tab.size() * sizeof(int), hipMemcpyHostToDevice, e->stream));
			}
			HIP_TRY(hipMemcpyAsync(e->d_stream_row_entries, e->stream_tab.row_entries.data(), e->stream_tab.row_entries.size() * sizeof(int), hipMemcpyHostToDevice, e->stream));
			HIP_TRY(hipMemcpyAsync(e->d_stream_site_tab, e->stream_tab.site_tab.data(), e->stream_tab.site_tab.size() * sizeof(int), hipMemcpyHostToDevice, e->stream));
			HIP_TRY(hipMemcpyAsync(e->d_stream_qnode, e->stream_tab.qnode.data(), e->stream_tab.qnode.size() * sizeof(int), hipMemcpyHostToDevice, e->stream));
			if ((rc = e->d_lstream_ops.ensure(e->N)) || (rc = e->d_lstream_chunks.ensure((size_t)e->N + 2))) return rc;
			HIP_TRY(hipMemcpyAsync(e->d_lstream_ops, e->stream_tab.lower_desc.data(), e->stream_tab.lower_desc.size() * sizeof(LowerDesc), hipMemcpyHostToDevice, e->stream));
			HIP_TRY(hipMemcpyAsync(e->d_lstream_chunks, e->stream_tab.lower_chunks.data(), e->stream_tab.lower_chunks.size() * sizeof(LowerChunk), hipMemcpyHostToDevice, e->stream));
		}
	}
	// rows of the gradient slab that are produced by the upper pass (every non-root node)
	std::vector<uint8_t> valid((size_t)e->N * e->C, 1);
	for (int c = 0; c < e->C; c++) valid[(size_t)e->root * e->C + c] = 0;
	HIP_TRY(hipMemcpyAsync(e->d_row_valid, valid.data(), valid.size(), hipMemcpyHostToDevice, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream));
	return PHYAMD_OK;
}

// the tree-walk schedule parks far fewer uppers than the level schedule keeps; parameter gradients and the Hessian can still run
// the level kernels, so the larger of the two is held once a Levels pre-order pass has run
size_t upper_slots_needed(const Shard *e) {
	const bool level_path = !e->sched.walking || e->level_upper_needed;  // (20-state walks: both, they alternate with level passes)
	return (size_t)std::max(1, level_path ? std::max(e->sched.upper_slots, e->sched.walk_upper_slots) : e->sched.walk_upper_slots);
}

// d_upper for a pre-order pass of family k (upper_kernel; the Hessian's: Levels)
int ensure_upper_storage(Shard *e, PassKernel k) {
	if (k == PassKernel::Levels) e->level_upper_needed = true;
	return e->d_upper.ensure(upper_slots_needed(e) * node_partial_doubles(e));
}

int ensure_scaling_storage(Shard *e) { return e->d_lscale.ensure(lower_slots(e) * e->P); }

int check_ready(Shard *e) {
	if (!e->have_topology) return fail(PHYAMD_EINVAL, "phyamd_set_topology has not been called");
	if (!e->have_lengths) return fail(PHYAMD_EINVAL, "phyamd_set_branch_lengths has not been called");
	if (!e->have_freqs) return fail(PHYAMD_EINVAL, "phyamd_set_frequencies has not been called");
	if (!e->have_rates) return fail(PHYAMD_EINVAL, "phyamd_set_category_rates has not been called");
	if (!e->have_weights) return fail(PHYAMD_EINVAL, "phyamd_set_pattern_weights has not been called");
	for (int t = 0; t < e->T; t++)
		if (!e->tip_set[t]) return fail(PHYAMD_EINVAL, "tip %d has no data (phyamd_set_tip_states / phyamd_set_tip_partials)", t);
	if (!e->have_eigen) {
		for (int n = 0; n < e->N; n++)
			if (n != e->root && !e->explicit_host[n]) return fail(PHYAMD_EINVAL, "no eigen system and node %d has no explicit matrices", n);
	}
	return PHYAMD_OK;
}
