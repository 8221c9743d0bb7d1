// phyamd_place_calls.inc -- the placement calls on one shard: query sequences scored on every edge of the engine's tree and the three
// branches around chosen placements optimised, for 4 and for 20 states.  What a 4-state call and its 20-state twin share is written
// once -- the chunk sizes and the loop over node columns x query chunks (place_chunk_sizes, run_place_chunks), the sorted
// candidates, their chunks and the scatter of their results (sort_candidates, qopt_chunk_size, run_qopt_chunks), the wording of the
// preconditions and the own-partial records of the 20-state calls (general_placement_call, place_own_of) -- and a call keeps what is its own:
// its scratch plan, what it prepares once, its tables or records and its kernels.  They read what the engine holds and write only
// the batch scratch (part of phyamd_engine.hip: one translation unit, internal linkage; behind phyamd_queries.inc, whose scratch
// plans, NNI walk and profiled_call these use)

// ---- what the four calls share ----------------------------------------------------------------------------------------------------

struct PlacementArgs {
	int32_t queries;
	const uint8_t *masks;  // [queries][P], validated (phyamd_placement_log_likelihoods)
	int32_t lengths;
	const double *pendant;
	double split;
	double *lnl;
	int32_t *best_node;
	double *best_lnl;
};

struct PlacementGeneralArgs {
	PlacementArgs p;       // masks: the class codes [queries][P], validated (phyamd_placement_log_likelihoods_general)
	int32_t set_count;
	const uint64_t *sets;  // [set_count], validated
};

struct PlacementOptimizeArgs {
	int32_t queries;
	const uint8_t *masks;       // [queries][P], validated (phyamd_placement_optimize)
	int32_t count;
	const int32_t *candidates;  // [count][2]: (query, node), the queries validated
	const double *pendant_start;
	double split;
	int32_t branches;
	double lower, upper, tolerance;
	int32_t max_iterations;
	double lnl_tolerance;
	int32_t max_passes;
	double *lengths, *lnl, *initial_lnl;
	int32_t *passes;
};

struct PlacementOptimizeGeneralArgs {
	PlacementOptimizeArgs p;  // masks: the class codes [queries][P], validated (phyamd_placement_optimize_general)
	int32_t set_count;
	const uint64_t *sets;     // [set_count], validated
};

constexpr size_t PLACE_GEN_MATRIX = (size_t)PLACE_GEN_STATES * PLACE_GEN_STATES;

// the largest x in lo..hi with ok(x), ok being true up to some x and false beyond; lo - 1: none
template <typename Ok>
size_t largest_that(size_t lo, size_t hi, Ok ok) {
	if (!ok(lo)) return lo - 1;
	while (lo < hi) {
		const size_t mid = lo + (hi - lo + 1) / 2;
		if (ok(mid)) lo = mid;
		else hi = mid - 1;
	}
	return lo;
}

// (the preconditions of the two 20-state calls: check_general_query_inputs / _resident, phyamd_queries.inc, which
// phyamd_placement_optimize_general runs in two halves with its candidates checked in between)
GeneralQueryCall general_placement_call(const char *name, const char *use_4_state_call, const char *eigen_use, const char *what_does_not_rescale) {
	return GeneralQueryCall{name, "the class tables are", use_4_state_call, "tables of 64 classes are", "which cannot be split at sigma", eigen_use, what_does_not_rescale};
}

// What k_classplace_own forms internal node `node`'s own partial from, into `out`: a stored array is the message P_n p_n, so the
// node's own partial is formed again from its two children (a tip child: its code row; an internal one: its stored message)
int place_own_of(Shard *e, const char *name, int node, double *out, PlaceGenOwn *own) {
	const size_t npd = node_partial_doubles(e), msz = (size_t)e->C * PLACE_GEN_MATRIX;
	const int T = e->T, ch[2] = {e->left[node], e->right[node]};
	*own = PlaceGenOwn{};
	own->out = out;
	for (int side = 0; side < 2; side++) {
		const int v = ch[side];
		if (v >= T && e->sched.core_index[v] < 0) return fail(PHYAMD_EDEVICE, "%s: node %d has no resident lower partial", name, v);
		(side ? own->mat_r : own->mat_l) = e->d_mats + (size_t)v * msz;
		(side ? own->src_r : own->src_l) = v < T ? nullptr : e->d_lower + (size_t)e->sched.core_index[v] * npd;
		(side ? own->row_r : own->row_l) = v < T ? e->d_tipmask + (size_t)v * e->P : nullptr;
	}
	return PHYAMD_OK;
}

// the internal nodes' own partials of a chunk, `owns` built by place_own_of
int launch_place_owns(Shard *e, const std::vector<PlaceGenOwn> &owns) {
	if (owns.empty()) return PHYAMD_OK;
	HIP_TRY(hipMemcpyAsync(e->d_placeg_owns, owns.data(), sizeof(PlaceGenOwn) * owns.size(), hipMemcpyHostToDevice, e->stream));
	hipLaunchKernelGGL(k_classplace_own, dim3((unsigned)((e->P + 255) / 256), (unsigned)owns.size(), (unsigned)e->C), dim3(256), 0, e->stream, e->d_placeg_owns.get(), e->P, e->Pp,
	                   e->d_tipsets.get());
	return PHYAMD_OK;
}

// ---- query sequences on every edge of the engine's tree (phyamd_placement_log_likelihoods[_general]) -----------------------------

// the NNI walk's (nni_base_plan, with d_nni_mats for the split matrices), and whatever the item count: the pendant lengths and
// their matrices, the edges, every query's best edge so far, and for a chunk of `cols` node columns and `queries` queries the
// table, the caller's mask rows and their packed form, the slab and the result
ScratchPlan place_plan(Shard *e, size_t L, size_t all_queries, size_t cols, size_t queries, size_t segments, bool want_lnl) {
	const size_t D = sizeof(double), N = (size_t)e->N, C = (size_t)e->C, Ppad = ((size_t)e->P + WAVE - 1) / WAVE * WAVE;
	ScratchPlan p = nni_base_plan(e);
	p.add(e->d_nni_mats, 0, D * 3 * N * C * 16);
	p.add(e->d_place_pend_len, 0, D * L);
	p.add(e->d_place_pend, 0, D * L * C * 16);
	p.add(e->d_place_edges, 0, sizeof(PlaceEdge) * N);
	p.add(e->d_place_best_lnl, 0, D * L * all_queries);
	p.add(e->d_place_best_node, 0, sizeof(int32_t) * L * all_queries);
	p.add(e->d_place_table, 0, D * L * cols * Ppad * 16);
	p.add(e->d_place_raw, 0, queries * (size_t)e->P);
	p.add(e->d_place_packed, 0, queries * Ppad);
	p.add(e->d_place_slab, 0, D * segments * L * cols * queries);
	p.add(e->d_place_out, 0, want_lnl ? D * L * cols * queries : 0);
	return p;
}

// whatever the item count: the lengths, their matrices and images, the call's sets and every query's best edge so far; for a chunk
// of `cols` node columns and `queries` queries: the edges, their nodes' own partials, the table, the caller's code rows and their
// packed form, the slab and the result
ScratchPlan place_gen_plan(Shard *e, size_t L, size_t all_queries, size_t cols, size_t queries, size_t segments, size_t Ppad, bool want_lnl) {
	const size_t D = sizeof(double), N = (size_t)e->N, C = (size_t)e->C, M = 2 * N + L, image = MatImage<2, 5>::SIZE;
	ScratchPlan p;
	p.add(e->d_placeg_len, 0, D * M);
	p.add(e->d_placeg_zero, 0, M);
	p.add(e->d_placeg_mats, 0, D * M * C * PLACE_GEN_MATRIX);
	p.add(e->d_placeg_dmats, 0, D * M * C * PLACE_GEN_MATRIX);
	p.add(e->d_placeg_imgs, 0, D * (2 * N * C * image + L * C * PLACE_GEN_CLASS_IMAGE));
	p.add(e->d_placeg_sets, 0, sizeof(unsigned long long) * PLACE_GEN_MAX_SETS);
	p.add(e->d_place_best_lnl, 0, D * L * all_queries);
	p.add(e->d_place_best_node, 0, sizeof(int32_t) * L * all_queries);
	p.add(e->d_placeg_edges, 0, sizeof(PlaceGenEdge) * cols);
	p.add(e->d_placeg_own, 0, D * cols * node_partial_doubles(e));
	p.add(e->d_placeg_owns, 0, sizeof(PlaceGenOwn) * cols);
	p.add(e->d_place_table, 0, D * L * cols * Ppad * PLACE_GEN_CLASSES);
	p.add(e->d_place_raw, 0, queries * (size_t)e->P);
	p.add(e->d_place_packed, 0, queries * Ppad);
	p.add(e->d_place_slab, 0, D * segments * L * cols * queries);
	p.add(e->d_place_out, 0, want_lnl ? D * L * cols * queries : 0);
	return p;
}

constexpr size_t PLACE_MAX_CHUNK_QUERIES = (size_t)1 << 20;
constexpr size_t PLACE_MIN_CHUNK_QUERIES = WAVE;  // queries are cut no further than a wave of lanes while edges can still be cut

// the chunks of the two scoring calls, fits(cols, queries) saying whether such a chunk's scratch fits: all N node columns and all Q
// queries if they fit; else fewer queries, down to a wave of them; else fewer columns; else, with one column, fewer queries still.
// false: not even one query on one column
template <typename Fits>
bool place_chunks(size_t N, size_t Q, Fits fits, size_t *cols_out, size_t *chunk_out) {
	const size_t max_cols = std::min<size_t>(N, BATCH_MAX_CHUNK), max_queries = std::min(Q, PLACE_MAX_CHUNK_QUERIES);
	const size_t min_queries = std::min(max_queries, PLACE_MIN_CHUNK_QUERIES);
	size_t cols = max_cols, chunk = max_queries;
	if (!fits(cols, chunk)) {
		chunk = largest_that(min_queries, max_queries, [&](size_t x) { return fits(max_cols, x); });
		if (chunk >= min_queries) chunk = chunk / min_queries * min_queries;
		else {
			chunk = min_queries;
			cols = largest_that(1, max_cols, [&](size_t x) { return fits(x, min_queries); });
			if (cols < 1) {
				cols = 1;
				chunk = largest_that(1, min_queries, [&](size_t x) { return fits(1, x); });
				if (chunk < 1) return false;
			}
		}
	}
	*cols_out = cols, *chunk_out = chunk;
	return true;
}

// what the two scoring calls differ in beside their tables: the patterns padded to the scoring kernel's block, the kernels that pack
// the caller's rows and gather the table (they share PlaceScoreArgs), and what the scratch of one query on one edge holds
struct PlaceKind {
	int Ppad;
	void (*pack)(int, int, int, const uint8_t *, unsigned long long *);
	void (*score)(PlaceScoreArgs);
	const char *one_holds;
};

// the segments of the padded patterns, which with the pendant lengths are gridDim.z of the scoring kernel
int place_segments(const char *name, int Ppad, size_t L, size_t *segments) {
	*segments = ((size_t)Ppad + REWEIGHT_SEGMENT - 1) / REWEIGHT_SEGMENT;
	if (*segments * L > 65535)
		return fail(PHYAMD_EUNSUPPORTED, "%s: %zu segments of %d patterns x %zu pendant lengths (their product is at most 65535: gridDim.z)", name, *segments, REWEIGHT_SEGMENT, L);
	return PHYAMD_OK;
}

// the node columns and queries of a chunk (place_chunks) whose scratch plan_of(cols, queries) the scratch holds or has room for
template <class PlanOf>
int place_chunk_sizes(Shard *e, const char *name, const PlacementArgs &o, const PlaceKind &kind, const PlanOf &plan_of, size_t *cols, size_t *chunk) {
	const double room = scratch_room(e, (double)batch_scratch_bytes(e), EngineRoom::MayGrow);
	const auto fits = [&](size_t c, size_t q) {
		const ScratchPlan p = plan_of(c, q);
		return p.held(1) || (double)(p.fixed_bytes() + p.item_bytes()) <= room;
	};
	if (place_chunks((size_t)e->N, (size_t)o.queries, fits, cols, chunk)) return PHYAMD_OK;
	const ScratchPlan one = plan_of(1, 1);
	return fail(PHYAMD_EUNSUPPORTED, "%s: the scratch of one query on one edge (%zu bytes: %s) does not fit the memory budget", name, one.fixed_bytes() + one.item_bytes(), kind.one_holds);
}

// Chunk by chunk of `cols` node columns the tables -- tables(first_node, ncols, first_edge, E): those of the chunk's E edges, which
// begin at first_edge of the non-root nodes in node order -- and chunk by chunk of `chunk` queries the gather: the caller's rows
// packed, scored against the tables, the segments added and the best edge kept (k_place_finish), the result copied into
// lnl [L][Q][N]; at the end every query's best edge
template <class Tables>
int run_place_chunks(Shard *e, const PlacementArgs &o, phyamd_placement_profile &prof, const PlaceKind &kind, size_t segments, size_t cols, size_t chunk, const Tables &tables) {
	const int N = e->N, P = e->P, root = e->root, Ppad = kind.Ppad;
	const size_t Q = (size_t)o.queries, L = (size_t)o.lengths;
	const bool want_lnl = o.lnl != nullptr, want_best = o.best_node != nullptr;
	for (size_t first_node = 0; first_node < (size_t)N; first_node += cols) {
		const size_t ncols = std::min(cols, (size_t)N - first_node);
		const bool holds_root = (size_t)root >= first_node && (size_t)root < first_node + ncols;
		const size_t first_edge = first_node <= (size_t)root ? first_node : first_node - 1, E = ncols - (holds_root ? 1 : 0);
		if (int rc = tables(first_node, ncols, first_edge, E)) return rc;
		prof.query_chunks = 0;
		for (size_t first = 0; first < Q; first += chunk) {
			const size_t n = std::min(chunk, Q - first);
			if (E > 0) {
				HIP_TRY(hipMemcpyAsync(e->d_place_raw, o.masks + first * (size_t)P, n * (size_t)P, hipMemcpyHostToDevice, e->stream));
				const int groups = Ppad / 8;
				hipLaunchKernelGGL(kind.pack, dim3((unsigned)(((size_t)groups * n + 255) / 256)), dim3(256), 0, e->stream, (int)n, P, groups, e->d_place_raw.get(), e->d_place_packed.get());
				const unsigned lanes = (unsigned)std::min<size_t>((n + WAVE - 1) / WAVE * WAVE, PLACE_MAX_QUERIES);
				const PlaceScoreArgs sa{e->d_place_table, e->d_place_packed, e->d_place_slab, (int)E, (int)n, Ppad, (int)segments, (int)L};
				hipLaunchKernelGGL(kind.score, dim3((unsigned)((n + lanes - 1) / lanes), (unsigned)((E + PLACE_EDGES - 1) / PLACE_EDGES), (unsigned)(segments * L)), dim3(lanes), 0, e->stream,
				                   sa);
			}
			const PlaceFinishArgs fa{e->d_place_slab, want_lnl ? e->d_place_out.get() : nullptr, want_best ? e->d_place_best_lnl.get() : nullptr, e->d_place_best_node,
			                         (int)E, (int)n, (int)segments, (int)L, (int)ncols, (int)first_node, (int)first_edge, root, (int)first, (int)Q, first_node > 0 ? 1 : 0};
			hipLaunchKernelGGL(k_place_finish, dim3((unsigned)((L * n + 255) / 256)), dim3(256), 0, e->stream, fa);
			HIP_TRY(hipGetLastError());
			for (size_t l = 0; l < L && want_lnl; l++) {  // out [L][n][ncols] into lnl [L][Q][N] at (l, first, first_node)
				double *dst = o.lnl + (l * Q + first) * N + first_node;
				const double *src = e->d_place_out.get() + l * n * ncols;
				if (ncols == (size_t)N) HIP_TRY(hipMemcpyAsync(dst, src, sizeof(double) * n * N, hipMemcpyDeviceToHost, e->stream));
				else HIP_TRY(hipMemcpy2DAsync(dst, sizeof(double) * N, src, sizeof(double) * ncols, sizeof(double) * ncols, n, hipMemcpyDeviceToHost, e->stream));
			}
			HIP_TRY(hipStreamSynchronize(e->stream));  // (the next chunk writes the same arrays; also covers the caller's lists)
			prof.query_chunks++;
		}
		prof.edge_chunks++;
	}
	if (want_best) {
		HIP_TRY(hipMemcpyAsync(o.best_node, e->d_place_best_node, sizeof(int32_t) * L * Q, hipMemcpyDeviceToHost, e->stream));
		if (o.best_lnl) HIP_TRY(hipMemcpyAsync(o.best_lnl, e->d_place_best_lnl, sizeof(double) * L * Q, hipMemcpyDeviceToHost, e->stream));
		HIP_TRY(hipStreamSynchronize(e->stream));
	}
	return PHYAMD_OK;
}

// 4 states: one walk of the engine's tree with every upper parked (two tips: nothing is walked), the split and pendant matrices and
// the edges; a column chunk's tables are k_place_table4's.  Nothing in Shard::state changes
int run_placement(Shard *e, int flags, const PlacementArgs &o, phyamd_placement_profile &prof) {
	static const NniWalkCall call{"phyamd_placement_log_likelihoods", "", "", "the split and pendant matrices are"};
	int rc;
	std::vector<double> lengths;
	if ((rc = check_nni_walk(e, call, flags, nullptr, lengths))) return rc;
	const int T = e->T, N = e->N, C = e->C, P = e->P, root = e->root;
	const size_t Q = (size_t)o.queries, L = (size_t)o.lengths;
	const int nblk = (P + WAVE - 1) / WAVE;
	const PlaceKind kind{nblk * WAVE, k_place_masks, k_place_score4, "every internal node's lower and upper partial, and the edge's table"};
	size_t segments, cols, chunk;
	if ((rc = place_segments(call.name, kind.Ppad, L, &segments))) return rc;
	prof.edges = N - 1;
	for (int n = 0; n < N; n++) {  // d_nni_len [3][N]: sigma t_n | (1 - sigma) t_n | t_n
		lengths[n] = o.split * e->lengths[n];
		lengths[(size_t)N + n] = (1.0 - o.split) * e->lengths[n];
	}
	std::vector<PlaceEdge> edges;  // the non-root nodes in node order: node n is edge n, or n - 1 above the root
	for (int n = 0; n < N; n++) {
		if (n == root) continue;
		const int u = e->sched.parent[n];
		edges.push_back(PlaceEdge{n, u == root ? BATCH_ROOT : u, e->left[u] == n ? e->right[u] : e->left[u], {0, 0, 0, 0, 0}});
	}
	const auto plan_of = [&](size_t c, size_t q) { return place_plan(e, L, Q, c, q, segments, o.lnl != nullptr); };
	if ((rc = place_chunk_sizes(e, call.name, o, kind, plan_of, &cols, &chunk))) return rc;
	const ScratchPlan plan = plan_of(cols, chunk);
	if (T > 2) {
		if ((rc = launch_nni_walk(e, plan, lengths, true))) return rc;
	} else {  // two tips: both edges hang off the root, no partial is read and nothing is walked
		if ((rc = ensure_batch_scratch(e, 1, plan))) return rc;
		HIP_TRY(hipMemcpyAsync(e->d_nni_len, lengths.data(), sizeof(double) * lengths.size(), hipMemcpyHostToDevice, e->stream));
		launch_batch_matrices(e, 1, e->d_lengths, nullptr, e->d_batch_mats);
		launch_batch_matrices(e, 3, e->d_nni_len, nullptr, e->d_nni_mats);
	}
	HIP_TRY(hipMemcpyAsync(e->d_place_pend_len, o.pendant, sizeof(double) * L, hipMemcpyHostToDevice, e->stream));
	hipLaunchKernelGGL(k_batch_matrices, dim3((unsigned)((L * C * 16 + 255) / 256)), dim3(256), 0, e->stream, C, (int)L, 1, e->d_model, e->d_rates, e->d_place_pend_len.get(), -1,
	                   (const int32_t *)nullptr, e->d_place_pend.get());
	HIP_TRY(hipMemcpyAsync(e->d_place_edges, edges.data(), sizeof(PlaceEdge) * edges.size(), hipMemcpyHostToDevice, e->stream));
	HIP_TRY(hipGetLastError());
	return run_place_chunks(e, o, prof, kind, segments, cols, chunk, [&](size_t, size_t, size_t first_edge, size_t E) -> int {
		if (E == 0) return PHYAMD_OK;
		const PlaceTableArgs ta{e->d_place_edges.get() + first_edge, T, N, P, C, nblk, (int)L, e->d_tipmask, e->d_freqs, e->d_props, e->d_weights, e->d_batch_mats, e->d_nni_mats,
		                        e->d_place_pend, e->d_batch_lower, e->d_batch_upper, e->d_place_table};
		hipLaunchKernelGGL(k_place_table4, dim3(nblk, (unsigned)E), dim3(WAVE, C), 0, e->stream, ta);
		return PHYAMD_OK;
	});
}

int shard_placement(Shard *e, int flags, const PlacementArgs &o) {
	CHECK_ENGINE(e);
	phyamd_placement_profile start{};
	start.queries = o.queries, start.lengths = o.lengths;
	return profiled_call(e, &Shard::place_prof, start, [&](phyamd_placement_profile &prof) { return run_placement(e, flags, o, prof); });
}

// 20 states: the engine's resident partials, the lengths sigma t_n | (1 - sigma) t_n | pendant, their matrices and images; a column
// chunk's tables are k_classplace_table's, from the chunk's edge records and its internal nodes' own partials.  Writes only the batch
// scratch beyond the evaluation that made the partials resident
int run_placement_general(Shard *e, int flags, const PlacementGeneralArgs &g, phyamd_placement_profile &prof) {
	static const char *const name = "phyamd_placement_log_likelihoods_general";
	const PlacementArgs &o = g.p;
	int rc;
	const GeneralQueryCall call = general_placement_call(name, "phyamd_placement_log_likelihoods", "the split and pendant matrices are", "tables do");
	if ((rc = check_general_query_inputs(e, call, flags)) || (rc = check_general_query_resident(e, call))) return rc;
	const int T = e->T, N = e->N, C = e->C, P = e->P, root = e->root;
	const size_t Q = (size_t)o.queries, L = (size_t)o.lengths, groups_l = (L + PLACE_GEN_LENGTHS - 1) / PLACE_GEN_LENGTHS;
	const PlaceKind kind{(P + PLACE_GEN_BLOCK - 1) / PLACE_GEN_BLOCK * PLACE_GEN_BLOCK, k_classplace_codes, k_classplace_score,
	                     "the split and pendant matrices and their images, the node's own partial and the edge's table"};
	const int Ppad = kind.Ppad;
	size_t segments, cols, chunk;
	if ((rc = place_segments(name, Ppad, L, &segments))) return rc;
	prof.edges = N - 1;
	const size_t npd = node_partial_doubles(e);
	for (int n = 0; n < N; n++)
		if (n != root && (e->sched.upper_slot[n] < 0 || !e->d_upper)) return fail(PHYAMD_EDEVICE, "%s: node %d has no resident upper partial", name, n);
	const auto plan_of = [&](size_t c, size_t q) { return place_gen_plan(e, L, Q, c, q, segments, (size_t)Ppad, o.lnl != nullptr); };
	if ((rc = place_chunk_sizes(e, name, o, kind, plan_of, &cols, &chunk))) return rc;
	if ((rc = ensure_batch_scratch(e, 1, plan_of(cols, chunk)))) return rc;
	// the lengths, their matrices through the engine's own matrix kernel, and the images
	const size_t M = 2 * (size_t)N + L, image = MatImage<2, 5>::SIZE;
	std::vector<double> lengths(M);
	for (int n = 0; n < N; n++) {
		lengths[n] = o.split * e->lengths[n];
		lengths[(size_t)N + n] = (1.0 - o.split) * e->lengths[n];
	}
	std::copy(o.pendant, o.pendant + L, lengths.begin() + 2 * (size_t)N);
	unsigned long long sets[PLACE_GEN_MAX_SETS] = {};
	for (int q = 0; q < g.set_count; q++) sets[q] = g.sets[q];
	HIP_TRY(hipMemcpyAsync(e->d_placeg_len, lengths.data(), sizeof(double) * M, hipMemcpyHostToDevice, e->stream));
	HIP_TRY(hipMemcpyAsync(e->d_placeg_sets, sets, sizeof sets, hipMemcpyHostToDevice, e->stream));
	HIP_TRY(hipMemsetAsync(e->d_placeg_zero, 0, M, e->stream));
	{
		const size_t total = M * C * PLACE_GEN_MATRIX;
		hipLaunchKernelGGL(k_transition_matrices, dim3((unsigned)std::min<size_t>((total + 255) / 256, 4096)), dim3(256), 0, e->stream, PLACE_GEN_STATES, C, (int)M, e->d_model.get(),
		                   e->d_rates.get(), e->d_placeg_len.get(), e->d_placeg_zero.get(), -1, e->d_placeg_mats.get(), e->d_placeg_dmats.get());
	}
	double *img_lo = e->d_placeg_imgs.get(), *img_hi = img_lo + (size_t)N * C * image, *img_cls = img_hi + (size_t)N * C * image;
	const double *mats_hi = e->d_placeg_mats.get() + (size_t)N * C * PLACE_GEN_MATRIX, *mats_pend = mats_hi + (size_t)N * C * PLACE_GEN_MATRIX;
	build_matrix_images(e, N * C, e->d_placeg_mats, img_lo);
	hipLaunchKernelGGL(k_classplace_transposed_images, dim3((unsigned)(N * C)), dim3(256), 0, e->stream, mats_hi, img_hi);
	hipLaunchKernelGGL(k_classplace_images, dim3((unsigned)(L * C)), dim3(256), 0, e->stream, C, mats_pend, e->d_props.get(), e->d_placeg_sets.get(), (int)g.set_count, img_cls);
	HIP_TRY(hipGetLastError());
	std::vector<PlaceGenEdge> edges;
	std::vector<PlaceGenOwn> owns;
	return run_place_chunks(e, o, prof, kind, segments, cols, chunk, [&](size_t first_node, size_t ncols, size_t, size_t E) -> int {
		edges.clear();
		owns.clear();
		for (size_t col = 0; col < ncols; col++) {  // the chunk's non-root nodes in node order
			const int n = (int)(first_node + col);
			if (n == root) continue;
			PlaceGenEdge ed{e->d_upper + (size_t)e->sched.upper_slot[n] * npd, nullptr, n, {0, 0, 0}};
			if (n >= T) {  // the node's own partial, into this column's temporary
				PlaceGenOwn own;
				if (int rc = place_own_of(e, name, n, e->d_placeg_own.get() + col * npd, &own)) return rc;
				owns.push_back(own);
				ed.own = own.out;
			}
			edges.push_back(ed);
		}
		if (int rc = launch_place_owns(e, owns)) return rc;
		if (E == 0) return PHYAMD_OK;
		HIP_TRY(hipMemcpyAsync(e->d_placeg_edges, edges.data(), sizeof(PlaceGenEdge) * E, hipMemcpyHostToDevice, e->stream));
		const PlaceTableGenArgs ta{e->d_placeg_edges, P, e->Pp, Ppad, C, (int)L, e->upper_fold ? 1 : 0, PLACE_GEN_STATES + 1 + g.set_count, e->d_tipmask, e->d_tipsets,
		                           e->d_freqs, e->d_weights, img_lo, img_hi, img_cls, e->d_place_table};
		hipLaunchKernelGGL(k_classplace_table, dim3((unsigned)(Ppad / PLACE_GEN_BLOCK), (unsigned)E, (unsigned)groups_l), dim3(GenGeo<2>::WAVES * 64), 0, e->stream, ta);
		return PHYAMD_OK;
	});
}

int shard_placement_general(Shard *e, int flags, const PlacementGeneralArgs &g) {
	CHECK_ENGINE(e);
	phyamd_placement_profile start{};
	start.queries = g.p.queries, start.lengths = g.p.lengths;
	return profiled_call(e, &Shard::place_prof, start, [&](phyamd_placement_profile &prof) { return run_placement_general(e, flags, g, prof); });
}

// ---- the three branches around chosen placements, optimised (phyamd_placement_optimize[_general]) --------------------------------

// the NNI walk's (nni_base_plan), and for the `chunk` candidates that run at once -- whatever their edges and queries: as many of
// each as there can be -- the distinct edges and pi o U of each, the distinct queries' mask rows, the candidates, their starts,
// coefficients, results and status words
ScratchPlan qopt_plan(Shard *e, size_t chunk) {
	const size_t D = sizeof(double), C = (size_t)e->C, plane = ((size_t)e->P + WAVE - 1) / WAVE * WAVE * 4;
	const size_t edges = std::min(chunk, (size_t)e->N - 1);
	ScratchPlan p = nni_base_plan(e);
	p.add(e->d_qopt_edges, 0, sizeof(PlaceEdge) * edges);
	p.add(e->d_qopt_fU, 0, D * edges * C * plane);
	p.add(e->d_qopt_masks, 0, chunk * (size_t)e->P);
	p.add(e->d_qopt_cands, 0, sizeof(QoptCand) * chunk);
	p.add(e->d_qopt_start, 0, D * chunk * 3);
	p.add(e->d_qopt_K, 0, D * chunk * C * plane);
	p.add(e->d_qopt_res, 0, D * chunk * 5);
	p.add(e->d_qopt_status, 0, sizeof(int32_t) * chunk * QOPT_STATUS);
	return p;
}

// for the `chunk` candidates that run at once -- whatever their edges and queries: as many of each as there can be -- the call's
// sets, the own partials of the distinct internal edges and what k_classplace_own forms each from, the distinct queries' code rows,
// the candidates, their starts, coefficients, results and status words
ScratchPlan qopt_gen_plan(Shard *e, size_t chunk) {
	const size_t D = sizeof(double), npd = node_partial_doubles(e);
	const size_t owns = std::min(chunk, (size_t)std::max(0, e->T - 2));
	ScratchPlan p;
	p.add(e->d_placeg_sets, 0, sizeof(unsigned long long) * PLACE_GEN_MAX_SETS);
	p.add(e->d_placeg_own, 0, D * owns * npd);
	p.add(e->d_placeg_owns, 0, sizeof(PlaceGenOwn) * owns);
	p.add(e->d_qopt_masks, 0, chunk * (size_t)e->P);
	p.add(e->d_qoptg_cands, 0, sizeof(ClassOptCand) * chunk);
	p.add(e->d_qopt_start, 0, D * chunk * 3);
	p.add(e->d_qopt_K, 0, D * chunk * npd);
	p.add(e->d_qopt_res, 0, D * chunk * 5);
	p.add(e->d_qopt_status, 0, sizeof(int32_t) * chunk * QOPT_STATUS);
	return p;
}

// the root has no branch: no candidate may name it
int check_candidates_off_root(const char *name, const PlacementOptimizeArgs &o, int root) {
	for (size_t i = 0; i < (size_t)o.count; i++)
		if (o.candidates[2 * i + 1] == root)
			return fail(PHYAMD_EINVAL, "%s: candidates[%zu] = (%d, %d): the root (node %d) has no branch to place a query on", name, i, o.candidates[2 * i], root, root);
	return PHYAMD_OK;
}

// the candidates by edge, then query, then position -- a chunk's candidates of one edge read what is formed once per edge -- and the
// distinct edges among them
std::vector<int32_t> sort_candidates(const PlacementOptimizeArgs &o, phyamd_placement_optimize_profile &prof) {
	const size_t count = (size_t)o.count;
	std::vector<int32_t> order(count);
	for (size_t i = 0; i < count; i++) order[i] = (int32_t)i;
	std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
		const int32_t *ca = o.candidates + 2 * (size_t)a, *cb = o.candidates + 2 * (size_t)b;
		return ca[1] != cb[1] ? ca[1] < cb[1] : ca[0] != cb[0] ? ca[0] < cb[0] : a < b;
	});
	prof.edges = 1;
	for (size_t i = 1; i < count; i++) prof.edges += o.candidates[2 * (size_t)order[i] + 1] != o.candidates[2 * (size_t)order[i - 1] + 1];
	return order;
}

// the candidates of a chunk: all (at most gridDim.x's) if the scratch holds as much -- held(plan), each call's own test -- else
// what plan_of(chunk) has room for.  one_holds: what the scratch of one candidate holds
template <class PlanOf, class Held>
int qopt_chunk_size(Shard *e, const char *name, size_t count, const char *one_holds, const PlanOf &plan_of, const Held &held, size_t *chunk) {
	const size_t want = std::min<size_t>(count, BATCH_MAX_CHUNK);
	*chunk = want;
	if (held(plan_of(want))) return PHYAMD_OK;
	const double room = scratch_room(e, (double)batch_scratch_bytes(e), EngineRoom::MayGrow);
	*chunk = largest_that(1, want, [&](size_t x) {
		const ScratchPlan p = plan_of(x);
		return (double)(p.fixed_bytes() + p.item_bytes()) <= room;
	});
	if (*chunk >= 1) return PHYAMD_OK;
	const ScratchPlan one = plan_of(1);
	return fail(PHYAMD_EUNSUPPORTED, "%s: the scratch of one candidate (%zu bytes: %s) does not fit the memory budget", name, one.fixed_bytes() + one.item_bytes(), one_holds);
}

// Chunk by chunk of the sorted candidates (`order`: sort_candidates'): the distinct queries' rows and the starts gathered and
// uploaded, one workgroup per candidate that runs its whole rule, and the results scattered to the candidates' own positions.
// add(i, query_row, node, new_edge) is told candidate i of the chunk (0: a new chunk begins) -- its query's row among the chunk's
// rows, its node, whether the node is another than the candidate's before -- and appends the call's own record of it;
// launch(n) uploads those records and launches the kernels of the chunk's n candidates, which leave out [n][5] in d_qopt_res and
// the status words in d_qopt_status
template <class Add, class Launch>
int run_qopt_chunks(Shard *e, const PlacementOptimizeArgs &o, phyamd_placement_optimize_profile &prof, const std::vector<int32_t> &order, size_t chunk, const Add &add,
                    const Launch &launch) {
	const size_t count = (size_t)o.count, P = (size_t)e->P;
	std::vector<double> start, out;
	std::vector<uint8_t> rows;
	std::vector<int32_t> row_of((size_t)o.queries), status;
	for (size_t first = 0; first < count; first += chunk) {
		const size_t n = std::min(chunk, count - first);
		start.clear(), rows.clear();
		std::fill(row_of.begin(), row_of.end(), -1);
		int last_node = -1;
		for (size_t i = 0; i < n; i++) {
			const size_t at = (size_t)order[first + i];
			const int q = o.candidates[2 * at], node = o.candidates[2 * at + 1];
			if (row_of[q] < 0) {
				row_of[q] = (int32_t)(rows.size() / P);
				rows.insert(rows.end(), o.masks + (size_t)q * P, o.masks + (size_t)(q + 1) * P);
			}
			if (int rc = add(i, row_of[q], node, node != last_node)) return rc;
			last_node = node;
			start.push_back(o.split * e->lengths[node]);
			start.push_back(o.pendant_start ? o.pendant_start[at] : 0.1);
			start.push_back((1.0 - o.split) * e->lengths[node]);
		}
		HIP_TRY(hipMemcpyAsync(e->d_qopt_masks, rows.data(), rows.size(), hipMemcpyHostToDevice, e->stream));
		HIP_TRY(hipMemcpyAsync(e->d_qopt_start, start.data(), sizeof(double) * start.size(), hipMemcpyHostToDevice, e->stream));
		if (int rc = launch(n)) return rc;
		HIP_TRY(hipGetLastError());
		out.resize(n * 5);
		status.resize(n * QOPT_STATUS);
		HIP_TRY(hipMemcpyAsync(out.data(), e->d_qopt_res, sizeof(double) * out.size(), hipMemcpyDeviceToHost, e->stream));
		HIP_TRY(hipMemcpyAsync(status.data(), e->d_qopt_status, sizeof(int32_t) * status.size(), hipMemcpyDeviceToHost, e->stream));
		HIP_TRY(hipStreamSynchronize(e->stream));  // (the next chunk writes the same arrays; also covers the caller's lists)
		for (size_t i = 0; i < n; i++) {
			const size_t to = (size_t)order[first + i];
			const double *v = &out[i * 5];
			std::copy(v, v + 3, o.lengths + to * 3);
			o.lnl[to] = v[3];
			if (o.initial_lnl) o.initial_lnl[to] = v[4];
			if (o.passes) o.passes[to] = status[i * QOPT_STATUS + QOPT_PASSES];
			prof.visits += status[i * QOPT_STATUS + QOPT_VISITS];
			prof.iterations += status[i * QOPT_STATUS + QOPT_ITERATIONS];
		}
		prof.chunks++;
	}
	return PHYAMD_OK;
}

// 4 states: one walk of the engine's tree with every upper parked (two tips: nothing is walked); a chunk's records are its distinct
// edges, of which k_qopt_upper4 forms pi o U, and its candidates.  Nothing in Shard::state changes
int run_placement_optimize(Shard *e, int flags, const PlacementOptimizeArgs &o, phyamd_placement_optimize_profile &prof) {
	static const NniWalkCall call{"phyamd_placement_optimize", "", "", "the likelihood in a branch length is"};
	int rc;
	std::vector<double> lengths;
	if ((rc = check_ready(e))) return fail(rc, "%s: the engine is not ready: %s", call.name, std::string(g_last_error).c_str());
	if ((rc = check_nni_walk(e, call, flags, nullptr, lengths))) return rc;
	const int T = e->T, N = e->N, C = e->C, P = e->P, root = e->root, nblk = (P + WAVE - 1) / WAVE;
	if ((rc = check_candidates_off_root(call.name, o, root))) return rc;
	const std::vector<int32_t> order = sort_candidates(o, prof);
	size_t chunk;
	if ((rc = qopt_chunk_size(
	         e, call.name, (size_t)o.count, "every internal node's lower and upper partial, and two planes", [&](size_t x) { return qopt_plan(e, x); },
	         [&](const ScratchPlan &p) { return batch_items_held(e, p) >= 1; }, &chunk)))
		return rc;
	const ScratchPlan plan = qopt_plan(e, chunk);
	if (T > 2) {
		if ((rc = launch_nni_walk(e, plan, lengths, false))) return rc;
	} else {  // two tips: both edges hang off the root, no partial is read and nothing is walked
		if ((rc = ensure_batch_scratch(e, 1, plan))) return rc;
		launch_batch_matrices(e, 1, e->d_lengths, nullptr, e->d_batch_mats);
	}
	HIP_TRY(hipGetLastError());
	std::vector<PlaceEdge> edges;
	std::vector<QoptCand> cands;
	return run_qopt_chunks(
	    e, o, prof, order, chunk,
	    [&](size_t i, int32_t row, int node, bool new_edge) -> int {
		    if (i == 0) edges.clear(), cands.clear();
		    if (new_edge) {
			    const int u = e->sched.parent[node];
			    edges.push_back(PlaceEdge{node, u == root ? BATCH_ROOT : u, e->left[u] == node ? e->right[u] : e->left[u], {0, 0, 0, 0, 0}});
		    }
		    cands.push_back(QoptCand{node, (int32_t)edges.size() - 1, row, {0, 0, 0, 0, 0}});
		    return PHYAMD_OK;
	    },
	    [&](size_t n) -> int {
		    HIP_TRY(hipMemcpyAsync(e->d_qopt_edges, edges.data(), sizeof(PlaceEdge) * edges.size(), hipMemcpyHostToDevice, e->stream));
		    HIP_TRY(hipMemcpyAsync(e->d_qopt_cands, cands.data(), sizeof(QoptCand) * n, hipMemcpyHostToDevice, e->stream));
		    const QoptUpperArgs ua{e->d_qopt_edges, T, N, P, C, nblk, e->d_tipmask, e->d_freqs, e->d_batch_mats, e->d_batch_lower, e->d_batch_upper, e->d_qopt_fU};
		    hipLaunchKernelGGL(k_qopt_upper4, dim3(nblk, (unsigned)edges.size()), dim3(WAVE, C), 0, e->stream, ua);
		    QoptSolveArgs s{};
		    s.cands = e->d_qopt_cands, s.T = T, s.P = P, s.C = C, s.nblk = nblk, s.branches = o.branches, s.max_iterations = o.max_iterations, s.max_passes = o.max_passes;
		    s.lower = o.lower, s.upper = o.upper, s.tolerance = o.tolerance, s.lnl_tolerance = o.lnl_tolerance;
		    s.tipmask = e->d_tipmask, s.masks = e->d_qopt_masks, s.props = e->d_props, s.model = e->d_model, s.rates = e->d_rates, s.weights = e->d_weights;
		    s.start = e->d_qopt_start, s.lower_all = e->d_batch_lower, s.fU = e->d_qopt_fU, s.K = e->d_qopt_K, s.out = e->d_qopt_res, s.status = e->d_qopt_status;
		    hipLaunchKernelGGL(k_qopt_solve4, dim3((unsigned)n), dim3(CBOPT_THREADS), 0, e->stream, s);
		    return PHYAMD_OK;
	    });
}

int shard_placement_optimize(Shard *e, int flags, const PlacementOptimizeArgs &o) {
	CHECK_ENGINE(e);
	phyamd_placement_optimize_profile start{};
	start.candidates = o.count;
	return profiled_call(e, &Shard::qopt_prof, start, [&](phyamd_placement_optimize_profile &prof) { return run_placement_optimize(e, flags, o, prof); });
}

// 20 states: the engine's resident partials and the call's sets; a chunk's records are the own partials of its distinct internal
// edges (place_own_of) and its candidates.  Writes only the batch scratch beyond the evaluation that made the partials resident
int run_placement_optimize_general(Shard *e, int flags, const PlacementOptimizeGeneralArgs &g, phyamd_placement_optimize_profile &prof) {
	static const char *const name = "phyamd_placement_optimize_general";
	const PlacementOptimizeArgs &o = g.p;
	int rc;
	const GeneralQueryCall call = general_placement_call(name, "phyamd_placement_optimize", "the likelihood in a branch length is", "solve does");
	if ((rc = check_general_query_inputs(e, call, flags))) return rc;
	if ((rc = check_candidates_off_root(name, o, e->root))) return rc;
	if ((rc = check_general_query_resident(e, call))) return rc;
	const int T = e->T, C = e->C, P = e->P;
	const size_t npd = node_partial_doubles(e);
	const std::vector<int32_t> order = sort_candidates(o, prof);
	for (size_t i = 0; i < (size_t)o.count; i++) {
		const int n = o.candidates[2 * i + 1];
		if (e->sched.upper_slot[n] < 0 || !e->d_upper) return fail(PHYAMD_EDEVICE, "%s: node %d has no resident upper partial", name, n);
	}
	size_t chunk;
	if ((rc = qopt_chunk_size(
	         e, name, (size_t)o.count, "its node's own partial and its coefficients, a node's partial each", [&](size_t x) { return qopt_gen_plan(e, x); },
	         [](const ScratchPlan &p) { return p.held(1); }, &chunk)))
		return rc;
	if ((rc = ensure_batch_scratch(e, 1, qopt_gen_plan(e, chunk)))) return rc;
	unsigned long long sets[PLACE_GEN_MAX_SETS] = {};
	for (int q = 0; q < g.set_count; q++) sets[q] = g.sets[q];
	HIP_TRY(hipMemcpyAsync(e->d_placeg_sets, sets, sizeof sets, hipMemcpyHostToDevice, e->stream));
	std::vector<PlaceGenOwn> owns;
	std::vector<ClassOptCand> cands;
	const double *own_of_last = nullptr;
	return run_qopt_chunks(
	    e, o, prof, order, chunk,
	    [&](size_t i, int32_t row, int node, bool new_edge) -> int {
		    if (i == 0) owns.clear(), cands.clear();
		    if (new_edge) {
			    own_of_last = nullptr;
			    if (node >= T) {  // the node's own partial, into this edge's temporary
				    PlaceGenOwn own;
				    if (int rc = place_own_of(e, name, node, e->d_placeg_own.get() + owns.size() * npd, &own)) return rc;
				    owns.push_back(own);
				    own_of_last = own.out;
			    }
		    }
		    cands.push_back(ClassOptCand{e->d_upper + (size_t)e->sched.upper_slot[node] * npd, own_of_last, node, row});
		    return PHYAMD_OK;
	    },
	    [&](size_t n) -> int {
		    if (int rc = launch_place_owns(e, owns)) return rc;
		    HIP_TRY(hipMemcpyAsync(e->d_qoptg_cands, cands.data(), sizeof(ClassOptCand) * n, hipMemcpyHostToDevice, e->stream));
		    ClassOptArgs s{};
		    s.cands = e->d_qoptg_cands, s.P = P, s.Pp = e->Pp, s.C = C, s.fold = e->upper_fold ? 1 : 0, s.set_count = g.set_count;
		    s.branches = o.branches, s.max_iterations = o.max_iterations, s.max_passes = o.max_passes;
		    s.lower = o.lower, s.upper = o.upper, s.tolerance = o.tolerance, s.lnl_tolerance = o.lnl_tolerance;
		    s.tipcode = e->d_tipmask, s.tipsets = e->d_tipsets, s.sets = e->d_placeg_sets, s.codes = e->d_qopt_masks;
		    s.freqs = e->d_freqs, s.props = e->d_props, s.model = e->d_model, s.rates = e->d_rates, s.weights = e->d_weights;
		    s.start = e->d_qopt_start, s.K = e->d_qopt_K, s.out = e->d_qopt_res, s.status = e->d_qopt_status;
		    hipLaunchKernelGGL(k_classopt_solve, dim3((unsigned)n), dim3(CLASSOPT_THREADS), 0, e->stream, s);
		    return PHYAMD_OK;
	    });
}

int shard_placement_optimize_general(Shard *e, int flags, const PlacementOptimizeGeneralArgs &g) {
	CHECK_ENGINE(e);
	phyamd_placement_optimize_profile start{};
	start.candidates = g.p.count;
	return profiled_call(e, &Shard::qopt_prof, start, [&](phyamd_placement_optimize_profile &prof) { return run_placement_optimize_general(e, flags, g, prof); });
}
