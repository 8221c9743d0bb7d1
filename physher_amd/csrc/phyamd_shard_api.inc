// phyamd_shard_api.inc -- the per-device half of every C-ABI entry point (phyamd_abi.inc fans calls out over the shards)
// (part of phyamd_engine.hip: one translation unit, internal linkage)

// ---- pattern tiling (cfg.max_device_bytes; SURVEY 8d "memory feasibility") -------------------------------------------
// Working set of one tile of p patterns.  Before the tree is known (phyamd_create) an estimate for a random tree: 4 states --
// about half of the internal nodes' partials are stored (fringe / DEEP nodes are not), plus parked uppers; 20 / 60 / 61 states
// -- every internal node's lower partial and the level schedule's uppers.  With a schedule (phyamd_set_topology) the real
// counts: stored nodes, the upper slots either schedule may ask for, scale factors, the generic kernels' scratch, the
// gradient slabs.  (A ladder-like tree stores twice what a random one does.)  A 4-state engine that may rescale also holds the
// streamed walks' power-of-two exponents: one int per (stored lower or upper slot, category, pattern), plus the root's per
// category and per pattern (d_lexp, d_uexp, d_Ec, d_Eroot; ensure_exponent_storage).
// the counts of the schedule the tiles must hold (ScheduleCounts: the current one's, or those of the schedule a lazy switch builds)
ScheduleCounts schedule_counts(const Shard *e) {
	ScheduleCounts c{e->core_count, std::max(e->upper_slots, e->walk_upper_slots), 1};
	for (size_t i = 0; i + 1 < e->lower_level_off.size(); i++) c.widest = std::max(c.widest, e->lower_level_off[i + 1] - e->lower_level_off[i]);
	for (size_t i = 0; i + 1 < e->upper_level_off.size(); i++) c.widest = std::max(c.widest, e->upper_level_off[i + 1] - e->upper_level_off[i]);
	return c;
}

double tile_working_set(const Shard *e, double p, bool exact, const ScheduleCounts &k) {
	const double pp = e->S == 4 ? p : std::ceil(p / 16.0) * 16.0, npd = (double)e->C * e->S * pp;
	const double per_pattern = (double)e->T * p + 8.0 * p * (3.0 + (e->S == 4 ? 0.0 : (double)e->C));
	const bool may_scale = e->cfg.rescale != PHYAMD_RESCALE_NEVER, exponents = may_scale && e->S == 4 && e->exp2_on;
	if (!exact) return 8.0 * (exponents ? 1.125 : 1.0) * ((e->S == 4 ? 0.5 : 1.6) * (double)(e->N - e->T) * npd + 2.0 * npd) + per_pattern;
	double doubles = (double)(std::max(1, k.core_count) + std::max(1, k.upper_slots)) * npd;
	if (may_scale) doubles += (double)std::max(1, k.core_count) * p + (e->S == 4 ? 0.0 : 5.0 * k.widest * e->C * p);
	if (exponents) doubles += 0.5 * ((double)(std::max(1, k.core_count) + std::max(1, k.upper_slots) + 1) * e->C * p + p);
	if (e->S == 4) doubles += (double)e->C * p;  // the streamed post-order walk's per-category root terms (d_Lc)
	doubles += (double)e->N * e->C * (p / (WAVE * std::max(1, 4 / e->C)) + 1.0);  // gradient slabs, one entry per wave group
	if (e->S == 4) doubles += 2.0 * e->N * (p / (WAVE * PPT_UPPER) + 19.0) + 0.5 * p / 64.0;  // the Hessian diagonal's slab and its table
	return 8.0 * doubles + per_pattern;
}

// the larger of the working sets of the current schedule and, if a lazy switch may still replace it, of the rescaled one
double tile_working_set(const Shard *e, double p, bool exact) {
	const double now = tile_working_set(e, p, exact, schedule_counts(e));
	return e->have_scaled_counts ? std::max(now, tile_working_set(e, p, exact, e->scaled_counts)) : now;
}

// buffers the 4-state walks make on demand whose size does not follow the tile (whether or not the engine may rescale): the streamed walks' table blocks ([C][ops], ops < N)
// and the pre-order walk's per-op scratch (d_oct: 8 C R doubles, R < N).  What is held already counts in device_bytes.
double walk_reserve(const Shard *e) {
	if (e->S != 4) return 0.0;
	return std::max(0.0, (double)e->N * e->C * OPBLK_BYTES - (double)e->d_optab.size()) + std::max(0.0, 8.0 * (8.0 * e->C * e->N - (double)e->d_oct.size()));
}

// tiles / patterns per tile for the cap (the caller's max_device_bytes, else most of what the device has free right now, so that
// a problem larger than the card runs in tiles instead of failing to allocate)
int choose_tiles(Shard *e, bool exact) {
	double cap = (double)e->cfg.max_device_bytes;
	const bool automatic = e->cfg.max_device_bytes <= 0;
	// what this engine holds now in buffers sized by the tile (they are dropped and re-made if the tile size changes), as ever without
	// the Hessian slab and the mask words, and a one-category engine's d_inv_part (evaluations make them)
	const double tile_sized = (double)(e->tile_mem.bytes - (int64_t)(e->d_hess.bytes() + e->d_hess_tab.bytes() + e->d_mstream.bytes() +
	                                                                   (e->C < 2 ? e->d_inv_part.bytes() : 0)));
	if (automatic) {
		size_t free_bytes = 0, total_bytes = 0;
		cap = hipMemGetInfo(&free_bytes, &total_bytes) == hipSuccess ? 0.92 * ((double)free_bytes + tile_sized) : 0.0;
	} else
		cap -= (double)e->mem.bytes - tile_sized + 65536.0 + walk_reserve(e);  // resident whatever the tile size, and buffers made on demand
	if (!automatic && cap <= 0)
		return fail(PHYAMD_ENOMEM, "max_device_bytes (%lld) does not even hold what is resident whatever the tile size (%lld bytes)",
		            (long long)e->cfg.max_device_bytes, (long long)(e->mem.bytes - (int64_t)tile_sized));
	e->P = e->Ptot;
	e->tiles = 1;
	if (cap > 0 && tile_working_set(e, (double)e->Ptot, exact) > cap) {
		const double resident = (double)e->T * e->Ptot + 16.0 * e->Ptot;
		int tiles = 2, per = 0;
		for (;; tiles++) {
			per = ((e->Ptot + tiles - 1) / tiles + 255) / 256 * 256;
			if (tile_working_set(e, (double)per, exact) + resident <= cap) break;
			if (per <= 256)
				return fail(PHYAMD_ENOMEM, "%s (%.3g bytes) is below the smallest tiled working set (%.3g bytes)",
				            automatic ? "free device memory" : "max_device_bytes", cap, tile_working_set(e, 256.0, exact) + resident);
		}
		e->P = per;
		e->tiles = (e->Ptot + per - 1) / per;
	}
	return PHYAMD_OK;
}

// launch geometry and every allocation whose size follows the tile size e->P (the partial arrays themselves are sized by the
// schedule: ensure_lower_storage / ensure_upper_storage)
int allocate_pattern_storage(Shard *e) {
	e->G = std::max(1, 4 / e->C);  // at least 4 waves per workgroup
	e->nblk = (e->P + WAVE * e->G * PPT_UPPER - 1) / (WAVE * e->G * PPT_UPPER);        // pre-order kernel / gradient slabs
	e->nblk_lower = (e->P + WAVE * e->G * PPT_LOWER - 1) / (WAVE * e->G * PPT_LOWER);  // post-order kernel / lnL slab
	{
		// Tree-walk geometry.  The pre-order walk always takes one pattern per thread (see k_upper4_walk); the plain post-order walk
		// one or two, chosen per launch by shard size (launch_lower_walk), the rescaled one one.
		const int groups = (e->P + WAVE * e->G - 1) / (WAVE * e->G);  // workgroups at one pattern per thread
		e->lower_walk_slots[0] = e->lower_walk_slots[1] = 0;
		e->nblk_walk = groups;
		e->nblk_walk_upper = groups;
	}
	if (e->generic) {
		e->Pp = (e->P + 15) / 16 * 16;
		const int ppb = e->S == 20 ? GenGeo<2>::MIN_PATTERNS_PER_BLOCK : GenGeo<4>::MIN_PATTERNS_PER_BLOCK;  // the finest grid a level may take
		e->nblk = (e->P + ppb - 1) / ppb;
		e->nblk_lower = e->nblk;
		e->nblk_root = (e->P + 255) / 256;
	}
	int rc;
	if ((rc = e->d_tipmask.ensure((size_t)e->T * e->P + 8))) return rc;  // (+8: the matrix-core walk reads a lane's four mask bytes as one dword)
	if (e->tiles > 1) {
		if ((rc = e->d_tip_all.ensure((size_t)e->T * e->Ptot)) || (rc = e->d_weights_all.ensure(e->Ptot)) || (rc = e->d_plk_all.ensure(e->Ptot)) ||
		    (rc = e->d_total.ensure((size_t)1 + e->N * e->C + 2 * PHYAMD_MAX_PARAMETERS)))
			return rc;
	}
	if ((rc = e->d_weights.ensure(e->P)) || (rc = e->d_plk.ensure(e->P)) || (rc = e->d_wl.ensure(e->P))) return rc;
	if ((rc = e->d_lnl_part.ensure(std::max(std::max(std::max(e->nblk, e->nblk_lower), (e->nblk_walk_upper + 2) * e->G), e->nblk_root))))  // (walk: one entry per 64 patterns)
		return rc;
	if (e->generic && (rc = e->d_Lc.ensure((size_t)e->C * e->P))) return rc;
	if (e->C >= 2 && (rc = e->d_inv_part.ensure((size_t)(e->P + 255) / 256 + 1))) return rc;  // (the +I root term: held like the lnL slab)
	e->gpart_row = (size_t)std::max(e->nblk, e->generic ? 0 : e->nblk_walk_upper * e->G);  // the tree-walk kernels write one entry per wave-group
	if ((rc = e->d_gpart.ensure((size_t)e->N * e->C * e->gpart_row))) return rc;
	HIP_TRY(hipMemsetAsync(e->d_gpart, 0, sizeof(double) * (size_t)e->N * e->C * e->gpart_row, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream));
	return PHYAMD_OK;
}

// before any tip data or weights have been loaded: drop everything sized by the tile (phyamd_set_topology re-tiles)
void free_pattern_storage(Shard *e) {
	e->tile_mem.release_all();
	e->batch_mem.release_all();
	e->d_gslab = nullptr;
	e->hess_P = -1;
	e->mstream_epoch = 0;
}

void shard_destroy(Shard *e);
int shard_set_eigen(Shard *e, const double *eval, const double *evec, const double *ivec);
int shard_set_frequencies(Shard *e, const double *freqs);
int shard_set_category_rates(Shard *e, const double *rates, const double *proportions);

int shard_create(const phyamd_config *cfg, Shard **out) {
	if (!cfg || !out) return fail(PHYAMD_EINVAL, "null argument");
	*out = nullptr;
	if (cfg->tip_count < 2) return fail(PHYAMD_EINVAL, "tip_count must be >= 2 (got %d)", cfg->tip_count);
	if (cfg->pattern_count < 1) return fail(PHYAMD_EINVAL, "pattern_count must be >= 1 (got %d)", cfg->pattern_count);
	if (cfg->category_count < 1) return fail(PHYAMD_EINVAL, "category_count must be >= 1 (got %d)", cfg->category_count);
	if (cfg->state_count != 4 && cfg->state_count != 20 && cfg->state_count != 60 && cfg->state_count != 61)
		return fail(PHYAMD_EUNSUPPORTED, "state_count %d: kernels are built for 4, 20, 60 and 61 states", cfg->state_count);
	if (cfg->rescale < 0 || cfg->rescale > 2) return fail(PHYAMD_EINVAL, "rescale must be PHYAMD_RESCALE_*");
	if (cfg->category_count > MAX_WAVES)
		return fail(PHYAMD_EUNSUPPORTED, "category_count %d exceeds %d (one wave per category)", cfg->category_count, MAX_WAVES);
	int ndev = 0;
	HIP_TRY(hipGetDeviceCount(&ndev));
	if (ndev == 0) return fail(PHYAMD_EDEVICE, "no HIP device visible");
	Shard *e = new Shard();
	e->cfg = *cfg;
	e->mem.cap = cfg->max_device_bytes;
	e->T = cfg->tip_count;
	e->N = 2 * e->T - 1;
	e->P = e->Ptot = cfg->pattern_count;
	e->S = cfg->state_count;
	e->C = cfg->category_count;
	if (cfg->device >= 0) e->device = cfg->device;
	else if (hipGetDevice(&e->device) != hipSuccess) e->device = 0;
	if (e->device >= ndev) {
		delete e;
		return fail(PHYAMD_EINVAL, "device %d out of range (%d visible)", cfg->device, ndev);
	}
	auto bail = [&](int rc) {
		shard_destroy(e);
		return rc;
	};
	int rc;
	{
		hipError_t err = hipSetDevice(e->device);
		if (err != hipSuccess) return bail(fail(PHYAMD_EDEVICE, "hipSetDevice(%d): %s", e->device, hipGetErrorString(err)));
	}
	if ((rc = choose_tiles(e, false))) return bail(rc);
	if (cfg->stream) e->stream = (hipStream_t)cfg->stream;
	else {
		hipError_t err = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking);
		if (err != hipSuccess) return bail(fail(PHYAMD_EDEVICE, "hipStreamCreate: %s", hipGetErrorString(err)));
		e->own_stream = true;
	}
	e->scaling_on = cfg->rescale == PHYAMD_RESCALE_ALWAYS;
	if (const char *env = std::getenv("PHYAMD_FUSE")) e->fusion_enabled = std::atoi(env) != 0;  // A/B switch for the fringe fusion
	if (const char *env = std::getenv("PHYAMD_WALK")) e->walk_enabled = std::atoi(env) != 0;
	if (const char *env = std::getenv("PHYAMD_GEN_FUSION")) e->generic_fusion = std::atoi(env) != 0;
	if (const char *env = std::getenv("PHYAMD_XCD_MAP")) e->xcd_map = std::atoi(env) != 0;
	if (const char *env = std::getenv("PHYAMD_SCALE_EXP2")) e->exp2_on = std::atoi(env) != 0;
	if (const char *env = std::getenv("PHYAMD_STREAM_TFORM")) e->tform_on = std::atoi(env) != 0;
	if (const char *env = std::getenv("PHYAMD_LOWER_PARK2")) e->lower_park2_on = std::atoi(env) != 0;
	e->generic = e->S != 4;
	e->tip_set.assign(e->T, 0);
	e->tip_empty.assign(e->T, 0);
	e->mem.spare = &e->batch_mem;
	e->batch_max_patterns = BATCH_MAX_PATTERNS;
	if (const char *env = std::getenv("PHYAMD_BATCH_MAX_PATTERNS")) e->batch_max_patterns = std::atoi(env);
	if (const char *env = std::getenv("PHYAMD_BATCH_TRACE")) e->batch_trace = std::atoi(env) != 0;
	e->explicit_host.assign(e->N, 0);
	const size_t msz = (size_t)e->N * e->C * e->S * e->S;
	if (e->generic && ((rc = e->d_tipsets.ensure(256)) || (rc = e->d_imgs.ensure(((size_t)e->N * e->C + 2) * gen_image_doubles(e))))) return bail(rc);
	if (e->S == 20 && GenFuse<2>::QP) {  // Qf P(t) per (tip, category) and its images (ensure_tip_rate_products): made here, so that the tile plan counts them
		if ((rc = e->d_qp_mats.ensure((size_t)e->T * e->C * e->S * e->S)) || (rc = e->d_qp_imgs.ensure((size_t)e->T * e->C * gen_image_doubles(e)))) return bail(rc);
	}
	// d_lower is sized by the schedule (stored "core" nodes only): ensure_lower_storage
	if ((rc = e->d_mats.ensure(msz)) || (rc = e->d_dmats.ensure(msz)) || (rc = e->d_model.ensure((size_t)e->S + 2 * e->S * e->S)) ||
	    (rc = e->d_Q.ensure((size_t)e->S * e->S)))
		return bail(rc);
	if (!e->generic && (rc = e->d_tiptab.ensure((size_t)e->T * e->C * 64 + (size_t)e->N * 6))) return bail(rc);
	if ((rc = e->d_freqs.ensure(e->S)) || (rc = e->d_rates.ensure(e->C)) || (rc = e->d_props.ensure(e->C)) || (rc = e->d_lengths.ensure(e->N)) ||
	    (rc = e->d_result.ensure((size_t)1 + e->N * e->C + 2 * PHYAMD_MAX_PARAMETERS)) || (rc = e->d_explicit.ensure(e->N)) ||
	    (rc = e->d_row_valid.ensure((size_t)e->N * e->C)))
		return bail(rc);
	{
		hipError_t err = hipHostMalloc(reinterpret_cast<void **>(&e->h_result), sizeof(double) * ((size_t)2 + e->N * e->C + 2 * PHYAMD_MAX_PARAMETERS), hipHostMallocDefault);  // (+1: the lazy-switch copy)
		if (err != hipSuccess) return bail(fail(PHYAMD_EDEVICE, "hipHostMalloc: %s", hipGetErrorString(err)));
		err = hipMemsetAsync(e->d_explicit, 0, e->N, e->stream);
		if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
		if (err != hipSuccess) return bail(fail(PHYAMD_EDEVICE, "memset: %s", hipGetErrorString(err)));
		for (auto &ev : e->ev) {
			err = hipEventCreate(&ev);
			if (err != hipSuccess) return bail(fail(PHYAMD_EDEVICE, "hipEventCreate: %s", hipGetErrorString(err)));
		}
	}
	if ((rc = allocate_pattern_storage(e))) return bail(rc);
	*out = e;
	return PHYAMD_OK;
}

void shard_destroy(Shard *e) {  // (the device arrays free themselves)
	if (!e) return;
	(void)hipSetDevice(e->device);
	if (e->stream) (void)hipStreamSynchronize(e->stream);
	if (e->h_result) (void)hipHostFree(e->h_result);
	if (e->h_lengths) (void)hipHostFree(e->h_lengths);
	if (e->ev_lengths) (void)hipEventDestroy(e->ev_lengths);
	if (e->ev_check) (void)hipEventDestroy(e->ev_check);
	for (auto &ev : e->ev)
		if (ev) (void)hipEventDestroy(ev);
	if (e->own_stream && e->stream) (void)hipStreamDestroy(e->stream);
	delete e;
}

#define CHECK_ENGINE(e) \
	if (!(e)) return fail(PHYAMD_EINVAL, "null engine")

int shard_set_tip_states(Shard *e, int tip, const uint8_t *states) {
	CHECK_ENGINE(e);
	if (tip < 0 || tip >= e->T || !states) return fail(PHYAMD_EINVAL, "bad tip %d or null states", tip);
	int rc;
	if ((rc = bind_device(e))) return rc;
	std::vector<uint8_t> mask(e->Ptot);
	if (e->generic)
		for (int k = 0; k < e->Ptot; k++) mask[k] = states[k] < e->S ? states[k] : (uint8_t)e->S;  // raw codes; S = unknown
	else
		for (int k = 0; k < e->Ptot; k++) mask[k] = states[k] < 4 ? (uint8_t)(1u << states[k]) : (uint8_t)0xF;  // code >= S: unknown (treelikelihood4.c:946-988)
	HIP_TRY(hipMemcpyAsync(tip_row(e, tip), mask.data(), e->Ptot, hipMemcpyHostToDevice, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream));
	e->tip_set[tip] = 1;
	e->tip_empty[tip] = 0;
	input_changed(e, Input::TipData);
	return PHYAMD_OK;
}

int shard_set_tip_partials(Shard *e, int tip, const double *partials) {
	CHECK_ENGINE(e);
	if (tip < 0 || tip >= e->T || !partials) return fail(PHYAMD_EINVAL, "bad tip %d or null partials", tip);
	int rc;
	if ((rc = bind_device(e))) return rc;
	std::vector<uint8_t> mask(e->Ptot);
	if (e->generic) {  // 0/1 vectors: one state, all states, or a set of states (datatype.c:212-240)
		const int S = e->S;
		for (int k = 0; k < e->Ptot; k++) {
			int ones = 0, last = -1;
			unsigned long long members = 0;
			for (int s = 0; s < S; s++) {
				const double v = partials[(size_t)k * S + s];
				if (v == 1.0) ones++, last = s, members |= 1ull << s;
				else if (v != 0.0) return fail(PHYAMD_EUNSUPPORTED, "tip %d pattern %d: only 0/1 tip partials are built", tip, k);
			}
			if (ones == 1) mask[k] = (uint8_t)last;
			else if (ones == S) mask[k] = (uint8_t)S;
			else {
				size_t q = std::find(e->tipsets_host.begin(), e->tipsets_host.end(), members) - e->tipsets_host.begin();
				if (q == e->tipsets_host.size()) {
					if ((int)q + S + 1 > 255) return fail(PHYAMD_EUNSUPPORTED, "tip %d pattern %d: more than %d distinct ambiguity sets", tip, k, 255 - S);
					e->tipsets_host.push_back(members);  // uploaded below, or by the next call if this one is refused part-way
				}
				mask[k] = (uint8_t)(S + 1 + q);
			}
		}
		if (e->tipsets_uploaded != e->tipsets_host.size()) {
			HIP_TRY(hipMemcpyAsync(e->d_tipsets, e->tipsets_host.data(), e->tipsets_host.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, e->stream));
			e->tipsets_uploaded = e->tipsets_host.size();
		}
	} else {
		for (int k = 0; k < e->Ptot; k++) {
			unsigned m = 0;
			for (int s = 0; s < 4; s++) {
				const double v = partials[(size_t)k * 4 + s];
				if (v == 1.0) m |= 1u << s;
				else if (v != 0.0)
					return fail(PHYAMD_EUNSUPPORTED, "tip %d pattern %d: tip partials other than 0/1 ambiguity masks are not built in this revision", tip, k);
			}
			mask[k] = (uint8_t)m;
		}
		e->tip_empty[tip] = std::find(mask.begin(), mask.end(), (uint8_t)0) != mask.end();
	}
	HIP_TRY(hipMemcpyAsync(tip_row(e, tip), mask.data(), e->Ptot, hipMemcpyHostToDevice, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream));
	e->tip_set[tip] = 1;
	input_changed(e, Input::TipData);
	return PHYAMD_OK;
}

int shard_set_pattern_weights(Shard *e, const double *weights) {
	CHECK_ENGINE(e);
	if (!weights) return fail(PHYAMD_EINVAL, "null weights");
	int rc;
	if ((rc = bind_device(e))) return rc;
	HIP_TRY(hipMemcpyAsync(e->tiles > 1 ? e->d_weights_all : e->d_weights, weights, sizeof(double) * e->Ptot, hipMemcpyHostToDevice, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream));
	e->have_weights = true;
	input_changed(e, Input::PatternWeights);
	return PHYAMD_OK;
}

int shard_set_topology(Shard *e, const int32_t *left, const int32_t *right, int root) {
	CHECK_ENGINE(e);
	if (!left || !right) return fail(PHYAMD_EINVAL, "null topology arrays");
	int rc;
	if ((rc = bind_device(e))) return rc;
	e->batch_mem.release_all();  // (sized by the old tree; the tile plan below counts what the engine itself holds)
	lowers_discarded(e);         // (whichever way this call ends: the schedule is built anew, every partial belongs to the old tree)
	std::vector<int32_t> old_l = e->left, old_r = e->right;
	const int old_root = e->root;
	e->left.assign(left, left + e->N);
	e->right.assign(right, right + e->N);
	e->root = root;
	// every failure from here on leaves the engine on the tree it had (host lists, device op tables) -- or, if that cannot be
	// re-established, without a topology, so that the next evaluation is refused instead of walking half-updated tables
	const bool had_topology = e->have_topology;
	auto roll_back = [&](int code) {
		const std::string why = g_last_error;
		e->left = old_l;
		e->right = old_r;
		e->root = old_root;
		if (had_topology && (build_schedule(e) != PHYAMD_OK || upload_schedule(e) != PHYAMD_OK)) e->have_topology = false;
		g_last_error = why;
		return code;
	};
	if ((rc = build_schedule(e))) return roll_back(rc);
	e->have_scaled_counts = false;
	if (e->generic && e->cfg.rescale == PHYAMD_RESCALE_AUTO && !e->scaling_on) {
		// the lazy switch rebuilds the 20 / 60 / 61-state schedule without fringe fusion or tree walk (more stored nodes and upper
		// slots): the tiles are sized for that schedule too, so that the switch never needs more than the cap
		e->scaling_on = true;
		rc = build_schedule(e);
		if (!rc) e->scaled_counts = schedule_counts(e);
		e->scaling_on = false;
		if (rc || (rc = build_schedule(e))) return roll_back(rc);
		e->have_scaled_counts = true;
	}
	{
		// now that the tree is known the tile size follows its real storage needs (a ladder-like tree stores twice what the
		// estimate of phyamd_create assumed): possible as long as no tip data or weights sit in buffers of the old tile size
		const bool data_loaded = e->have_weights || std::find(e->tip_set.begin(), e->tip_set.end(), (uint8_t)1) != e->tip_set.end();
		const int old_tiles = e->tiles, old_P = e->P;
		if ((rc = choose_tiles(e, true))) {
			e->tiles = old_tiles;
			e->P = old_P;
			return roll_back(rc);
		}
		if (e->tiles != old_tiles || e->P != old_P) {
			const int want_tiles = e->tiles, want_P = e->P;
			e->tiles = old_tiles;
			e->P = old_P;
			if (want_tiles > old_tiles && data_loaded)
				return roll_back(fail(PHYAMD_ENOMEM, "this tree needs %d pattern tiles to stay within the memory cap (the engine was created with %d): "
				                      "call phyamd_set_topology before loading tip data and weights", want_tiles, old_tiles));
			if (!data_loaded) {
				free_pattern_storage(e);
				e->tiles = want_tiles;
				e->P = want_P;
				if ((rc = allocate_pattern_storage(e))) {  // (the pattern buffers are gone: nothing can be evaluated until a later call succeeds)
					e->have_topology = false;
					return rc;
				}
			}
		}
	}
	if ((rc = upload_schedule(e))) return roll_back(rc);
	if ((rc = ensure_lower_storage(e))) return roll_back(rc);
	e->have_topology = true;
	input_changed(e, Input::Topology);
	return PHYAMD_OK;
}

int shard_set_branch_lengths(Shard *e, const double *lengths) {
	CHECK_ENGINE(e);
	if (!lengths) return fail(PHYAMD_EINVAL, "null lengths");
	int rc;
	if ((rc = bind_device(e))) return rc;
	e->lengths.assign(lengths, lengths + e->N);
	if (e->have_topology) e->lengths[e->root] = 0.0;
	// no stream synchronisation per call (one per evaluation in an optimiser's loop): the vector goes through a pinned staging
	// buffer that is only waited for if the previous upload from it is still in flight
	if (!e->h_lengths) {
		HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&e->h_lengths), sizeof(double) * e->N, hipHostMallocDefault));
		HIP_TRY(hipEventCreateWithFlags(&e->ev_lengths, hipEventDisableTiming));
	} else
		HIP_TRY(hipEventSynchronize(e->ev_lengths));
	std::memcpy(e->h_lengths, e->lengths.data(), sizeof(double) * e->N);
	HIP_TRY(hipMemcpyAsync(e->d_lengths, e->h_lengths, sizeof(double) * e->N, hipMemcpyHostToDevice, e->stream));
	HIP_TRY(hipEventRecord(e->ev_lengths, e->stream));
	e->have_lengths = true;
	input_changed(e, Input::BranchLengths);
	return PHYAMD_OK;
}

int shard_set_branch_length(Shard *e, int node, double length) {
	CHECK_ENGINE(e);
	if (!e->have_topology || !e->have_lengths) return fail(PHYAMD_EINVAL, "phyamd_set_topology and phyamd_set_branch_lengths come first");
	if (node < 0 || node >= e->N || node == e->root) return fail(PHYAMD_EINVAL, "node %d has no branch", node);
	int rc;
	if ((rc = bind_device(e))) return rc;
	if (e->lengths[node] == length) return PHYAMD_OK;
	e->lengths[node] = length;
	HIP_TRY(hipMemcpyAsync(e->d_lengths + node, &e->lengths[node], sizeof(double), hipMemcpyHostToDevice, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream));
	input_changed(e, Input::BranchLength, node);
	return PHYAMD_OK;
}

int shard_store(Shard *e) {
	CHECK_ENGINE(e);
	NOT_TILED(e, "phyamd_store");
	int rc;
	if ((rc = bind_device(e))) return rc;
	if ((rc = require_reference_form(e))) return rc;  // (stored partials: the partials themselves, in the reference's form)
	for (uint8_t x : e->explicit_host)
		if (x) return fail(PHYAMD_EUNSUPPORTED, "phyamd_store does not cover explicit node matrices");
	if ((rc = run_lower(e, true))) return rc;  // the state that is stored is an evaluated one (a no-op when nothing is pending)
	if (!e->two_slots) {  // first store: a second slot per stored node (allocate_storage(tlk, 1), treelikelihood.c:977-1003), contents kept
		// the allocation never shrinks (keep_partials on and off again, a new topology with fewer stored nodes): only the
		// core_count live slots move over.  Allocated next to the one-slot arrays, within the cap: if they do not fit, the engine
		// keeps its one-slot state
		const size_t npd = node_partial_doubles(e), want = (size_t)std::max(1, e->core_count) * 2;
		const size_t live = std::min(lower_slots(e), (size_t)std::max(1, e->core_count));
		DeviceArray<double> lower{&e->tile_mem}, lscale{&e->tile_mem};
		if ((rc = lower.ensure(want * npd)) || (e->d_lscale && (rc = lscale.ensure(want * e->P)))) return rc;
		hipError_t err = hipMemcpyAsync(lower, e->d_lower, live * npd * sizeof(double), hipMemcpyDeviceToDevice, e->stream);
		if (err == hipSuccess && e->d_lscale) err = hipMemcpyAsync(lscale, e->d_lscale, live * e->P * sizeof(double), hipMemcpyDeviceToDevice, e->stream);
		if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
		if (err != hipSuccess) {
			(void)hipStreamSynchronize(e->stream);
			return fail(err == hipErrorOutOfMemory ? PHYAMD_ENOMEM : PHYAMD_EDEVICE, "phyamd_store: second slot per stored node: %s", hipGetErrorString(err));
		}
		e->d_lower.swap(lower);
		e->d_lscale.swap(lscale);  // (the one-slot arrays are freed on leaving this scope)
		e->two_slots = true;
	}
	HIP_TRY(hipMemcpyAsync(e->h_result, e->d_result, sizeof(double), hipMemcpyDeviceToHost, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream));
	auto &st = e->stored;
	st.lnl = e->h_result[0];
	st.lengths = e->lengths;
	st.model = e->model;
	st.freqs = e->freqs;
	st.rates = e->rates;
	st.props = e->props;
	st.have_eigen = e->have_eigen;
	st.scaling_on = e->scaling_on;
	st.core_index = e->core_index;
	st.epoch = e->schedule_epoch;
	state_stored(e);
	return PHYAMD_OK;
}

int shard_restore(Shard *e) {
	CHECK_ENGINE(e);
	if (!e->state.stored_valid) return fail(PHYAMD_EINVAL, "nothing is stored (phyamd_store has not been called, or tree / data changed since)");
	int rc;
	if ((rc = bind_device(e))) return rc;
	const Shard::Stored st = e->stored;  // the setters below write the engine's own copies
	const int S = e->S;
	if (st.have_eigen && (rc = shard_set_eigen(e, st.model.data(), st.model.data() + S, st.model.data() + S + S * S))) return rc;
	if ((rc = shard_set_frequencies(e, st.freqs.data()))) return rc;
	if ((rc = shard_set_category_rates(e, st.rates.data(), st.props.data()))) return rc;
	if ((rc = shard_set_branch_lengths(e, st.lengths.data()))) return rc;
	if (st.epoch == e->schedule_epoch && st.scaling_on == e->scaling_on && e->two_slots) {
		// the stored partials are still in their slots: point the nodes back at them (treelikelihood.c:116-124) and
		// re-integrate the root, whose per-pattern outputs belong to the discarded state
		bool moved = false;
		for (int n = e->T; n < e->N; n++)
			if (e->core_index[n] != st.core_index[n]) {
				e->core_index[n] = st.core_index[n];
				moved = true;
			}
		if (moved) {
			refresh_op_cores(e);
			if ((rc = upload_schedule(e))) return rc;
		}
		lowers_restored(e);
	}  // else: slots were reassigned since (schedule rebuilt, rescaling switched on): the restored parameters are recomputed in full
	return PHYAMD_OK;
}

int shard_update_all_nodes(Shard *e) {
	CHECK_ENGINE(e);
	input_changed(e, Input::UpdateAllNodes);
	return PHYAMD_OK;
}

int shard_set_eigen(Shard *e, const double *eval, const double *evec, const double *ivec) {
	CHECK_ENGINE(e);
	if (!eval || !evec || !ivec) return fail(PHYAMD_EINVAL, "null eigen system");
	int rc;
	if ((rc = bind_device(e))) return rc;
	const int S = e->S;
	e->model.resize((size_t)S + 2 * S * S);
	std::copy(eval, eval + S, e->model.begin());
	std::copy(evec, evec + S * S, e->model.begin() + S);
	std::copy(ivec, ivec + S * S, e->model.begin() + S + S * S);
	HIP_TRY(hipMemcpyAsync(e->d_model, e->model.data(), sizeof(double) * e->model.size(), hipMemcpyHostToDevice, e->stream));
	// Q = evec diag(eval) ivec: the gradient kernels use (dP/dt) p = Q (P p)
	std::vector<double> Q((size_t)S * S, 0.0);
	for (int i = 0; i < S; i++)
		for (int j = 0; j < S; j++) {
			double q = 0.0;
			for (int k = 0; k < S; k++) q += evec[i * S + k] * eval[k] * ivec[k * S + j];
			Q[(size_t)i * S + j] = q;
		}
	HIP_TRY(hipMemcpyAsync(e->d_Q, Q.data(), sizeof(double) * Q.size(), hipMemcpyHostToDevice, e->stream));
	e->Q_host = Q;
	e->have_Q = true;
	std::fill(e->explicit_host.begin(), e->explicit_host.end(), 0);
	HIP_TRY(hipMemsetAsync(e->d_explicit, 0, e->N, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream));
	e->have_eigen = true;
	input_changed(e, Input::Eigen);
	return PHYAMD_OK;
}

int shard_set_frequencies(Shard *e, const double *freqs) {
	CHECK_ENGINE(e);
	if (!freqs) return fail(PHYAMD_EINVAL, "null freqs");
	int rc;
	if ((rc = bind_device(e))) return rc;
	e->freqs.assign(freqs, freqs + e->S);
	HIP_TRY(hipMemcpyAsync(e->d_freqs, e->freqs.data(), sizeof(double) * e->S, hipMemcpyHostToDevice, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream));
	e->have_freqs = true;
	input_changed(e, Input::Frequencies);
	return PHYAMD_OK;
}

int shard_set_category_rates(Shard *e, const double *rates, const double *proportions) {
	CHECK_ENGINE(e);
	if (!rates || !proportions) return fail(PHYAMD_EINVAL, "null rates/proportions");
	int rc;
	if ((rc = bind_device(e))) return rc;
	e->rates.assign(rates, rates + e->C);
	e->props.assign(proportions, proportions + e->C);
	HIP_TRY(hipMemcpyAsync(e->d_rates, e->rates.data(), sizeof(double) * e->C, hipMemcpyHostToDevice, e->stream));
	HIP_TRY(hipMemcpyAsync(e->d_props, e->props.data(), sizeof(double) * e->C, hipMemcpyHostToDevice, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream));
	e->have_rates = true;
	input_changed(e, Input::CategoryRates);
	return PHYAMD_OK;
}

int shard_set_node_matrices(Shard *e, int node, const double *matrices) {
	CHECK_ENGINE(e);
	if (node < 0 || node >= e->N || !matrices) return fail(PHYAMD_EINVAL, "bad node %d or null matrices", node);
	int rc;
	if ((rc = bind_device(e))) return rc;
	const size_t sz = (size_t)e->C * e->S * e->S;
	HIP_TRY(hipMemcpyAsync(e->d_mats + (size_t)node * sz, matrices, sizeof(double) * sz, hipMemcpyHostToDevice, e->stream));
	e->explicit_host[node] = 1;
	HIP_TRY(hipMemcpyAsync(e->d_explicit + node, &e->explicit_host[node], 1, hipMemcpyHostToDevice, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream));
	input_changed(e, Input::NodeMatrices, e->have_topology && node != e->root ? node : -1);  // like a branch-length change of this one node
	return PHYAMD_OK;
}

int shard_set_matrices(Shard *e, const double *matrices) {
	CHECK_ENGINE(e);
	if (!matrices) return fail(PHYAMD_EINVAL, "null matrices");
	int rc;
	if ((rc = bind_device(e))) return rc;
	const size_t sz = (size_t)e->N * e->C * e->S * e->S;
	HIP_TRY(hipMemcpyAsync(e->d_mats, matrices, sizeof(double) * sz, hipMemcpyHostToDevice, e->stream));
	std::fill(e->explicit_host.begin(), e->explicit_host.end(), 1);
	HIP_TRY(hipMemsetAsync(e->d_explicit, 1, e->N, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream));
	input_changed(e, Input::Matrices);
	return PHYAMD_OK;
}

int shard_set_rate_matrix(Shard *e, const double *Q) {
	CHECK_ENGINE(e);
	if (!Q) return fail(PHYAMD_EINVAL, "null Q");
	int rc;
	if ((rc = bind_device(e))) return rc;
	HIP_TRY(hipMemcpyAsync(e->d_Q, Q, sizeof(double) * e->S * e->S, hipMemcpyHostToDevice, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream));
	e->Q_host.assign(Q, Q + (size_t)e->S * e->S);
	e->have_Q = true;
	input_changed(e, Input::RateMatrix);
	return PHYAMD_OK;
}

int shard_log_likelihood(Shard *e, double *lnl) {
	CHECK_ENGINE(e);
	if (!lnl) return fail(PHYAMD_EINVAL, "null lnl");
	int rc;
	if ((rc = eval_lower(e))) return rc;
	HIP_TRY(hipMemcpyAsync(e->h_result, e->d_result, sizeof(double), hipMemcpyDeviceToHost, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream));
	finish_profile(e, false);
	*lnl = e->h_result[0];
	return PHYAMD_OK;
}

int shard_log_likelihood_device(Shard *e, double *device_out) {
	CHECK_ENGINE(e);
	if (!device_out) return fail(PHYAMD_EINVAL, "null device_out");
	int rc;
	if ((rc = eval_lower(e))) return rc;
	HIP_TRY(hipMemcpyAsync(device_out, e->d_result, sizeof(double), hipMemcpyDeviceToDevice, e->stream));
	return PHYAMD_OK;
}

int shard_gradient_device(Shard *e, int flags, double *device_out) {
	CHECK_ENGINE(e);
	if (!device_out) return fail(PHYAMD_EINVAL, "null device_out");
	int rc;
	if ((rc = eval_gradient(e, flags))) return rc;
	HIP_TRY(hipMemcpyAsync(device_out, e->d_result, sizeof(double) * ((size_t)1 + e->N * e->C), hipMemcpyDeviceToDevice, e->stream));
	return PHYAMD_OK;
}

int shard_gradient(Shard *e, int flags, double *lnl, double *cat_gradient) {
	CHECK_ENGINE(e);
	if (!cat_gradient) return fail(PHYAMD_EINVAL, "null cat_gradient");
	int rc;
	if ((rc = eval_gradient(e, flags))) return rc;
	const size_t n = (size_t)1 + e->N * e->C;
	HIP_TRY(hipMemcpyAsync(e->h_result, e->d_result, sizeof(double) * n, hipMemcpyDeviceToHost, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream));
	finish_profile(e, true);
	const double l = e->h_result[0];
	if (lnl) *lnl = l;
	if (std::isnan(l) || std::isinf(l)) {  // treelikelihood.c:327-332
		for (size_t i = 0; i < n - 1; i++) cat_gradient[i] = NAN;
	} else
		std::memcpy(cat_gradient, e->h_result + 1, sizeof(double) * (n - 1));
	return PHYAMD_OK;
}

int shard_branch_gradient(Shard *e, int flags, const double *rates_without_mu, double *lnl, double *branch_gradient) {
	CHECK_ENGINE(e);
	if (!branch_gradient) return fail(PHYAMD_EINVAL, "null branch_gradient");
	std::vector<double> cg((size_t)e->N * e->C);
	int rc;
	if ((rc = shard_gradient(e, flags, lnl, cg.data()))) return rc;
	const double *r = rates_without_mu ? rates_without_mu : e->rates.data();
	for (int n = 0; n < e->N; n++) {  // gradient_branch_length_from_cat_inplace, treelikelihood.c:3129-3143
		if (e->C == 1) {
			branch_gradient[n] = cg[n];  // catCount == 1: no rate/weight factor (treelikelihood.c:3258-3266)
			continue;
		}
		double g = cg[(size_t)n * e->C] * e->props[0] * r[0];
		for (int c = 1; c < e->C; c++) g += cg[(size_t)n * e->C + c] * e->props[c] * r[c];
		branch_gradient[n] = g;
	}
	return PHYAMD_OK;
}

int shard_set_rate_matrix_derivatives(Shard *e, int count, const double *dQ) {
	CHECK_ENGINE(e);
	if (count < 0 || count > PHYAMD_MAX_PARAMETERS) return fail(PHYAMD_EINVAL, "count %d outside 0..%d", count, PHYAMD_MAX_PARAMETERS);
	if (count > 0 && !dQ) return fail(PHYAMD_EINVAL, "null dQ");
	e->np = count;
	e->dQ_host.assign(dQ, dQ + (size_t)count * e->S * e->S);
	input_changed(e, Input::RateMatrixDerivatives);
	return PHYAMD_OK;
}

int shard_parameter_gradient(Shard *e, int flags, double *lnl, double *cat_gradient, double *parameter_gradient) {
	CHECK_ENGINE(e);
	if (!parameter_gradient) return fail(PHYAMD_EINVAL, "null parameter_gradient");
	int rc;
	if ((rc = eval_gradient(e, flags, true))) return rc;
	const size_t ncat = (size_t)e->N * e->C, n = 1 + ncat + e->np;
	HIP_TRY(hipMemcpyAsync(e->h_result, e->d_result, sizeof(double) * n, hipMemcpyDeviceToHost, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream));
	finish_profile(e, true);
	const double l = e->h_result[0];
	if (lnl) *lnl = l;
	const bool bad = std::isnan(l) || std::isinf(l);  // treelikelihood.c:327-332
	for (size_t i = 0; cat_gradient && i < ncat; i++) cat_gradient[i] = bad ? NAN : e->h_result[1 + i];
	for (int i = 0; i < e->np; i++) parameter_gradient[i] = bad ? NAN : e->h_result[1 + ncat + i];
	return PHYAMD_OK;
}

int shard_parameter_gradient_device(Shard *e, int flags, double *device_out) {
	CHECK_ENGINE(e);
	if (!device_out) return fail(PHYAMD_EINVAL, "null device_out");
	int rc;
	if ((rc = eval_gradient(e, flags, true))) return rc;
	HIP_TRY(hipMemcpyAsync(device_out, e->d_result, sizeof(double) * ((size_t)1 + e->N * e->C + e->np + e->S), hipMemcpyDeviceToDevice, e->stream));
	return PHYAMD_OK;
}

// ---- every branch's first and second derivative at once (phyamd_branch_hessian_diagonal) ----
// what the single-branch evaluation would return as d1, d2 for every node at its current length: the level pre-order pass in its
// HESS form (k_upper4), which forms r_c Q P p and r_c^2 Q Q P p against the upper partial it builds anyway
int hessian_ready(Shard *e, int flags) {
	if (flags != 0) return fail(PHYAMD_EINVAL, "phyamd_branch_hessian_diagonal: flags %d (no flags are defined: pass 0)", flags);
	if (!e->have_eigen) return fail(PHYAMD_EINVAL, "the Hessian diagonal needs the eigen system (phyamd_set_eigen)");
	// The pass differentiates the matrices it multiplies with: Q P and Q Q P are the derivatives of P = exp(Q t r) only.  The
	// single-branch call rebuilds P from the eigen system and ignores an explicit matrix, so here the two would disagree.
	for (int n = 0; n < e->N; n++)
		if (n != e->root && e->explicit_host[n])
			return fail(PHYAMD_EUNSUPPORTED, "the Hessian diagonal differentiates exp(Q t r): node %d has explicit matrices", n);
	// 4 states: one workgroup holds all categories' exchange (hess_lds: 124 KB at 8); more are refused
	if (!e->generic && e->C > 8) return fail(PHYAMD_EUNSUPPORTED, "the Hessian diagonal takes at most 8 categories with 4 states (this engine has %d)", e->C);
	return check_ready(e);
}

int shard_branch_hessian_diagonal_device(Shard *e, int flags, double *device_out) {
	CHECK_ENGINE(e);
	if (!device_out) return fail(PHYAMD_EINVAL, "null device_out");
	int rc;
	if ((rc = hessian_ready(e, flags)) || (rc = eval_hessian(e))) return rc;
	HIP_TRY(hipMemcpyAsync(device_out, hess_result(e), sizeof(double) * ((size_t)1 + 2 * e->N), hipMemcpyDeviceToDevice, e->stream));
	return PHYAMD_OK;
}

// out[1 + 2 N] = [lnL | d1 | d2] on the host
int shard_branch_hessian_diagonal(Shard *e, int flags, double *out) {
	CHECK_ENGINE(e);
	int rc;
	if ((rc = hessian_ready(e, flags)) || (rc = eval_hessian(e))) return rc;
	HIP_TRY(hipMemcpyAsync(out, hess_result(e), sizeof(double) * ((size_t)1 + 2 * e->N), hipMemcpyDeviceToHost, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream));
	return PHYAMD_OK;
}

int shard_root_frequency_term(Shard *e, double *out) {
	CHECK_ENGINE(e);
	if (!out) return fail(PHYAMD_EINVAL, "null out");
	int rc;
	if ((rc = bind_device(e))) return rc;
	if ((rc = check_ready(e))) return rc;
	if (e->tiles == 1 && (!lowers_current(e) || e->core_index[e->root] < 0 || !e->d_lower)) return fail(PHYAMD_EINVAL, "no evaluation has been run yet");
	// (the root's array is p_root in every storage convention: only a rescaled evaluation's factors have to be the reference's)
	if (e->scaling_on && (rc = require_reference_form(e))) return rc;
	if (e->tiles > 1) {  // the per-tile terms were summed by the last phyamd_parameter_gradient
		if (!tiled_totals_current(e, true)) return fail(PHYAMD_EINVAL, "with tiled patterns the root frequency term comes with phyamd_parameter_gradient: call that first");
		HIP_TRY(hipMemcpyAsync(e->h_result, e->d_result + 1 + (size_t)e->N * e->C + e->np, sizeof(double) * e->S, hipMemcpyDeviceToHost, e->stream));
		HIP_TRY(hipStreamSynchronize(e->stream));
		std::memcpy(out, e->h_result, sizeof(double) * e->S);
		return PHYAMD_OK;
	}
	if ((rc = launch_root_frequency_term(e, nullptr))) return rc;
	HIP_TRY(hipMemcpyAsync(e->h_result, e->d_rf_part + (size_t)((e->P + 255) / 256) * e->S, sizeof(double) * e->S, hipMemcpyDeviceToHost, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream));
	std::memcpy(out, e->h_result, sizeof(double) * e->S);
	return PHYAMD_OK;
}

// the sibling subtree `s` as child_message / PathStep take it
static void describe_subtree(const Shard *e, int s, PathStep &st) {
	st.kind = e->node_kind[s];
	st.node = s;
	st.core = e->core_index[s];
	st.t0 = st.t1 = st.t2 = st.inner = -1;
	if (st.kind == CH_CHERRY) {
		st.t0 = e->left[s];
		st.t1 = e->right[s];
	} else if (st.kind == CH_CHERRY_TIP) {
		const int l = e->left[s], r = e->right[s];
		st.inner = l < e->T ? r : l;
		st.t2 = l < e->T ? l : r;
		st.t0 = e->left[st.inner];
		st.t1 = e->right[st.inner];
	}
}

// 20 states: the lower partial of a fused cherry as an array
static int cherry_partial_gen(Shard *e, int node, double *out) {
	const int l = e->left[node], r = e->right[node];
	const size_t msz = (size_t)e->C * e->S * e->S;
	hipLaunchKernelGGL(k_cherry_partial_gen, dim3((e->P + 255) / 256), dim3(256), 0, e->stream, e->P, e->Pp, e->S, e->C, e->d_mats + (size_t)l * msz, e->d_mats + (size_t)r * msz,
	                   e->d_tipmask + (size_t)l * e->P, e->d_tipmask + (size_t)r * e->P, e->d_tipsets, out);
	HIP_TRY(hipGetLastError());
	return PHYAMD_OK;
}

// upper partial of `node` into d_path_upper (and, for a node without a stored lower partial, that partial into d_path_lower)
static int rebuild_path_upper(Shard *e, int node) {
	int rc;
	const size_t npd = node_partial_doubles(e);
	if ((rc = e->d_path_upper.ensure(npd)) || (rc = e->d_path_lower.ensure(npd)) || (rc = e->d_path_steps.ensure(e->N))) return rc;
	if (e->generic && (rc = e->d_path_tmp.ensure(npd))) return rc;
	std::vector<int> path;  // node, parent, ..., root
	for (int a = node; a >= 0; a = e->parent[a]) path.push_back(a);
	const int m = (int)path.size() - 1;  // steps
	if (!e->generic) {
		std::vector<PathStep> steps(m);
		for (int j = 0; j < m; j++) {
			const int par = path[m - j], child = path[m - j - 1];
			steps[j].mat = par == e->root ? -1 : par;
			describe_subtree(e, e->left[par] == child ? e->right[par] : e->left[par], steps[j]);
		}
		HIP_TRY(hipMemcpyAsync(e->d_path_steps, steps.data(), sizeof(PathStep) * m, hipMemcpyHostToDevice, e->stream));
		const dim3 grid((e->P + WAVE - 1) / WAVE), block(WAVE, e->C);
		if (e->scaling_on)
			hipLaunchKernelGGL(k_path_upper4<true>, grid, block, sizeof(double) * e->C * WAVE, e->stream, e->d_path_steps, m, e->T, e->P, e->C, e->d_tipmask, e->d_lower,
			                   e->d_mats, e->d_tiptab, e->d_path_upper);
		else
			hipLaunchKernelGGL(k_path_upper4<false>, grid, block, 0, e->stream, e->d_path_steps, m, e->T, e->P, e->C, e->d_tipmask, e->d_lower, e->d_mats,
			                   e->d_tiptab, e->d_path_upper);
		if (node >= e->T && e->core_index[node] < 0) {  // fringe / DEEP node: its own partial is not stored either
			PathStep self;
			describe_subtree(e, node, self);
			hipLaunchKernelGGL(k_unstored_partial4, grid, block, 0, e->stream, self.kind, node, self.t0, self.t1, self.t2, self.inner, e->T, e->P, e->C, e->d_tipmask,
			                   e->d_mats, e->d_tiptab, e->d_path_lower);
		}
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipStreamSynchronize(e->stream));  // `steps` is a stack-lifetime buffer
	} else {
		// one launch per step, ping-pong between two buffers so that the last step lands in d_path_upper
		const size_t msz = (size_t)e->C * e->S * e->S;
		const int pb = (e->P + 255) / 256;
		double *cur = nullptr;
		for (int j = 0; j < m; j++) {
			const int par = path[m - j], child = path[m - j - 1];
			const int sib = e->left[par] == child ? e->right[par] : e->left[par];
			double *dst = ((m - 1 - j) & 1) ? e->d_path_tmp : e->d_path_upper;
			const double *sp = sib < e->T ? nullptr : e->d_lower + (size_t)e->core_index[sib] * npd;  // a stored node: t = P p (k_lower_gen)
			int carried = 1;
			if (sib >= e->T && e->core_index[sib] < 0) {  // a fused cherry: its partial is formed on the side (d_path_lower is free until the end)
				if ((rc = cherry_partial_gen(e, sib, e->d_path_lower))) return rc;
				sp = e->d_path_lower;
				carried = 0;
			}
			hipLaunchKernelGGL(k_path_step_gen, dim3(pb), dim3(256), 0, e->stream, e->P, e->Pp, e->S, e->C, par == e->root ? (const double *)nullptr : e->d_mats + (size_t)par * msz,
			                   par == e->root ? (const double *)nullptr : cur, e->d_mats + (size_t)sib * msz, sp, carried,
			                   sib < e->T ? e->d_tipmask + (size_t)sib * e->P : (const uint8_t *)nullptr, e->d_tipsets, dst);
			if (e->scaling_on) hipLaunchKernelGGL(k_path_scale_gen, dim3(pb), dim3(256), 0, e->stream, e->P, e->Pp, e->S, e->C, dst);
			cur = dst;
		}
		HIP_TRY(hipGetLastError());  // (the node's own partial: true_lower_gen, shard_branch_log_likelihood)
	}
	path_upper_rebuilt(e, node);
	return PHYAMD_OK;
}

int shard_branch_log_likelihood(Shard *e, int node, double length, double *lnl, double *d1, double *d2) {
	CHECK_ENGINE(e);
	NOT_TILED(e, "the single-branch evaluation");
	if (node < 0 || node >= e->N || node == e->root) return fail(PHYAMD_EINVAL, "node %d has no branch", node);
	if (!e->have_eigen) return fail(PHYAMD_EINVAL, "the single-branch evaluation needs the eigen system (phyamd_set_eigen)");
	int rc;
	if ((rc = bind_device(e))) return rc;
	if ((rc = require_reference_form(e))) return rc;  // (stored partials: the partials themselves, in the reference's form)
	const size_t npd = node_partial_doubles(e);
	// the two partials that meet on the branch: resident after a keep-partials gradient, else the upper one is rebuilt by a
	// walk down the path from the root (pending changes are evaluated first; the result is kept until partials change)
	const double *up, *low;
	int fold = 0;
	if (uppers_resident(e)) {
		up = e->d_upper + (size_t)e->upper_slot[node] * npd;
		low = node < e->T ? nullptr : e->d_lower + (size_t)e->core_index[node] * npd;
		fold = e->upper_fold ? 1 : 0;
	} else {
		if ((rc = run_lower(e, true))) return rc;
		if (e->state.path_node != node && (rc = rebuild_path_upper(e, node))) return rc;
		up = e->d_path_upper;
		low = node < e->T ? nullptr : (e->core_index[node] >= 0 ? e->d_lower + (size_t)e->core_index[node] * npd : e->d_path_lower);
	}
	if (e->generic && node >= e->T) {  // the branch's P(t) changes here: p_node itself, not the stored P p (k_lower_gen)
		if ((rc = e->d_path_lower.ensure(npd)) || (rc = e->d_path_side.ensure(2 * npd))) return rc;
		if ((rc = true_lower_gen(e, node, e->d_path_lower, e->d_path_side))) return rc;
		low = e->d_path_lower;
	}
	const int C = e->C, S = e->S, S2 = S * S;
	const int per_block = e->generic ? 256 : WAVE, nb = (e->P + per_block - 1) / per_block;
	const size_t msz = (size_t)C * (e->generic ? 4 : 3) * S2, need = msz + (size_t)3 * nb + 3;
	if ((rc = e->d_branch.ensure(need))) return rc;
	// P(t r_c), r_c Q P, r_c^2 Q Q P from the eigen system (host: S^3 per category)
	const double *ev = e->model.data(), *U = ev + S, *Ui = U + S2;
	std::vector<double> pm(msz), ex(S);
	const int stride = e->generic ? 4 * S2 : 48;
	for (int c = 0; c < C; c++) {
		const double r = e->rates[c], t = length * r;
		for (int a = 0; a < S; a++) ex[a] = std::exp(ev[a] * t);
		for (int i = 0; i < S; i++)
			for (int j = 0; j < S; j++) {
				double p0 = 0.0, p1 = 0.0, p2 = 0.0;
				for (int a = 0; a < S; a++) {
					const double w = U[i * S + a] * Ui[a * S + j] * ex[a];
					p0 += w;
					p1 += w * ev[a];
					p2 += w * ev[a] * ev[a];
				}
				pm[(size_t)c * stride + i * S + j] = std::fabs(p0);  // substmodel.c:552
				pm[(size_t)c * stride + S2 + i * S + j] = r * p1;
				pm[(size_t)c * stride + 2 * S2 + i * S + j] = r * r * p2;
			}
	}
	HIP_TRY(hipMemcpyAsync(e->d_branch, pm.data(), sizeof(double) * pm.size(), hipMemcpyHostToDevice, e->stream));
	// rescaled evaluations: the per-pattern lnL of the resident evaluation anchors the stored (scaled) partials
	const double *plk = e->scaling_on ? e->d_plk : nullptr;
	const double *m0 = e->d_mats + (size_t)node * C * S2;
	double *part = e->d_branch + msz;
	if (e->generic) {
		if (plk)
			for (int c = 0; c < C; c++)
				HIP_TRY(hipMemcpyAsync(e->d_branch + (size_t)c * stride + 3 * S2, m0 + (size_t)c * S2, sizeof(double) * S2, hipMemcpyDeviceToDevice, e->stream));
		hipLaunchKernelGGL(k_branch_eval_gen, dim3(nb), dim3(256), 0, e->stream, node, e->T, e->P, e->Pp, S, C, up, low, e->d_tipmask, e->d_tipsets, e->d_branch,
		                   e->d_freqs, fold, e->d_props, e->d_weights, plk, part);
	} else
		hipLaunchKernelGGL(k_branch_eval4, dim3(nb), dim3(WAVE, C), sizeof(double) * 4 * C * WAVE, e->stream, e->P, C, up, low,
		                   node < e->T ? e->d_tipmask + (size_t)node * e->P : (const uint8_t *)nullptr, e->d_branch, e->d_freqs, fold, e->d_props, e->d_weights, plk,
		                   m0, part);
	hipLaunchKernelGGL(k_reduce_rows, dim3(3), dim3(64), 0, e->stream, part, nb, (const uint8_t *)nullptr, part + (size_t)3 * nb);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(e->h_result, part + (size_t)3 * nb, sizeof(double) * 3, hipMemcpyDeviceToHost, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream));  // also covers pm (stack-lifetime buffer)
	if (lnl) *lnl = e->h_result[0];
	if (d1) *d1 = e->h_result[1];
	if (d2) *d2 = e->h_result[2];
	return PHYAMD_OK;
}

int shard_root_invariant_term(Shard *e, double *out) {
	CHECK_ENGINE(e);
	if (!out) return fail(PHYAMD_EINVAL, "null out");
	if (e->C < 2) return fail(PHYAMD_EINVAL, "the invariant-class term needs at least two categories");
	int rc;
	if ((rc = bind_device(e))) return rc;
	if ((rc = check_ready(e))) return rc;
	const double *src;
	if (e->tiles > 1) {  // summed over the tiles by the last evaluation (one entry behind everything else in the total), each tile in its own form
		if (!tiled_totals_current(e)) return fail(PHYAMD_EINVAL, "no evaluation has been run yet");
		src = e->d_total + (size_t)e->N * e->C + 2 * PHYAMD_MAX_PARAMETERS;
	} else {
		if (!lowers_current(e) || e->core_index[e->root] < 0 || !e->d_lower) return fail(PHYAMD_EINVAL, "no evaluation has been run yet");
		if (e->scaling_on && (rc = require_reference_form(e))) return rc;  // (see shard_root_frequency_term)
		if ((rc = launch_root_invariant_term(e, nullptr))) return rc;
		src = e->d_inv_part + (e->P + 255) / 256;
	}
	HIP_TRY(hipMemcpyAsync(e->h_result, src, sizeof(double), hipMemcpyDeviceToHost, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream));
	*out = e->h_result[0];
	return PHYAMD_OK;
}

int shard_synchronize(Shard *e) {
	CHECK_ENGINE(e);
	int rc;
	if ((rc = bind_device(e))) return rc;
	HIP_TRY(hipStreamSynchronize(e->stream));
	return PHYAMD_OK;
}

int shard_get_pattern_log_likelihoods(Shard *e, double *out) {
	CHECK_ENGINE(e);
	if (!out) return fail(PHYAMD_EINVAL, "null out");
	int rc;
	if ((rc = bind_device(e))) return rc;
	HIP_TRY(hipMemcpyAsync(out, e->tiles > 1 ? e->d_plk_all : e->d_plk, sizeof(double) * e->Ptot, hipMemcpyDeviceToHost, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream));
	return PHYAMD_OK;
}

int shard_get_partials(Shard *e, int node, int upper, double *out) {
	CHECK_ENGINE(e);
	NOT_TILED(e, "reading partials back");
	if (!out || node < 0 || node >= e->N) return fail(PHYAMD_EINVAL, "bad node %d or null out", node);
	int rc;
	if ((rc = bind_device(e))) return rc;
	if ((rc = require_reference_form(e))) return rc;  // (stored partials: the partials themselves, in the reference's form)
	const size_t np = node_partial_doubles(e);
	if (upper) {
		if (!uppers_resident(e)) return fail(PHYAMD_EINVAL, "upper partials need shard_set_keep_partials(1) before phyamd_gradient");
		if (node == e->root) return fail(PHYAMD_EINVAL, "the root has no upper partial");
	}
	if (!upper && node < e->T) {  // rebuild the replicated tip partial from its mask / code
		std::vector<uint8_t> mask(e->P);
		HIP_TRY(hipMemcpyAsync(mask.data(), e->d_tipmask + (size_t)node * e->P, e->P, hipMemcpyDeviceToHost, e->stream));
		HIP_TRY(hipStreamSynchronize(e->stream));
		const int S = e->S;
		for (int c = 0; c < e->C; c++)
			for (int k = 0; k < e->P; k++)
				for (int s = 0; s < S; s++)
					out[((size_t)c * e->P + k) * S + s] = !e->generic        ? ((mask[k] >> s) & 1 ? 1.0 : 0.0)
					                                      : mask[k] > S      ? (double)((e->tipsets_host[mask[k] - S - 1] >> s) & 1)
					                                      : (mask[k] == S || mask[k] == s) ? 1.0 : 0.0;
		return PHYAMD_OK;
	}
	if (!upper && e->core_index[node] < 0)
		return fail(PHYAMD_EINVAL, "node %d is fused into its parent (cherry / cherry+tip) and not stored: shard_set_keep_partials(1) first", node);
	const double *src = upper ? e->d_upper + (size_t)e->upper_slot[node] * np : e->d_lower + (size_t)e->core_index[node] * np;
	if (e->generic) {  // planes [C][S][Pp] -> the reference's [C][P][S]
		DeviceArray<double> tmp;  // (a temporary: not counted in device_bytes)
		const size_t cnt = (size_t)e->C * e->P * e->S;
		if ((rc = tmp.ensure(cnt + (upper ? 0 : 3 * np)))) return rc;
		if (!upper) {  // a stored lower array is t = P p (k_lower_gen): the partial itself is formed from the node's children
			if ((rc = true_lower_gen(e, node, tmp + cnt, tmp + cnt + np))) return rc;
			src = tmp + cnt;
		}
		hipLaunchKernelGGL(k_planes_to_reference, dim3((unsigned)std::min<size_t>((cnt + 255) / 256, 4096)), dim3(256), 0, e->stream, e->P, e->Pp, e->S,
		                   e->C, src, tmp);
		hipError_t err = hipMemcpyAsync(out, tmp, cnt * sizeof(double), hipMemcpyDeviceToHost, e->stream);
		if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
		if (err != hipSuccess) return fail(PHYAMD_EDEVICE, "get_partials: %s", hipGetErrorString(err));
		return PHYAMD_OK;
	}
	HIP_TRY(hipMemcpyAsync(out, src, sizeof(double) * np, hipMemcpyDeviceToHost, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream));
	return PHYAMD_OK;
}

int shard_get_node_matrices(Shard *e, int node, int derivative, double *out) {
	CHECK_ENGINE(e);
	if (!out || node < 0 || node >= e->N) return fail(PHYAMD_EINVAL, "bad node %d or null out", node);
	int rc;
	if ((rc = bind_device(e))) return rc;
	if ((rc = check_ready(e))) return rc;
	if ((rc = update_matrices(e))) return rc;
	const size_t sz = (size_t)e->C * e->S * e->S;
	HIP_TRY(hipMemcpyAsync(out, (derivative ? e->d_dmats : e->d_mats) + (size_t)node * sz, sizeof(double) * sz, hipMemcpyDeviceToHost, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream));
	return PHYAMD_OK;
}

int shard_is_rescaling(Shard *e) {
	CHECK_ENGINE(e);
	return e->scaling_on ? 1 : 0;
}

int shard_set_rescaling(Shard *e, int policy) {
	CHECK_ENGINE(e);
	if (policy < 0 || policy > 2) return fail(PHYAMD_EINVAL, "rescale must be PHYAMD_RESCALE_*");
	e->cfg.rescale = policy;
	// NEVER / ALWAYS take effect at once; AUTO keeps what the engine is doing now (the lazy switch only ever turns rescaling on)
	const bool want = policy == PHYAMD_RESCALE_ALWAYS ? true : policy == PHYAMD_RESCALE_NEVER ? false : e->scaling_on;
	if (want == e->scaling_on) return PHYAMD_OK;
	e->scaling_on = want;
	lowers_discarded(e);
	if (e->have_topology) {
		int rc;
		if ((rc = bind_device(e))) return rc;
		if ((rc = rebuild_schedule(e))) return rc;
	}
	return PHYAMD_OK;
}

int shard_set_keep_partials(Shard *e, int on) {
	CHECK_ENGINE(e);
	if (on) NOT_TILED(e, "keeping every partial");
	const bool want = on != 0;
	if (want == e->keep_partials) return PHYAMD_OK;
	if (want) prefer_reference_form(e);  // (resident partials are the reference's)
	e->keep_partials = want;
	lowers_discarded(e);
	if (e->have_topology) {
		int rc;
		if ((rc = bind_device(e))) return rc;
		if ((rc = rebuild_schedule(e))) return rc;
	}
	return PHYAMD_OK;
}

int shard_set_profiling(Shard *e, int on) {
	CHECK_ENGINE(e);
	e->profiling = on != 0;
	return PHYAMD_OK;
}

int shard_get_profile(Shard *e, phyamd_profile *out) {
	CHECK_ENGINE(e);
	if (!out) return fail(PHYAMD_EINVAL, "null out");
	finish_profile(e, e->prof_with_upper);  // waits for the last evaluation's events if they are still pending
	e->prof.device_bytes = e->mem.bytes;
	e->prof.tiles = e->tiles;
	*out = e->prof;
	return PHYAMD_OK;
}

// ---- a batch of branch-length vectors (phyamd_gradient_batch) ----------------------------------------------------------------

// the two op lists of the batched walk for a tree (T tips; left / right / root in phyamd_set_topology's convention, already
// validated), appended to `ops` as [post-order T - 1 | pre-order T - 1]; returns the upper slots the pre-order list parks in.
// ops == null: only counts the slots.  Post-order: depth first, the larger subtree first, so that the child finished last hands
// its partial on in registers.  Pre-order: of two internal children the smaller subtree is entered first with its upper in
// registers and the other's upper is parked in a slot that is free again once its op has read it: at most log2(T) + 1 slots,
// whatever the shape (a caterpillar parks nothing).  Ties go by left / right, never by node id: the lists of one tree under two
// labellings of its internal nodes differ in the ids only.
// park_all (phyamd_nni_log_likelihoods): every internal child's upper is parked in a slot of its own, slot = node - T, and none
// is handed on in registers: T - 1 slots, and after the walk every internal non-root node's upper is in the scratch.
int build_batch_ops(int T, const int32_t *left, const int32_t *right, int root, std::vector<BatchOp> *ops, bool park_all = false) {
	const int N = 2 * T - 1;
	std::vector<int> size(N, 1), order;
	{
		std::vector<int> stack{root};
		while (!stack.empty()) {
			const int n = stack.back();
			stack.pop_back();
			order.push_back(n);
			if (n >= T) {
				stack.push_back(left[n]);
				stack.push_back(right[n]);
			}
		}
		for (size_t i = order.size(); i-- > 0;)
			if (order[i] >= T) size[order[i]] += size[left[order[i]]] + size[right[order[i]]];
	}
	if (ops) {  // post-order: (node, children done?) on an explicit stack
		std::vector<std::pair<int, bool>> stack{{root, false}};
		int last = -1;
		while (!stack.empty()) {
			const auto [n, done] = stack.back();
			stack.pop_back();
			const int l = left[n], r = right[n];
			if (!done) {
				stack.push_back({n, true});
				const int first = size[l] >= size[r] ? l : r, second = first == l ? r : l;
				if (second >= T) stack.push_back({second, false});
				if (first >= T) stack.push_back({first, false});
				continue;
			}
			BatchOp op{n, l, r, last == l && l >= T ? 1 : last == r && r >= T ? 2 : 0, BATCH_NONE, BATCH_NONE, BATCH_NONE, 0};
			ops->push_back(op);
			last = n;
		}
	}
	int slots = 0;
	{  // pre-order
		std::vector<std::pair<int, int>> stack{{root, BATCH_ROOT}};  // (node, where its upper is)
		std::vector<int> free_slots;
		while (!stack.empty()) {
			const auto [n, src] = stack.back();
			stack.pop_back();
			const int l = left[n], r = right[n];
			BatchOp op{n, l, r, 0, src, BATCH_NONE, BATCH_NONE, 0};
			if (park_all) {
				if (l >= T) op.dst_left = l - T, stack.push_back({l, l - T});
				if (r >= T) op.dst_right = r - T, stack.push_back({r, r - T});
				if (ops) ops->push_back(op);
				continue;
			}
			if (l >= T && r >= T) {
				int slot;
				if (free_slots.empty()) slot = slots++;
				else {
					slot = free_slots.back();
					free_slots.pop_back();
				}
				const bool left_first = size[l] <= size[r];
				op.dst_left = left_first ? BATCH_CARRY : slot;
				op.dst_right = left_first ? slot : BATCH_CARRY;
				stack.push_back({left_first ? r : l, slot});
				stack.push_back({left_first ? l : r, BATCH_CARRY});
			} else if (l >= T) {
				op.dst_left = BATCH_CARRY;
				stack.push_back({l, BATCH_CARRY});
			} else if (r >= T) {
				op.dst_right = BATCH_CARRY;
				stack.push_back({r, BATCH_CARRY});
			}
			if (ops) ops->push_back(op);
			if (src >= 0) free_slots.push_back(src);  // read by this op: later ops may park in it
		}
	}
	return park_all ? std::max(1, T - 1) : std::max(1, slots);
}

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

// what a batch call needs of the scratch per item: the pre-order pass's part, so many upper slots, its own op lists and root;
// nni: the one item of phyamd_nni_log_likelihoods -- every upper parked (slots = T - 1) and that call's own arrays; spr: the
// items are rows of phyamd_spr_log_likelihoods -- every upper parked, their own op lists, and that call's arrays
struct BatchShape {
	bool grad;
	int slots;
	bool trees;
	bool nni = false;
	bool spr = false;
};

size_t nni_candidates(const Shard *e) { return (size_t)std::max(0, e->T - 2); }

// bytes of batch scratch one item takes
size_t batch_item_bytes(const Shard *e, BatchShape w) {
	const size_t nblk = ((size_t)e->P + WAVE - 1) / WAVE, plane = nblk * WAVE * 4;
	size_t doubles = (size_t)e->N + (size_t)e->N * e->C * 16 + 1 + (w.grad ? (size_t)e->N * e->C : 0) + (size_t)(e->T - 1) * e->C * plane + nblk;
	if (w.grad) doubles += (size_t)w.slots * e->C * plane + nblk * e->C * e->N;
	size_t bytes = sizeof(double) * doubles + (w.trees ? sizeof(BatchOp) * 2 * (size_t)(e->T - 1) + sizeof(int32_t) : 0);
	if (w.nni) {  // trial lengths and matrices, the slab, the result; the op lists, the candidates and their index by node
		const size_t cands = std::max<size_t>(nni_candidates(e), 1);
		bytes += sizeof(double) * ((size_t)3 * e->N + (size_t)3 * e->N * e->C * 16 + cands * nblk * 9 + (size_t)9 * e->N);
		bytes += sizeof(BatchOp) * 2 * (size_t)(e->T - 1) + sizeof(NniCand) * cands + sizeof(int32_t) * e->N;
	}
	if (w.spr) {  // the row's candidates, their index by cell, the slab, the result; the two length vectors and their matrices (once: counted per row)
		bytes += (sizeof(SprCand) + sizeof(int32_t) + sizeof(double) * (nblk + 1)) * (size_t)e->N;
		bytes += sizeof(double) * ((size_t)2 * e->N + (size_t)2 * e->N * e->C * 16);
	}
	return bytes;
}

size_t batch_scratch_bytes(const Shard *e) { return (size_t)e->batch_mem.bytes; }

void release_batch_scratch(Shard *e) {
	e->batch_mem.release_all();
	e->batch_items = 0;
}

// items of shape w the scratch holds now (none once the group has been released to make room)
size_t batch_items_held(const Shard *e, BatchShape w) {
	const bool serves = e->d_batch_lower.get() && (e->batch_grad || !w.grad) && (!w.grad || e->batch_slots >= w.slots) && (e->batch_trees || !w.trees) &&
	                    (e->batch_nni || !w.nni) && (e->batch_spr || !w.spr);
	return serves ? (size_t)e->batch_items : 0;
}

constexpr int BATCH_MAX_CHUNK = 65535;  // gridDim.y

// items of a batch (count items of shape w) whose scratch fits beside the engine: within the cap less everything the engine holds
// or may still allocate -- what is resident whatever the tile size, the tile's working set as choose_tiles reserves it, the walks'
// on-demand buffers -- or, without a cap, within most of what the device has free right now.  What the scratch holds already is
// kept unless more items would fit.
size_t batch_items_that_fit(const Shard *e, size_t count, BatchShape w) {
	const size_t want = std::min<size_t>(count, BATCH_MAX_CHUNK), have = batch_items_held(e, w);
	if (have >= want) return want;
	const double held = (double)batch_scratch_bytes(e);
	double room;
	if (e->cfg.max_device_bytes > 0) {
		const double tile_now = (double)e->tile_mem.bytes, resident = (double)e->mem.bytes - held - tile_now;
		room = (double)e->cfg.max_device_bytes - (resident + 65536.0 + walk_reserve(e) + std::max(tile_now, tile_working_set(e, (double)e->P, true)));
	} else {
		size_t free_bytes = 0, total_bytes = 0;
		room = hipMemGetInfo(&free_bytes, &total_bytes) == hipSuccess ? 0.8 * ((double)free_bytes + held) : 0.0;
	}
	const double fit = std::floor(room / (double)batch_item_bytes(e, w));
	if (fit <= (double)have) return have;
	return (size_t)std::min((double)want, fit);
}

int allocate_batch_scratch(Shard *e, size_t items, BatchShape w) {
	release_batch_scratch(e);  // (the arrays grow together: all are freed before any is allocated again)
	const size_t nblk = ((size_t)e->P + WAVE - 1) / WAVE, plane = nblk * WAVE * 4, rows = w.grad ? (size_t)1 + e->N * e->C : 1;
	int rc;
	if ((rc = e->d_batch_len.ensure(items * e->N)) || (rc = e->d_batch_mats.ensure(items * e->N * e->C * 16)) || (rc = e->d_batch_out.ensure(items * rows)) ||
	    (rc = e->d_batch_lower.ensure(items * (e->T - 1) * e->C * plane)) || (rc = e->d_batch_lnl.ensure(items * nblk)) ||
	    (w.grad && ((rc = e->d_batch_upper.ensure(items * w.slots * e->C * plane)) || (rc = e->d_batch_slab.ensure(items * nblk * e->C * e->N)))) ||
	    (w.trees && ((rc = e->d_batch_item_ops.ensure(items * 2 * (e->T - 1))) || (rc = e->d_batch_roots.ensure(items)))) ||
	    (w.nni && ((rc = e->d_nni_ops.ensure((size_t)2 * (e->T - 1))) || (rc = e->d_nni_cands.ensure(nni_candidates(e))) || (rc = e->d_nni_cand_of.ensure(e->N)) ||
	               (rc = e->d_nni_len.ensure((size_t)3 * e->N)) || (rc = e->d_nni_mats.ensure((size_t)3 * e->N * e->C * 16)) ||
	               (rc = e->d_nni_slab.ensure(nni_candidates(e) * nblk * 9)) || (rc = e->d_nni_out.ensure((size_t)9 * e->N)))) ||
	    (w.spr && ((rc = e->d_spr_cands.ensure(items * e->N)) || (rc = e->d_spr_cand_of.ensure(items * e->N)) || (rc = e->d_spr_slab.ensure(items * e->N * nblk)) ||
	               (rc = e->d_spr_out.ensure(items * e->N)) || (rc = e->d_spr_len.ensure((size_t)2 * e->N)) || (rc = e->d_spr_mats.ensure((size_t)2 * e->N * e->C * 16))))) {
		release_batch_scratch(e);
		return rc;
	}
	e->batch_nni = w.nni;
	e->nni_lists_valid = false;  // (freed above with everything else)
	e->batch_spr = w.spr;
	e->batch_items = (int)items;
	e->batch_grad = w.grad;
	e->batch_slots = w.grad ? w.slots : 0;
	e->batch_trees = w.trees;
	return PHYAMD_OK;
}

int ensure_batch_scratch(Shard *e, size_t items, BatchShape w) {
	if (batch_items_held(e, w) >= items) return PHYAMD_OK;
	if (e->cfg.max_device_bytes <= 0 && e->d_batch_lower.get()) {
		// without a cap the scratch keeps what the previous call needed as well: calls of the two kinds, or of trees that park in
		// fewer and in more slots, may alternate without an allocation each (under a cap every call gets exactly its own)
		const BatchShape both{w.grad || e->batch_grad, std::max(w.slots, e->batch_slots), w.trees || e->batch_trees, w.nni || e->batch_nni, w.spr || e->batch_spr};
		if (allocate_batch_scratch(e, items, both) == PHYAMD_OK) return PHYAMD_OK;
	}
	return allocate_batch_scratch(e, items, w);
}

// one chunk of `items` items through the batched walk: lengths [items][N] (host) -> out [items][rows] (host), rows = 1 or 1 + N C.
// w.trees: the items walk their own op lists from their own roots, already in d_batch_item_ops and d_batch_roots; else the
// engine's.  w.slots: the upper slots an item of this chunk has in d_batch_upper (at least what its list parks in)
int run_batch_chunk(Shard *e, int flags, int items, const double *lengths, BatchShape w, double *out) {
	const int nblk = (e->P + WAVE - 1) / WAVE, rows = w.grad ? 1 + e->N * e->C : 1, nops = e->T - 1;
	const BatchOp *ops = w.trees ? e->d_batch_item_ops.get() : e->d_batch_ops.get();
	const int32_t *roots = w.trees ? e->d_batch_roots.get() : nullptr;
	HIP_TRY(hipMemcpyAsync(e->d_batch_len, lengths, sizeof(double) * (size_t)items * e->N, hipMemcpyHostToDevice, e->stream));
	const size_t total = (size_t)items * e->N * e->C * 16;
	hipLaunchKernelGGL(k_batch_matrices, dim3((unsigned)std::min<size_t>((total + 255) / 256, 4096)), dim3(256), 0, e->stream, e->C, e->N, items, e->d_model, e->d_rates,
	                   e->d_batch_len, e->root, roots, e->d_batch_mats);
	const BatchArgs a{ops, ops + nops, w.trees ? 2 * nops : 0, e->T, e->N, e->P, e->C, nblk, w.slots, w.grad ? 1 : 0, e->d_tipmask, e->d_freqs, e->d_props,
	                  e->d_weights, e->d_Q, e->d_batch_mats, e->d_batch_lower, e->d_batch_upper, e->d_batch_lnl, e->d_batch_slab};
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

// the definition of the call: item by item through the ordinary path (the caller puts the engine's lengths back)
int batch_item_sequential(Shard *e, int flags, const double *lengths, double *lnl, double *cat_gradient) {
	int rc;
	if ((rc = shard_set_branch_lengths(e, lengths))) return rc;
	return cat_gradient ? shard_gradient(e, flags, lnl, cat_gradient) : shard_log_likelihood(e, lnl);
}

// the items of a batch, each through the batched walk or the ordinary path; prof: how many went which way
int run_batch(Shard *e, int flags, int32_t count, const double *branch_lengths, double *lnl, double *cat_gradient, phyamd_batch_profile &prof) {
	int rc;
	{  // ready but for the lengths, which the call brings itself
		const bool had = e->have_lengths;
		e->have_lengths = true;
		rc = check_ready(e);
		e->have_lengths = had;
		if (rc) return rc;
	}
	for (int n = 0; n < e->N; n++)
		if (n != e->root && e->explicit_host[n])
			return fail(PHYAMD_EUNSUPPORTED, "phyamd_gradient_batch: node %d has explicit matrices, which cannot follow per-item branch lengths", n);
	if (cat_gradient && !e->have_Q) return fail(PHYAMD_EINVAL, "the gradient needs the rate matrix: phyamd_set_eigen or phyamd_set_rate_matrix");
	const bool grad = cat_gradient != nullptr;
	const size_t N = (size_t)e->N, ncat = N * e->C, rows = grad ? 1 + ncat : 1;
	std::vector<uint8_t> redo(count, 1);  // items the sequential path (still) has to evaluate
	if ((rc = ensure_engine_batch_ops(e))) return rc;
	const BatchShape shape{grad, e->batch_upper_slots, false};
	std::vector<double> lengths, out;
	for (size_t first = 0; first < (size_t)count && batch_fast_path(e, flags, 1);) {
		// (every chunk asks again: an item that went through the ordinary path may have taken the scratch's room)
		const size_t chunk = batch_items_that_fit(e, (size_t)count - first, shape);
		if (!batch_fast_path(e, flags, chunk)) break;
		if ((rc = ensure_batch_scratch(e, chunk, shape))) return rc;
		const size_t items = std::min(chunk, (size_t)count - first);
		lengths.assign(branch_lengths + first * N, branch_lengths + (first + items) * N);
		out.resize(items * rows);
		for (size_t b = 0; b < items; b++) lengths[b * N + e->root] = 0.0;  // (ignored, as phyamd_set_branch_lengths does)
		if ((rc = run_batch_chunk(e, flags, (int)items, lengths.data(), shape, out.data()))) return rc;
		prof.chunks++;
		for (size_t b = 0; b < items; b++) {
			const double l = out[b * rows];
			const bool bad = std::isnan(l) || std::isinf(l);
			if (bad && e->cfg.rescale == PHYAMD_RESCALE_AUTO) {
				// the lazy switch's case (treelikelihood.c:1496-1519): this item goes through the ordinary path right away, and
				// if that turns rescaling on, so does the rest of the batch
				if ((rc = batch_item_sequential(e, flags, branch_lengths + (first + b) * N, lnl + first + b, grad ? cat_gradient + (first + b) * ncat : nullptr))) return rc;
				redo[first + b] = 0;
				prof.items_sequential++;
				continue;
			}
			lnl[first + b] = l;
			for (size_t i = 0; grad && i < ncat; i++) cat_gradient[(first + b) * ncat + i] = bad ? NAN : out[b * rows + 1 + i];  // treelikelihood.c:327-332
			redo[first + b] = 0;
			prof.items_fast++;
		}
		first += items;
	}
	for (int b = 0; b < count; b++) {
		if (!redo[b]) continue;
		if ((rc = batch_item_sequential(e, flags, branch_lengths + (size_t)b * N, lnl + b, grad ? cat_gradient + (size_t)b * ncat : nullptr))) return rc;
		prof.items_sequential++;
	}
	return PHYAMD_OK;
}

int shard_gradient_batch(Shard *e, int flags, int32_t count, const double *branch_lengths, double *lnl, double *cat_gradient) {
	CHECK_ENGINE(e);
	if (count < 1) return fail(PHYAMD_EINVAL, "phyamd_gradient_batch: count must be >= 1 (got %d)", count);
	if (!branch_lengths || !lnl) return fail(PHYAMD_EINVAL, "phyamd_gradient_batch: null branch_lengths or lnl");
	const auto t0 = std::chrono::steady_clock::now();
	int rc;
	if ((rc = bind_device(e))) return rc;
	const std::vector<double> lengths = e->lengths;
	const bool had_lengths = e->have_lengths;
	phyamd_batch_profile prof{};
	rc = run_batch(e, flags, count, branch_lengths, lnl, cat_gradient, prof);
	if (prof.items_sequential > 0 || rc) {  // the ordinary path has set items' lengths: the engine's own go back
		const std::string why = g_last_error;
		if (had_lengths) {
			const int rc2 = shard_set_branch_lengths(e, lengths.data());
			if (!rc) rc = rc2;
			else g_last_error = why;
		} else
			e->have_lengths = false;
	}
	prof.scratch_bytes = (int64_t)batch_scratch_bytes(e);
	prof.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
	e->batch_prof = prof;
	return rc;
}

// ---- a batch of trees (phyamd_gradient_batch_trees) ---------------------------------------------------------------------------

// item `item` of a batch of trees is one binary tree over all 2T - 1 nodes in phyamd_set_topology's convention (build_schedule's
// checks, on the item's arrays)
int validate_batch_tree(int T, const int32_t *left, const int32_t *right, int root, int item, std::vector<int> &parents, std::vector<int> &stack) {
	const int N = 2 * T - 1;
	parents.assign(N, 0);
	for (int n = 0; n < N; n++) {
		const int l = left[n], r = right[n];
		if (n < T) {
			if (l != -1 || r != -1) return fail(PHYAMD_EINVAL, "phyamd_gradient_batch_trees: item %d: node %d is a tip (id < tip_count) but has children", item, n);
			continue;
		}
		if (l < 0 || r < 0 || l >= N || r >= N || l == r)
			return fail(PHYAMD_EINVAL, "phyamd_gradient_batch_trees: item %d: internal node %d has invalid children (%d, %d)", item, n, l, r);
		if (++parents[l] > 1 || ++parents[r] > 1) return fail(PHYAMD_EINVAL, "phyamd_gradient_batch_trees: item %d: node %d or %d has two parents", item, l, r);
	}
	if (root < T || root >= N || parents[root] != 0) return fail(PHYAMD_EINVAL, "phyamd_gradient_batch_trees: item %d: root %d is not a parentless internal node", item, root);
	// (no node has two parents and the root has none: the walk from the root meets no node twice)
	int reached = 0;
	stack.assign(1, root);
	while (!stack.empty()) {
		const int n = stack.back();
		stack.pop_back();
		reached++;
		if (n >= T) {
			stack.push_back(left[n]);
			stack.push_back(right[n]);
		}
	}
	if (reached != N) return fail(PHYAMD_EINVAL, "phyamd_gradient_batch_trees: item %d: the topology is not a single binary tree over all %d nodes", item, N);
	return PHYAMD_OK;
}

// the items of a batch of trees through the batched walk, in chunks of what the scratch holds.  Per chunk: the items' op lists are
// built and uploaded with their roots, the upper slots are those of the chunk's deepest-parking item, three launches
int run_tree_batch(Shard *e, int flags, int32_t count, const int32_t *left, const int32_t *right, const int32_t *roots, const double *branch_lengths, double *lnl,
                   double *cat_gradient, phyamd_batch_profile &prof) {
	int rc;
	{  // ready but for the lengths, which the call brings itself
		const bool had = e->have_lengths;
		e->have_lengths = true;
		rc = check_ready(e);
		e->have_lengths = had;
		if (rc) return rc;
	}
	const bool grad = cat_gradient != nullptr;
	if (const char *why = tree_batch_refusal(e, flags, 1)) return fail(PHYAMD_EUNSUPPORTED, "phyamd_gradient_batch_trees: %s", why);
	if (grad && !e->have_Q) return fail(PHYAMD_EINVAL, "the gradient needs the rate matrix: phyamd_set_eigen or phyamd_set_rate_matrix");
	const int T = e->T;
	const size_t N = (size_t)e->N, ncat = N * e->C, rows = grad ? 1 + ncat : 1, nops = 2 * (size_t)(T - 1);
	std::vector<int> slots(count);  // per item: the upper slots its pre-order list parks in
	{
		std::vector<int> parents, stack;
		for (int32_t b = 0; b < count; b++) {  // every item, before anything is launched
			const int32_t *l = left + (size_t)b * N, *r = right + (size_t)b * N;
			if ((rc = validate_batch_tree(T, l, r, roots[b], b, parents, stack))) return rc;
			slots[b] = grad ? build_batch_ops(T, l, r, roots[b], nullptr) : 1;
		}
	}
	std::vector<double> lengths, out;
	std::vector<BatchOp> ops;
	for (size_t first = 0; first < (size_t)count;) {
		// the chunk and its slot count settle each other: fewer items never need more slots
		size_t items = std::min<size_t>((size_t)count - first, BATCH_MAX_CHUNK);
		BatchShape shape{grad, 1, true};
		for (;;) {
			shape.slots = *std::max_element(slots.begin() + first, slots.begin() + first + items);
			const size_t fit = batch_items_that_fit(e, items, shape);
			if (const char *why = tree_batch_refusal(e, flags, fit)) return fail(PHYAMD_EUNSUPPORTED, "phyamd_gradient_batch_trees: %s", why);
			if (fit >= items) break;
			items = fit;
		}
		if ((rc = ensure_batch_scratch(e, items, shape))) return rc;
		const auto t0 = std::chrono::steady_clock::now();
		ops.clear();
		for (size_t b = first; b < first + items; b++) build_batch_ops(T, left + b * N, right + b * N, roots[b], &ops);
		const auto t1 = std::chrono::steady_clock::now();
		HIP_TRY(hipMemcpyAsync(e->d_batch_item_ops, ops.data(), sizeof(BatchOp) * items * nops, hipMemcpyHostToDevice, e->stream));
		HIP_TRY(hipMemcpyAsync(e->d_batch_roots, roots + first, sizeof(int32_t) * items, hipMemcpyHostToDevice, e->stream));
		HIP_TRY(hipStreamSynchronize(e->stream));  // (ops is reused by the next chunk)
		const auto t2 = std::chrono::steady_clock::now();
		lengths.assign(branch_lengths + first * N, branch_lengths + (first + items) * N);
		out.resize(items * rows);
		for (size_t b = 0; b < items; b++) lengths[b * N + roots[first + b]] = 0.0;  // (ignored, as phyamd_set_branch_lengths does)
		if ((rc = run_batch_chunk(e, flags, (int)items, lengths.data(), shape, out.data()))) return rc;
		if (e->batch_trace) {
			const auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
			std::fprintf(stderr, "phyamd_gradient_batch_trees: chunk %d items %zu slots %d build_ms %.6f upload_ms %.6f\n", prof.chunks, items, shape.slots, ms(t0, t1),
			             ms(t1, t2));
		}
		prof.chunks++;
		for (size_t b = 0; b < items; b++) {
			const double l = out[b * rows];
			const bool bad = std::isnan(l) || std::isinf(l);  // in-band, whatever the rescaling mode: the engine is never switched
			lnl[first + b] = l;
			for (size_t i = 0; grad && i < ncat; i++) cat_gradient[(first + b) * ncat + i] = bad ? NAN : out[b * rows + 1 + i];  // treelikelihood.c:327-332
			prof.items_fast++;
		}
		first += items;
	}
	return PHYAMD_OK;
}

// reads the engine's inputs and writes only the batch scratch: nothing in Shard::state changes
int shard_gradient_batch_trees(Shard *e, int flags, int32_t count, const int32_t *left, const int32_t *right, const int32_t *roots, const double *branch_lengths,
                               double *lnl, double *cat_gradient) {
	CHECK_ENGINE(e);
	if (count < 1) return fail(PHYAMD_EINVAL, "phyamd_gradient_batch_trees: count must be >= 1 (got %d)", count);
	if (!left || !right || !roots || !branch_lengths || !lnl) return fail(PHYAMD_EINVAL, "phyamd_gradient_batch_trees: null left, right, roots, branch_lengths or lnl");
	const auto t0 = std::chrono::steady_clock::now();
	int rc;
	if ((rc = bind_device(e))) return rc;
	phyamd_batch_profile prof{};
	rc = run_tree_batch(e, flags, count, left, right, roots, branch_lengths, lnl, cat_gradient, prof);
	prof.scratch_bytes = (int64_t)batch_scratch_bytes(e);
	prof.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
	e->batch_prof = prof;
	return rc;
}

int shard_get_batch_profile(Shard *e, phyamd_batch_profile *out) {
	CHECK_ENGINE(e);
	if (!out) return fail(PHYAMD_EINVAL, "null out");
	*out = e->batch_prof;
	return PHYAMD_OK;
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
		const int u = e->parent[v];
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

// out [3 terms][3][N] (host): one walk of the engine's tree with every upper parked, the trial matrices, every edge's three
// arrangements in one launch.  Reads the engine's inputs and writes only the batch scratch: nothing in Shard::state changes
int run_nni(Shard *e, int flags, const double *central_lengths, bool deriv, double *out, phyamd_nni_profile &prof) {
	int rc;
	if ((rc = check_ready(e))) return rc;
	if (flags != 0) return fail(PHYAMD_EUNSUPPORTED, "phyamd_nni_log_likelihoods: flags %d (no flags are defined: pass 0)", flags);
	if (const char *why = tree_batch_refusal(e, 0, 1)) return fail(PHYAMD_EUNSUPPORTED, "phyamd_nni_log_likelihoods: %s", why);
	if (!e->have_eigen || !e->have_Q)
		return fail(PHYAMD_EINVAL, "phyamd_nni_log_likelihoods needs the eigen system (phyamd_set_eigen): the trial matrices, d1 and d2 are formed from it");
	const int T = e->T, N = e->N, C = e->C;
	// the trial lengths: a candidate's own three, every other entry the engine's (ignored: no arrangement reads that matrix)
	std::vector<double> trial((size_t)3 * N);
	for (int k = 0; k < 3; k++) std::copy(e->lengths.begin(), e->lengths.end(), trial.begin() + (size_t)k * N);
	for (int v = T; v < N && central_lengths; v++) {
		if (v == e->root) continue;
		for (int k = 0; k < 3; k++) {
			const double t = central_lengths[(size_t)k * N + v];
			if (!std::isfinite(t) || t < 0.0)
				return fail(PHYAMD_EINVAL, "phyamd_nni_log_likelihoods: central_lengths[%d][%d] = %g: a trial length is finite and not negative", k, v, t);
			trial[(size_t)k * N + v] = t;
		}
	}
	const size_t cands = nni_candidates(e);
	prof.candidates = (int32_t)cands;
	std::fill(out, out + (size_t)9 * N, NAN);
	if (cands == 0) return PHYAMD_OK;  // two tips: no internal edge
	const BatchShape shape{true, T - 1, false, true};
	if (batch_items_that_fit(e, 1, shape) < 1)
		return fail(PHYAMD_EUNSUPPORTED, "phyamd_nni_log_likelihoods: the scratch (%zu bytes: every internal node's lower and upper partial) does not fit the memory budget",
		            batch_item_bytes(e, shape));
	if ((rc = ensure_batch_scratch(e, 1, shape)) || (rc = upload_nni_lists(e))) return rc;
	const int nblk = (e->P + WAVE - 1) / WAVE, nops = T - 1;
	HIP_TRY(hipMemcpyAsync(e->d_nni_len, trial.data(), sizeof(double) * trial.size(), hipMemcpyHostToDevice, e->stream));
	const auto matrices = [&](int items, const double *lengths, double *mats) {
		const size_t total = (size_t)items * N * C * 16;
		hipLaunchKernelGGL(k_batch_matrices, dim3((unsigned)std::min<size_t>((total + 255) / 256, 4096)), dim3(256), 0, e->stream, C, N, items, e->d_model, e->d_rates, lengths,
		                   e->root, (const int32_t *)nullptr, mats);
	};
	matrices(1, e->d_lengths, e->d_batch_mats);  // the walk's item: the engine's lengths
	matrices(3, e->d_nni_len, e->d_nni_mats);
	const BatchOp *ops = e->d_nni_ops.get();
	const BatchArgs walk{ops, ops + nops, 0, T, N, e->P, C, nblk, T - 1, 1, e->d_tipmask, e->d_freqs, e->d_props, e->d_weights, e->d_Q, e->d_batch_mats, e->d_batch_lower,
	                     e->d_batch_upper, e->d_batch_lnl, e->d_batch_slab};
	hipLaunchKernelGGL(k_batch_walk4<false>, dim3(nblk, 1), dim3(WAVE, C), 0, e->stream, walk);
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

// an entry whose lnL is not finite reports it in band with NaN derivatives (treelikelihood.c:327-332, per entry); out: [lnl | d1 | d2]
void nni_mask_derivatives(size_t entries, double *out) {
	for (size_t i = 0; i < entries; i++)
		if (std::isnan(out[i]) || std::isinf(out[i])) out[entries + i] = out[2 * entries + i] = NAN;
}

// out [3 terms][3][N] on the host; deriv: d1 and d2 as well (else those rows are NaN at tips and the root, 0 elsewhere)
int shard_nni_log_likelihoods(Shard *e, int flags, const double *central_lengths, bool deriv, double *out) {
	CHECK_ENGINE(e);
	if (!out) return fail(PHYAMD_EINVAL, "phyamd_nni_log_likelihoods: null lnl");
	const auto t0 = std::chrono::steady_clock::now();
	int rc;
	if ((rc = bind_device(e))) return rc;
	phyamd_nni_profile prof{};
	rc = run_nni(e, flags, central_lengths, deriv, out, prof);
	if (!rc) nni_mask_derivatives((size_t)3 * e->N, out);
	prof.scratch_bytes = (int64_t)batch_scratch_bytes(e);
	prof.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
	e->nni_prof = prof;
	return rc;
}

int shard_get_nni_profile(Shard *e, phyamd_nni_profile *out) {
	CHECK_ENGINE(e);
	if (!out) return fail(PHYAMD_EINVAL, "null out");
	*out = e->nni_prof;
	return PHYAMD_OK;
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
	const int u = e->parent[p], s = e->left[u] == p ? e->right[u] : e->left[u];
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
		const int x = e->parent[w];
		cand_of[w] = (int32_t)cands->size();
		cands->push_back(SprCand{row, w, x == e->root ? BATCH_ROOT : x, e->left[x] == w ? e->right[x] : e->left[x], p, {0, 0, 0}});
	}
}

// lnl [count][N] (host).  Reads the engine's inputs and writes only the batch scratch: nothing in Shard::state changes but the
// record that the host lists are the tree's
int run_spr(Shard *e, int flags, int32_t count, const int32_t *prune, double *lnl, phyamd_spr_profile &prof) {
	int rc;
	if ((rc = check_ready(e))) return rc;
	if (flags != 0) return fail(PHYAMD_EUNSUPPORTED, "phyamd_spr_log_likelihoods: flags %d (no flags are defined: pass 0)", flags);
	if (const char *why = tree_batch_refusal(e, 0, 1)) return fail(PHYAMD_EUNSUPPORTED, "phyamd_spr_log_likelihoods: %s", why);
	if (!e->have_eigen) return fail(PHYAMD_EINVAL, "phyamd_spr_log_likelihoods needs the eigen system (phyamd_set_eigen): the half-length matrices are formed from it");
	const int T = e->T, N = e->N, C = e->C, nops = T - 1;
	if (!prune && count != N) return fail(PHYAMD_EINVAL, "phyamd_spr_log_likelihoods: prune is null, so count must be the node count %d (got %d)", N, count);
	std::vector<int32_t> live;  // indices of the rows that have candidates: p is neither the root nor a child of it
	for (int32_t i = 0; i < count; i++) {
		const int p = prune ? prune[i] : i;
		if (p < 0 || p >= N) return fail(PHYAMD_EINVAL, "phyamd_spr_log_likelihoods: prune[%d] = %d is not a node id (0..%d)", i, p, N - 1);
		if (p != e->root && e->parent[p] != e->root) live.push_back(i);
	}
	std::fill(lnl, lnl + (size_t)count * N, NAN);
	prof.prunes = count;
	if (live.empty()) return PHYAMD_OK;
	ensure_spr_lists(e);
	const BatchShape shape{true, T - 1, true, false, true};
	const int nblk = (e->P + WAVE - 1) / WAVE;
	std::vector<double> lengths((size_t)2 * N), out;
	for (int n = 0; n < N; n++) lengths[n] = e->lengths[n], lengths[N + n] = 0.5 * e->lengths[n];
	std::vector<BatchOp> ops;
	std::vector<SprCand> cands;
	std::vector<int32_t> cand_of;
	for (size_t first = 0; first < live.size();) {
		const size_t rows = std::min(batch_items_that_fit(e, live.size() - first, shape), live.size() - first);
		if (rows < 1)
			return fail(PHYAMD_EUNSUPPORTED, "phyamd_spr_log_likelihoods: the scratch of one row (%zu bytes: every internal node's lower and upper partial) does not fit the memory budget",
			            batch_item_bytes(e, shape));
		if ((rc = ensure_batch_scratch(e, rows, shape))) return rc;
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
		const size_t total = (size_t)2 * N * C * 16;  // the engine's lengths, then their halves
		hipLaunchKernelGGL(k_batch_matrices, dim3((unsigned)std::min<size_t>((total + 255) / 256, 4096)), dim3(256), 0, e->stream, C, N, 2, e->d_model, e->d_rates,
		                   e->d_spr_len.get(), e->root, (const int32_t *)nullptr, e->d_spr_mats.get());
		const double *mats = e->d_spr_mats.get(), *half = mats + (size_t)N * C * 16;
		const SprWalkArgs walk{e->d_batch_item_ops.get(), T, N, e->P, C, nblk, e->d_tipmask, mats, e->d_batch_lower, e->d_batch_upper};
		hipLaunchKernelGGL(k_spr_walk4, dim3(nblk, (unsigned)rows), dim3(WAVE, C), 0, e->stream, walk);
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
		first += rows;
	}
	return PHYAMD_OK;
}

int shard_spr_log_likelihoods(Shard *e, int flags, int32_t count, const int32_t *prune, double *lnl) {
	CHECK_ENGINE(e);
	if (count < 1) return fail(PHYAMD_EINVAL, "phyamd_spr_log_likelihoods: count must be >= 1 (got %d)", count);
	if (!lnl) return fail(PHYAMD_EINVAL, "phyamd_spr_log_likelihoods: null lnl");
	const auto t0 = std::chrono::steady_clock::now();
	int rc;
	if ((rc = bind_device(e))) return rc;
	phyamd_spr_profile prof{};
	rc = run_spr(e, flags, count, prune, lnl, prof);
	prof.scratch_bytes = (int64_t)batch_scratch_bytes(e);
	prof.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
	e->spr_prof = prof;
	return rc;
}

int shard_get_spr_profile(Shard *e, phyamd_spr_profile *out) {
	CHECK_ENGINE(e);
	if (!out) return fail(PHYAMD_EINVAL, "null out");
	*out = e->spr_prof;
	return PHYAMD_OK;
}

// ---- per-pattern posteriors (phyamd_state_posteriors, phyamd_site_rate_posteriors) ---------------------------------------------

// The staging arrays of the two calls, and rows of a chunk that fit beside the engine.  per_row[a]: bytes a row takes in array a
// for this call, 0: the call does not use the array -- it is released first, so that what an earlier call left never takes this
// call's room.  An array the call uses is kept where it is large enough (DeviceBuffer::reserve frees only an array it regrows),
// so the arrays are counted at the larger of what they hold and what n rows need: n is the most rows that keep the engine's other
// arrays (the batch scratch not counted: reserve() releases it when an array needs its room), these and a margin within the cap;
// if arrays kept from a roomier time leave no such n, they are released and the rows sized for empty ones.  Without a cap: within
// most of what the device has free right now.  At least one row: if even that does not fit, the allocation reports it
constexpr int POST_ARRAYS = 4;
size_t post_rows_that_fit(Shard *e, size_t count, const size_t (&per_row)[POST_ARRAYS]) {
	DeviceBuffer *const arrays[POST_ARRAYS] = {&e->d_post_rows, &e->d_post_out, &e->d_post_lower, &e->d_post_states};
	size_t row_bytes = 0;
	for (int a = 0; a < POST_ARRAYS; a++) {
		if (per_row[a] == 0) arrays[a]->release();
		row_bytes += per_row[a];
	}
	const size_t most = std::min<size_t>(count, BATCH_MAX_CHUNK);
	const auto held = [&] {
		double h = 0.0;
		for (DeviceBuffer *a : arrays) h += (double)a->bytes();
		return h;
	};
	const auto rows_in = [&](double room) { return (size_t)std::min((double)most, std::max(std::floor(room / (double)row_bytes), 1.0)); };
	if (e->cfg.max_device_bytes <= 0) {
		size_t free_bytes = 0, total_bytes = 0;
		return rows_in(hipMemGetInfo(&free_bytes, &total_bytes) == hipSuccess ? 0.8 * ((double)free_bytes + held()) : 0.0);
	}
	const double room = (double)e->cfg.max_device_bytes - ((double)e->mem.bytes - held() - (double)e->batch_mem.bytes) - 65536.0;
	const size_t n = rows_in(room);
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
	// every partial resident: the engine becomes one with phyamd_set_keep_partials(1) that has run the flags-0 gradient
	if (!e->keep_partials && (rc = shard_set_keep_partials(e, 1))) return rc;
	if ((!uppers_resident(e) || !lowers_current(e)) && (rc = eval_gradient(e, 0))) return rc;
	if ((rc = require_reference_form(e))) return rc;  // (stored partials: the partials themselves, in the reference's form)
	if (!uppers_resident(e) || e->core_index[e->root] < 0) return fail(PHYAMD_EDEVICE, "phyamd_state_posteriors: the gradient left no resident partials");
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
				if (e->upper_slot[node] < 0) return fail(PHYAMD_EDEVICE, "phyamd_state_posteriors: node %d has no resident upper partial", node);
				d.up = e->d_upper + (size_t)e->upper_slot[node] * npd;
			}
			if (node >= e->T) {
				if (e->core_index[node] < 0) return fail(PHYAMD_EDEVICE, "phyamd_state_posteriors: node %d has no resident lower partial", node);
				d.low = e->d_lower + (size_t)e->core_index[node] * npd;
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

// a NaN / inf lnL of the evaluation is reported in band (treelikelihood.c:327-332): NaN posteriors, state 255
void post_mask_rows(double lnl, size_t cells, int S, double *posteriors, uint8_t *states) {
	if (!std::isnan(lnl) && !std::isinf(lnl)) return;
	if (posteriors) std::fill(posteriors, posteriors + cells * S, NAN);
	if (states) std::fill(states, states + cells, (uint8_t)255);
}

// posteriors [P][C] and mean_rates [P] (or null) of this shard's patterns.  Reads the root's stored partial, like
// phyamd_root_frequency_term: whatever is pending is evaluated by a post-order pass, and the engine is afterwards what that pass
// leaves -- the root's array is p_root in every storage convention, only a rescaled evaluation's factors have to be the reference's
int shard_site_rate_posteriors(Shard *e, double *posteriors, double *mean_rates) {
	CHECK_ENGINE(e);
	NOT_TILED(e, "phyamd_site_rate_posteriors (the root partial of every pattern resident)");
	if (!posteriors) return fail(PHYAMD_EINVAL, "phyamd_site_rate_posteriors: null posteriors");
	int rc;
	if ((rc = bind_device(e)) || (rc = check_ready(e))) return rc;
	if ((rc = run_lower(e, 1))) return rc;
	if (e->scaling_on && (rc = require_reference_form(e))) return rc;  // (see shard_root_frequency_term: factors common to the categories)
	if (e->core_index[e->root] < 0 || !e->d_lower) return fail(PHYAMD_EDEVICE, "phyamd_site_rate_posteriors: the root partial is not resident");
	const int P = e->P, C = e->C;
	e->d_post_rows.release(), e->d_post_lower.release(), e->d_post_states.release();  // (what a state call left is not this call's: its room is)
	if ((rc = e->d_post_out.ensure((size_t)P * C + P))) return rc;
	const double *root = e->d_lower + (size_t)e->core_index[e->root] * node_partial_doubles(e);
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
		for (int cur = a, m = e->parent[a];; cur = m, m = e->parent[m]) {
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
	// every partial resident: the engine becomes one with phyamd_set_keep_partials(1) that has run the flags-0 gradient
	if (!e->keep_partials && (rc = shard_set_keep_partials(e, 1))) return rc;
	if ((!uppers_resident(e) || !lowers_current(e)) && (rc = eval_gradient(e, 0))) return rc;
	if (e->scaling_on) return fail(PHYAMD_EUNSUPPORTED, rescaling, name);  // (PHYAMD_RESCALE_AUTO: that evaluation switched)
	if ((rc = require_reference_form(e))) return rc;
	if (!uppers_resident(e) || e->core_index[e->root] < 0) return fail(PHYAMD_EDEVICE, "%s: the gradient left no resident partials", name);

	BhessLists L;
	build_bhess_lists(e, L);
	std::vector<int32_t> lower_of(N), upper_of(N);
	for (int n = 0; n < N; n++) {
		lower_of[n] = n < e->T ? -1 : e->core_index[n];
		upper_of[n] = n == e->root ? 0 : e->upper_slot[n];
		if ((n >= e->T && lower_of[n] < 0) || upper_of[n] < 0) return fail(PHYAMD_EDEVICE, "%s: node %d has no resident partial", name, n);
	}
	const size_t nsteps = L.steps.size(), ntc = L.cousins.size(), nto = L.outer.size(), nn = (size_t)N * N;
	const size_t at_steps = sizeof(BhessStart) * L.starts.size(), at_cousins = at_steps + sizeof(BhessStep) * nsteps, at_outer = at_cousins + sizeof(BhessTile) * ntc,
	             at_lower = at_outer + sizeof(BhessTile) * nto, at_upper = at_lower + sizeof(int32_t) * N, list_bytes = at_upper + sizeof(int32_t) * N;
	// the chunk: whole blocks whose scratch fits beside the engine (batch_items_that_fit's room, the whole scratch group counted free)
	const size_t nblk_all = ((size_t)P + WAVE - 1) / WAVE;
	const double block_bytes = 8.0 * ((double)nsteps * C * WAVE * 4 + 2.0 * WAVE + (double)N * WAVE + (double)(nsteps + 2 * (size_t)N) + 256.0 * (double)(ntc + nto));
	const size_t sums = 2 * nn + 2 * (size_t)N + 2 * (size_t)N * C * 16;
	const double fixed_bytes = 8.0 * (double)sums + (double)list_bytes;
	const double held = (double)batch_scratch_bytes(e);
	double room;
	if (e->cfg.max_device_bytes > 0) {
		const double tile_now = (double)e->tile_mem.bytes, resident = (double)e->mem.bytes - held - tile_now;
		room = (double)e->cfg.max_device_bytes - (resident + 65536.0 + walk_reserve(e) + std::max(tile_now, tile_working_set(e, (double)e->P, true)));
	} else {
		size_t free_bytes = 0, total_bytes = 0;
		room = hipMemGetInfo(&free_bytes, &total_bytes) == hipSuccess ? 0.8 * ((double)free_bytes + held) : 0.0;
	}
	const double fit = std::floor((room - fixed_bytes) / block_bytes);
	if (fit < 1.0)
		return fail(PHYAMD_ENOMEM, "%s: the scratch of one block of 64 patterns (%.0f bytes, and %.0f for the matrix and the lists) does not fit the memory budget", name,
		            block_bytes, fixed_bytes);
	const size_t nblk = (size_t)std::min((double)nblk_all, fit), Pc = nblk * WAVE;
	const size_t n_tan = nsteps * C * Pc * 4, n_rows = 2 * Pc + (size_t)N * Pc + (nsteps + 2 * (size_t)N) * nblk, n_tiles = (ntc + nto) * nblk * 256;
	const bool serves = e->d_bhess_tan.size() >= n_tan && e->d_bhess_rows.size() >= n_rows && e->d_bhess_tiles.size() >= n_tiles && e->d_bhess_sums.size() >= sums &&
	                    e->d_bhess_lists.size() >= list_bytes && e->d_bhess_tan.get();
	if (!serves && e->cfg.max_device_bytes > 0) release_batch_scratch(e);  // (under a cap a call gets exactly its own scratch)
	if ((rc = e->d_bhess_tan.ensure(n_tan)) || (rc = e->d_bhess_rows.ensure(n_rows)) || (rc = e->d_bhess_tiles.ensure(n_tiles)) || (rc = e->d_bhess_sums.ensure(sums)) ||
	    (rc = e->d_bhess_lists.ensure(list_bytes)))
		return rc;

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

// a NaN / inf lnL of the evaluation is reported in band (treelikelihood.c:327-332): every derivative NaN
void bhess_mask(double lnl, size_t N, double *gradient, double *hessian) {
	if (!std::isnan(lnl) && !std::isinf(lnl)) return;
	if (gradient) std::fill(gradient, gradient + N, NAN);
	std::fill(hessian, hessian + N * N, NAN);
}

int shard_branch_hessian(Shard *e, int flags, double *lnl, double *gradient, double *hessian) {
	if (!e) return fail(PHYAMD_EINVAL, "phyamd_branch_hessian: null engine");
	if (!lnl || !hessian) return fail(PHYAMD_EINVAL, "phyamd_branch_hessian: null %s", !lnl ? "lnl" : "hessian");
	if (flags != 0) return fail(PHYAMD_EINVAL, "phyamd_branch_hessian: flags %d (no flags are defined: pass 0)", flags);
	const auto t0 = std::chrono::steady_clock::now();
	int rc;
	if ((rc = bind_device(e))) return rc;
	phyamd_hessian_profile prof{};
	prof.pairs = (int64_t)(e->N - 1) * e->N / 2;
	rc = run_branch_hessian(e, lnl, gradient, hessian, prof);
	if (!rc) bhess_mask(*lnl, (size_t)e->N, gradient, hessian);
	prof.scratch_bytes = (int64_t)batch_scratch_bytes(e);
	prof.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
	e->bhess_prof = prof;
	return rc;
}

int shard_get_hessian_profile(Shard *e, phyamd_hessian_profile *out) {
	CHECK_ENGINE(e);
	if (!out) return fail(PHYAMD_EINVAL, "null out");
	*out = e->bhess_prof;
	return PHYAMD_OK;
}
