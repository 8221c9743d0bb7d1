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
ScheduleCounts schedule_counts(const Schedule &s) {
	ScheduleCounts c{s.core_count, std::max(s.upper_slots, s.walk_upper_slots), 1};
	for (size_t i = 0; i + 1 < s.lower_level_off.size(); i++) c.widest = std::max(c.widest, s.lower_level_off[i + 1] - s.lower_level_off[i]);
	for (size_t i = 0; i + 1 < s.upper_level_off.size(); i++) c.widest = std::max(c.widest, s.upper_level_off[i + 1] - s.upper_level_off[i]);
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
	const double now = tile_working_set(e, p, exact, schedule_counts(e->sched));
	return e->have_scaled_counts ? std::max(now, tile_working_set(e, p, exact, e->scaled_counts)) : now;
}

// buffers the 4-state walks make on demand whose size does not follow the tile (whether or not the engine may rescale): the streamed walks' table blocks ([C][ops], ops < N)
// and the pre-order walk's per-op scratch (d_oct: 8 C R doubles, R < N).  What is held already counts in device_bytes.
double walk_reserve(const Shard *e) {
	if (e->S != 4) return 0.0;
	return std::max(0.0, (double)e->N * e->C * OPBLK_BYTES - (double)e->d_optab.size()) + std::max(0.0, 8.0 * (8.0 * e->C * e->N - (double)e->d_oct.size()));
}

// Room for a query call's scratch beside the engine (phyamd_queries.inc), `held` being what the call's own arrays hold already and
// may reuse: within the cap less what the engine holds or may still allocate, or, without a cap, within most of what the device
// has free right now.  What the engine may still allocate is the caller's to say:
//   MayGrow   the call can run on any engine (the batch, NNI and SPR calls; the Hessian sizes its chunk the same way): what is
//             resident whatever the tile size, the tile's working set as choose_tiles reserves it, the walks' on-demand buffers
//   Resident  the posterior calls, which run right after a keep-partials gradient has allocated everything the engine needs and
//             stage into arrays of the engine's own budget: nothing is reserved, and the batch scratch counts as free, because an
//             array outside that group has it released when it needs the room (DeviceBuffer::reserve)
enum class EngineRoom { MayGrow, Resident };
double scratch_room(const Shard *e, double held, EngineRoom engine) {
	if (e->cfg.max_device_bytes <= 0) {
		size_t free_bytes = 0, total_bytes = 0;
		return hipMemGetInfo(&free_bytes, &total_bytes) == hipSuccess ? 0.8 * ((double)free_bytes + held) : 0.0;
	}
	if (engine == EngineRoom::Resident) return (double)e->cfg.max_device_bytes - ((double)e->mem.bytes - held - (double)e->batch_mem.bytes) - 65536.0;
	const double tile_now = (double)e->tile_mem.bytes, resident = (double)e->mem.bytes - held - tile_now;
	return (double)e->cfg.max_device_bytes - (resident + 65536.0 + walk_reserve(e) + std::max(tile_now, tile_working_set(e, (double)e->P, true)));
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
	if (const char *env = std::getenv("PHYAMD_STREAM_ELIDE")) e->stream_elide_on = std::atoi(env) != 0;
	if (const char *env = std::getenv("PHYAMD_STREAM_PAIRS")) e->stream_pairs_on = std::atoi(env) != 0;
	if (const char *env = std::getenv("PHYAMD_STREAM_KEEP")) e->stream_keep_on = std::atoi(env) != 0;
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
	if (weights != e->weights_host.data()) e->weights_host.assign(weights, weights + e->Ptot);
	e->weights_epoch++;
	e->have_weights = true;
	input_changed(e, Input::PatternWeights);
	return PHYAMD_OK;
}

int upload_lengths(Shard *e);  // (below)

int shard_set_topology(Shard *e, const int32_t *left, const int32_t *right, int root) {
	CHECK_ENGINE(e);
	if (!left || !right) return fail(PHYAMD_EINVAL, "null topology arrays");
	int rc;
	if ((rc = bind_device(e))) return rc;
	e->batch_mem.release_all();  // (sized by the old tree; the tile plan below counts what the engine itself holds)
	lowers_discarded(e);         // (whichever way this call ends: every partial belongs to the old tree or to a schedule put back)
	// the new tree's schedule from the caller's arrays: a refused tree changes nothing.  The lazy switch rebuilds the 20 / 60 /
	// 61-state schedule without fringe fusion or tree walk (more stored nodes and upper slots): the tiles are sized for that
	// schedule too, so that the switch never needs more than the cap
	const TreeRef tree{e->T, left, right, root};
	ScheduleOptions options = schedule_options(e);
	Schedule other = std::move(e->sched_spare);  // (built into the lists the last call replaced: a topology change per MCMC move allocates nothing)
	const std::string err = build_schedule(tree, options, &other);
	if (!err.empty()) return fail(PHYAMD_EINVAL, "%s", err.c_str());
	e->have_scaled_counts = e->generic && e->cfg.rescale == PHYAMD_RESCALE_AUTO && !e->scaling_on;
	if (e->have_scaled_counts) {
		Schedule rescaled;
		options.scaling_on = true;
		build_schedule(tree, options, &rescaled);  // (the tree has passed the check)
		e->scaled_counts = schedule_counts(rescaled);
	}
	// tree and schedule are installed together; the old ones wait in other_* for a failure further down, which leaves the engine on
	// the tree it had (host lists, device op tables) -- or, if that cannot be re-established, without a topology, so that the next
	// evaluation is refused instead of walking half-updated tables
	std::vector<int32_t> other_l(left, left + e->N), other_r(right, right + e->N);
	int other_root = root;
	const int old_root = e->root;
	auto exchange = [&] {
		e->left.swap(other_l);
		e->right.swap(other_r);
		std::swap(e->root, other_root);
		std::swap(e->sched, other);
	};
	exchange();
	const bool had_topology = e->have_topology;
	auto roll_back = [&](int code) {
		const std::string why = g_last_error;
		exchange();
		if (had_topology) {  // the old schedule as a build leaves it: stored nodes in id order (a store may have moved them)
			int next = 0;
			for (int32_t &slot : e->sched.core_index)
				if (slot >= 0) slot = next++;
			refresh_op_cores(e->sched);
			if (upload_schedule(e) != PHYAMD_OK) e->have_topology = false;
		}
		g_last_error = why;
		return code;
	};
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
	e->sched_spare = std::move(other);
	// lengths go by node id: the branch above the old root's id is the one the caller sent for that id, the new root's is ignored
	if (e->have_lengths && (!had_topology || root != old_root) && (rc = upload_lengths(e))) return rc;
	input_changed(e, Input::Topology);
	return PHYAMD_OK;
}

int shard_set_branch_lengths(Shard *e, const double *lengths) {
	CHECK_ENGINE(e);
	if (!lengths) return fail(PHYAMD_EINVAL, "null lengths");
	int rc;
	if ((rc = bind_device(e))) return rc;
	e->lengths_sent.assign(lengths, lengths + e->N);
	if ((rc = upload_lengths(e))) return rc;
	e->have_lengths = true;
	input_changed(e, Input::BranchLengths);
	return PHYAMD_OK;
}

// the caller's lengths with the entry at the root's id zeroed (the kernels skip the root; the batch calls copy the vector) -> device
int upload_lengths(Shard *e) {
	e->lengths = e->lengths_sent;
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
	return PHYAMD_OK;
}

int shard_set_branch_length(Shard *e, int node, double length) {
	CHECK_ENGINE(e);
	if (!e->have_topology || !e->have_lengths) return fail(PHYAMD_EINVAL, "phyamd_set_topology and phyamd_set_branch_lengths come first");
	if (node < 0 || node >= e->N || node == e->root) return fail(PHYAMD_EINVAL, "node %d has no branch", node);
	int rc;
	if ((rc = bind_device(e))) return rc;
	if (e->lengths[node] == length) return PHYAMD_OK;
	e->lengths[node] = e->lengths_sent[node] = length;
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
		const size_t npd = node_partial_doubles(e), want = (size_t)std::max(1, e->sched.core_count) * 2;
		const size_t live = std::min(lower_slots(e), (size_t)std::max(1, e->sched.core_count));
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
	st.lengths = e->lengths_sent;
	st.model = e->model;
	st.freqs = e->freqs;
	st.rates = e->rates;
	st.props = e->props;
	st.have_eigen = e->have_eigen;
	st.scaling_on = e->scaling_on;
	st.core_index = e->sched.core_index;
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
			if (e->sched.core_index[n] != st.core_index[n]) {
				e->sched.core_index[n] = st.core_index[n];
				moved = true;
			}
		if (moved) {
			refresh_op_cores(e->sched);
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
	if (e->tiles == 1 && (!lowers_current(e) || e->sched.core_index[e->root] < 0 || !e->d_lower)) return fail(PHYAMD_EINVAL, "no evaluation has been run yet");
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
	st.kind = e->sched.node_kind[s];
	st.node = s;
	st.core = e->sched.core_index[s];
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
	for (int a = node; a >= 0; a = e->sched.parent[a]) path.push_back(a);
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
		if (node >= e->T && e->sched.core_index[node] < 0) {  // fringe / DEEP node: its own partial is not stored either
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
			const double *sp = sib < e->T ? nullptr : e->d_lower + (size_t)e->sched.core_index[sib] * npd;  // a stored node: t = P p (k_lower_gen)
			int carried = 1;
			if (sib >= e->T && e->sched.core_index[sib] < 0) {  // a fused cherry: its partial is formed on the side (d_path_lower is free until the end)
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
		up = e->d_upper + (size_t)e->sched.upper_slot[node] * npd;
		low = node < e->T ? nullptr : e->d_lower + (size_t)e->sched.core_index[node] * npd;
		fold = e->upper_fold ? 1 : 0;
	} else {
		if ((rc = run_lower(e, true))) return rc;
		if (e->state.path_node != node && (rc = rebuild_path_upper(e, node))) return rc;
		up = e->d_path_upper;
		low = node < e->T ? nullptr : (e->sched.core_index[node] >= 0 ? e->d_lower + (size_t)e->sched.core_index[node] * npd : e->d_path_lower);
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
		if (!lowers_current(e) || e->sched.core_index[e->root] < 0 || !e->d_lower) return fail(PHYAMD_EINVAL, "no evaluation has been run yet");
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
	if (!upper && e->sched.core_index[node] < 0)
		return fail(PHYAMD_EINVAL, "node %d is fused into its parent (cherry / cherry+tip) and not stored: shard_set_keep_partials(1) first", node);
	const double *src = upper ? e->d_upper + (size_t)e->sched.upper_slot[node] * np : e->d_lower + (size_t)e->sched.core_index[node] * np;
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
	const bool from_Q = derivative && e->explicit_host[node];  // (k_transition_matrices skips the node: d_dmats holds nothing of it)
	if (from_Q && !e->have_Q)
		return fail(PHYAMD_EINVAL, "node %d has explicit matrices: their derivative is Q P, which needs phyamd_set_rate_matrix or phyamd_set_eigen", node);
	HIP_TRY(hipMemcpyAsync(out, (derivative && !from_Q ? e->d_dmats : e->d_mats) + (size_t)node * sz, sizeof(double) * sz, hipMemcpyDeviceToHost, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream));
	if (from_Q) {  // the only derivative the engine defines for such a node: Q P per category, without r_c like the eigen nodes' rows
		const int S = e->S;
		std::vector<double> P(out, out + sz);
		for (int c = 0; c < e->C; c++)
			for (int i = 0; i < S; i++)
				for (int j = 0; j < S; j++) {
					double v = 0.0;
					for (int k = 0; k < S; k++) v += e->Q_host[(size_t)i * S + k] * P[((size_t)c * S + k) * S + j];
					out[((size_t)c * S + i) * S + j] = v;
				}
	}
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
