// phyamd_launch.inc -- kernel launches of the post-order and pre-order passes (4 states and 20 / 60 / 61 states)
// (part of phyamd_engine.hip: one translation unit, internal linkage)

size_t gen_image_doubles(const Shard *e) {
	return e->S == 20 ? MatImage<2, 5>::SIZE : e->S == 60 ? MatImage<4, 15>::SIZE : MatImage<4, 16>::SIZE;
}

template <int RT, int KT>
void launch_matrix_images(Shard *e, int count, const double *src, double *dst, const double *rowscale) {
	hipLaunchKernelGGL((k_matrix_images<RT, KT>), dim3(count), dim3(256), 0, e->stream, e->S, src, dst, rowscale);
}

void build_matrix_images(Shard *e, int count, const double *src, double *dst, const double *rowscale = nullptr) {
	if (e->S == 20) launch_matrix_images<2, 5>(e, count, src, dst, rowscale);
	else if (e->S == 60) launch_matrix_images<4, 15>(e, count, src, dst, rowscale);
	else launch_matrix_images<4, 16>(e, count, src, dst, rowscale);
}

int update_matrices(Shard *e) {
	if (e->generic && e->state.qimg_dirty && e->have_Q && e->have_freqs) {  // images of Q and of diag(pi) Q behind the per-(node, category) ones
		build_matrix_images(e, 1, e->d_Q, e->d_imgs + (size_t)e->N * e->C * gen_image_doubles(e));
		build_matrix_images(e, 1, e->d_Q, e->d_imgs + ((size_t)e->N * e->C + 1) * gen_image_doubles(e), e->d_freqs);
		HIP_TRY(hipGetLastError());
		q_images_rebuilt(e);
	}
	if (!e->state.matrices_dirty) return PHYAMD_OK;
	if (e->have_eigen) {
		const size_t total = (size_t)e->N * e->C * e->S * e->S;
		const int blocks = (int)std::min<size_t>((total + 255) / 256, 4096);
		hipLaunchKernelGGL(k_transition_matrices, dim3(blocks), dim3(256), 0, e->stream, e->S, e->C, e->N, e->d_model, e->d_rates, e->d_lengths,
		                   e->d_explicit, e->root, e->d_mats, e->d_dmats);
		HIP_TRY(hipGetLastError());
	}
	if (!e->generic) {  // explicit matrices included: the tables are built from whatever d_mats holds
		const int n = e->T * e->C * 64;
		hipLaunchKernelGGL(k_tip_tables, dim3((n + 255) / 256), dim3(256), 0, e->stream, e->T, e->C, e->d_mats, e->d_tiptab);
		HIP_TRY(hipGetLastError());
	} else {
		build_matrix_images(e, e->N * e->C, e->d_mats, e->d_imgs);
		HIP_TRY(hipGetLastError());
	}
	matrices_rebuilt(e);
	return PHYAMD_OK;
}

// 20 / 60 / 61 states: p_node itself into `out` (planes [C][S][Pp]) -- the stored array of a node is t = P p (k_lower_gen); the root's
// is its partial.  `side`: a second buffer of the same size for fused cherries below the node (formed on the way)
int true_lower_gen(Shard *e, int node, double *out, double *side) {
	const size_t npd = node_partial_doubles(e), msz = (size_t)e->C * e->S * e->S;
	if (node == e->root && e->sched.core_index[node] >= 0) {
		HIP_TRY(hipMemcpyAsync(out, e->d_lower + (size_t)e->sched.core_index[node] * npd, sizeof(double) * npd, hipMemcpyDeviceToDevice, e->stream));
		return PHYAMD_OK;
	}
	int mode[2];
	const double *src[2];
	const int ch[2] = {e->left[node], e->right[node]};
	const dim3 grid((e->P + 255) / 256);
	for (int q = 0; q < 2; q++) {
		const int n = ch[q];
		if (n < e->T) {
			mode[q] = 0;
			src[q] = nullptr;
		} else if (e->sched.core_index[n] >= 0) {
			mode[q] = 1;
			src[q] = e->d_lower + (size_t)e->sched.core_index[n] * npd;
		} else {  // a fused cherry: two tips
			const int l = e->left[n], r = e->right[n];
			if (l >= e->T || r >= e->T || !side) return fail(PHYAMD_EINVAL, "node %d is neither stored nor a fused cherry", n);
			double *dst = side + (q ? npd : 0);
			hipLaunchKernelGGL(k_node_lower_gen, grid, dim3(256), 0, e->stream, e->P, e->Pp, e->S, e->C, 0, e->d_mats + (size_t)l * msz, (const double *)nullptr,
			                   e->d_tipmask + (size_t)l * e->P, 0, e->d_mats + (size_t)r * msz, (const double *)nullptr, e->d_tipmask + (size_t)r * e->P, e->d_tipsets, 0, dst);
			mode[q] = 2;
			src[q] = dst;
		}
	}
	hipLaunchKernelGGL(k_node_lower_gen, grid, dim3(256), 0, e->stream, e->P, e->Pp, e->S, e->C, mode[0], e->d_mats + (size_t)ch[0] * msz, src[0],
	                   ch[0] < e->T ? e->d_tipmask + (size_t)ch[0] * e->P : (const uint8_t *)nullptr, mode[1], e->d_mats + (size_t)ch[1] * msz, src[1],
	                   ch[1] < e->T ? e->d_tipmask + (size_t)ch[1] * e->P : (const uint8_t *)nullptr, e->d_tipsets, e->scaling_on ? 1 : 0, out);
	HIP_TRY(hipGetLastError());
	return PHYAMD_OK;
}

// Images of Qf P(t) for every (tip, category) -- Qf = Q when pi is folded into the uppers, else diag(pi) Q: the pre-order kernels take
// the branch term of a tip child, sum_i u_i (Qf P e_code)_i, from a column of that product instead of forming Qf . (P e_code)
int ensure_tip_rate_products(Shard *e, bool fold) {
	const int kind = fold ? 0 : 1;
	if (e->state.qp_kind == kind) return PHYAMD_OK;
	const size_t count = (size_t)e->T * e->C;  // (d_qp_mats, d_qp_imgs: allocated with the engine, phyamd_create)
	hipLaunchKernelGGL(k_tip_rate_products, dim3((unsigned)count), dim3(256), 0, e->stream, e->S, e->d_mats, e->d_Q, fold ? (const double *)nullptr : e->d_freqs,
	                   e->d_qp_mats);
	build_matrix_images(e, (int)count, e->d_qp_mats, e->d_qp_imgs);
	HIP_TRY(hipGetLastError());
	tip_rate_products_rebuilt(e, kind);
	return PHYAMD_OK;
}

dim3 block_dims(const Shard *e) { return dim3(WAVE, e->C, e->G); }

// launch(W) with the wave bound W of a workgroup of `waves` waves as a template argument: 4, 8 or 16 (so that small groups are not
// register-capped for 1024 threads)
template <typename F>
int by_waves(int waves, F launch) {
	if (waves <= 4) return launch(std::integral_constant<int, 4>());
	if (waves <= 8) return launch(std::integral_constant<int, 8>());
	return launch(std::integral_constant<int, 16>());
}

// Workgroups the card runs at once for one kernel (occupancy x CUs), asked once per kernel instantiation and device.
template <typename K>
int resident_workgroups(Shard *e, K kernel, int threads, size_t lds) {
	int per_cu = 0, cus = 0;
	if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void *>(kernel), threads, lds) != hipSuccess || per_cu < 1) per_cu = 1;
	if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, e->device) != hipSuccess || cus < 1) cus = 256;
	return per_cu * cus;
}


// which instantiation a 4-state pass launched (phyamd_get_pass_profile): the launchers call these where they have picked it
void record_lower_pass(Shard *e, PassKernel family, int scale, bool ambiguous, bool incremental, int waves, int ppt) {
	phyamd_pass_profile &p = e->pass_prof;
	p.lower_family = (int)family, p.lower_form = (int)e->lower_form, p.lower_scale = scale, p.lower_ambiguous = ambiguous;
	p.lower_incremental = incremental, p.lower_waves = waves, p.lower_ppt = ppt;
}
struct UpperPass { int scale = 0; bool ambiguous = false; int waves = 0; bool tf = false, fold = false, compat = false, params = false, catblk = false; int pair_ops = 0; };
void record_upper_pass(Shard *e, PassKernel family, const UpperPass &u) {
	phyamd_pass_profile &p = e->pass_prof;
	p.upper_family = (int)family, p.upper_scale = u.scale, p.upper_ambiguous = u.ambiguous, p.upper_waves = u.waves, p.upper_tf = u.tf;
	p.upper_fold = u.fold, p.upper_compat = u.compat, p.upper_params = u.params, p.upper_catblk = u.catblk, p.upper_pair_ops = u.pair_ops;
}

template <int WAVES, bool SCALE>
int launch_lower_levels(Shard *e) {
	const std::vector<int> &level_off = *e->act_level_off;  // all core nodes, or only the dirty ones (incremental update)
	const int levels = (int)level_off.size() - 1;
	int launched = 0;
	const size_t lds = sizeof(double) * ((size_t)4 * e->G * e->C * WAVE + e->G);
	for (int lv = 0; lv < levels; lv++) {
		const int off = level_off[lv], cnt = level_off[lv + 1] - off;
		if (cnt == 0) continue;
		const bool is_root = lv == levels - 1;
		dim3 grid(e->nblk_lower, cnt);
		launched++;
		if (is_root)
			hipLaunchKernelGGL((k_lower4<WAVES, SCALE, true>), grid, block_dims(e), lds, e->stream, e->act_lower_ops + off, e->T, e->P, e->C,
			                   e->d_tipmask, e->d_lower, e->d_mats, e->d_tiptab, e->d_lscale, e->d_freqs, e->d_props, e->d_weights, e->d_plk, e->d_wl,
			                   e->d_lnl_part);
		else
			hipLaunchKernelGGL((k_lower4<WAVES, SCALE, false>), grid, block_dims(e), SCALE ? lds : 0, e->stream, e->act_lower_ops + off, e->T, e->P,
			                   e->C, e->d_tipmask, e->d_lower, e->d_mats, e->d_tiptab, e->d_lscale, e->d_freqs, e->d_props, e->d_weights, e->d_plk, e->d_wl,
			                   e->d_lnl_part);
	}
	HIP_TRY(hipGetLastError());
	e->prof.lower_launches = launched;
	e->lnl_blocks = e->nblk_lower;
	e->lnl_per_block = false;
	record_lower_pass(e, PassKernel::Levels, SCALE, false, e->act_level_off == &e->inc_level_off, WAVES, 0);
	return PHYAMD_OK;
}

template <int WAVES, bool SCALE, int PPT>
void launch_lower_walk_ppt(Shard *e, size_t lds) {
	const int nb = (e->nblk_walk_upper + PPT - 1) / PPT;  // nblk_walk_upper = workgroups at one pattern per thread
	e->lnl_blocks = nb * PPT * e->G;  // one entry per block of 64 patterns (a trailing all-padding block adds 0)
	e->lnl_per_block = true;
	lds += sizeof(double) * ((size_t)(e->G & 1) + (size_t)e->G * e->C * PPT * 4 * WAVE);  // + one park slot per wave and pattern group (LPARK)
	// the chunked list: every cut subtree as workgroups of its own (blockIdx.y), then the top part with the root
	const int subtrees = (int)e->sched.walk_lower_chunk_off.size() - 2;
	for (int phase = subtrees > 0 ? 0 : 1; phase < 2; phase++)
		hipLaunchKernelGGL((k_lower4_walk<WAVES, PPT, SCALE>), dim3(nb, phase ? 1 : subtrees), block_dims(e), lds, e->stream, e->d_walk_lower_chunk_ops,
		                   (int)e->sched.walk_lower_chunk_ops.size(), e->T, e->P, e->C, e->d_tipmask, e->d_lower, e->d_mats, e->d_tiptab, e->d_lscale, e->d_freqs,
		                   e->d_props, e->d_weights, e->d_plk, e->d_wl, e->d_lnl_part, (const int *)e->d_walk_lower_chunk_off, phase ? std::max(0, subtrees) : 0,
		                   phase);
	e->prof.lower_launches = subtrees > 0 ? 2 : 1;
	record_lower_pass(e, PassKernel::Walk, SCALE, false, false, WAVES, PPT);
}

template <int WAVES, bool SCALE>
int launch_lower_walk(Shard *e) {
	const size_t lds = sizeof(double) * ((size_t)e->G * e->C * WAVE * (SCALE ? 3 : 1) + e->G);
	// rescaled walks take one pattern per thread: the cross-category exchange costs a workgroup barrier per op and pattern slot
	// (two per thread: 19.1 ms, one: 16.7 ms at 1000 taxa x 1e6 patterns).  The plain walk measures the same either way on a
	// full card, so it takes whichever needs fewer rounds of resident workgroups (a workgroup's walk takes as long whatever
	// shares its CU): two per thread make a 125k-pattern shard ONE round of 977 workgroups instead of two of 1954 (1.9 vs 2.1 ms).
	int ppt = 1;
	if (!SCALE) {
		const size_t park = sizeof(double) * ((size_t)(e->G & 1) + (size_t)e->G * e->C * 4 * WAVE);
		const int threads = e->C * e->G * WAVE;  // the block that is launched (block_dims), not the template's bound
		if (e->lower_walk_slots[0] == 0) {  // (reset with the pattern storage: the launch shape follows G and C)
			e->lower_walk_slots[0] = resident_workgroups(e, k_lower4_walk<WAVES, 1, SCALE>, threads, lds + park);
			e->lower_walk_slots[1] = resident_workgroups(e, k_lower4_walk<WAVES, 2, SCALE>, threads, lds + 2 * park);
		}
		const long slots1 = e->lower_walk_slots[0], slots2 = e->lower_walk_slots[1];
		const long g = e->nblk_walk_upper, r1 = (g + slots1 - 1) / slots1, r2 = 2 * (((g + 1) / 2 + slots2 - 1) / slots2);
		ppt = (r2 <= r1 || g <= slots1) ? 2 : 1;  // (less than one round either way: two per thread measure 7 % better at 1e5 patterns)
	}
	if (ppt == 1) launch_lower_walk_ppt<WAVES, SCALE, 1>(e, lds);
	else launch_lower_walk_ppt<WAVES, SCALE, 2>(e, lds);
	HIP_TRY(hipGetLastError());
	return PHYAMD_OK;
}

template <int WAVES>
int launch_lower_w(Shard *e, PassKernel k) {
	if (k == PassKernel::Walk) return e->scaling_on ? launch_lower_walk<WAVES, true>(e) : launch_lower_walk<WAVES, false>(e);
	return e->scaling_on ? launch_lower_levels<WAVES, true>(e) : launch_lower_levels<WAVES, false>(e);
}

template <typename K>
int allow_big_lds(K kernel, size_t bytes) {
	if (bytes > 64 * 1024) HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
	return PHYAMD_OK;
}

// one pre-order pass.  PARAMS: also accumulate the substitution-parameter sums of parameters [p0, p0 + pc)
template <int WAVES, bool SCALE, bool FOLD, bool COMPAT, bool PARAMS>
int launch_upper_levels(Shard *e, int p0 = 0, int pc = 0) {
	const int levels = (int)e->sched.upper_level_off.size() - 1;
	int launched = 0;
	const size_t nw = (size_t)e->G * e->C, nacc = NACC + (PARAMS ? pc : 0);
	const size_t lds = sizeof(double) * ((SCALE ? 6 * nw * WAVE : 0) + nw * nacc * WAVE + nw * nacc);
	int rc;
	if ((rc = check_reference_form(e, "k_upper4"))) return rc;
	if ((rc = allow_big_lds(k_upper4<WAVES, SCALE, FOLD, COMPAT, PARAMS, false>, lds))) return rc;
	const int op_total = (int)e->sched.upper_ops.size();
	const double *dpm = PARAMS ? e->d_dpm + (size_t)p0 * e->N * e->C * 16 : nullptr;
	const double *dptab = PARAMS ? e->d_dptab + (size_t)p0 * e->T * e->C * 64 : nullptr;
	double *ppart = PARAMS ? e->d_ppart + (size_t)p0 * op_total * e->nblk : nullptr;
	for (int lv = 0; lv < levels; lv++) {
		const int off = e->sched.upper_level_off[lv], cnt = e->sched.upper_level_off[lv + 1] - off;
		if (cnt == 0) continue;
		dim3 grid(e->nblk, cnt);
		launched++;
		hipLaunchKernelGGL((k_upper4<WAVES, SCALE, FOLD, COMPAT, PARAMS, false>), grid, block_dims(e), lds, e->stream, e->d_upper_ops + off, e->T, e->P, e->C,
		                   e->d_tipmask, e->d_lower, e->d_upper, e->d_mats, e->d_tiptab, e->d_Q, e->d_freqs, e->d_props, e->d_weights, e->d_wl, e->d_gpart,
		                   e->nblk, dpm, dptab, pc, e->N, ppart, off, op_total, (const double *)nullptr, (const int *)nullptr, (double *)nullptr);
	}
	HIP_TRY(hipGetLastError());
	e->prof.upper_launches = launched;
	UpperPass u;
	u.scale = SCALE, u.waves = WAVES, u.fold = FOLD, u.compat = COMPAT, u.params = PARAMS;
	record_upper_pass(e, PassKernel::Levels, u);
	return PHYAMD_OK;
}

// ---- every branch's first and second derivative (phyamd_branch_hessian_diagonal): the level pre-order pass, HESS form ----
// LDS of one k_upper4<HESS> workgroup (C waves): the rescaled form's exchanges, the 2 NACC branch-term columns, 2 ceil(NACC / C)
// accumulator columns and their lane sums
void bisect_blocks(int lo, int hi, int levels, std::vector<int> &bounds);

size_t hess_lds(const Shard *e) {
	const size_t nw = (size_t)e->C, nacc = 2 * (size_t)((NACC + e->C - 1) / e->C);
	return sizeof(double) * ((6 + 2 * NACC) * nw * WAVE + nw * nacc * WAVE + nw * nacc);
}

// Workgroups of the HESS pass: the canonical 64-pattern block range [0, ceil(P / 64)) is bisected like reduce_block_sums does, and
// every segment is cut into workgroups of at most PPT_UPPER blocks from its own start.  A shard cut by the same bisection holds
// whole segments with the same workgroups, so the slab entries, their segment sums and the pairwise additions on top are the
// same whatever the shard count.  Device: d_hess_tab = [nwg][2] block ranges | [segments + 1] first workgroup of each segment;
// d_hess = slab [nwg][2 N] | segment sums [8][2 N] | result [1 + 2 N] | tile total [1 + 2 N].
int ensure_hess_storage(Shard *e) {
	if (e->d_hess && e->hess_P == e->P && e->hess_levels == e->reduce_levels) return PHYAMD_OK;
	const int nb = (e->P + WAVE - 1) / WAVE, segments = 1 << e->reduce_levels;
	std::vector<int> bounds, wg, first;
	bisect_blocks(0, nb, e->reduce_levels, bounds);
	bounds.push_back(nb);
	for (int o = 0; o < segments; o++) {
		first.push_back((int)wg.size() / 2);
		for (int b = bounds[o]; b < bounds[o + 1]; b += PPT_UPPER) {
			wg.push_back(b);
			wg.push_back(std::min(b + PPT_UPPER, bounds[o + 1]));
		}
	}
	const int nwg = (int)wg.size() / 2;
	first.push_back(nwg);
	wg.insert(wg.end(), first.begin(), first.end());
	e->d_hess_tab.release();
	e->d_hess.release();
	e->hess_P = -1;
	int rc;
	const size_t R = (size_t)2 * e->N, need = (size_t)nwg * R + 8 * R + 2 * (R + 1);
	if ((rc = e->d_hess_tab.ensure(wg.size())) || (rc = e->d_hess.ensure(need))) return rc;
	HIP_TRY(hipMemcpyAsync(e->d_hess_tab, wg.data(), sizeof(int) * wg.size(), hipMemcpyHostToDevice, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream));  // (wg is a stack-lifetime buffer)
	e->hess_nwg = nwg;
	e->hess_P = e->P;
	e->hess_levels = e->reduce_levels;
	return PHYAMD_OK;
}
double *hess_result(const Shard *e) { return e->d_hess + (size_t)e->hess_nwg * 2 * e->N + (size_t)8 * 2 * e->N; }
double *hess_total(const Shard *e) { return hess_result(e) + 1 + (size_t)2 * e->N; }

// the HESS slab's segment sums, added pairwise (reduce_block_sums' order) -> out[1 ..], and lnL of the post-order pass -> out[0]
int finish_hess_slab(Shard *e, double *out, int launched) {
	const int R = 2 * e->N, segments = 1 << e->reduce_levels;
	double *seg = e->d_hess + (size_t)e->hess_nwg * R;
	hipLaunchKernelGGL(k_slab_segments, dim3((R + 31) / 32, 1, segments), dim3(256), 0, e->stream, e->d_hess, 1, R, (const int *)e->d_hess_tab + 2 * e->hess_nwg, seg);
	hipLaunchKernelGGL(k_slab_finish, dim3((R + 255) / 256), dim3(256), 0, e->stream, seg, segments, 1, R, (const int *)nullptr, out + 1);
	HIP_TRY(hipMemcpyAsync(out, e->d_result, sizeof(double), hipMemcpyDeviceToDevice, e->stream));
	HIP_TRY(hipGetLastError());
	e->prof.upper_launches = launched;
	return PHYAMD_OK;
}

// one HESS pre-order pass over the stored lowers (reference form) -> out[1 + 2 N] = [lnL | d1 | d2], sums over this engine's patterns
template <int WAVES, bool SCALE>
int launch_upper_hess(Shard *e, double *out) {
	const int levels = (int)e->sched.upper_level_off.size() - 1, R = 2 * e->N;
	const size_t lds = hess_lds(e);
	int rc;
	if ((rc = check_reference_form(e, "k_upper4"))) return rc;
	if ((rc = allow_big_lds(k_upper4<WAVES, SCALE, false, false, false, true>, lds))) return rc;
	const int op_total = (int)e->sched.upper_ops.size();
	HIP_TRY(hipMemsetAsync(e->d_hess, 0, sizeof(double) * (size_t)e->hess_nwg * R, e->stream));  // (the root's entries stay zero)
	int launched = 0;
	for (int lv = 0; lv < levels; lv++) {
		const int off = e->sched.upper_level_off[lv], cnt = e->sched.upper_level_off[lv + 1] - off;
		if (cnt == 0 || e->hess_nwg == 0) continue;
		launched++;
		hipLaunchKernelGGL((k_upper4<WAVES, SCALE, false, false, false, true>), dim3(e->hess_nwg, cnt), dim3(WAVE, e->C, 1), lds, e->stream, e->d_upper_ops + off, e->T,
		                   e->P, e->C, e->d_tipmask, e->d_lower, e->d_upper, e->d_mats, e->d_tiptab, e->d_Q, e->d_freqs, e->d_props, e->d_weights, e->d_wl,
		                   (double *)nullptr, 0, (const double *)nullptr, (const double *)nullptr, 0, e->N, (double *)nullptr, off, op_total, e->d_rates,
		                   (const int *)e->d_hess_tab, e->d_hess);
	}
	HIP_TRY(hipGetLastError());
	return finish_hess_slab(e, out, launched);
}

int launch_hess4(Shard *e, double *out) {
	return by_waves(e->C, [&](auto w) {
		constexpr int W = decltype(w)::value;
		return e->scaling_on ? launch_upper_hess<W, true>(e, out) : launch_upper_hess<W, false>(e, out);
	});
}

int upload_qpi(Shard *e) {
	if (!e->state.qpi_dirty) return PHYAMD_OK;  // diag(pi) Q, 16 doubles
	int rc;
	if ((rc = e->d_Qpi.ensure(16))) return rc;
	double qpi[16];
	for (int i = 0; i < 4; i++)
		for (int j = 0; j < 4; j++) qpi[i * 4 + j] = e->freqs[i] * e->Q_host[i * 4 + j];
	HIP_TRY(hipMemcpyAsync(e->d_Qpi, qpi, sizeof(qpi), hipMemcpyHostToDevice, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream));
	qpi_rebuilt(e);
	return PHYAMD_OK;
}

// mask words of the streamed walk: rebuilt when the tip data or the word layout (topology) changed
int ensure_mask_stream(Shard *e) {
	const size_t mstride = (size_t)e->nblk_walk_upper * e->G * WAVE;
	bool grew;
	if (int rc = e->d_mstream.ensure((size_t)std::max(1, e->stream_tab.words) * mstride, &grew)) return rc;
	if (grew) e->mstream_epoch = 0;
	if (e->mstream_epoch == e->state.tip_epoch && e->mstride == mstride && e->mstream_layout == e->stream_tab.row_entries) return PHYAMD_OK;
	e->mstride = mstride;
	e->stream_unsupported = false;
	e->stream_ambiguous = false;
	if (e->stream_tab.words > 0) {
		int flag = 0;
		HIP_TRY(hipMemsetAsync(e->d_stream_flag, 0, sizeof(int), e->stream));
		hipLaunchKernelGGL(k_build_mask_stream, dim3((unsigned)((mstride + 255) / 256), std::min(e->stream_tab.words, 32768)), dim3(256), 0, e->stream, e->stream_tab.words, e->P, mstride,
		                   (const int *)e->d_stream_row_entries, e->d_tipmask, e->d_mstream, e->d_stream_flag);
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipMemcpyAsync(&flag, e->d_stream_flag, sizeof(int), hipMemcpyDeviceToHost, e->stream));
		HIP_TRY(hipStreamSynchronize(e->stream));
		e->stream_unsupported = (flag & 1) != 0;
		e->stream_ambiguous = (flag & 2) != 0;
	}
	e->mstream_epoch = e->state.tip_epoch;
	e->mstream_layout = e->stream_tab.row_entries;
	return PHYAMD_OK;
}

// table blocks of the streamed walk: one per (pre-order op, category)
int ensure_optab(Shard *e) {
	return e->d_optab.ensure((size_t)std::max<size_t>(1, e->stream_tab.ops.size()) * e->C * OPBLK_BYTES);
}

// the exponents of the power-of-two rescaling (LowerForm::CarriedExp2), the pre-order walk's included: made before the post-order
// pass that writes that form, so that a memory cap without room for them is met while the reference's form can still be written
int ensure_exponent_storage(Shard *e) {
	int rc;
	if ((rc = e->d_lexp.ensure(lower_slots(e) * e->C * e->P)) || (rc = e->d_uexp.ensure(std::max(upper_slots_held(e), upper_slots_needed(e)) * e->C * e->P)) ||
	    (rc = e->d_Ec.ensure((size_t)e->C * e->P)) || (rc = e->d_Eroot.ensure(e->P)))
		return rc;
	return PHYAMD_OK;
}
void free_exponent_storage(Shard *e) {
	e->d_lexp.release();
	e->d_uexp.release();
	e->d_Ec.release();
	e->d_Eroot.release();
}

// The buffers of a streamed walk that lower_kernel / upper_kernel chose (lower: the post-order walk), made before its pass: mask
// words and table blocks, for the post-order walk also its per-category root terms and the exponents of CarriedExp2.  What only
// this step finds out is recorded for the second question (made = true): a cap without room for the words, the tables or the root
// terms (the table-gather walk from then on), a cap without room for the exponents (the reference's form from then on), tip data
// with an empty state mask.
int make_stream_buffers(Shard *e, bool lower) {
	const bool capped = e->cfg.max_device_bytes > 0;
	int rc = ensure_mask_stream(e);  // (pattern tiles: the mask words follow the tile's tip codes, rebuilt with every tile copy: ~0.1 ms per tile)
	if (!rc) rc = ensure_optab(e);
	if (!rc && lower) rc = e->d_Lc.ensure((size_t)e->C * e->P);  // per-category root terms for k_root_finish64
	if (rc == PHYAMD_ENOMEM && capped) {
		(lower ? e->lower_stream_capped : e->upper_stream_capped) = true;
		return PHYAMD_OK;
	}
	if (rc || !lower || e->stream_unsupported || stream_lower_form(e) != LowerForm::CarriedExp2) return rc;
	if ((rc = ensure_exponent_storage(e)) == PHYAMD_ENOMEM && capped) {
		prefer_reference_form(e);
		free_exponent_storage(e);
		return PHYAMD_OK;
	}
	return rc;
}

// the streamed post-order walk (k_lower4_stream): every cut subtree as workgroups of its own, then the top part with the root
int launch_lower_stream(Shard *e) {
	int rc;
	const int nb = (e->P + WAVE - 1) / WAVE, nops = (int)e->stream_tab.ops.size();
	if (e->stream_tab.P != e->P || e->stream_tab.mstride != e->mstride) {  // (the descriptors' byte offsets: see launch_upper_stream)
		if ((rc = upload_schedule(e))) return rc;
		if (e->stream_tab.P != e->P || e->stream_tab.mstride != e->mstride) return fail(PHYAMD_EDEVICE, "streamed walk: descriptors do not match the pattern storage");
	}
	hipLaunchKernelGGL(k_op_tables, dim3(nops, e->C), dim3(64), 0, e->stream, nops, e->C, (const int *)e->d_stream_op_tips, (const int *)e->d_stream_op_deep,
	                   (const int *)e->d_stream_site_tab, (const int *)e->d_stream_pair_tab, e->d_mats, (const double *)nullptr, reinterpret_cast<double *>(e->d_optab.get()));
	// rescaled: powers of two per category (the plain workgroup shape), or the reference's maxima over categories -- workgroup = the
	// category waves of one block + their exchange buffer
	const LowerForm form = stream_lower_form(e);
	const StreamVariant v = stream_variant(form, e->scaling_on);
	const bool exp2 = v.scale == 2, scale = v.scale == 1, tf = v.tf;
	e->lower_form = form;
	const int waves = scale ? e->C : STREAM_WAVES;
	const size_t lds = (size_t)LSTREAM_LDS_PER_WAVE * waves + (scale ? sizeof(double) * 2 * e->C * WAVE : 0);
	const unsigned gx = scale ? (unsigned)nb : (unsigned)((nb + STREAM_WAVES - 1) / STREAM_WAVES) * e->C;
	const int subtrees = (int)e->sched.walk_lower_chunk_off.size() - 2;
	const bool amb = e->stream_ambiguous;
	auto *kernel = exp2 ? (amb ? k_lower4_stream<true, 2, true> : k_lower4_stream<false, 2, true>)
	             : scale ? (amb ? k_lower4_stream<true, 1, false> : k_lower4_stream<false, 1, false>)
	             : tf    ? (amb ? k_lower4_stream<true, 0, true> : k_lower4_stream<false, 0, true>)
	                     : (amb ? k_lower4_stream<true, 0, false> : k_lower4_stream<false, 0, false>);
	for (int phase = subtrees > 0 ? 0 : 1; phase < 2; phase++)
		hipLaunchKernelGGL(kernel, dim3(gx, phase ? 1 : subtrees), dim3(WAVE, waves), lds, e->stream, (const LowerDesc *)e->d_lstream_ops,
		                   (const LowerChunk *)e->d_lstream_chunks, (const int *)e->d_walk_lower_chunk_off, phase ? std::max(0, subtrees) : 0, nops, e->P, e->C, nb,
		                   (const uint32_t *)e->d_mstream, e->mstride, e->d_lower, (const double *)e->d_mats, (const char *)e->d_optab, (const double *)e->d_freqs,
		                   (const double *)e->d_props, e->d_Lc, phase, exp2 ? reinterpret_cast<double *>(e->d_lexp.get()) : scale ? e->d_lscale : (double *)nullptr, e->xcd_map,
		                   exp2 ? e->d_Ec : (int *)nullptr);
	hipLaunchKernelGGL(k_root_finish64, dim3(nb), dim3(64), 0, e->stream, e->P, e->C, (const double *)e->d_Lc, (const double *)e->d_weights, e->d_plk, e->d_wl, e->d_lnl_part,
	                   scale ? (const double *)(e->d_lscale + (size_t)e->sched.core_index[e->root] * e->P) : (const double *)nullptr, exp2 ? (const int *)e->d_Ec : (const int *)nullptr,
	                   exp2 ? e->d_Eroot : (int *)nullptr);
	HIP_TRY(hipGetLastError());
	e->prof.lower_launches = subtrees > 0 ? 2 : 1;
	e->lnl_blocks = nb;
	e->lnl_per_block = true;
	record_lower_pass(e, PassKernel::Stream, v.scale, amb, false, STREAM_WAVES, 0);
	return PHYAMD_OK;
}

// the streamed plain pre-order walk (phyamd_walk4s.inc): the top part, then every cut subtree as workgroups of its own
template <bool FOLD, bool SCALE>
int launch_upper_stream(Shard *e) {
	int rc;
	const int nb = (e->P + WAVE - 1) / WAVE, R = e->stream_tab.R, nops = (int)e->stream_tab.ops.size();  // blocks of 64 patterns
	// the walk-order slab [nb][C][R] lives in the [row][block] slab's storage (N * C * gpart_row doubles, gpart_row >= nb, R = N - 1)
	if ((size_t)nb * e->C * R > (size_t)e->N * e->C * e->gpart_row) return fail(PHYAMD_EDEVICE, "gradient slab too small for the streamed walk");
	e->d_gslab = e->d_gpart;
	// the descriptors carry byte offsets multiplied out for a pattern count and a mask-row stride: rebuilt if either has moved
	if (e->stream_tab.P != e->P || e->stream_tab.mstride != e->mstride) {
		if ((rc = upload_schedule(e))) return rc;
		if (e->stream_tab.P != e->P || e->stream_tab.mstride != e->mstride) return fail(PHYAMD_EDEVICE, "streamed walk: descriptors do not match the pattern storage");
	}
	if ((rc = e->d_oct.ensure((size_t)8 * e->C * R))) return rc;
	// plain: workgroup = four blocks of one category; rescaled as the reference does: the C <= 4 category waves of one block + their
	// exchange buffers; rescaled by powers of two (the stored lowers are in that form): the plain shape + the parks' exponents
	const StreamVariant v = stream_variant(e->lower_form, SCALE);  // (the stored lowers decide: they are what this walk reads)
	if (v.scale < 0) return fail(PHYAMD_EDEVICE, "streamed walk: the stored lowers hold the %s form, which no %s post-order pass writes", form_name(e->lower_form), SCALE ? "rescaled" : "plain");
	const bool exp2 = v.scale == 2, tf = v.tf;
	if (exp2 && (rc = e->d_uexp.ensure(std::max<size_t>(1, upper_slots_held(e)) * e->C * e->P))) return rc;
	const int waves = SCALE && !exp2 ? e->C : STREAM_WAVES;
	const size_t lds = (size_t)STREAM_LDS_PER_WAVE * waves + (exp2 ? (size_t)waves * STREAM_PARK_SLOTS * WAVE * sizeof(int) : SCALE ? (size_t)4 * e->C * WAVE * sizeof(double) : 0);
	const dim3 grid_x(SCALE && !exp2 ? (unsigned)nb : (unsigned)((nb + STREAM_WAVES - 1) / STREAM_WAVES) * e->C), block(WAVE, waves);
	hipLaunchKernelGGL(k_op_tables, dim3(nops, e->C), dim3(64), 0, e->stream, nops, e->C, (const int *)e->d_stream_op_tips, (const int *)e->d_stream_op_deep,
	                   (const int *)e->d_stream_site_tab, (const int *)e->d_stream_pair_tab, e->d_mats, FOLD ? e->d_Q : e->d_Qpi, reinterpret_cast<double *>(e->d_optab.get()));
	const int subtrees = (int)e->sched.walk_chunk_off.size() - 2;
	UpperPass rec;
	for (int phase = 0; phase < (subtrees > 0 ? 2 : 1); phase++) {
		const bool amb = e->stream_ambiguous;
		auto *kernel = exp2 ? (amb ? k_upper4_stream<FOLD, 2, true, true> : k_upper4_stream<FOLD, 2, false, true>)
		             : SCALE ? (amb ? k_upper4_stream<FOLD, 1, true, false> : k_upper4_stream<FOLD, 1, false, false>)
		             : tf    ? (amb ? k_upper4_stream<FOLD, 0, true, true> : k_upper4_stream<FOLD, 0, false, true>)
		                     : (amb ? k_upper4_stream<FOLD, 0, true, false> : k_upper4_stream<FOLD, 0, false, false>);
		// (descriptors that name unstored children belong to the TF forms; any other pass reads the plain ones behind them: upload_schedule)
		// (... and the one instantiation that knows pair ops, the plain TF one, reads the set that has them: stream_pairs)
		const bool plain = !tf && !e->stream_tab.plain_desc.empty();
		const bool pairs = tf && !exp2 && !SCALE && !amb && !e->stream_tab.pair_desc.empty();
		rec.scale = v.scale, rec.ambiguous = amb, rec.waves = STREAM_WAVES, rec.tf = tf, rec.fold = FOLD;
		rec.pair_ops = pairs;  // (counted below, once)
		hipLaunchKernelGGL(kernel, dim3(grid_x.x, phase ? subtrees : 1), block, lds, e->stream,
		                   (const StreamDesc *)e->d_stream_ops + (plain ? e->stream_tab.desc.size() : pairs ? 2 * e->stream_tab.desc.size() : 0), (const StreamChunk *)e->d_stream_chunks + (plain ? e->stream_tab.chunks.size() : 0),
		                   (const int *)e->d_walk_chunk_off, phase, nops, e->P, e->C, nb, (const uint32_t *)e->d_mstream, e->mstride, (const double *)e->d_lower, e->d_upper,
		                   (const double *)e->d_mats, (const char *)e->d_optab, (const double *)(FOLD ? e->d_Q : e->d_Qpi), (const double *)e->d_freqs, (const double *)e->d_wl,
		                   e->d_gslab, R, (const double *)e->d_props, (const double *)e->d_weights, e->xcd_map, (const int *)e->d_lexp, e->d_uexp, (const int *)e->d_Eroot);
	}
	HIP_TRY(hipGetLastError());
	e->prof.upper_launches = subtrees > 0 ? 2 : 1;
	e->grad_blocks = nb;
	e->slab_walk_order = true;
	if (rec.pair_ops) rec.pair_ops = (int)std::count_if(e->stream_tab.pairs.begin(), e->stream_tab.pairs.end(), [](const StreamPair &p) { return p.reason == PAIR_FUSED; });
	record_upper_pass(e, PassKernel::Stream, rec);
	return PHYAMD_OK;
}

// bisection segments of the block range [0, nb) (k_slab_segments): 2^levels + 1 boundaries
void bisect_blocks(int lo, int hi, int levels, std::vector<int> &bounds) {
	if (levels == 0) {
		bounds.push_back(lo);
		return;
	}
	const int mid = lo + (hi - lo) / 2;
	bisect_blocks(lo, mid, levels - 1, bounds);
	bisect_blocks(mid, hi, levels - 1, bounds);
}

// [nb][C][R] per-block values -> out[(row_of[q] or q) * C + c], in the order described at k_slab_segments.  The segments bisect
// the CANONICAL block range [0, ceil(P / 64)); entries past it (launch padding) are zeros and ride in the last segment.
// which: 0 = lnL, 1 = gradient (each keeps its boundary table on the device)
int reduce_block_sums(Shard *e, int which, const double *slab, int nb, int C, int R, const int *row_of, double *out) {
	int rc;
	const int segments = 1 << e->reduce_levels;
	if ((rc = e->d_oct_lo.ensure(20)) || (rc = e->d_oct.ensure((size_t)8 * C * R))) return rc;
	int *table = e->d_oct_lo + 10 * which;
	if (e->seg_nb[which] != nb || e->seg_levels[which] != e->reduce_levels) {
		std::vector<int> bounds;
		bisect_blocks(0, std::min(nb, (e->P + WAVE - 1) / WAVE), e->reduce_levels, bounds);
		bounds.push_back(nb);
		HIP_TRY(hipMemcpyAsync(table, bounds.data(), sizeof(int) * bounds.size(), hipMemcpyHostToDevice, e->stream));
		HIP_TRY(hipStreamSynchronize(e->stream));  // (bounds is a stack-lifetime buffer)
		e->seg_nb[which] = nb;
		e->seg_levels[which] = e->reduce_levels;
	}
	hipLaunchKernelGGL(k_slab_segments, dim3((R + 31) / 32, C, segments), dim3(256), 0, e->stream, slab, C, R, (const int *)table, e->d_oct);
	hipLaunchKernelGGL(k_slab_finish, dim3((C * R + 255) / 256), dim3(256), 0, e->stream, e->d_oct, segments, C, R, row_of, out);
	HIP_TRY(hipGetLastError());
	return PHYAMD_OK;
}

// gradient rows from the walk-order slab
int reduce_stream_slab(Shard *e, double *out) {
	HIP_TRY(hipMemsetAsync(out, 0, sizeof(double) * (size_t)e->N * e->C, e->stream));  // the root's rows
	return reduce_block_sums(e, 1, e->d_gslab, e->grad_blocks, e->C, e->stream_tab.R, (const int *)e->d_stream_qnode, out);
}

template <int WAVES, bool FOLD, bool SCALE, bool COMPAT>
int launch_upper_walk_v(Shard *e) {
	const int ops = (int)e->sched.walk_upper_ops.size(), nb = e->nblk_walk_upper * e->G;
	int rc;
	if ((rc = check_reference_form(e, "k_upper4_walk"))) return rc;
	// columns, the rescaling exchange, then the leaf parks' LDS slots (LPARK: 2 KB per wave)
	const size_t lds = sizeof(double) * ((size_t)e->G * e->C * NACC * WCOL + (SCALE ? (size_t)4 * e->G * e->C * WAVE : 0) + (size_t)4 * e->G * e->C * WAVE);
	if ((rc = allow_big_lds(k_upper4_walk<WAVES, FOLD, false, SCALE, COMPAT>, lds))) return rc;
	// the chunked list: the top part, then every cut subtree as workgroups of its own (blockIdx.y)
	const int subtrees = (int)e->sched.walk_chunk_off.size() - 2;
	for (int phase = 0; phase < (subtrees > 0 ? 2 : 1); phase++)
		hipLaunchKernelGGL((k_upper4_walk<WAVES, FOLD, false, SCALE, COMPAT>), dim3(e->nblk_walk_upper, phase ? subtrees : 1), block_dims(e), lds, e->stream,
		                   e->d_walk_chunk_ops, ops, e->T, e->P, e->C, e->d_tipmask, e->d_lower, e->d_upper, e->d_mats, e->d_tiptab, FOLD ? e->d_Q : e->d_Qpi,
		                   e->d_freqs, e->d_wl, e->d_gpart, nb, (const double *)nullptr, (const double *)nullptr, (double *)nullptr, e->d_props, e->d_weights,
		                   (const int *)e->d_walk_chunk_off, phase);
	HIP_TRY(hipGetLastError());
	e->prof.upper_launches = subtrees > 0 ? 2 : 1;
	e->grad_blocks = nb;
	UpperPass u;
	u.scale = SCALE, u.waves = WAVES, u.fold = FOLD, u.compat = COMPAT;
	record_upper_pass(e, PassKernel::Walk, u);
	return PHYAMD_OK;
}

template <int WAVES>
int launch_upper_walk(Shard *e, bool fold, bool compat) {
	if (e->scaling_on) {
		if (fold) return compat ? launch_upper_walk_v<WAVES, true, true, true>(e) : launch_upper_walk_v<WAVES, true, true, false>(e);
		return compat ? launch_upper_walk_v<WAVES, false, true, true>(e) : launch_upper_walk_v<WAVES, false, true, false>(e);
	}
	return fold ? launch_upper_walk_v<WAVES, true, false, false>(e) : launch_upper_walk_v<WAVES, false, false, false>(e);
}

// B_theta = U^-1 dQ_theta U of every parameter theta, [np][S][S] (U, U^-1: the eigen system in e->model)
std::vector<double> eigen_basis_derivatives(const Shard *e) {
	const int S = e->S;
	const double *evec = e->model.data() + S, *ivec = e->model.data() + S + S * S;
	std::vector<double> B((size_t)e->np * S * S), tmp((size_t)S * S);
	for (int th = 0; th < e->np; th++) {
		const double *dQ = e->dQ_host.data() + (size_t)th * S * S;
		for (int a = 0; a < S; a++)
			for (int j = 0; j < S; j++) {
				double v = 0.0;
				for (int i = 0; i < S; i++) v += ivec[a * S + i] * dQ[i * S + j];
				tmp[a * S + j] = v;
			}
		for (int a = 0; a < S; a++)
			for (int b = 0; b < S; b++) {
				double v = 0.0;
				for (int j = 0; j < S; j++) v += tmp[a * S + j] * evec[j * S + b];
				B[((size_t)th * S + a) * S + b] = v;
			}
	}
	return B;
}

// G2 through the tree walk: B = U^-1 dQ U per parameter, the eigen-basis tables, one walk, then 16 sums and a contraction
template <int WAVES, bool SCALE>
int launch_upper_walk_params(Shard *e) {
	const int ops = (int)e->sched.walk_upper_ops.size(), nb = e->nblk_walk_upper * e->G, S = 4, np = e->np;
	const size_t lds = sizeof(double) * ((size_t)e->G * e->C * 16 * WCOL + (SCALE ? (size_t)4 * e->G * e->C * WAVE : 0));
	int rc;
	if ((rc = check_reference_form(e, "k_upper4_walk (parameters)"))) return rc;
	if ((rc = e->d_Bw.ensure((size_t)np * 16)) || (rc = e->d_pbuf.ensure(96)) || (rc = e->d_Fw.ensure((size_t)e->N * e->C * 20)) ||
	    (rc = e->d_gacc.ensure((size_t)16 * nb * e->C + 16)))
		return rc;
	{
		const double *evec = e->model.data() + S, *ivec = e->model.data() + S + S * S;
		const std::vector<double> B = eigen_basis_derivatives(e);
		std::vector<double> pb(96);
		for (int a = 0; a < 4; a++)
			for (int i = 0; i < 4; i++) {
				pb[a * 4 + i] = evec[i * 4 + a] * e->freqs[i];  // (diag(pi) U)^T
				pb[16 + a * 4 + i] = ivec[a * 4 + i];
			}
		for (int m = 0; m < 16; m++)
			for (int b = 0; b < 4; b++) {
				double v = 0.0;
				for (int j = 0; j < 4; j++)
					if (m >> j & 1) v += ivec[b * 4 + j];
				pb[32 + m * 4 + b] = v;  // U^-1 . mask
			}
		HIP_TRY(hipMemcpyAsync(e->d_Bw, B.data(), sizeof(double) * B.size(), hipMemcpyHostToDevice, e->stream));
		HIP_TRY(hipMemcpyAsync(e->d_pbuf, pb.data(), sizeof(double) * pb.size(), hipMemcpyHostToDevice, e->stream));
		HIP_TRY(hipStreamSynchronize(e->stream));
	}
	const int nf = e->N * e->C * 20;
	hipLaunchKernelGGL(k_eigen_weights, dim3((nf + 255) / 256), dim3(256), 0, e->stream, e->C, e->N, e->d_model, e->d_rates, e->d_props, e->d_lengths, e->d_explicit,
	                   e->root, e->d_Fw);
	if constexpr (!SCALE && WAVES == 4) {  // four pattern groups of one category per workgroup (see k_upper4_walk, CATBLK)
		const size_t lds4 = sizeof(double) * (size_t)4 * 16 * WCOL;
		hipLaunchKernelGGL((k_upper4_walk<4, false, true, false, false, true>), dim3((unsigned)((nb + 3) / 4) * e->C), dim3(WAVE, 1, 4), lds4, e->stream,
		                   e->d_walk_upper_ops, ops, e->T, e->P, e->C, e->d_tipmask, e->d_lower, e->d_upper, e->d_mats, e->d_tiptab, e->d_Qpi, e->d_freqs, e->d_wl,
		                   e->d_gpart, nb, e->d_pbuf, e->d_Fw, e->d_gacc, e->d_props, e->d_weights, (const int *)nullptr, 0);
	} else
		hipLaunchKernelGGL((k_upper4_walk<WAVES, false, true, SCALE, false>), dim3(e->nblk_walk_upper), block_dims(e), lds, e->stream, e->d_walk_upper_ops, ops, e->T,
		                   e->P, e->C, e->d_tipmask, e->d_lower, e->d_upper, e->d_mats, e->d_tiptab, e->d_Qpi, e->d_freqs, e->d_wl, e->d_gpart, nb, e->d_pbuf, e->d_Fw,
		                   e->d_gacc, e->d_props, e->d_weights, (const int *)nullptr, 0);
	double *gsum = e->d_gacc + (size_t)16 * nb * e->C;
	hipLaunchKernelGGL(k_reduce_rows, dim3(16), dim3(64), 0, e->stream, e->d_gacc, nb * e->C, (const uint8_t *)nullptr, gsum);
	hipLaunchKernelGGL(k_contract_parameters, dim3((np + 63) / 64), dim3(64), 0, e->stream, np, e->d_Bw, gsum, e->d_result + 1 + (size_t)e->N * e->C);
	HIP_TRY(hipGetLastError());
	e->prof.upper_launches = 1;
	e->grad_blocks = nb;
	UpperPass u;
	u.scale = SCALE, u.waves = WAVES, u.params = true, u.catblk = !SCALE && WAVES == 4;
	record_upper_pass(e, PassKernel::Walk, u);
	return PHYAMD_OK;
}

template <int WAVES>
int launch_upper_w(Shard *e, int flags, PassKernel k) {
	const bool fold = flags & PHYAMD_GRAD_FOLD_ROOT_FREQS, compat = (flags & PHYAMD_GRAD_COMPAT_SCALED) && e->scaling_on;
	e->grad_blocks = e->nblk;
	if (k == PassKernel::Walk) return launch_upper_walk<WAVES>(e, fold, compat);
	if (e->scaling_on) {
		if (fold) return compat ? launch_upper_levels<WAVES, true, true, true, false>(e) : launch_upper_levels<WAVES, true, true, false, false>(e);
		return compat ? launch_upper_levels<WAVES, true, false, true, false>(e) : launch_upper_levels<WAVES, true, false, false, false>(e);
	}
	return fold ? launch_upper_levels<WAVES, false, true, false, false>(e) : launch_upper_levels<WAVES, false, false, false, false>(e);
}

// largest number of parameter accumulators one workgroup's LDS holds next to the NACC branch accumulators
int parameter_chunk(const Shard *e) {
	const size_t nw = (size_t)e->G * e->C, budget = 160 * 1024 / sizeof(double) - (e->scaling_on ? 6 * nw * WAVE : 0);
	const long cols = (long)(budget / (nw * (WAVE + 1))) - NACC;
	return (int)std::max(0L, std::min(32L, cols));
}

template <int WAVES>
int launch_upper_params_w(Shard *e, int flags) {
	const bool compat = (flags & PHYAMD_GRAD_COMPAT_SCALED) && e->scaling_on;
	const int chunk = parameter_chunk(e);
	if (chunk < 1) return fail(PHYAMD_EUNSUPPORTED, "%d categories leave no LDS for parameter accumulators", e->C);
	int rc = PHYAMD_OK;
	// more parameters than one workgroup can accumulate: repeat the pass (uppers and branch sums are rewritten with identical values)
	for (int p0 = 0; p0 < e->np && !rc; p0 += chunk) {
		const int pc = std::min(chunk, e->np - p0);
		if (e->scaling_on)
			rc = compat ? launch_upper_levels<WAVES, true, false, true, true>(e, p0, pc) : launch_upper_levels<WAVES, true, false, false, true>(e, p0, pc);
		else
			rc = launch_upper_levels<WAVES, false, false, false, true>(e, p0, pc);
	}
	return rc;
}

// ---- S != 4: MFMA kernels -----------------------------------------------------------------------------------
// scratch of the rescaled S != 4 path: per op of a level, 5 rows [C][P] (lower: 1 row of maxima; upper: 3 rows num_l,
// num_r, den + 2 rows of maxima)
// rows: 5, or 7 for the HESS pre-order pass (num2_l, num2_r besides)
int ensure_gen_scale_storage(Shard *e, int rows = 5) {
	int widest = 1;
	for (size_t i = 0; i + 1 < e->sched.lower_level_off.size(); i++) widest = std::max(widest, e->sched.lower_level_off[i + 1] - e->sched.lower_level_off[i]);
	for (size_t i = 0; i + 1 < e->sched.upper_level_off.size(); i++) widest = std::max(widest, e->sched.upper_level_off[i + 1] - e->sched.upper_level_off[i]);
	return e->d_gen_scratch.ensure((size_t)widest * rows * e->C * e->P);
}

// 16-pattern tiles per wave for one level of `work` = ops x categories workgroup columns.  A workgroup costs one staging of its
// matrix images (stage_cost, in units of one tile's products) plus its tiles, and a level costs whole rounds of the `slots`
// resident workgroups: thin levels near the root take few tiles per wave (more workgroups: one node is 79 workgroups of 256
// patterns at 2e4 patterns, a third of the card), wide ones as many as amortise the staging.
inline int choose_gen_tiles(int P, int waves, long work, int slots, double stage_cost) {
	const long tiles_total = (P + 15) / 16;
	int best = 1;
	double best_cost = 0.0;
	for (int q = 1; q <= GEN_TILES_MAX; q++) {
		const long wgs = work * ((tiles_total + (long)waves * q - 1) / ((long)waves * q));
		const double cost = (double)((wgs + slots - 1) / slots) * (stage_cost + q);
		if (q == 1 || cost < best_cost * (1.0 - 1e-9)) {
			best_cost = cost;
			best = q;
		}
	}
	return best;
}

inline double gen_stage_cost(int S) { return S == 20 ? 2.0 : 0.6; }

// the levels a pass launched and the fewest and the most tiles per wave among them (phyamd_get_general_profile)
struct TileRange {
	int levels = 0, lo = 0, hi = 0;
	void add(int tiles) {
		lo = levels ? std::min(lo, tiles) : tiles;
		hi = levels ? std::max(hi, tiles) : tiles;
		levels++;
	}
};
void record_lower_levels(Shard *e, int slots, const TileRange &r) {
	phyamd_general_profile &g = e->gen_prof;
	g.lower_family = 0, g.lower_slots = slots, g.lower_levels = r.levels, g.lower_tiles_min = r.lo, g.lower_tiles_max = r.hi;
	g.walk_units = g.walk_workgroups = 0;
}
void record_upper_levels(Shard *e, bool hess, int slots, const TileRange &r) {
	phyamd_general_profile &g = e->gen_prof;
	g.upper_hess = hess, g.upper_slots = slots, g.upper_levels = r.levels, g.upper_tiles_min = r.lo, g.upper_tiles_max = r.hi;
}

template <int RT, int KT, bool SCALE>
int launch_lower_gen(Shard *e) {
	const std::vector<int> &level_off = *e->act_level_off;
	const int levels = (int)level_off.size() - 1;
	const size_t lds = sizeof(double) * GenFuse<RT>::LOWER_IMAGES * MatImage<RT, KT>::SIZE;
	int rc;
	if ((rc = allow_big_lds(k_lower_gen<RT, KT, true, SCALE>, lds)) || (rc = allow_big_lds(k_lower_gen<RT, KT, false, SCALE>, lds))) return rc;
	if (SCALE && (rc = ensure_gen_scale_storage(e))) return rc;
	const int pblocks = (e->P + 255) / 256;
	constexpr int WV = GenGeo<RT>::WAVES;
	if (e->gen_slots[0][SCALE] == 0) e->gen_slots[0][SCALE] = resident_workgroups(e, k_lower_gen<RT, KT, false, SCALE>, WV * 64, lds);  // per engine: per device
	const int slots = e->gen_slots[0][SCALE];
	int launched = 0;
	TileRange range;
	for (int lv = 0; lv < levels; lv++) {
		const int off = level_off[lv], cnt = level_off[lv + 1] - off;
		if (cnt == 0) continue;
		launched++;
		const int tiles = choose_gen_tiles(e->P, WV, (long)cnt * e->C, slots, gen_stage_cost(e->S));
		range.add(tiles);
		dim3 grid((e->P + WV * 16 * tiles - 1) / (WV * 16 * tiles), cnt, e->C);
		const bool is_root = lv == levels - 1;
		if (is_root)
			hipLaunchKernelGGL((k_lower_gen<RT, KT, true, SCALE>), grid, dim3(WV * 64), lds, e->stream, e->act_lower_ops + off, e->T, e->P, e->Pp, e->C,
			                   e->d_tipmask, e->d_tipsets, e->d_lower, e->d_imgs, e->d_freqs, e->d_props, e->d_Lc, e->d_gen_scratch, tiles);
		else
			hipLaunchKernelGGL((k_lower_gen<RT, KT, false, SCALE>), grid, dim3(WV * 64), lds, e->stream, e->act_lower_ops + off, e->T, e->P, e->Pp, e->C,
			                   e->d_tipmask, e->d_tipsets, e->d_lower, e->d_imgs, e->d_freqs, e->d_props, e->d_Lc, e->d_gen_scratch, tiles);
		if (SCALE)
			hipLaunchKernelGGL(k_scale_gen, dim3(pblocks, cnt), dim3(256), 0, e->stream, e->act_lower_ops + off, e->P, e->Pp, e->S, e->C, e->d_lower, e->d_gen_scratch,
			                   e->d_lscale, is_root ? e->d_Lc : (double *)nullptr);
	}
	const double *lscale_root = SCALE ? e->d_lscale + (size_t)e->sched.core_index[e->root] * e->P : nullptr;
	hipLaunchKernelGGL(k_root_finish, dim3(e->nblk_root), dim3(256), 0, e->stream, e->P, e->C, e->d_Lc, e->d_weights, lscale_root, e->d_plk, e->d_wl, e->d_lnl_part);
	HIP_TRY(hipGetLastError());
	e->prof.lower_launches = launched;
	record_lower_levels(e, slots, range);
	return PHYAMD_OK;
}

template <int RT, int KT, bool FOLD, bool SCALE>
int launch_upper_gen_v(Shard *e, bool compat) {
	const int levels = (int)e->sched.upper_level_off.size() - 1;
	const size_t lds = sizeof(double) * (GenFuse<RT>::UPPER_IMAGES * MatImage<RT, KT>::SIZE + 6 * GenGeo<RT>::WAVES);
	int rc;
	if ((rc = allow_big_lds(k_upper_gen<RT, KT, FOLD, SCALE, false>, lds))) return rc;
	if (SCALE && (rc = ensure_gen_scale_storage(e))) return rc;
	if (GenFuse<RT>::QP && (rc = ensure_tip_rate_products(e, FOLD))) return rc;
	const int pblocks = (e->P + 255) / 256;
	constexpr int WV = GenGeo<RT>::WAVES;
	if (e->gen_slots[1 + FOLD][SCALE] == 0) e->gen_slots[1 + FOLD][SCALE] = resident_workgroups(e, k_upper_gen<RT, KT, FOLD, SCALE, false>, WV * 64, lds);
	const int slots = e->gen_slots[1 + FOLD][SCALE];
	double *nd = e->d_gen_scratch, *mxu = SCALE ? e->d_gen_scratch : nullptr;
	// rows of the gradient slabs are e->nblk wide (the finest grid); a level writes the first grid.x entries of its rows and
	// the reduction adds the whole row in a fixed order: the rest must be zero
	HIP_TRY(hipMemsetAsync(e->d_gpart, 0, sizeof(double) * (size_t)e->N * e->C * e->gpart_row, e->stream));
	TileRange range;
	for (int lv = 0; lv < levels; lv++) {
		const int off = e->sched.upper_level_off[lv], cnt = e->sched.upper_level_off[lv + 1] - off;
		if (cnt == 0) continue;
		const int tiles = choose_gen_tiles(e->P, WV, (long)cnt * e->C, slots, gen_stage_cost(e->S));
		range.add(tiles);
		dim3 grid((e->P + WV * 16 * tiles - 1) / (WV * 16 * tiles), cnt, e->C);
		if (SCALE) mxu = e->d_gen_scratch + (size_t)cnt * 3 * e->C * e->P;
		hipLaunchKernelGGL((k_upper_gen<RT, KT, FOLD, SCALE, false>), grid, dim3(WV * 64), lds, e->stream, e->d_upper_ops + off, e->T, e->P, e->Pp, e->C,
		                   e->d_tipmask, e->d_tipsets, e->d_lower, e->d_upper, e->d_imgs, e->d_imgs + ((size_t)e->N * e->C + (FOLD ? 0 : 1)) * MatImage<RT, KT>::SIZE, e->d_freqs, e->d_wl,
		                   e->d_gpart, e->nblk, nd, mxu, tiles, e->d_qp_imgs, (const double *)nullptr);
		if (SCALE) {
			hipLaunchKernelGGL(k_scale_upper_gen, dim3(pblocks, cnt), dim3(256), 0, e->stream, e->d_upper_ops + off, e->P, e->Pp, e->S, e->C, e->d_upper, mxu);
			const int ppb = 256;  // one pattern per thread and slab entry; pblocks <= e->nblk
			if (compat)
				hipLaunchKernelGGL(k_scaled_gradient_gen<true>, dim3(pblocks, cnt), dim3(256), 0, e->stream, e->d_upper_ops + off, e->P, e->C, ppb, nd, e->d_weights,
				                   e->d_props, e->d_gpart, e->nblk);
			else
				hipLaunchKernelGGL(k_scaled_gradient_gen<false>, dim3(pblocks, cnt), dim3(256), 0, e->stream, e->d_upper_ops + off, e->P, e->C, ppb, nd, e->d_weights,
				                   e->d_props, e->d_gpart, e->nblk);
		}
	}
	HIP_TRY(hipGetLastError());
	e->prof.upper_launches = levels;
	record_upper_levels(e, false, slots, range);
	return PHYAMD_OK;
}

// The HESS pre-order pass, 20 / 60 / 61 states (unfused schedule: phyamd_eval.inc, run_hessian): k_upper_gen writes the five rows
// of every op of a level, k_hess_gen mixes them into the Hessian slab.
template <int RT, int KT, bool SCALE>
int launch_upper_gen_hess(Shard *e, double *out) {
	using Img = MatImage<RT, KT>;
	const int levels = (int)e->sched.upper_level_off.size() - 1, S = e->S;
	for (int i = 0; i < S; i++)
		if (!(e->freqs[i] > 0.0)) return fail(PHYAMD_EUNSUPPORTED, "the Hessian diagonal divides by the frequencies: state %d has frequency %g", i, e->freqs[i]);
	const size_t lds = sizeof(double) * (GenFuse<RT>::UPPER_IMAGES * Img::SIZE + 6 * GenGeo<RT>::WAVES);
	int rc;
	if (e->sched.fused) return fail(PHYAMD_EDEVICE, "k_upper_gen<HESS> runs on the unfused schedule");
	if ((rc = allow_big_lds(k_upper_gen<RT, KT, false, SCALE, true>, lds))) return rc;
	if ((rc = ensure_gen_scale_storage(e, 7))) return rc;
	if (GenFuse<RT>::QP && (rc = ensure_tip_rate_products(e, false))) return rc;
	if ((rc = e->d_hess_invf.ensure(S))) return rc;
	std::vector<double> invf(S);
	for (int i = 0; i < S; i++) invf[i] = 1.0 / e->freqs[i];
	HIP_TRY(hipMemcpyAsync(e->d_hess_invf, invf.data(), sizeof(double) * S, hipMemcpyHostToDevice, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream));  // (invf is a stack-lifetime buffer)
	const int pblocks = (e->P + 255) / 256;
	constexpr int WV = GenGeo<RT>::WAVES;
	if (e->gen_hess_slots[SCALE] == 0) e->gen_hess_slots[SCALE] = resident_workgroups(e, k_upper_gen<RT, KT, false, SCALE, true>, WV * 64, lds);
	const int slots = e->gen_hess_slots[SCALE];
	HIP_TRY(hipMemsetAsync(e->d_hess, 0, sizeof(double) * (size_t)e->hess_nwg * 2 * e->N, e->stream));  // (the root's entries stay zero)
	double *nd = e->d_gen_scratch;
	int launched = 0;
	TileRange range;
	for (int lv = 0; lv < levels; lv++) {
		const int off = e->sched.upper_level_off[lv], cnt = e->sched.upper_level_off[lv + 1] - off;
		if (cnt == 0) continue;
		launched++;
		const int tiles = choose_gen_tiles(e->P, WV, (long)cnt * e->C, slots, gen_stage_cost(e->S));
		range.add(tiles);
		dim3 grid((e->P + WV * 16 * tiles - 1) / (WV * 16 * tiles), cnt, e->C);
		double *mxu = SCALE ? e->d_gen_scratch + (size_t)cnt * 5 * e->C * e->P : nullptr;
		hipLaunchKernelGGL((k_upper_gen<RT, KT, false, SCALE, true>), grid, dim3(WV * 64), lds, e->stream, e->d_upper_ops + off, e->T, e->P, e->Pp, e->C,
		                   e->d_tipmask, e->d_tipsets, e->d_lower, e->d_upper, e->d_imgs, e->d_imgs + ((size_t)e->N * e->C + 1) * Img::SIZE, e->d_freqs, e->d_wl,
		                   (double *)nullptr, 0, nd, mxu, tiles, e->d_qp_imgs, (const double *)e->d_hess_invf);
		if (SCALE)
			hipLaunchKernelGGL(k_scale_upper_gen, dim3(pblocks, cnt), dim3(256), 0, e->stream, e->d_upper_ops + off, e->P, e->Pp, e->S, e->C, e->d_upper, mxu);
		if (e->hess_nwg > 0)
			hipLaunchKernelGGL(k_hess_gen, dim3(e->hess_nwg, cnt), dim3(256), 0, e->stream, e->d_upper_ops + off, e->P, e->C, e->N, (const double *)nd, e->d_weights,
			                   e->d_props, e->d_rates, (const int *)e->d_hess_tab, e->d_hess);
	}
	HIP_TRY(hipGetLastError());
	record_upper_levels(e, true, slots, range);
	return finish_hess_slab(e, out, launched);
}

int launch_hess(Shard *e, double *out) {
	if (!e->generic) return launch_hess4(e, out);
	if (e->S == 20) return e->scaling_on ? launch_upper_gen_hess<2, 5, true>(e, out) : launch_upper_gen_hess<2, 5, false>(e, out);
	if (e->S == 60) return e->scaling_on ? launch_upper_gen_hess<4, 15, true>(e, out) : launch_upper_gen_hess<4, 15, false>(e, out);
	return e->scaling_on ? launch_upper_gen_hess<4, 16, true>(e, out) : launch_upper_gen_hess<4, 16, false>(e, out);
}

// the 20-state post-order tree walk (phyamd_genwalk.inc): one launch, workgroups draw (pattern group, category) units from a counter
template <int RT, int KT>
int launch_lower_gen_walk(Shard *e) {
	using W = GenWalk<RT, KT>;
	constexpr int WV = W::WV;
	const size_t lds = sizeof(double) * 2 * W::LOWER_IMAGES * MatImage<RT, KT>::SIZE;
	int rc;
	if ((rc = allow_big_lds(k_lower_gen_walk<RT, KT>, lds))) return rc;
	if (e->gen_walk_slots[0] == 0) e->gen_walk_slots[0] = resident_workgroups(e, k_lower_gen_walk<RT, KT>, WV * 64, lds);
	const int groups = (e->P + WV * 16 - 1) / (WV * 16), nops = (int)e->sched.walk_lower_ops.size(), units = groups * e->C;
	const int wgs = std::max(1, std::min(units, e->gen_walk_slots[0]));
	if ((rc = e->d_gen_walk_counter.ensure(1))) return rc;
	HIP_TRY(hipMemsetAsync(e->d_gen_walk_counter, 0, sizeof(int), e->stream));
	hipLaunchKernelGGL((k_lower_gen_walk<RT, KT>), dim3(wgs), dim3(WV * 64), lds, e->stream, e->d_walk_lower_ops, nops, e->T, e->P, e->Pp, e->C, e->d_tipmask,
	                   e->d_tipsets, e->d_lower, e->d_imgs, e->d_freqs, e->d_props, e->d_Lc, units, e->d_gen_walk_counter);
	hipLaunchKernelGGL(k_root_finish, dim3(e->nblk_root), dim3(256), 0, e->stream, e->P, e->C, e->d_Lc, e->d_weights, (const double *)nullptr, e->d_plk, e->d_wl,
	                   e->d_lnl_part);
	HIP_TRY(hipGetLastError());
	e->prof.lower_launches = 1;
	e->gen_prof.lower_family = 1, e->gen_prof.lower_slots = e->gen_walk_slots[0], e->gen_prof.lower_levels = 0;
	e->gen_prof.lower_tiles_min = e->gen_prof.lower_tiles_max = 0;
	e->gen_prof.walk_units = units, e->gen_prof.walk_workgroups = wgs;
	return PHYAMD_OK;
}
template <int RT, int KT>
int launch_upper_gen(Shard *e, int flags) {
	const bool fold = flags & PHYAMD_GRAD_FOLD_ROOT_FREQS, compat = flags & PHYAMD_GRAD_COMPAT_SCALED;
	if (e->scaling_on) return fold ? launch_upper_gen_v<RT, KT, true, true>(e, compat) : launch_upper_gen_v<RT, KT, false, true>(e, compat);
	return fold ? launch_upper_gen_v<RT, KT, true, false>(e, false) : launch_upper_gen_v<RT, KT, false, false>(e, false);
}

template <int RT, int KT>
int launch_lower_gen_s(Shard *e) {
	return e->scaling_on ? launch_lower_gen<RT, KT, true>(e) : launch_lower_gen<RT, KT, false>(e);
}

// The post-order and pre-order passes of family k (lower_kernel, upper_kernel); the walks' workgroups hold C * G waves
int launch_lower(Shard *e, PassKernel k) {
	if (e->generic) {
		if (k == PassKernel::Walk) return launch_lower_gen_walk<2, 5>(e);  // (20 states only)
		return e->S == 20 ? launch_lower_gen_s<2, 5>(e) : e->S == 60 ? launch_lower_gen_s<4, 15>(e) : launch_lower_gen_s<4, 16>(e);
	}
	if (k == PassKernel::Stream) return launch_lower_stream(e);
	e->lower_form = LowerForm::Reference;
	return by_waves(e->C * e->G, [&](auto w) { return launch_lower_w<decltype(w)::value>(e, k); });
}
int launch_upper(Shard *e, int flags, PassKernel k) {
	if (e->generic) return e->S == 20 ? launch_upper_gen<2, 5>(e, flags) : e->S == 60 ? launch_upper_gen<4, 15>(e, flags) : launch_upper_gen<4, 16>(e, flags);
	if (k == PassKernel::Stream) {
		const bool fold = flags & PHYAMD_GRAD_FOLD_ROOT_FREQS;
		if (e->scaling_on) return fold ? launch_upper_stream<true, true>(e) : launch_upper_stream<false, true>(e);
		return fold ? launch_upper_stream<true, false>(e) : launch_upper_stream<false, false>(e);
	}
	return by_waves(e->C * e->G, [&](auto w) { return launch_upper_w<decltype(w)::value>(e, flags, k); });
}
// 4 states, the substitution-parameter gradient (update_parameter_matrices first for the Levels family)
int launch_upper_params(Shard *e, int flags, PassKernel k) {
	return by_waves(e->C * e->G, [&](auto w) {
		constexpr int W = decltype(w)::value;
		if (k == PassKernel::Levels) return launch_upper_params_w<W>(e, flags);
		return e->scaling_on ? launch_upper_walk_params<W, true>(e) : launch_upper_walk_params<W, false>(e);
	});
}
