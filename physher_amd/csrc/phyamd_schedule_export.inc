// phyamd_schedule_export.inc -- a tree's host schedules as the walks run them, for tests and tools (no device, no engine)
// (part of phyamd_engine.hip: included by phyamd_abi.inc inside its extern "C" block)

// the post-order walk's chunked op list of a tree as the streamed walk runs it: host code only (no device, no engine)
int phyamd_post_order_parks(int32_t tip_count, const int32_t *left, const int32_t *right, int32_t root, int32_t second_slot, int32_t *out, int32_t capacity) {
	if (tip_count < 2) return fail(PHYAMD_EINVAL, "tip_count must be >= 2 (got %d)", tip_count);
	if (!left || !right) return fail(PHYAMD_EINVAL, "null left or right");
	if (capacity < 0 || (capacity > 0 && !out)) return fail(PHYAMD_EINVAL, "null out with capacity %d", capacity);
	ScheduleOptions options;  // 4 states, an engine's defaults
	options.lower_park2_on = second_slot != 0;
	Schedule sched;
	const std::string err = build_schedule(TreeRef{tip_count, left, right, root}, options, &sched);
	if (!err.empty()) return fail(PHYAMD_EINVAL, "%s", err.c_str());
	const std::vector<NodeOp> &ops = sched.walk_lower_chunk_ops;
	const std::vector<int> &off = sched.walk_lower_chunk_off;
	std::vector<char> is_cut_root(2 * tip_count - 1, 0);  // the roots of the cut subtrees: every chunk's last op but the top part's
	for (size_t k = 1; k + 1 < off.size(); k++)
		if (off[k] > off[k - 1]) is_cut_root[ops[off[k] - 1].parent] = 1;
	int chunk = 0;
	for (int i = 0; i < (int)ops.size() && i < capacity; i++) {
		const NodeOp &o = ops[i];
		while (i >= off[chunk + 1]) chunk++;
		auto source = [&](int side) {
			if ((side ? o.kind_right : o.kind_left) != CH_CORE) return -1;
			return o.carry_in == side + 1 ? 1 : (o.lds_park & (1 << side)) ? 2 : (o.lds_park & (0x10 << side)) ? 3 : 0;
		};
		const int32_t rec[8] = {chunk, o.parent, o.left, o.right, source(0), source(1), ((o.lds_park & 4) ? 1 : 0) | ((o.lds_park & 0x40) ? 2 : 0),
		                        (is_cut_root[o.left] ? 1 : 0) | (is_cut_root[o.right] ? 2 : 0)};
		std::memcpy(out + (size_t)i * 8, rec, sizeof(rec));
	}
	return (int)ops.size();
}

// the post-order pass of a tree as k_sitelnl_walk4 runs it: host code only (no device, no engine)
int phyamd_post_order_slots(int32_t tip_count, const int32_t *left, const int32_t *right, int32_t root, int32_t *out, int32_t capacity, int32_t *slots) {
	static const char *const name = "phyamd_post_order_slots";
	if (tip_count < 2) return fail(PHYAMD_EINVAL, "%s: tip_count must be >= 2 (got %d)", name, tip_count);
	if (!left || !right) return fail(PHYAMD_EINVAL, "%s: null left or right", name);
	if (capacity < 0 || (capacity > 0 && !out)) return fail(PHYAMD_EINVAL, "%s: null out with capacity %d", name, capacity);
	std::vector<int32_t> parents;
	const std::string err = validate_tree(TreeRef{tip_count, left, right, root}, parents, name, 0);
	if (!err.empty()) return fail(PHYAMD_EINVAL, "%s", err.c_str());
	std::vector<BatchOp> work, ops;
	const int used = site_lnl_ops(tip_count, left, right, root, work, &ops);
	if (slots) *slots = used;
	for (int i = 0; i < (int)ops.size() && i < capacity; i++) {
		const BatchOp &o = ops[i];
		const int32_t rec[6] = {o.node, o.left, o.right, o.src, o.dst_left, o.dst_right};
		std::memcpy(out + (size_t)i * 6, rec, sizeof(rec));
	}
	return (int)ops.size();
}

// one pass of phyamd_optimize_branch_lengths over a tree as k_blopt_step4 and k_blopt_solve4 run it: host code only (no device, no engine)
int phyamd_branch_sweep_schedule(int32_t tip_count, const int32_t *left, const int32_t *right, int32_t root, int32_t *out, int32_t capacity) {
	static const char *const name = "phyamd_branch_sweep_schedule";
	if (tip_count < 2) return fail(PHYAMD_EINVAL, "%s: tip_count must be >= 2 (got %d)", name, tip_count);
	if (!left || !right) return fail(PHYAMD_EINVAL, "%s: null left or right", name);
	if (capacity < 0 || (capacity > 0 && !out)) return fail(PHYAMD_EINVAL, "%s: null out with capacity %d", name, capacity);
	std::vector<int32_t> parents;
	const std::string err = validate_tree(TreeRef{tip_count, left, right, root}, parents, name, 0);
	if (!err.empty()) return fail(PHYAMD_EINVAL, "%s", err.c_str());
	std::vector<SweepOp> ops;
	build_branch_sweep(tip_count, left, right, root, &ops);
	const int T = tip_count, N = 2 * T - 1;
	for (int i = 0; i < (int)ops.size() && i < capacity; i++) {
		const SweepOp &o = ops[i];
		const int32_t lower_plane = o.node >= T ? N + (o.node - T) : -1;
		const int32_t rec[6] = {o.visit, o.kind, o.node, o.a, o.kind == SWEEP_VISIT ? lower_plane : o.b, o.kind == SWEEP_UPPER ? o.node : o.kind == SWEEP_LOWER ? lower_plane : -1};
		std::memcpy(out + (size_t)i * 6, rec, sizeof(rec));
	}
	return (int)ops.size();
}

// the pre-order walk's op list of a tree as one of its readers runs it: host code only (no device, no engine)
int phyamd_pre_order_schedule(int32_t tip_count, const int32_t *left, const int32_t *right, int32_t root, int32_t form, int32_t *out, int32_t capacity,
                              int32_t *hbm_slots) {
	constexpr int W = PHYAMD_PRE_ORDER_COLUMNS;
	enum { S_ROOT = 0, S_CARRY = 1, S_LDS0 = 2, S_LDS1 = 3, S_HBM = 4, D_NONE = 0 };  // (destinations: the same codes, 0 = none)
	if (tip_count < 2) return fail(PHYAMD_EINVAL, "tip_count must be >= 2 (got %d)", tip_count);
	if (!left || !right) return fail(PHYAMD_EINVAL, "null left or right");
	if (form < 0 || form > 2) return fail(PHYAMD_EINVAL, "form must be 0 (chunked list), 1 (streamed walk) or 2 (one list), got %d", form);
	if (capacity < 0 || (capacity > 0 && !out)) return fail(PHYAMD_EINVAL, "null out with capacity %d", capacity);
	const int N = 2 * tip_count - 1;
	Schedule sched;  // 4 states, an engine's defaults; the streamed walk's tables for one pattern of one category
	StreamTables stream_tab;
	const std::string err = build_schedule(TreeRef{tip_count, left, right, root}, ScheduleOptions{}, &sched);
	if (!err.empty()) return fail(PHYAMD_EINVAL, "%s", err.c_str());
	if (form == 1) build_stream_tables(sched, StreamGeometry{1, 1, WAVE}, &stream_tab);
	const std::vector<NodeOp> &ops = form == 2 ? sched.walk_upper_ops : sched.walk_chunk_ops;
	const std::vector<int> one_chunk{0, (int)ops.size()};
	const std::vector<int> &off = form == 2 ? one_chunk : sched.walk_chunk_off;
	if (hbm_slots) {
		*hbm_slots = sched.walk_chunk_slots;
		if (form == 2) {  // (walk_upper_slots has become the larger of the two lists' counts: the one list's own is its highest index + 1)
			int most = -1;
			for (const NodeOp &o : ops) most = std::max({most, o.upper_slot_parent, o.upper_slot_left, o.upper_slot_right});
			*hbm_slots = most + 1;
		}
	}
	std::vector<char> has_op(N, 0), is_cut_root(N, 0);  // the roots of the cut subtrees: every chunk's first op but the top part's
	for (const NodeOp &o : ops) has_op[o.parent] = 1;
	for (size_t k = 1; k + 1 < off.size(); k++)
		if (off[k + 1] > off[k]) is_cut_root[ops[off[k]].parent] = 1;
	auto half_ch = [](int hk) { return hk == HK_TIP ? (int)CH_TIP : hk == HK_CHERRY ? (int)CH_CHERRY : (int)CH_CHERRY_TIP; };
	int chunk = 0;
	for (int i = 0; i < (int)ops.size() && i < capacity; i++) {
		while (i >= off[chunk + 1]) chunk++;
		int32_t rec[W];
		for (int j = 0; j < W; j++) rec[j] = -1;
		rec[0] = chunk;
		int32_t *q = rec + 20;
		int nq = 0;
		if (form == 1) {  // what k_upper4_stream reads: the descriptor's flags and slots
			const StreamOp &s = stream_tab.ops[i];
			const int fl = stream_tab.desc[i].flags, kl = fl & 7, kr = (fl >> 3) & 7, usrc = (fl >> 9) & 7, pk = (fl >> 12) & 3;
			rec[1] = s.parent;
			rec[2] = s.lnode;
			rec[3] = s.rnode;
			rec[4] = kl;
			rec[5] = kr;
			if (kl == CH_DEEP) rec[6] = half_ch((fl >> 16) & 3), rec[7] = half_ch((fl >> 18) & 3);
			if (kr == CH_DEEP) rec[8] = half_ch((fl >> 20) & 3), rec[9] = half_ch((fl >> 22) & 3);
			rec[10] = usrc == SU_ROOT ? S_ROOT : usrc == SU_CARRY ? S_CARRY : usrc == SU_LDS ? (((fl >> 7) & 1) ? S_LDS1 : S_LDS0) : S_HBM;
			rec[11] = usrc == SU_U ? s.slot_parent : -1;
			for (int side = 0; side < 2; side++) {
				const bool stored = fl & (1 << (29 + side));
				const int slot = side ? s.slot_right : s.slot_left;
				int d = D_NONE;
				if (pk == side + 1) d = ((fl >> 6) & 1) ? S_LDS1 : S_LDS0;
				else if (stored) d = S_HBM;
				else if (side == 0 && has_op[s.lnode]) d = S_CARRY;  // (the kernel hands `ul` on, always: neither parked nor stored = carried)
				rec[12 + 2 * side] = d;
				rec[13 + 2 * side] = stored ? slot : -1;
			}
			rec[16] = (fl & (1 << 28)) ? s.nx_u : -1;
			rec[18] = rec[12] == S_CARRY ? 1 : 0;  // (after stream_pre_order's swap the carried child, if any, is the left one)
			for (int j = 0; j < 10; j++) {
				const int at = stream_tab.site_tab[(size_t)i * 16 + j];
				if (at >= 0) q[nq++] = stream_tab.qnode[at / 8];
			}
		} else {  // what k_upper4_walk reads: the NodeOp itself (form 2: its PARAMS form, which has no LDS slot)
			const NodeOp &o = ops[i];
			const bool lpark = form == 0;
			rec[1] = o.parent;
			rec[2] = o.left;
			rec[3] = o.right;
			rec[4] = o.kind_left;
			rec[5] = o.kind_right;
			if (o.kind_left == CH_DEEP) rec[6] = sched.deep_host[o.left].kind_left, rec[7] = sched.deep_host[o.left].kind_right;
			if (o.kind_right == CH_DEEP) rec[8] = sched.deep_host[o.right].kind_left, rec[9] = sched.deep_host[o.right].kind_right;
			const bool proot = o.upper_slot_parent < 0 && !o.carry_in && !(o.lds_park & 1);
			rec[10] = proot ? S_ROOT : o.carry_in ? S_CARRY : (lpark && (o.lds_park & 1)) ? S_LDS0 : S_HBM;
			rec[11] = rec[10] == S_HBM ? o.upper_slot_parent : -1;
			for (int side = 0; side < 2; side++) {
				const int slot = side ? o.upper_slot_right : o.upper_slot_left, ch = side ? o.right : o.left;
				int d = D_NONE;
				if (lpark && (o.lds_park & 6) && ((o.lds_park & 2) ? 0 : 1) == side) d = S_LDS0;
				else if (slot >= 0) d = S_HBM;
				else if (o.carry_out == side + 1 && has_op[ch]) d = S_CARRY;
				rec[12 + 2 * side] = d;
				rec[13 + 2 * side] = slot;
			}
			rec[18] = o.carry_out;
			const int kl = o.kind_left, kr = o.kind_right;  // the rows the kernel's accumulators are stored to, in its order
			const int rows[10] = {o.left, o.right, kl >= CH_CHERRY ? o.lt0 : -1, kl >= CH_CHERRY ? o.lt1 : -1, kl == CH_CHERRY_TIP ? o.linner : -1,
			                      kl == CH_CHERRY_TIP ? o.lt2 : -1, kr >= CH_CHERRY ? o.rt0 : -1, kr >= CH_CHERRY ? o.rt1 : -1,
			                      kr == CH_CHERRY_TIP ? o.rinner : -1, kr == CH_CHERRY_TIP ? o.rt2 : -1};
			for (int j = 0; j < 10; j++)
				if (rows[j] >= 0) q[nq++] = rows[j];
		}
		rec[17] = (is_cut_root[rec[2]] ? 1 : 0) | (is_cut_root[rec[3]] ? 2 : 0);
		rec[19] = nq;
		std::memcpy(out + (size_t)i * W, rec, sizeof(rec));
	}
	return (int)ops.size();
}

// the stored nodes the streamed walks of a tree do without (stream_elide): host code only (no device, no engine)
int phyamd_stream_elisions(int32_t tip_count, const int32_t *left, const int32_t *right, int32_t root, int32_t *out, int32_t capacity) {
	if (tip_count < 2) return fail(PHYAMD_EINVAL, "tip_count must be >= 2 (got %d)", tip_count);
	if (!left || !right) return fail(PHYAMD_EINVAL, "null left or right");
	if (capacity < 0 || (capacity > 0 && !out)) return fail(PHYAMD_EINVAL, "null out with capacity %d", capacity);
	Schedule sched;  // 4 states, an engine's defaults; the streamed walks' tables for one pattern of one category, as an engine builds them
	StreamTables stream_tab;
	const std::string err = build_schedule(TreeRef{tip_count, left, right, root}, ScheduleOptions{}, &sched);
	if (!err.empty()) return fail(PHYAMD_EINVAL, "%s", err.c_str());
	build_stream_tables(sched, StreamGeometry{1, 1, WAVE, true}, &stream_tab);
	const std::vector<StreamElision> &el = stream_tab.elisions;
	for (int i = 0; i < (int)el.size() && i < capacity; i++) {
		const int32_t rec[8] = {el[i].node, el[i].parent, el[i].stored, el[i].sibling, el[i].sibling_kind, el[i].source, el[i].side, el[i].chunk};
		std::memcpy(out + (size_t)i * 8, rec, sizeof(rec));
	}
	return (int)el.size();
}

// the elided nodes whose op takes its stored child's plane from its parent's op in registers (stream_keep): host code only (no
// device, no engine)
int phyamd_stream_keeps(int32_t tip_count, const int32_t *left, const int32_t *right, int32_t root, int32_t keep, int32_t *out, int32_t capacity) {
	if (tip_count < 2) return fail(PHYAMD_EINVAL, "tip_count must be >= 2 (got %d)", tip_count);
	if (!left || !right) return fail(PHYAMD_EINVAL, "null left or right");
	if (capacity < 0 || (capacity > 0 && !out)) return fail(PHYAMD_EINVAL, "null out with capacity %d", capacity);
	Schedule sched;  // 4 states, an engine's defaults; the streamed walks' tables for one pattern of one category, as an engine builds them
	StreamTables tab;
	const std::string err = build_schedule(TreeRef{tip_count, left, right, root}, ScheduleOptions{}, &sched);
	if (!err.empty()) return fail(PHYAMD_EINVAL, "%s", err.c_str());
	build_stream_tables(sched, StreamGeometry{1, 1, WAVE, true, true, keep != 0}, &tab);
	const std::vector<StreamKeep> &kp = tab.keeps;
	for (int i = 0; i < (int)kp.size() && i < capacity; i++) {
		// what the two descriptor sets that know elided kinds say of the request, so that a test can hold the rewrite itself
		const int at = [&] {
			for (int j = 0; j < (int)tab.ops.size(); j++)
				if (tab.ops[j].parent == kp[i].parent) return j;
			return -1;
		}();
		const int bit = 1 << (26 + kp[i].side);
		const int32_t rec[PHYAMD_STREAM_KEEP_COLUMNS] = {kp[i].node, kp[i].parent, kp[i].side, kp[i].reason, at >= 0 && (tab.desc[at].flags & bit) ? 1 : 0,
		                                                 at >= 0 && (tab.pair_desc[at].flags & bit) ? 1 : 0};
		std::memcpy(out + (size_t)i * PHYAMD_STREAM_KEEP_COLUMNS, rec, sizeof(rec));
	}
	return (int)kp.size();
}

// what stream_pairs makes of the streamed pre-order walk of a tree: host code only (no device, no engine)
int phyamd_stream_pairs(int32_t tip_count, const int32_t *left, const int32_t *right, int32_t root, int32_t pairs, int32_t *out, int32_t capacity) {
	constexpr int W = PHYAMD_STREAM_PAIR_COLUMNS;
	if (tip_count < 2) return fail(PHYAMD_EINVAL, "tip_count must be >= 2 (got %d)", tip_count);
	if (!left || !right) return fail(PHYAMD_EINVAL, "null left or right");
	if (capacity < 0 || (capacity > 0 && !out)) return fail(PHYAMD_EINVAL, "null out with capacity %d", capacity);
	Schedule sched;  // 4 states, an engine's defaults; the streamed walks' tables for one pattern of one category, as an engine builds them
	StreamTables tab;
	const std::string err = build_schedule(TreeRef{tip_count, left, right, root}, ScheduleOptions{}, &sched);
	if (!err.empty()) return fail(PHYAMD_EINVAL, "%s", err.c_str());
	build_stream_tables(sched, StreamGeometry{1, 1, WAVE, true, pairs != 0}, &tab);
	const int ns = (int)tab.ops.size();
	auto digest = [](uint32_t h, const void *data, size_t bytes) {  // FNV-1a
		const unsigned char *b = static_cast<const unsigned char *>(data);
		for (size_t j = 0; j < bytes; j++) h = (h ^ b[j]) * 16777619u;
		return h;
	};
	int chunk = 0;
	for (int i = 0; i < ns && i < capacity; i++) {
		while (i >= sched.walk_chunk_off[chunk + 1]) chunk++;
		int32_t rec[W];
		for (int j = 0; j < W; j++) rec[j] = -1;
		rec[0] = chunk;
		rec[1] = tab.ops[i].parent;
		uint32_t h = 2166136261u;
		h = digest(h, &tab.ops[i], sizeof(StreamOp));
		h = digest(h, &tab.desc[i], sizeof(StreamDesc));
		if (!tab.plain_desc.empty()) h = digest(h, &tab.plain_desc[i], sizeof(StreamDesc));
		h = digest(h, &tab.site_tab[(size_t)i * 16], 16 * sizeof(int));
		h = digest(h, &tab.op_tips[(size_t)i * 12], 12 * sizeof(int));
		rec[13] = (int32_t)(h & 0x7FFFFFFFu);
		if (!tab.pairs.empty()) {
			const StreamPair &pr = tab.pairs[i];
			const StreamDesc &d = tab.pair_desc[i];
			const int fl = d.flags, usrc = (fl >> 9) & 7, pk = (fl >> 12) & 3;
			rec[2] = pr.reason;
			rec[3] = pr.child;
			rec[4] = pr.sibling;
			rec[5] = pr.sibling_kind;
			rec[6] = pr.child_tips;
			rec[7] = pr.carry;
			rec[8] = usrc == SU_ROOT ? 0 : usrc == SU_CARRY ? 1 : usrc == SU_LDS ? (((fl >> 7) & 1) ? 3 : 2) : 4;
			rec[9] = pk == 2 ? (((fl >> 6) & 1) ? 3 : 2) : (fl & (1 << 30)) ? 4 : 0;
			rec[10] = (fl & (1 << 28)) ? (int32_t)(d.nx_u / ((int64_t)4 * 8)) : -1;  // (one pattern, one category: an array is 32 bytes)
			const int next = i + 1 + (pr.reason == PAIR_FUSED ? 1 : 0);
			rec[11] = next < sched.walk_chunk_off[chunk + 1] ? next : -1;
			rec[12] = (fl >> 24) & 1;
			rec[14] = (int32_t)(digest(2166136261u, &d, sizeof(StreamDesc)) & 0x7FFFFFFFu);
			for (int j = 0; j < 16; j++) {
				const int at = tab.pair_tab[(size_t)i * 16 + j];
				if (at >= 0) rec[16 + j] = tab.qnode[at / 8], rec[32 + j] = at / 8;
			}
		}
		std::memcpy(out + (size_t)i * W, rec, sizeof(rec));
	}
	return ns;
}
