// phyamd_tree_schedule.h -- the host-built lists every tree pass runs from, as values built by pure functions: the tree check, the
// level schedule, the two depth-first walk lists and their chunked forms (Schedule), the streamed walks' descriptors and mask-row
// layout (StreamTables), and the batched walks' op lists.  Standard C++17 over phyamd_types.h: no HIP, no engine state, no global
// state -- an error leaves as its text.  phyamd_engine.hip includes it inside its anonymous namespace (after the standard headers
// below); tests/cpp/schedule_sanitize.cpp runs it under the host sanitizers.
#ifndef PHYAMD_TREE_SCHEDULE_H
#define PHYAMD_TREE_SCHEDULE_H

#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "phyamd_types.h"

// a binary tree over N = 2 T - 1 nodes in phyamd_set_topology's convention: tips are 0..T-1 with children -1, arrays of N entries
struct TreeRef {
	int T;
	const int32_t *left, *right;
	int root;
};

inline std::string schedule_error(const char *fmt, ...) {
	char buf[512];
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(buf, sizeof buf, fmt, ap);
	va_end(ap);
	return buf;
}

// The one tree check: every tip childless, every internal node with two distinct children in range, no node with two parents, the
// root a parentless internal node that reaches all N nodes.  Returns the error's text (empty: the tree is fine, and parent holds
// every node's parent, -1 for the root; after an error parent holds nothing of use).  call: the entry point's name for a tree that
// is item `item` of a batch, whose messages carry both.  order: if given, receives the nodes as the check's walk from the root
// meets them, parents before children
inline std::string validate_tree(const TreeRef &t, std::vector<int32_t> &parent, const char *call = nullptr, int item = 0, std::vector<int> *order = nullptr) {
	const int T = t.T, N = 2 * T - 1;
	const std::string where = call ? schedule_error("%s: item %d: ", call, item) : std::string();
	const char *w = where.c_str();
	parent.assign(N, -1);
	for (int n = 0; n < N; n++) {
		const int l = t.left[n], r = t.right[n];
		if (n < T) {
			if (l != -1 || r != -1) return schedule_error("%snode %d is a tip (id < tip_count) but has children", w, n);
			continue;
		}
		if (l < 0 || r < 0 || l >= N || r >= N || l == r) return schedule_error("%sinternal node %d has invalid children (%d, %d)", w, n, l, r);
		if (parent[l] >= 0 || parent[r] >= 0) return schedule_error("%snode %d or %d has two parents", w, l, r);
		parent[l] = n;
		parent[r] = n;
	}
	if (t.root < T || t.root >= N || parent[t.root] != -1) return schedule_error("%sroot %d is not a parentless internal node", w, t.root);
	// (no node has two parents and the root has none: the walk from the root meets no node twice)
	int reached = 0;
	std::vector<int> stack{t.root};
	if (order) order->clear(), order->reserve(N);
	while (!stack.empty()) {
		const int n = stack.back();
		stack.pop_back();
		reached++;
		if (order) order->push_back(n);
		if (n >= T) {
			stack.push_back(t.left[n]);
			stack.push_back(t.right[n]);
		}
	}
	if (reached != N) return schedule_error("%s%stopology is not a single binary tree over all %d nodes", w, call ? "the " : "", N);
	return std::string();
}

// everything a schedule depends on that is not the tree (the engine's: schedule_options, phyamd_shard.inc)
struct ScheduleOptions {
	int S = 4;                    // states; S != 4: the 20 / 60 / 61-state (MFMA) kernels
	bool keep_partials = false;   // every node's lower and upper partial stays resident: nothing fused, no walk lists
	bool scaling_on = false;      // the evaluation rescales (20 states: every node stored, no walk lists)
	bool fusion_enabled = true;   // fringe nodes are fused into their parents' ops
	bool generic_fusion = true;   // ... 20 states: cherries
	bool walk_enabled = true;     // depth-first walk lists are built
	bool lower_park2_on = true;   // the post-order walk parks in a second slot
};

// the lists of one tree under one set of options
struct Schedule {
	std::vector<int32_t> parent;      // -1: the root
	std::vector<int> node_kind;       // CH_* of every node
	std::vector<int32_t> core_index;  // node -> index of its stored lower array (-1: tip or fused)
	int core_count = 0;
	std::vector<DeepDesc> deep_host;  // by node id (only DEEP nodes filled)
	int deep_count = 0;
	bool fused = false;
	// walk lists were built (not keep_partials): 4 states / 20 states unscaled (phyamd_genwalk.inc)
	bool walking = false, gen_walking = false;
	// one launch per tree level
	std::vector<NodeOp> lower_ops, upper_ops;
	std::vector<int> lower_level_off, upper_level_off;  // offsets into the op arrays, one past the last at the end
	std::vector<int32_t> upper_slot;                    // node -> slot of its upper partial (-1 none)
	int upper_slots = 0;
	// depth-first op orders
	std::vector<NodeOp> walk_lower_ops, walk_upper_ops;
	int walk_upper_slots = 0;
	std::vector<NodeOp> walk_chunk_ops;  // chunked form of walk_upper_ops (chunk_pre_order)
	std::vector<int> walk_chunk_off;     // chunk offsets into walk_chunk_ops: [0] top part, then one per cut subtree
	int walk_chunk_slots = 0;
	std::vector<NodeOp> walk_lower_chunk_ops;  // chunked form of walk_lower_ops: cut subtrees, then the top part (chunk_post_order)
	std::vector<int> walk_lower_chunk_off;
};

// Chunked form of the pre-order walk (the launches with LDS park slots).  A workgroup's walk takes as long whatever shares its CU,
// and the card holds 1280 of them: 15 625 workgroups (1e6 patterns) are 12.2 rounds, i.e. 13, and 1 563 (1e5 patterns) are two.
// Cutting the op list into a top part and subtrees of at most 1 / WALK_CHUNKS of the ops that run as workgroups of their own
// (second launch, blockIdx.y = subtree) makes the rounds short and many, so the unfilled last one costs a fraction of a walk.
// A cut node's upper crosses from one workgroup to another through HBM; since the subtrees of one pattern block run at the same
// time, no HBM slot is recycled here (every HBM park has its own), and LDS parks stay inside a chunk.
// walk_chunk_ops: [top ops | subtree 1 | subtree 2 | ...], walk_chunk_off: offsets (chunks + 1 entries)
inline void chunk_pre_order(Schedule &sc) {
	const std::vector<NodeOp> &src = sc.walk_upper_ops;
	const int n = (int)src.size(), N = (int)sc.parent.size();
	sc.walk_chunk_ops = src;
	sc.walk_chunk_off.assign({0, n});
	sc.walk_chunk_slots = 0;
	if (n == 0) return;
	std::vector<int> opi(N, -1), size(n, 1);
	for (int i = 0; i < n; i++) opi[src[i].parent] = i;
	for (int i = n - 1; i >= 0; i--)
		for (int ch : {src[i].left, src[i].right})
			if (opi[ch] >= 0) size[i] += size[opi[ch]];
	const int target = std::max(16, (n + WALK_CHUNKS - 1) / WALK_CHUNKS);
	std::vector<char> top(n, 0), cut(n, 0);
	if (n >= 32) {
		std::vector<int> stack{0};
		while (!stack.empty()) {
			const int i = stack.back();
			stack.pop_back();
			top[i] = 1;
			for (int ch : {src[i].left, src[i].right}) {
				const int j = opi[ch];
				if (j < 0) continue;
				if (size[j] > target) stack.push_back(j);
				else cut[j] = 1;
			}
		}
	} else
		std::fill(top.begin(), top.end(), 1);  // one chunk: the whole list (with the slot fields of this form)
	// chunk of every op: 0 = the top part, m = the m-th cut subtree (in list order)
	std::vector<int> chunk_of(n, 0);
	int chunks = 1;
	for (int j = 0; j < n; j++)
		if (cut[j]) {
			for (int i = j; i < j + size[j]; i++) chunk_of[i] = chunks;
			chunks++;
		}
	// Where each child's upper goes: nowhere (carried inside a chunk), the LDS slot, an HBM slot private to the chunk (recycled
	// inside it like the one-list walk does: a slot is free again once its reader has run), or an HBM slot that crosses chunks
	// (unique).  Chunks of one pattern block run concurrently, so their private ranges are disjoint.
	enum { NONE = 0, LDS = 1, INTERNAL = 2, CROSS = 3 };
	std::vector<NodeOp> ops = src;
	std::vector<int> kind(2 * n, NONE), local(2 * n, -1);          // [op * 2 + side]
	std::vector<int> writer(n, -1);                                  // op j: index (op * 2 + side) of the entry that feeds it
	std::vector<std::vector<int>> free_list(chunks);
	std::vector<int> next_local(chunks, 0);
	int cross = 0;
	for (int i = 0; i < n; i++) {
		const int k = chunk_of[i];
		int freed = -1;
		if (writer[i] >= 0 && kind[writer[i]] == INTERNAL) freed = local[writer[i]];
		for (int side = 0; side < 2; side++) {
			const int ch = side ? src[i].right : src[i].left, j = opi[ch];
			if (j < 0) continue;
			const int w = i * 2 + side;
			writer[j] = w;
			const bool carried = src[i].carry_out == side + 1;
			const int lds_bit = side ? 4 : 2;
			if (carried && !cut[j]) kind[w] = NONE;
			else if (cut[j]) {  // a cut subtree (visited first or parked): its upper crosses to another workgroup through HBM
				kind[w] = CROSS;
				local[w] = cross++;
			} else if (src[i].lds_park & lds_bit) kind[w] = LDS;
			else {
				kind[w] = INTERNAL;
				std::vector<int> &fl = free_list[k];
				if (!fl.empty()) {
					local[w] = fl.back();
					fl.pop_back();
				} else
					local[w] = next_local[k]++;
			}
		}
		if (freed >= 0) free_list[k].push_back(freed);  // read by this op: reusable by the ops after it
	}
	std::vector<int> base(chunks + 1, 0);
	for (int k = 0; k < chunks; k++) base[k + 1] = base[k] + next_local[k];
	const int slots = base[chunks] + cross;
	for (int i = 0; i < n; i++)
		for (int side = 0; side < 2; side++) {
			const int ch = side ? src[i].right : src[i].left, j = opi[ch];
			if (j < 0) continue;
			const int w = i * 2 + side, lds_bit = side ? 4 : 2;
			int32_t &slot = side ? ops[i].upper_slot_right : ops[i].upper_slot_left;
			if (kind[w] == NONE) slot = -1;
			else if (kind[w] == LDS) {
				slot = -1;
				ops[j].upper_slot_parent = -1;  // (lds_park bit 0 of the reader is set in the source list)
			} else {
				slot = kind[w] == INTERNAL ? base[chunk_of[i]] + local[w] : base[chunks] + local[w];
				ops[i].lds_park &= ~lds_bit;
				if (kind[w] == CROSS) {  // (second LDS slot of the streamed walk: inside one workgroup only)
					ops[i].lds_park &= ~(side ? 0x40 : 0x20);
					ops[j].lds_park &= ~0x10;
				}
				ops[j].carry_in = 0;
				ops[j].upper_slot_parent = slot;
				ops[j].lds_park &= ~1;
			}
		}
	sc.walk_chunk_ops.clear();
	sc.walk_chunk_off.assign(1, 0);
	for (int i = 0; i < n; i++)
		if (top[i] && !cut[i]) sc.walk_chunk_ops.push_back(ops[i]);
	sc.walk_chunk_off.push_back((int)sc.walk_chunk_ops.size());
	std::vector<int> cuts;
	for (int j = 0; j < n; j++)
		if (cut[j]) cuts.push_back(j);
	std::stable_sort(cuts.begin(), cuts.end(), [&](int a, int b) { return size[a] > size[b]; });  // longest first: the launch's last workgroups are the short ones
	for (int j : cuts) {
		for (int i = j; i < j + size[j]; i++) sc.walk_chunk_ops.push_back(ops[i]);
		sc.walk_chunk_off.push_back((int)sc.walk_chunk_ops.size());
	}
	sc.walk_chunk_slots = slots;
	sc.walk_upper_slots = std::max(sc.walk_upper_slots, slots);
}

// The same for the post-order walk: cut subtrees first (second index of the launch = subtree), then the top part, which reads a cut
// subtree's root like any stored child.  Carries follow the op actually in front of an op in its chunk, and an op next to a cut
// gives up its parks (both slots) together with their writers' bits: a cut child was parked by another workgroup, and the other
// child of such an op is either cut as well or the op in front of it in the top part, i.e. carried -- no park is lost that could
// have been kept, and a park that survives has its writer and its reader in one chunk.
// walk_lower_chunk_ops: [subtree 1 | subtree 2 | ... | top], offsets in walk_lower_chunk_off.
inline void chunk_post_order(Schedule &sc) {
	const std::vector<NodeOp> &src = sc.walk_lower_ops;
	const int n = (int)src.size(), N = (int)sc.parent.size();
	sc.walk_lower_chunk_ops = src;
	sc.walk_lower_chunk_off.assign({0, n});
	if (n == 0) return;
	std::vector<int> opi(N, -1), size(n, 1);
	for (int i = 0; i < n; i++) opi[src[i].parent] = i;
	for (int i = 0; i < n; i++)  // post-order: children's ops come first
		for (int ch : {src[i].left, src[i].right})
			if (opi[ch] >= 0) size[i] += size[opi[ch]];
	const int target = std::max(16, (n + WALK_CHUNKS - 1) / WALK_CHUNKS);
	if (n < 32) return;
	std::vector<char> cut(n, 0), in_cut(n, 0);
	std::vector<int> stack{n - 1};  // the root's op is the last one
	while (!stack.empty()) {
		const int i = stack.back();
		stack.pop_back();
		for (int ch : {src[i].left, src[i].right}) {
			const int j = opi[ch];
			if (j < 0) continue;
			if (size[j] > target) stack.push_back(j);
			else cut[j] = 1;
		}
	}
	std::vector<NodeOp> out;
	std::vector<int> off{0}, cuts, at(n, -1);  // at: op of the source list -> its place in `out`
	for (int j = 0; j < n; j++)
		if (cut[j]) cuts.push_back(j);
	std::stable_sort(cuts.begin(), cuts.end(), [&](int a, int b) { return size[a] > size[b]; });  // longest first
	for (int j : cuts) {
		for (int i = j - size[j] + 1; i <= j; i++) {
			in_cut[i] = 1;
			at[i] = (int)out.size();
			out.push_back(src[i]);
		}
		out[off.back()].carry_in = 0;  // (a subtree's first op has two unstored children anyway)
		off.push_back((int)out.size());
	}
	int prev = -1;  // node of the op in front, inside the top part
	for (int i = 0; i < n; i++) {
		if (in_cut[i]) continue;
		NodeOp op = src[i];
		const int jl = opi[op.left], jr = opi[op.right];
		const bool next_to_cut = (jl >= 0 && cut[jl]) || (jr >= 0 && cut[jr]);
		op.carry_in = prev >= 0 && prev == op.left ? 1 : prev >= 0 && prev == op.right ? 2 : 0;
		if (next_to_cut) {
			for (int side = 0; side < 2; side++) {
				const int j = side ? jr : jl;
				if (op.lds_park & (side ? 2 : 1)) out[at[j]].lds_park &= ~4;
				if (op.lds_park & (side ? 0x20 : 0x10)) out[at[j]].lds_park &= ~0x40;
			}
			op.lds_park &= ~0x33;
		}
		at[i] = (int)out.size();
		out.push_back(op);
		prev = op.parent;
	}
	off.push_back((int)out.size());
	sc.walk_lower_chunk_ops = out;
	sc.walk_lower_chunk_off = off;
}

// build_schedule's working state: the tree, the options, the traversal and classification its four parts share
struct ScheduleBuilder {
	const int T, N, root;
	const int32_t *const left, *const right;
	const ScheduleOptions &o;
	const bool generic;
	Schedule &sc;
	std::vector<int> depth, order;  // depth (root = 0); every node, parents before children (validate_tree's walk)
	std::vector<int> kind;          // CH_* (Schedule::node_kind)

	ScheduleBuilder(const TreeRef &t, const ScheduleOptions &opt, Schedule &sched)
	    : T(t.T), N(2 * t.T - 1), root(t.root), left(t.left), right(t.right), o(opt), generic(opt.S != 4), sc(sched) {}

	void describe(int ch, int32_t &k, int32_t &core, int32_t &t0, int32_t &t1, int32_t &t2, int32_t &inner) const {
		k = kind[ch];
		core = sc.core_index[ch];
		t0 = t1 = t2 = inner = -1;
		if (k == CH_CHERRY) {
			t0 = left[ch];
			t1 = right[ch];
		} else if (k == CH_CHERRY_TIP) {
			const int l = left[ch], r = right[ch];
			inner = l < T ? r : l;
			t2 = l < T ? l : r;
			t0 = left[inner];
			t1 = right[inner];
		}
	}
	NodeOp make_op(int n) const {
		NodeOp op{};
		op.parent = n;
		op.left = left[n];
		op.right = right[n];
		op.upper_slot_parent = op.upper_slot_left = op.upper_slot_right = -1;
		op.core_parent = sc.core_index[n];
		describe(op.left, op.kind_left, op.core_left, op.lt0, op.lt1, op.lt2, op.linner);
		describe(op.right, op.kind_right, op.core_right, op.rt0, op.rt1, op.rt2, op.rinner);
		return op;
	}

	void classify() {
		// depth (root = 0) along the tree check's walk
		depth.assign(N, 0);
		for (int i = 1; i < N; i++) depth[order[i]] = depth[sc.parent[order[i]]] + 1;
		// Fringe classification (4-state, not keep_partials): cherries (tip, tip) and cherry + tip nodes are fused
		// into their parent's work and never stored.  Everything else that is internal is a "core" node with an array in HBM.
		// (rescaled evaluations keep the fusion: fringe nodes never reach the rescaling threshold themselves)
		// 20 states: cherries only, and only in plain evaluations -- the MFMA kernels rebuild a cherry's partial from two columns of
		// LDS-resident matrix images (six images of 5 KB fit; 61-state images are 33 KB each) and push its upper down in registers;
		// rescaled evaluations keep every node stored (their per-op scratch rows are indexed by the level's ops).
		const bool fuse = o.fusion_enabled && !o.keep_partials && (!generic || (o.S == 20 && !o.scaling_on && o.generic_fusion));
		sc.fused = fuse;
		kind.assign(N, CH_CORE);
		for (int n = 0; n < T; n++) kind[n] = CH_TIP;
		if (fuse) {
			for (int i = N - 1; i >= 0; i--) {  // children before parents
				const int n = order[i];
				if (n < T || n == root) continue;
				const int l = left[n], r = right[n];
				if (l < T && r < T) kind[n] = CH_CHERRY;
				else if (generic) continue;
				else if ((l < T && kind[r] == CH_CHERRY) || (r < T && kind[l] == CH_CHERRY)) kind[n] = CH_CHERRY_TIP;
				else if (kind[l] != CH_CORE && kind[l] != CH_DEEP && kind[r] != CH_CORE && kind[r] != CH_DEEP)
					kind[n] = CH_DEEP;  // both children are tips or fringe: 4-6 tips below, rebuilt in registers wherever its partial is needed
			}
		}
		sc.node_kind = kind;
		// stored lower arrays: core nodes in id order
		sc.core_index.assign(N, -1);
		sc.core_count = 0;
		for (int n = T; n < N; n++)
			if (kind[n] == CH_CORE) sc.core_index[n] = sc.core_count++;
		sc.deep_host.assign(N, DeepDesc{});
		sc.deep_count = 0;
		for (int n = T; n < N; n++)
			if (kind[n] == CH_DEEP) {
				DeepDesc &d = sc.deep_host[n];
				int32_t core_unused;
				d.left = left[n];
				d.right = right[n];
				describe(d.left, d.kind_left, core_unused, d.lt0, d.lt1, d.lt2, d.linner);
				describe(d.right, d.kind_right, core_unused, d.rt0, d.rt1, d.rt2, d.rinner);
				sc.deep_count++;
			}
	}

	void level_lists() {
		// height over the core tree (tips and fused nodes = 0), children before parents: reverse of the pre-order list
		std::vector<int> height(N, 0);
		int H = 0, Dmax = 0;
		for (int i = N - 1; i >= 0; i--) {
			const int n = order[i];
			if (kind[n] == CH_CORE) height[n] = 1 + std::max(height[left[n]], height[right[n]]);
			H = std::max(H, height[n]);
			Dmax = std::max(Dmax, depth[n]);
		}
		// lower levels: core nodes by height 1..H (the root has the largest height and is alone on its level)
		sc.lower_ops.clear();
		sc.lower_ops.reserve(N - T);  // (at most one op per internal node, here and in the lists below: a fresh Schedule grows once)
		sc.lower_level_off.assign(1, 0);
		for (int h = 1; h <= H; h++) {
			for (int n = T; n < N; n++)
				if (kind[n] == CH_CORE && height[n] == h) sc.lower_ops.push_back(make_op(n));
			sc.lower_level_off.push_back((int)sc.lower_ops.size());
		}
		// upper levels: core parents by depth 0..Dmax-1.  Upper partials of depth-d nodes are only read while
		// depth d+1 is produced, so slots are recycled two levels later (keep_partials: slot = own index).
		sc.upper_ops.clear();
		sc.upper_ops.reserve(N - T);
		sc.upper_level_off.assign(1, 0);
		sc.upper_slot.assign(N, -1);
		std::vector<int> free_slots;
		int next_slot = 0;
		std::vector<std::vector<int>> slots_of_depth(Dmax + 2);
		for (int d = 0; d < Dmax; d++) {
			if (!o.keep_partials && d >= 2) {  // uppers of depth d-1 were consumed while producing depth d
				for (int s : slots_of_depth[d - 1]) free_slots.push_back(s);
				slots_of_depth[d - 1].clear();
			}
			for (int n = T; n < N; n++) {
				if (depth[n] != d || (kind[n] != CH_CORE && kind[n] != CH_DEEP)) continue;
				NodeOp op = make_op(n);
				op.upper_slot_parent = n == root ? -1 : sc.upper_slot[n];
				for (int side = 0; side < 2; side++) {
					const int ch = side ? right[n] : left[n];
					if (kind[ch] != CH_CORE && kind[ch] != CH_DEEP && !o.keep_partials) continue;  // uppers of tips and fringe nodes stay in registers
					int s;
					if (o.keep_partials) s = ch;
					else if (!free_slots.empty()) {
						s = free_slots.back();
						free_slots.pop_back();
					} else
						s = next_slot++;
					sc.upper_slot[ch] = s;
					slots_of_depth[d + 1].push_back(s);
					(side ? op.upper_slot_right : op.upper_slot_left) = s;
				}
				sc.upper_ops.push_back(op);
			}
			sc.upper_level_off.push_back((int)sc.upper_ops.size());
		}
		sc.upper_slots = o.keep_partials ? N : next_slot;
	}

	// Depth-first op orders for the tree-walk kernels (see k_lower4_walk).
	void walk_post_order() {
		std::vector<int> csize(N, 0);  // stored nodes in the subtree
		for (int i = N - 1; i >= 0; i--) {
			const int n = order[i];
			if (kind[n] == CH_CORE) csize[n] = 1 + csize[left[n]] + csize[right[n]];
		}
		// post-order, larger core subtree first: the op before a node is its second (smaller) core child, or its only one
		struct Frame {
			int node, stage;
		};
		// two_core[n]: the subtree of n holds a node with two stored children, i.e. walking it re-reads a stored partial
		// lparks[n]: the largest number of stored partials that wait at one time while the subtree of n is walked (the first-walked
		// child of a node with two stored children waits while the second one's subtree is walked); two_core[n] = lparks[n] > 0
		std::vector<uint8_t> two_core(N, 0);
		std::vector<int> lparks(N, 0);
		for (int i = N - 1; i >= 0; i--) {
			const int n = order[i];
			if (kind[n] != CH_CORE) continue;
			const int l = left[n], r = right[n];
			const bool lo = kind[l] == CH_CORE, ro = kind[r] == CH_CORE;
			two_core[n] = (lo && ro) || (lo && two_core[l]) || (ro && two_core[r]);
			if (lo && ro) lparks[n] = csize[l] >= csize[r] ? std::max(lparks[l], 1 + lparks[r]) : std::max(lparks[r], 1 + lparks[l]);
			else lparks[n] = lo ? lparks[l] : ro ? lparks[r] : 0;
		}
		std::vector<int> lower_op_of(N, -1);
		std::vector<Frame> st{{root, 0}};
		while (!st.empty()) {
			Frame &f = st.back();
			const int n = f.node, l = left[n], r = right[n];
			const int first = csize[l] >= csize[r] ? l : r, second = first == l ? r : l;
			if (f.stage == 0) {
				f.stage = 1;
				if (kind[first] == CH_CORE) st.push_back({first, 0});
			} else if (f.stage == 1) {
				f.stage = 2;
				if (kind[second] == CH_CORE) st.push_back({second, 0});
			} else {
				NodeOp op = make_op(n);
				op.carry_in = 0;
				if (!sc.walk_lower_ops.empty()) {
					const int prev = sc.walk_lower_ops.back().parent;
					if (prev == l) op.carry_in = 1;
					else if (prev == r) op.carry_in = 2;
				}
				// Both children stored: the second one arrives in registers, the first was written a subtree ago.  If walking the
				// second's subtree re-reads nothing itself, the first can also wait in the wave's LDS slot (it is still stored for
				// the pre-order pass): bit 2 on the child's op = keep a copy in LDS, bit 0 / 1 here = left / right child from LDS.
				// Second tier (the streamed walk only; the pre-order walk's in_lds2 rule): if every wait inside the second's subtree is
				// of that kind, i.e. at most one of them is held at a time, the first waits in the wave's second slot: bit 0x40 on the
				// child's op = keep a copy there, bit 0x10 / 0x20 here = left / right child from it.  No slot then ever holds two values.
				op.lds_park = 0;
				if (kind[first] == CH_CORE && kind[second] == CH_CORE && lower_op_of[first] >= 0) {
					if (!two_core[second]) {
						sc.walk_lower_ops[lower_op_of[first]].lds_park |= 4;
						op.lds_park |= first == l ? 1 : 2;
					} else if (o.lower_park2_on && lparks[second] == 1) {
						sc.walk_lower_ops[lower_op_of[first]].lds_park |= 0x40;
						op.lds_park |= first == l ? 0x10 : 0x20;
					}
				}
				lower_op_of[n] = (int)sc.walk_lower_ops.size();
				sc.walk_lower_ops.push_back(op);
				st.pop_back();
			}
		}
	}

	void walk_pre_order() {
		std::vector<int> usize(N, 0);  // pre-order ops (stored + DEEP) in the subtree
		for (int i = N - 1; i >= 0; i--) {
			const int n = order[i];
			if (kind[n] == CH_CORE || kind[n] == CH_DEEP) usize[n] = 1 + usize[left[n]] + usize[right[n]];
		}
		// pre-order, SMALLER core subtree first: the first-visited core child takes its upper in registers (never stored);
		// the other child's upper waits in a slot while the small subtree is walked (nesting depth <= log2 of the core count)
		// parks[n]: the subtree of n holds an op with two op-children, i.e. walking it parks an upper
		// height[n]: the largest number of uppers parked at one time while the subtree of n is walked
		std::vector<uint8_t> parks(N, 0), in_lds(N, 0), in_lds2(N, 0);
		std::vector<int> height(N, 0);
		for (int i = N - 1; i >= 0; i--) {
			const int n = order[i];
			if (kind[n] != CH_CORE && kind[n] != CH_DEEP) continue;
			const int l = left[n], r = right[n];
			const bool lo = kind[l] == CH_CORE || kind[l] == CH_DEEP, ro = kind[r] == CH_CORE || kind[r] == CH_DEEP;
			parks[n] = (lo && ro) || (lo && parks[l]) || (ro && parks[r]);
			if (lo && ro) {
				const int first = usize[l] <= usize[r] ? l : r, second = first == l ? r : l;
				height[n] = std::max(1 + height[first], height[second]);
			} else
				height[n] = lo ? height[l] : ro ? height[r] : 0;
		}
		std::vector<int> free_w;
		int next_w = 0;
		std::vector<int> slot_of(N, -1);
		std::vector<int> stack2{root};
		int carried_node = -1;  // node whose upper the previous op carried out
		while (!stack2.empty()) {
			const int n = stack2.back();
			stack2.pop_back();
			NodeOp op = make_op(n);
			op.carry_in = (n != root && carried_node == n) ? 1 : 0;
			op.upper_slot_parent = -1;
			op.lds_park = 0;
			if (n != root && !op.carry_in) {
				op.upper_slot_parent = slot_of[n];
				free_w.push_back(slot_of[n]);  // read by this op; reusable by ops after it
				if (in_lds[n]) op.lds_park |= 1;
				if (in_lds2[n]) op.lds_park |= 0x10;
			}
			const int l = left[n], r = right[n];
			const bool lc = kind[l] == CH_CORE || kind[l] == CH_DEEP, rc2 = kind[r] == CH_CORE || kind[r] == CH_DEEP;  // children with ops of their own
			int first = -1, second = -1;
			if (lc && rc2) {
				first = usize[l] <= usize[r] ? l : r;
				second = first == l ? r : l;
			} else if (lc || rc2)
				first = lc ? l : r;
			op.carry_out = first < 0 ? 0 : (first == l ? 1 : 2);
			carried_node = first;
			if (second >= 0) {
				int sl;
				// a slot freed by THIS op (its own parent upper) must not be reused for its output: lanes of other waves may
				// still be reading it -- not an issue within a thread, but keep it simple and safe: take another one
				if (free_w.size() > 1 || (free_w.size() == 1 && free_w.back() != op.upper_slot_parent)) {
					size_t pick = free_w.size() - 1;
					if (free_w[pick] == op.upper_slot_parent) pick--;
					sl = free_w[pick];
					free_w.erase(free_w.begin() + pick);
				} else
					sl = next_w++;
				slot_of[second] = sl;
				(second == l ? op.upper_slot_left : op.upper_slot_right) = sl;
				if (!parks[first]) {  // nothing else is parked while `second` waits: one LDS slot per wave is enough
					in_lds[second] = 1;
					op.lds_park |= second == l ? 2 : 4;
				} else if (height[first] == 1) {
					// one park at a time inside the wait (leaf parks, all of them in LDS slot 0): the streamed walk keeps this one in
					// a second LDS slot (bits 0x20 / 0x40 store, 0x10 read); the other kernels park it in the HBM slot assigned above
					in_lds2[second] = 1;
					op.lds_park |= second == l ? 0x20 : 0x40;
				}
				stack2.push_back(second);
			}
			if (first >= 0) stack2.push_back(first);  // visited next
			sc.walk_upper_ops.push_back(op);
		}
		sc.walk_upper_slots = next_w;
	}
};

// Build the level schedule, the upper-slot assignment and the walk lists of a tree.  Returns the tree check's error text (empty: fine);
// an error leaves *out untouched.
inline std::string build_schedule(const TreeRef &tree, const ScheduleOptions &options, Schedule *out) {
	Schedule &sc = *out;
	ScheduleBuilder b(tree, options, sc);
	std::vector<int32_t> parent;
	std::string err = validate_tree(tree, parent, nullptr, 0, &b.order);
	if (!err.empty()) return err;
	const ScheduleOptions &o = options;
	const bool generic = o.S != 4;
	sc.parent = std::move(parent);
	b.classify();
	b.level_lists();
	sc.walking = o.walk_enabled && !generic && !o.keep_partials;
	// 20 states, plain evaluations: the post-order list drives k_lower_gen_walk (phyamd_genwalk.inc)
	sc.gen_walking = o.walk_enabled && generic && o.S == 20 && !o.keep_partials && !o.scaling_on;
	sc.walk_lower_ops.clear();
	sc.walk_upper_ops.clear();
	sc.walk_upper_slots = 0;
	if (sc.walking || sc.gen_walking) {
		sc.walk_lower_ops.reserve(tree.T - 1);
		sc.walk_upper_ops.reserve(tree.T - 1);
		b.walk_post_order();
		b.walk_pre_order();
		if (sc.walking) {
			chunk_pre_order(sc);
			chunk_post_order(sc);
		}
	}
	return std::string();
}

// what the streamed walks' byte offsets are multiplied out for: patterns per tile, categories, dwords per mask row
struct StreamGeometry {
	int P, C;
	size_t mstride;
	bool elide = false;  // stream_elide: the post-order walk stops storing the nodes the pre-order walk can form beside a tip or a cherry
	bool pairs = false;  // stream_pairs: a third descriptor set in which a DEEP child's pre-order op runs inside its parent's
	bool keep = false;   // stream_keep: an elided child's op, where it runs next, takes its stored child's plane from its parent's op in registers
};

// a stored node the streamed walks no longer store (stream_elide)
struct StreamElision {
	int32_t node, parent, stored, sibling, sibling_kind;  // its parent, its stored child, its other child (CH_TIP / CH_CHERRY)
	int32_t source;                                       // how the post-order walk hands it to its parent: 1 the op in front, 2 park slot 0
	int32_t side;                                         // the side it has in its parent's pre-order op (0 left, 1 right)
	int32_t chunk;                                        // the post-order chunk of both ops
};

// what stream_keep decided for one elided node
enum { KEEP_KEPT = 0, KEEP_NOT_NEXT = 1, KEEP_OTHER_SIDE = 2, KEEP_OPENER = 3, KEEP_OFF = 4 };
struct StreamKeep {
	int32_t node, parent, side;  // the elided node, its parent, the side it has in its parent's pre-order op (StreamElision)
	int32_t reason;              // KEEP_KEPT, or why its own op requests its stored child's plane again: the op is not the next of its
	                             // parent's chunk (its upper is parked, or the other child is walked first); the stored child sits on
	                             // the other side there; the op opens a chunk (the prologue fetches its operands); the switch is off
};

// what stream_pairs decided for one pre-order op
enum { PAIR_FUSED = 0, PAIR_NO_DEEP = 1, PAIR_NOT_NEXT = 2, PAIR_SIBLING = 3, PAIR_BLOCK = 4, PAIR_ABSORBED = 5 };
struct StreamPair {
	int32_t node;          // the op's node
	int32_t reason;        // PAIR_FUSED, or why not: no DEEP child; no DEEP child's op directly behind in the chunk; the other child
	                       // neither stored nor a tip; a tip beside a DEEP child of five or six tips; the op runs inside the pair in front
	int32_t child;         // the DEEP child the rule looked at (-1: none)
	int32_t sibling, sibling_kind;  // the other child and its kind in the descriptor (CH_*, SK_*)
	int32_t child_tips;    // tips of `child`
	int32_t carry;         // fused: 1 = the op behind the pair is the sibling's and takes its upper in registers
};

// the streamed 4-state walks' host tables (phyamd_walk4s.inc), built from the chunked lists of a Schedule for one geometry
struct StreamTables {
	std::vector<StreamOp> ops;      // one per op of walk_chunk_ops
	std::vector<StreamDesc> desc;   // ... as the kernel reads them (byte offsets multiplied out for P patterns, mstride)
	int P = 0;
	size_t mstride = 0;
	std::vector<StreamChunk> chunks;
	std::vector<LowerDesc> lower_desc;  // k_lower4_stream: one per op of walk_lower_chunk_ops (empty: the post-order walk does not stream)
	std::vector<LowerChunk> lower_chunks;
	std::vector<int> row_entries;   // [rows][8] nibbles of the packed mask words (MaskPacker): the pre-order walk's rows, then the post-order walk's
	std::vector<int> site_tab;      // [ops][16] byte offset of each result lane's branch in a slab row (-1: none)
	std::vector<int> qnode;         // slab position -> node
	std::vector<int> op_tips;       // [ops][12] tip of every table slot (-1: unused)
	std::vector<int> op_deep;       // [ops] bit 0 / 1: the left / right child is a DEEP node (its table slots hold messages only)
	// stream_elide (StreamGeometry::elide; otherwise empty): the pre-order walk's descriptors and chunks as they were before it, for a
	// pass over stored lowers in the reference's form, and the nodes it took out
	std::vector<StreamDesc> plain_desc;
	std::vector<StreamChunk> plain_chunks;
	std::vector<StreamElision> elisions;
	// stream_keep (with the elisions; otherwise empty): one decision per elided node, in their order
	std::vector<StreamKeep> keeps;
	// stream_pairs (StreamGeometry::pairs; otherwise empty): a copy of `desc` with the pair ops, for the plain TF pass; the pair
	// blocks' position tables [ops][16] (OPBLK_PAIR_SITES); the decision per op
	std::vector<StreamDesc> pair_desc;
	std::vector<int> pair_tab;
	std::vector<StreamPair> pairs;
	int words = 0, R = 0;           // mask rows of both walks; slab positions
};

// Packed mask groups (phyamd_walk4s.inc, "Mask words"): the tips of one child of one op = one group = flag bit + one nibble per tip
// slot (slots keep their positions: a DEEP child's halves sit at nibbles 0..2 and 3..5), appended to the current dword row while it
// fits; a walk's groups are packed in its own op order.  rows: [row][8] entries for k_build_mask_stream.
struct MaskPacker {
	std::vector<int> &rows;
	int row = -1, used = 32, entries = 8;
	explicit MaskPacker(std::vector<int> &r) : rows(r), row((int)r.size() / 8 - 1) {}
	void add(const int *tips, int &out_row, int &out_shift) {  // tips[6], -1 = unused slot
		int span = 0, n = 0;
		for (int j = 0; j < 6; j++)
			if (tips[j] >= 0) {
				span = j + 1;
				n++;
			}
		const int bits = 1 + 4 * span;
		if (used + bits > 32 || entries + n > 8) {
			rows.insert(rows.end(), 8, -1);
			row++;
			used = 0;
			entries = 0;
		}
		out_row = row;
		out_shift = used;
		for (int j = 0; j < 6; j++)
			if (tips[j] >= 0) rows[(size_t)row * 8 + entries++] = tips[j] | (used + 1 + 4 * j) << 20 | used << 25;
		used += bits;
	}
};

// Flattened form of the chunked pre-order list for k_upper4_stream (phyamd_walk4s.inc): one 128-byte descriptor per op with its
// DEEP children expanded, the mask groups (one per child that has tips: nibble j = the child's j-th tip, a DEEP child's halves at
// nibbles 0..2 and 3..5; MaskPacker), what the NEXT op of the chunk wants prefetched, and each op's slab positions in walk order.
// Every op's children are ordered so that the one whose upper the next op takes in registers is the LEFT one.
inline void stream_pre_order(const Schedule &sc, const StreamGeometry &g, StreamTables &t) {
	const int n = (int)sc.walk_chunk_ops.size();
	t.ops.assign(n, StreamOp{});
	t.chunks.clear();
	t.row_entries.clear();
	t.site_tab.assign((size_t)n * 16, -1);
	t.op_tips.assign((size_t)n * 12, -1);
	t.op_deep.assign(n, 0);
	t.qnode.clear();
	t.words = 0;
	if (n == 0) return;
	std::vector<NodeOp> src = sc.walk_chunk_ops;
	std::vector<char> chunk_start(n + 1, 0);
	for (int off : sc.walk_chunk_off) chunk_start[off] = 1;
	// In the chunked list the op in front may have produced this op's upper for an HBM slot (its carried child was cut away): a
	// prefetch would read the slot before that op's store, and the value is in its registers anyway -- it is carried instead.
	std::vector<char> from_prev(n, 0);
	for (int i = 1; i < n; i++) {
		const NodeOp &o = src[i];
		NodeOp &pv = src[i - 1];
		const bool proot = o.upper_slot_parent < 0 && !o.carry_in && !(o.lds_park & 1);
		if (chunk_start[i] || proot || o.carry_in || (o.lds_park & 0x11) || o.upper_slot_parent < 0) continue;
		if (pv.upper_slot_left == o.upper_slot_parent) {
			pv.carry_out = 1;
			pv.upper_slot_left = -1;
			from_prev[i] = 1;
		} else if (pv.upper_slot_right == o.upper_slot_parent) {
			pv.carry_out = 2;
			pv.upper_slot_right = -1;
			from_prev[i] = 1;
		}
	}
	for (NodeOp &o : src)
		if (o.carry_out == 2) {  // the carried child becomes the left one
			std::swap(o.left, o.right);
			std::swap(o.core_left, o.core_right);
			std::swap(o.kind_left, o.kind_right);
			std::swap(o.lt0, o.rt0);
			std::swap(o.lt1, o.rt1);
			std::swap(o.lt2, o.rt2);
			std::swap(o.linner, o.rinner);
			std::swap(o.upper_slot_left, o.upper_slot_right);
			o.lds_park = (o.lds_park & 0x11) | ((o.lds_park & 2) ? 4 : 0) | ((o.lds_park & 4) ? 2 : 0) | ((o.lds_park & 0x20) ? 0x40 : 0) | ((o.lds_park & 0x40) ? 0x20 : 0);
			o.carry_out = 1;
		}
	auto half_kind = [](int k) { return k == CH_TIP ? HK_TIP : k == CH_CHERRY ? HK_CHERRY : HK_CHERRY_TIP; };
	std::vector<int> first_word(n, -1), words(n, 0), same_row(n, 0), want_a(n, -1), want_b(n, -1), want_u(n, -1);
	MaskPacker packer(t.row_entries);
	for (int i = 0; i < n; i++) {
		const NodeOp &o = src[i];
		StreamOp &s = t.ops[i];
		const bool proot = o.upper_slot_parent < 0 && !o.carry_in && !(o.lds_park & 1) && !from_prev[i];
		int fl = (o.kind_left & 7) | (o.kind_right & 7) << 3;
		fl |= ((o.lds_park & 2) ? 1 : (o.lds_park & 4) ? 2 : 0) << 12;
		s.parent = o.parent;
		s.slot_parent = o.upper_slot_parent;
		s.slot_left = o.upper_slot_left;
		s.slot_right = o.upper_slot_right;
		const bool lds2_on = STREAM_PARK_SLOTS > 1;
		if (lds2_on && (o.lds_park & 0x60)) {  // parked in the wave's second LDS slot instead of its HBM slot
			fl |= ((o.lds_park & 0x20) ? 1 : 2) << 12 | 1 << 6;
			((o.lds_park & 0x20) ? s.slot_left : s.slot_right) = -1;
		}
		s.lnode = o.left;
		s.rnode = o.right;
		for (int side = 0; side < 2; side++) {
			const int kind = side ? o.kind_right : o.kind_left, node = side ? o.right : o.left;
			int32_t *a = side ? s.ra : s.la;
			for (int j = 0; j < 10; j++) a[j] = -1;
			int tips[8] = {-1, -1, -1, -1, -1, -1, -1, -1};
			if (kind == CH_TIP) tips[0] = node;
			else if (kind == CH_CHERRY || kind == CH_CHERRY_TIP) {
				a[0] = side ? o.rt0 : o.lt0;
				a[1] = side ? o.rt1 : o.lt1;
				a[2] = side ? o.rt2 : o.lt2;
				a[3] = side ? o.rinner : o.linner;
				tips[0] = a[0];
				tips[1] = a[1];
				if (kind == CH_CHERRY_TIP) tips[2] = a[2];
			} else if (kind == CH_DEEP) {
				const DeepDesc &d = sc.deep_host[node];
				t.op_deep[i] |= 1 << side;
				for (int h = 0; h < 2; h++) {
					const int hk = h ? d.kind_right : d.kind_left;
					int32_t *q = a + 5 * h;
					q[0] = h ? d.right : d.left;
					q[1] = h ? d.rt0 : d.lt0;
					q[2] = h ? d.rt1 : d.lt1;
					q[3] = h ? d.rt2 : d.lt2;
					q[4] = h ? d.rinner : d.linner;
					fl |= half_kind(hk) << (16 + 4 * side + 2 * h);
					if (hk == CH_TIP) tips[3 * h] = q[0];
					else {
						tips[3 * h] = q[1];
						tips[3 * h + 1] = q[2];
						if (hk == CH_CHERRY_TIP) tips[3 * h + 2] = q[3];
					}
				}
			}
			for (int j = 0; j < 6; j++) t.op_tips[(size_t)i * 12 + 6 * side + j] = tips[j];
			if (kind != CH_CORE) {
				int row, shift;
				packer.add(tips, row, shift);
				if (words[i] == 0) first_word[i] = row;
				else same_row[i] = row == first_word[i];
				s.wsh |= shift << (5 * words[i]);
				words[i]++;
			}
		}
		// where the parent's upper comes from, and what the two register sets must hold when this op starts
		int usrc;
		if (o.kind_left == CH_CORE) want_a[i] = o.core_left;
		if (o.kind_right == CH_CORE) want_b[i] = o.core_right;
		if (proot) usrc = SU_ROOT;
		else if (o.carry_in || from_prev[i]) usrc = SU_CARRY;
		else if (o.lds_park & 1) usrc = SU_LDS;
		else if (lds2_on && (o.lds_park & 0x10)) {
			usrc = SU_LDS;
			fl |= 1 << 7;
		} else {
			usrc = SU_U;
			want_u[i] = o.upper_slot_parent;
		}
		fl |= usrc << 9;
		s.flags = fl;
		// slab positions, in the order the walk produces them; entry j belongs to result lane class j (k_upper4_stream: cid)
		const int sites[10] = {o.left, o.kind_left >= CH_CHERRY ? o.lt0 : -1, o.kind_left >= CH_CHERRY ? o.lt1 : -1, o.kind_left == CH_CHERRY_TIP ? o.linner : -1,
		                       o.right, o.kind_right >= CH_CHERRY ? o.rt0 : -1, o.kind_right >= CH_CHERRY ? o.rt1 : -1, o.kind_right == CH_CHERRY_TIP ? o.rinner : -1,
		                       o.kind_left == CH_CHERRY_TIP ? o.lt2 : -1, o.kind_right == CH_CHERRY_TIP ? o.rt2 : -1};
		for (int j = 0; j < 10; j++)
			if (sites[j] >= 0) {
				t.site_tab[(size_t)i * 16 + j] = 8 * (int)t.qnode.size();
				t.qnode.push_back(sites[j]);
			}
	}
	t.R = (int)t.qnode.size();
	t.words = (int)t.row_entries.size() / 8;  // (stream_post_order appends the post-order walk's rows)
	const int chunks = (int)sc.walk_chunk_off.size() - 1;
	for (int k = 0; k < chunks; k++) {
		const int b = sc.walk_chunk_off[k], en = sc.walk_chunk_off[k + 1];
		StreamChunk ch{-1, 0, -1, -1, -1, 0, {0, 0}};
		if (b < en) ch = StreamChunk{first_word[b], words[b], want_a[b], want_b[b], want_u[b], same_row[b], {0, 0}};
		t.chunks.push_back(ch);
		for (int i = b; i < en; i++) {
			StreamOp &s = t.ops[i];
			const bool last = i + 1 == en;
			s.nx_mask_word = last ? -1 : first_word[i + 1];
			s.flags |= (last ? 0 : words[i + 1]) << 14;
			s.flags |= (!last && src[i + 1].kind_right != CH_CORE ? 1 : 0) << 24;  // the right child's tip slots are the block's second piece
			s.flags |= (!last && same_row[i + 1] ? 1 : 0) << 25;
			s.nx_a = last ? -1 : want_a[i + 1];
			s.nx_b = last ? -1 : want_b[i + 1];
			s.nx_u = last ? -1 : want_u[i + 1];
		}
	}
	// the rows the kernel reads: matrices by byte offset (SX::M), every array the op touches by the byte offset of its plane of
	// category 0 (the kernel adds c * plane once per wave), the next op's mask words by the byte offset of their first row
	t.P = g.P;
	t.mstride = g.mstride;
	const int64_t plane_bytes = (int64_t)g.P * 4 * 8, array_bytes = plane_bytes * g.C, row_bytes = (int64_t)t.mstride * 4;
	t.desc.assign(n, StreamDesc{});
	for (int i = 0; i < n; i++) {
		const StreamOp &s = t.ops[i];
		StreamDesc &d = t.desc[i];
		auto moff = [&](int32_t node) { return node >= 0 ? node * g.C * 128 : 0; };
		const int kinds[2] = {s.flags & 7, (s.flags >> 3) & 7};
		d.flags = s.flags;
		d.parent = moff(s.parent);
		d.lnode = moff(s.lnode);
		d.rnode = moff(s.rnode);
		for (int side = 0; side < 2; side++) {
			const int32_t *a = side ? s.ra : s.la;
			int32_t *m = side ? d.rm : d.lm;
			for (int j = 0; j < 5; j++) m[j] = 0;
			if (kinds[side] == CH_DEEP) {
				m[0] = moff(a[0]);
				m[1] = moff(a[4]);
				m[2] = moff(a[5]);
				m[3] = moff(a[9]);
			} else if (kinds[side] == CH_CHERRY_TIP)
				m[4] = moff(a[3]);
		}
		d.nx_words = s.nx_mask_word >= 0 ? (int64_t)s.nx_mask_word * row_bytes : 0;
		d.nx_a = s.nx_a >= 0 ? (int64_t)s.nx_a * array_bytes : 0;
		d.nx_b = s.nx_b >= 0 ? (int64_t)s.nx_b * array_bytes : 0;
		d.nx_u = s.nx_u >= 0 ? (int64_t)s.nx_u * array_bytes : 0;
		d.st_left = s.slot_left >= 0 ? (int64_t)s.slot_left * array_bytes : 0;
		d.st_right = s.slot_right >= 0 ? (int64_t)s.slot_right * array_bytes : 0;
		d.wsh = s.wsh;
		d.flags |= (s.nx_a >= 0 ? 1 << 26 : 0) | (s.nx_b >= 0 ? 1 << 27 : 0) | (s.nx_u >= 0 ? 1 << 28 : 0) | (s.slot_left >= 0 ? 1 << 29 : 0) | (s.slot_right >= 0 ? 1 << 30 : 0);
	}
}

// Descriptors of k_lower4_stream (phyamd_walk4s.inc): the chunked post-order list, every op taking its children (in the order
// of the pre-order op of the same node: that is the order of its table block and of its mask groups' nibbles) and its table block
// from the pre-order stream tables; its mask groups are packed again in post-order (rows appended to the pre-order walk's);
// addresses multiplied out as in StreamDesc.  After stream_pre_order.
inline void stream_post_order(const Schedule &sc, const StreamGeometry &g, StreamTables &t) {
	const int n = (int)sc.walk_lower_chunk_ops.size(), ns = (int)t.ops.size();
	t.lower_desc.clear();
	t.lower_chunks.clear();
	if (n == 0 || ns == 0) return;
	std::vector<int> sop((int)sc.parent.size(), -1);
	for (int i = 0; i < ns; i++) sop[sc.walk_chunk_ops[i].parent] = i;  // (stream_ops follow walk_chunk_ops one to one)
	for (const NodeOp &o : sc.walk_lower_chunk_ops)
		if (sop[o.parent] < 0) return;  // every stored node has a pre-order op; without one the streamed post-order walk is not used
	const int64_t plane_bytes = (int64_t)g.P * 4 * 8, array_bytes = plane_bytes * g.C, row_bytes = (int64_t)t.mstride * 4;
	auto moff = [&](int32_t node) { return node >= 0 ? node * g.C * 128 : 0; };
	t.lower_desc.assign(n, LowerDesc{});
	std::vector<int> pieces(n, 0), first_word(n, 0), last_word(n, 0), words(n, 0);
	MaskPacker packer(t.row_entries);
	for (int i = 0; i < n; i++) {
		const NodeOp &o = sc.walk_lower_chunk_ops[i];
		const StreamOp &u = t.ops[sop[o.parent]];
		LowerDesc &d = t.lower_desc[i];
		const int kinds[2] = {u.flags & 7, (u.flags >> 3) & 7};
		for (int side = 0; side < 2; side++)
			if (kinds[side] != CH_CORE) {
				int row, shift;
				packer.add(&t.op_tips[(size_t)sop[o.parent] * 12 + 6 * side], row, shift);
				if (words[i] == 0) first_word[i] = row;
				last_word[i] = row;
				d.wsh |= shift << (5 * words[i]) | (row & 3) << (10 + 2 * words[i]);  // shift 0-4 / 5-9, ring slot 10-11 / 12-13
				words[i]++;
			}
		int fl = (u.flags & 0x3F) | (u.flags & 0x00FF0000);  // kinds and half kinds
		d.lnode = moff(u.lnode);
		d.rnode = moff(u.rnode);
		d.self = sc.parent[o.parent] < 0 ? 0 : moff(o.parent);  // (the root)
		d.store = (int64_t)o.core_parent * array_bytes;
		d.ls_store = (int64_t)o.core_parent * g.P * 8;
		for (int side = 0; side < 2; side++) {
			const int32_t *a = side ? u.ra : u.la;
			int32_t *m = side ? d.rm : d.lm;
			for (int j = 0; j < 5; j++) m[j] = 0;
			if (kinds[side] == CH_DEEP) {
				m[0] = moff(a[0]);
				m[1] = moff(a[4]);
				m[2] = moff(a[5]);
				m[3] = moff(a[9]);
			} else if (kinds[side] == CH_CHERRY_TIP)
				m[4] = moff(a[3]);
			if (kinds[side] != CH_CORE) continue;
			// where a stored child comes from: the previous op's registers, one of the two parked partials, or memory
			const int ch = side ? u.rnode : u.lnode;
			const bool is_left = ch == o.left;  // of the post-order op (the pre-order op may have swapped its children)
			int src = 0;
			if (o.carry_in == (is_left ? 1 : 2)) src = 1;
			else if (o.lds_park & (is_left ? 1 : 2)) src = 2;
			else if (o.lds_park & (is_left ? 0x10 : 0x20)) src = 3;
			if (src == 0 || src == 3) {  // (3: for the instantiations that have one slot, lstream_park_slots; the others fetch nothing)
				(side ? d.mem_r : d.mem_l) = (int64_t)sc.core_index[ch] * array_bytes;
				(side ? d.ls_r : d.ls_l) = (int64_t)sc.core_index[ch] * g.P * 8;
			}
			fl |= src << (6 + 2 * side);
		}
		if (o.lds_park & 4) fl |= 1 << 10;
		if (o.lds_park & 0x40) fl |= 1 << 26;
		pieces[i] = (kinds[0] != CH_CORE ? 1 : 0) | (kinds[1] != CH_CORE ? 2 : 0);
		d.flags = fl;
	}
	const int chunks = (int)sc.walk_lower_chunk_off.size() - 1;
	for (int k = 0; k < chunks; k++) {
		const int b = sc.walk_lower_chunk_off[k], en = sc.walk_lower_chunk_off[k + 1];
		// mask rows wait in a ring of four LDS slots (slot = row & 3) and are requested once: by the op in front of the first op that
		// reads them (the rows of a chunk's groups are consecutive, an op reads at most two)
		LowerChunk ch{0, 0, 0, 0, 0};
		int have = -1;  // the highest row requested so far
		auto fresh_rows = [&](int i, int &first) {  // rows op i reads that have not been requested yet
			if (words[i] == 0) return 0;
			first = have < 0 ? first_word[i] : std::max(first_word[i], have + 1);
			const int count = last_word[i] - first + 1;
			have = std::max(have, last_word[i]);
			return std::max(0, count);
		};
		if (b < en) {
			const int si = sop[sc.walk_lower_chunk_ops[b].parent];
			int first = 0;
			const int count = fresh_rows(b, first);
			ch = LowerChunk{si, pieces[b], count, first & 3, (int64_t)first * row_bytes};
		}
		t.lower_chunks.push_back(ch);
		for (int i = b; i < en; i++) {
			LowerDesc &d = t.lower_desc[i];
			const bool last = i + 1 == en;
			const int sn = last ? 0 : sop[sc.walk_lower_chunk_ops[i + 1].parent];
			d.nx_block = sn;
			int first = 0;
			const int count = last ? 0 : fresh_rows(i + 1, first);
			d.nx_words = (int64_t)first * row_bytes;
			d.flags |= count << 14;
			d.flags |= (first & 3) << 12;
			d.flags |= (last ? 0 : ((pieces[i + 1] & 2) ? 1 : 0)) << 24;
			d.flags |= (last ? 0 : (pieces[i + 1] & 1)) << 25;
		}
	}
	t.words = (int)t.row_entries.size() / 8;
}

// Stored nodes the two streamed walks can do without (the TF forms only, LowerForm::Carried / CarriedExp2): a stored node n with one
// stored child s and one child f that is a tip or a cherry.  Its parent's pre-order op needs t_n = P_n (m_f o t_s): m_f is a table
// row (a tip) or one mat-vec over two (a cherry), and t_s is stored anyway -- the op reads s's plane where it read n's, forms t_n in
// a few dozen instructions, and the post-order walk, which is bound by its writes, keeps n in registers only.
// E is chosen bottom-up over the chunked post-order list.  n is in E if
//   * n is stored and not the root, s is stored and not in E (t_s must be in memory), f is CH_TIP or CH_CHERRY;
//   * the post-order walk hands n to its parent in registers, inside one chunk: as the op in front's result (source 1) or from
//     park slot 0 (source 2) -- not from memory, and not from the second slot, which the AMBIG instantiations read from memory.
// A rewrite of the flattened tables only (Schedule, the walk lists, core_index and the storage stay as they are):
//   * LowerDesc of n: bit 11, "no store" (honoured by the TF instantiations);
//   * StreamDesc of the parent's op: the child's kind becomes SK_CORE_TIP / SK_CORE_CHERRY, lnode / rnode stay n, f's matrices go
//     to lm[0] / rm[0], f's tips to table slots 0 and 1 of the side (message rows), and the op's mask groups -- the child now has
//     one -- are packed again into rows behind the post-order walk's; the op in front (or the chunk's prologue) requests those
//     rows, both pieces of the block where the right child has tips now, and s's plane instead of n's.  n's own op reads s as before.
// The descriptors and chunks as they were are kept (plain_desc, plain_chunks) for a pass that reads the reference's form; the
// StreamOp rows (node ids, the host's bookkeeping) and the post-order walk's own kinds and mask groups stay plain as well.
// After stream_pre_order and stream_post_order.
inline void stream_elide(const Schedule &sc, const StreamGeometry &g, StreamTables &t) {
	t.plain_desc = t.desc;
	t.plain_chunks = t.chunks;
	t.elisions.clear();
	const int n = (int)t.lower_desc.size(), ns = (int)t.ops.size(), N = (int)sc.parent.size();
	if (n == 0 || ns == 0) return;
	const std::vector<NodeOp> &lops = sc.walk_lower_chunk_ops;
	std::vector<int> sop(N, -1), lop(N, -1), lchunk(n, 0);
	for (int i = 0; i < ns; i++) sop[sc.walk_chunk_ops[i].parent] = i;
	for (int i = 0; i < n; i++) lop[lops[i].parent] = i;
	for (int k = 0; k + 1 < (int)sc.walk_lower_chunk_off.size(); k++)
		for (int i = sc.walk_lower_chunk_off[k]; i < sc.walk_lower_chunk_off[k + 1]; i++) lchunk[i] = k;
	std::vector<char> in_e(N, 0);
	std::vector<int> elided_at((size_t)ns * 2, -1);  // [pre-order op][side] -> index into t.elisions
	for (int i = 0; i < n; i++) {  // children before parents: the cut subtrees' chunks, then the top part, each in post-order
		const NodeOp &o = lops[i];
		const int nd = o.parent, p = sc.parent[nd];
		if (p < 0 || lop[p] < 0 || sop[p] < 0) continue;
		const int kl = sc.node_kind[o.left], kr = sc.node_kind[o.right];
		int s, f;
		if (kl == CH_CORE && (kr == CH_TIP || kr == CH_CHERRY)) s = o.left, f = o.right;
		else if (kr == CH_CORE && (kl == CH_TIP || kl == CH_CHERRY)) s = o.right, f = o.left;
		else continue;
		if (in_e[s] || lchunk[lop[p]] != lchunk[i]) continue;
		const StreamOp &pu = t.ops[sop[p]];
		const int side = pu.lnode == nd ? 0 : 1;
		if ((side ? pu.rnode : pu.lnode) != nd || ((pu.flags >> (3 * side)) & 7) != CH_CORE) continue;
		const int source = (t.lower_desc[lop[p]].flags >> (6 + 2 * side)) & 3;
		if (source != 1 && source != 2) continue;
		in_e[nd] = 1;
		elided_at[(size_t)sop[p] * 2 + side] = (int)t.elisions.size();
		t.elisions.push_back(StreamElision{nd, p, s, f, sc.node_kind[f], source, side, lchunk[i]});
		t.lower_desc[i].flags |= 1 << 11;
	}
	if (t.elisions.empty()) return;
	const int64_t plane_bytes = (int64_t)g.P * 4 * 8, array_bytes = plane_bytes * g.C, row_bytes = (int64_t)t.mstride * 4;
	std::vector<int> chunk_of_start(ns, -1);
	for (int k = 0; k + 1 < (int)sc.walk_chunk_off.size(); k++)
		if (sc.walk_chunk_off[k] < sc.walk_chunk_off[k + 1]) chunk_of_start[sc.walk_chunk_off[k]] = k;
	MaskPacker packer(t.row_entries);
	for (int i = 0; i < ns; i++) {
		if (elided_at[(size_t)i * 2] < 0 && elided_at[(size_t)i * 2 + 1] < 0) continue;
		StreamDesc &d = t.desc[i];
		int want[2] = {-1, -1};
		for (int side = 0; side < 2; side++) {
			if (elided_at[(size_t)i * 2 + side] < 0) continue;
			const StreamElision &el = t.elisions[elided_at[(size_t)i * 2 + side]];
			const NodeOp &o = lops[lop[el.node]];
			const bool f_left = o.left == el.sibling;
			int *tips = &t.op_tips[(size_t)i * 12 + 6 * side];
			if (el.sibling_kind == CH_TIP) tips[0] = el.sibling;
			else {
				tips[0] = f_left ? o.lt0 : o.rt0;
				tips[1] = f_left ? o.lt1 : o.rt1;
			}
			d.flags = (d.flags & ~(7 << (3 * side))) | (el.sibling_kind == CH_TIP ? SK_CORE_TIP : SK_CORE_CHERRY) << (3 * side);
			(side ? d.rm : d.lm)[0] = el.sibling * g.C * 128;
			want[side] = sc.core_index[el.stored];
		}
		// the op's mask groups again, the new ones among them: the left child's first, the second in the first one's row or the next
		int words = 0, first_word = -1, same_row = 0, wsh = 0;
		for (int side = 0; side < 2; side++)
			if (((d.flags >> (3 * side)) & 7) != CH_CORE) {
				int row, shift;
				packer.add(&t.op_tips[(size_t)i * 12 + 6 * side], row, shift);
				if (words == 0) first_word = row;
				else same_row = row == first_word;
				wsh |= shift << (5 * words);
				words++;
			}
		d.wsh = wsh;
		const int two_pieces = ((d.flags >> 3) & 7) != CH_CORE;
		if (chunk_of_start[i] >= 0) {
			StreamChunk &ch = t.chunks[chunk_of_start[i]];
			ch.mask_word = first_word;
			ch.mask_words = words;
			ch.same_row = same_row;
			if (want[0] >= 0) ch.a = want[0];
			if (want[1] >= 0) ch.b = want[1];
		} else {
			StreamDesc &pv = t.desc[i - 1];
			pv.flags = (pv.flags & ~(3 << 14 | 1 << 24 | 1 << 25)) | words << 14 | two_pieces << 24 | same_row << 25;
			pv.nx_words = (int64_t)first_word * row_bytes;
			if (want[0] >= 0) pv.nx_a = (int64_t)want[0] * array_bytes;
			if (want[1] >= 0) pv.nx_b = (int64_t)want[1] * array_bytes;
		}
	}
	t.words = (int)t.row_entries.size() / 8;
}

// An elided node's stored child is read twice, one op apart: the parent's op is handed s's plane in register set A (B) and forms
// t_n = P_n (m_f o t_s) from it, and n's own op reads the same plane as its stored child.  Where n's op is the very next op the
// loop runs, and s sits there on the side n had in its parent's op, the wave still holds t_s in that register set when the
// parent's op issues its requests: the kernel keeps A / B across the loop edge when descriptor bit 26 / 27 is clear (under
// SCALE == 2 the exponent eA / eB with it, guarded by the same bits), nothing but the prefetch writes them between the elided
// child's message and the loop edge, and n's op copies the kept value as it copies a fetched one (own_registers).  So the
// parent's op does not request the plane: the bit is cleared, nx_a / nx_b is unused.  Everything else keeps its requests: an
// elided node whose op is not the next one (its upper is parked, or the other child is walked first), one whose op opens a chunk
// (the prologue fetches its operands), one whose stored child changes sides, and the plain descriptors.  A pair op never has an
// elided child and an elided node never a DEEP one, so stream_pairs, which copies `desc` afterwards, neither moves nor absorbs
// an op this rule looks at.  A rewrite of `desc` only; one StreamKeep per elided node.  After stream_elide.
inline void stream_keep(const Schedule &sc, const StreamGeometry &g, StreamTables &t) {
	t.keeps.clear();
	const int ns = (int)t.ops.size();
	std::vector<int> sop((size_t)sc.parent.size(), -1), chunk_of(ns, 0);
	std::vector<char> opens(ns, 0);
	for (int i = 0; i < ns; i++) sop[t.ops[i].parent] = i;
	for (int k = 0; k + 1 < (int)sc.walk_chunk_off.size(); k++)
		for (int i = sc.walk_chunk_off[k]; i < sc.walk_chunk_off[k + 1]; i++) {
			chunk_of[i] = k;
			opens[i] = i == sc.walk_chunk_off[k];
		}
	for (const StreamElision &el : t.elisions) {
		StreamKeep kp{el.node, el.parent, el.side, KEEP_KEPT};
		const int i = sop[el.parent], j = sop[el.node];
		if (!g.keep) kp.reason = KEEP_OFF;
		else if (j >= 0 && opens[j]) kp.reason = KEEP_OPENER;
		else if (i < 0 || j != i + 1 || chunk_of[j] != chunk_of[i]) kp.reason = KEEP_NOT_NEXT;
		else if ((el.side ? t.ops[j].rnode : t.ops[j].lnode) != el.stored || ((t.desc[j].flags >> (3 * el.side)) & 7) != CH_CORE) kp.reason = KEEP_OTHER_SIDE;
		else {
			StreamDesc &d = t.desc[i];
			d.flags &= ~(1 << (26 + el.side));
			(el.side ? d.nx_b : d.nx_a) = 0;
		}
		t.keeps.push_back(kp);
	}
}

// Pair ops: a third set of pre-order descriptors, read by the plain TF pass alone (k_upper4_stream<.., 0, false, true>).  A DEEP
// node d has no stored partial: its parent's op n rebuilds its message from its two half messages, and d's own op, when it is the
// next one, forms the same two halves again as its children's messages and pays an op's fixed cost.  In this set n runs d's op
// inside its own (descriptor bit 8) and the walk steps over d's descriptor, which stays where it is, unread.  n and d are fused when
//   * d is n's LEFT child (the one walked first: its upper arrives in registers) and d's op is the next of the same chunk;
//   * n's other child s is CH_CORE or CH_TIP in the descriptor -- not a fringe child, a second DEEP child or an elided kind;
//   * s is stored, or d has four tips: the block's other side holds s's tip rows (320 bytes) and the Qs P rows of d's tips (160 each).
// n's descriptor already names d's matrices, half kinds and mask group.  What changes:
//   * n requests what the op behind d wants (d's request fields), and the op in front of n both pieces of n's block;
//   * the block of n gains the Qs P rows and a position table of the pair's twelve terms (pair_tab; op_deep bit 2; phyamd_types.h),
//     in places no other reader of the block looks at -- the table blocks are shared with the other descriptor sets;
//   * s stored and its op directly behind d's: that op takes s's upper as the carry (it IS the left child's upper of the op in
//     front, as the kernel keeps it), and n neither parks nor stores it.
// `desc`, `ops`, the chunks, the site table and the slab positions stay as they are.  After stream_elide.
inline void stream_pairs(const Schedule &sc, const StreamGeometry &g, StreamTables &t) {
	const int ns = (int)t.ops.size();
	t.pair_desc = t.desc;
	t.pair_tab.assign((size_t)ns * 16, -1);
	t.pairs.assign(ns, StreamPair{-1, PAIR_NO_DEEP, -1, -1, -1, 0, 0});
	if (ns == 0) return;
	std::vector<int> chunk_of(ns, 0);
	for (int k = 0; k + 1 < (int)sc.walk_chunk_off.size(); k++)
		for (int i = sc.walk_chunk_off[k]; i < sc.walk_chunk_off[k + 1]; i++) chunk_of[i] = k;
	auto tips_of = [&](int i, int side) {
		int n = 0;
		for (int j = 0; j < 6; j++) n += t.op_tips[(size_t)i * 12 + 6 * side + j] >= 0;
		return n;
	};
	for (int i = 0; i < ns; i++) {
		StreamPair &pr = t.pairs[i];
		const StreamOp &s = t.ops[i];
		const int fl = t.desc[i].flags, kl = fl & 7, kr = (fl >> 3) & 7;
		pr.node = s.parent;
		if (i > 0 && t.pairs[i - 1].reason == PAIR_FUSED) {
			pr.reason = PAIR_ABSORBED;
			continue;
		}
		if (kl != CH_DEEP && kr != CH_DEEP) continue;
		const bool next_here = i + 1 < ns && chunk_of[i + 1] == chunk_of[i];
		const int side = kl == CH_DEEP && (kr != CH_DEEP || !next_here || t.ops[i + 1].parent != s.rnode) ? 0 : 1;
		pr.child = side ? s.rnode : s.lnode;
		pr.sibling = side ? s.lnode : s.rnode;
		pr.sibling_kind = side ? kl : kr;
		pr.child_tips = tips_of(i, side);
		if (side != 0 || !next_here || t.ops[i + 1].parent != pr.child || ((t.desc[i + 1].flags >> 9) & 7) != SU_CARRY) pr.reason = PAIR_NOT_NEXT;
		else if (pr.sibling_kind != CH_CORE && pr.sibling_kind != CH_TIP) pr.reason = PAIR_SIBLING;
		else if (pr.sibling_kind == CH_TIP && pr.child_tips > 4) pr.reason = PAIR_BLOCK;
		else pr.reason = PAIR_FUSED;
	}
	const int next_mask = 3 << 14 | 1 << 24 | 1 << 25 | 1 << 26 | 1 << 27 | 1 << 28;
	for (int i = 0; i < ns; i++) {
		if (t.pairs[i].reason != PAIR_FUSED) continue;
		StreamPair &pr = t.pairs[i];
		StreamDesc &pd = t.pair_desc[i];
		const StreamDesc &dd = t.desc[i + 1];
		const StreamOp &s = t.ops[i];
		pd.flags = (pd.flags & ~next_mask) | (dd.flags & next_mask) | 1 << 8;
		pd.nx_words = dd.nx_words;
		pd.nx_a = dd.nx_a;
		pd.nx_b = dd.nx_b;
		pd.nx_u = dd.nx_u;
		t.op_deep[i] |= 4;
		// the twelve terms by result lane: this op's two where they were, d's by the places of its own op's rows
		std::vector<int> pos_of((size_t)sc.parent.size(), -1);
		for (int j = 0; j < 10; j++) {
			const int at = t.site_tab[(size_t)(i + 1) * 16 + j];
			if (at >= 0) pos_of[t.qnode[at / 8]] = at;
		}
		int *tab = &t.pair_tab[(size_t)i * 16];
		tab[0] = t.site_tab[(size_t)i * 16];
		tab[4] = t.site_tab[(size_t)i * 16 + 4];
		for (int h = 0; h < 2; h++) {
			const int32_t *q = s.la + 5 * h;  // {node, t0, t1, t2, inner}
			const int hk = (pd.flags >> (16 + 2 * h)) & 3;
			tab[10 + h] = pos_of[q[0]];
			if (hk == HK_TIP) continue;
			tab[4 * h + 1] = pos_of[q[1]];
			tab[4 * h + 2] = pos_of[q[2]];
			if (hk == HK_CHERRY_TIP) {
				tab[4 * h + 3] = pos_of[q[4]];
				tab[8 + h] = pos_of[q[3]];
			}
		}
		// s's upper in registers to s's own op
		const int j = i + 2;
		if (pr.sibling_kind == CH_CORE && j < ns && chunk_of[j] == chunk_of[i] && t.ops[j].parent == pr.sibling) {
			StreamDesc &sd = t.pair_desc[j];
			const int usrc = (sd.flags >> 9) & 7;
			if (usrc == SU_LDS || usrc == SU_U) {
				pr.carry = 1;
				sd.flags = (sd.flags & ~(7 << 9 | 1 << 7)) | SU_CARRY << 9;
				pd.flags &= ~(3 << 12 | 1 << 6 | 1 << 28 | 1 << 30);
				pd.nx_u = 0;
				pd.st_right = 0;
			}
		}
	}
	// the op in front of a pair requests both pieces of its block (a chunk's first block is requested whole)
	for (int i = 0, front = -1; i < ns; i++) {
		if (t.pairs[i].reason == PAIR_ABSORBED) continue;
		if (t.pairs[i].reason == PAIR_FUSED && front >= 0 && chunk_of[front] == chunk_of[i]) t.pair_desc[front].flags |= 1 << 24;
		front = i;
	}
}

// both walks' tables (the post-order walk's mask rows follow the pre-order walk's; g.elide: stream_elide's rewrite of both)
inline void build_stream_tables(const Schedule &sc, const StreamGeometry &g, StreamTables *out) {
	stream_pre_order(sc, g, *out);
	stream_post_order(sc, g, *out);
	out->plain_desc.clear();
	out->plain_chunks.clear();
	out->elisions.clear();
	out->keeps.clear();
	out->pair_desc.clear();
	out->pair_tab.clear();
	out->pairs.clear();
	if (g.elide) stream_elide(sc, g, *out);
	if (g.elide) stream_keep(sc, g, *out);
	if (g.pairs) stream_pairs(sc, g, *out);
}

// ---- the batched walks' op lists ----------------------------------------------------------------------------------------------

// the two op lists of the batched walk for a tree (T tips; left / right / root in phyamd_set_topology's convention, already
// validated), appended to `ops` as [post-order T - 1 | pre-order T - 1]; returns the upper slots the pre-order list parks in.
// ops == null: only counts the slots.  Post-order: depth first, the larger subtree first, so that the child finished last hands
// its partial on in registers.  Pre-order: of two internal children the smaller subtree is entered first with its upper in
// registers and the other's upper is parked in a slot that is free again once its op has read it: at most log2(T) + 1 slots,
// whatever the shape (a caterpillar parks nothing).  Ties go by left / right, never by node id: the lists of one tree under two
// labellings of its internal nodes differ in the ids only.
// park_all (phyamd_nni_log_likelihoods): every internal child's upper is parked in a slot of its own, slot = node - T, and none
// is handed on in registers: T - 1 slots, and after the walk every internal non-root node's upper is in the scratch.
inline int build_batch_ops(int T, const int32_t *left, const int32_t *right, int root, std::vector<BatchOp> *ops, bool park_all = false) {
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

// The post-order list of build_batch_ops for a tree (already validated) with the slot words k_sitelnl_walk4 reads
// (phyamd_sitelnl.inc), appended to `ops` (null: only counted); returns the slots the list parks in.  A result whose parent is the
// next op is handed on in registers; any other waits in a slot, which is free again once the parent has read it -- before the
// parent's own result looks for one.  The list takes the larger subtree first, so the result that waits while a sibling subtree is
// walked belongs to a subtree at least as large: at most floor(log2 T) - 1 wait at once, and a caterpillar parks none.
// work: the builder's list, reused from call to call
inline int site_lnl_ops(int T, const int32_t *left, const int32_t *right, int root, std::vector<BatchOp> &work, std::vector<BatchOp> *ops) {
	work.clear();
	build_batch_ops(T, left, right, root, &work);
	const int nops = T - 1;
	std::vector<int> slot_of(2 * T - 1, BATCH_NONE), free_slots;
	int slots = 0;
	for (int i = 0; i < nops; i++) {
		BatchOp op = work[i];
		const auto source = [&](int child, int side) {
			if (child < T) return (int)BATCH_NONE;
			if (op.carry == side) return (int)BATCH_CARRY;
			const int s = slot_of[child];
			free_slots.push_back(s);
			return s;
		};
		op.src = source(op.left, 1);
		op.dst_left = source(op.right, 2);
		if (i + 1 == nops) op.dst_right = BATCH_NONE;  // the root's
		else if (work[i + 1].carry != 0) op.dst_right = BATCH_CARRY;
		else {
			if (free_slots.empty()) slot_of[op.node] = slots++;
			else {
				slot_of[op.node] = free_slots.back();
				free_slots.pop_back();
			}
			op.dst_right = slot_of[op.node];
		}
		if (ops) ops->push_back(op);
	}
	return slots;
}

// ---- the branch-length sweep (phyamd_optimize_branch_lengths, phyamd_blopt4.inc) -------------------------------------------------

// One pass over a tree (already validated) as a depth-first tour, appended to `ops` in launch order.  O_n is what meets the
// branch of a non-root node n from above -- A_m o msg(sibling), A_m = P_m O_m of the parent m, ones when m is the root -- and has
// a plane of its own per node; p_n is internal node n's lower partial, in the plane the batched walk stores it in.
//   SWEEP_UPPER: O_node from the parent a (BATCH_ROOT: the root) and the sibling b;
//   SWEEP_LOWER: p_node from its children a and b;
//   SWEEP_VISIT: the branch of `node` is optimised from O_node and p_node.
// The tour enters an internal node n, forms O_left, tours the left subtree, forms O_right from the left child's new message, tours
// the right subtree, forms p_n and visits n: the visits are the post-order (left subtree, right subtree, node) of the nodes other
// than the root, and nothing outside a subtree changes while the tour is inside it, so O_n is still current when n is visited.
// visit: the index of the visit the op belongs to -- the next one in the tour (a visit's own).  The root's p is never formed:
// nothing reads it.  2 (T - 1) uppers, T - 2 lowers and 2 (T - 1) visits
enum { SWEEP_UPPER = 0, SWEEP_LOWER = 1, SWEEP_VISIT = 2 };
struct SweepOp {
	int32_t visit, kind, node, a, b;
};
inline void build_branch_sweep(int T, const int32_t *left, const int32_t *right, int root, std::vector<SweepOp> *ops) {
	std::vector<std::pair<int, int>> stack{{root, 0}};  // (node, children toured)
	int32_t visit = 0;
	while (!stack.empty()) {
		const int n = stack.back().first, stage = stack.back().second;
		if (n >= T && stage < 2) {
			const int child = stage == 0 ? left[n] : right[n], sibling = stage == 0 ? right[n] : left[n];
			ops->push_back(SweepOp{visit, SWEEP_UPPER, child, n == root ? (int32_t)BATCH_ROOT : n, sibling});
			stack.back().second = stage + 1;
			stack.push_back({child, 0});
			continue;
		}
		stack.pop_back();
		if (n == root) continue;
		if (n >= T) ops->push_back(SweepOp{visit, SWEEP_LOWER, n, left[n], right[n]});
		ops->push_back(SweepOp{visit, SWEEP_VISIT, n, n, n >= T ? n : (int32_t)BATCH_NONE});
		visit++;
	}
}

#endif
