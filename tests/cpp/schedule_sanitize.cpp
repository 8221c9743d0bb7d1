// Sanitizer driver for the host-built tree schedules (physher_amd/csrc/phyamd_tree_schedule.h over phyamd_types.h): no GPU, no engine.
// Built and run by tests/test_schedule_sanitizers.py with -fsanitize=address,undefined; exits non-zero on any finding
// (ASan/UBSan abort) or on a failed structure check.  The trees are generated here: caterpillar, balanced and seeded random ones
// from 2 to 130 tips (both sides of the 32-op chunking threshold), one random 1000-tip tree, and the tree check's failing cases.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "phyamd_tree_schedule.h"

static int fails = 0;
#define CHECK(c)                                                  \
	do {                                                          \
		if (!(c)) {                                               \
			std::fprintf(stderr, "CHECK failed: %s (line %d, %s)\n", #c, __LINE__, context.c_str()); \
			fails++;                                              \
		}                                                         \
	} while (0)

static std::string context;

struct Tree {
	int T, root;
	std::vector<int32_t> left, right;
	TreeRef ref() const { return TreeRef{T, left.data(), right.data(), root}; }
};

// shape 0: caterpillar, 1: balanced (joins in a queue), 2: random joins (a linear congruential generator seeded by `seed`)
static Tree make_tree(int T, int shape, unsigned seed) {
	Tree t{T, 2 * T - 2, std::vector<int32_t>(2 * T - 1, -1), std::vector<int32_t>(2 * T - 1, -1)};
	std::vector<int> active;
	for (int i = 0; i < T; i++) active.push_back(i);
	unsigned state = seed * 2654435761u + 12345u;
	auto draw = [&](int n) {
		state = state * 1664525u + 1013904223u;
		return (int)((state >> 8) % (unsigned)n);
	};
	for (int next = T; active.size() > 1; next++) {
		int i = 0, j = 1;
		if (shape == 2) {
			i = draw((int)active.size());
			j = draw((int)active.size() - 1);
			if (j >= i) j++;
		}
		t.left[next] = active[i];
		t.right[next] = active[j];
		active.erase(active.begin() + std::max(i, j));
		active.erase(active.begin() + std::min(i, j));
		if (shape == 0) active.insert(active.begin(), next);
		else active.push_back(next);
	}
	return t;
}

struct NamedOptions {
	const char *name;
	ScheduleOptions o;
};

static std::vector<NamedOptions> option_sets() {
	std::vector<NamedOptions> v;
	auto add = [&](const char *name, int S, void (*change)(ScheduleOptions &)) {
		ScheduleOptions o;
		o.S = S;
		if (change) change(o);
		v.push_back({name, o});
	};
	add("4 states", 4, nullptr);
	add("4 states, keep_partials", 4, [](ScheduleOptions &o) { o.keep_partials = true; });
	add("4 states, scaling_on", 4, [](ScheduleOptions &o) { o.scaling_on = true; });
	add("4 states, fusion off", 4, [](ScheduleOptions &o) { o.fusion_enabled = false; });
	add("4 states, walk off", 4, [](ScheduleOptions &o) { o.walk_enabled = false; });
	add("4 states, lower_park2 off", 4, [](ScheduleOptions &o) { o.lower_park2_on = false; });
	add("20 states", 20, nullptr);
	add("20 states, scaling_on", 20, [](ScheduleOptions &o) { o.scaling_on = true; });
	add("20 states, generic_fusion off", 20, [](ScheduleOptions &o) { o.generic_fusion = false; });
	add("20 states, keep_partials", 20, [](ScheduleOptions &o) { o.keep_partials = true; });
	add("61 states", 61, nullptr);
	return v;
}

static void check_offsets(const std::vector<int> &off, size_t size) {
	CHECK(!off.empty() && off.front() == 0 && off.back() == (int)size);
	for (size_t i = 0; i + 1 < off.size(); i++) CHECK(off[i] <= off[i + 1]);
}

// cores below core_count, upper slots below `slots`
static void check_ops(const std::vector<NodeOp> &ops, const Schedule &s, int slots) {
	const int N = (int)s.parent.size();
	for (const NodeOp &op : ops) {
		CHECK(op.parent >= 0 && op.parent < N && op.left >= 0 && op.left < N && op.right >= 0 && op.right < N);
		for (int core : {op.core_parent, op.core_left, op.core_right}) CHECK(core >= -1 && core < s.core_count);
		for (int slot : {op.upper_slot_parent, op.upper_slot_left, op.upper_slot_right}) CHECK(slot >= -1 && slot < slots);
		CHECK(op.core_parent == s.core_index[op.parent] && op.core_left == s.core_index[op.left] && op.core_right == s.core_index[op.right]);
	}
}

static void check_schedule(const Tree &t, const Schedule &s) {
	const int T = t.T, N = 2 * T - 1;
	CHECK((int)s.parent.size() == N && (int)s.node_kind.size() == N && (int)s.core_index.size() == N && (int)s.deep_host.size() == N && (int)s.upper_slot.size() == N);
	CHECK(s.parent[t.root] == -1);
	int stored = 0, with_upper_op = 0, deep = 0;
	std::vector<char> seen(s.core_count > 0 ? s.core_count : 1, 0);
	for (int n = 0; n < N; n++) {
		const int k = s.node_kind[n];
		CHECK((n < T) == (k == CH_TIP));
		CHECK((k == CH_CORE) == (s.core_index[n] >= 0));
		if (k == CH_CORE) {
			stored++;
			CHECK(s.core_index[n] < s.core_count);
			if (s.core_index[n] < s.core_count) {  // dense: every index once
				CHECK(!seen[s.core_index[n]]);
				seen[s.core_index[n]] = 1;
			}
		}
		if (k == CH_CORE || k == CH_DEEP) with_upper_op++;
		if (k == CH_DEEP) deep++;
		CHECK(s.upper_slot[n] >= -1 && s.upper_slot[n] < s.upper_slots);
	}
	CHECK(stored == s.core_count && deep == s.deep_count);
	// one op per stored node (post-order) and per node with a pre-order op of its own (stored or DEEP)
	CHECK((int)s.lower_ops.size() == stored && (int)s.upper_ops.size() == with_upper_op);
	check_offsets(s.lower_level_off, s.lower_ops.size());
	check_offsets(s.upper_level_off, s.upper_ops.size());
	check_ops(s.lower_ops, s, 0);
	check_ops(s.upper_ops, s, s.upper_slots);
	if (s.walking || s.gen_walking) {
		CHECK((int)s.walk_lower_ops.size() == stored && (int)s.walk_upper_ops.size() == with_upper_op);
		check_ops(s.walk_lower_ops, s, 0);
		check_ops(s.walk_upper_ops, s, s.walk_upper_slots);
	} else
		CHECK(s.walk_lower_ops.empty() && s.walk_upper_ops.empty() && s.walk_upper_slots == 0);
	if (s.walking) {
		CHECK((int)s.walk_lower_chunk_ops.size() == stored && (int)s.walk_chunk_ops.size() == with_upper_op);
		check_offsets(s.walk_chunk_off, s.walk_chunk_ops.size());
		check_offsets(s.walk_lower_chunk_off, s.walk_lower_chunk_ops.size());
		check_ops(s.walk_chunk_ops, s, s.walk_chunk_slots);
		check_ops(s.walk_lower_chunk_ops, s, 0);
		CHECK(s.walk_chunk_slots <= s.walk_upper_slots);
	}
}

static void check_stream_tables(const Tree &t, const Schedule &s, const StreamGeometry &g, const StreamTables &tb) {
	const int T = t.T, N = 2 * T - 1, n = (int)s.walk_chunk_ops.size();
	CHECK((int)tb.ops.size() == n && (int)tb.desc.size() == n && (int)tb.op_deep.size() == n);
	CHECK(tb.site_tab.size() == (size_t)n * 16 && tb.op_tips.size() == (size_t)n * 12);
	CHECK(tb.chunks.size() + 1 == s.walk_chunk_off.size());
	CHECK(tb.P == g.P && tb.mstride == g.mstride && tb.R == (int)tb.qnode.size());
	CHECK(tb.row_entries.size() == (size_t)tb.words * 8);
	for (const StreamOp &o : tb.ops)
		for (int slot : {o.slot_parent, o.slot_left, o.slot_right, o.nx_u}) CHECK(slot >= -1 && slot < s.walk_chunk_slots);
	for (int at : tb.site_tab) CHECK(at == -1 || (at >= 0 && at % 8 == 0 && at / 8 < tb.R));
	for (int node : tb.qnode) CHECK(node >= 0 && node < N);
	for (int tip : tb.op_tips) CHECK(tip >= -1 && tip < T);
	for (int ent : tb.row_entries) CHECK(ent == -1 || (ent & 0xFFFFF) < T);
	for (const StreamChunk &c : tb.chunks) CHECK(c.mask_word >= -1 && c.mask_word < tb.words);
	CHECK(tb.lower_desc.empty() || tb.lower_desc.size() == s.walk_lower_chunk_ops.size());
	if (!tb.lower_desc.empty()) CHECK(tb.lower_chunks.size() + 1 == s.walk_lower_chunk_off.size());
	for (const LowerDesc &d : tb.lower_desc) CHECK(d.nx_block >= 0 && d.nx_block < n);
	for (const LowerChunk &c : tb.lower_chunks) CHECK(c.block >= 0 && c.block < std::max(1, n));
}

static void check_batch_lists(const Tree &t) {
	const int T = t.T, N = 2 * T - 1;
	for (bool park_all : {false, true}) {
		std::vector<BatchOp> ops;
		const int slots = build_batch_ops(T, t.left.data(), t.right.data(), t.root, &ops, park_all);
		CHECK(slots == build_batch_ops(T, t.left.data(), t.right.data(), t.root, nullptr, park_all));
		CHECK((int)ops.size() == 2 * (T - 1) && slots >= 1 && slots <= std::max(1, T - 1));
		if (park_all) CHECK(slots == std::max(1, T - 1));
		for (size_t i = 0; i < ops.size(); i++) {
			const BatchOp &o = ops[i];
			CHECK(o.node >= T && o.node < N && o.left >= 0 && o.left < N && o.right >= 0 && o.right < N);
			if (i >= (size_t)(T - 1))  // pre-order: where the node's upper is, where the children's go
				for (int where : {o.src, o.dst_left, o.dst_right}) CHECK(where >= BATCH_ROOT && where < slots);
		}
	}
	std::vector<BatchOp> work, ops;
	const int slots = site_lnl_ops(T, t.left.data(), t.right.data(), t.root, work, &ops);
	CHECK(slots == site_lnl_ops(T, t.left.data(), t.right.data(), t.root, work, nullptr));
	CHECK((int)ops.size() == T - 1 && slots >= 0 && slots < std::max(1, T - 1));
	for (const BatchOp &o : ops)
		for (int where : {o.src, o.dst_left, o.dst_right}) CHECK(where >= BATCH_CARRY && where < slots);
}

static void check_tree(const Tree &t, const std::vector<NamedOptions> &sets, const std::string &name) {
	for (const NamedOptions &set : sets) {
		context = name + ", " + set.name;
		Schedule s;
		const std::string err = build_schedule(t.ref(), set.o, &s);
		CHECK(err.empty());
		if (!err.empty()) continue;
		check_schedule(t, s);
		if (!s.walking) continue;
		StreamTables tb;  // (built again and again into one value, as an engine does)
		for (int P : {64, 65, 1000})
			for (int C : {1, 4}) {
				const StreamGeometry g{P, C, (size_t)((P + WAVE - 1) / WAVE) * WAVE};
				build_stream_tables(s, g, &tb);
				check_stream_tables(t, s, g, tb);
			}
	}
	context = name;
	check_batch_lists(t);
}

// a refused tree: the error names what is wrong, with and without a call's name and item index, and the schedule is left alone
static void check_refused(Tree t, const char *what, const Schedule &before) {
	context = what;
	Schedule s = before;
	const std::string err = build_schedule(t.ref(), ScheduleOptions{}, &s);
	CHECK(err.find(what) != std::string::npos);
	CHECK(s.parent == before.parent && s.node_kind == before.node_kind && s.core_index == before.core_index && s.core_count == before.core_count);
	CHECK(s.lower_ops.size() == before.lower_ops.size() && s.walk_chunk_ops.size() == before.walk_chunk_ops.size() && s.walk_chunk_off == before.walk_chunk_off);
	CHECK(s.upper_slot == before.upper_slot && s.lower_level_off == before.lower_level_off && s.walking == before.walking);
	std::vector<int32_t> parent;
	const std::string in_batch = validate_tree(t.ref(), parent, "phyamd_gradient_batch_trees", 3);
	CHECK(in_batch.find("phyamd_gradient_batch_trees: item 3: ") == 0 && in_batch.find(what) != std::string::npos);
}

int main() {
	const std::vector<NamedOptions> sets = option_sets();
	static const char *const shapes[3] = {"caterpillar", "balanced", "random"};
	for (int T = 2; T <= 130; T++)
		for (int shape = 0; shape < 3; shape++) check_tree(make_tree(T, shape, (unsigned)T), sets, std::string(shapes[shape]) + " " + std::to_string(T));
	check_tree(make_tree(1000, 2, 7), sets, "random 1000");

	const Tree good = make_tree(9, 2, 1);
	Schedule before;
	context = "the tree the refused ones are derived from";
	CHECK(build_schedule(good.ref(), ScheduleOptions{}, &before).empty());
	{
		Tree t = good;  // a tip with children
		t.left[0] = 1, t.right[0] = 2;
		check_refused(t, "is a tip", before);
	}
	{
		Tree t = good;  // l == r
		t.right[t.root] = t.left[t.root];
		check_refused(t, "invalid children", before);
	}
	{
		Tree t = good;  // a child out of range
		t.left[t.root] = 2 * t.T - 1;
		check_refused(t, "invalid children", before);
	}
	{
		Tree t = good;  // two parents: the root takes a child of another node
		const int other = t.T;  // the first internal node
		t.left[t.root] = t.left[other];
		check_refused(t, "two parents", before);
	}
	{
		Tree t = good;  // a tip as root
		t.root = 0;
		check_refused(t, "not a parentless internal node", before);
	}
	{
		Tree t = good;  // an internal node that has a parent as root
		t.root = t.T;
		check_refused(t, "not a parentless internal node", before);
	}
	{
		// unreachable nodes: node 3 is its own parent, the root reaches 0, 1 and itself only
		Tree t{3, 4, {-1, -1, -1, 2, 0}, {-1, -1, -1, 3, 1}};
		check_refused(t, "not a single binary tree", before);
	}
	if (fails) return 1;
	std::puts("schedule_sanitize: ok");
	return 0;
}
