// Sanitizer driver for stream_keep (physher_amd/csrc/phyamd_tree_schedule.h): the rewrite of the streamed pre-order walk's
// descriptors that stops an op from requesting, for the next op, a plane it holds in registers itself.  No GPU, no engine.  Built
// and run by tests/test_stream_keep_sanitizers.py with -fsanitize=address,undefined; exits non-zero on any finding (ASan/UBSan
// abort) or on a failed check.  The check is a replay of the kernel's loop over both descriptor sets that know elided kinds (the
// one with pair ops steps over an absorbed op as the kernel does): which plane register sets A and B hold at the top of every op,
// with the switch on and off -- wherever an op reads a set (a stored child, or an elided one's stored child), both replays hold the
// same plane in it.  The trees are generated here: caterpillars, balanced, seeded random ones and caterpillars of tips and
// cherries from 2 to 130 tips, and random trees of 500 and 1000 tips, each with both park-slot schedules.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "phyamd_tree_schedule.h"

static int fails = 0;
static std::string context;
#define CHECK(c)                                                  \
	do {                                                          \
		if (!(c)) {                                               \
			std::fprintf(stderr, "CHECK failed: %s (line %d, %s)\n", #c, __LINE__, context.c_str()); \
			fails++;                                              \
		}                                                         \
	} while (0)

struct Tree {
	int T, root;
	std::vector<int32_t> left, right;
	TreeRef ref() const { return TreeRef{T, left.data(), right.data(), root}; }
};

// shape 0: caterpillar, 1: balanced (joins in a queue), 2: random joins (a linear congruential generator seeded by `seed`),
// 3: a caterpillar whose rungs alternate between tips and cherries (every rung a node stream_elide looks at)
static Tree make_tree(int T, int shape, unsigned seed) {
	Tree t{T, 2 * T - 2, std::vector<int32_t>(2 * T - 1, -1), std::vector<int32_t>(2 * T - 1, -1)};
	unsigned state = seed * 2654435761u + 12345u;
	auto draw = [&](int n) {
		state = state * 1664525u + 1013904223u;
		return (int)((state >> 8) % (unsigned)n);
	};
	int next = T;
	auto join = [&](int l, int r) {
		t.left[next] = l, t.right[next] = r;
		return next++;
	};
	if (shape == 3) {
		int used = 0, spine = -1;
		if (T >= 4) spine = join(join(0, 1), join(2, 3)), used = 4;
		else spine = 0, used = 1;
		for (int rung = 0; used < T; rung++) {
			if (rung % 2 && used + 2 <= T) spine = join(spine, join(used, used + 1)), used += 2;
			else spine = rung % 4 ? join(used, spine) : join(spine, used), used += 1;
		}
		return t;
	}
	std::vector<int> active;
	for (int i = 0; i < T; i++) active.push_back(i);
	while (active.size() > 1) {
		int i = 0, j = 1;
		if (shape == 2) {
			i = draw((int)active.size());
			j = draw((int)active.size() - 1);
			if (j >= i) j++;
		}
		const int node = join(active[i], active[j]);
		active.erase(active.begin() + std::max(i, j));
		active.erase(active.begin() + std::min(i, j));
		if (shape == 0) active.insert(active.begin(), node);
		else active.push_back(node);
	}
	return t;
}

static int total_kept = 0, total_reads = 0;

// the kernel's loop over one descriptor set: the plane (byte offset; -1: whatever the wave started with) in A / B at the top of
// every op the loop runs, -2 for an op it steps over
static void replay(const Schedule &s, const StreamTables &tb, const std::vector<StreamDesc> &desc, int64_t array_bytes, std::vector<int64_t> held[2]) {
	const int n = (int)desc.size();
	held[0].assign(n, -2);
	held[1].assign(n, -2);
	for (size_t k = 0; k + 1 < s.walk_chunk_off.size(); k++) {
		const int b = s.walk_chunk_off[k], e = s.walk_chunk_off[k + 1];
		if (b >= e) continue;
		int64_t A = tb.chunks[k].a != -1 ? (int64_t)tb.chunks[k].a * array_bytes : -1, B = tb.chunks[k].b != -1 ? (int64_t)tb.chunks[k].b * array_bytes : -1;
		for (int i = b; i < e; i++) {
			const StreamDesc &d = desc[i];
			held[0][i] = A;
			held[1][i] = B;
			if (d.flags & (1 << 26)) A = d.nx_a;
			if (d.flags & (1 << 27)) B = d.nx_b;
			if (d.flags & (1 << 8)) i++;  // a pair op: the next descriptor stays unread
		}
	}
}

static void check_kept(const Tree &t, const Schedule &s, const StreamGeometry &g, const StreamTables &on, const StreamTables &off) {
	const int N = 2 * t.T - 1, n = (int)on.desc.size();
	const int64_t array_bytes = (int64_t)g.P * 4 * 8 * g.C;
	CHECK(on.keeps.size() == on.elisions.size() && off.keeps.size() == off.elisions.size() && on.keeps.size() == off.keeps.size());
	CHECK(on.desc.size() == off.desc.size() && on.pair_desc.size() == off.pair_desc.size() && on.pair_desc.size() == on.desc.size());
	if (on.desc.size() != off.desc.size() || on.pair_desc.size() != off.pair_desc.size() || on.keeps.size() != off.keeps.size()) return;
	// everything but the descriptors' request bits and fields is the same with the switch off
	CHECK(on.chunks.size() == off.chunks.size() && (on.chunks.empty() || std::memcmp(on.chunks.data(), off.chunks.data(), on.chunks.size() * sizeof(StreamChunk)) == 0));
	CHECK(on.plain_desc.size() == off.plain_desc.size() && (on.plain_desc.empty() || std::memcmp(on.plain_desc.data(), off.plain_desc.data(), on.plain_desc.size() * sizeof(StreamDesc)) == 0));
	CHECK(on.lower_desc.size() == off.lower_desc.size() && (on.lower_desc.empty() || std::memcmp(on.lower_desc.data(), off.lower_desc.data(), on.lower_desc.size() * sizeof(LowerDesc)) == 0));
	CHECK(on.row_entries == off.row_entries && on.site_tab == off.site_tab && on.qnode == off.qnode && on.op_tips == off.op_tips && on.op_deep == off.op_deep && on.pair_tab == off.pair_tab);
	std::vector<int> sop(N, -1), cleared((size_t)n * 2, 0);
	for (int i = 0; i < n; i++) sop[on.ops[i].parent] = i;
	for (size_t k = 0; k < on.keeps.size(); k++) {
		const StreamKeep &a = on.keeps[k], &b = off.keeps[k];
		const StreamElision &e = on.elisions[k];
		CHECK(a.node == e.node && a.parent == e.parent && a.side == e.side && b.node == e.node && b.reason == KEEP_OFF);
		CHECK(a.reason >= KEEP_KEPT && a.reason <= KEEP_OPENER);
		if (a.reason != KEEP_KEPT) continue;
		total_kept++;
		const int i = sop[e.parent];
		CHECK(i >= 0 && i + 1 < n && sop[e.node] == i + 1);
		if (i < 0 || i + 1 >= n) continue;
		cleared[(size_t)i * 2 + e.side] = 1;
		CHECK((off.desc[i].flags & (1 << (26 + e.side))) && (e.side ? off.desc[i].nx_b : off.desc[i].nx_a) == (int64_t)s.core_index[e.stored] * array_bytes);
	}
	for (int set = 0; set < 2; set++) {
		const std::vector<StreamDesc> &a = set ? on.pair_desc : on.desc, &b = set ? off.pair_desc : off.desc;
		for (int i = 0; i < n; i++) {
			StreamDesc x = a[i];
			for (int side = 0; side < 2; side++)
				if (cleared[(size_t)i * 2 + side]) {
					CHECK(!(x.flags & (1 << (26 + side))) && (side ? x.nx_b : x.nx_a) == 0);
					x.flags |= 1 << (26 + side);
					(side ? x.nx_b : x.nx_a) = side ? b[i].nx_b : b[i].nx_a;
				}
			CHECK(std::memcmp(&x, &b[i], sizeof(StreamDesc)) == 0);
		}
		std::vector<int64_t> held_on[2], held_off[2];
		replay(s, on, a, array_bytes, held_on);
		replay(s, off, b, array_bytes, held_off);
		for (int i = 0; i < n; i++)
			for (int side = 0; side < 2; side++) {
				CHECK((held_on[side][i] == -2) == (held_off[side][i] == -2));
				const int kind = (a[i].flags >> (3 * side)) & 7;
				if (held_on[side][i] == -2 || (kind != CH_CORE && kind < SK_CORE_TIP)) continue;
				total_reads++;
				CHECK(held_on[side][i] == held_off[side][i] && held_on[side][i] >= 0);
				const int node = side ? on.ops[i].rnode : on.ops[i].lnode;
				int stored = node;  // an elided child is formed from its stored child's plane
				for (const StreamElision &e : on.elisions)
					if (e.node == node) stored = e.stored;
				CHECK(held_on[side][i] == (int64_t)s.core_index[stored] * array_bytes);
			}
	}
}

static void check_tree(const Tree &t, const std::string &name) {
	for (bool park2 : {true, false}) {
		context = name + (park2 ? "" : ", lower_park2 off");
		ScheduleOptions o;
		o.lower_park2_on = park2;
		Schedule s;
		const std::string err = build_schedule(t.ref(), o, &s);
		CHECK(err.empty());
		if (!err.empty() || !s.walking) continue;
		StreamTables on, off;  // (built again and again into one value, as an engine does)
		for (int P : {1, 1000})
			for (int C : {1, 4}) {
				const size_t mstride = (size_t)((P + WAVE - 1) / WAVE) * WAVE;
				build_stream_tables(s, StreamGeometry{P, C, mstride, true, true, true}, &on);
				build_stream_tables(s, StreamGeometry{P, C, mstride, true, true, false}, &off);
				check_kept(t, s, StreamGeometry{P, C, mstride, true, true, true}, on, off);
			}
		// without the elision there is nothing to keep
		build_stream_tables(s, StreamGeometry{1, 1, WAVE, false, true, true}, &on);
		CHECK(on.keeps.empty() && on.elisions.empty());
	}
}

int main() {
	static const char *const shapes[4] = {"caterpillar", "balanced", "random", "cherry caterpillar"};
	for (int T = 2; T <= 130; T++)
		for (int shape = 0; shape < 4; shape++) check_tree(make_tree(T, shape, (unsigned)T), std::string(shapes[shape]) + " " + std::to_string(T));
	check_tree(make_tree(500, 2, 3), "random 500");
	check_tree(make_tree(1000, 2, 7), "random 1000");
	context = "all trees";
	CHECK(total_kept > 1000 && total_reads > total_kept);  // (the program would prove nothing about a rewrite that never happened)
	if (fails) return 1;
	std::printf("keep_sanitize: ok (%d operands kept, %d operand reads replayed)\n", total_kept, total_reads);
	return 0;
}
