// Sanitizer driver for stream_elide (physher_amd/csrc/phyamd_tree_schedule.h): the rewrite of the streamed walks' tables that takes
// stored nodes beside a tip or a cherry out of the post-order walk's stores.  No GPU, no engine.  Built and run by
// tests/test_stream_elide_sanitizers.py with -fsanitize=address,undefined; exits non-zero on any finding (ASan/UBSan abort) or on a
// failed structure check.  The trees are generated here: caterpillar, balanced and seeded random ones from 2 to 130 tips (both
// sides of the 32-op chunking threshold) and random trees of 500 and 1000 tips, each with both park-slot schedules.
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
// 3: a caterpillar whose rungs alternate between tips and cherries (every rung an eligible node)
static Tree make_tree(int T, int shape, unsigned seed) {
	Tree t{T, 2 * T - 2, std::vector<int32_t>(2 * T - 1, -1), std::vector<int32_t>(2 * T - 1, -1)};
	std::vector<int> active;
	for (int i = 0; i < T; i++) active.push_back(i);
	unsigned state = seed * 2654435761u + 12345u;
	auto draw = [&](int n) {
		state = state * 1664525u + 1013904223u;
		return (int)((state >> 8) % (unsigned)n);
	};
	if (shape == 3) {  // the spine's foot: four tips joined pairwise (a stored node), or what there is of them
		int next = T, used = 0, spine = -1;
		auto join = [&](int l, int r) {
			t.left[next] = l, t.right[next] = r;
			return next++;
		};
		if (T >= 4) spine = join(join(0, 1), join(2, 3)), used = 4;
		else spine = 0, used = 1;
		for (int rung = 0; used < T; rung++) {
			if (rung % 2 && used + 2 <= T) spine = join(spine, join(used, used + 1)), used += 2;
			else spine = rung % 4 ? join(used, spine) : join(spine, used), used += 1;
		}
		return t;
	}
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

static int total_elided = 0;

static void check_elided(const Tree &t, const Schedule &s, const StreamGeometry &g, const StreamTables &tb, const StreamTables &off) {
	const int T = t.T, N = 2 * T - 1, n = (int)tb.desc.size();
	const int64_t array_bytes = (int64_t)g.P * 4 * 8 * g.C, row_bytes = (int64_t)tb.mstride * 4;
	// what the switch leaves alone: the plain tables are those of a build without it, the post-order walk's but for bit 11
	CHECK(tb.plain_desc.size() == off.desc.size() && tb.plain_chunks.size() == off.chunks.size());
	CHECK(off.plain_desc.empty() && off.plain_chunks.empty() && off.elisions.empty());
	if (tb.plain_desc.size() == off.desc.size() && !off.desc.empty())
		CHECK(std::memcmp(tb.plain_desc.data(), off.desc.data(), off.desc.size() * sizeof(StreamDesc)) == 0);
	if (tb.plain_chunks.size() == off.chunks.size() && !off.chunks.empty())
		CHECK(std::memcmp(tb.plain_chunks.data(), off.chunks.data(), off.chunks.size() * sizeof(StreamChunk)) == 0);
	CHECK(tb.ops.size() == off.ops.size() && tb.lower_desc.size() == off.lower_desc.size() && tb.site_tab == off.site_tab && tb.qnode == off.qnode);
	CHECK(tb.row_entries.size() >= off.row_entries.size() && std::equal(off.row_entries.begin(), off.row_entries.end(), tb.row_entries.begin()));
	CHECK(tb.row_entries.size() == (size_t)tb.words * 8 && tb.row_entries.size() <= (size_t)N * 32);
	for (int ent : tb.row_entries) CHECK(ent == -1 || (ent & 0xFFFFF) < T);
	for (int tip : tb.op_tips) CHECK(tip >= -1 && tip < T);
	std::vector<int> el_of(N, -1), lop(N, -1), sop(N, -1);
	for (size_t i = 0; i < tb.elisions.size(); i++) el_of[tb.elisions[i].node] = (int)i;
	for (size_t i = 0; i < s.walk_lower_chunk_ops.size(); i++) lop[s.walk_lower_chunk_ops[i].parent] = (int)i;
	for (size_t i = 0; i < s.walk_chunk_ops.size(); i++) sop[s.walk_chunk_ops[i].parent] = (int)i;
	int flagged = 0;
	for (size_t i = 0; i < tb.lower_desc.size(); i++) {
		const bool bit = tb.lower_desc[i].flags & (1 << 11);
		flagged += bit;
		CHECK(bit == (el_of[s.walk_lower_chunk_ops[i].parent] >= 0));
		CHECK((tb.lower_desc[i].flags & ~(1 << 11)) == off.lower_desc[i].flags);
	}
	CHECK(flagged == (int)tb.elisions.size());
	total_elided += flagged;
	for (const StreamElision &e : tb.elisions) {
		CHECK(e.node >= T && e.node < N && e.node != t.root && s.parent[e.node] == e.parent && s.node_kind[e.node] == CH_CORE);
		CHECK(s.parent[e.stored] == e.node && s.parent[e.sibling] == e.node && e.stored != e.sibling);
		CHECK(s.node_kind[e.stored] == CH_CORE && el_of[e.stored] < 0);
		CHECK(e.sibling_kind == s.node_kind[e.sibling] && (e.sibling_kind == CH_TIP || e.sibling_kind == CH_CHERRY));
		CHECK(e.source == 1 || e.source == 2);
		CHECK(lop[e.node] >= 0 && lop[e.parent] > lop[e.node] && sop[e.parent] >= 0);
		if (sop[e.parent] < 0 || lop[e.node] < 0) continue;
		// the parent's pre-order op: the kind, the cherry's matrices, the tips' table slots, and who requests the stored child's plane
		const int ip = sop[e.parent];
		const StreamDesc &d = tb.desc[ip];
		CHECK(((d.flags >> (3 * e.side)) & 7) == (e.sibling_kind == CH_TIP ? SK_CORE_TIP : SK_CORE_CHERRY));
		CHECK((e.side ? d.rnode : d.lnode) == e.node * g.C * 128 && (e.side ? d.rm : d.lm)[0] == e.sibling * g.C * 128);
		const int *tips = &tb.op_tips[(size_t)ip * 12 + 6 * e.side];
		if (e.sibling_kind == CH_TIP) CHECK(tips[0] == e.sibling && tips[1] == -1);
		else CHECK(tips[0] >= 0 && tips[1] >= 0 && s.parent[tips[0]] == e.sibling && s.parent[tips[1]] == e.sibling && tips[0] != tips[1] && tips[2] == -1);
		const int64_t want = (int64_t)s.core_index[e.stored] * array_bytes;
		bool first = false;
		for (size_t k = 0; k + 1 < s.walk_chunk_off.size(); k++)
			if (s.walk_chunk_off[k] == ip && s.walk_chunk_off[k + 1] > ip) {
				first = true;
				CHECK((e.side ? tb.chunks[k].b : tb.chunks[k].a) == s.core_index[e.stored]);
				CHECK(tb.chunks[k].mask_words >= 1 && tb.chunks[k].mask_word >= off.words && tb.chunks[k].mask_word + (tb.chunks[k].same_row ? 0 : tb.chunks[k].mask_words - 1) < tb.words);
			}
		if (!first) {
			const StreamDesc &pv = tb.desc[ip - 1];
			CHECK((e.side ? pv.nx_b : pv.nx_a) == want && (pv.flags & (1 << (26 + e.side))));
			const int words = (pv.flags >> 14) & 3, same = (pv.flags >> 25) & 1;
			CHECK(words >= 1 && pv.nx_words >= (int64_t)off.words * row_bytes && pv.nx_words + (same ? 0 : (words - 1) * row_bytes) < (int64_t)tb.words * row_bytes);
			CHECK(((pv.flags >> 24) & 1) == (((d.flags >> 3) & 7) != CH_CORE));
		}
	}
	// every other descriptor field is the plain one's
	for (int i = 0; i < n; i++) {
		const StreamDesc &a = tb.desc[i], &b = tb.plain_desc[i];
		CHECK(a.parent == b.parent && a.lnode == b.lnode && a.rnode == b.rnode && a.nx_u == b.nx_u && a.st_left == b.st_left && a.st_right == b.st_right);
		CHECK((a.flags & ~(0x3F | 3 << 14 | 1 << 24 | 1 << 25)) == (b.flags & ~(0x3F | 3 << 14 | 1 << 24 | 1 << 25)));
		for (int side = 0; side < 2; side++) {
			const int ka = (a.flags >> (3 * side)) & 7, kb = (b.flags >> (3 * side)) & 7;
			CHECK(ka == kb || (kb == CH_CORE && (ka == SK_CORE_TIP || ka == SK_CORE_CHERRY)));
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
		StreamTables tb, off;  // (built again and again into one value, as an engine does)
		for (int P : {1, 65, 1000})
			for (int C : {1, 4}) {
				const size_t mstride = (size_t)((P + WAVE - 1) / WAVE) * WAVE;
				build_stream_tables(s, StreamGeometry{P, C, mstride, true}, &tb);
				build_stream_tables(s, StreamGeometry{P, C, mstride}, &off);
				check_elided(t, s, StreamGeometry{P, C, mstride, true}, tb, off);
			}
	}
}

int main() {
	static const char *const shapes[4] = {"caterpillar", "balanced", "random", "cherry caterpillar"};
	for (int T = 2; T <= 130; T++)
		for (int shape = 0; shape < 4; shape++) check_tree(make_tree(T, shape, (unsigned)T), std::string(shapes[shape]) + " " + std::to_string(T));
	check_tree(make_tree(500, 2, 3), "random 500");
	check_tree(make_tree(1000, 2, 7), "random 1000");
	context = "all trees";
	CHECK(total_elided > 1000);  // (the program would prove nothing about a rewrite that never happened)
	if (fails) return 1;
	std::printf("elide_sanitize: ok (%d nodes elided)\n", total_elided);
	return 0;
}
