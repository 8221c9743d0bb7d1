// phyamd_place4.inc: 4-state kernels of phyamd_placement_log_likelihoods -- lnL of query sequences placed on every edge of the
// engine's tree in one call -- included by phyamd_engine.hip inside its anonymous namespace.
//
// An EDGE is a non-root node n (the branch above it); u its parent, s its sibling.  The tree side of a placement is independent of
// the query: after the NNI call's walk (launch_nni_walk: every internal node's lower p_n and every internal non-root node's upper
// u_n in the batch scratch) k_place_table4 forms, per (edge, 64 patterns, category c), with P_lo = P(sigma t_n r_c) and
// P_hi = P((1 - sigma) t_n r_c),
//   U   = A_u o m_s,   A_u = P_u u_u (ones when u is the root),   m_s = P_s p_s (a tip's p is its mask)
//   E_c = [P_hi^T (pi o U)] o (P_lo p_n)
// so that the site likelihood of a query with tip vector x on a pendant branch of length l is sum_c w_c sum_i E_c,i (P(l r_c) x)_i.
// x enters only through its 4-bit state mask, so per (pendant length, edge, pattern) there are 16 possible site likelihoods: the
// categories meet once in LDS, y = sum_c w_c P(l r_c)^T E_c is added in category order, the 16 subset sums F[m] = sum_{s in m} y_s
// are formed in state order, and w_k log F[m] goes to table [length][edge][pattern][16] (padded patterns and patterns of weight 0
// store 0).  k_place_score4 is then a gather-and-add: a lane is a query, a workgroup stages the 128-byte rows of PLACE_EDGES edges
// and PLACE_TILE patterns in LDS, and a lane reads the entry its mask selects -- every lane of a wave inside the same row, so no
// bank conflict -- and adds it to the edge's sum, pattern after pattern through a fixed segment of REWEIGHT_SEGMENT patterns.  An
// entry that underflowed to -inf reaches exactly the queries that select it.  The segment sums go to the slab and k_place_finish
// adds them in segment order, writes the lnL rows and keeps each query's best edge in node order.  No atomics: a (query, edge,
// length) result depends on nothing but the engine's inputs, the query's masks, the split and the length.

// an edge: the node below it, its parent (BATCH_ROOT: the root, whose upper is ones) and its sibling
struct PlaceEdge {
	int32_t n, u, s;
	int32_t pad[5];
};

__device__ __forceinline__ PlaceEdge load_place_edge(const PlaceEdge *edges, int i) { return load_const_record<3>(edges, i); }

// y = M^T v, M row-major 4x4 at a wave-uniform address (scalar loads; matvec4's fence)
__device__ __forceinline__ d4 matvec4_transposed(cptr M, const d4 &v) {
	d4 r;
	r.x = M[0] * v.x + M[4] * v.y + M[8] * v.z + M[12] * v.w;
	r.y = M[1] * v.x + M[5] * v.y + M[9] * v.z + M[13] * v.w;
	r.z = M[2] * v.x + M[6] * v.y + M[10] * v.z + M[14] * v.w;
	r.w = M[3] * v.x + M[7] * v.y + M[11] * v.z + M[15] * v.w;
	__builtin_amdgcn_sched_barrier(0);
	return r;
}

struct PlaceTableArgs {
	const PlaceEdge *edges;  // [gridDim.y]: the chunk's
	int T, N, P, C, nblk, L;
	const uint8_t *tipmask;  // [T][P]
	const double *freqs, *props, *weights;
	const double *mats;      // [N][C][16]: the engine's lengths (the walk's item)
	const double *split;     // [3][N][C][16]: 0: sigma t_n, 1: (1 - sigma) t_n
	const double *pend;      // [L][C][16]: the pendant lengths
	const double *lower;     // [T - 1][C][nblk * 64][4]: p_n of internal node n at n - T
	const double *upper;     // [T - 1][C][nblk * 64][4]: u_n of internal non-root node n at n - T
	double *table;           // [L][gridDim.y][nblk * 64][16]
};

// grid (nblk, edges of the chunk), block (64, C): the C category waves of 64 patterns of one edge (k_nni4's shape)
__global__ __launch_bounds__(BATCH_MAX_CATEGORIES *WAVE) void k_place_table4(const PlaceTableArgs a) {
	__shared__ double sh[BATCH_MAX_CATEGORIES * WAVE * 4];  // E_c: [C][64][4]
	const int lane = threadIdx.x, c = __builtin_amdgcn_readfirstlane(threadIdx.y);  // this wave's category
	const int blk = blockIdx.x;
	const PlaceEdge ed = load_place_edge(a.edges, blockIdx.y);
	const int k0 = blk * WAVE + lane;  // the scratch is padded to whole blocks and the walk has written every lane's cells
	const bool valid = k0 < a.P;
	const int k = valid ? k0 : a.P - 1;
	const size_t plane = (size_t)a.nblk * WAVE * 4, node_stride = (size_t)a.C * plane;
	const cptr mats_c = as_const(a.mats + (size_t)c * 16), split_c = as_const(a.split + (size_t)c * 16);
	const double *lower_c = a.lower + (size_t)c * plane + (size_t)k0 * 4, *upper_c = a.upper + (size_t)c * plane + (size_t)k0 * 4;
	const auto message = [&](cptr M, int node) { return child_message4(M, a.tipmask + k, a.P, lower_c, node_stride, a.T, node); };
	d4 U = message(mats_c + (size_t)ed.s * a.C * 16, ed.s);
	if (ed.u != BATCH_ROOT) U = mul4(matvec4(opaque(mats_c + (size_t)ed.u * a.C * 16), load4(upper_c + (size_t)(ed.u - a.T) * node_stride)), U);
	const d4 f = mul4(d4{a.freqs[0], a.freqs[1], a.freqs[2], a.freqs[3]}, U);  // pi o U
	const d4 hi = matvec4_transposed(opaque(split_c + ((size_t)a.N + ed.n) * a.C * 16), f);
	const d4 lo = message(split_c + (size_t)ed.n * a.C * 16, ed.n);
	store4(sh + ((size_t)c * WAVE + lane) * 4, mul4(hi, lo));
	__syncthreads();  // the one meeting of the categories
	const double w = valid ? a.weights[k] : 0.0;
	for (int l = c; l < a.L; l += a.C) {  // the pendant lengths go round the category waves; each is summed in category order
		d4 y = d4{0., 0., 0., 0.};
		for (int cc = 0; cc < a.C; cc++) {
			const d4 t = matvec4_transposed(opaque(as_const(a.pend + ((size_t)l * a.C + cc) * 16)), load4(sh + ((size_t)cc * WAVE + lane) * 4));
			const double wc = a.props[cc];
			y = d4{y.x + wc * t.x, y.y + wc * t.y, y.z + wc * t.z, y.w + wc * t.w};
		}
		double *row = a.table + (((size_t)l * gridDim.y + blockIdx.y) * a.nblk * WAVE + k0) * 16;
		const double ys[4] = {y.x, y.y, y.z, y.w};
#pragma unroll
		for (int m = 0; m < 16; m += 2) {  // two masks per 16-byte store; F[m]: the states of m added in state order
			double v[2];
#pragma unroll
			for (int h = 0; h < 2; h++) {
				double F = 0.0;
#pragma unroll
				for (int s = 0; s < 4; s++)
					if ((m + h) >> s & 1) F += ys[s];
				v[h] = (m + h) != 0 && w != 0.0 ? w * log(F) : 0.0;
			}
			reinterpret_cast<double2 *>(row + m)[0] = double2{v[0], v[1]};
		}
	}
}

// raw [Q][P] (the caller's rows) -> packed [ceil(Ppad / 8)][Q]: query q's masks of patterns 8 g .. 8 g + 7 as the bytes of one
// 64-bit word, pattern-major, so that the lanes of a wave (queries) load neighbouring words; patterns past the last: 15 (their
// table rows hold 0)
__global__ __launch_bounds__(256) void k_place_masks(int Q, int P, int groups, const uint8_t *__restrict__ raw, unsigned long long *__restrict__ packed) {
	const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (idx >= (size_t)groups * Q) return;
	const int q = (int)(idx % Q), g = (int)(idx / Q);
	unsigned long long word = 0;
	for (int b = 0; b < 8; b++) {
		const int k = g * 8 + b;
		const unsigned long long m = k < P ? raw[(size_t)q * P + k] : 15;
		word |= m << (8 * b);
	}
	packed[idx] = word;
}

// Edges a workgroup holds per mask load.  A pattern costs a lane two integer instructions to turn its mask byte into an LDS
// address, whatever the number of edges, and one ds_read_b64 and one add per edge, so more edges spread the address work; fewer
// edges make more workgroups and smaller tiles.  Measured, whole best-only calls at 69 taxa x 238 patterns and 200 x 512 with 1024
// and 16384 queries (DESIGN.md): 2 is 3-5 % faster than 4 at 1024 queries and level with it at 16384; 8 is 3-7 % slower than 4
constexpr int PLACE_EDGES = 2;
constexpr int PLACE_TILE = WAVE;            // patterns of a tile: a block of the table kernel
constexpr int PLACE_MAX_QUERIES = 1024;     // queries (lanes) of a workgroup: the tile is loaded once for all of them

struct PlaceScoreArgs {
	const double *table;                // [L][E][Ppad][16]
	const unsigned long long *packed;   // [Ppad / 8][Q]
	double *slab;                       // [segments][L][E][Q]
	int E, Q, Ppad, segments, L;
};

// grid (blocks of blockDim.x queries, groups of PLACE_EDGES edges, segments * L), block (64 .. 1024): a lane is a query
__global__ __launch_bounds__(PLACE_MAX_QUERIES) void k_place_score4(const PlaceScoreArgs a) {
	__shared__ double tile[PLACE_EDGES * PLACE_TILE * 16];
	const int seg = blockIdx.z % a.segments, l = blockIdx.z / a.segments;
	const int e0 = blockIdx.y * PLACE_EDGES;
	const int q = blockIdx.x * blockDim.x + threadIdx.x, qc = q < a.Q ? q : a.Q - 1;
	const int kbegin = seg * REWEIGHT_SEGMENT, kend = min(kbegin + REWEIGHT_SEGMENT, a.Ppad);
	double acc[PLACE_EDGES];
#pragma unroll
	for (int j = 0; j < PLACE_EDGES; j++) acc[j] = 0.0;
	for (int kt = kbegin; kt < kend; kt += PLACE_TILE) {
		__syncthreads();  // (the previous tile has been read)
#pragma unroll
		for (int j = 0; j < PLACE_EDGES; j++) {
			const int e = min(e0 + j, a.E - 1);  // (past the last edge: a copy of it, never stored)
			const double2 *src = reinterpret_cast<const double2 *>(a.table + (((size_t)l * a.E + e) * a.Ppad + kt) * 16);
			double2 *dst = reinterpret_cast<double2 *>(tile + j * PLACE_TILE * 16);
			for (int i = threadIdx.x; i < PLACE_TILE * 8; i += blockDim.x) dst[i] = src[i];
		}
		__syncthreads();
		const unsigned long long *words = a.packed + (size_t)(kt / 8) * a.Q + qc;
#pragma unroll 2
		for (int g = 0; g < PLACE_TILE / 8; g++) {
			const unsigned long long word = words[(size_t)g * a.Q];
#pragma unroll
			for (int b = 0; b < 8; b++) {
				const int m = (int)(word >> (8 * b)) & 15;
#pragma unroll
				for (int j = 0; j < PLACE_EDGES; j++) acc[j] += tile[(j * PLACE_TILE + g * 8 + b) * 16 + m];
			}
		}
	}
	if (q >= a.Q) return;
#pragma unroll
	for (int j = 0; j < PLACE_EDGES; j++)
		if (e0 + j < a.E) a.slab[(((size_t)seg * a.L + l) * a.E + e0 + j) * a.Q + q] = acc[j];
}

struct PlaceFinishArgs {
	const double *slab;   // [segments][L][E][Q]
	double *out;          // [L][Q][cols] or null: the chunk's columns are the nodes first_node .. first_node + cols - 1
	double *best_lnl;     // [L][best_stride] or null, the chunk's queries from first_query on
	int32_t *best_node;
	int E, Q, segments, L, cols, first_node, first_edge, root, first_query, best_stride;
	int resume;           // an earlier edge chunk has left this query's best so far
};

// a thread is a (length, query): its columns in node order, a column's segments added in segment order, NaN in the root's column;
// the best edge so far is replaced only by a strictly larger lnL, so the smallest node id with the largest lnL stays
__global__ __launch_bounds__(256) void k_place_finish(const PlaceFinishArgs a) {
	const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (idx >= (size_t)a.L * a.Q) return;
	const int q = (int)(idx % a.Q), l = (int)(idx / a.Q);
	const size_t at = (size_t)l * a.best_stride + a.first_query + q;
	double best = 0.0;
	int node = -1;
	if (a.best_lnl && a.resume) best = a.best_lnl[at], node = a.best_node[at];
	for (int col = 0; col < a.cols; col++) {
		const int n = a.first_node + col;
		double s = NAN;
		if (n != a.root) {
			const int e = (n < a.root ? n : n - 1) - a.first_edge;
			s = 0.0;
			for (int seg = 0; seg < a.segments; seg++) s += a.slab[(((size_t)seg * a.L + l) * a.E + e) * a.Q + q];
			if (node < 0 || s > best) best = s, node = n;
		}
		if (a.out) a.out[idx * a.cols + col] = s;
	}
	if (a.best_lnl) a.best_lnl[at] = best, a.best_node[at] = node;
}
