// phyamd_reweight.inc: 4-state kernels of phyamd_gradient_batch_weights without per-item branch lengths -- lnL and the branch
// gradient of one tree under many pattern-weight vectors (bootstrap and jackknife replicates, RELL, site minibatches) from ONE walk
// of the tree -- included by phyamd_engine.hip inside its anonymous namespace.
//
// Partials and matrices do not depend on the pattern weights: with R[0][k] = log L_k and R[1 + c N + node][k] = the branch term of
// (node, category c) at pattern k over L_k, replicate b's results are the products
//   lnl[b] = sum_k W[b][k] R[0][k],      g[b][node][c] = sum_k W[b][k] R[1 + c N + node][k].
// k_reweight_terms4 is the batched walk (phyamd_batch4.inc) of the engine's own tree, lengths and matrices that leaves R;
// k_reweight_mfma forms the products on the matrix pipe, K = the pattern axis, cut into segments of REWEIGHT_SEGMENT patterns that
// depend on the pattern index alone; k_reweight_finish adds a replicate's segments in segment order.  No floating-point atomics: a
// replicate's bits depend on its weight row and R only -- not on the replicate count, its position, the chunks of replicates, or
// what the scratch held.  A call runs the patterns in chunks of whole blocks (k0: the chunk's first pattern, Pc: its padded width).

// grid (blocks of the chunk), block (64, C): k_batch_walk4's walk in its terms form (BatchArgs::R)
template <bool FOLD>
__global__ __launch_bounds__(BATCH_MAX_CATEGORIES *WAVE) void k_reweight_terms4(const BatchArgs a) {
	__shared__ double sh[BATCH_MAX_CATEGORIES * WAVE];
	batch_walk4<FOLD, true>(a, sh);
}

constexpr int REWEIGHT_SEGMENT = 64 * WAVE;  // patterns per segment of the K axis: 64 blocks

struct ReweightArgs {
	const double *W;  // [items][Pc] weight rows of the chunk's patterns, 0 past the last pattern
	const double *R;  // [rows][Pc]
	double *part;     // [segments][items][rows]
	double *out;      // [items][rows]
	int items, rows, Pc, segments;
	int N, C;         // (k_reweight_finish: row 1 + c N + node goes to entry 1 + node C + c)
};

// A 16 replicates x 16 rows tile of W R^T over one segment: grid (row tiles, replicate tiles, segments), one wave.
// v_mfma_f64_16x16x4_f64 takes A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15]: lane l holds replicate l & 15 in A and row
// l & 15 in B, and reads 4 consecutive patterns of each (32 bytes) that feed four instructions: in lane group q = l >> 4, step j
// takes pattern k + 4 q + j from both operands -- a permuted but fixed order over the 16 patterns of a round.  A tile's edge:
// replicates and rows that do not exist enter as zeros (their pointers stay on row 0) and are not written
__global__ __launch_bounds__(WAVE) void k_reweight_mfma(const ReweightArgs a) {
	const int lane = threadIdx.x, q = lane >> 4, i = lane & 15;
	const int b = blockIdx.y * 16 + i, row = blockIdx.x * 16 + i, seg = blockIdx.z;
	const bool has_b = b < a.items, has_row = row < a.rows;
	const int first = seg * REWEIGHT_SEGMENT, last = min(first + REWEIGHT_SEGMENT, a.Pc);
	const double *w = a.W + (size_t)(has_b ? b : 0) * a.Pc + 4 * q, *r = a.R + (size_t)(has_row ? row : 0) * a.Pc + 4 * q;
	f64x4 acc = {0., 0., 0., 0.};
	for (int k = first; k < last; k += 16) {  // (Pc is a multiple of 64)
		d4 wv = load4(w + k), rv = load4(r + k);
		if (!has_b) wv = d4{0., 0., 0., 0.};
		if (!has_row) rv = d4{0., 0., 0., 0.};
		acc = __builtin_amdgcn_mfma_f64_16x16x4f64(wv.x, rv.x, acc, 0, 0, 0);
		acc = __builtin_amdgcn_mfma_f64_16x16x4f64(wv.y, rv.y, acc, 0, 0, 0);
		acc = __builtin_amdgcn_mfma_f64_16x16x4f64(wv.z, rv.z, acc, 0, 0, 0);
		acc = __builtin_amdgcn_mfma_f64_16x16x4f64(wv.w, rv.w, acc, 0, 0, 0);
	}
	const int orow = blockIdx.x * 16 + i;  // (the f64 D layout: register reg of lane l is D[(l >> 4) + 4 reg][l & 15])
	for (int reg = 0; reg < 4; reg++) {
		const int ob = blockIdx.y * 16 + q + 4 * reg;
		if (ob < a.items && orow < a.rows) a.part[((size_t)seg * a.items + ob) * a.rows + orow] = acc[reg];
	}
}

// out[b][0] = lnl, out[b][1 + node C + c] = g[node][c] of the chunk's patterns: a replicate's segments added in segment order;
// one thread per (replicate, row)
__global__ __launch_bounds__(256) void k_reweight_finish(const ReweightArgs a) {
	const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (idx >= (size_t)a.items * a.rows) return;
	const size_t b = idx / a.rows;
	const int r = (int)(idx % a.rows);
	double s = 0.0;
	for (int seg = 0; seg < a.segments; seg++) s += a.part[((size_t)seg * a.items + b) * a.rows + r];
	const int c = (r - 1) / a.N, node = (r - 1) % a.N;
	a.out[b * a.rows + (r == 0 ? 0 : 1 + (size_t)node * a.C + c)] = s;
}
