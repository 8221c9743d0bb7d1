// phyamd_bhess.inc -- 4-state kernels of phyamd_branch_hessian: the full branch-length Hessian of lnL, every pair of branches
// (_singleTreeLikelihood_ddlogP, treelikelihood.c:532-690, as calculate_hessian asks for it, hessian.c:14-25) without pruning the
// tree per pair -- included by phyamd_engine.hip inside its anonymous namespace.
//
// Read-only kernels over the partials a keep-partials gradient leaves resident (the layouts k_post4 reads).  Per category c and
// pattern k, with p_n the lower and u_n the upper partial of node n and P_n its matrix,
//   msg(n)      = P_n p_n                                   the message n sends to its parent
//   A_m         = P_m^T (pi o u_m)     (m = root: pi)        the message that reaches m from above
//   T_a^(par a) = r_c Q P_a p_a                             tangent in t_a of the message a sends to its parent
//   T_a^(par m) = P_m (T_a^(m) o msg(other child of m))     carried up one node at a time
// and the site likelihood's derivatives are
//   L_a   = sum_c w_c (pi o u_a) . T_a^(par a)
//   L_aa  = sum_c w_c r_c^2 (pi o u_a) . (Q Q P_a p_a)
//   L_ab  = sum_c w_c r_c (pi o u_b) . (Q P_b (T_a^(b) o msg(other child of b)))       a below b
//   L_ab  = sum_c w_c sum_i (A_m)_i (T_a^(m))_i (T_b^(m))_i                           a, b on two sides of m
//   H[a][b] = sum_k w_k (L_ab / L - L_a L_b / L^2)
// k_bhess_walk climbs from every node to the root: it leaves every tangent T_a^(m) in a slot of its own and G[a][k] = L_a / L_k, and
// scores the diagonal and the (node, ancestor) pairs on the way.  The remaining pairs are products of stored rows: k_bhess_cousins
// (K axis = pattern x category x state: one v_mfma_f64_16x16x4_f64 consumes the 4 states of one (pattern, category) for a 16 x 16
// tile of pairs) and k_bhess_outer (-sum_k w_k G[a][k] G[b][k], K axis = patterns).  Every kernel writes one partial sum per
// block of 64 patterns; k_bhess_finish adds them in block order, so no sum depends on an atomic or on what the scratch held.
// A call runs the patterns in chunks of whole blocks (k0: the chunk's first pattern, Pc = 64 nblk: its padded width).

constexpr int BHESS_MAX_CATEGORIES = 8;  // the category waves of a workgroup (k_bhess_walk), like BATCH_MAX_CATEGORIES

// step s of the walk that starts at node a: the ancestor m the tangent in slot s enters (slots = steps: T_a^(m) lives in slot s),
// and the child of m that is not on a's path.  A start's steps run from its parent to the root
struct BhessStep {
	int32_t m, sib, a, pad;
};
struct BhessStart {
	int32_t node, first, count, pad;  // steps [first, first + count): count = the depth of the node
};
// a 16 x 16 tile of pairs (a, b): the rows the two operands read -- tangent slots (k_bhess_cousins, with the node m whose two
// subtrees the pairs span) or rows of G (k_bhess_outer) -- and the nodes they stand for.  A tile's edge repeats a row it has and
// names no node (-1): the products are formed and dropped
struct BhessTile {
	int32_t m, pad;
	int32_t row_a[16], row_b[16], node_a[16], node_b[16];
};

struct BhessArgs {
	const BhessStart *starts;  // [gridDim.y] (k_bhess_walk)
	const BhessStep *steps;
	const int32_t *lower_of, *upper_of;  // [N]: index of a node's stored lower (-1: a tip) and of its upper partial
	int T, N, P, C, root, fold;
	int k0, Pc, nblk, nsteps;
	const uint8_t *tipmask;                // [T][P]
	const double *lower, *upper;           // node partials [C][P][4]
	const double *mats, *qp, *qqp;         // [N][C][16]: P, r Q P, r^2 Q Q P
	const double *freqs, *props, *weights;
	double *site;                          // [2][Pc]: w_k / L_k | 1 / L_k, 0 past the last pattern
	double *tan;                           // [slots][C][Pc][4]
	double *G;                             // [N][Pc]
	double *slab;                          // [nsteps][nblk] (node, ancestor) terms | [N][nblk] gradient | [N][nblk] diagonal
};

// r_c Q P and r_c^2 Q Q P of every (node, category): one thread per entry
__global__ __launch_bounds__(256) void k_bhess_matrices(int count, int C, const double *__restrict__ mats, const double *__restrict__ Q,
                                                       const double *__restrict__ rates, double *__restrict__ qp, double *__restrict__ qqp) {
	const int idx = blockIdx.x * 256 + threadIdx.x;
	if (idx >= count * 16) return;
	const int j = idx & 3, i = (idx >> 2) & 3, nc = idx >> 4;
	const double r = rates[nc % C];
	const double *Pm = mats + (size_t)nc * 16;
	double one = 0.0, two = 0.0;
	for (int k = 0; k < 4; k++) {
		double qpkj = 0.0;  // (Q P)[k][j]
		for (int l = 0; l < 4; l++) qpkj += Q[k * 4 + l] * Pm[l * 4 + j];
		one += i == k ? qpkj : 0.0;
		two += Q[i * 4 + k] * qpkj;
	}
	qp[idx] = r * one;
	qqp[idx] = r * r * two;
}

// w_k / L_k and 1 / L_k of a chunk's patterns from the root's lower partial: one thread per pattern
__global__ __launch_bounds__(256) void k_bhess_site(const BhessArgs a) {
	const int kl = blockIdx.x * 256 + threadIdx.x;
	if (kl >= a.Pc) return;
	const int k = a.k0 + kl;
	double wl = 0.0, inv = 0.0;
	if (k < a.P) {
		const double *root = a.lower + (size_t)a.lower_of[a.root] * a.C * a.P * 4;
		double L = 0.0;
		for (int c = 0; c < a.C; c++) {
			const d4 p = load4(root + ((size_t)c * a.P + k) * 4);
			L += a.props[c] * (a.freqs[0] * p.x + a.freqs[1] * p.y + a.freqs[2] * p.z + a.freqs[3] * p.w);
		}
		inv = 1.0 / L;
		wl = a.weights[k] / L;
	}
	a.site[kl] = wl;
	a.site[a.Pc + kl] = inv;
}

__device__ __forceinline__ int32_t scalar_int(const int32_t *p, int i) {  // a wave-uniform entry of a list: one s_load_dword
	return ((const __attribute__((address_space(4))) int32_t *)p)[i];
}

// The tangent walk.  Grid (blocks of 64 patterns, start nodes), workgroup = 64 patterns x C category waves, as k_post4; the path
// is a wave-uniform list, the matrices come through scalar loads.  The categories meet in LDS once per step, wave 0 adds them in
// category order and reduces the lanes to one partial sum per (pair, block).  Three LDS rows in turn: a step's row is written
// only after the barrier that follows wave 0's reading of its previous use
__global__ __launch_bounds__(WAVE *BHESS_MAX_CATEGORIES) void k_bhess_walk(const BhessArgs a) {
	__shared__ double sh[3][BHESS_MAX_CATEGORIES][WAVE];
	const int lane = threadIdx.x, c = __builtin_amdgcn_readfirstlane(threadIdx.y), blk = blockIdx.x;
	const int kl = blk * WAVE + lane, k0 = a.k0 + kl;
	const bool valid = k0 < a.P;
	const int k = valid ? k0 : a.P - 1;
	const size_t npd = (size_t)a.C * a.P * 4, cell = ((size_t)c * a.P + k) * 4;
	const int32_t *const st = reinterpret_cast<const int32_t *>(a.starts + blockIdx.y);
	const int node = scalar_int(st, 0), first = scalar_int(st, 1), count = scalar_int(st, 2);
	const auto lower = [&](int n) {  // p_n
		const int at = scalar_int(a.lower_of, n);
		if (at < 0) return mask4(a.tipmask[(size_t)n * a.P + k]);
		return load4_global(a.lower + (size_t)at * npd + cell);
	};
	const cptr pi = as_const(a.freqs);
	const d4 f = d4{pi[0], pi[1], pi[2], pi[3]};
	const auto upper = [&](int n) {  // pi o u_n
		const d4 u = load4_global(a.upper + (size_t)scalar_int(a.upper_of, n) * npd + cell);
		return a.fold ? u : mul4(f, u);
	};
	const auto matrix = [&](const double *set, int n) { return opaque(as_const(set + ((size_t)n * a.C + c) * 16)); };
	const auto slot = [&](int s) { return a.tan + (((size_t)s * a.C + c) * a.Pc + kl) * 4; };
	const double wc = as_const(a.props)[c], wl = a.site[kl];

	const d4 pa = lower(node), fu = upper(node);
	d4 t = matvec4(matrix(a.qp, node), pa);
	sh[0][c][lane] = valid ? wc * dot4(fu, t) : 0.0;
	sh[1][c][lane] = valid ? wc * dot4(fu, matvec4(matrix(a.qqp, node), pa)) : 0.0;
	if (!valid) t = d4{0., 0., 0., 0.};  // (a padding lane's tangents are zeros: the products that read them add nothing)
	store4(slot(first), t);
	lds_barrier();
	if (c == 0) {
		double La = 0.0, Laa = 0.0;
		for (int cc = 0; cc < a.C; cc++) La += sh[0][cc][lane], Laa += sh[1][cc][lane];
		a.G[(size_t)node * a.Pc + kl] = La * a.site[a.Pc + kl];
		const double g = wave_sum(wl * La), d = wave_sum(wl * Laa);
		if (lane == 0) {
			a.slab[((size_t)a.nsteps + node) * a.nblk + blk] = g;
			a.slab[((size_t)a.nsteps + a.N + node) * a.nblk + blk] = d;
		}
	}
	for (int j = 0; j + 1 < count; j++) {  // the tangent enters m = ancestor j, not the root: the pair (node, m), then on through P_m
		const int32_t *const sp = reinterpret_cast<const int32_t *>(a.steps + first + j);
		const int m = scalar_int(sp, 0), sib = scalar_int(sp, 1);
		const d4 x = mul4(t, matvec4(matrix(a.mats, sib), lower(sib)));
		const int buf = (j & 1) ? 0 : 2;
		sh[buf][c][lane] = wc * dot4(upper(m), matvec4(matrix(a.qp, m), x));
		t = matvec4(matrix(a.mats, m), x);
		store4(slot(first + j + 1), t);
		lds_barrier();
		if (c == 0) {
			double Lam = 0.0;
			for (int cc = 0; cc < a.C; cc++) Lam += sh[buf][cc][lane];
			const double s = wave_sum(wl * Lam);
			if (lane == 0) a.slab[(size_t)(first + j) * a.nblk + blk] = s;
		}
	}
}

// Cousin pairs.  Grid (blocks of 64 patterns, tiles), 4 waves.  Per category the workgroup stages the tile's 16 + 16 tangent
// rows of its 64 patterns through LDS -- coalesced 32-byte loads, the a rows multiplied by (w_k / L_k) w_c A_m on the way -- and
// each wave runs 16 of the patterns through the matrix pipe: lane l holds A[a = l & 15][state l >> 4] and B[state l >> 4][b = l & 15].
// An LDS row is [64 patterns][4 states] with its 16-byte pairs at (2 pattern + state / 2) ^ row, so the 32 lanes of a ds_read_b64
// phase (16 rows x 2 states) fall on 32 different 8-byte banks.  The waves' tiles are added in wave order.
// out [tiles][nblk][16][16]
__global__ __launch_bounds__(256) void k_bhess_cousins(const BhessArgs a, const BhessTile *__restrict__ tiles, double *__restrict__ out) {
	__shared__ double sA[16 * 256], sB[16 * 256];
	const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), blk = blockIdx.x;
	const int32_t *const tile = reinterpret_cast<const int32_t *>(tiles + blockIdx.y);
	const int m = scalar_int(tile, 0);
	const int kl = blk * WAVE + lane, k0 = a.k0 + kl;
	const int k = k0 < a.P ? k0 : a.P - 1;
	const cptr pi = as_const(a.freqs);
	const d4 f = d4{pi[0], pi[1], pi[2], pi[3]};
	const double wl = a.site[kl];
	const int row = lane & 15, state = lane >> 4;
	f64x4 acc = {0., 0., 0., 0.};
	for (int c = 0; c < a.C; c++) {
		d4 fac = f;
		if (m != a.root) {
			const d4 u = load4_global(a.upper + ((size_t)scalar_int(a.upper_of, m) * a.C + c) * a.P * 4 + (size_t)k * 4);
			fac = matvecT4(opaque(as_const(a.mats + ((size_t)m * a.C + c) * 16)), a.fold ? u : mul4(f, u));
		}
		const double s = wl * as_const(a.props)[c];
		fac = d4{fac.x * s, fac.y * s, fac.z * s, fac.w * s};
		if (c > 0) lds_barrier();  // (every wave has read the previous category's rows)
#pragma unroll
		for (int r = 0; r < 4; r++) {
			const int sr = wv + 4 * r;
			const d4 ta = load4_global(a.tan + (((size_t)scalar_int(tile, 2 + sr) * a.C + c) * a.Pc + kl) * 4);
			const d4 tb = load4_global(a.tan + (((size_t)scalar_int(tile, 18 + sr) * a.C + c) * a.Pc + kl) * 4);
			const int lo = sr * 256 + (((2 * lane) ^ sr) << 1), hi = sr * 256 + (((2 * lane + 1) ^ sr) << 1);
			*reinterpret_cast<double2 *>(sA + lo) = double2{ta.x * fac.x, ta.y * fac.y};
			*reinterpret_cast<double2 *>(sA + hi) = double2{ta.z * fac.z, ta.w * fac.w};
			*reinterpret_cast<double2 *>(sB + lo) = double2{tb.x, tb.y};
			*reinterpret_cast<double2 *>(sB + hi) = double2{tb.z, tb.w};
		}
		lds_barrier();
#pragma unroll
		for (int j = 0; j < 16; j++) {
			const int at = row * 256 + (((2 * (wv * 16 + j) + (state >> 1)) ^ row) << 1) + (state & 1);
			acc = __builtin_amdgcn_mfma_f64_16x16x4f64(sA[at], sB[at], acc, 0, 0, 0);
		}
	}
	lds_barrier();
	double *const red = sA;  // [wave][register][lane]
	for (int reg = 0; reg < 4; reg++) red[(wv * 4 + reg) * WAVE + lane] = acc[reg];
	lds_barrier();
	const int reg = tid >> 6;
	const double sum = ((red[reg * WAVE + lane] + red[(4 + reg) * WAVE + lane]) + red[(8 + reg) * WAVE + lane]) + red[(12 + reg) * WAVE + lane];
	out[((size_t)blockIdx.y * a.nblk + blk) * 256 + ((lane >> 4) + 4 * reg) * 16 + (lane & 15)] = sum;  // (the f64 D layout)
}

// The outer-product term -sum_k w_k G[a][k] G[b][k] of a tile: grid (blocks of 64 patterns, tiles), one wave; the same instruction
// with K over the patterns -- step j takes patterns 16 q + j, q = l >> 4, from both operands.  out [tiles][nblk][16][16]
__global__ __launch_bounds__(WAVE) void k_bhess_outer(const BhessArgs a, const BhessTile *__restrict__ tiles, double *__restrict__ out) {
	const int lane = threadIdx.x, blk = blockIdx.x;
	const BhessTile *const tile = tiles + blockIdx.y;
	const int kl0 = blk * WAVE + (lane >> 4) * 16;
	const double *ga = a.G + (size_t)tile->row_a[lane & 15] * a.Pc + kl0, *gb = a.G + (size_t)tile->row_b[lane & 15] * a.Pc + kl0;
	f64x4 acc = {0., 0., 0., 0.};
#pragma unroll
	for (int j = 0; j < 16; j++) {
		const int k0 = a.k0 + kl0 + j;
		const double w = a.weights[k0 < a.P ? k0 : a.P - 1];  // (G is 0 past the last pattern)
		acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-w * ga[j], gb[j], acc, 0, 0, 0);
	}
	for (int reg = 0; reg < 4; reg++) out[((size_t)blockIdx.y * a.nblk + blk) * 256 + ((lane >> 4) + 4 * reg) * 16 + (lane & 15)] = acc[reg];
}

// The chunk's matrix from the partial sums, blocks added in block order, in four launches one after the other (every entry has
// one writer per launch):
//   0  Hc[a][b] = Hc[b][a] = the outer-product term of the pair (Hc was zeroed: the root's row and column stay 0); of a tile on
//      the diagonal of the tiling the entries with row <= column, so that both triangles hold the same bits
//   1  += the (node, ancestor) terms, one thread per step, and after them one thread per node: the diagonal's term and gc[node]
//   2  += the cousin tiles
//   3  the running matrix and gradient take the chunk: H = Hc (the first chunk) or H + Hc
struct BhessFinish {
	int mode, N, nblk, root, nsteps, first;
	size_t count;             // threads with work
	const BhessTile *tiles;
	const BhessStep *steps;
	const double *slab;       // the walk's slab (mode 1) or a tile slab (0, 2)
	double *Hc, *gc, *H, *g;  // [N][N], [N]
};
__global__ __launch_bounds__(256) void k_bhess_finish(const BhessFinish a) {
	const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (idx >= a.count) return;
	const auto blocks = [&](size_t row, size_t stride, size_t at) {
		double s = 0.0;
		for (int b = 0; b < a.nblk; b++) s += a.slab[(row * a.nblk + b) * stride + at];
		return s;
	};
	const size_t N = (size_t)a.N;
	if (a.mode == 0 || a.mode == 2) {
		const BhessTile &t = a.tiles[idx >> 8];
		const int r = (int)(idx >> 4) & 15, col = (int)idx & 15, na = t.node_a[r], nb = t.node_b[col];
		if (na < 0 || nb < 0 || (a.mode == 0 && t.node_a[0] == t.node_b[0] && r > col)) return;
		const double v = blocks(idx >> 8, 256, idx & 255);
		a.Hc[na * N + nb] = a.mode == 0 ? v : a.Hc[na * N + nb] + v;
		a.Hc[nb * N + na] = a.Hc[na * N + nb];
	} else if (a.mode == 1) {
		if (idx < (size_t)a.nsteps) {
			const BhessStep s = a.steps[idx];
			if (s.m == a.root) return;
			a.Hc[(size_t)s.a * N + s.m] += blocks(idx, 1, 0);
			a.Hc[(size_t)s.m * N + s.a] = a.Hc[(size_t)s.a * N + s.m];
		} else {
			const size_t n = idx - a.nsteps;
			const bool root = (int)n == a.root;
			a.gc[n] = root ? 0.0 : blocks(a.nsteps + n, 1, 0);
			if (!root) a.Hc[n * N + n] += blocks(a.nsteps + N + n, 1, 0);
		}
	} else {
		a.H[idx] = a.first ? a.Hc[idx] : a.H[idx] + a.Hc[idx];
		if (idx < N) a.g[idx] = a.first ? a.gc[idx] : a.g[idx] + a.gc[idx];
	}
}
