// phyamd_batch4.inc: 4-state kernels of phyamd_gradient_batch and phyamd_gradient_batch_trees -- lnL and the branch gradient for
// many branch-length vectors on one tree, or for many trees, and one alignment in a single launch -- included by phyamd_engine.hip
// inside its anonymous namespace.
//
// The single-evaluation walks are built to fill the card with ONE evaluation.  A batch of B small ones (69 taxa x 238 patterns x 4
// categories is 16 waves each) fills it along the item axis instead: workgroup (block, item) = the category waves of 64 patterns of
// one item.  A wave walks the whole tree twice from two host-built op lists (build_batch_ops) -- shared by every item of a batch of
// lengths (built once per topology), the item's own in a batch of trees (BatchArgs::item_stride) --: post-order, storing every
// internal node's partial p_n in the item's scratch (one 32-byte access per lane);
// after ONE meeting of the categories in LDS for the site likelihood, pre-order with the branch terms.  Matrices are wave-uniform
// and come through scalar loads from the item's block; tip messages are P . mask from the 4-bit tip codes, the same bytes for
// every item.  No floating-point atomics: a branch term is summed over the 64 lanes by wave_sum (fixed order), written to the
// slab [item][block][C][node], and k_batch_finish adds the blocks in block order.  An item's arithmetic therefore depends on
// nothing but its own lengths and op lists: not on the batch size, its position in the batch, or the chunk it ran in.
// phyamd_gradient_batch_weights gives every item a weight row of its own (BatchArgs::weight_stride) and, where the items share the
// engine's lengths, runs the walk once in its terms form (batch_walk4<FOLD, true>, phyamd_reweight.inc).

// (BatchOp and BATCH_*: phyamd_types.h)
constexpr int BATCH_MAX_CATEGORIES = 8;  // one LDS row of site-likelihood terms per category; at most 8 category waves per workgroup

// record i of a list of eight-dword records, its first WORDS words (the others 0), through the constant address space like the
// matrices: the lists are read-only kernel inputs at wave-uniform addresses, so the words come by one s_load_dwordx8 instead of
// vector loads on the walk's dependent chain
template <int WORDS, typename Rec>
__device__ __forceinline__ Rec load_const_record(const Rec *list, int i) {
	static_assert(sizeof(Rec) == 32 && WORDS <= 8, "a record is eight dwords");
	typedef const __attribute__((address_space(4))) int32_t *cint;
	const cint o = (cint)reinterpret_cast<const int32_t *>(list + i);
	int32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
	for (int j = 0; j < WORDS; j++) w[j] = o[j];
	Rec r;
	__builtin_memcpy(&r, w, sizeof r);
	return r;
}
__device__ __forceinline__ BatchOp load_batch_op(const BatchOp *ops, int i) { return load_const_record<7>(ops, i); }

struct BatchArgs {
	const BatchOp *lower_ops, *upper_ops;  // T - 1 ops each; item b's lists are at + b * item_stride
	int item_stride;                       // in ops: 0 (every item walks the same lists) or 2 (T - 1) (a batch of trees)
	int T, N, P, C, nblk, upper_slots;
	int grad;                              // 0: the post-order pass and lnL only
	const uint8_t *tipmask;                // [T][P]
	const double *freqs, *props, *weights, *Q;
	const double *mats;                    // [item][N][C][16]
	double *lower;                         // [item][T - 1][C][nblk * 64][4]
	double *upper;                         // [item][upper_slots][C][nblk * 64][4]
	double *lnl_part;                      // [item][nblk]
	double *slab;                          // [item][nblk][C][N]
	// a weight row per item (phyamd_gradient_batch_weights): item b reads weights + b * weight_stride; 0: every item the same row
	size_t weight_stride;
	// the terms form (k_reweight_terms4, phyamd_reweight.inc): ONE item over the blocks of a pattern chunk that starts at pattern
	// k0, its unweighted per-pattern rows in R [1 + N C][Pc] (Pc = 64 nblk); not_finite: set to 1.0 by a pattern whose log L_k is
	// not finite (null: nobody asks)
	int k0, Pc;
	double *R, *not_finite;
};

// P(t) of every (item, node, category) from the eigen system: k_transition_matrices' arithmetic, each item with its own lengths
// ([items][N]; the root's entry is skipped, nothing reads its matrix).  roots: [items], each item's own root (a batch of trees),
// or null: `root` is every item's
__global__ void k_batch_matrices(int C, int N, int items, const double *__restrict__ model, const double *__restrict__ rates,
                                 const double *__restrict__ lengths, int root, const int32_t *__restrict__ roots, double *__restrict__ mats) {
	const size_t total = (size_t)items * N * C * 16;
	const double *eval = model, *evec = model + 4, *ivec = model + 4 + 16;
	for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
		const int j = idx & 3, i = (idx >> 2) & 3;
		const int c = (idx >> 4) % C;
		const size_t in = idx / ((size_t)16 * C);  // item * N + node
		if ((int)(in % N) == (roots ? roots[in / N] : root)) continue;
		const double t = lengths[in] * rates[c];
		double p = 0.;
		for (int k = 0; k < 4; k++) p += ivec[k * 4 + j] * evec[i * 4 + k] * exp(eval[k] * t);
		mats[idx] = fabs(p);  // substmodel.c:552
	}
}

// message of a node through the matrix M at this lane's pattern: M . mask for a tip (node < T; tip_k: the lane's pattern in the
// tips' code rows, P apart), M . p_node for an internal node (lower_c: the lane's cell of internal node T's stored partial, the
// nodes' node_stride apart).  The product is formed inside either branch (k_spr4)
__device__ __forceinline__ d4 child_message4(cptr M, const uint8_t *tip_k, int P, const double *lower_c, size_t node_stride, int T, int node) {
	if (node < T) return matvec4(opaque(M), mask4(tip_k[(size_t)node * P]));
	return matvec4(opaque(M), load4(lower_c + (size_t)(node - T) * node_stride));
}

// message of a child to its parent at (pattern lane, category c): P_child . mask for a tip, P_child . p_child for an internal node
__device__ __forceinline__ d4 batch_message(const BatchArgs &a, cptr mats_c, const double *lower_c, size_t node_stride, int child, int k) {
	return child_message4(mats_c + (size_t)child * a.C * 16, a.tipmask + k, a.P, lower_c, node_stride, a.T, child);
}

// The walk of one (item, block) by its C category waves: the body of k_batch_walk4 below and of k_reweight_terms4
// (phyamd_reweight.inc).  a.grad: the pre-order pass too (a launch argument, not an instantiation: the lnL-only form runs the very
// instructions of the gradient form's first half, so both return the same lnL bits); FOLD: PHYAMD_GRAD_FOLD_ROOT_FREQS (k_upper4's
// arithmetic: the root's children start from pi, the state sum drops it).
// TERMS: the same arithmetic for one item, but what k_batch_walk4 weights by w_k and sums over the lanes is stored per lane,
// unweighted, as a row of a.R: row 0 = log L_k, row 1 + c N + node = f . u . (Q P p) / L_k, the root's rows and every row past the
// last pattern 0
template <bool FOLD, bool TERMS>
__device__ __forceinline__ void batch_walk4(const BatchArgs &a, double *sh) {
	const int lane = threadIdx.x, c = __builtin_amdgcn_readfirstlane(threadIdx.y);  // this wave's category
	const int blk = blockIdx.x, item = blockIdx.y;
	// the item's op lists: a wave-uniform offset (the workgroup id times a launch argument) on a kernel argument, so the lists stay
	// at scalar addresses
	const BatchOp *lower_ops = a.lower_ops + (size_t)item * a.item_stride, *upper_ops = a.upper_ops + (size_t)item * a.item_stride;
	const int k0 = blk * WAVE + lane;  // the scratch is padded to whole blocks: every lane owns its cells
	const int kg = TERMS ? a.k0 + k0 : k0;
	const bool valid = kg < a.P;
	const int k = valid ? kg : a.P - 1;
	const int nops = a.T - 1;
	const size_t plane = (size_t)a.nblk * WAVE * 4, node_stride = (size_t)a.C * plane;
	const double *mats_i = a.mats + (size_t)item * a.N * a.C * 16;
	double *lower_i = a.lower + (size_t)item * nops * node_stride + (size_t)k0 * 4;
	const d4 pi = d4{a.freqs[0], a.freqs[1], a.freqs[2], a.freqs[3]};

	{
		const cptr mats_c = as_const(mats_i + (size_t)c * 16);
		double *lower_c = lower_i + (size_t)c * plane;
		d4 p = d4{0., 0., 0., 0.};
#pragma unroll 1
		for (int i = 0; i < nops; i++) {
			const BatchOp op = load_batch_op(lower_ops, i);
			const d4 l = op.carry == 1 ? matvec4(opaque(mats_c + (size_t)op.left * a.C * 16), p) : batch_message(a, mats_c, lower_c, node_stride, op.left, k);
			const d4 r = op.carry == 2 ? matvec4(opaque(mats_c + (size_t)op.right * a.C * 16), p) : batch_message(a, mats_c, lower_c, node_stride, op.right, k);
			p = mul4(l, r);
			store4(lower_c + (size_t)(op.node - a.T) * node_stride, p);
		}
		// the last op is the root's: integrate_partials (treelikelihood.c:1473-1487), as k_lower4 forms it
		sh[c * WAVE + lane] = a.props[c] * (pi.x * p.x + pi.y * p.y + pi.z * p.z + pi.w * p.w);
	}
	__syncthreads();  // the one meeting of the categories
	double L = 0.0;
	for (int cc = 0; cc < a.C; cc++) L += sh[cc * WAVE + lane];
	double w = 1.0;
	if constexpr (TERMS) {
		if (c == 0) {
			const double ll = log(L);
			a.R[k0] = valid ? ll : 0.0;
			if (valid && a.not_finite && !isfinite(ll)) *a.not_finite = 1.0;
		}
	} else {
		w = valid ? a.weights[(size_t)item * a.weight_stride + k] : 0.0;
		if (c == 0) {
			const double s = wave_sum(valid ? log(L) * w : 0.0);
			if (lane == 0) a.lnl_part[(size_t)item * a.nblk + blk] = s;
		}
	}
	if (!a.grad) return;

	const double wl = valid ? w / L : 0.0;  // the gradient's w_k / L_k (treelikelihood.c:2879); TERMS: 1 / L_k
	const d4 one = d4{1., 1., 1., 1.}, f = FOLD ? one : pi;
	const cptr Q = as_const(a.Q);
	double *upper_i = a.upper + (size_t)item * a.upper_slots * node_stride + (size_t)k0 * 4;
	{
		const cptr mats_c = as_const(mats_i + (size_t)c * 16);
		const double *lower_c = lower_i + (size_t)c * plane;
		double *upper_c = upper_i + (size_t)c * plane;
		double *slab = TERMS ? nullptr : a.slab + (((size_t)item * a.nblk + blk) * a.C + c) * a.N;
		double *rows = TERMS ? a.R + ((size_t)1 + (size_t)c * a.N) * a.Pc + k0 : nullptr;  // this lane's cell of the category's rows
		d4 carried = one;
#pragma unroll 1
		for (int i = 0; i < nops; i++) {
			const BatchOp op = load_batch_op(upper_ops, i);
			const d4 bl = batch_message(a, mats_c, lower_c, node_stride, op.left, k);
			const d4 br = batch_message(a, mats_c, lower_c, node_stride, op.right, k);
			d4 up = FOLD ? pi : one;
			if (op.src != BATCH_ROOT) {
				const d4 u = op.src == BATCH_CARRY ? carried : load4(upper_c + (size_t)op.src * node_stride);
				up = matvec4(opaque(mats_c + (size_t)op.node * a.C * 16), u);
			}
			const d4 ul = mul4(up, br), ur = mul4(up, bl);  // treelikelihood.c:2142-2147
			// g[child][c] = sum_k w_k / L_k sum_i f_i u_i (Q P p)_i   (treelikelihood.c:2846-2939)
			const double tl = wl * dot4(mul4(f, ul), matvec4(opaque(Q), bl));
			const double tr = wl * dot4(mul4(f, ur), matvec4(opaque(Q), br));
			if constexpr (TERMS) {  // one 512-byte row segment per wave each
				rows[(size_t)op.left * a.Pc] = valid ? tl : 0.0;
				rows[(size_t)op.right * a.Pc] = valid ? tr : 0.0;
				if (op.src == BATCH_ROOT) rows[(size_t)op.node * a.Pc] = 0.0;
			} else {
				const double gl = wave_sum(tl), gr = wave_sum(tr);
				if (lane == 0) {
					slab[op.left] = gl;
					slab[op.right] = gr;
				}
			}
			if (op.dst_left >= 0) store4(upper_c + (size_t)op.dst_left * node_stride, ul);
			if (op.dst_right >= 0) store4(upper_c + (size_t)op.dst_right * node_stride, ur);
			if (op.dst_left == BATCH_CARRY) carried = ul;
			if (op.dst_right == BATCH_CARRY) carried = ur;
		}
	}
}

// grid (nblk, items), block (64, C): the C category waves of one (item, block)
template <bool FOLD>
__global__ __launch_bounds__(BATCH_MAX_CATEGORIES *WAVE) void k_batch_walk4(const BatchArgs a) {
	__shared__ double sh[BATCH_MAX_CATEGORIES * WAVE];
	batch_walk4<FOLD, false>(a, sh);
}

// out[item][0] = lnL, out[item][1 + node * C + c] = g[node][c] (the root's row 0): the blocks' entries added in block order.
// rows = 1 (lnL only) or 1 + N C; thread r of an item reads the slab's entry r - 1 of every block ([C][N]: coalesced).  roots:
// as k_batch_matrices'
__global__ __launch_bounds__(256) void k_batch_finish(int items, int N, int C, int nblk, int root, const int32_t *__restrict__ roots, int rows,
                                                     const double *__restrict__ lnl_part, const double *__restrict__ slab, double *__restrict__ out) {
	const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (idx >= (size_t)items * rows) return;
	const size_t item = idx / rows;
	const int r = (int)(idx % rows);
	double s = 0.0;
	if (r == 0) {
		for (int b = 0; b < nblk; b++) s += lnl_part[item * nblk + b];
		out[item * rows] = s;
		return;
	}
	const int c = (r - 1) / N, node = (r - 1) % N;
	if (node != (roots ? roots[item] : root))
		for (int b = 0; b < nblk; b++) s += slab[((item * nblk + b) * C + c) * N + node];
	out[item * rows + 1 + (size_t)node * C + c] = s;
}
