// phyamd_spr4.inc: 4-state kernels of phyamd_spr_log_likelihoods -- lnL of every SPR regraft of chosen subtrees of the engine's tree
// in one call -- included by phyamd_engine.hip inside its anonymous namespace.
//
// A ROW is a prune node p; u its parent, s its sibling.  Removing p is the same as letting it send the all-ones message to u
// (P . 1 = 1): the pruned tree is the engine's tree with one ghost child (BATCH_GHOST), u a pass-through node whose lower is s's
// message and which hands its own upper on to s through P_u -- the branch of s has absorbed the branch of u, and no merged matrix
// is formed.  k_spr_walk4 walks each row's ghosted copy of the engine's park_all op lists (build_batch_ops) once up and once
// down, which leaves every internal node's lower p_n and every internal non-root node's upper u_n OF THE PRUNED TREE in the row's
// scratch (the lowers inside p's subtree are the engine's own; no upper is formed there).  A CANDIDATE is a target edge, named
// by the node w below it: x its parent, y its sibling (never p: w = s is no candidate).  k_spr4 forms, per (candidate, 64
// patterns, category c), with H_w = P(0.5 t_w r_c),
//   lo  = H_w p_w,   m_p = P_p p_p                       (a tip's p is its mask)
//   U   = (x is the root ? 1 : P_x u_x) o P_y p_y        (w's upper in the pruned tree, formed here: a tip needs none stored)
//   L_c = sum_i pi_i U_i (H_w (lo o m_p))_i
// then L = sum_c w_c L_c through LDS in category order and w_k log L per lane.  Every row reads the engine's matrices [N][C][16]
// and the half-length ones through scalar loads.  No floating-point atomics: the 64 lanes are summed by wave_sum, one double per
// (candidate, block) goes to the slab, and k_spr_finish adds a candidate's blocks in block order.  A row's arithmetic therefore
// depends on nothing but the engine's inputs and p: not on the other rows, its position among them, or the chunk it ran in.

struct SprWalkArgs {
	const BatchOp *ops;      // [row][post-order T - 1 | pre-order T - 1]: the engine's park_all lists with p a ghost in u's ops
	int T, N, P, C, nblk;
	const uint8_t *tipmask;  // [T][P]
	const double *mats;      // [N][C][16]: the engine's lengths, shared by every row
	double *lower;           // [row][T - 1][C][nblk * 64][4]: p_n of internal node n at n - T
	double *upper;           // [row][T - 1][C][nblk * 64][4]: u_n of internal non-root node n at n - T
};

// grid (nblk, rows), block (64, C): the C category waves of 64 patterns of one row (k_batch_walk4's shape).  Stores partials only:
// no site likelihood, no branch term, and the categories never meet
__global__ __launch_bounds__(BATCH_MAX_CATEGORIES *WAVE) void k_spr_walk4(const SprWalkArgs a) {
	const int lane = threadIdx.x, c = __builtin_amdgcn_readfirstlane(threadIdx.y);  // this wave's category
	const int blk = blockIdx.x, row = blockIdx.y;
	const int nops = a.T - 1;
	const BatchOp *lower_ops = a.ops + (size_t)row * 2 * nops, *upper_ops = lower_ops + nops;  // (wave-uniform: scalar addresses)
	const int k0 = blk * WAVE + lane;  // the scratch is padded to whole blocks: every lane owns its cells
	const int k = k0 < a.P ? k0 : a.P - 1;
	const size_t plane = (size_t)a.nblk * WAVE * 4, node_stride = (size_t)a.C * plane;
	const size_t cell = ((size_t)row * nops * a.C + c) * plane + (size_t)k0 * 4;
	const cptr mats_c = as_const(a.mats + (size_t)c * 16);
	double *lower_c = a.lower + cell, *upper_c = a.upper + cell;
	const d4 one = d4{1., 1., 1., 1.};
	const auto message = [&](int child) {  // ones for the ghost, P_child . mask for a tip, P_child . p_child for an internal node
		if (child == BATCH_GHOST) return one;
		const cptr M = opaque(mats_c + (size_t)child * a.C * 16);
		if (child < a.T) return matvec4(M, mask4(a.tipmask[(size_t)child * a.P + k]));
		return matvec4(M, load4(lower_c + (size_t)(child - a.T) * node_stride));
	};
	d4 p = d4{0., 0., 0., 0.};
#pragma unroll 1
	for (int i = 0; i < nops; i++) {
		const BatchOp op = load_batch_op(lower_ops, i);
		const d4 l = op.carry == 1 ? matvec4(opaque(mats_c + (size_t)op.left * a.C * 16), p) : message(op.left);
		const d4 r = op.carry == 2 ? matvec4(opaque(mats_c + (size_t)op.right * a.C * 16), p) : message(op.right);
		p = mul4(l, r);
		store4(lower_c + (size_t)(op.node - a.T) * node_stride, p);
	}
#pragma unroll 1
	for (int i = 0; i < nops; i++) {  // park_all lists: an upper is the root's (ones) or in its node's slot, never carried
		const BatchOp op = load_batch_op(upper_ops, i);
		if (op.dst_left < 0 && op.dst_right < 0) continue;  // two tips below, or a node of the pruned subtree
		d4 up = one;
		if (op.src != BATCH_ROOT) up = matvec4(opaque(mats_c + (size_t)op.node * a.C * 16), load4(upper_c + (size_t)op.src * node_stride));
		if (op.dst_left >= 0) store4(upper_c + (size_t)op.dst_left * node_stride, mul4(up, message(op.right)));
		if (op.dst_right >= 0) store4(upper_c + (size_t)op.dst_right * node_stride, mul4(up, message(op.left)));
	}
}

// a regraft: row (prune node p) onto the edge above w; x: w's parent (BATCH_ROOT: the root, whose upper is ones), y: w's sibling;
// p_left: p is its parent's left child (phyamd_tripod4.inc: the order of a pass)
struct SprCand {
	int32_t row, w, x, y, p, p_left;
	int32_t pad[2];
};

__device__ __forceinline__ SprCand load_spr_cand(const SprCand *cands, int i) { return load_const_record<5>(cands, i); }

struct SprArgs {
	const SprCand *cands;    // [gridDim.y], row-major: neighbouring workgroups share p's lower and the row's scratch in L2
	int T, N, P, C, nblk;
	const uint8_t *tipmask;  // [T][P]
	const double *freqs, *props, *weights;
	const double *mats;      // [N][C][16]: the engine's lengths
	const double *half;      // [N][C][16]: half the engine's lengths
	const double *lower;     // the walk's
	const double *upper;
	double *slab;            // [gridDim.y][nblk]: the block's sum of w log L
};

// grid (nblk, candidates), block (64, C): the C category waves of 64 patterns of one regraft
__global__ __launch_bounds__(BATCH_MAX_CATEGORIES *WAVE) void k_spr4(const SprArgs a) {
	__shared__ double sh[BATCH_MAX_CATEGORIES * WAVE];  // [C][64]
	const int lane = threadIdx.x, c = __builtin_amdgcn_readfirstlane(threadIdx.y);  // this wave's category
	const int blk = blockIdx.x;
	const SprCand cd = load_spr_cand(a.cands, blockIdx.y);
	const int k0 = blk * WAVE + lane;  // the scratch is padded to whole blocks and the walk has written every lane's cells
	const bool valid = k0 < a.P;
	const int k = valid ? k0 : a.P - 1;
	const size_t plane = (size_t)a.nblk * WAVE * 4, node_stride = (size_t)a.C * plane;
	const size_t cell = ((size_t)cd.row * (a.T - 1) * a.C + c) * plane + (size_t)k0 * 4;
	const cptr mats_c = as_const(a.mats + (size_t)c * 16), half_c = as_const(a.half + (size_t)c * 16);
	const double *lower_c = a.lower + cell, *upper_c = a.upper + cell;
	// M . mask for a tip, M . p_node (the pruned tree's) for an internal node.  The product is formed inside either branch
	// (child_message4 does): after them, the scalar loads of three matrices meet in one block and overflow the SGPRs
	const auto message = [&](cptr M, int node) { return child_message4(M, a.tipmask + k, a.P, lower_c, node_stride, a.T, node); };
	const cptr Hw = half_c + (size_t)cd.w * a.C * 16;
	const d4 lo = message(Hw, cd.w), mp = message(mats_c + (size_t)cd.p * a.C * 16, cd.p);
	d4 U = message(mats_c + (size_t)cd.y * a.C * 16, cd.y);
	if (cd.x != BATCH_ROOT) U = mul4(matvec4(opaque(mats_c + (size_t)cd.x * a.C * 16), load4(upper_c + (size_t)(cd.x - a.T) * node_stride)), U);
	const d4 f = mul4(d4{a.freqs[0], a.freqs[1], a.freqs[2], a.freqs[3]}, U);
	sh[c * WAVE + lane] = a.props[c] * dot4(f, matvec4(opaque(Hw), mul4(lo, mp)));
	__syncthreads();  // the one meeting of the categories
	if (c != 0) return;
	double L = 0.0;
	for (int cc = 0; cc < a.C; cc++) L += sh[cc * WAVE + lane];
	const double s = wave_sum(valid ? a.weights[k] * log(L) : 0.0);
	if (lane == 0) a.slab[(size_t)blockIdx.y * a.nblk + blk] = s;
}

// out [rows][N]: a candidate's blocks added in block order, NaN in every other cell (cand_of [rows][N]: the cell's candidate
// index, -1: none)
__global__ __launch_bounds__(256) void k_spr_finish(size_t cells, int nblk, const int32_t *__restrict__ cand_of, const double *__restrict__ slab,
                                                   double *__restrict__ out) {
	const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (idx >= cells) return;
	const int ci = cand_of[idx];
	double s = NAN;
	if (ci >= 0) {
		s = 0.0;
		for (int b = 0; b < nblk; b++) s += slab[(size_t)ci * nblk + b];
	}
	out[idx] = s;
}
