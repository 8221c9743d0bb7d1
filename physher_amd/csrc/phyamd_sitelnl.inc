// phyamd_sitelnl.inc: 4-state kernels of phyamd_pattern_log_likelihoods_trees -- the per-pattern log-likelihoods of many trees on one
// alignment, their weighted sums, and RELL replicates of them -- included by phyamd_engine.hip inside its anonymous namespace.
//
// k_sitelnl_walk4 is the batched walk's (phyamd_batch4.inc) post-order pass alone, and it keeps only what a later op still has to
// read: an op's result stays in registers when the next op is its parent, and is parked in a slot plane of the item otherwise.  The
// list is build_batch_ops' post-order (the larger subtree first), so at most floor(log2 T) - 1 results wait at any time and a
// caterpillar parks none (site_lnl_ops, phyamd_queries.inc), where the batched walk stores all T - 1.  What the batched walk forms
// per lane and drops -- log L_k -- is the result: a row per item, padded to whole blocks with zeros, which is also the operand R of
// the replicates' product W R^T (k_reweight_mfma, as it is: W the replicates' weight rows, R the items' rows).
// k_sitelnl_rell_finish adds a (replicate, item)'s segments in segment order.  No floating-point atomics: an item's row and sums
// depend on its own op list and lengths only, a replicate's entry on its weight row and the item's row only.

// A post-order list with its slot words (site_lnl_ops): BatchOp's fields that post-order lists leave unused say where the children's
// partials are and where the result goes.  src = the left child's partial, dst_left = the right child's (BATCH_NONE: a tip, formed
// from its codes; BATCH_CARRY: the op in front's result, in registers; >= 0: a slot); dst_right = the result (BATCH_CARRY: handed
// on in registers; >= 0: a slot; BATCH_NONE: the root's, integrated at once)
struct SiteLnlArgs {
	const BatchOp *ops;      // [item][T - 1]
	int T, N, P, C, nblk, slots;
	const uint8_t *tipmask;  // [T][P]
	const double *freqs, *props, *weights;
	const double *mats;      // [item][N][C][16] (k_batch_matrices)
	double *park;            // [item][slots][C][nblk * 64][4]
	double *rows;            // [item][nblk * 64]: log L_k, 0 past the last pattern
	double *lnl_part;        // [item][nblk]: sum over the block's patterns of w_k log L_k
};

// message of a child to its parent: P_child . (mask of a tip | the op in front's result | a parked partial)
__device__ __forceinline__ d4 sitelnl_message(const SiteLnlArgs &a, cptr mats_c, const double *park_c, size_t slot_stride, int child, int src, const d4 &carried, int k) {
	const cptr M = opaque(mats_c + (size_t)child * a.C * 16);
	if (src == BATCH_NONE) return matvec4(M, mask4(a.tipmask[(size_t)child * a.P + k]));
	if (src == BATCH_CARRY) return matvec4(M, carried);
	return matvec4(M, load4(park_c + (size_t)src * slot_stride));
}

// grid (nblk, items), block (64, C): the C category waves of one (item, block), as k_batch_walk4
__global__ __launch_bounds__(BATCH_MAX_CATEGORIES *WAVE) void k_sitelnl_walk4(const SiteLnlArgs a) {
	__shared__ double sh[BATCH_MAX_CATEGORIES * WAVE];
	const int lane = threadIdx.x, c = __builtin_amdgcn_readfirstlane(threadIdx.y);  // this wave's category
	const int blk = blockIdx.x, item = blockIdx.y;
	const int nops = a.T - 1;
	const BatchOp *ops = a.ops + (size_t)item * nops;
	const int k0 = blk * WAVE + lane;  // the scratch is padded to whole blocks: every lane owns its cells
	const bool valid = k0 < a.P;
	const int k = valid ? k0 : a.P - 1;
	const size_t plane = (size_t)a.nblk * WAVE * 4, slot_stride = (size_t)a.C * plane;
	const cptr mats_c = as_const(a.mats + ((size_t)item * a.N * a.C + c) * 16);
	double *park_c = a.park + (size_t)item * a.slots * slot_stride + (size_t)c * plane + (size_t)k0 * 4;
	d4 p = d4{0., 0., 0., 0.};
#pragma unroll 1
	for (int i = 0; i < nops; i++) {
		const BatchOp op = load_batch_op(ops, i);
		const d4 l = sitelnl_message(a, mats_c, park_c, slot_stride, op.left, op.src, p, k);
		const d4 r = sitelnl_message(a, mats_c, park_c, slot_stride, op.right, op.dst_left, p, k);
		p = mul4(l, r);
		if (op.dst_right >= 0) store4(park_c + (size_t)op.dst_right * slot_stride, p);  // (a slot this op has read may be the one it fills: a lane reads its cell first)
	}
	// the last op is the root's: integrate_partials (treelikelihood.c:1473-1487), as the batched walk forms it
	sh[c * WAVE + lane] = a.props[c] * (a.freqs[0] * p.x + a.freqs[1] * p.y + a.freqs[2] * p.z + a.freqs[3] * p.w);
	__syncthreads();  // the one meeting of the categories
	if (c != 0) return;
	double L = 0.0;
	for (int cc = 0; cc < a.C; cc++) L += sh[cc * WAVE + lane];
	const double ll = valid ? log(L) : 0.0;
	a.rows[(size_t)item * a.nblk * WAVE + k0] = ll;
	const double s = wave_sum(valid ? ll * a.weights[k] : 0.0);
	if (lane == 0) a.lnl_part[(size_t)item * a.nblk + blk] = s;
}

// out[replicate][item] of a (replicate chunk, item chunk): the segments of k_reweight_mfma's part [segment][replicate][item]
// added in segment order; one thread per entry
__global__ __launch_bounds__(256) void k_sitelnl_rell_finish(int replicates, int items, int segments, const double *__restrict__ part, double *__restrict__ out) {
	const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x, n = (size_t)replicates * items;
	if (idx >= n) return;
	double s = 0.0;
	for (int seg = 0; seg < segments; seg++) s += part[(size_t)seg * n + idx];
	out[idx] = s;
}
