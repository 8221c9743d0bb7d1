// phyamd_tripod4.inc: 4-state kernels of phyamd_spr_optimize -- for every SPR regraft of chosen subtrees the three branch lengths
// that meet at the graft point, optimised one at a time, pass after pass -- included by phyamd_engine.hip inside its anonymous
// namespace.
//
// The walk is phyamd_spr_log_likelihoods' (k_spr_walk4, phyamd_spr4.inc): per ROW (prune node p) every internal lower and upper of
// the pruned tree in the row's scratch.  Per candidate (target edge w; x its parent, y its sibling) three messages meet at the new
// central node u, and none of them depends on the three lengths a = t_p, b = t_w, cu = t_u being optimised:
//   A = p's lower (a tip: its mask),   B = w's lower in the pruned tree,   U = (x is the root ? 1 : P_x u_x) o P_y p_y   (k_spr4's)
//   L_c = sum_i pi_i U_i [P(cu) ((P(b) B) o (P(a) A))]_i,      P(t) = V e^(lambda t r_c) V^-1
// In the length of the branch being visited L is k_cbopt_solve4's exponential sum, sum_c sum_e K[c][e] exp(lambda_e r_c t), with
//   u:  K = w_c (V^T (pi o U))_e (V^-1 [(P(b) B) o (P(a) A)])_e
//   w:  K = w_c (V^T [(P(cu)^T (pi o U)) o (P(a) A)])_e (V^-1 B)_e
//   p:  the same with A and B (a and b) exchanged
// (no reversibility is used).  k_tripod_upper4 writes pi o U once per candidate; k_tripod_solve4 runs a candidate's whole rule
// (include/physher_amd.h; its one body: three_branch_rule, phyamd_rule.inc) in one workgroup: per visit two 4x4 matrices per category in LDS, K formed per pattern by the thread that
// reads it back, then the safeguarded Newton iteration on cbopt_evaluate's fixed-order sums, so every thread holds the same bits and
// takes the same accept, bisect and stop decisions.  No walk, no matrix launch and no host round trip per visit; no floating-point
// atomics.  A candidate's arithmetic depends on the engine's inputs, p and w alone.

struct TripodUpperArgs {
	const SprCand *cands;    // [gridDim.y]
	int T, N, P, C, nblk;
	const uint8_t *tipmask;  // [T][P]
	const double *freqs;
	const double *mats;      // [N][C][16]: the engine's lengths
	const double *lower;     // the walk's (SprWalkArgs)
	const double *upper;
	double *fU;              // [gridDim.y][C][nblk * 64][4]: pi o U
};

// grid (nblk, candidates), block (64, C): the C category waves of 64 patterns of one regraft (k_spr4's shape and U)
__global__ __launch_bounds__(BATCH_MAX_CATEGORIES *WAVE) void k_tripod_upper4(const TripodUpperArgs a) {
	const int lane = threadIdx.x, c = __builtin_amdgcn_readfirstlane(threadIdx.y);  // this wave's category
	const SprCand cd = load_spr_cand(a.cands, blockIdx.y);
	const int k0 = blockIdx.x * WAVE + lane;  // the scratch is padded to whole blocks and the walk has written every lane's cells
	const int k = k0 < a.P ? k0 : a.P - 1;
	const size_t plane = (size_t)a.nblk * WAVE * 4, node_stride = (size_t)a.C * plane;
	const size_t cell = ((size_t)cd.row * (a.T - 1) * a.C + c) * plane + (size_t)k0 * 4;
	const cptr mats_c = as_const(a.mats + (size_t)c * 16);
	const double *lower_c = a.lower + cell, *upper_c = a.upper + cell;
	d4 U = child_message4(mats_c + (size_t)cd.y * a.C * 16, a.tipmask + k, a.P, lower_c, node_stride, a.T, cd.y);
	if (cd.x != BATCH_ROOT) U = mul4(matvec4(opaque(mats_c + (size_t)cd.x * a.C * 16), load4(upper_c + (size_t)(cd.x - a.T) * node_stride)), U);
	store4(a.fU + ((size_t)blockIdx.y * a.C + c) * plane + (size_t)k0 * 4, mul4(d4{a.freqs[0], a.freqs[1], a.freqs[2], a.freqs[3]}, U));
}

// y = M v and y = M^T v, M row-major 4x4 in LDS (every lane reads the same words: a broadcast)
__device__ __forceinline__ d4 tripod_matvec(const double *M, const d4 &v) {
	return d4{M[0] * v.x + M[1] * v.y + M[2] * v.z + M[3] * v.w, M[4] * v.x + M[5] * v.y + M[6] * v.z + M[7] * v.w,
	          M[8] * v.x + M[9] * v.y + M[10] * v.z + M[11] * v.w, M[12] * v.x + M[13] * v.y + M[14] * v.z + M[15] * v.w};
}
__device__ __forceinline__ d4 tripod_matvec_t(const double *M, const d4 &v) {
	return d4{M[0] * v.x + M[4] * v.y + M[8] * v.z + M[12] * v.w, M[1] * v.x + M[5] * v.y + M[9] * v.z + M[13] * v.w,
	          M[2] * v.x + M[6] * v.y + M[10] * v.z + M[14] * v.w, M[3] * v.x + M[7] * v.y + M[11] * v.z + M[15] * v.w};
}

enum { TRIPOD_P = 0, TRIPOD_W = 1, TRIPOD_U = 2 };                                     // the three branches, in `lengths`' order
enum { TRIPOD_PASSES = RULE_PASSES, TRIPOD_VISITS = RULE_VISITS, TRIPOD_ITERATIONS = RULE_ITERATIONS, TRIPOD_STATUS = RULE_STATUS };  // a candidate's status words

struct TripodSolveArgs {
	const SprCand *cands;    // [gridDim.x]
	int T, P, C, nblk;
	int max_iterations, max_passes;
	double lower, upper, tolerance, lnl_tolerance;
	const uint8_t *tipmask;  // [T][P]
	const double *props;
	const double *model;     // eval [4] | evec [4][4] | ivec [4][4]
	const double *rates, *weights;
	const double *lengths;   // [N]: the engine's
	const double *row_lower; // the walk's (SprWalkArgs)
	const double *fU;        // [gridDim.x][C][nblk * 64][4]
	double *K;               // [gridDim.x][C][4][nblk * 64]
	double *out;             // [gridDim.x][t_p, t_w, t_u, lnl, initial_lnl]
	int32_t *status;         // [gridDim.x][TRIPOD_STATUS]
};

// a thread's own cells of its first pattern (k = threadIdx.x), category 0, formed once per candidate and kept in vector registers,
// so that the kernel's many wave-uniform bases need not stay live in scalar ones: p's and w's lower in the row's scratch (null: a
// tip, whose mask is read instead), pi o U and K
struct TripodCells {
	const double *lower_p, *lower_w, *fU;
	const uint8_t *mask_p, *mask_w;
	double *K;
};
template <typename T>
__device__ __forceinline__ T *tripod_in_vgprs(T *p) {
	asm volatile("" : "+v"(p));
	return p;
}

// K of the visit of branch z at the lengths (ta, tb, tu) of p, w and u, for this thread's patterns.  sh_m [C][2][16]: two matrices per
// category, P(t r_c) of the other two branches in k_batch_matrices' arithmetic -- u: of p and of w; p or w: of u and of the other one --
// from their exponentials sh_x [C][2][4]; sh_v: V | V^-1
__device__ __forceinline__ void tripod_coefficients(const TripodSolveArgs &a, const TripodCells &cells, int z, double ta, double tb, double tu, double *sh_m, double *sh_x,
                                                    const double *sh_v) {
	const int tid = threadIdx.x;
	if (tid < 8 * a.C) {  // e^(lambda_s t r_c) of (category, matrix, eigenvalue)
		const int s = tid & 3, m = (tid >> 2) & 1, c = tid >> 3;
		const double t = m == 0 ? (z == TRIPOD_U ? ta : tu) : (z == TRIPOD_W ? ta : tb);
		sh_x[tid] = exp(a.model[s] * (t * a.rates[c]));
	}
	__syncthreads();
	if (tid < 32 * a.C) {
		const int j = tid & 3, i = (tid >> 2) & 3;
		const double *evec = a.model + 4, *ivec = a.model + 20, *e = sh_x + (tid >> 4) * 4;
		double p = 0.;
		for (int s = 0; s < 4; s++) p += ivec[s * 4 + j] * evec[i * 4 + s] * e[s];
		sh_m[tid] = fabs(p);  // substmodel.c:552
	}
	__syncthreads();
	const size_t Pp = (size_t)a.nblk * WAVE, plane = Pp * 4;
#pragma unroll 1
	for (int k = tid; k < a.P; k += CBOPT_THREADS) {
		const size_t ahead = (size_t)(k - tid);
		const d4 mask_p = mask4(cells.mask_p[ahead]), mask_w = mask4(cells.mask_w[ahead]);
#pragma unroll 1
		for (int c = 0; c < a.C; c++) {
			const size_t at = (size_t)c * plane + ahead * 4;
			const d4 A = cells.lower_p ? load4(cells.lower_p + at) : mask_p, B = cells.lower_w ? load4(cells.lower_w + at) : mask_w;
			const d4 fU = load4(cells.fU + at);
			const double *M0 = sh_m + c * 32, *M1 = M0 + 16;
			d4 f, low;  // what meets the visited branch from above (times pi), and from below
			if (z == TRIPOD_U) f = fU, low = mul4(tripod_matvec(M1, B), tripod_matvec(M0, A));
			else f = mul4(tripod_matvec_t(M0, fU), tripod_matvec(M1, z == TRIPOD_W ? A : B)), low = z == TRIPOD_W ? B : A;
			const d4 q = tripod_matvec(sh_v + 16, low), g = tripod_matvec_t(sh_v, f);  // V^-1 low, V^T f
			const double wc = a.props[c];
			double *Kc = cells.K + (size_t)c * plane + ahead;
			Kc[0] = wc * (g.x * q.x);
			Kc[Pp] = wc * (g.y * q.y);
			Kc[2 * Pp] = wc * (g.z * q.z);
			Kc[3 * Pp] = wc * (g.w * q.w);
		}
	}
	// (the thread that wrote a pattern's K is the one that reads it in cbopt_evaluate: no barrier; sh_m and sh_x are written again
	// only after the barriers of the evaluations in between)
}

// grid (candidates of the chunk), block 256: one candidate's whole rule (three_branch_rule, phyamd_rule.inc: every slot is visited,
// the start is lnl_0 in the length of u as it is given; tripod_coefficients and cbopt_evaluate are expanded once each), every thread
// with the same bits
__global__ __launch_bounds__(CBOPT_THREADS) void k_tripod_solve4(const TripodSolveArgs a) {
	__shared__ double sh_e[3 * 4 * BATCH_MAX_CATEGORIES], sh_w[3 * CBOPT_WAVES], sh_m[2 * 16 * BATCH_MAX_CATEGORIES], sh_x[2 * 4 * BATCH_MAX_CATEGORIES], sh_v[32];
	if (threadIdx.x < 32) sh_v[threadIdx.x] = a.model[4 + threadIdx.x];  // (the first barrier is tripod_coefficients')
	const size_t cand = blockIdx.x;
	const SprCand cd = load_const_record<6>(a.cands, (int)cand);
	CboptSolveArgs ev{};  // what cbopt_evaluate reads
	ev.P = a.P, ev.C = a.C, ev.Pp = a.nblk * WAVE, ev.model = a.model, ev.rates = a.rates, ev.weights = tripod_in_vgprs(a.weights);
	const size_t node_stride = (size_t)a.C * 4 * ev.Pp;
	const double *K = tripod_in_vgprs(a.K + cand * node_stride);
	const int tid = threadIdx.x, k_first = tid < a.P ? tid : 0;  // (a thread without a pattern reads nothing: a valid address all the same)
	const double *row = a.row_lower + (size_t)cd.row * (a.T - 1) * node_stride + (size_t)tid * 4;
	TripodCells cells;
	cells.lower_p = tripod_in_vgprs(cd.p < a.T ? nullptr : row + (size_t)(cd.p - a.T) * node_stride);
	cells.lower_w = tripod_in_vgprs(cd.w < a.T ? nullptr : row + (size_t)(cd.w - a.T) * node_stride);
	cells.mask_p = tripod_in_vgprs(a.tipmask + (size_t)(cd.p < a.T ? cd.p : 0) * a.P + k_first);
	cells.mask_w = tripod_in_vgprs(a.tipmask + (size_t)(cd.w < a.T ? cd.w : 0) * a.P + k_first);
	cells.fU = tripod_in_vgprs(a.fU + cand * node_stride + (size_t)tid * 4);
	cells.K = tripod_in_vgprs(a.K + cand * node_stride + tid);
	double *const out = tripod_in_vgprs(a.out + cand * 5);
	int32_t *const status = tripod_in_vgprs(a.status + cand * TRIPOD_STATUS);
	const double tw = 0.5 * a.lengths[cd.w];
	const bool p_first = cd.p_left != 0;
	three_branch_rule<true>(
	    [&](int z, double ta, double tb, double tu) { tripod_coefficients(a, cells, z, ta, tb, tu, sh_m, sh_x, sh_v); },
	    [&](double t, bool final, double *lnl, double *d1, double *d2, bool *bad) { cbopt_evaluate(ev, K, t, final, sh_e, sh_w, lnl, d1, d2, bad); },
	    // u's left child, its right child, u: p keeps its slot, w has the one s had
	    [p_first](int slot) { return slot == 2 ? TRIPOD_U : (slot == 0) == p_first ? TRIPOD_P : TRIPOD_W; }, 7, a.lengths[cd.p], tw, tw, a.lower, a.upper, a.tolerance,
	    a.max_iterations, a.lnl_tolerance, a.max_passes, out, status);
}

// results [rows][N][5] and counts [rows][N][3] (passes, visits, iterations): a candidate's in its cell, NaN and 0 in every other
// (cand_of [rows][N]: the cell's candidate index, -1: none; k_spr_finish's idiom)
__global__ __launch_bounds__(256) void k_tripod_finish(size_t cells, const int32_t *__restrict__ cand_of, const double *__restrict__ out, const int32_t *__restrict__ status,
                                                      double *__restrict__ results, int32_t *__restrict__ counts) {
	const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (idx >= cells) return;
	const int ci = cand_of[idx];
	for (int j = 0; j < 5; j++) results[idx * 5 + j] = ci >= 0 ? out[(size_t)ci * 5 + j] : NAN;
	for (int j = 0; j < 3; j++) counts[idx * 3 + j] = ci >= 0 ? status[(size_t)ci * TRIPOD_STATUS + j] : 0;
}
