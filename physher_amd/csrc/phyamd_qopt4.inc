// phyamd_qopt4.inc: 4-state kernels of phyamd_placement_optimize -- for chosen (query, edge) placements the three branch lengths
// that meet at the insertion point, optimised one at a time, pass after pass -- included by phyamd_engine.hip inside its anonymous
// namespace.
//
// The walk is phyamd_placement_log_likelihoods' (launch_nni_walk: every internal node's lower p_n and every internal non-root
// node's upper u_n of the ENGINE'S tree in the batch scratch): nothing is walked per query.  Per candidate (query x on edge n; u
// n's parent, s its sibling) three messages meet at the new node z, and none of them depends on the three lengths
// a = t_n (distal), b = t_x (pendant), cz = t_z (proximal) being optimised:
//   A = x's mask vector,   B = p_n (a tip: its mask),   U = (u is the root ? 1 : P_u u_u) o P_s p_s   (k_place_table4's)
//   L_c = sum_i pi_i U_i [P(cz) ((P(a) B) o (P(b) A))]_i,      P(t) = V e^(lambda t r_c) V^-1
// In the length of the branch being visited L is k_cbopt_solve4's exponential sum, sum_c sum_e K[c][e] exp(lambda_e r_c t), with
//   z:  K = w_c (V^T (pi o U))_e (V^-1 [(P(a) B) o (P(b) A)])_e
//   n:  K = w_c (V^T [(P(cz)^T (pi o U)) o (P(b) A)])_e (V^-1 B)_e
//   x:  K = w_c (V^T [(P(cz)^T (pi o U)) o (P(a) B)])_e (V^-1 A)_e
// (phyamd_tripod4.inc's, with p = x and w = n; no reversibility is used).  A is one of 16 vectors, so P(b r_c) A and V^-1 A are
// not multiplied out per pattern: a visit of z or n tabulates P(b r_c) A for the 16 masks in LDS ([C][16] 4-vectors, summed in
// state order like the mat-vec they replace), V^-1 A is tabulated once per candidate, and a pattern looks its vector up.
// k_qopt_upper4 writes pi o U once per distinct EDGE of a chunk -- every candidate of the edge reads the same plane -- and
// k_qopt_solve4 runs a candidate's whole rule (include/physher_amd.h; its one body: three_branch_rule, phyamd_rule.inc) in one
// workgroup: per visit two 4x4 matrices per category in LDS, K formed per pattern by the thread that reads it back, then the safeguarded Newton iteration on cbopt_evaluate's
// fixed-order sums, so every thread holds the same bits and takes the same accept, bisect and stop decisions.  No walk, no matrix
// launch and no host round trip per visit; no floating-point atomics.  A candidate's arithmetic depends on the engine's inputs,
// its query's masks, its edge and its start alone: not on the chunk, the order of the candidates or what else the chunk holds.

struct QoptUpperArgs {
	const PlaceEdge *edges;  // [gridDim.y]: the chunk's distinct edges
	int T, N, P, C, nblk;
	const uint8_t *tipmask;  // [T][P]
	const double *freqs;
	const double *mats;      // [N][C][16]: the engine's lengths (the walk's item)
	const double *lower;     // [T - 1][C][nblk * 64][4]: p_n of internal node n at n - T
	const double *upper;     // [T - 1][C][nblk * 64][4]: u_n of internal non-root node n at n - T
	double *fU;              // [gridDim.y][C][nblk * 64][4]: pi o U
};

// grid (nblk, edges of the chunk), block (64, C): the C category waves of 64 patterns of one edge (k_place_table4's shape and U).
// Two tips: both edges hang off the root and the sibling is a tip, so no partial is read
__global__ __launch_bounds__(BATCH_MAX_CATEGORIES *WAVE) void k_qopt_upper4(const QoptUpperArgs a) {
	const int lane = threadIdx.x, c = __builtin_amdgcn_readfirstlane(threadIdx.y);  // this wave's category
	const PlaceEdge ed = load_place_edge(a.edges, blockIdx.y);
	const int k0 = blockIdx.x * WAVE + lane;  // the scratch is padded to whole blocks and the walk has written every lane's cells
	const int k = k0 < a.P ? k0 : a.P - 1;
	const size_t plane = (size_t)a.nblk * WAVE * 4, node_stride = (size_t)a.C * plane;
	const cptr mats_c = as_const(a.mats + (size_t)c * 16);
	const double *lower_c = a.lower + (size_t)c * plane + (size_t)k0 * 4, *upper_c = a.upper + (size_t)c * plane + (size_t)k0 * 4;
	d4 U = child_message4(mats_c + (size_t)ed.s * a.C * 16, a.tipmask + k, a.P, lower_c, node_stride, a.T, ed.s);
	if (ed.u != BATCH_ROOT) U = mul4(matvec4(opaque(mats_c + (size_t)ed.u * a.C * 16), load4(upper_c + (size_t)(ed.u - a.T) * node_stride)), U);
	store4(a.fU + ((size_t)blockIdx.y * a.C + c) * plane + (size_t)k0 * 4, mul4(d4{a.freqs[0], a.freqs[1], a.freqs[2], a.freqs[3]}, U));
}

// a candidate: its edge's node, the edge's index among the chunk's distinct edges, its query's row among the chunk's mask rows
struct QoptCand {
	int32_t n, edge, query;
	int32_t pad[5];
};

enum { QOPT_N = 0, QOPT_X = 1, QOPT_Z = 2 };  // the three branches, in `lengths`' order, the visit order and `branches`' bits
enum { QOPT_PASSES = RULE_PASSES, QOPT_VISITS = RULE_VISITS, QOPT_ITERATIONS = RULE_ITERATIONS, QOPT_STATUS = RULE_STATUS };  // a candidate's status words

struct QoptSolveArgs {
	const QoptCand *cands;   // [gridDim.x]
	int T, P, C, nblk;
	int branches;            // bit QOPT_*: the branch is visited
	int max_iterations, max_passes;
	double lower, upper, tolerance, lnl_tolerance;
	const uint8_t *tipmask;  // [T][P]
	const uint8_t *masks;    // [queries of the chunk][P]
	const double *props;
	const double *model;     // eval [4] | evec [4][4] | ivec [4][4]
	const double *rates, *weights;
	const double *start;     // [gridDim.x][t_n, t_x, t_z]
	const double *lower_all; // the walk's lowers: [T - 1][C][nblk * 64][4]
	const double *fU;        // [edges of the chunk][C][nblk * 64][4]
	double *K;               // [gridDim.x][C][4][nblk * 64]
	double *out;             // [gridDim.x][t_n, t_x, t_z, lnl, initial_lnl]
	int32_t *status;         // [gridDim.x][QOPT_STATUS]
};

// a thread's own cells of its first pattern (k = threadIdx.x), category 0, kept in vector registers (tripod_in_vgprs): n's lower in
// the scratch (null: a tip, whose mask is read instead), pi o U of the edge, K, and the two mask rows
struct QoptCells {
	const double *lower_n, *fU;
	const uint8_t *mask_n, *mask_x;
	double *K;
};

// K of the visit of branch z at the lengths (tn, tx, tz), for this thread's patterns.  sh_m [C][2][16]: two matrices per category,
// P(t r_c) of the other two branches in k_batch_matrices' arithmetic -- z: of x and of n; n: of z and of x; x: of z and of n -- from
// their exponentials sh_x [C][2][4]; sh_t [C][16][4]: x's matrix times the 16 mask vectors (visits of z and n); sh_q [16][4]:
// V^-1 times them; sh_v: V | V^-1
__device__ __forceinline__ void qopt_coefficients(const QoptSolveArgs &a, const QoptCells &cells, int z, double tn, double tx, double tz, double *sh_m, double *sh_x, double *sh_t,
                                                  const double *sh_q, const double *sh_v) {
	const int tid = threadIdx.x;
	if (tid < 8 * a.C) {  // e^(lambda_s t r_c) of (category, matrix, eigenvalue)
		const int s = tid & 3, m = (tid >> 2) & 1, c = tid >> 3;
		const double t = m == 0 ? (z == QOPT_Z ? tx : tz) : (z == QOPT_N ? tx : tn);
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
	if (z != QOPT_X) {  // (P(tx r_c) mask(m))_i, the states of m added in state order
		const int which = z == QOPT_Z ? 0 : 1;
		for (int idx = tid; idx < 64 * a.C; idx += CBOPT_THREADS) {
			const int i = idx & 3, m = (idx >> 2) & 15, c = idx >> 6;
			const double *row = sh_m + c * 32 + which * 16 + i * 4;
			const d4 v = mask4((unsigned)m);
			sh_t[idx] = row[0] * v.x + row[1] * v.y + row[2] * v.z + row[3] * v.w;
		}
		__syncthreads();
	}
	const size_t Pp = (size_t)a.nblk * WAVE, plane = Pp * 4;
#pragma unroll 1
	for (int k = tid; k < a.P; k += CBOPT_THREADS) {
		const size_t ahead = (size_t)(k - tid);
		const d4 mask_n = mask4(cells.mask_n[ahead]);
		const int mx = cells.mask_x[ahead] & 15;
#pragma unroll 1
		for (int c = 0; c < a.C; c++) {
			const size_t at = (size_t)c * plane + ahead * 4;
			const d4 B = cells.lower_n ? load4(cells.lower_n + at) : mask_n;
			const d4 fU = load4(cells.fU + at);
			const double *M0 = sh_m + c * 32, *M1 = M0 + 16, *tab = sh_t + (c * 16 + mx) * 4;
			d4 f, q;  // what meets the visited branch from above (times pi), and V^-1 of what meets it from below
			if (z == QOPT_Z) f = fU, q = tripod_matvec(sh_v + 16, mul4(tripod_matvec(M1, B), d4{tab[0], tab[1], tab[2], tab[3]}));
			else if (z == QOPT_N) f = mul4(tripod_matvec_t(M0, fU), d4{tab[0], tab[1], tab[2], tab[3]}), q = tripod_matvec(sh_v + 16, B);
			else f = mul4(tripod_matvec_t(M0, fU), tripod_matvec(M1, B)), q = d4{sh_q[mx * 4], sh_q[mx * 4 + 1], sh_q[mx * 4 + 2], sh_q[mx * 4 + 3]};
			const d4 g = tripod_matvec_t(sh_v, f);  // V^T f
			const double wc = a.props[c];
			double *Kc = cells.K + (size_t)c * plane + ahead;
			Kc[0] = wc * (g.x * q.x);
			Kc[Pp] = wc * (g.y * q.y);
			Kc[2 * Pp] = wc * (g.z * q.z);
			Kc[3 * Pp] = wc * (g.w * q.w);
		}
	}
	// (the thread that wrote a pattern's K is the one that reads it in cbopt_evaluate: no barrier; sh_m, sh_x and sh_t are written
	// again only after the barriers of the evaluations in between)
}

// grid (candidates of the chunk), block 256: one candidate's whole rule (three_branch_rule, phyamd_rule.inc: a slot is its branch,
// the start is lnl_0 in the length of z as it is given), every thread with the same bits
__global__ __launch_bounds__(CBOPT_THREADS) void k_qopt_solve4(const QoptSolveArgs a) {
	__shared__ double sh_e[3 * 4 * BATCH_MAX_CATEGORIES], sh_w[3 * CBOPT_WAVES], sh_m[2 * 16 * BATCH_MAX_CATEGORIES], sh_x[2 * 4 * BATCH_MAX_CATEGORIES], sh_v[32];
	__shared__ double sh_t[16 * 4 * BATCH_MAX_CATEGORIES], sh_q[16 * 4];
	if (threadIdx.x < 32) sh_v[threadIdx.x] = a.model[4 + threadIdx.x];
	if (threadIdx.x < 64) {  // (V^-1 mask(m))_i; the first barrier is qopt_coefficients'
		const int i = threadIdx.x & 3, m = threadIdx.x >> 2;
		const double *row = a.model + 20 + i * 4;
		const d4 v = mask4((unsigned)m);
		sh_q[threadIdx.x] = row[0] * v.x + row[1] * v.y + row[2] * v.z + row[3] * v.w;
	}
	const size_t cand = blockIdx.x;
	const QoptCand cd = load_const_record<3>(a.cands, (int)cand);
	CboptSolveArgs ev{};  // what cbopt_evaluate reads
	ev.P = a.P, ev.C = a.C, ev.Pp = a.nblk * WAVE, ev.model = a.model, ev.rates = a.rates, ev.weights = tripod_in_vgprs(a.weights);
	const size_t node_stride = (size_t)a.C * 4 * ev.Pp;
	const double *K = tripod_in_vgprs(a.K + cand * node_stride);
	const int tid = threadIdx.x, k_first = tid < a.P ? tid : 0;  // (a thread without a pattern reads nothing: a valid address all the same)
	QoptCells cells;
	cells.lower_n = tripod_in_vgprs(cd.n < a.T ? nullptr : a.lower_all + (size_t)(cd.n - a.T) * node_stride + (size_t)tid * 4);
	cells.mask_n = tripod_in_vgprs(a.tipmask + (size_t)(cd.n < a.T ? cd.n : 0) * a.P + k_first);
	cells.mask_x = tripod_in_vgprs(a.masks + (size_t)cd.query * a.P + k_first);
	cells.fU = tripod_in_vgprs(a.fU + (size_t)cd.edge * node_stride + (size_t)tid * 4);
	cells.K = tripod_in_vgprs(a.K + cand * node_stride + tid);
	double *const out = tripod_in_vgprs(a.out + cand * 5);
	int32_t *const status = tripod_in_vgprs(a.status + cand * QOPT_STATUS);
	three_branch_rule<false>(
	    [&](int z, double tn, double tx, double tz) { qopt_coefficients(a, cells, z, tn, tx, tz, sh_m, sh_x, sh_t, sh_q, sh_v); },
	    [&](double t, bool final, double *lnl, double *d1, double *d2, bool *bad) { cbopt_evaluate(ev, K, t, final, sh_e, sh_w, lnl, d1, d2, bad); },
	    [](int slot) { return slot; },  // z's left child n, its right child x, z
	    a.branches, a.start[cand * 3], a.start[cand * 3 + 1], a.start[cand * 3 + 2], a.lower, a.upper, a.tolerance, a.max_iterations, a.lnl_tolerance, a.max_passes, out, status);
}
