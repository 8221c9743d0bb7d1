// phyamd_nni4.inc: 4-state kernels of phyamd_nni_log_likelihoods -- lnL and its first two derivatives in the central branch for
// every NNI neighbour of the engine's tree in one call -- included by phyamd_engine.hip inside its anonymous namespace.
//
// A candidate is an internal node v other than the root; u its parent, s its sibling, a / b its left / right child.  The three
// arrangements of the four subtrees around the edge (u, v) differ in four messages only, so nothing is walked per neighbour: ONE
// item goes through the batched walk (k_batch_walk4<false>, phyamd_batch4.inc) with a pre-order op list that parks every internal
// node's upper in a slot of its own (build_batch_ops, park_all), which leaves every internal node's lower p_n and every internal
// non-root node's upper u_n in the batch scratch.  k_nni4 then forms, per (candidate, 64 patterns, category c),
//   m_x = P_x p_x  (x = a, b, s; a tip's p is its mask),   A_u = P_u u_u  (ones when u is the root),
//   k = 0: U = A_u o m_s, p = m_a o m_b     (the engine's tree)
//   k = 1: U = A_u o m_a, p = m_s o m_b     (a and s exchanged)
//   k = 2: U = A_u o m_b, p = m_a o m_s     (b and s exchanged)
//   x = P_v(t_k r_c) p,  y = Q x,  z = Q y,
//   L = sum_c w_c sum_i pi_i U_i x_i,  L' = sum_c w_c r_c sum_i pi_i U_i y_i,  L'' = sum_c w_c r_c^2 sum_i pi_i U_i z_i
// (phyamd_branch_hessian_diagonal's definitions: k_branch_eval4 with the partials of the rearranged tree), and per lane
// w log L, w L'/L, w (L''/L - (L'/L)^2).  P_v(t_k r_c) are the trial matrices [3][N][C][16] k_batch_matrices makes from the trial
// lengths; every other matrix is the walk's item's.  No floating-point atomics: a term is summed over the 64 lanes by wave_sum,
// written to the slab [candidate][block][9], and k_nni_finish adds the blocks in block order.

// a candidate edge: v, its parent (BATCH_ROOT: the root, whose upper is ones), its sibling and its two children
struct NniCand {
	int32_t v, u, s, a, b;
	int32_t pad[3];
};

__device__ __forceinline__ NniCand load_nni_cand(const NniCand *cands, int i) { return load_const_record<5>(cands, i); }

struct NniArgs {
	const NniCand *cands;    // [gridDim.y]
	int T, N, P, C, nblk;
	int deriv;               // 0: lnL only (the y, z work is skipped; the lnL instructions are the same)
	const uint8_t *tipmask;  // [T][P]
	const double *freqs, *props, *rates, *weights, *Q;
	const double *mats;      // [N][C][16]: the engine's lengths (the walk's item)
	const double *trial;     // [3][N][C][16]: the trial lengths
	const double *lower;     // [T - 1][C][nblk * 64][4]: p_n of internal node n at n - T
	const double *upper;     // [T - 1][C][nblk * 64][4]: u_n of internal non-root node n at n - T
	double *slab;            // [gridDim.y][nblk][9]: per arrangement k the block's sums of w log L, w L'/L, w (L''/L - (L'/L)^2)
};

// grid (nblk, candidates), block (64, C): the C category waves of 64 patterns of one edge (k_batch_walk4's shape)
__global__ __launch_bounds__(BATCH_MAX_CATEGORIES *WAVE) void k_nni4(const NniArgs a) {
	__shared__ double sh[9 * BATCH_MAX_CATEGORIES * WAVE];  // [3 k + term][C][64]
	const int lane = threadIdx.x, c = __builtin_amdgcn_readfirstlane(threadIdx.y);  // this wave's category
	const int blk = blockIdx.x;
	const NniCand cd = load_nni_cand(a.cands, blockIdx.y);
	const int k0 = blk * WAVE + lane;  // the scratch is padded to whole blocks and the walk has written every lane's cells
	const bool valid = k0 < a.P;
	const int k = valid ? k0 : a.P - 1;
	const size_t plane = (size_t)a.nblk * WAVE * 4, node_stride = (size_t)a.C * plane;
	const cptr mats_c = as_const(a.mats + (size_t)c * 16);
	const double *lower_c = a.lower + (size_t)c * plane + (size_t)k0 * 4, *upper_c = a.upper + (size_t)c * plane + (size_t)k0 * 4;
	const auto message = [&](int child) {  // P_child . mask for a tip, P_child . p_child for an internal node
		const cptr M = opaque(mats_c + (size_t)child * a.C * 16);
		if (child < a.T) return matvec4(M, mask4(a.tipmask[(size_t)child * a.P + k]));
		return matvec4(M, load4(lower_c + (size_t)(child - a.T) * node_stride));
	};
	const d4 ma = message(cd.a), mb = message(cd.b), ms = message(cd.s);
	d4 Au = d4{1., 1., 1., 1.};
	if (cd.u != BATCH_ROOT) Au = matvec4(opaque(mats_c + (size_t)cd.u * a.C * 16), load4(upper_c + (size_t)(cd.u - a.T) * node_stride));
	const d4 f = mul4(d4{a.freqs[0], a.freqs[1], a.freqs[2], a.freqs[3]}, Au);  // pi o A_u
	const double wc = a.props[c], rc = a.rates[c];
	const cptr Q = as_const(a.Q);
#pragma unroll
	for (int arr = 0; arr < 3; arr++) {
		const d4 fU = mul4(f, arr == 0 ? ms : arr == 1 ? ma : mb);
		const d4 p = arr == 0 ? mul4(ma, mb) : arr == 1 ? mul4(ms, mb) : mul4(ma, ms);
		const d4 x = matvec4(opaque(as_const(a.trial + (((size_t)arr * a.N + cd.v) * a.C + c) * 16)), p);
		sh[((3 * arr + 0) * a.C + c) * WAVE + lane] = wc * dot4(fU, x);
		if (a.deriv) {
			const d4 y = matvec4(opaque(Q), x), z = matvec4(opaque(Q), y);
			sh[((3 * arr + 1) * a.C + c) * WAVE + lane] = wc * rc * dot4(fU, y);
			sh[((3 * arr + 2) * a.C + c) * WAVE + lane] = wc * rc * rc * dot4(fU, z);
		}
	}
	__syncthreads();  // the one meeting of the categories
	const double w = valid ? a.weights[k] : 0.0;
	double *slab = a.slab + ((size_t)blockIdx.y * a.nblk + blk) * 9;
	for (int arr = c; arr < 3; arr += a.C) {  // the arrangements go round the category waves; each is summed in category order
		double L = 0.0, L1 = 0.0, L2 = 0.0;
		for (int cc = 0; cc < a.C; cc++) L += sh[((3 * arr + 0) * a.C + cc) * WAVE + lane];
		const double s0 = wave_sum(valid ? w * log(L) : 0.0);
		double s1 = 0.0, s2 = 0.0;
		if (a.deriv) {
			for (int cc = 0; cc < a.C; cc++) {
				L1 += sh[((3 * arr + 1) * a.C + cc) * WAVE + lane];
				L2 += sh[((3 * arr + 2) * a.C + cc) * WAVE + lane];
			}
			const double r1 = L1 / L, r2 = L2 / L;
			s1 = wave_sum(valid ? w * r1 : 0.0);
			s2 = wave_sum(valid ? w * (r2 - r1 * r1) : 0.0);
		}
		if (lane == 0) {
			slab[3 * arr + 0] = s0;
			slab[3 * arr + 1] = s1;
			slab[3 * arr + 2] = s2;
		}
	}
}

// out [3 terms][3 k][N] = lnl | d1 | d2, each [3][N]: a candidate's blocks added in block order, NaN in the columns of tips and
// of the root (cand_of[node]: the node's candidate index, -1: none)
__global__ __launch_bounds__(256) void k_nni_finish(int N, int nblk, const int32_t *__restrict__ cand_of, const double *__restrict__ slab,
                                                   double *__restrict__ out) {
	const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (idx >= (size_t)9 * N) return;
	const int node = (int)(idx % N), arr = (int)(idx / N) % 3, term = (int)(idx / N) / 3;
	const int ci = cand_of[node];
	double s = NAN;
	if (ci >= 0) {
		s = 0.0;
		for (int b = 0; b < nblk; b++) s += slab[((size_t)ci * nblk + b) * 9 + 3 * arr + term];
	}
	out[idx] = s;
}
