// phyamd_post.inc -- per-pattern posteriors: the marginal state posterior of a node (phyamd_state_posteriors; asr_marginal /
// _marginal_reconstruction, asr.c:28-134) and the rate-category posterior of a site (phyamd_site_rate_posteriors;
// SingleTreeLikelihood_posterior_sites, ppsites.c:17-43) -- included by phyamd_engine.hip inside its anonymous namespace.
//
// Read-only kernels over the partials a keep-partials gradient leaves resident: the lower and the upper partial that meet on a
// node's branch, in the reference's form (the pair k_branch_eval4 takes).  With p the node's own partial, u its upper partial
// and P_c the matrices of its branch,
//   J[j] = sum_c w_c p[c][j] sum_i pi_i u[c][i] P_c[i][j]      (the root: J[j] = sum_c w_c pi_j p[c][j])
// is the site likelihood with the node held in state j: sum_j J[j] = L_k.  posterior[j] = J[j] / sum_j' J[j'], so a per-pattern
// factor of a rescaled evaluation cancels; state = the smallest j with the largest J (asr.c:73-86: strict >).

// one row of a chunk = one node
struct PostRow {
	const double *low;   // the node's own partial, [C][P][4] or planes [C][S][Pp]; null: a tip
	const uint8_t *tip;  // a tip's row of masks (4 states) or codes [P]
	const double *up;    // its upper partial (unused for the root)
	int32_t node;
	int32_t mat;         // the node whose matrices carry the branch, -1: the root
};

constexpr int POST_MAX_CATEGORIES = MAX_WAVES;  // a workgroup holds the category waves of one block of patterns (phyamd_create admits no more)

// a lane's 32 bytes through a pointer that came out of a row's descriptor: said to be global memory, so that the loads are
// global_load_dwordx4 and not flat ones (a pointer loaded from memory has no address space the compiler could infer)
typedef const __attribute__((address_space(1))) double *gptr;
__device__ __forceinline__ d4 load4_global(const double *p) {
	typedef const __attribute__((address_space(1))) dv2 *gptr2;
	const gptr2 q = (gptr2)(gptr)p;
	const dv2 a = q[0], b = q[1];
	return d4{a.x, a.y, b.x, b.y};
}

// y = M^T v, M row-major 4x4 at a wave-uniform address (scalar loads)
__device__ __forceinline__ d4 matvecT4(cptr M, const d4 &v) {
	d4 r;
	r.x = M[0] * v.x + M[4] * v.y + M[8] * v.z + M[12] * v.w;
	r.y = M[1] * v.x + M[5] * v.y + M[9] * v.z + M[13] * v.w;
	r.z = M[2] * v.x + M[6] * v.y + M[10] * v.z + M[14] * v.w;
	r.w = M[3] * v.x + M[7] * v.y + M[11] * v.z + M[15] * v.w;
	return r;
}

// 4 states.  Grid (blocks of 64 patterns, rows); workgroup = 64 patterns x C category waves of one (row, block), like
// k_branch_eval4.  The row's descriptor and matrix are wave-uniform (scalar loads); a lane loads its own u and p and forms
// w_c p o (P^T (pi o u)); the categories meet once in LDS, wave 0 adds them in category order, normalises and picks the state.
// fold: pi is inside the uppers already (a PHYAMD_GRAD_FOLD_ROOT_FREQS gradient left them).  post [rows][P][4] and states
// [rows][P]: either may be null.
__global__ __launch_bounds__(WAVE * POST_MAX_CATEGORIES) void k_post4(const PostRow *__restrict__ rows, int P, int C, const double *__restrict__ mats,
                                                                      const double *__restrict__ freqs, int fold, const double *__restrict__ props,
                                                                      double *__restrict__ post, uint8_t *__restrict__ states) {
	extern __shared__ double sh[];  // [C][64][4]
	const int lane = threadIdx.x, c = __builtin_amdgcn_readfirstlane(threadIdx.y);
	const int k0 = blockIdx.x * WAVE + lane;
	const bool valid = k0 < P;
	const int k = valid ? k0 : P - 1;
	const size_t plane = (size_t)P * 4;
	// the row's descriptor through the constant address space, field by field: a wave-uniform address, so scalar loads
	const __attribute__((address_space(4))) PostRow *const row = (const __attribute__((address_space(4))) PostRow *)rows + blockIdx.y;
	PostRow r;
	r.low = row->low, r.tip = row->tip, r.up = row->up, r.mat = row->mat;
	const cptr pi = as_const(freqs);
	const d4 f = d4{pi[0], pi[1], pi[2], pi[3]};
	const d4 p = r.low ? load4_global(r.low + (size_t)c * plane + (size_t)k * 4) : mask4(((const __attribute__((address_space(1))) uint8_t *)r.tip)[k]);
	d4 J;
	if (r.mat < 0)
		J = mul4(f, p);
	else {
		const d4 u = load4_global(r.up + (size_t)c * plane + (size_t)k * 4);
		J = mul4(p, matvecT4(as_const(mats + ((size_t)r.mat * C + c) * 16), fold ? u : mul4(f, u)));
	}
	const double w = as_const(props)[c];
	store4(sh + ((size_t)c * WAVE + lane) * 4, d4{w * J.x, w * J.y, w * J.z, w * J.w});
	__syncthreads();
	if (c != 0 || !valid) return;
	d4 s = load4(sh + (size_t)lane * 4);
	for (int cc = 1; cc < C; cc++) {
		const d4 t = load4(sh + ((size_t)cc * WAVE + lane) * 4);
		s = d4{s.x + t.x, s.y + t.y, s.z + t.z, s.w + t.w};
	}
	const size_t cell = (size_t)blockIdx.y * P + k;
	if (post) {
		const double total = (s.x + s.y) + (s.z + s.w);
		store4(post + cell * 4, d4{s.x / total, s.y / total, s.z / total, s.w / total});
	}
	if (states) {
		int best = 0;
		double top = s.x;
		if (s.y > top) top = s.y, best = 1;
		if (s.z > top) top = s.z, best = 2;
		if (s.w > top) best = 3;
		states[cell] = (uint8_t)best;
	}
}

// 20 / 60 / 61 states: one pattern per thread, plain loops, in the style of k_branch_eval_gen -- an analysis asks for its
// ancestral states once, not per iteration, and S^2 C multiply-adds per cell are microseconds at these sizes.  Grid (blocks of
// 256 patterns, rows).  low: p_n itself in planes [C][S][Pp] (the caller forms it: a stored array is P p, true_lower_gen).
// Nothing is kept in a per-thread array: J[j] goes to the output as it is formed and is divided by the total in a second sweep.
__global__ __launch_bounds__(256) void k_post_gen(const PostRow *__restrict__ rows, int P, int Pp, int S, int C, const double *__restrict__ mats,
                                                 const double *__restrict__ freqs, int fold, const double *__restrict__ props,
                                                 const unsigned long long *__restrict__ tipsets, double *__restrict__ post, uint8_t *__restrict__ states) {
	const int k = blockIdx.x * 256 + threadIdx.x;
	if (k >= P) return;
	const PostRow r = rows[blockIdx.y];
	const int code = r.low ? 0 : r.tip[k];
	const size_t cell = (size_t)blockIdx.y * P + k;
	double *out = post ? post + cell * S : nullptr;
	double total = 0.0, top = 0.0;
	int best = 0;
	for (int j = 0; j < S; j++) {
		double Jj = 0.0;
		for (int c = 0; c < C; c++) {
			const double pj = r.low ? r.low[((size_t)c * S + j) * Pp + k] : tip_indicator(code, S, tipsets, j);
			double m = freqs[j];
			if (r.mat >= 0) {
				const double *M = mats + ((size_t)r.mat * C + c) * S * S, *u = r.up + (size_t)c * S * Pp + k;
				m = 0.0;
				for (int i = 0; i < S; i++) m += (fold ? 1.0 : freqs[i]) * u[(size_t)i * Pp] * M[i * S + j];
			}
			Jj += props[c] * pj * m;
		}
		if (j == 0 || Jj > top) top = Jj, best = j;
		total += Jj;
		if (out) out[j] = Jj;
	}
	if (out)
		for (int j = 0; j < S; j++) out[j] = out[j] / total;
	if (states) states[cell] = (uint8_t)best;
}

// sum_i pi_i p_root[c][k][i] through the strides of k_root_invariant_term
__device__ __forceinline__ double root_category_likelihood(const double *__restrict__ p, int S, size_t state_stride, const double *__restrict__ freqs) {
	double s = 0.0;
	for (int i = 0; i < S; i++) s += freqs[i] * p[(size_t)i * state_stride];
	return s;
}

// R[k][c] = w_c sum_i pi_i p_root[c][k][i] / sum_c' (the same), mean[k] = sum_c R[k][c] r_c (ppsites.c:29-39, 100), any state
// count: root is the stored root partial, laid out by cat_stride / pat_stride / state_stride ([C][P][4] or planes [C][S][Pp]).
// The quotient is formed over the categories' own sum, not over exp(lnL_k): identical without rescaling, and the only one of the
// two that is defined with it (the per-pattern factor cancels).  R [P][C]; mean [P] or null
__global__ __launch_bounds__(256) void k_site_rate_post(int P, int S, int C, const double *__restrict__ root, size_t cat_stride, size_t pat_stride,
                                                       size_t state_stride, const double *__restrict__ freqs, const double *__restrict__ props,
                                                       const double *__restrict__ rates, double *__restrict__ R, double *__restrict__ mean) {
	const int k = blockIdx.x * 256 + threadIdx.x;
	if (k >= P) return;
	const double *p = root + (size_t)k * pat_stride;
	double total = 0.0;
	for (int c = 0; c < C; c++) total += props[c] * root_category_likelihood(p + (size_t)c * cat_stride, S, state_stride, freqs);
	double m = 0.0;
	for (int c = 0; c < C; c++) {
		const double q = props[c] * root_category_likelihood(p + (size_t)c * cat_stride, S, state_stride, freqs) / total;
		R[(size_t)k * C + c] = q;
		m += q * rates[c];
	}
	if (mean) mean[k] = m;
}
