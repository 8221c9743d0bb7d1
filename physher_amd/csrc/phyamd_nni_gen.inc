// phyamd_nni_gen.inc: 20-state kernel of phyamd_nni_log_likelihoods_general -- lnL and its first two derivatives in the central branch
// for every NNI neighbour of the engine's tree in one call -- included by phyamd_engine.hip inside its anonymous namespace, behind
// phyamd_nni4.inc (whose definition, candidates, slab and finish these are) and phyamd_place_gen.inc (whose resident partials it reads).
//
// A candidate is an internal node v other than the root; u its parent, s its sibling, a / b its left / right child.  The three
// arrangements round the edge (u, v) differ in four messages only, and a keep-partials gradient leaves all four resident: a stored
// lower is the message m_x = P_x p_x itself (a tip: tip_matvec of its branch's image with its code over the engine's sets), and
// A_u = P_u u_u with u_u the upper at the top of u's branch (d_upper; ones when u is the root).  Nothing is walked.  Per arrangement
//   k = 0: F = pi o A_u o m_s, p = m_a o m_b     (the engine's tree)
//   k = 1: F = pi o A_u o m_a, p = m_s o m_b     (a and s exchanged)
//   k = 2: F = pi o A_u o m_b, p = m_a o m_s     (b and s exchanged)
// (uppers that carry pi already -- fold -- are used as they are: pi is left out, as k_classplace_table does; at the root F = pi o m_o
// either way).  In the eigen basis the site likelihood in the central length t is an exponential sum (phyamd_qopt_gen.inc's visit of
// n, with messages in place of the query):
//   K[c][e] = w_c (V^T F)_e (V^-1 p)_e,   L = sum_c sum_e K e^(x t),  L' = sum_c sum_e K x e^(x t),  L'' = sum_c sum_e K x^2 e^(x t),
//   x = lambda_e r_c
// so no trial matrix is formed (P_v(t r_c) enters without the reference's fabs: a rounding difference) and d1, d2 cost no further
// product: seven 20-wide products on v_mfma_f64_16x16x4_f64 per (candidate, category, 16-pattern tile) -- A_u, and V^T F and V^-1 p of
// each arrangement; the D layout of one product is the B layout of the next.  One wave owns a 16-pattern tile of one candidate; the
// eight waves of a workgroup share the LDS images (V^T and V^-1 once, P_u and the tip children's per category from the engine's
// prebuilt images) and the tables e, x e, x^2 e [3 arrangements][C][20] of the candidate's three trial lengths.  The categories run
// in order inside the wave and accumulate per lane -- a lane holds the eigen terms 4 ks + (lane >> 4) of its pattern --, the four
// lanes of a pattern meet once by lanes_sum16, then w log L, w L'/L, w (L''/L - (L'/L)^2) are added over the tile (wave_sum), over the
// waves in wave order and written to the slab [candidate][block][9]; k_nni_finish adds the blocks in block order.  No atomics: an
// entry's bits depend on the engine's inputs and its own trial length alone.
// (The kernel is named k_classnni, not k_nni_*: tests/test_nni_abi.py and its neighbours count the kernels whose names hold "k_nni",
// "k_place", "k_classplace", "k_classopt", ... and expect the existing calls' own.)

constexpr int CLASSNNI_BLOCK = GenGeo<2>::WAVES * 16;  // patterns of a workgroup: a tile per wave

// a candidate edge: the resident upper of u (null: u is the root), the resident lowers of a, b and s (null: a tip, whose codes are
// that row of tipcode), and the nodes
struct ClassNniCand {
	const double *up, *la, *lb, *ls;
	int32_t v, u, a, b, s, pad[3];
};

struct ClassNniArgs {
	const ClassNniCand *cands;  // [gridDim.y]
	int N, P, Pp, C, fold;
	int deriv;                  // 0: lnL only (the sums of L' and L'' are skipped; the lnL instructions are the same)
	const uint8_t *tipcode;     // [T][P]
	const unsigned long long *tipsets;  // the engine's sets
	const double *freqs, *props, *rates, *weights;
	const double *eval;         // [20] eigenvalues
	const double *imgs;         // [N][C][MatImage<2, 5>::SIZE]: the engine's images of P(t_n r_c)
	const double *eig;          // images of V^T and of V^-1
	const double *trial;        // [3][N]: the trial lengths
	double *slab;               // [gridDim.y][gridDim.x][9]: per arrangement k the block's sums of w log L, w L'/L, w (L''/L - (L'/L)^2)
};

// m_x of a child in D layout: the stored message as it is, or the tip's column(s) of its branch's image
__device__ __forceinline__ void classnni_message(const double *lower, const double *img, size_t Pp, const TileAddr<2, 5> &ta, int code, const unsigned long long *tipsets,
                                                 f64x4 (&m)[2]) {
	if (lower) {
		double frag[5];
		load_b<2, 5>(lower, Pp, ta, frag);
		b_as_d<2, 5>(frag, m);
	} else
		tip_matvec<2, 5>(img, PLACE_GEN_STATES, code, tipsets, m);
}

// grid (Ppad / CLASSNNI_BLOCK, candidates of the chunk), block 8 waves: a wave owns the 16-pattern tile blockIdx.x * 8 + wave
__global__ __launch_bounds__(GenGeo<2>::WAVES * 64) void k_classnni(const ClassNniArgs a) {
	constexpr int RT = 2, KT = 5, S = PLACE_GEN_STATES, WV = GenGeo<RT>::WAVES, TAB = 3 * BATCH_MAX_CATEGORIES * S;
	using Img = MatImage<RT, KT>;
	__shared__ double sh[6 * Img::SIZE + 3 * TAB + 9 * WV];
	double *imgVT = sh, *imgVi = sh + Img::SIZE, *imgU = sh + 2 * Img::SIZE, *imgA = sh + 3 * Img::SIZE, *imgB = sh + 4 * Img::SIZE, *imgS = sh + 5 * Img::SIZE;
	double *tab = sh + 6 * Img::SIZE;  // [e | x e | x^2 e][k][c][20]
	double *red = tab + 3 * TAB;       // [wave][9]
	const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), rq = lane >> 4;
	const ClassNniCand cd = a.cands[blockIdx.y];
	const int CS = a.C * S;
	stage_image<RT, KT>(imgVT, a.eig);
	stage_image<RT, KT>(imgVi, a.eig + Img::SIZE);
	for (int idx = threadIdx.x; idx < 3 * CS; idx += WV * 64) {  // (arrangement idx / CS, category, eigenvalue)
		const int k = idx / CS, c = (idx % CS) / S;
		const double lam = a.eval[idx % S], r = a.rates[c], t = a.trial[(size_t)k * a.N + cd.v];
		const double x = lam * r, e = exp(lam * (t * r));
		tab[idx] = e;
		tab[TAB + idx] = x * e;
		tab[2 * TAB + idx] = x * x * e;
	}
	const int pat = (blockIdx.x * WV + wave) * 16 + (lane & 15);
	const size_t Pp = (size_t)a.Pp;
	const TileAddr<RT, KT> ta(pat, a.P, (unsigned)a.Pp);  // (a pattern past the last reads pattern 0 and adds 0)
	const int code_a = !cd.la && ta.ok ? a.tipcode[(size_t)cd.a * a.P + pat] : S;
	const int code_b = !cd.lb && ta.ok ? a.tipcode[(size_t)cd.b * a.P + pat] : S;
	const int code_s = !cd.ls && ta.ok ? a.tipcode[(size_t)cd.s * a.P + pat] : S;
	f64x4 fpi[RT];
	load_state_weights<RT>(a.freqs, S, cd.up && a.fold != 0, fpi);  // pi, or ones when u's upper carries it
	double L[3] = {0., 0., 0.}, L1[3] = {0., 0., 0.}, L2[3] = {0., 0., 0.};
#pragma unroll 1
	for (int c = 0; c < a.C; c++) {
		__syncthreads();  // (the previous category's images have been read; the first: the tables are written)
		if (cd.up) stage_image<RT, KT>(imgU, a.imgs + ((size_t)cd.u * a.C + c) * Img::SIZE);
		if (!cd.la) stage_image<RT, KT>(imgA, a.imgs + ((size_t)cd.a * a.C + c) * Img::SIZE);
		if (!cd.lb) stage_image<RT, KT>(imgB, a.imgs + ((size_t)cd.b * a.C + c) * Img::SIZE);
		if (!cd.ls) stage_image<RT, KT>(imgS, a.imgs + ((size_t)cd.s * a.C + c) * Img::SIZE);
		__syncthreads();
		const size_t plane = (size_t)c * S * Pp;
		f64x4 m[3][RT], f[RT];  // m_a, m_b, m_s; pi o A_u
		classnni_message(cd.la ? cd.la + plane : nullptr, imgA, Pp, ta, code_a, a.tipsets, m[0]);
		classnni_message(cd.lb ? cd.lb + plane : nullptr, imgB, Pp, ta, code_b, a.tipsets, m[1]);
		classnni_message(cd.ls ? cd.ls + plane : nullptr, imgS, Pp, ta, code_s, a.tipsets, m[2]);
		if (cd.up) {
			double frag[KT];
			load_b<RT, KT>(cd.up + plane, Pp, ta, frag);
			mfma_matvec<RT, KT>(imgU, frag, f);
#pragma unroll
			for (int t = 0; t < RT; t++) f[t] = f[t] * fpi[t];
		} else {
#pragma unroll
			for (int t = 0; t < RT; t++) f[t] = fpi[t];
		}
		const double wc = a.props[c];
#pragma unroll
		for (int k = 0; k < 3; k++) {
			const int o = k == 0 ? 2 : k == 1 ? 0 : 1, x = k == 1 ? 2 : 0, y = k == 2 ? 2 : 1;  // (o; x, y) = (s; a, b), (a; s, b), (b; a, s)
			f64x4 F[RT], p[RT], g[RT], q[RT];
			double frag[KT];
#pragma unroll
			for (int t = 0; t < RT; t++) F[t] = f[t] * m[o][t], p[t] = m[x][t] * m[y][t];
			d_as_b<RT, KT>(F, frag);
			mfma_matvec<RT, KT>(imgVT, frag, g);
			d_as_b<RT, KT>(p, frag);
			mfma_matvec<RT, KT>(imgVi, frag, q);
			const double *ec = tab + (k * a.C + c) * S + rq;
#pragma unroll
			for (int ks = 0; ks < KT; ks++) {
				const double K = wc * (g[ks >> 2][ks & 3] * q[ks >> 2][ks & 3]);  // eigen term 4 ks + rq
				L[k] = __builtin_fma(K, ec[4 * ks], L[k]);
				if (a.deriv) {
					L1[k] = __builtin_fma(K, ec[TAB + 4 * ks], L1[k]);
					L2[k] = __builtin_fma(K, ec[2 * TAB + 4 * ks], L2[k]);
				}
			}
		}
	}
	const double w = ta.ok ? a.weights[pat] : 0.0;
	const bool counts = ta.ok && rq == 0 && w != 0.0;  // one lane of a pattern's four adds it
#pragma unroll
	for (int k = 0; k < 3; k++) {
		const double Lk = lanes_sum16(L[k]);  // the pattern's 20 terms of every category: the same bits in its four lanes
		const double s0 = wave_sum(counts ? w * log(Lk) : 0.0);
		double s1 = 0.0, s2 = 0.0;
		if (a.deriv) {
			const double r1 = lanes_sum16(L1[k]) / Lk, r2 = lanes_sum16(L2[k]) / Lk;
			s1 = wave_sum(counts ? w * r1 : 0.0);
			s2 = wave_sum(counts ? w * (r2 - r1 * r1) : 0.0);
		}
		if (lane == 0) red[wave * 9 + 3 * k] = s0, red[wave * 9 + 3 * k + 1] = s1, red[wave * 9 + 3 * k + 2] = s2;
	}
	__syncthreads();
	if (threadIdx.x < 9) {
		double s = 0.0;
		for (int v = 0; v < WV; v++) s += red[v * 9 + threadIdx.x];
		a.slab[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 9 + threadIdx.x] = s;
	}
}
