// phyamd_qopt_gen.inc: 20-state kernel of phyamd_placement_optimize_general -- for chosen (query, edge) placements the three branch
// lengths that meet at the insertion point, optimised one at a time, pass after pass -- included by phyamd_engine.hip inside its
// anonymous namespace, behind phyamd_place_gen.inc (whose resident partials, own-partial kernel and class codes it shares) and
// phyamd_qopt4.inc (whose K formulas these are, with 20-vectors in place of 4-vectors).  The rule and its visit loop are
// phyamd_rule.inc's three_branch_rule.
//
// Three messages meet at the new node z and none depends on the three lengths a = t_n (distal), b = t_x (pendant), cz = t_z
// (proximal): A, the 0/1 member vector of the query's class code; B = p_n, the node's own partial (a tip: its code over the ENGINE's
// sets; an internal node: k_classplace_own's temporary); F = pi o u_n, u_n the resident upper partial at the top of n's branch (it
// carries pi already when the gradient folded it in).  In the length of the visited branch the site likelihood is
// sum_c sum_e K[c][e] exp(lambda_e r_c t) with
//   z:  K = w_c (V^T F)_e (V^-1 [(P(a) B) o (P(b) A)])_e
//   n:  K = w_c (V^T [(P(cz)^T F) o (P(b) A)])_e (V^-1 B)_e
//   x:  K = w_c (V^T [(P(cz)^T F) o (P(a) B)])_e (V^-1 A)_e
// One workgroup of four waves runs a candidate's whole rule.  Per visit the categories run in order: the two P(t r_c) =
// |V e^(lambda t r_c) V^-1| the visit needs are formed in LDS from the eigen system (k_transition_matrices' arithmetic) and written
// as MFMA images (stage_matrix's layout; P(cz) transposed), P(b r_c) A is tabulated over the 32 classes, the members added in state
// order, and V^-1 A once per candidate; then a wave takes the 16-pattern tiles wave, wave + 4, ... and forms K with three 20-wide
// products on v_mfma_f64_16x16x4_f64 (mfma_matvec; a tip's B is a column gather, tip_matvec).  K goes to global scratch
// [C][20][Pp] in the partials' plane layout: lane (row quarter rq, pattern) holds the eigen terms 4 ks + rq, ks = 0..4, of its
// pattern, stores them and is the lane that reads them back in every evaluation of the visit, so no barrier stands between the two.
// The evaluation is cbopt_evaluate over 20 eigen terms: e, x e, x^2 e of the C x 20 (category, eigenvalue) pairs once per workgroup
// in LDS; per lane its five terms of every category in category order, the four lanes of a pattern by lanes_sum16; per wave the
// patterns of its tiles in tile order, wave_sum, and the waves in wave order.  Every thread holds the same bits and takes the same
// accept, bisect and stop decisions.  No atomics; a candidate's bits depend on the engine's inputs, its query's codes, the call's
// sets, its edge and its start alone.
// (The kernel is named k_classopt_*, not k_qopt_* or k_classplace_*: tests/test_placement_optimize_abi.py,
// tests/test_placement_abi.py and tests/test_placement_general_resources.py count kernels by those substrings.)

constexpr int CLASSOPT_WAVES = 4, CLASSOPT_THREADS = CLASSOPT_WAVES * WAVE;
constexpr int CLASSOPT_ROW = PLACE_GEN_STATES + 1;  // doubles between two classes' rows of a table in LDS (odd: 16 patterns' rows meet different banks)

// a candidate: the upper partial of its edge, its node's own partial (null: a tip, whose codes are row n of tipcode), the node and
// its query's row among the chunk's code rows
struct ClassOptCand {
	const double *up, *own;
	int32_t n, query;
};

struct ClassOptArgs {
	const ClassOptCand *cands;  // [gridDim.x]
	int P, Pp, C, fold, set_count;
	int branches;               // bit QOPT_*: the branch is visited
	int max_iterations, max_passes;
	double lower, upper, tolerance, lnl_tolerance;
	const uint8_t *tipcode;     // [T][P]
	const unsigned long long *tipsets;  // the ENGINE's sets (the reference tips')
	const unsigned long long *sets;     // the CALL's sets (the queries')
	const uint8_t *codes;       // [queries of the chunk][P]
	const double *freqs, *props;
	const double *model;        // eval [20] | evec [20][20] | ivec [20][20]
	const double *rates, *weights;
	const double *start;        // [gridDim.x][t_n, t_x, t_z]
	double *K;                  // [gridDim.x][C][20][Pp]
	double *out;                // [gridDim.x][t_n, t_x, t_z, lnl, initial_lnl]
	int32_t *status;            // [gridDim.x][QOPT_STATUS]
};

// the image of the row-major 20 x 20 matrix M in LDS (TRANSPOSED: of its transpose): stage_matrix's fragments and row sums
template <bool TRANSPOSED>
__device__ __forceinline__ void classopt_image(double *img, const double *M) {
	constexpr int S = PLACE_GEN_STATES, KT = 5, FRAG = MatImage<2, 5>::FRAG;
	for (int idx = threadIdx.x; idx < FRAG; idx += CLASSOPT_THREADS) {
		const int lane = idx & 63, ks = (idx >> 6) % KT, t = (idx >> 6) / KT;
		const int i = t == 1 ? 16 + (lane & 3) : (lane & 15), j = 4 * ks + (lane >> 4);  // (the tail tile: stage_matrix)
		img[idx] = TRANSPOSED ? M[j * S + i] : M[i * S + j];
	}
	for (int i = threadIdx.x; i < 32; i += CLASSOPT_THREADS) {
		double s = 0.0;
		if (i < S && !TRANSPOSED)  // (a transposed image meets no tip: its row sums are not read)
			for (int j = 0; j < S; j++) s += M[i * S + j];
		img[FRAG + i] = s;
	}
}

// table [32][CLASSOPT_ROW]: (M m_k)_i of the 32 classes' member vectors, the members added in state order
__device__ __forceinline__ void classopt_table(double *tab, const double *M, const unsigned long long *members) {
	constexpr int S = PLACE_GEN_STATES;
	for (int idx = threadIdx.x; idx < PLACE_GEN_CLASSES * S; idx += CLASSOPT_THREADS) {
		const int k = idx / S, i = idx % S;
		const unsigned long long m = members[k];
		double s = 0.0;
		for (int j = 0; j < S; j++)
			if ((m >> j) & 1ull) s += M[i * S + j];
		tab[k * CLASSOPT_ROW + i] = s;
	}
}

// row k of a table as a D-layout vector
__device__ __forceinline__ void classopt_lookup(const double *tab, int k, f64x4 (&d)[2]) {
	const double *row = tab + k * CLASSOPT_ROW + ((threadIdx.x & 63) >> 4);
	d[0] = f64x4{row[0], row[4], row[8], row[12]};
	d[1] = f64x4{row[16], 0., 0., 0.};
}

struct ClassOptShared {
	double V[400], Vi[400];                 // the eigenvectors, row-major
	double imgVT[MatImage<2, 5>::SIZE], imgVi[MatImage<2, 5>::SIZE];  // images of V^T and of V^-1
	double imgA[MatImage<2, 5>::SIZE], imgB[MatImage<2, 5>::SIZE];    // a category's: of P(a) (z) or P(cz)^T (n, x); of P(a) (x)
	double Pm[2 * 400];                     // a category's two matrices, row-major
	double x[2 * PLACE_GEN_STATES];         // their exponentials
	double tabA[PLACE_GEN_CLASSES * CLASSOPT_ROW], tabQ[PLACE_GEN_CLASSES * CLASSOPT_ROW];  // P(b r_c) A (z, n) and V^-1 A
	double e[3 * PLACE_GEN_STATES * BATCH_MAX_CATEGORIES], w[3 * CLASSOPT_WAVES];           // an evaluation's
	unsigned long long members[PLACE_GEN_CLASSES];
};

// K of the visit of branch z at the lengths (tn, tx, tz), for the patterns of this wave's tiles
__device__ __forceinline__ void classopt_coefficients(const ClassOptArgs &a, const ClassOptCand &cd, double *Kcand, int z, double tn, double tx, double tz, ClassOptShared &sh) {
	constexpr int S = PLACE_GEN_STATES, RT = 2, KT = 5;
	const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
	const size_t Pp = (size_t)a.Pp;
	const int tiles = a.Pp / 16;
	const double t0 = z == QOPT_Z ? tn : tz, t1 = z == QOPT_X ? tn : tx;  // the two matrices' lengths: z: a, b; n: cz, b; x: cz, a
	f64x4 fpi[RT];
	load_state_weights<RT>(a.freqs, S, a.fold != 0, fpi);  // pi, or ones when the uppers carry it
#pragma unroll 1
	for (int c = 0; c < a.C; c++) {
		__syncthreads();  // (the previous category's images and table have been read; so have the previous evaluation's sums)
		if (tid < 2 * S) sh.x[tid] = exp(a.model[tid % S] * ((tid < S ? t0 : t1) * a.rates[c]));
		__syncthreads();
		for (int idx = tid; idx < 2 * S * S; idx += CLASSOPT_THREADS) {
			const int m = idx / (S * S), i = (idx / S) % S, j = idx % S;
			const double *ex = sh.x + m * S;
			double p = 0.0;
			for (int s = 0; s < S; s++) p += sh.Vi[s * S + j] * sh.V[i * S + s] * ex[s];
			sh.Pm[idx] = fabs(p);  // substmodel.c:552
		}
		__syncthreads();
		if (z == QOPT_Z) classopt_image<false>(sh.imgA, sh.Pm);
		else classopt_image<true>(sh.imgA, sh.Pm);
		if (z == QOPT_X) classopt_image<false>(sh.imgB, sh.Pm + S * S);
		else classopt_table(sh.tabA, sh.Pm + S * S, sh.members);
		__syncthreads();
		const double wc = a.props[c];
		const double *up = cd.up + (size_t)c * S * Pp, *own = cd.own ? cd.own + (size_t)c * S * Pp : nullptr;
		double *Kc = Kcand + (size_t)c * S * Pp;
#pragma unroll 1
		for (int tile = wave; tile < tiles; tile += CLASSOPT_WAVES) {
			const int pat = tile * 16 + (lane & 15);
			const TileAddr<RT, KT> ta(pat, a.P, (unsigned)a.Pp);  // (a pattern past the last reads pattern 0 and stores nothing)
			const int kx = ta.ok ? a.codes[(size_t)cd.query * a.P + pat] : S;
			const int kn = !own && ta.ok ? a.tipcode[(size_t)cd.n * a.P + pat] : S;
			double frag[KT];
			f64x4 f[RT], g[RT], q[RT], v[RT];
			load_b<RT, KT>(up, Pp, ta, frag);
			b_as_d<RT, KT>(frag, f);
#pragma unroll
			for (int t = 0; t < RT; t++) f[t] = f[t] * fpi[t];
			d_as_b<RT, KT>(f, frag);  // F = pi o u_n
			if (z == QOPT_Z) {
				mfma_matvec<RT, KT>(sh.imgVT, frag, g);
				if (own) {
					load_b<RT, KT>(own, Pp, ta, frag);
					mfma_matvec<RT, KT>(sh.imgA, frag, v);
				} else
					tip_matvec<RT, KT>(sh.imgA, S, kn, a.tipsets, v);
				classopt_lookup(sh.tabA, kx, q);
#pragma unroll
				for (int t = 0; t < RT; t++) v[t] = v[t] * q[t];
				d_as_b<RT, KT>(v, frag);
				mfma_matvec<RT, KT>(sh.imgVi, frag, q);
			} else {
				mfma_matvec<RT, KT>(sh.imgA, frag, f);  // P(cz)^T F
				if (z == QOPT_N) classopt_lookup(sh.tabA, kx, v);
				else if (own) {
					load_b<RT, KT>(own, Pp, ta, frag);
					mfma_matvec<RT, KT>(sh.imgB, frag, v);
				} else
					tip_matvec<RT, KT>(sh.imgB, S, kn, a.tipsets, v);
#pragma unroll
				for (int t = 0; t < RT; t++) f[t] = f[t] * v[t];
				d_as_b<RT, KT>(f, frag);
				mfma_matvec<RT, KT>(sh.imgVT, frag, g);
				if (z == QOPT_X) classopt_lookup(sh.tabQ, kx, q);
				else if (own) {
					load_b<RT, KT>(own, Pp, ta, frag);
					mfma_matvec<RT, KT>(sh.imgVi, frag, q);
				} else
					tip_matvec<RT, KT>(sh.imgVi, S, kn, a.tipsets, q);
			}
			if (ta.ok) {
				double *dst = reinterpret_cast<double *>(reinterpret_cast<char *>(Kc) + ta.off);  // row (lane >> 4), this pattern
#pragma unroll
				for (int ks = 0; ks < KT; ks++) dst[(size_t)(4 * ks) * Pp] = wc * (g[ks >> 2][ks & 3] * q[ks >> 2][ks & 3]);
			}
		}
	}
	// (the lane that wrote a pattern's K is the one that reads it in classopt_evaluate: no barrier; the LDS arrays are written again
	// only after the barriers of the evaluations in between)
}

// the sums of w log L (final only), w L'/L and w (L''/L - (L'/L)^2) over the patterns at length t, the same bits in every thread;
// *bad: some pattern's L is not in (0, inf), so lnL at t is not finite.  cbopt_evaluate over 20 eigen terms.  Args: P, Pp, C, model
// (its eigenvalues), rates, weights; Shared: e [3 C 20] and w [3 waves] (k_classopt_solve, and k_classcb_solve of phyamd_nniopt_gen.inc)
template <class Args, class Shared>
__device__ __forceinline__ void classopt_evaluate(const Args &a, const double *Kcand, double t, bool final, Shared &sh, double *lnl, double *d1, double *d2, bool *bad) {
	constexpr int S = PLACE_GEN_STATES, KT = 5;
	const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), rq = lane >> 4, CS = a.C * S;
	const size_t Pp = (size_t)a.Pp;
	if (tid < CS) {  // e, x e, x^2 e of (category tid / 20, eigenvalue tid % 20), once per workgroup
		const double lam = a.model[tid % S], r = a.rates[tid / S], x = lam * r, e = exp(lam * (t * r));
		sh.e[tid] = e;
		sh.e[CS + tid] = x * e;
		sh.e[2 * CS + tid] = x * x * e;
	}
	__syncthreads();
	double s0 = 0.0, s1 = 0.0, s2 = 0.0;
	int wrong = 0;
	const int tiles = a.Pp / 16;
#pragma unroll 1
	for (int tile = wave; tile < tiles; tile += CLASSOPT_WAVES) {
		const int pat = tile * 16 + (lane & 15);
		const bool ok = pat < a.P;
		const double *src = Kcand + (size_t)rq * Pp + (ok ? pat : 0);
		double L = 0.0, L1 = 0.0, L2 = 0.0;
#pragma unroll 1
		for (int c = 0; c < a.C; c++) {
			const double *Kc = src + (size_t)c * S * Pp, *ec = sh.e + c * S + rq;
#pragma unroll
			for (int ks = 0; ks < KT; ks++) {
				const double Kv = ok ? Kc[(size_t)(4 * ks) * Pp] : 0.0;
				L += Kv * ec[4 * ks];
				L1 += Kv * ec[CS + 4 * ks];
				L2 += Kv * ec[2 * CS + 4 * ks];
			}
		}
		L = lanes_sum16(L), L1 = lanes_sum16(L1), L2 = lanes_sum16(L2);  // the pattern's 20 terms: the same bits in its four lanes
		if (ok && rq == 0) {
			const double w = a.weights[pat], r1 = L1 / L, r2 = L2 / L;
			if (final) s0 += w * log(L);
			s1 += w * r1;
			s2 += w * (r2 - r1 * r1);
			wrong |= !(L > 0.0 && L < INFINITY);
		}
	}
	s0 = wave_sum(s0), s1 = wave_sum(s1), s2 = wave_sum(s2);
	if (lane == 0) sh.w[wave * 3 + 0] = s0, sh.w[wave * 3 + 1] = s1, sh.w[wave * 3 + 2] = s2;
	*bad = __syncthreads_or(wrong) != 0;  // (also the barrier between the waves' stores and the loads below)
	s0 = s1 = s2 = 0.0;
	for (int v = 0; v < CLASSOPT_WAVES; v++) s0 += sh.w[v * 3 + 0], s1 += sh.w[v * 3 + 1], s2 += sh.w[v * 3 + 2];
	*lnl = s0, *d1 = s1, *d2 = s2;
	__syncthreads();  // sh.e and sh.w are free for the next evaluation
}

// grid (candidates of the chunk), block 256: one candidate's whole rule (three_branch_rule, phyamd_rule.inc: a slot is its branch),
// every thread with the same bits.  Compiled for two waves per SIMD: left alone the compiler takes 277 registers (255 + 22 accumulation), one workgroup per
// CU; bounded it takes 165, nothing spills, and three workgroups share a CU and its 160 KB of LDS
__global__ __launch_bounds__(CLASSOPT_THREADS, 2) void k_classopt_solve(const ClassOptArgs a) {
	constexpr int S = PLACE_GEN_STATES;
	__shared__ ClassOptShared sh;
	const int tid = threadIdx.x;
	for (int idx = tid; idx < S * S; idx += CLASSOPT_THREADS) sh.V[idx] = a.model[S + idx], sh.Vi[idx] = a.model[S + S * S + idx];
	if (tid < PLACE_GEN_CLASSES)  // a class's members: a state, all states, a set of the call; a class no set stands for: none
		sh.members[tid] = tid < S ? 1ull << tid : tid == S ? (1ull << S) - 1 : tid - S - 1 < a.set_count ? a.sets[tid - S - 1] : 0ull;
	__syncthreads();
	classopt_image<true>(sh.imgVT, sh.V);
	classopt_image<false>(sh.imgVi, sh.Vi);
	classopt_table(sh.tabQ, sh.Vi, sh.members);  // (the first barrier after these is classopt_coefficients')
	const size_t cand = blockIdx.x;
	const ClassOptCand cd = a.cands[cand];
	double *const Kcand = a.K + cand * (size_t)a.C * S * a.Pp;
	three_branch_rule<false>(
	    [&](int z, double tn, double tx, double tz) { classopt_coefficients(a, cd, Kcand, z, tn, tx, tz, sh); },
	    [&](double t, bool final, double *lnl, double *d1, double *d2, bool *bad) { classopt_evaluate(a, Kcand, t, final, sh, lnl, d1, d2, bad); },
	    [](int slot) { return slot; },  // z's left child n, its right child x, z
	    a.branches, a.start[cand * 3], a.start[cand * 3 + 1], a.start[cand * 3 + 2], a.lower, a.upper, a.tolerance, a.max_iterations, a.lnl_tolerance, a.max_passes,
	    a.out + cand * 5, a.status + cand * QOPT_STATUS);
}
