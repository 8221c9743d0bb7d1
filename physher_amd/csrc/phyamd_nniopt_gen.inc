// phyamd_nniopt_gen.inc: 20-state kernels of phyamd_nni_optimize_general -- for every NNI neighbour of the engine's tree the central
// branch length that maximises its lnL, with lnL, d1 and d2 there -- included by phyamd_engine.hip inside its anonymous namespace,
// behind phyamd_nni_gen.inc (whose candidates, messages and products these are) and phyamd_qopt_gen.inc (whose evaluation of an
// exponential sum over 20 eigen terms this is: classopt_evaluate).  The rule is phyamd_rule.inc's solve_one_length.
//
// The coefficients K[c][e] = w_c (V^T F)_e (V^-1 p)_e of an entry (phyamd_nni_gen.inc) do not depend on the central length, so they
// are formed ONCE per entry and the whole iteration reads them: k_classcb_coeff is k_classnni up to its seven products per
// (candidate, category, 16-pattern tile) and stores K where k_classnni meets it with the exponentials; k_classcb_solve runs one
// entry's safeguarded Newton iteration in one workgroup, per step C x 20 exponentials per workgroup and 3 x 20 C FMAs per pattern:
// no walk, no launch, no host round trip.  K lies in the batch scratch as [entry][C][20][Pp], the partials' plane layout: lane
// (row quarter rq, pattern) of a tile holds the eigen terms 4 ks + rq, ks = 0..4, so each store and each load is a run of 16
// consecutive patterns.  No atomics: the sums go per lane in category order, the four lanes of a pattern by lanes_sum16, the tiles
// of a wave in tile order, wave_sum, and the waves in wave order through LDS, so every thread holds the same bits, takes the same
// accept, bisect and stop decisions, and an entry's bits depend on the engine's inputs and its own start alone.
// (The kernels are named k_classcb_*, not k_cbopt_*, k_classnni_* or k_classopt_*: the resource tests of those calls count kernels by
// these substrings and expect their own.  k_classcb_coeff is k_classnni's SIBLING, not a caller of a shared function: with the
// messages and products in one inlined function k_classnni kept its bits but took other registers and ran 4 % slower at 50 000
// patterns, so it stays as it is and the category body below repeats its.)

struct ClassCbCoeffArgs {
	const ClassNniCand *cands;  // [gridDim.y]: the chunk's candidates
	int P, Pp, C, fold;
	const uint8_t *tipcode;     // [T][P]
	const unsigned long long *tipsets;  // the engine's sets
	const double *freqs, *props;
	const double *imgs;         // [N][C][MatImage<2, 5>::SIZE]: the engine's images of P(t_n r_c)
	const double *eig;          // images of V^T and of V^-1
	double *K;                  // [gridDim.y][3][C][20][Pp]
};

// grid (Ppad / CLASSNNI_BLOCK, candidates of the chunk), block 8 waves: a wave owns the 16-pattern tile blockIdx.x * 8 + wave of one
// candidate and writes its three entries' K.  No exponential and no reduction
__global__ __launch_bounds__(GenGeo<2>::WAVES * 64) void k_classcb_coeff(const ClassCbCoeffArgs a) {
	constexpr int RT = 2, KT = 5, S = PLACE_GEN_STATES, WV = GenGeo<RT>::WAVES;
	using Img = MatImage<RT, KT>;
	__shared__ double sh[6 * Img::SIZE];
	double *imgVT = sh, *imgVi = sh + Img::SIZE, *imgU = sh + 2 * Img::SIZE, *imgA = sh + 3 * Img::SIZE, *imgB = sh + 4 * Img::SIZE, *imgS = sh + 5 * Img::SIZE;
	const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const ClassNniCand cd = a.cands[blockIdx.y];
	stage_image<RT, KT>(imgVT, a.eig);
	stage_image<RT, KT>(imgVi, a.eig + Img::SIZE);
	const int pat = (blockIdx.x * WV + wave) * 16 + (lane & 15);
	const size_t Pp = (size_t)a.Pp;
	const TileAddr<RT, KT> ta(pat, a.P, (unsigned)a.Pp);  // (a pattern past the last reads pattern 0 and stores nothing)
	const int code_a = !cd.la && ta.ok ? a.tipcode[(size_t)cd.a * a.P + pat] : S;
	const int code_b = !cd.lb && ta.ok ? a.tipcode[(size_t)cd.b * a.P + pat] : S;
	const int code_s = !cd.ls && ta.ok ? a.tipcode[(size_t)cd.s * a.P + pat] : S;
	f64x4 fpi[RT];
	load_state_weights<RT>(a.freqs, S, cd.up && a.fold != 0, fpi);  // pi, or ones when u's upper carries it
	double *const Kcand = a.K + (size_t)blockIdx.y * 3 * a.C * S * Pp;
#pragma unroll 1
	for (int c = 0; c < a.C; c++) {
		__syncthreads();  // (the previous category's images have been read)
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
			if (ta.ok) {
				double *dst = reinterpret_cast<double *>(reinterpret_cast<char *>(Kcand + ((size_t)k * a.C + c) * S * Pp) + ta.off);  // row (lane >> 4), this pattern
#pragma unroll
				for (int ks = 0; ks < KT; ks++) dst[(size_t)(4 * ks) * Pp] = wc * (g[ks >> 2][ks & 3] * q[ks >> 2][ks & 3]);  // eigen term 4 ks + rq
			}
		}
	}
}

struct ClassCbSolveArgs {
	const ClassNniCand *cands;  // the chunk's candidates: entry i is arrangement i % 3 of candidate i / 3
	int N, P, Pp, C;
	int max_iterations;
	double lower, upper, tolerance;
	const double *model;        // eval [20] | ...
	const double *rates, *weights;
	const double *start;        // [3][N]: the start lengths (the candidates' columns are read)
	const double *K;            // [entries][C][20][Pp]
	double *out;                // [entries][4]: t*, lnL, d1, d2 at t*
	int32_t *iterations;        // [entries]: proposals made, negated where the entry did not converge
};

struct ClassCbShared {
	double e[3 * PLACE_GEN_STATES * BATCH_MAX_CATEGORIES], w[3 * CLASSOPT_WAVES];  // an evaluation's (classopt_evaluate)
};

// grid (entries of the chunk), block 256: one entry's whole iteration (the rule of include/physher_amd.h), every thread with the
// same bits
__global__ __launch_bounds__(CLASSOPT_THREADS) void k_classcb_solve(const ClassCbSolveArgs a) {
	__shared__ ClassCbShared sh;
	const size_t entry = blockIdx.x;
	const int arr = (int)(entry % 3);
	const int v = a.cands[entry / 3].v;
	const double *K = a.K + entry * (size_t)a.C * PLACE_GEN_STATES * a.Pp;
	solve_one_length([&](double t, bool final, double *lnl, double *d1, double *d2, bool *bad) { classopt_evaluate(a, K, t, final, sh, lnl, d1, d2, bad); },
	                 a.start[(size_t)arr * a.N + v], a.lower, a.upper, a.tolerance, a.max_iterations, a.out + entry * 4, a.iterations + entry);
}
