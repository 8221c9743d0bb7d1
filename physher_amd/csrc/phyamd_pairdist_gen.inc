// phyamd_pairdist_gen.inc: 20-state kernels of phyamd_pairwise_distances_general -- the maximum-likelihood distance of pairs of taxa
// under the engine's own model, before any topology exists -- included by phyamd_engine.hip inside its anonymous namespace, behind
// phyamd_pairdist4.inc, whose scheme this is (see its head for the likelihood and the sums over the bins).
//
// A tip cell's CLASS is the code a generic engine stores in d_tipmask: a state 0..19, 20 = unknown, 21 + q = ambiguity set q of
// d_tipsets.  The call refuses engines with more than PAIRDIST_GEN_CLASSES - 21 sets, so every code is below 32 and the sufficient
// statistic is the weighted 32 x 32 table N[ci][cj] = sum_k w_k [class_i[k] = ci][class_j[k] = cj]: four 16 x 16 tiles of
// A^T diag(w) B, by the low and the high half of each side's classes.  k_classpair_counts forms them over the fixed segments of
// REWEIGHT_SEGMENT patterns; k_pairdist_finish (phyamd_pairdist4.inc) adds a pair's segments in segment order, a table being four of
// its 256-bin records; k_classpair_solve runs a pair's whole safeguarded Newton iteration in one workgroup, a thread owning four
// bins.  No floating-point atomics: a pair's bits depend on its two rows of codes, the weights, the sets and the model only.
// (The two kernels are named k_classpair_*, not k_pairdist_*: tests/test_pair_distance_abi.py counts the kernels whose names hold
// "k_pairdist" and expects the 4-state call's three.)

constexpr int PAIRDIST_GEN_CLASSES = 32, PAIRDIST_GEN_BINS = PAIRDIST_GEN_CLASSES * PAIRDIST_GEN_CLASSES, PAIRDIST_GEN_STATES = 20;

// partners j a wave runs against one taxon i's operands, four accumulators of 8 VGPRs each.  Not measured yet
// (profiles/pair_distance_general_timing.py times the whole call at 200 taxa x 50 000 patterns): 4 partners hold 128 accumulator
// VGPRs, and the kernel is built without spills or scratch memory at this count.  A run shorter than this still issues every
// partner's instructions
constexpr int PAIRDIST_GEN_PARTNERS = 4;

// One segment of the tables of up to PAIRDIST_GEN_PARTNERS pairs that share taxon i: grid (groups, segments), one wave; the
// arguments and the reads of k_pairdist_counts4, with part [segments][pairs][1024].  Lane l holds class values v = l & 15 and
// v + 16 in both operands -- A = w if taxon i's code is that value, else 0; B = 1 if the partner's is, else 0 -- and each step of
// four patterns issues four instructions per partner: tile 2 hi + hj takes A of half hi and B of half hj.  A code of 32 or more
// (the bytes behind the last row) meets no lane and enters with weight 0 anyway.  Register reg of lane l of tile 2 hi + hj is
// counts[16 hi + (l >> 4) + 4 reg][16 hj + (l & 15)]
__global__ __launch_bounds__(WAVE) void k_classpair_counts(const PairCountArgs a) {
	constexpr int NP = PAIRDIST_GEN_PARTNERS;
	const int lane = threadIdx.x, q = lane >> 4, v = lane & 15, seg = blockIdx.y;
	const int first = a.groups[2 * blockIdx.x], n = a.groups[2 * blockIdx.x + 1];
	const uint8_t *row_i = a.tipmask + (size_t)a.pairs[2 * first] * a.P;
	const uint8_t *row_j[NP];
#pragma unroll
	for (int p = 0; p < NP; p++) row_j[p] = a.tipmask + (size_t)a.pairs[2 * (first + min(p, n - 1)) + 1] * a.P;  // (a partner that does not exist repeats the last and is not written)
	f64x4 acc[NP][4];
#pragma unroll
	for (int p = 0; p < NP; p++)
#pragma unroll
		for (int t = 0; t < 4; t++) acc[p][t] = f64x4{0., 0., 0., 0.};
	const int k0 = seg * REWEIGHT_SEGMENT, k1 = min(k0 + REWEIGHT_SEGMENT, a.P);
	for (int kb = k0; kb < k1; kb += 16) {  // (wave-uniform)
		const int k = kb + 4 * q;
		d4 w;
		uint32_t mi, mj[NP];
		if (kb + 16 <= a.P) {
			w = load4(a.weights + k);
			mi = pairdist_mask_word(row_i, k);
#pragma unroll
			for (int p = 0; p < NP; p++) mj[p] = pairdist_mask_word(row_j[p], k);
		} else {  // the round that holds the last pattern
			w.x = k < a.P ? a.weights[k] : 0.0;
			w.y = k + 1 < a.P ? a.weights[k + 1] : 0.0;
			w.z = k + 2 < a.P ? a.weights[k + 2] : 0.0;
			w.w = k + 3 < a.P ? a.weights[k + 3] : 0.0;
			mi = k < a.P ? pairdist_mask_word(row_i, k) : 0u;
#pragma unroll
			for (int p = 0; p < NP; p++) mj[p] = k < a.P ? pairdist_mask_word(row_j[p], k) : 0u;
		}
		const double ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
		for (int s = 0; s < 4; s++) {
			const int ci = (int)((mi >> (8 * s)) & 255u);
			const double A0 = ci == v ? ws[s] : 0.0, A1 = ci == v + 16 ? ws[s] : 0.0;
#pragma unroll
			for (int p = 0; p < NP; p++) {
				const int cj = (int)((mj[p] >> (8 * s)) & 255u);
				const double B0 = cj == v ? 1.0 : 0.0, B1 = cj == v + 16 ? 1.0 : 0.0;
				acc[p][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(A0, B0, acc[p][0], 0, 0, 0);
				acc[p][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(A0, B1, acc[p][1], 0, 0, 0);
				acc[p][2] = __builtin_amdgcn_mfma_f64_16x16x4f64(A1, B0, acc[p][2], 0, 0, 0);
				acc[p][3] = __builtin_amdgcn_mfma_f64_16x16x4f64(A1, B1, acc[p][3], 0, 0, 0);
			}
		}
	}
#pragma unroll
	for (int p = 0; p < NP; p++) {
		if (p >= n) break;
		double *out = a.part + ((size_t)seg * a.npairs + first + p) * PAIRDIST_GEN_BINS;
#pragma unroll
		for (int t = 0; t < 4; t++)
#pragma unroll
			for (int reg = 0; reg < 4; reg++) out[(16 * (t >> 1) + q + 4 * reg) * PAIRDIST_GEN_CLASSES + 16 * (t & 1) + v] = acc[p][t][reg];
	}
}

constexpr int PAIRDIST_GEN_OWN = PAIRDIST_GEN_BINS / PAIRDIST_THREADS;  // bins a thread owns: b = tid + PAIRDIST_THREADS r
constexpr int PAIRDIST_GEN_ROW = PAIRDIST_GEN_STATES + 1;               // doubles between two classes' rows in LDS (odd: a wave's 32 rows of q meet 32 banks)

struct PairSolveGenArgs {
	PairSolveArgs s;  // counts [pairs][1024]; model eval [20] | evec [20][20] | ivec [20][20]
	const unsigned long long *tipsets;  // [sets]: bit s = state s is a member
	int sets;
};

// lnL (final only), d1 and d2 of the pair at length t, the same bits in every thread: the 60 values S_n[a] once per workgroup, the
// categories in category order; then this thread's bins r = 0..3 with N > 0 in that order, the eigen terms a = 0..19 in that order;
// then pairdist_evaluate's reduction -- wave_sum, the waves in wave order through LDS.  *bad: some bin's F_0 is not in (0, inf)
__device__ __forceinline__ void pairdist_evaluate_gen(const PairSolveArgs &a, const double (&N)[PAIRDIST_GEN_OWN], const double *sh_g, const double *sh_q, double t, bool final,
                                                      double *sh_S, double *sh_w, double *lnl, double *d1, double *d2, bool *bad) {
	constexpr int S = PAIRDIST_GEN_STATES;
	const int tid = threadIdx.x;
	if (tid < S) {  // eigenvalue tid
		const double lam = a.model[tid];
		double s0 = 0.0, s1 = 0.0, s2 = 0.0;
		for (int c = 0; c < a.C; c++) {
			const double r = a.rates[c], x = lam * r, e = a.props[c] * exp(lam * (t * r));
			s0 += e;
			s1 += x * e;
			s2 += x * x * e;
		}
		sh_S[tid] = s0, sh_S[S + tid] = s1, sh_S[2 * S + tid] = s2;
	}
	__syncthreads();
	double s0 = 0.0, s1 = 0.0, s2 = 0.0;
	int wrong = 0;
#pragma unroll
	for (int r = 0; r < PAIRDIST_GEN_OWN; r++) {
		if (!(N[r] > 0.0)) continue;
		const int b = tid + PAIRDIST_THREADS * r;
		const double *g = sh_g + (b >> 5) * PAIRDIST_GEN_ROW, *q = sh_q + (b & 31) * PAIRDIST_GEN_ROW;
		double F0 = 0.0, F1 = 0.0, F2 = 0.0;
#pragma unroll
		for (int i = 0; i < S; i++) {
			const double G = g[i] * q[i];
			F0 += G * sh_S[i], F1 += G * sh_S[S + i], F2 += G * sh_S[2 * S + i];
		}
		const double r1 = F1 / F0, r2 = F2 / F0;
		if (final) s0 += N[r] * log(F0);
		s1 += N[r] * r1;
		s2 += N[r] * (r2 - r1 * r1);
		wrong |= !(F0 > 0.0 && F0 < INFINITY);
	}
	s0 = wave_sum(s0), s1 = wave_sum(s1), s2 = wave_sum(s2);
	const int wave = tid / WAVE;
	if (tid % WAVE == 0) sh_w[wave * 3 + 0] = s0, sh_w[wave * 3 + 1] = s1, sh_w[wave * 3 + 2] = s2;
	*bad = __syncthreads_or(wrong) != 0;  // (also the barrier between the waves' stores and the loads below)
	s0 = s1 = s2 = 0.0;
	for (int v = 0; v < PAIRDIST_WAVES; v++) s0 += sh_w[v * 3 + 0], s1 += sh_w[v * 3 + 1], s2 += sh_w[v * 3 + 2];
	*lnl = s0, *d1 = s1, *d2 = s2;
	__syncthreads();  // sh_S and sh_w are free for the next evaluation
}

// grid (pairs of the chunk), block 256: one pair's whole iteration (the rule of include/physher_amd.h), the iteration and the record
// of k_pairdist_solve4.  The class tables g[c] = V^T (pi o m_c) and q[c] = V^-1 m_c are built once in LDS, m_c the 0/1 vector of
// class c (a state, all states, a set's members; a class no set stands for: zero, and its bins are empty); thread tid owns the bins
// tid + 256 r = 32 ci + cj, r = 0..3
__global__ __launch_bounds__(PAIRDIST_THREADS) void k_classpair_solve(const PairSolveGenArgs ga) {
	constexpr int S = PAIRDIST_GEN_STATES, ROW = PAIRDIST_GEN_ROW;
	__shared__ double sh_g[PAIRDIST_GEN_CLASSES * ROW], sh_q[PAIRDIST_GEN_CLASSES * ROW], sh_S[3 * S], sh_w[3 * PAIRDIST_WAVES];
	const PairSolveArgs &a = ga.s;
	const int pair = blockIdx.x;
	for (int idx = threadIdx.x; idx < PAIRDIST_GEN_CLASSES * S; idx += PAIRDIST_THREADS) {
		const int c = idx / S, i = idx % S;
		const unsigned long long members = c < S ? 1ull << c : c == S ? (1ull << S) - 1 : c - S - 1 < ga.sets ? ga.tipsets[c - S - 1] : 0ull;
		const double *V = a.model + S, *Vi = a.model + S + S * S;
		double g = 0.0, q = 0.0;
		for (int s = 0; s < S; s++)
			if ((members >> s) & 1ull) g += V[s * S + i] * a.freqs[s], q += Vi[i * S + s];
		sh_g[c * ROW + i] = g, sh_q[c * ROW + i] = q;
	}
	double N[PAIRDIST_GEN_OWN];
#pragma unroll
	for (int r = 0; r < PAIRDIST_GEN_OWN; r++) N[r] = a.counts[(size_t)pair * PAIRDIST_GEN_BINS + threadIdx.x + PAIRDIST_THREADS * r];
	__syncthreads();
	solve_one_length(
	    [&](double t, bool final, double *lnl, double *d1, double *d2, bool *bad) { pairdist_evaluate_gen(a, N, sh_g, sh_q, t, final, sh_S, sh_w, lnl, d1, d2, bad); },
	    a.start[pair], a.lower, a.upper, a.tolerance, a.max_iterations, a.out + (size_t)pair * 4, a.iterations + pair);
}
