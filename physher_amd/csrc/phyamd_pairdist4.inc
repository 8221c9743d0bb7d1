// phyamd_pairdist4.inc: 4-state kernels of phyamd_pairwise_distances -- the maximum-likelihood distance of pairs of taxa under the
// engine's own model, before any topology exists -- included by phyamd_engine.hip inside its anonymous namespace.
//
// For a pair (i, j) and a length t pattern k has
//   L_k(t) = sum_c w_c sum_a (V^T (pi o m_i))_a (V^-1 m_j)_a exp(lambda_a r_c t)
// with m_i, m_j the two 0/1 state masks: phyamd_nniopt4.inc's exponential sum with two tips as the messages.  L_k depends on k only
// through the pair of 4-bit masks, so the weighted table N[mi][mj] = sum_k w_k [mask_i[k] = mi][mask_j[k] = mj] is a sufficient
// statistic, and with S_n[a](t) = sum_c w_c (lambda_a r_c)^n exp(lambda_a r_c t) and G[mi][mj][a] = (V^T (pi o mi))_a (V^-1 mj)_a
//   F_n[mi][mj] = sum_a G[mi][mj][a] S_n[a],   lnL = sum N log F_0,   d1 = sum N F_1 / F_0,   d2 = sum N (F_2 / F_0 - (F_1 / F_0)^2)
// over the bins with N > 0 -- no pattern axis and no category axis per bin.
// k_pairdist_counts4 forms the tables on the matrix pipe: a pair's table is A^T diag(w) B of two one-hot P x 16 matrices, one
// 16 x 16 tile with the pattern axis as K, cut into segments of REWEIGHT_SEGMENT patterns that depend on the pattern index alone;
// k_pairdist_finish adds a pair's segments in segment order; k_pairdist_solve4 runs a pair's whole safeguarded Newton iteration (the
// rule of phyamd_nni_optimize, include/physher_amd.h) in one workgroup, thread b owning bin b.  No floating-point atomics: a pair's
// bits depend on its two mask rows, the weights and the model only -- not on the other pairs, its position, the groups or the chunks.

// partners j a wave runs against one taxon i's operands, an accumulator of 8 VGPRs each.  Measured on all pairs of 1000 taxa x 100 000
// patterns (profiles/pair_distance_timing.py, whole call): 4 partners 486 ms, 8 partners 430 ms, 16 partners 615 ms (300 VGPRs, and
// the row pointers go to scratch memory).  A run shorter than this still issues every partner's instructions
constexpr int PAIRDIST_PARTNERS = 8;

struct PairCountArgs {
	const int32_t *pairs;    // [pairs][2]: the chunk's pairs (i, j)
	const int32_t *groups;   // [gridDim.x][2]: first pair and pair count (1..PAIRDIST_PARTNERS) of a run of pairs that share i
	const uint8_t *tipmask;  // [T][P], and 8 bytes behind the last row
	const double *weights;   // [P]
	double *part;            // [segments][pairs][256]
	double *counts;          // [pairs][256]
	int P, npairs, segments;
};

// the four mask bytes of patterns k .. k + 3 of a row (k < P: the bytes behind a row's end are the next row's, or the array's slack)
__device__ __forceinline__ uint32_t pairdist_mask_word(const uint8_t *row, int k) {
	uint32_t m;
	__builtin_memcpy(&m, row + k, sizeof(m));
	return m;
}

// One segment of the tables of up to PAIRDIST_PARTNERS pairs that share taxon i: grid (groups, segments), one wave.
// v_mfma_f64_16x16x4_f64 takes A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15] (k_reweight_mfma): lane l holds mask value
// l & 15 in both -- A = w if taxon i's mask is that value, else 0; B = 1 if the partner's is, else 0 -- and reads one dword of four
// mask bytes of each row and four weights per round of 16 patterns, which feed four instructions per partner: in lane group
// q = l >> 4, step s takes pattern k + 4 q + s.  Patterns past P enter with weight 0.  Register reg of lane l is
// D[(l >> 4) + 4 reg][l & 15] = counts[mi][mj]
__global__ __launch_bounds__(WAVE) void k_pairdist_counts4(const PairCountArgs a) {
	const int lane = threadIdx.x, q = lane >> 4, v = lane & 15, seg = blockIdx.y;
	const int first = a.groups[2 * blockIdx.x], n = a.groups[2 * blockIdx.x + 1];
	const uint8_t *row_i = a.tipmask + (size_t)a.pairs[2 * first] * a.P;
	const uint8_t *row_j[PAIRDIST_PARTNERS];
#pragma unroll
	for (int p = 0; p < PAIRDIST_PARTNERS; p++) row_j[p] = a.tipmask + (size_t)a.pairs[2 * (first + min(p, n - 1)) + 1] * a.P;  // (a partner that does not exist repeats the last and is not written)
	f64x4 acc[PAIRDIST_PARTNERS];
#pragma unroll
	for (int p = 0; p < PAIRDIST_PARTNERS; p++) acc[p] = f64x4{0., 0., 0., 0.};
	const int k0 = seg * REWEIGHT_SEGMENT, k1 = min(k0 + REWEIGHT_SEGMENT, a.P);
	for (int kb = k0; kb < k1; kb += 16) {  // (wave-uniform)
		const int k = kb + 4 * q;
		d4 w;
		uint32_t mi, mj[PAIRDIST_PARTNERS];
		if (kb + 16 <= a.P) {
			w = load4(a.weights + k);
			mi = pairdist_mask_word(row_i, k);
#pragma unroll
			for (int p = 0; p < PAIRDIST_PARTNERS; p++) mj[p] = pairdist_mask_word(row_j[p], k);
		} else {  // the round that holds the last pattern
			w.x = k < a.P ? a.weights[k] : 0.0;
			w.y = k + 1 < a.P ? a.weights[k + 1] : 0.0;
			w.z = k + 2 < a.P ? a.weights[k + 2] : 0.0;
			w.w = k + 3 < a.P ? a.weights[k + 3] : 0.0;
			mi = k < a.P ? pairdist_mask_word(row_i, k) : 0u;
#pragma unroll
			for (int p = 0; p < PAIRDIST_PARTNERS; p++) mj[p] = k < a.P ? pairdist_mask_word(row_j[p], k) : 0u;
		}
		const double ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
		for (int s = 0; s < 4; s++) {
			const double A = (int)((mi >> (8 * s)) & 255u) == v ? ws[s] : 0.0;
#pragma unroll
			for (int p = 0; p < PAIRDIST_PARTNERS; p++) {
				const double B = (int)((mj[p] >> (8 * s)) & 255u) == v ? 1.0 : 0.0;
				acc[p] = __builtin_amdgcn_mfma_f64_16x16x4f64(A, B, acc[p], 0, 0, 0);
			}
		}
	}
#pragma unroll
	for (int p = 0; p < PAIRDIST_PARTNERS; p++) {
		if (p >= n) break;
		double *out = a.part + ((size_t)seg * a.npairs + first + p) * 256 + q * 16 + v;
#pragma unroll
		for (int reg = 0; reg < 4; reg++) out[reg * 64] = acc[p][reg];
	}
}

// counts[pair][bin]: a pair's segments added in segment order; one thread per (pair, bin)
__global__ __launch_bounds__(256) void k_pairdist_finish(const PairCountArgs a) {
	const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x, total = (size_t)a.npairs * 256;
	if (idx >= total) return;
	double s = 0.0;
	for (int seg = 0; seg < a.segments; seg++) s += a.part[(size_t)seg * total + idx];
	a.counts[idx] = s;
}

constexpr int PAIRDIST_THREADS = 256, PAIRDIST_WAVES = PAIRDIST_THREADS / WAVE;

struct PairSolveArgs {
	const double *counts;  // [pairs][256]
	const double *start;   // [pairs]
	int C, max_iterations;
	double lower, upper, tolerance;
	const double *model;   // eval [4] | evec [4][4] | ivec [4][4]
	const double *freqs, *rates, *props;
	double *out;           // [pairs][4]: t*, lnL, d1, d2 at t*
	int32_t *iterations;   // [pairs]: proposals made, negated where the pair did not converge
};

// lnL (final only), d1 and d2 of the pair at length t, the same bits in every thread: the 12 values S_n[a] once per workgroup, this
// thread's bin (count N, coefficients G) with 12 FMAs and two divisions, then cbopt_evaluate's reduction -- wave_sum, the waves in
// wave order through LDS.  *bad: some bin's F_0 is not in (0, inf), so lnL at t is not finite
__device__ __forceinline__ void pairdist_evaluate(const PairSolveArgs &a, double N, const double (&G)[4], double t, bool final, double *sh_S, double *sh_w, double *lnl,
                                                  double *d1, double *d2, bool *bad) {
	const int tid = threadIdx.x;
	if (tid < 4) {  // eigenvalue tid: the categories in category order
		const double lam = a.model[tid];
		double s0 = 0.0, s1 = 0.0, s2 = 0.0;
		for (int c = 0; c < a.C; c++) {
			const double r = a.rates[c], x = lam * r, e = a.props[c] * exp(lam * (t * r));
			s0 += e;
			s1 += x * e;
			s2 += x * x * e;
		}
		sh_S[tid] = s0, sh_S[4 + tid] = s1, sh_S[8 + tid] = s2;
	}
	__syncthreads();
	double s0 = 0.0, s1 = 0.0, s2 = 0.0;
	int wrong = 0;
	if (N > 0.0) {
		double F0 = 0.0, F1 = 0.0, F2 = 0.0;
#pragma unroll
		for (int i = 0; i < 4; i++) F0 += G[i] * sh_S[i], F1 += G[i] * sh_S[4 + i], F2 += G[i] * sh_S[8 + i];
		const double r1 = F1 / F0, r2 = F2 / F0;
		if (final) s0 = N * log(F0);
		s1 = N * r1;
		s2 = N * (r2 - r1 * r1);
		wrong = !(F0 > 0.0 && F0 < INFINITY);
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

// grid (pairs of the chunk), block 256: one pair's whole iteration (the rule of include/physher_amd.h); thread b owns bin
// b = 16 mi + mj and forms its four coefficients G[mi][mj][a] itself
__global__ __launch_bounds__(PAIRDIST_THREADS) void k_pairdist_solve4(const PairSolveArgs a) {
	__shared__ double sh_S[12], sh_w[3 * PAIRDIST_WAVES];
	const int pair = blockIdx.x, b = threadIdx.x, mi = b >> 4, mj = b & 15;
	const double N = a.counts[(size_t)pair * 256 + b];
	double G[4];
	{
		const double *V = a.model + 4, *Vi = a.model + 20;
		double f[4], m[4];
#pragma unroll
		for (int s = 0; s < 4; s++) f[s] = (mi >> s) & 1 ? a.freqs[s] : 0.0, m[s] = (mj >> s) & 1 ? 1.0 : 0.0;
#pragma unroll
		for (int i = 0; i < 4; i++) {
			const double g = V[i] * f[0] + V[4 + i] * f[1] + V[8 + i] * f[2] + V[12 + i] * f[3];                       // (V^T (pi o mi))_i
			const double q = Vi[4 * i] * m[0] + Vi[4 * i + 1] * m[1] + Vi[4 * i + 2] * m[2] + Vi[4 * i + 3] * m[3];  // (V^-1 mj)_i
			G[i] = g * q;
		}
	}
	solve_one_length([&](double t, bool final, double *lnl, double *d1, double *d2, bool *bad) { pairdist_evaluate(a, N, G, t, final, sh_S, sh_w, lnl, d1, d2, bad); },
	                 a.start[pair], a.lower, a.upper, a.tolerance, a.max_iterations, a.out + (size_t)pair * 4, a.iterations + pair);
}
