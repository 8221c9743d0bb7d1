// phyamd_nniopt4.inc: 4-state kernels of phyamd_nni_optimize -- for every NNI neighbour of the engine's tree the central branch
// length that maximises its lnL, with lnL, d1 and d2 there -- included by phyamd_engine.hip inside its anonymous namespace.
//
// The walk is phyamd_nni_log_likelihoods' (phyamd_nni4.inc): ONE item through k_batch_walk4<false> with every upper parked, which
// leaves every internal node's lower p_n and every internal non-root node's upper u_n in the batch scratch.  The four messages that
// meet on a candidate edge do not depend on the trial length, so with U and p of arrangement k (the table of phyamd_nni4.inc) and
// the eigen system Q = V diag(lambda) V^-1 an entry's site likelihood is an exponential sum in the length t of v:
//   L(t)   = sum_c sum_a K[c][a] e_ca(t),          e_ca(t) = exp(lambda_a (t r_c))
//   L'(t)  = sum_c sum_a K[c][a] x_ca e_ca(t),     x_ca = lambda_a r_c
//   L''(t) = sum_c sum_a K[c][a] x_ca^2 e_ca(t),   K[c][a] = w_c (V^T (pi o U))_a (V^-1 p)_a
// -- k_nni4's L, L', L'' with P(t) = V e^(lambda t) V^-1 multiplied out (but for the fabs on P's entries, substmodel.c:552: a
// rounding difference).  k_cbopt_coeff4 writes K once per entry; k_cbopt_solve4 runs the whole safeguarded Newton iteration of an
// entry in one workgroup: per step C x 4 exponentials per workgroup and 3 x 4 C FMAs per pattern, no walk, no matrix launch, no
// host round trip.  No floating-point atomics: the pattern sums go per thread in stride order, then wave_sum, then the waves in
// wave order through LDS, so every thread holds the same bits and the accept / bisect decision is uniform.

struct CboptCoeffArgs {
	const NniCand *cands;    // [gridDim.y]: the chunk's candidates
	int T, N, P, C, nblk;
	const uint8_t *tipmask;  // [T][P]
	const double *freqs, *props;
	const double *model;     // eval [4] | evec [4][4] | ivec [4][4]
	const double *mats;      // [N][C][16]: the engine's lengths (the walk's item)
	const double *lower;     // [T - 1][C][nblk * 64][4]
	const double *upper;     // [T - 1][C][nblk * 64][4]
	double *K;               // [gridDim.y][3][C][4][nblk * 64]
};

// grid (nblk, candidates of the chunk), block (64, C): the C category waves of 64 patterns of one edge, its three arrangements
__global__ __launch_bounds__(BATCH_MAX_CATEGORIES *WAVE) void k_cbopt_coeff4(const CboptCoeffArgs a) {
	const int lane = threadIdx.x, c = __builtin_amdgcn_readfirstlane(threadIdx.y);  // this wave's category
	const NniCand cd = load_nni_cand(a.cands, blockIdx.y);
	const int k0 = blockIdx.x * WAVE + lane;  // the scratch is padded to whole blocks and the walk has written every lane's cells
	const int k = k0 < a.P ? k0 : a.P - 1;
	const size_t Pp = (size_t)a.nblk * WAVE, plane = Pp * 4, node_stride = (size_t)a.C * plane;
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
	const double wc = a.props[c];
	const cptr V = as_const(a.model + 4), Vi = as_const(a.model + 20);
	double *Kc = a.K + (((size_t)blockIdx.y * 3) * a.C + c) * 4 * Pp + k0;
#pragma unroll
	for (int arr = 0; arr < 3; arr++) {
		const d4 fU = mul4(f, arr == 0 ? ms : arr == 1 ? ma : mb);
		const d4 p = arr == 0 ? mul4(ma, mb) : arr == 1 ? mul4(ms, mb) : mul4(ma, ms);
		const d4 q = matvec4(opaque(Vi), p);  // V^-1 p
		const cptr W = opaque(V);
		d4 g;                                 // V^T (pi o U)
		g.x = W[0] * fU.x + W[4] * fU.y + W[8] * fU.z + W[12] * fU.w;
		g.y = W[1] * fU.x + W[5] * fU.y + W[9] * fU.z + W[13] * fU.w;
		g.z = W[2] * fU.x + W[6] * fU.y + W[10] * fU.z + W[14] * fU.w;
		g.w = W[3] * fU.x + W[7] * fU.y + W[11] * fU.z + W[15] * fU.w;
		double *Ka = Kc + (size_t)arr * a.C * 4 * Pp;  // one 512-byte row segment per wave each
		Ka[0] = wc * (g.x * q.x);
		Ka[Pp] = wc * (g.y * q.y);
		Ka[2 * Pp] = wc * (g.z * q.z);
		Ka[3 * Pp] = wc * (g.w * q.w);
	}
}

constexpr int CBOPT_THREADS = 256, CBOPT_WAVES = CBOPT_THREADS / WAVE;

struct CboptSolveArgs {
	const NniCand *cands;  // the chunk's candidates: entry i is arrangement i % 3 of candidate i / 3
	int N, P, C, Pp;
	int max_iterations;
	double lower, upper, tolerance;
	const double *model;   // eval [4] | ...
	const double *rates, *weights;
	const double *start;   // [3][N]: the start lengths (the candidates' columns are read)
	const double *K;       // [entries][C][4][Pp]
	double *out;           // [entries][4]: t*, lnL, d1, d2 at t*
	int32_t *iterations;   // [entries]: proposals made, negated where the entry did not converge
};

// the sums of w log L (final only), w L'/L and w (L''/L - (L'/L)^2) over the patterns at length t, the same bits in every
// thread; *bad: some pattern's L is not in (0, inf), so lnL at t is not finite
__device__ __forceinline__ void cbopt_evaluate(const CboptSolveArgs &a, const double *K, double t, bool final, double *sh_e, double *sh_w, double *lnl, double *d1,
                                               double *d2, bool *bad) {
	const int tid = threadIdx.x, C4 = a.C * 4;
	if (tid < C4) {  // e, x e, x^2 e of (category tid / 4, eigenvalue tid % 4), once per workgroup
		const double lam = a.model[tid & 3], r = a.rates[tid >> 2], x = lam * r, e = exp(lam * (t * r));
		sh_e[tid] = e;
		sh_e[C4 + tid] = x * e;
		sh_e[2 * C4 + tid] = x * x * e;
	}
	__syncthreads();
	double s0 = 0.0, s1 = 0.0, s2 = 0.0;
	int wrong = 0;
	for (int k = tid; k < a.P; k += CBOPT_THREADS) {
		double L = 0.0, L1 = 0.0, L2 = 0.0;
		for (int i = 0; i < C4; i++) {
			const double Kv = K[(size_t)i * a.Pp + k];
			L += Kv * sh_e[i];
			L1 += Kv * sh_e[C4 + i];
			L2 += Kv * sh_e[2 * C4 + i];
		}
		const double w = a.weights[k], r1 = L1 / L, r2 = L2 / L;
		if (final) s0 += w * log(L);
		s1 += w * r1;
		s2 += w * (r2 - r1 * r1);
		wrong |= !(L > 0.0 && L < INFINITY);
	}
	s0 = wave_sum(s0), s1 = wave_sum(s1), s2 = wave_sum(s2);
	const int wave = tid / WAVE;
	if (tid % WAVE == 0) sh_w[wave * 3 + 0] = s0, sh_w[wave * 3 + 1] = s1, sh_w[wave * 3 + 2] = s2;
	*bad = __syncthreads_or(wrong) != 0;  // (also the barrier between the waves' stores and the loads below)
	s0 = s1 = s2 = 0.0;
	for (int v = 0; v < CBOPT_WAVES; v++) s0 += sh_w[v * 3 + 0], s1 += sh_w[v * 3 + 1], s2 += sh_w[v * 3 + 2];
	*lnl = s0, *d1 = s1, *d2 = s2;
	__syncthreads();  // sh_e and sh_w are free for the next evaluation
}

// grid (entries of the chunk), block 256: one entry's whole iteration (the rule of include/physher_amd.h)
__global__ __launch_bounds__(CBOPT_THREADS) void k_cbopt_solve4(const CboptSolveArgs a) {
	__shared__ double sh_e[3 * 4 * BATCH_MAX_CATEGORIES], sh_w[3 * CBOPT_WAVES];
	const int entry = blockIdx.x, arr = entry % 3;
	const NniCand cd = load_nni_cand(a.cands, entry / 3);
	const double *K = a.K + (size_t)entry * a.C * 4 * a.Pp;
	solve_one_length([&](double t, bool final, double *lnl, double *d1, double *d2, bool *bad) { cbopt_evaluate(a, K, t, final, sh_e, sh_w, lnl, d1, d2, bad); },
	                 a.start[(size_t)arr * a.N + cd.v], a.lower, a.upper, a.tolerance, a.max_iterations, a.out + (size_t)entry * 4, a.iterations + entry);
}
