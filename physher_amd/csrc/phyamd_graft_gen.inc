// phyamd_graft_gen.inc: 20-state kernels of phyamd_spr_optimize_general -- for every SPR regraft of chosen subtrees of the engine's tree
// the three branch lengths that meet at the graft point, optimised one at a time, pass after pass -- included by phyamd_engine.hip
// inside its anonymous namespace, behind phyamd_spr_gen.inc (whose rows, walk, candidates and messages these read), phyamd_tripod4.inc
// (whose definition and finish kernel these share) and phyamd_qopt_gen.inc (whose K formulas, images and evaluation these are, with a
// general 20-vector where the query's class tables stood).  The rule and its visit loop are phyamd_rule.inc's three_branch_rule.
//
// The walk is phyamd_spr_log_likelihoods_general's (k_classspr_walk): per ROW (prune node p) the path messages and the pruned tree's
// uppers in the row's planes.  Per candidate (target edge w; x its parent, y its sibling) three vectors meet at the new central node
// u, and none depends on the three lengths t_p, t_w, t_u:
//   A = p_p, p's own partial (a tip: its code over the engine's sets; an internal node: k_classplace_own's plane, formed once per call)
//   B = p'_w, w's own partial in the pruned tree (off the row's path: the engine's, the same plane as an A; on the path above u: formed
//       per row from the path messages)
//   F = pi o U,  U = (x is the root ? 1 : P_x u'_x) o m'_y: k_classspr's U, written once per candidate by k_classgraft_upper
// In the length of the visited branch the site likelihood is sum_c sum_e K[c][e] exp(lambda_e r_c t) with
//   u:  K = w_c (V^T F)_e (V^-1 [(P(t_w) B) o (P(t_p) A)])_e
//   w:  K = w_c (V^T [(P(t_u)^T F) o (P(t_p) A)])_e (V^-1 B)_e
//   p:  K = w_c (V^T [(P(t_u)^T F) o (P(t_w) B)])_e (V^-1 A)_e
// k_classgraft_solve is k_classopt_solve's sibling: one workgroup of four waves runs a candidate's whole rule.  Per visit the
// categories run in order: the two held P(t r_c) = |V e^(lambda t r_c) V^-1| are formed in LDS from the eigen system
// (k_transition_matrices' arithmetic) and written as MFMA images (classopt_image; P(t_u) transposed); then a wave takes the
// 16-pattern tiles wave, wave + 4, ... and forms K with four 20-wide products on v_mfma_f64_16x16x4_f64 (a tip's A or B is a column
// gather, tip_matvec).  K goes to the candidate's plane [C][20][Pp]: lane (row quarter rq, pattern) holds the eigen terms 4 ks + rq of
// its pattern, stores them and is the lane that reads them back in every evaluation of the visit, so no barrier stands between the
// two.  Every iterate is classopt_evaluate: every thread holds the same bits and takes the same accept, bisect and stop decisions.
// No atomics; a candidate's bits depend on the engine's inputs and on (p, w) alone.
// (The kernels are named k_classgraft_*: the resource tests of the other calls count kernels by the substrings k_spr, k_tripod,
// k_classspr, k_classopt, ... and expect their own.  k_classgraft_solve shares classopt_image and classopt_evaluate, which are inlined
// into each kernel that names them, and nothing else: k_classopt_solve's instructions are untouched.)

// a regraft: p's own partial and w's in the pruned tree (null: a tip, whose codes are that row of tipcode); p_left: p is u's left child
struct ClassGraftCand {
	const double *A, *B;
	int32_t p, w, p_left, pad;
};
// ... as the solve kernel holds it: which of the two are tips in scalar registers (a uniform branch), the rest in vector ones
struct ClassGraftHeld {
	ClassGraftCand cd;
	bool tip_p, tip_w;
};

struct ClassGraftUpperArgs {
	const ClassSprCand *cands;  // [gridDim.y]: the scoring call's records (ux, my, x, y are read)
	int P, Pp, C;
	const uint8_t *tipcode;     // [T][P]
	const unsigned long long *tipsets;
	const double *freqs;
	const double *imgs;         // [N][C][image]: the engine's lengths
	double *F;                  // [gridDim.y][C][20][Pp]: pi o U
};

// grid (Ppad / CLASSSPR_BLOCK, candidates of the chunk), block 8 waves: a wave owns the 16-pattern tile blockIdx.x * 8 + wave
// (k_classspr's shape and U; a pattern past the last reads pattern 0 and stores nothing)
__global__ __launch_bounds__(GenGeo<2>::WAVES * 64) void k_classgraft_upper(const ClassGraftUpperArgs a) {
	constexpr int RT = 2, KT = 5, S = PLACE_GEN_STATES, WV = GenGeo<RT>::WAVES;
	using Img = MatImage<RT, KT>;
	__shared__ double sh[2 * Img::SIZE];
	double *imgX = sh, *imgY = sh + Img::SIZE;
	const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const ClassSprCand cd = a.cands[blockIdx.y];
	const int pat = (blockIdx.x * WV + wave) * 16 + (lane & 15);
	const size_t Pp = (size_t)a.Pp;
	const TileAddr<RT, KT> ta(pat, a.P, (unsigned)a.Pp);
	const bool tip_y = !cd.my;
	const int code_y = tip_y && ta.ok ? (int)a.tipcode[(size_t)cd.y * a.P + pat] : S;
	f64x4 fpi[RT];
	load_state_weights<RT>(a.freqs, S, false, fpi);
	double *const Fcand = a.F + (size_t)blockIdx.y * a.C * S * Pp;
#pragma unroll 1
	for (int c = 0; c < a.C; c++) {
		__syncthreads();  // (the previous category's images have been read)
		if (cd.ux) stage_image<RT, KT>(imgX, a.imgs + ((size_t)cd.x * a.C + c) * Img::SIZE);
		if (tip_y) stage_image<RT, KT>(imgY, a.imgs + ((size_t)cd.y * a.C + c) * Img::SIZE);
		__syncthreads();
		const size_t plane = (size_t)c * S * Pp;
		f64x4 f[RT], m[RT];
		double frag[KT];
		classspr_message(cd.my ? cd.my + plane : nullptr, cd.y, imgY, Pp, ta, code_y, a.tipsets, f);
		if (cd.ux) {
			load_b<RT, KT>(cd.ux + plane, Pp, ta, frag);
			mfma_matvec<RT, KT>(imgX, frag, m);  // A_x
#pragma unroll
			for (int t = 0; t < RT; t++) f[t] = f[t] * m[t];
		}
#pragma unroll
		for (int t = 0; t < RT; t++) f[t] = fpi[t] * f[t];
		store_d<RT, KT>(Fcand + plane, Pp, ta, f);
	}
}

enum { MEET_P = 0, MEET_W = 1, MEET_U = 2 };  // the three branches, in `lengths`' order

struct ClassGraftArgs {
	const ClassGraftCand *cands;  // [gridDim.x]
	int P, Pp, C;
	int max_iterations, max_passes;
	double lower, upper, tolerance, lnl_tolerance;
	const uint8_t *tipcode;       // [T][P]
	const unsigned long long *tipsets;
	const double *props;
	const double *model;          // eval [20] | evec [20][20] | ivec [20][20]
	const double *rates, *weights;
	const double *start;          // [gridDim.x][t_p, t_w, t_u]
	const double *F;              // [gridDim.x][C][20][Pp]
	double *K;                    // [gridDim.x][C][20][Pp]
	double *out;                  // [gridDim.x][t_p, t_w, t_u, lnl, initial_lnl]
	int32_t *status;              // [gridDim.x][RULE_STATUS]
};

struct ClassGraftShared {
	double V[400], Vi[400];                 // the eigenvectors, row-major
	double imgVT[MatImage<2, 5>::SIZE], imgVi[MatImage<2, 5>::SIZE];  // images of V^T and of V^-1
	double img0[MatImage<2, 5>::SIZE], img1[MatImage<2, 5>::SIZE];    // a category's: of P(t_p) (u) or P(t_u)^T (w, p); of P(t_w) (u, p) or P(t_p) (w)
	double Pm[2 * 400];                     // a category's two matrices, row-major
	double x[2 * PLACE_GEN_STATES];         // their exponentials
	double e[3 * PLACE_GEN_STATES * BATCH_MAX_CATEGORIES], w[3 * CLASSOPT_WAVES];  // an evaluation's
};

// img . (own partial, or -- tip -- the tip's code) in D layout
__device__ __forceinline__ void classgraft_product(const double *img, bool tip, const double *own, size_t Pp, const TileAddr<2, 5> &ta, int code, const unsigned long long *tipsets,
                                                   f64x4 (&d)[2]) {
	if (!tip) {
		double frag[5];
		load_b<2, 5>(own, Pp, ta, frag);
		mfma_matvec<2, 5>(img, frag, d);
	} else
		tip_matvec<2, 5>(img, PLACE_GEN_STATES, code, tipsets, d);
}

// K of the visit of branch z at the lengths (tp, tw, tu), for the patterns of this wave's tiles
__device__ __forceinline__ void classgraft_coefficients(const ClassGraftArgs &a, const ClassGraftHeld &held, const double *Fcand, double *Kcand, int z, double tp, double tw,
                                                        double tu, ClassGraftShared &sh) {
	constexpr int S = PLACE_GEN_STATES, RT = 2, KT = 5;
	const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
	size_t npc = (size_t)PLACE_GEN_STATES * a.Pp;  // doubles of a category's plane
	asm volatile("" : "+v"(npc));                    // (added to bases that live in vector registers)
	const int tiles = a.Pp / 16;
	const double t0 = z == MEET_U ? tp : tu, t1 = z == MEET_W ? tp : tw;  // the two matrices' lengths: u: t_p, t_w; w: t_u, t_p; p: t_u, t_w
#pragma unroll 1
	for (int c = 0; c < a.C; c++) {
		__syncthreads();  // (the previous category's images have been read; so have the previous evaluation's sums)
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
		if (z == MEET_U) classopt_image<false>(sh.img0, sh.Pm);
		else classopt_image<true>(sh.img0, sh.Pm);
		classopt_image<false>(sh.img1, sh.Pm + S * S);
		__syncthreads();
		const double wc = a.props[c];
		const size_t plane = (size_t)c * npc;
		const ClassGraftCand &cd = held.cd;
		const bool tip_p = held.tip_p, tip_w = held.tip_w;
		const double *Fc = Fcand + plane, *A = cd.A + plane, *B = cd.B + plane;  // (a tip's is not read)
		double *Kc = Kcand + plane;
#pragma unroll 1
		for (int tile = wave; tile < tiles; tile += CLASSOPT_WAVES) {
			const int pat = tile * 16 + (lane & 15);
			const size_t Pp = opaque_stride(a.Pp);  // (row pointers formed per tile, not kept across the loop in scalar registers)
			const TileAddr<RT, KT> ta(pat, a.P, (unsigned)a.Pp);  // (a pattern past the last reads pattern 0 and stores nothing)
			const int kp = tip_p && ta.ok ? (int)a.tipcode[(size_t)cd.p * a.P + pat] : S;
			const int kw = tip_w && ta.ok ? (int)a.tipcode[(size_t)cd.w * a.P + pat] : S;
			double frag[KT];
			f64x4 f[RT], g[RT], q[RT], v[RT];
			load_b<RT, KT>(Fc, Pp, ta, frag);
			if (z == MEET_U) {
				mfma_matvec<RT, KT>(sh.imgVT, frag, g);
				classgraft_product(sh.img1, tip_w, B, Pp, ta, kw, a.tipsets, v);  // P(t_w) B
				classgraft_product(sh.img0, tip_p, A, Pp, ta, kp, a.tipsets, q);  // P(t_p) A
#pragma unroll
				for (int t = 0; t < RT; t++) v[t] = v[t] * q[t];
				d_as_b<RT, KT>(v, frag);
				mfma_matvec<RT, KT>(sh.imgVi, frag, q);
			} else {
				mfma_matvec<RT, KT>(sh.img0, frag, f);  // P(t_u)^T F
				if (z == MEET_W) classgraft_product(sh.img1, tip_p, A, Pp, ta, kp, a.tipsets, v);  // P(t_p) A
				else classgraft_product(sh.img1, tip_w, B, Pp, ta, kw, a.tipsets, v);               // P(t_w) B
#pragma unroll
				for (int t = 0; t < RT; t++) f[t] = f[t] * v[t];
				d_as_b<RT, KT>(f, frag);
				mfma_matvec<RT, KT>(sh.imgVT, frag, g);
				if (z == MEET_W) classgraft_product(sh.imgVi, tip_w, B, Pp, ta, kw, a.tipsets, q);
				else classgraft_product(sh.imgVi, tip_p, A, Pp, ta, kp, a.tipsets, q);
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

// grid (candidates of the chunk), block 256: one candidate's whole rule (three_branch_rule, phyamd_rule.inc: every slot is visited,
// the start is lnl_0 in the length of u as it is given), every thread with the same bits.  Compiled for two waves per SIMD like
// k_classopt_solve
__global__ __launch_bounds__(CLASSOPT_THREADS, 2) void k_classgraft_solve(const ClassGraftArgs args) {
	constexpr int S = PLACE_GEN_STATES;
	__shared__ ClassGraftShared sh;
	const int tid = threadIdx.x;
	// the arguments that are no base of a tile's row pointers, once, into vector registers (k_tripod_solve4's remedy): left in scalar
	// ones for the whole rule they and the loop's own uniform values are more than the scalar file holds
	ClassGraftArgs a = args;
	a.tipcode = tripod_in_vgprs(a.tipcode), a.tipsets = tripod_in_vgprs(a.tipsets), a.props = tripod_in_vgprs(a.props), a.model = tripod_in_vgprs(a.model);
	a.rates = tripod_in_vgprs(a.rates), a.weights = tripod_in_vgprs(a.weights), a.start = tripod_in_vgprs(a.start), a.out = tripod_in_vgprs(a.out);
	a.status = tripod_in_vgprs(a.status);
	asm volatile("" : "+v"(a.lower), "+v"(a.upper), "+v"(a.tolerance), "+v"(a.lnl_tolerance), "+v"(a.max_iterations), "+v"(a.max_passes), "+v"(a.P));  // (P is compared per lane)
	for (int idx = tid; idx < S * S; idx += CLASSOPT_THREADS) sh.V[idx] = a.model[S + idx], sh.Vi[idx] = a.model[S + S * S + idx];
	__syncthreads();
	classopt_image<true>(sh.imgVT, sh.V);
	classopt_image<false>(sh.imgVi, sh.Vi);  // (the first barrier after these is classgraft_coefficients')
	const size_t cand = blockIdx.x;
	ClassGraftHeld held;
	held.cd = a.cands[cand];
	held.tip_p = __builtin_amdgcn_readfirstlane(held.cd.A == nullptr) != 0, held.tip_w = __builtin_amdgcn_readfirstlane(held.cd.B == nullptr) != 0;
	held.cd.A = tripod_in_vgprs(held.cd.A), held.cd.B = tripod_in_vgprs(held.cd.B);
	asm volatile("" : "+v"(held.cd.p), "+v"(held.cd.w), "+v"(held.cd.p_left));  // (a tip's code row is addressed per lane anyway)
	const int p_left = held.cd.p_left;
	__builtin_assume(a.C >= 1);  // (check_general_query_inputs: no loop over the categories needs a guard kept in scalar registers)
	const size_t npd = (size_t)a.C * S * a.Pp;
	const double *const Fcand = tripod_in_vgprs(a.F + cand * npd);
	double *const Kcand = tripod_in_vgprs(a.K + cand * npd);  // (every use is a lane's own address)
	// thread 0's record and the start, addressed once: the candidate's index need not stay live through the rule
	double *const out = tripod_in_vgprs(a.out + cand * 5);
	int32_t *const status = tripod_in_vgprs(a.status + cand * RULE_STATUS);
	const double start_p = a.start[cand * 3], start_w = a.start[cand * 3 + 1], start_u = a.start[cand * 3 + 2];
	three_branch_rule<true>(
	    [&](int z, double tp, double tw, double tu) { classgraft_coefficients(a, held, Fcand, Kcand, z, tp, tw, tu, sh); },
	    [&](double t, bool final, double *lnl, double *d1, double *d2, bool *bad) { classopt_evaluate(a, Kcand, t, final, sh, lnl, d1, d2, bad); },
	    // u's left child, its right child, u: p keeps its slot, w has the one s had
	    // (p_left is 0 or 1 and lives in a vector register: slot 0 is p where p is the left child, slot 1 where it is the right one)
	    [p_left](int slot) { return slot == 2 ? (int)MEET_U : slot ^ p_left ^ 1; }, 7, start_p, start_w, start_u, a.lower, a.upper, a.tolerance,
	    a.max_iterations, a.lnl_tolerance, a.max_passes, out, status);
}
