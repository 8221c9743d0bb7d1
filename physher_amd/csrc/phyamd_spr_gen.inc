// phyamd_spr_gen.inc: 20-state kernels of phyamd_spr_log_likelihoods_general -- lnL of every SPR regraft of chosen subtrees of the
// engine's tree in one call -- included by phyamd_engine.hip inside its anonymous namespace, behind phyamd_spr4.inc (whose definition,
// candidates, slab and finish kernel these are) and phyamd_place_gen.inc (whose resident partials and helpers they read).
//
// A ROW is a prune node p; u its parent, s its sibling, g = parent(u).  A stored 20-state lower is already the message m_n = P_n p_n
// (a tip: tip_matvec of its branch's image with its code over the engine's sets), so pruning p changes two things only, and the row
// walk k_classspr_walk forms both in the row's scratch (planes [C][20][Pp] like the engine's partials):
//   PATH ops, from u to the root (g = a_1, ..., a_d = root):  m'(slot of u at g) = P_u m_s -- the sibling's branch absorbs the
//     parent's, no merged matrix is formed --, then m'(a_j) = P_(a_j) (m'(path child of a_j) o m(its other child)) for every a_j but
//     the root: depth(u) products;
//   PRE-ORDER ops, for every internal node x outside p's subtree, parent before child:  A_x = P_x u'_x (ones at the root),
//     u'_l = A_x o m'_r and u'_r = A_x o m'_l for the internal children (a tip needs no upper stored), with m' the path message where
//     the child is on the path or is u's slot, the engine's stored message otherwise, and ones for p itself: u is a pass-through node
//     that hands A_u on to s.  The walk never enters p's subtree.
// No resident upper is read and pi enters in the regraft kernel only, so nothing depends on PHYAMD_GRAD_FOLD_ROOT_FREQS.  An op reads
// what earlier ops of its own row wrote, per pattern: a (row, 128 patterns) workgroup runs the row's ops in order and every lane
// reads back exactly the cells it stored itself (the D layout of a product is the B layout of the next), so there is no
// synchronisation across workgroups -- the barriers are for the LDS images alone.
//
// A CANDIDATE is a target edge, named by the node w below it: x its parent, y its sibling.  k_classspr forms, per (candidate,
// category c, 16-pattern tile), with H_w = P(0.5 t_w r_c),
//   lo  = H_w p'_w,   p'_w = m'_left o m'_right (a tip: the column of H_w's image)
//   U   = (x is the root ? 1 : P_x u'_x) o m'_y
//   L_c = sum_i pi_i U_i (H_w (lo o m_p))_i
// three 20-wide products on v_mfma_f64_16x16x4_f64.  The categories run in order inside the wave and accumulate w_c L_c per lane -- a
// lane holds the states 4 ks + (lane >> 4) of its pattern --, the four lanes of a pattern meet once by lanes_sum16, then w_k log L is
// added over the tile (wave_sum), over the waves in wave order, and written to the slab [candidate][block]; k_spr_finish adds the
// blocks in block order.  No atomics: a row's bits depend on the engine's inputs and on p alone.
// (The kernels are named k_classspr*, not k_spr_*: tests/test_spr_abi.py and tests/test_spr_optimize_abi.py count the kernels whose
// names hold "k_spr" and expect the 4-state calls' own.)

constexpr int CLASSSPR_BLOCK = GenGeo<2>::WAVES * 16;  // patterns of a workgroup: a tile per wave

// one op of a row.  A factor message is a pointer (a resident lower or a path message of the row's scratch), or -- null -- the column
// of the tip a / b's image, or ones where the id is negative (the pruned subtree)
struct ClassSprOp {
	const double *src;      // pre-order: u'_x (null: x is the root, A_x = ones); path: null
	const double *ma, *mb;  // the factor messages
	double *da, *db;        // pre-order: where u'_left / u'_right go (null: not stored); path: da is where the message goes
	int32_t mat;            // the node whose image carries: x, or the path node
	int32_t a, b;           // the factors' nodes
	int32_t path;           // 1: a path op, da = P_mat (ma o mb)
	int32_t pad[2];
};

struct ClassSprWalkArgs {
	const ClassSprOp *ops;    // [row][stride]
	const int32_t *nops;      // [row]
	int stride, P, Pp, C;
	const uint8_t *tipcode;   // [T][P]
	const unsigned long long *tipsets;  // the engine's sets
	const double *imgs;       // [N][C][MatImage<2, 5>::SIZE]: the engine's images of P(t_n r_c)
};

// a factor message in D layout
__device__ __forceinline__ void classspr_message(const double *msg, int node, const double *img, size_t Pp, const TileAddr<2, 5> &ta, int code,
                                                 const unsigned long long *tipsets, f64x4 (&m)[2]) {
	if (msg) {
		double frag[5];
		load_b<2, 5>(msg, Pp, ta, frag);
		b_as_d<2, 5>(frag, m);
	} else if (node >= 0) tip_matvec<2, 5>(img, PLACE_GEN_STATES, code, tipsets, m);
	else load_state_weights<2>(nullptr, PLACE_GEN_STATES, true, m);
}

// grid (Ppad / CLASSSPR_BLOCK, rows of the chunk), block 8 waves: a wave owns the 16-pattern tile blockIdx.x * 8 + wave of its row
__global__ __launch_bounds__(GenGeo<2>::WAVES * 64) void k_classspr_walk(const ClassSprWalkArgs a) {
	constexpr int RT = 2, KT = 5, S = PLACE_GEN_STATES, WV = GenGeo<RT>::WAVES;
	using Img = MatImage<RT, KT>;
	__shared__ double sh[3 * Img::SIZE];
	double *imgM = sh, *imgA = sh + Img::SIZE, *imgB = sh + 2 * Img::SIZE;
	const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const int pat = (blockIdx.x * WV + wave) * 16 + (lane & 15);
	const size_t Pp = (size_t)a.Pp;
	const TileAddr<RT, KT> ta(pat, a.P, (unsigned)a.Pp);  // (a pattern past the last reads pattern 0 and stores nothing)
	const ClassSprOp *ops = a.ops + (size_t)blockIdx.y * a.stride;
	const int nops = a.nops[blockIdx.y];
#pragma unroll 1
	for (int i = 0; i < nops; i++) {
		const ClassSprOp op = ops[i];
		const bool tip_a = !op.ma && op.a >= 0, tip_b = !op.mb && op.b >= 0;
		const int code_a = tip_a && ta.ok ? a.tipcode[(size_t)op.a * a.P + pat] : S;
		const int code_b = tip_b && ta.ok ? a.tipcode[(size_t)op.b * a.P + pat] : S;
#pragma unroll 1
		for (int c = 0; c < a.C; c++) {
			__syncthreads();  // (the previous images have been read)
			if (op.path || op.src) stage_image<RT, KT>(imgM, a.imgs + ((size_t)op.mat * a.C + c) * Img::SIZE);
			if (tip_a) stage_image<RT, KT>(imgA, a.imgs + ((size_t)op.a * a.C + c) * Img::SIZE);
			if (tip_b) stage_image<RT, KT>(imgB, a.imgs + ((size_t)op.b * a.C + c) * Img::SIZE);
			__syncthreads();
			const size_t plane = (size_t)c * S * Pp;
			f64x4 ma[RT], mb[RT], A[RT];
			double frag[KT];
			classspr_message(op.ma ? op.ma + plane : nullptr, op.a, imgA, Pp, ta, code_a, a.tipsets, ma);
			classspr_message(op.mb ? op.mb + plane : nullptr, op.b, imgB, Pp, ta, code_b, a.tipsets, mb);
			if (op.path) {
#pragma unroll
				for (int t = 0; t < RT; t++) ma[t] = ma[t] * mb[t];
				d_as_b<RT, KT>(ma, frag);
				mfma_matvec<RT, KT>(imgM, frag, A);
				store_d<RT, KT>(op.da + plane, Pp, ta, A);
				continue;
			}
			if (op.src) {
				load_b<RT, KT>(op.src + plane, Pp, ta, frag);
				mfma_matvec<RT, KT>(imgM, frag, A);
			} else load_state_weights<RT>(nullptr, S, true, A);
			if (op.da) {
				f64x4 u[RT];
#pragma unroll
				for (int t = 0; t < RT; t++) u[t] = A[t] * mb[t];
				store_d<RT, KT>(op.da + plane, Pp, ta, u);
			}
			if (op.db) {
				f64x4 u[RT];
#pragma unroll
				for (int t = 0; t < RT; t++) u[t] = A[t] * ma[t];
				store_d<RT, KT>(op.db + plane, Pp, ta, u);
			}
		}
	}
}

// a regraft onto the edge above w: the pruned tree's upper of x = parent(w) in the row's scratch (null: x is the root), the messages
// of y = sibling(w), of w's children l and r and of p (null: a tip, whose codes are that row of tipcode; l = r = -1: w is a tip)
struct ClassSprCand {
	const double *ux, *my, *ml, *mr, *mp;
	int32_t w, x, y, l, r, p;
};

struct ClassSprArgs {
	const ClassSprCand *cands;  // [gridDim.y], row-major
	int P, Pp, C;
	const uint8_t *tipcode;     // [T][P]
	const unsigned long long *tipsets;
	const double *freqs, *props, *weights;
	const double *imgs;         // [N][C][image]: the engine's lengths
	const double *half;         // [N][C][image]: half the engine's lengths
	double *slab;               // [gridDim.y][gridDim.x]: the block's sum of w log L
};

// grid (Ppad / CLASSSPR_BLOCK, candidates of the chunk), block 8 waves: a wave owns the 16-pattern tile blockIdx.x * 8 + wave
__global__ __launch_bounds__(GenGeo<2>::WAVES * 64) void k_classspr(const ClassSprArgs a) {
	constexpr int RT = 2, KT = 5, S = PLACE_GEN_STATES, WV = GenGeo<RT>::WAVES;
	using Img = MatImage<RT, KT>;
	__shared__ double sh[6 * Img::SIZE + WV];
	double *imgX = sh, *imgH = sh + Img::SIZE, *imgY = sh + 2 * Img::SIZE, *imgL = sh + 3 * Img::SIZE, *imgR = sh + 4 * Img::SIZE, *imgP = sh + 5 * Img::SIZE;
	double *red = sh + 6 * Img::SIZE;  // [wave]
	const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), rq = lane >> 4;
	const ClassSprCand cd = a.cands[blockIdx.y];
	const int pat = (blockIdx.x * WV + wave) * 16 + (lane & 15);
	const size_t Pp = (size_t)a.Pp;
	const TileAddr<RT, KT> ta(pat, a.P, (unsigned)a.Pp);  // (a pattern past the last reads pattern 0 and adds 0)
	const bool tip_w = cd.l < 0, tip_y = !cd.my, tip_l = !tip_w && !cd.ml, tip_r = !tip_w && !cd.mr, tip_p = !cd.mp;
	const auto code_of = [&](bool tip, int node) { return tip && ta.ok ? (int)a.tipcode[(size_t)node * a.P + pat] : S; };
	const int code_w = code_of(tip_w, cd.w), code_y = code_of(tip_y, cd.y), code_l = code_of(tip_l, cd.l), code_r = code_of(tip_r, cd.r), code_p = code_of(tip_p, cd.p);
	f64x4 fpi[RT];
	load_state_weights<RT>(a.freqs, S, false, fpi);
	double L = 0.0;
#pragma unroll 1
	for (int c = 0; c < a.C; c++) {
		__syncthreads();  // (the previous category's images have been read)
		if (cd.ux) stage_image<RT, KT>(imgX, a.imgs + ((size_t)cd.x * a.C + c) * Img::SIZE);
		stage_image<RT, KT>(imgH, a.half + ((size_t)cd.w * a.C + c) * Img::SIZE);
		if (tip_y) stage_image<RT, KT>(imgY, a.imgs + ((size_t)cd.y * a.C + c) * Img::SIZE);
		if (tip_l) stage_image<RT, KT>(imgL, a.imgs + ((size_t)cd.l * a.C + c) * Img::SIZE);
		if (tip_r) stage_image<RT, KT>(imgR, a.imgs + ((size_t)cd.r * a.C + c) * Img::SIZE);
		if (tip_p) stage_image<RT, KT>(imgP, a.imgs + ((size_t)cd.p * a.C + c) * Img::SIZE);
		__syncthreads();
		const size_t plane = (size_t)c * S * Pp;
		f64x4 lo[RT], f[RT], m[RT];
		double frag[KT];
		if (tip_w) tip_matvec<RT, KT>(imgH, S, code_w, a.tipsets, lo);
		else {
			classspr_message(cd.ml ? cd.ml + plane : nullptr, cd.l, imgL, Pp, ta, code_l, a.tipsets, lo);
			classspr_message(cd.mr ? cd.mr + plane : nullptr, cd.r, imgR, Pp, ta, code_r, a.tipsets, m);
#pragma unroll
			for (int t = 0; t < RT; t++) m[t] = lo[t] * m[t];
			d_as_b<RT, KT>(m, frag);
			mfma_matvec<RT, KT>(imgH, frag, lo);
		}
		classspr_message(cd.mp ? cd.mp + plane : nullptr, cd.p, imgP, Pp, ta, code_p, a.tipsets, m);
#pragma unroll
		for (int t = 0; t < RT; t++) m[t] = lo[t] * m[t];
		d_as_b<RT, KT>(m, frag);
		mfma_matvec<RT, KT>(imgH, frag, lo);  // H_w (lo o m_p)
		classspr_message(cd.my ? cd.my + plane : nullptr, cd.y, imgY, Pp, ta, code_y, a.tipsets, f);
		if (cd.ux) {
			load_b<RT, KT>(cd.ux + plane, Pp, ta, frag);
			mfma_matvec<RT, KT>(imgX, frag, m);  // A_x
#pragma unroll
			for (int t = 0; t < RT; t++) f[t] = f[t] * m[t];
		}
		double s = 0.0;
#pragma unroll
		for (int ks = 0; ks < KT; ks++) s = __builtin_fma(fpi[ks >> 2][ks & 3] * f[ks >> 2][ks & 3], lo[ks >> 2][ks & 3], s);  // state 4 ks + rq
		L = __builtin_fma(a.props[c], s, L);
	}
	const double w = ta.ok ? a.weights[pat] : 0.0;
	const bool counts = ta.ok && rq == 0 && w != 0.0;  // one lane of a pattern's four adds it
	const double Lp = lanes_sum16(L);  // the pattern's 20 terms of every category: the same bits in its four lanes
	const double s0 = wave_sum(counts ? w * log(Lp) : 0.0);
	if (lane == 0) red[wave] = s0;
	__syncthreads();
	if (threadIdx.x == 0) {
		double s = 0.0;
		for (int v = 0; v < WV; v++) s += red[v];
		a.slab[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
	}
}
