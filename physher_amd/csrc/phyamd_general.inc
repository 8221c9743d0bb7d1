// phyamd_general.inc -- kernels for 20 / 60 / 61 states (amino acids, codons) on the fp64 matrix cores.
// Included by phyamd_engine.hip inside its anonymous namespace.
//
// Reference: the P.partial contractions of treelikelihood20.c:114-620 and treelikelihoodX.c:166-576, 878-1001.
// Here one wave owns a tile of 16 patterns of one (node, category) and forms  out[i][pat] = sum_j M[i][j] p[j][pat]
// with v_mfma_f64_16x16x4_f64:  A = M (16 rows x 4 columns from an LDS image), B = p (4 states x 16 patterns).
//
//   * partial layout for S != 4: planes [C][S][Pp] (pattern fastest, Pp = P rounded up to 16), so a B fragment is
//     four 128-byte segments (states 4ks..4ks+3 x 16 consecutive patterns) and a D tile stores the same way;
//   * the f64 MFMA's D layout (row = (lane>>4) + 4*reg, col = lane&15) IS its B layout for k-step 4*tile + reg:
//     a product's result feeds the next product (Q.(P.p)) with no data movement;
//   * matrices are staged once per workgroup into LDS as fragment-major images [RT][KT][64] (conflict-free
//     ds_read_b64, zero padded to 16*RT x 4*KT) plus their row sums; a tip child skips the MFMAs altogether:
//     P.onehot = one gathered column, P.ones = the row sums;
//   * what the post-order pass STORES for an internal node is t_n = P_n p_n, its partial carried through its own branch (the root:
//     p_root): a parent multiplies its stored children element by element, and the pre-order pass reads the same array as the
//     "P_l p_l" of its branch terms -- one product per internal node and evaluation instead of two (k_lower_gen);
//   * 20 states: the branch term of a tip child is a column of an image of Qf P(t) (GenFuse::QP) instead of a product.
//
// Rescaling (SingleTreeLikelihood_scalePartials, treelikelihood.c:1790-1836): a workgroup owns ONE category, while the
// scale factor of a (node, pattern) is the maximum over all categories and states.  The SCALE variants therefore write
// each category's per-pattern maximum (from registers, P doubles per category) and a small per-level kernel combines
// them, divides the few patterns that fell below the threshold and keeps the cumulative log factors; the rescaled
// gradient (a ratio in each branch's own scaled units, like the 4-state path) is finished by a third small kernel.

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int GEN_WAVES20 = 8, GEN_OCC20 = 4;  // 20 states: waves per workgroup, and waves per SIMD the kernels are compiled for
constexpr int GEN_TILES_MAX = 8;  // 16-pattern tiles per wave: chosen per level by choose_gen_tiles (phyamd_launch.inc)
// Workgroups are 8 waves, two per SIMD, that share the LDS images: the f64 MFMA is a 64-cycle instruction issued in order, so a
// lone wave per SIMD leaves the matrix pipe idle through every load, state sum and store (measured at 61 states with one wave per
// SIMD: 24 us per 5-product tile against 10 us of MFMA time).  Two waves need <= 256 registers each: operands are addressed as
// uniform row pointer + one 32-bit byte offset per lane (global_load ... s[base:base+1]), pi is folded into the rate matrix's
// image, and B fragments are loaded right before the product that consumes them.
template <int RT>
struct GenGeo {
	static constexpr int WAVES = RT == 2 ? GEN_WAVES20 : 8;
	static constexpr int MIN_WAVES_PER_SIMD = RT >= 4 ? 2 : GEN_OCC20;
	static constexpr int MIN_PATTERNS_PER_BLOCK = WAVES * 16;  // one tile per wave: the finest grid, which sizes the gradient slabs
};
// state count of a tile shape: (2, 5) = 20, (4, 15) = 60, (4, 16) = 61
template <int RT, int KT>
struct GenStates {
	static constexpr int S = KT == 5 ? 20 : KT == 15 ? 60 : 61;
	static_assert((RT == 2 && KT == 5) || (RT == 4 && (KT == 15 || KT == 16)), "tile shapes of 20 / 60 / 61 states");
};

// 20 states (RT = 2, KT = 5): rows 16..19 go through the 4x4x4 MFMA (see mfma_matvec)
template <int RT, int KT>
struct TailRows {
	static constexpr bool ON = RT == 2 && KT == 5;
};

template <int RT, int KT>
struct MatImage {
	static constexpr int FRAG = RT * KT * 64;   // doubles of fragments
	static constexpr int SIZE = FRAG + RT * 16; // + row sums
};

// one S x S matrix (row-major at M) as MFMA A fragments + row sums; rowscale != nullptr: diag(rowscale) M
template <int RT, int KT>
__device__ __forceinline__ void stage_matrix(double *img, const double *__restrict__ M, int S, const double *__restrict__ rowscale) {
	for (int idx = threadIdx.x; idx < RT * KT * 64; idx += blockDim.x) {
		const int lane = idx & 63, ks = (idx >> 6) % KT, t = (idx >> 6) / KT;
		// (20 states: the second row tile holds rows 16..19 in the A layout of v_mfma_f64_4x4x4_4b, the same 4 x 4 block for each
		// of the instruction's four pattern blocks: lane = 16 k + 4 block + row)
		const int i = (TailRows<RT, KT>::ON && t == 1) ? 16 + (lane & 3) : 16 * t + (lane & 15), j = 4 * ks + (lane >> 4);
		img[idx] = (i < S && j < S) ? (rowscale ? rowscale[i] : 1.0) * M[(size_t)i * S + j] : 0.0;
	}
	for (int i = threadIdx.x; i < RT * 16; i += blockDim.x) {
		double s = 0.0;
		if (i < S)
			for (int j = 0; j < S; j++) s += M[(size_t)i * S + j];
		img[RT * KT * 64 + i] = (i < S && rowscale ? rowscale[i] : 1.0) * s;
	}
}

// The images are built ONCE per evaluation in global memory (one workgroup per matrix): workgroups then stage by a straight
// copy.  Staging from the row-major matrix cost a 61-state workgroup ~36 us (strided 8-byte loads + serial row sums) against
// ~14 us of work per 16-pattern tile.  imgs: [count][MatImage::SIZE]
template <int RT, int KT>
__global__ __launch_bounds__(256) void k_matrix_images(int S, const double *__restrict__ mats, double *__restrict__ imgs, const double *__restrict__ rowscale) {
	stage_matrix<RT, KT>(imgs + (size_t)blockIdx.x * MatImage<RT, KT>::SIZE, mats + (size_t)blockIdx.x * S * S, S, rowscale);
}

// out[(tip, category)] = diag(rowscale) Q . P(t) of that tip branch, row-major (one workgroup per matrix): ensure_tip_rate_products
__global__ __launch_bounds__(256) void k_tip_rate_products(int S, const double *__restrict__ mats, const double *__restrict__ Q, const double *__restrict__ rowscale,
                                                          double *__restrict__ out) {
	const double *Pm = mats + (size_t)blockIdx.x * S * S;  // tips are nodes 0 .. T-1: the first T * C matrices
	double *o = out + (size_t)blockIdx.x * S * S;
	for (int idx = threadIdx.x; idx < S * S; idx += 256) {
		const int i = idx / S, j = idx % S;
		double v = 0.0;
		for (int k = 0; k < S; k++) v += Q[(size_t)i * S + k] * Pm[(size_t)k * S + j];
		o[idx] = rowscale ? rowscale[i] * v : v;
	}
}

// straight copy of a prebuilt image into LDS: every thread issues all of its 16-byte loads before the first LDS store, so a
// workgroup pays one memory round trip per image (the rolled loop paid one per 4 KB: 9 per 61-state image)
template <int RT, int KT>
__device__ __forceinline__ void stage_image(double *img, const double *__restrict__ G) {
	typedef double dv2g __attribute__((ext_vector_type(2)));
	static_assert(MatImage<RT, KT>::SIZE % 2 == 0, "image copied in 16-byte pieces");
	constexpr int N2 = MatImage<RT, KT>::SIZE / 2, THREADS = GenGeo<RT>::WAVES * 64, BATCH = (N2 + THREADS - 1) / THREADS;
	dv2g r[BATCH];
#pragma unroll
	for (int j = 0; j < BATCH; j++) {
		const int idx = j * THREADS + (int)threadIdx.x;
		if (idx < N2) r[j] = reinterpret_cast<const dv2g *>(G)[idx];
	}
#pragma unroll
	for (int j = 0; j < BATCH; j++) {
		const int idx = j * THREADS + (int)threadIdx.x;
		if (idx < N2) reinterpret_cast<dv2g *>(img)[idx] = r[j];
	}
}

// d = M b : RT row tiles, KT k-steps
template <int RT, int KT>
__device__ __forceinline__ void mfma_matvec(const double *img, const double (&b)[KT], f64x4 (&d)[RT]) {
	const int lane = threadIdx.x & 63;
	if (TailRows<RT, KT>::ON) {
		// rows 16..19 of a 20-state product: v_mfma_f64_4x4x4_4b (four 4 x 4 x 4 blocks = the tile's sixteen patterns, 19 cycles)
		// instead of a second 16-row tile that is three quarters padding (64 cycles).  Its B layout (lane = 16 k + pattern) IS
		// the 16x16x4 one, and its single result register is rows 16 + (lane >> 4): register 0 of the second row tile.
		// The 16-row chain and the chain of rows 16..19 advance together -- each instruction's predecessor in its own
		// chain is two issues back, and all ten fragments are requested before the first product
		f64x4 acc = {0., 0., 0., 0.};
		double acc1 = 0.0;
#pragma unroll
		for (int ks = 0; ks < KT; ks++) {
			acc = __builtin_amdgcn_mfma_f64_16x16x4f64(img[ks * 64 + lane], b[ks], acc, 0, 0, 0);
			acc1 = __builtin_amdgcn_mfma_f64_4x4x4f64(img[(KT + ks) * 64 + lane], b[ks], acc1, 0, 0, 0);
		}
		d[0] = acc;
		d[RT - 1] = f64x4{acc1, 0., 0., 0.};
		__builtin_amdgcn_sched_barrier(0);
		return;
	}
#pragma unroll
	for (int t = 0; t < RT; t++) {
		f64x4 acc = {0., 0., 0., 0.};
#pragma unroll
		for (int ks = 0; ks < KT; ks++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(img[(t * KT + ks) * 64 + lane], b[ks], acc, 0, 0, 0);
		d[t] = acc;
		// one row tile's fragments at a time: left alone the scheduler hoists all RT * KT LDS reads (128 registers at 61 states)
		// above the first MFMA and the kernel spills
		__builtin_amdgcn_sched_barrier(0);
	}
}

// a D-layout vector seen as the B fragments of the next product (rows >= S are zero by construction)
template <int RT, int KT>
__device__ __forceinline__ void d_as_b(const f64x4 (&d)[RT], double (&b)[KT]) {
#pragma unroll
	for (int ks = 0; ks < KT; ks++) b[ks] = d[ks >> 2][ks & 3];
}

// ... and B fragments as they come from memory (load_b) seen as a D-layout vector.  The final k-step's rows past S - 1 were read
// from a clamped address (TileAddr::last): as a B operand they meet zero columns of the image, as a VALUE they have to be zero
template <int RT, int KT>
__device__ __forceinline__ void b_as_d(const double (&b)[KT], f64x4 (&d)[RT]) {
	constexpr int S = GenStates<RT, KT>::S;
	const int rq = (threadIdx.x & 63) >> 4;
#pragma unroll
	for (int t = 0; t < RT; t++)
#pragma unroll
		for (int r = 0; r < 4; r++) {
			const int ks = 4 * t + r;
			if (ks >= KT) d[t][r] = 0.0;
			else if (4 * ks + 3 < S) d[t][r] = b[ks];
			else d[t][r] = 4 * ks + rq < S ? b[ks] : 0.0;
		}
}

// Per-lane addressing of one 16-pattern tile in a [S][Pp] plane: byte offsets of (row lane>>4, pattern) -- every row of the
// tile is then a wave-uniform pointer plus this offset.  `last` serves the final k-step, whose rows past S - 1 are clamped to
// S - 1 (they meet zero columns of the image; reading a valid neighbour saves a branch).  Planes are < 4 GB (choose_tiles).
template <int RT, int KT>
struct TileAddr {
	unsigned off, last;
	bool ok;
	__device__ __forceinline__ TileAddr(int pat, int P, unsigned Pp) {
		constexpr int S = GenStates<RT, KT>::S;
		const unsigned rq = (threadIdx.x & 63) >> 4;
		ok = pat < P;
		const unsigned pc = ok ? (unsigned)pat : 0u;
		off = (rq * Pp + pc) * 8u;
		const unsigned rl = min(4u * (KT - 1) + rq, (unsigned)(S - 1)) - 4u * (KT - 1);
		last = (rl * Pp + pc) * 8u;
	}
};

// The row stride as a fresh scalar per tile: row pointers (plane + 4 ks Pp) are loop-invariant, and hoisted out of the tile loop
// they are 16 x 5 planes of 64-bit scalars -- SGPR spills into vector registers.  Recomputed per tile they cost scalar adds.
__device__ __forceinline__ size_t opaque_stride(int Pp) {
	int v = Pp;
	asm volatile("" : "+s"(v));
	return (size_t)(unsigned)v;
}

// partials are written once and read once or twice, launches apart: non-temporal loads and stores (plain / nt stores / nt both:
// cfg3 192 / 199 / 205 evals/s, cfg4 457 / 461 / 469)
__device__ __forceinline__ double ld_row(const double *row, unsigned byte_off) {
	return __builtin_nontemporal_load(reinterpret_cast<const double *>(reinterpret_cast<const char *>(row) + byte_off));
}
__device__ __forceinline__ void st_row(double *row, unsigned byte_off, double v) {
	__builtin_nontemporal_store(v, reinterpret_cast<double *>(reinterpret_cast<char *>(row) + byte_off));
}

// B fragments of an internal node's partial: state 4ks + (lane>>4), pattern pat
template <int RT, int KT>
__device__ __forceinline__ void load_b(const double *__restrict__ plane0, size_t Pp, const TileAddr<RT, KT> &ta, double (&b)[KT]) {
#pragma unroll
	for (int ks = 0; ks < KT; ks++) b[ks] = ld_row(plane0 + (size_t)(4 * ks) * Pp, ks == KT - 1 ? ta.last : ta.off);
}

// M . tip in D layout without MFMAs: one-hot -> column `code` of M, unknown (code S) -> row sums, code S + 1 + q -> the
// columns of ambiguity set q (a bit per state; named sets of a general data type, datatype.c:212-262) summed
template <int RT, int KT>
__device__ __forceinline__ void tip_matvec(const double *img, int S, int code, const unsigned long long *__restrict__ sets, f64x4 (&d)[RT]) {
	const int lane = threadIdx.x & 63;
	if (code > S) {
#pragma unroll
		for (int t = 0; t < RT; t++) d[t] = f64x4{0., 0., 0., 0.};
		for (unsigned long long m = sets[code - S - 1]; m; m &= m - 1) {
			const int j = __ffsll(m) - 1;
			const double *col = img + (j >> 2) * 64 + 16 * (j & 3) + (lane >> 4);
#pragma unroll
			for (int t = 0; t < RT; t++)
#pragma unroll
				for (int r = 0; r < 4; r++)
					if (!(TailRows<RT, KT>::ON && t == 1 && r > 0)) d[t][r] += col[t * KT * 64 + 4 * r];  // row i = 16 t + 4 r + (lane >> 4): i & 15 = 4 r + (lane >> 4)
		}
		return;
	}
#pragma unroll
	for (int t = 0; t < RT; t++)
#pragma unroll
		for (int r = 0; r < 4; r++) {
			const int i = 16 * t + 4 * r + (lane >> 4);
			double v;
			if (code < S) v = img[(t * KT + (code >> 2)) * 64 + (i & 15) + 16 * (code & 3)];
			else v = img[RT * KT * 64 + i];
			if (TailRows<RT, KT>::ON && t == 1 && r > 0) v = 0.0;  // rows 20..31: the tail tile repeats rows 16..19 there
			d[t][r] = v;
		}
}

// sum over states of x_i y_i z_i (z optional weights by state in D layout); every lane ends with its pattern's total
template <int RT>
__device__ __forceinline__ double state_sum(const f64x4 (&x)[RT]) {
	double s = 0.0;
#pragma unroll
	for (int t = 0; t < RT; t++) s += (x[t][0] + x[t][1]) + (x[t][2] + x[t][3]);
	s += __shfl_xor(s, 16, 64);
	s += __shfl_xor(s, 32, 64);
	return s;
}

// max over states (D layout; padded rows are 0 and partials are >= 0); every lane ends with its pattern's maximum
template <int RT>
__device__ __forceinline__ double state_max(const f64x4 (&x)[RT]) {
	double m = 0.0;
#pragma unroll
	for (int t = 0; t < RT; t++) m = fmax(m, fmax(fmax(x[t][0], x[t][1]), fmax(x[t][2], x[t][3])));
	m = fmax(m, __shfl_xor(m, 16, 64));
	m = fmax(m, __shfl_xor(m, 32, 64));
	return m;
}

// Cherry fusion is compiled for the 20-state shape only (images of 5 KB: a workgroup holds up to eight of them)
template <int RT>
struct GenFuse {
	static constexpr bool ON = RT == 2;
	// QP (20 states): the branch term of a TIP child, sum_i u_i (Qf P e_code)_i, takes the column of Qf P(t) from an image of that
	// product (k_tip_rate_products, staged like the others: four more slots for the tips on either side) instead of forming
	// Qf . (P e_code) on the matrix cores -- 200 of the 794 products of a cfg3 evaluation.  33 KB images leave no room at 60 / 61 states.
	static constexpr bool QP = RT == 2;
	static constexpr int LOWER_IMAGES = ON ? 7 : 3, UPPER_IMAGES = (ON ? 8 : 4) + (QP ? 4 : 0);  // lower: the node's own, two children, four cherry tips
};

// B fragments of a cherry's own partial: the product of its two tips' columns (D layout = B layout, see the file header)
template <int RT, int KT>
__device__ __forceinline__ void cherry_fragments(const double *img0, const double *img1, int code0, int code1, const unsigned long long *__restrict__ sets,
                                                 double (&b)[KT]) {
	constexpr int S = GenStates<RT, KT>::S;
	f64x4 g0[RT], g1[RT];
	tip_matvec<RT, KT>(img0, S, code0, sets, g0);
	tip_matvec<RT, KT>(img1, S, code1, sets, g1);
#pragma unroll
	for (int t = 0; t < RT; t++) g0[t] = g0[t] * g1[t];
	d_as_b<RT, KT>(g0, b);
}

// a lane's partial over its own states -> the pattern's total / maximum (lanes l, l+16, l+32, l+48 hold one pattern)
__device__ __forceinline__ double lanes_sum16(double s) {
	s += __shfl_xor(s, 16, 64);
	s += __shfl_xor(s, 32, 64);
	return s;
}
__device__ __forceinline__ double lanes_max16(double m) {
	m = fmax(m, __shfl_xor(m, 16, 64));
	m = fmax(m, __shfl_xor(m, 32, 64));
	return m;
}

// one row tile of a D-layout vector -> plane
template <int RT, int KT>
__device__ __forceinline__ void store_d_tile(double *__restrict__ plane0, size_t Pp, const TileAddr<RT, KT> &ta, int t, const f64x4 &d) {
	constexpr int S = GenStates<RT, KT>::S;
	const int rq = (threadIdx.x & 63) >> 4;
#pragma unroll
	for (int r = 0; r < 4; r++) {
		const int base = 16 * t + 4 * r;  // a constant once the caller's loop over t is unrolled
		if (base < S && ta.ok && (base + 3 < S || rq < S - base)) st_row(plane0 + (size_t)base * Pp, ta.off, d[r]);
	}
}

// D-layout vector -> plane: row 16 t + 4 r + (lane >> 4)
template <int RT, int KT>
__device__ __forceinline__ void store_d(double *__restrict__ plane0, size_t Pp, const TileAddr<RT, KT> &ta, const f64x4 (&d)[RT]) {
#pragma unroll
	for (int t = 0; t < RT; t++) store_d_tile<RT, KT>(plane0, Pp, ta, t, d[t]);
}

// per-lane state weights (pi_i or 1) in D layout
template <int RT>
__device__ __forceinline__ void load_state_weights(const double *__restrict__ w, int S, bool ones, f64x4 (&f)[RT]) {
	const int lane = threadIdx.x & 63;
#pragma unroll
	for (int t = 0; t < RT; t++)
#pragma unroll
		for (int r = 0; r < 4; r++) {
			const int i = 16 * t + 4 * r + (lane >> 4);
			f[t][r] = i < S ? (ones ? 1.0 : w[i]) : 0.0;
		}
}

// f[i] *= w[i] in the state layout of load_state_weights (padding states stay 0)
template <int RT>
__device__ __forceinline__ void scale_by_states(const double *__restrict__ w, int S, f64x4 (&f)[RT]) {
	const int lane = threadIdx.x & 63;
#pragma unroll
	for (int t = 0; t < RT; t++)
#pragma unroll
		for (int r = 0; r < 4; r++) {
			const int i = 16 * t + 4 * r + (lane >> 4);
			f[t][r] = i < S ? f[t][r] * w[i] : 0.0;
		}
}

// ---- post-order level: grid (pattern blocks, nodes of the level, categories) ---------------------------------
// WHAT IS STORED for 20 / 60 / 61 states: node n at lower + core(n) * C*S*Pp holds  t_n = P_n . p_n,  its partial already carried
// through its own branch (the root, which has no branch, holds p_root itself).  A parent forms p = t_l o t_r without a product for
// its internal children, and the pre-order pass reads the very same t_l as "P_l p_l" -- the product it would otherwise repeat for
// every internal child (131 of 594 products at cfg3, 98 of 394 at cfg4).  Tips are columns of their matrix images as before, a
// fused cherry (20 states) is P_y (column o column).  Callers that want p_n itself: true_lower_gen (phyamd_shard_api.inc).
// ROOT additionally writes Lc[c][pat] = w_c sum_i pi_i p_i.  SCALE: mx[op of the level][c][pat] = max_i p_i for k_scale_gen (which
// divides the stored t_n by it: the same factor).  tiles: 16-pattern tiles per wave (choose_gen_tiles)
template <int RT, int KT, bool ROOT, bool SCALE>
__global__ __launch_bounds__(GenGeo<RT>::WAVES * 64, GenGeo<RT>::MIN_WAVES_PER_SIMD) void k_lower_gen(const NodeOp *__restrict__ ops, int T, int P, int Pp_arg, int C,
                                                            const uint8_t *__restrict__ tipcode, const unsigned long long *__restrict__ tipsets,
                                                            double *__restrict__ lower, const double *__restrict__ mats, const double *__restrict__ freqs,
                                                            const double *__restrict__ props, double *__restrict__ Lc,
                                                            double *__restrict__ mx, int tiles) {
	extern __shared__ double sh[];
	using Img = MatImage<RT, KT>;
	constexpr int S = GenStates<RT, KT>::S, WV = GenGeo<RT>::WAVES;
	const NodeOp op = ops[blockIdx.y];
	const int c = blockIdx.z, lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const bool ltip = op.left < T, rtip = op.right < T;
	// fused cherries (GenFuse: 20 states): the child's partial is the product of two tip columns, taken from the images of its
	// two tips' matrices (behind the children's own in LDS) -- never stored, never loaded
	const bool lch = GenFuse<RT>::ON && op.kind_left == CH_CHERRY, rch = GenFuse<RT>::ON && op.kind_right == CH_CHERRY;
	double *imgN = sh, *imgL = sh + Img::SIZE, *imgR = sh + 2 * Img::SIZE, *imgL0 = sh + 3 * Img::SIZE, *imgL1 = sh + 4 * Img::SIZE, *imgR0 = sh + 5 * Img::SIZE,
	       *imgR1 = sh + 6 * Img::SIZE;  // (the last four: GenFuse only)
	if (!ROOT) stage_image<RT, KT>(imgN, mats + ((size_t)op.parent * C + c) * Img::SIZE);  // mats: the per-(node, category) images
	if (ltip || lch) stage_image<RT, KT>(imgL, mats + ((size_t)op.left * C + c) * Img::SIZE);  // (an internal child arrives as t_l: no matrix)
	if (rtip || rch) stage_image<RT, KT>(imgR, mats + ((size_t)op.right * C + c) * Img::SIZE);
	if (lch) {
		stage_image<RT, KT>(imgL0, mats + ((size_t)op.lt0 * C + c) * Img::SIZE);
		stage_image<RT, KT>(imgL1, mats + ((size_t)op.lt1 * C + c) * Img::SIZE);
	}
	if (rch) {
		stage_image<RT, KT>(imgR0, mats + ((size_t)op.rt0 * C + c) * Img::SIZE);
		stage_image<RT, KT>(imgR1, mats + ((size_t)op.rt1 * C + c) * Img::SIZE);
	}
	__syncthreads();
	const size_t node_sz = (size_t)C * S * Pp_arg, cat_off = (size_t)c * S * Pp_arg;
	const double *pl = (ltip || lch) ? nullptr : lower + (size_t)op.core_left * node_sz + cat_off;
	const double *pr = (rtip || rch) ? nullptr : lower + (size_t)op.core_right * node_sz + cat_off;
	double *dst = lower + (size_t)op.core_parent * node_sz + cat_off;
#pragma unroll 1
	for (int q = 0; q < tiles; q++) {
		const int tile = (blockIdx.x * tiles + q) * WV + wave;
		if (tile * 16 >= P) break;  // wave-uniform
		const int pat = tile * 16 + (lane & 15);
		const size_t Pp = opaque_stride(Pp_arg);
		const TileAddr<RT, KT> ta(pat, P, Pp);
		f64x4 a[RT], b[RT];
		double fl[KT], fr[KT];
		// every tip code of the tile up front, with the operand fragments: one memory round trip for all of them
		int cl0 = S, cl1 = S, cr0 = S, cr1 = S;
		if (ta.ok) {
			if (ltip) cl0 = tipcode[(size_t)op.left * P + pat];
			if (rtip) cr0 = tipcode[(size_t)op.right * P + pat];
			if (lch) {
				cl0 = tipcode[(size_t)op.lt0 * P + pat];
				cl1 = tipcode[(size_t)op.lt1 * P + pat];
			}
			if (rch) {
				cr0 = tipcode[(size_t)op.rt0 * P + pat];
				cr1 = tipcode[(size_t)op.rt1 * P + pat];
			}
		}
		if (pl) load_b<RT, KT>(pl, Pp, ta, fl);  // both operands in flight together
		if (pr) load_b<RT, KT>(pr, Pp, ta, fr);
		if (ltip) tip_matvec<RT, KT>(imgL, S, cl0, tipsets, a);
		else if (lch) {
			cherry_fragments<RT, KT>(imgL0, imgL1, cl0, cl1, tipsets, fl);
			mfma_matvec<RT, KT>(imgL, fl, a);
		} else b_as_d<RT, KT>(fl, a);
		if (rtip) tip_matvec<RT, KT>(imgR, S, cr0, tipsets, b);
		else if (rch) {
			cherry_fragments<RT, KT>(imgR0, imgR1, cr0, cr1, tipsets, fr);
			mfma_matvec<RT, KT>(imgR, fr, b);
		} else b_as_d<RT, KT>(fr, b);
#pragma unroll
		for (int t = 0; t < RT; t++) a[t] = a[t] * b[t];  // p_n
		if (SCALE) {
			const double m = state_max<RT>(a);
			if (ta.ok && lane < 16) mx[((size_t)blockIdx.y * C + c) * P + pat] = m;
		}
		if (ROOT) {
			store_d<RT, KT>(dst, Pp, ta, a);
			f64x4 f[RT];
			load_state_weights<RT>(freqs, S, false, f);
#pragma unroll
			for (int t = 0; t < RT; t++) a[t] = a[t] * f[t];
			const double L = state_sum<RT>(a);
			if (ta.ok && lane < 16) Lc[(size_t)c * P + pat] = props[c] * L;
		} else {
			d_as_b<RT, KT>(a, fl);
			mfma_matvec<RT, KT>(imgN, fl, b);  // t_n = P_n p_n
			store_d<RT, KT>(dst, Pp, ta, b);
		}
	}
}

// Rescale the nodes of one post-order level (grid: pattern blocks x ops): m = max over categories of mx; below the
// threshold the pattern's C*S entries are divided by m and log m joins the children's cumulative factors
// (treelikelihood.c:1790-1836).  The root's per-category site likelihoods Lc are divided too.
__global__ __launch_bounds__(256) void k_scale_gen(const NodeOp *__restrict__ ops, int P, int Pp, int S, int C, double *__restrict__ lower,
                                                  const double *__restrict__ mx, double *__restrict__ lscale, double *__restrict__ Lc_root) {
	const int k = blockIdx.x * 256 + threadIdx.x;
	if (k >= P) return;
	const NodeOp op = ops[blockIdx.y];
	double m = 0.0;
	for (int c = 0; c < C; c++) m = fmax(m, mx[((size_t)blockIdx.y * C + c) * P + k]);
	double sf = (op.core_left >= 0 ? lscale[(size_t)op.core_left * P + k] : 0.0) + (op.core_right >= 0 ? lscale[(size_t)op.core_right * P + k] : 0.0);
	if (m < SCALING_THRESHOLD) {
		double *node = lower + (size_t)op.core_parent * C * S * Pp;
		for (int cs = 0; cs < C * S; cs++) node[(size_t)cs * Pp + k] /= m;
		if (Lc_root)
			for (int c = 0; c < C; c++) Lc_root[(size_t)c * P + k] /= m;
		sf += log(m);
	}
	lscale[(size_t)op.core_parent * P + k] = sf;
}

// same for the two upper partials an op of a pre-order level wrote; their factors cancel in the gradient's ratio and
// are not kept.  mxu: [op][side][c][pat]
__global__ __launch_bounds__(256) void k_scale_upper_gen(const NodeOp *__restrict__ ops, int P, int Pp, int S, int C, double *__restrict__ upper,
                                                        const double *__restrict__ mxu) {
	const int k = blockIdx.x * 256 + threadIdx.x;
	if (k >= P) return;
	const NodeOp op = ops[blockIdx.y];
	for (int side = 0; side < 2; side++) {
		const int slot = side ? op.upper_slot_right : op.upper_slot_left;
		if (slot < 0) continue;
		double m = 0.0;
		for (int c = 0; c < C; c++) m = fmax(m, mxu[(((size_t)blockIdx.y * 2 + side) * C + c) * P + k]);
		if (m < SCALING_THRESHOLD) {
			double *node = upper + (size_t)slot * C * S * Pp;
			for (int cs = 0; cs < C * S; cs++) node[(size_t)cs * Pp + k] /= m;
		}
	}
}

// Rescaled branch gradient of one pre-order level: g[child][c] = sum_k w_k num[child][c][k] / D_k with
// D_k = sum_c w_c den[c][k] the site likelihood in this branch's scaled units (COMPAT: den[c][k] alone, as
// treelikelihood.c:2851-2870).  nd: [op][num_l, num_r, den][c][pat]; one workgroup per gradient slab block.
template <bool COMPAT>
__global__ __launch_bounds__(256) void k_scaled_gradient_gen(const NodeOp *__restrict__ ops, int P, int C, int ppb, const double *__restrict__ nd,
                                                            const double *__restrict__ weights, const double *__restrict__ props,
                                                            double *__restrict__ gpart, int nblk) {
	__shared__ double red[4][2];
	const NodeOp op = ops[blockIdx.y];
	const double *base = nd + (size_t)blockIdx.y * 3 * C * P;
	const int k0 = blockIdx.x * ppb, k1 = min(P, k0 + ppb);
	for (int c = 0; c < C; c++) {
		double gl = 0.0, gr = 0.0;
		for (int k = k0 + threadIdx.x; k < k1; k += 256) {
			double D;
			if (COMPAT) D = base[((size_t)2 * C + c) * P + k];
			else {
				D = 0.0;
				for (int cc = 0; cc < C; cc++) D += props[cc] * base[((size_t)2 * C + cc) * P + k];
			}
			const double w = weights[k];
			gl += w * (base[(size_t)c * P + k] / D);
			gr += w * (base[((size_t)C + c) * P + k] / D);
		}
		const double sl = wave_sum(gl), sr = wave_sum(gr);
		__syncthreads();
		if ((threadIdx.x & 63) == 0) {
			red[threadIdx.x >> 6][0] = sl;
			red[threadIdx.x >> 6][1] = sr;
		}
		__syncthreads();
		if (threadIdx.x == 0) {
			gpart[((size_t)op.left * C + c) * nblk + blockIdx.x] = (red[0][0] + red[1][0]) + (red[2][0] + red[3][0]);
			gpart[((size_t)op.right * C + c) * nblk + blockIdx.x] = (red[0][1] + red[1][1]) + (red[2][1] + red[3][1]);
		}
	}
}

// HESS rows of one pre-order level -> the Hessian slab: per pattern D = sum_c w_c den_c, A = sum_c w_c r_c num_c,
// B = sum_c w_c r_c^2 num2_c (the branch's units cancel in both ratios), and per workgroup the sums of w_k A / D and
// w_k (B / D - (A / D)^2) of both children.  Workgroup x takes the 64-pattern blocks [hwg[2x], hwg[2x + 1]) like the 4-state pass,
// so the slab does not depend on the shard count.  nd: [op][5][c][pat]; hpart: [workgroup][2 N].
__global__ __launch_bounds__(256) void k_hess_gen(const NodeOp *__restrict__ ops, int P, int C, int N, const double *__restrict__ nd,
                                                 const double *__restrict__ weights, const double *__restrict__ props, const double *__restrict__ rates,
                                                 const int *__restrict__ hwg, double *__restrict__ hpart) {
	__shared__ double red[4][4];
	const NodeOp op = ops[blockIdx.y];
	const double *base = nd + (size_t)blockIdx.y * 5 * C * P;
	const int k0 = hwg[2 * blockIdx.x] * 64, k1 = min(P, hwg[2 * blockIdx.x + 1] * 64);
	double acc[4] = {0.0, 0.0, 0.0, 0.0};  // d1_l, d1_r, d2_l, d2_r
	for (int k = k0 + threadIdx.x; k < k1; k += 256) {
		double D = 0.0, Al = 0.0, Ar = 0.0, Bl = 0.0, Br = 0.0;
		for (int c = 0; c < C; c++) {
			const double w = props[c], wr = w * rates[c], wr2 = wr * rates[c];
			D += w * base[((size_t)2 * C + c) * P + k];
			Al += wr * base[(size_t)c * P + k];
			Ar += wr * base[((size_t)C + c) * P + k];
			Bl += wr2 * base[((size_t)3 * C + c) * P + k];
			Br += wr2 * base[((size_t)4 * C + c) * P + k];
		}
		const double w = weights[k], al = Al / D, ar = Ar / D;
		acc[0] += w * al;
		acc[1] += w * ar;
		acc[2] += w * (Bl / D - al * al);
		acc[3] += w * (Br / D - ar * ar);
	}
	for (int j = 0; j < 4; j++) {
		const double s = wave_sum(acc[j]);
		if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][j] = s;
	}
	__syncthreads();
	if (threadIdx.x < 4) {
		const int j = threadIdx.x, node = (j & 1) ? op.right : op.left;
		hpart[(size_t)blockIdx.x * 2 * N + (j >> 1) * N + node] = (red[0][j] + red[1][j]) + (red[2][j] + red[3][j]);
	}
}

// lnL_k = log sum_c Lc[c][k] (+ the root's cumulative log scale factor), w_k / L_k, and the fixed-order partial sums of
// w_k lnL_k (treelikelihood.c:1473-1487)
__global__ __launch_bounds__(256) void k_root_finish(int P, int C, const double *__restrict__ Lc, const double *__restrict__ weights,
                                                    const double *__restrict__ lscale_root, double *__restrict__ pattern_lk,
                                                    double *__restrict__ w_over_L, double *__restrict__ lnl_part) {
	__shared__ double red[4];
	const int k = blockIdx.x * 256 + threadIdx.x;
	double acc = 0.0;
	if (k < P) {
		double L = 0.0;
		for (int c = 0; c < C; c++) L += Lc[(size_t)c * P + k];
		const double lk = log(L) + (lscale_root ? lscale_root[k] : 0.0), w = weights[k];
		pattern_lk[k] = lk;
		w_over_L[k] = w / L;
		acc = lk * w;
	}
	const double s = wave_sum(acc);
	if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
	__syncthreads();
	if (threadIdx.x == 0) lnl_part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// ---- pre-order level with the fused branch gradient: grid (pattern blocks, parents of the level, categories) -----
// Qf: the image of diag(f) Q with f = pi, or of Q when pi is folded into the uppers (FOLD): the state weights of the final sum
// ride in the product (num_l = sum_i u_l,i (Qf bl)_i) instead of in registers.
// The plain kernel accumulates w_k / L_k-weighted sums per LANE (a lane holds 4 RT states of its pattern) and adds the lanes
// once, after the tile loop.  SCALE: the per-pattern numerators and denominator go to nd[op][num_l, num_r, den][c][pat] and the
// maxima of the two new uppers to mxu[op][side][c][pat] instead.
// A fused cherry below an op of the pre-order pass: its upper u (just formed, in registers) goes down through its own branch and
// meets the two tips; the branch terms of the two tip branches join the per-lane sums g0 / g1.  Same products, in the same order,
// as the cherry's own op would form from the stored upper.
template <int RT, int KT>
__device__ __forceinline__ void cherry_gradient(const double *imgY, const double *img0, const double *img1, const double *imgQ, const f64x4 (&u)[RT], int code0,
                                                int code1, const unsigned long long *__restrict__ sets, double wl, double &g0, double &g1,
                                                const double *qp0, const double *qp1) {
	constexpr int S = GenStates<RT, KT>::S;
	// register-lean order (three 2 RT-register vectors live at a time; the 20-state kernel has 128 registers per lane): a tip
	// column is eight LDS reads, so b0 is read again for the second term instead of being kept across two products
	f64x4 a2[RT], b[RT], tmp[RT];
	double frag[KT];
	d_as_b<RT, KT>(u, frag);
	mfma_matvec<RT, KT>(imgY, frag, a2);
	if (GenFuse<RT>::QP) tip_matvec<RT, KT>(qp0, S, code0, sets, tmp);  // Qf b0 = column code0 of the image of Qf P0
	else {
		tip_matvec<RT, KT>(img0, S, code0, sets, b);
		d_as_b<RT, KT>(b, frag);
		mfma_matvec<RT, KT>(imgQ, frag, tmp);  // Qf b0
	}
	tip_matvec<RT, KT>(img1, S, code1, sets, b);
	double s0 = 0.0, s1 = 0.0;
#pragma unroll
	for (int t = 0; t < RT; t++) {
		const f64x4 m = tmp[t] * (a2[t] * b[t]);
		s0 += (m[0] + m[1]) + (m[2] + m[3]);
	}
	g0 += wl * s0;
	if (GenFuse<RT>::QP) tip_matvec<RT, KT>(qp1, S, code1, sets, tmp);
	else {
		d_as_b<RT, KT>(b, frag);
		mfma_matvec<RT, KT>(imgQ, frag, tmp);  // Qf b1
	}
	tip_matvec<RT, KT>(img0, S, code0, sets, b);
#pragma unroll
	for (int t = 0; t < RT; t++) {
		const f64x4 m = tmp[t] * (a2[t] * b[t]);
		s1 += (m[0] + m[1]) + (m[2] + m[3]);
	}
	g1 += wl * s1;
}

// HESS (phyamd_branch_hessian_diagonal): rows in every evaluation, rescaled or not, and two more per op:
// nd[op][num_l, num_r, den, num2_l, num2_r][c][pat], num2 = sum_i u_i (Qf Q b)_i, formed as Qf (diag(1 / pi) (Qf b)) with the
// Qf b the gradient term has just formed and the staged image of Qf (invf = 1 / pi; no fifth image: a 60 / 61-state one does not
// fit next to the four in LDS).  Unfused schedules only; k_hess_gen mixes the categories.  No occupancy bound: at 61 states the
// second product does not fit in the two-waves-per-SIMD register budget.
template <int RT, int KT, bool FOLD, bool SCALE, bool HESS>
__global__ __launch_bounds__(GenGeo<RT>::WAVES * 64, HESS ? 1 : GenGeo<RT>::MIN_WAVES_PER_SIMD) void k_upper_gen(const NodeOp *__restrict__ ops, int T, int P, int Pp_arg, int C,
                                                            const uint8_t *__restrict__ tipcode, const unsigned long long *__restrict__ tipsets,
                                                            const double *__restrict__ lower, double *__restrict__ upper, const double *__restrict__ mats,
                                                            const double *__restrict__ Qf, const double *__restrict__ freqs,
                                                            const double *__restrict__ w_over_L, double *__restrict__ gpart, int nblk,
                                                            double *__restrict__ nd, double *__restrict__ mxu, int tiles, const double *__restrict__ qp,
                                                            const double *__restrict__ invf) {
	static_assert(!HESS || !FOLD, "the Hessian variant is the reference's unfolded arithmetic");
	extern __shared__ double sh[];
	using Img = MatImage<RT, KT>;
	constexpr int S = GenStates<RT, KT>::S, WV = GenGeo<RT>::WAVES, NIMG = GenFuse<RT>::UPPER_IMAGES;
	constexpr bool FUSE = GenFuse<RT>::ON && !SCALE && !HESS;  // (rescaled evaluations and the Hessian run the unfused schedule)
	constexpr bool ROWS = SCALE || HESS;  // per-pattern rows instead of per-lane sums
	const NodeOp op = ops[blockIdx.y];
	const int c = blockIdx.z, lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const bool ltip = op.left < T, rtip = op.right < T, proot = op.upper_slot_parent < 0;
	const bool lch = FUSE && op.kind_left == CH_CHERRY, rch = FUSE && op.kind_right == CH_CHERRY;
	double *imgP = sh, *imgL = sh + Img::SIZE, *imgR = sh + 2 * Img::SIZE, *imgQ = sh + 3 * Img::SIZE;
	double *imgL0 = sh + 4 * Img::SIZE, *imgL1 = sh + 5 * Img::SIZE, *imgR0 = sh + 6 * Img::SIZE, *imgR1 = sh + 7 * Img::SIZE;  // FUSE only
	constexpr bool QP = GenFuse<RT>::QP;
	double *imgQL0 = sh + (NIMG - 4) * Img::SIZE, *imgQL1 = sh + (NIMG - 3) * Img::SIZE, *imgQR0 = sh + (NIMG - 2) * Img::SIZE, *imgQR1 = sh + (NIMG - 1) * Img::SIZE;  // QP only
	double *red = sh + NIMG * Img::SIZE;
	if (!proot) stage_image<RT, KT>(imgP, mats + ((size_t)op.parent * C + c) * Img::SIZE);  // mats, Qf: images (k_matrix_images)
	if (ltip || lch) stage_image<RT, KT>(imgL, mats + ((size_t)op.left * C + c) * Img::SIZE);  // (an internal child's P_l p_l is what the post-order
	if (rtip || rch) stage_image<RT, KT>(imgR, mats + ((size_t)op.right * C + c) * Img::SIZE);  //  pass stored: k_lower_gen)
	stage_image<RT, KT>(imgQ, Qf);
	if (lch) {
		stage_image<RT, KT>(imgL0, mats + ((size_t)op.lt0 * C + c) * Img::SIZE);
		stage_image<RT, KT>(imgL1, mats + ((size_t)op.lt1 * C + c) * Img::SIZE);
	}
	if (rch) {
		stage_image<RT, KT>(imgR0, mats + ((size_t)op.rt0 * C + c) * Img::SIZE);
		stage_image<RT, KT>(imgR1, mats + ((size_t)op.rt1 * C + c) * Img::SIZE);
	}
	if (QP) {  // qp: images of Qf P(t) per (tip, category)
		if (ltip) stage_image<RT, KT>(imgQL0, qp + ((size_t)op.left * C + c) * Img::SIZE);
		if (rtip) stage_image<RT, KT>(imgQR0, qp + ((size_t)op.right * C + c) * Img::SIZE);
		if (lch) {
			stage_image<RT, KT>(imgQL0, qp + ((size_t)op.lt0 * C + c) * Img::SIZE);
			stage_image<RT, KT>(imgQL1, qp + ((size_t)op.lt1 * C + c) * Img::SIZE);
		}
		if (rch) {
			stage_image<RT, KT>(imgQR0, qp + ((size_t)op.rt0 * C + c) * Img::SIZE);
			stage_image<RT, KT>(imgQR1, qp + ((size_t)op.rt1 * C + c) * Img::SIZE);
		}
	}
	__syncthreads();
	const size_t node_sz = (size_t)C * S * Pp_arg, cat_off = (size_t)c * S * Pp_arg;
	const double *pl = (ltip || lch) ? nullptr : lower + (size_t)op.core_left * node_sz + cat_off;
	const double *pr = (rtip || rch) ? nullptr : lower + (size_t)op.core_right * node_sz + cat_off;
	const double *up = proot ? nullptr : upper + (size_t)op.upper_slot_parent * node_sz + cat_off;
	double *ul_dst = op.upper_slot_left < 0 ? nullptr : upper + (size_t)op.upper_slot_left * node_sz + cat_off;
	double *ur_dst = op.upper_slot_right < 0 ? nullptr : upper + (size_t)op.upper_slot_right * node_sz + cat_off;
	double gl = 0.0, gr = 0.0, gl0 = 0.0, gl1 = 0.0, gr0 = 0.0, gr1 = 0.0;
#pragma unroll 1
	for (int q = 0; q < tiles; q++) {
		const int tile = (blockIdx.x * tiles + q) * WV + wave;
		if (tile * 16 >= P) break;  // wave-uniform
		const int pat = tile * 16 + (lane & 15);
		const size_t Pp = opaque_stride(Pp_arg);
		const TileAddr<RT, KT> ta(pat, P, Pp);
		f64x4 a[RT], bl[RT], br[RT], tmp[RT];
		int cl0 = S, cl1 = S, cr0 = S, cr1 = S;  // every tip code of the tile (tip children, fused cherries) up front
		if (ta.ok) {
			if (ltip) cl0 = tipcode[(size_t)op.left * P + pat];
			if (rtip) cr0 = tipcode[(size_t)op.right * P + pat];
			if (lch) {
				cl0 = tipcode[(size_t)op.lt0 * P + pat];
				cl1 = tipcode[(size_t)op.lt1 * P + pat];
			}
			if (rch) {
				cr0 = tipcode[(size_t)op.rt0 * P + pat];
				cr1 = tipcode[(size_t)op.rt1 * P + pat];
			}
		}
		{
			// one fragment buffer, used in turn: with the stored children in buffers of their own -- requested together behind the
			// parent's product, or all three at the top of the tile -- the kernel spills (14 / 28 registers at 20 states, 32 / 64 at 61)
			// and loses a fifth: cfg3 2.86 -> 3.62 / 3.57 ms, cfg4 1.08 -> 1.32 / 1.35 ms
			double f0[KT];
			if (proot) load_state_weights<RT>(freqs, S, !FOLD, a);  // the root's own upper: pi if folded, else 1
			else {
				load_b<RT, KT>(up, Pp, ta, f0);
				mfma_matvec<RT, KT>(imgP, f0, a);
			}
			if (ltip) tip_matvec<RT, KT>(imgL, S, cl0, tipsets, bl);
			else if (lch) {
				cherry_fragments<RT, KT>(imgL0, imgL1, cl0, cl1, tipsets, f0);
				mfma_matvec<RT, KT>(imgL, f0, bl);
			} else {  // bl = P_l p_l as stored: a value, not the operand of a product
				load_b<RT, KT>(pl, Pp, ta, f0);
				b_as_d<RT, KT>(f0, bl);
			}
			if (rtip) tip_matvec<RT, KT>(imgR, S, cr0, tipsets, br);
			else if (rch) {
				cherry_fragments<RT, KT>(imgR0, imgR1, cr0, cr1, tipsets, f0);
				mfma_matvec<RT, KT>(imgR, f0, br);
			} else {
				load_b<RT, KT>(pr, Pp, ta, f0);
				b_as_d<RT, KT>(f0, br);
			}
		}
		const double wl = (!ROWS && ta.ok) ? w_over_L[pat] : 0.0;
		const size_t ndo = ((size_t)blockIdx.y * (HESS ? 5 : 3) * C + c) * P + pat, mxo = ((size_t)blockIdx.y * 2 * C + c) * P + pat;
		if (ROWS) {
			load_state_weights<RT>(freqs, S, FOLD, tmp);  // weights of the state sum: 1 if pi is folded into the uppers
#pragma unroll
			for (int t = 0; t < RT; t++) tmp[t] = tmp[t] * a[t] * bl[t] * br[t];
			const double den = state_sum<RT>(tmp);
			if (ta.ok && lane < 16) nd[ndo + (size_t)2 * C * P] = den;
		}
		double frag[KT];
		f64x4 uL[RT], uR[RT];  // FUSE: the uppers of fused cherries stay here
		// left child: u_l = a o br ; num_l = sum_i u_l,i (Qf bl)_i  (QP, a tip: Qf bl is a column of the image of Qf P_l)
		if (QP && ltip) tip_matvec<RT, KT>(imgQL0, S, cl0, tipsets, tmp);
		else {
			d_as_b<RT, KT>(bl, frag);
			mfma_matvec<RT, KT>(imgQ, frag, tmp);
		}
		double sl = 0.0, mxl = 0.0;
#pragma unroll
		for (int t = 0; t < RT; t++) {
			const f64x4 u = a[t] * br[t];
			if (ul_dst) store_d_tile<RT, KT>(ul_dst, Pp, ta, t, u);
			if (FUSE) uL[t] = u;
			const f64x4 m = tmp[t] * u;
			sl += (m[0] + m[1]) + (m[2] + m[3]);
			if (SCALE) mxl = fmax(mxl, fmax(fmax(u[0], u[1]), fmax(u[2], u[3])));
		}
		if (ROWS) {
			const double num = lanes_sum16(sl), m = SCALE ? lanes_max16(mxl) : 0.0;
			if (ta.ok && lane < 16) {
				nd[ndo] = num;
				if (SCALE) mxu[mxo] = m;
			}
		} else
			gl += wl * sl;
		if (HESS) {  // num2_l = sum_i u_l,i (Qf Q bl)_i; tmp still holds Qf bl
			scale_by_states<RT>(invf, S, tmp);  // diag(1 / pi) Qf b = Q b, in place (registers are short at 61 states)
			d_as_b<RT, KT>(tmp, frag);
			mfma_matvec<RT, KT>(imgQ, frag, tmp);
			double s2 = 0.0;
#pragma unroll
			for (int t = 0; t < RT; t++) {
				const f64x4 m = tmp[t] * (a[t] * br[t]);
				s2 += (m[0] + m[1]) + (m[2] + m[3]);
			}
			const double num2 = lanes_sum16(s2);
			if (ta.ok && lane < 16) nd[ndo + (size_t)3 * C * P] = num2;
		}
		// right child
		if (QP && rtip) tip_matvec<RT, KT>(imgQR0, S, cr0, tipsets, tmp);
		else {
			d_as_b<RT, KT>(br, frag);
			mfma_matvec<RT, KT>(imgQ, frag, tmp);
		}
		double sr = 0.0, mxr = 0.0;
#pragma unroll
		for (int t = 0; t < RT; t++) {
			const f64x4 u = a[t] * bl[t];
			if (ur_dst) store_d_tile<RT, KT>(ur_dst, Pp, ta, t, u);
			if (FUSE) uR[t] = u;
			const f64x4 m = tmp[t] * u;
			sr += (m[0] + m[1]) + (m[2] + m[3]);
			if (SCALE) mxr = fmax(mxr, fmax(fmax(u[0], u[1]), fmax(u[2], u[3])));
		}
		if (ROWS) {
			const double num = lanes_sum16(sr), m = SCALE ? lanes_max16(mxr) : 0.0;
			if (ta.ok && lane < 16) {
				nd[ndo + (size_t)C * P] = num;
				if (SCALE) mxu[mxo + (size_t)C * P] = m;
			}
		} else
			gr += wl * sr;
		if (HESS) {  // num2_r = sum_i u_r,i (Qf Q br)_i; tmp still holds Qf br
			scale_by_states<RT>(invf, S, tmp);  // diag(1 / pi) Qf b = Q b, in place (registers are short at 61 states)
			d_as_b<RT, KT>(tmp, frag);
			mfma_matvec<RT, KT>(imgQ, frag, tmp);
			double s2 = 0.0;
#pragma unroll
			for (int t = 0; t < RT; t++) {
				const f64x4 m = tmp[t] * (a[t] * bl[t]);
				s2 += (m[0] + m[1]) + (m[2] + m[3]);
			}
			const double num2 = lanes_sum16(s2);
			if (ta.ok && lane < 16) nd[ndo + (size_t)4 * C * P] = num2;
		}
		if (FUSE) {
			if (lch) cherry_gradient<RT, KT>(imgL, imgL0, imgL1, imgQ, uL, cl0, cl1, tipsets, wl, gl0, gl1, imgQL0, imgQL1);
			if (rch) cherry_gradient<RT, KT>(imgR, imgR0, imgR1, imgQ, uR, cr0, cr1, tipsets, wl, gr0, gr1, imgQR0, imgQR1);
		}
	}
	if (ROWS) return;  // k_scaled_gradient_gen / k_hess_gen finish the branch terms
	constexpr int NG = FUSE ? 6 : 2;
	const double sums[6] = {wave_sum(gl), wave_sum(gr), FUSE ? wave_sum(gl0) : 0.0, FUSE ? wave_sum(gl1) : 0.0, FUSE ? wave_sum(gr0) : 0.0, FUSE ? wave_sum(gr1) : 0.0};
	if (lane == 0) {
#pragma unroll
		for (int j = 0; j < NG; j++) red[wave * NG + j] = sums[j];
	}
	__syncthreads();
	if (threadIdx.x < NG) {
		const int j = threadIdx.x;
		const int node = j == 0 ? op.left : j == 1 ? op.right : j == 2 ? (lch ? op.lt0 : -1) : j == 3 ? (lch ? op.lt1 : -1) : j == 4 ? (rch ? op.rt0 : -1) : (rch ? op.rt1 : -1);
		if (node >= 0) {
			double x = red[j];
			for (int w = 1; w < WV; w++) x += red[w * NG + j];
			gpart[((size_t)node * C + c) * nblk + blockIdx.x] = x;
		}
	}
}

// [C][S][Pp] planes <-> the reference's [C][P][S] (inspection / parity only)
__global__ void k_planes_to_reference(int P, int Pp, int S, int C, const double *__restrict__ planes, double *__restrict__ out) {
	const size_t total = (size_t)C * P * S;
	for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
		const int s = idx % S;
		const int k = (idx / S) % P;
		const int c = idx / ((size_t)S * P);
		out[idx] = planes[((size_t)c * S + s) * Pp + k];
	}
}

// ---- substitution-parameter gradient for 20 / 60 / 61 states (calculate_dlnl_dQ, treelikelihood.c:2337-2583) ---------
// Runs on the stored partials of a keep-partials evaluation (every node's lower and upper partial resident); the use is
// discrete-trait models (one or a few patterns, general K-state rate matrices), so these are plain kernels, not MFMA ones.
//   den[n][k]   = sum_c w_c sum_i f_i u_n,i (P_n p_n)_i         the site likelihood in the units of branch n (any rescaling
//                                                                factors of u and p cancel against the numerator below)
//   W^{nc}_ij   = sum_k (w_k / den[n][k]) f_i u_i p_j            outer products over the patterns
//   G^{nc}      = w_c F(t_n r_c) o (U^T W U^-T),  F_ab = exp_divided_difference(l_a, l_b, t) (phyamd_device.inc)
//   d lnL / d theta = sum_ab (U^-1 dQ_theta U)_ab sum_{n,c} G^{nc}_ab      (dPdp_with_dQdp_general, gensubst.c:284-308)

// p_j of a tip from its code (state, S = unknown, S + 1 + q = ambiguity set q)
__device__ __forceinline__ double tip_indicator(int code, int S, const unsigned long long *__restrict__ sets, int j) {
	if (code < S) return code == j ? 1.0 : 0.0;
	if (code == S) return 1.0;
	return (double)((sets[code - S - 1] >> j) & 1ull);
}

// grid (pattern blocks, nodes); nodes[y] = node id (never the root)
__global__ __launch_bounds__(256) void k_param_den_gen(const int *__restrict__ nodes, int T, int P, int Pp, int S, int C, const int *__restrict__ core_index,
                                                      const uint8_t *__restrict__ tipcode, const unsigned long long *__restrict__ tipsets,
                                                      const double *__restrict__ lower, const double *__restrict__ upper,
                                                      const double *__restrict__ mats, const double *__restrict__ freqs,
                                                      const double *__restrict__ props, double *__restrict__ den) {
	const int n = nodes[blockIdx.y], k = blockIdx.x * 256 + threadIdx.x;
	if (k >= P) return;
	const size_t node_sz = (size_t)C * S * Pp;
	const int code = n < T ? tipcode[(size_t)n * P + k] : 0;
	double total = 0.0;
	for (int c = 0; c < C; c++) {
		const double *u = upper + (size_t)n * node_sz + (size_t)c * S * Pp + k;
		const double *p = n < T ? nullptr : lower + (size_t)core_index[n] * node_sz + (size_t)c * S * Pp + k;
		const double *M = mats + ((size_t)n * C + c) * S * S;
		double acc = 0.0;
		for (int i = 0; i < S; i++) {
			double m = 0.0;
			for (int j = 0; j < S; j++) m += M[i * S + j] * (p ? p[(size_t)j * Pp] : tip_indicator(code, S, tipsets, j));
			acc += freqs[i] * u[(size_t)i * Pp] * m;
		}
		total += props[c] * acc;
	}
	den[(size_t)blockIdx.y * P + k] = total;
}

constexpr int PARAM_CHUNK = 16;  // patterns staged per step

// grid (nodes, categories); dynamic LDS: 2 * max(S*S, S*(PARAM_CHUNK+1)) doubles.  Gw[(y*C + c)][a*S + b]
__global__ __launch_bounds__(256) void k_param_outer_gen(const int *__restrict__ nodes, int T, int P, int Pp, int S, int C, const int *__restrict__ core_index,
                                                        const uint8_t *__restrict__ tipcode, const unsigned long long *__restrict__ tipsets,
                                                        const double *__restrict__ lower, const double *__restrict__ upper,
                                                        const double *__restrict__ model, const double *__restrict__ freqs,
                                                        const double *__restrict__ props, const double *__restrict__ rates,
                                                        const double *__restrict__ lengths, const uint8_t *__restrict__ is_explicit,
                                                        const double *__restrict__ weights, const double *__restrict__ den, double *__restrict__ Gw) {
	extern __shared__ double sh[];
	constexpr int LD = PARAM_CHUNK + 1, MAXPAIRS = (61 * 61 + 255) / 256;
	const int n = nodes[blockIdx.x], c = blockIdx.y, S2 = S * S;
	const int region = max(S2, S * LD);
	double *A = sh, *B = sh + region;  // pattern loop: A = f u w/den [S][LD], B = p [S][LD]; epilogue: A = W, B = U^T W
	double *out = Gw + ((size_t)blockIdx.x * C + c) * S2;
	if (is_explicit[n]) {  // explicit matrices carry no eigen system to differentiate
		for (int ab = threadIdx.x; ab < S2; ab += 256) out[ab] = 0.0;
		return;
	}
	const size_t node_sz = (size_t)C * S * Pp;
	const double *u = upper + (size_t)n * node_sz + (size_t)c * S * Pp;
	const double *p = n < T ? nullptr : lower + (size_t)core_index[n] * node_sz + (size_t)c * S * Pp;
	double acc[MAXPAIRS];
#pragma unroll
	for (int m = 0; m < MAXPAIRS; m++) acc[m] = 0.0;
	for (int k0 = 0; k0 < P; k0 += PARAM_CHUNK) {
		const int cnt = min(PARAM_CHUNK, P - k0);
		__syncthreads();
		for (int idx = threadIdx.x; idx < S * PARAM_CHUNK; idx += 256) {
			const int i = idx / PARAM_CHUNK, kk = idx % PARAM_CHUNK, k = k0 + kk;
			double a = 0.0, b = 0.0;
			if (kk < cnt) {
				a = freqs[i] * u[(size_t)i * Pp + k] * (weights[k] / den[(size_t)blockIdx.x * P + k]);
				b = p ? p[(size_t)i * Pp + k] : tip_indicator(tipcode[(size_t)n * P + k], S, tipsets, i);
			}
			A[i * LD + kk] = a;
			B[i * LD + kk] = b;
		}
		__syncthreads();
#pragma unroll
		for (int m = 0; m < MAXPAIRS; m++) {
			const int ij = threadIdx.x + 256 * m;
			if (ij < S2) {
				const double *ar = A + (ij / S) * LD, *br = B + (ij % S) * LD;
				double s = acc[m];
				for (int kk = 0; kk < PARAM_CHUNK; kk++) s += ar[kk] * br[kk];
				acc[m] = s;
			}
		}
	}
	__syncthreads();
#pragma unroll
	for (int m = 0; m < MAXPAIRS; m++) {
		const int ij = threadIdx.x + 256 * m;
		if (ij < S2) A[ij] = acc[m];  // W
	}
	__syncthreads();
	const double *ev = model, *U = model + S, *Ui = model + S + S2;
	for (int aj = threadIdx.x; aj < S2; aj += 256) {  // (U^T W)_aj = sum_i U_ia W_ij
		const int a = aj / S, j = aj % S;
		double s = 0.0;
		for (int i = 0; i < S; i++) s += U[i * S + a] * A[i * S + j];
		B[aj] = s;
	}
	__syncthreads();
	const double t = lengths[n] * rates[c], w = props[c];
	for (int ab = threadIdx.x; ab < S2; ab += 256) {  // G_ab = sum_j (U^T W)_aj U^-1_bj
		const int a = ab / S, b = ab % S;
		double s = 0.0;
		for (int j = 0; j < S; j++) s += B[a * S + j] * Ui[b * S + j];
		out[ab] = w * exp_divided_difference(ev[a], ev[b], t) * s;
	}
}

// Gsum[ab] = sum over rows of Gw in row order (fixed order: reproducible)
__global__ void k_param_sum_gen(int rows, int S2, const double *__restrict__ Gw, double *__restrict__ Gsum) {
	const int ab = blockIdx.x * blockDim.x + threadIdx.x;
	if (ab >= S2) return;
	double s = 0.0;
	for (int r = 0; r < rows; r++) s += Gw[(size_t)r * S2 + ab];
	Gsum[ab] = s;
}

// out[theta] = sum_ab B_theta,ab Gsum_ab; one wave per parameter
__global__ void k_param_contract_gen(int S2, const double *__restrict__ Bm, const double *__restrict__ Gsum, double *__restrict__ out) {
	const double *row = Bm + (size_t)blockIdx.x * S2;
	double s = 0.0;
	for (int ab = threadIdx.x; ab < S2; ab += 64) s += row[ab] * Gsum[ab];
	s = wave_sum(s);
	if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// Single-branch likelihood for 20 / 60 / 61 states (see k_branch_eval4): one pattern per thread, plain loops -- the caller is
// a line search over ONE branch, and 4 S^2 multiply-adds per (pattern, category) are a few microseconds at these sizes.
// pm: [C][4][S][S] = P(t r_c), r Q P, r^2 Q Q P, and the branch's current P (used when plk != NULL: rescaled evaluations).
// part: [3][gridDim.x]
__global__ __launch_bounds__(256) void k_branch_eval_gen(int node, int T, int P, int Pp, int S, int C, const double *__restrict__ up,
                                                        const double *__restrict__ low, const uint8_t *__restrict__ tipcode,
                                                        const unsigned long long *__restrict__ tipsets, const double *__restrict__ pm,
                                                        const double *__restrict__ freqs, int fold, const double *__restrict__ props,
                                                        const double *__restrict__ weights, const double *__restrict__ plk, double *__restrict__ part) {
	__shared__ double red[3][4];
	const int k = blockIdx.x * 256 + threadIdx.x;
	const bool valid = k < P;
	double a = 0.0, b = 0.0, d = 0.0;
	if (valid) {
		const int code = low ? 0 : tipcode[(size_t)node * P + k];
		double L = 0.0, L1 = 0.0, L2 = 0.0, L0 = 0.0;
		for (int c = 0; c < C; c++) {
			const double *u = up + (size_t)c * S * Pp + k, *p = low ? low + (size_t)c * S * Pp + k : nullptr;
			const double *M = pm + (size_t)c * 4 * S * S;
			double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
			for (int i = 0; i < S; i++) {
				double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0;
				for (int j = 0; j < S; j++) {
					const double pj = p ? p[(size_t)j * Pp] : tip_indicator(code, S, tipsets, j);
					m0 += M[i * S + j] * pj;
					m1 += M[S * S + i * S + j] * pj;
					m2 += M[2 * S * S + i * S + j] * pj;
					if (plk) m3 += M[3 * S * S + i * S + j] * pj;
				}
				const double fu = (fold ? 1.0 : freqs[i]) * u[(size_t)i * Pp];
				s0 += fu * m0;
				s1 += fu * m1;
				s2 += fu * m2;
				s3 += fu * m3;
			}
			L += props[c] * s0;
			L1 += props[c] * s1;
			L2 += props[c] * s2;
			L0 += props[c] * s3;
		}
		const double w = weights[k], r1 = L1 / L, r2 = L2 / L;
		a = w * (plk ? plk[k] + log(L / L0) : log(L));
		b = w * r1;
		d = w * (r2 - r1 * r1);
	}
	a = wave_sum(a);
	b = wave_sum(b);
	d = wave_sum(d);
	if ((threadIdx.x & 63) == 0) {
		red[0][threadIdx.x >> 6] = a;
		red[1][threadIdx.x >> 6] = b;
		red[2][threadIdx.x >> 6] = d;
	}
	__syncthreads();
	if (threadIdx.x < 3) part[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = (red[threadIdx.x][0] + red[threadIdx.x][1]) + (red[threadIdx.x][2] + red[threadIdx.x][3]);
}

// The same path walk for 20 / 60 / 61 states (every internal node is stored there; siblings are stored nodes or tips): one launch
// per step, one pattern per thread, plain loops.  u_in == nullptr: the parent is the root (incoming upper = 1).
// planes [C][S][Pp]; sib: the sibling's stored array (sib_is_carried: t = P p, as the post-order pass stores it), the partial of a
// fused cherry formed on the side (sib_is_carried = 0), or nullptr for a tip (then its code row)
__global__ __launch_bounds__(256) void k_path_step_gen(int P, int Pp, int S, int C, const double *__restrict__ mat_parent, const double *__restrict__ u_in,
                                                      const double *__restrict__ mat_sib, const double *__restrict__ sib, int sib_is_carried,
                                                      const uint8_t *__restrict__ tiprow, const unsigned long long *__restrict__ tipsets, double *__restrict__ u_out) {
	const int k = blockIdx.x * 256 + threadIdx.x;
	if (k >= P) return;
	const int code = sib ? 0 : tiprow[k];
	for (int c = 0; c < C; c++) {
		const double *Mp = mat_parent ? mat_parent + (size_t)c * S * S : nullptr, *Ms = mat_sib + (size_t)c * S * S;
		const double *ui = u_in ? u_in + (size_t)c * S * Pp + k : nullptr, *ps = sib ? sib + (size_t)c * S * Pp + k : nullptr;
		double *uo = u_out + (size_t)c * S * Pp + k;
		for (int i = 0; i < S; i++) {
			double a = 1.0, b = 0.0;
			if (ui) {
				a = 0.0;
				for (int j = 0; j < S; j++) a += Mp[i * S + j] * ui[(size_t)j * Pp];
			}
			if (ps && sib_is_carried) b = ps[(size_t)i * Pp];  // a stored node: t = P p already (k_lower_gen)
			else
				for (int j = 0; j < S; j++) b += Ms[i * S + j] * (ps ? ps[(size_t)j * Pp] : tip_indicator(code, S, tipsets, j));
			uo[(size_t)i * Pp] = a * b;
		}
	}
}

// lower partial of a fused cherry (two tips, never stored by the 20-state schedule) for the callers that want it as an array:
// out[c][i][k] = (P_0 tip_0)_i (P_1 tip_1)_i, planes [C][S][Pp].  mat0 / mat1: [C][S][S] of the two tips
__global__ __launch_bounds__(256) void k_cherry_partial_gen(int P, int Pp, int S, int C, const double *__restrict__ mat0, const double *__restrict__ mat1,
                                                           const uint8_t *__restrict__ row0, const uint8_t *__restrict__ row1,
                                                           const unsigned long long *__restrict__ tipsets, double *__restrict__ out) {
	const int k = blockIdx.x * 256 + threadIdx.x;
	if (k >= P) return;
	const int c0 = row0[k], c1 = row1[k];
	for (int c = 0; c < C; c++) {
		const double *M0 = mat0 + (size_t)c * S * S, *M1 = mat1 + (size_t)c * S * S;
		for (int i = 0; i < S; i++) {
			double a = 0.0, b = 0.0;
			for (int j = 0; j < S; j++) {
				a += M0[i * S + j] * tip_indicator(c0, S, tipsets, j);
				b += M1[i * S + j] * tip_indicator(c1, S, tipsets, j);
			}
			out[((size_t)c * S + i) * Pp + k] = a * b;
		}
	}
}

// p_n of an internal node from its two children, for the callers that want the partial itself (the post-order pass stores
// t_n = P_n p_n): out[c][i][k] = T_l,i T_r,i, planes [C][S][Pp].  A child is  mode 0: a tip (code row, its matrices [C][S][S]);
// mode 1: a stored node (src = t, used as it is);  mode 2: a partial in src that still has to go through the child's matrices (a
// fused cherry formed on the side).  rescale: the node's own factor of a rescaled evaluation is applied as k_scale_gen applied it.
// One pattern per thread, plain loops: inspection, single-branch evaluation, parameter gradient
__global__ __launch_bounds__(256) void k_node_lower_gen(int P, int Pp, int S, int C, int mode_l, const double *__restrict__ mat_l, const double *__restrict__ src_l,
                                                       const uint8_t *__restrict__ row_l, int mode_r, const double *__restrict__ mat_r, const double *__restrict__ src_r,
                                                       const uint8_t *__restrict__ row_r, const unsigned long long *__restrict__ tipsets, int rescale,
                                                       double *__restrict__ out) {
	const int k = blockIdx.x * 256 + threadIdx.x;
	if (k >= P) return;
	const int code_l = mode_l == 0 ? row_l[k] : 0, code_r = mode_r == 0 ? row_r[k] : 0;
	double mx = 0.0;
	for (int c = 0; c < C; c++) {
		const double *Ml = mat_l ? mat_l + (size_t)c * S * S : nullptr, *Mr = mat_r ? mat_r + (size_t)c * S * S : nullptr;
		const double *sl = src_l ? src_l + (size_t)c * S * Pp + k : nullptr, *sr = src_r ? src_r + (size_t)c * S * Pp + k : nullptr;
		for (int i = 0; i < S; i++) {
			double a = 0.0, b = 0.0;
			if (mode_l == 1) a = sl[(size_t)i * Pp];
			else
				for (int j = 0; j < S; j++) a += Ml[i * S + j] * (mode_l == 2 ? sl[(size_t)j * Pp] : tip_indicator(code_l, S, tipsets, j));
			if (mode_r == 1) b = sr[(size_t)i * Pp];
			else
				for (int j = 0; j < S; j++) b += Mr[i * S + j] * (mode_r == 2 ? sr[(size_t)j * Pp] : tip_indicator(code_r, S, tipsets, j));
			out[((size_t)c * S + i) * Pp + k] = a * b;
			mx = fmax(mx, a * b);
		}
	}
	// a rescaled evaluation divided this node by its maximum over categories and states where that fell below the threshold
	// (k_scale_gen did it to the stored t_n; the children's own factors are in their arrays already)
	if (rescale && mx < SCALING_THRESHOLD)
		for (int cs = 0; cs < C * S; cs++) out[(size_t)cs * Pp + k] /= mx;
}

// rescaled evaluations: divide a pattern's upper by its maximum over categories and states when that is below the threshold
__global__ __launch_bounds__(256) void k_path_scale_gen(int P, int Pp, int S, int C, double *__restrict__ u) {
	const int k = blockIdx.x * 256 + threadIdx.x;
	if (k >= P) return;
	double m = 0.0;
	for (int cs = 0; cs < C * S; cs++) m = fmax(m, u[(size_t)cs * Pp + k]);
	if (m < 1.0e-40 && m > 0.0)
		for (int cs = 0; cs < C * S; cs++) u[(size_t)cs * Pp + k] /= m;
}
