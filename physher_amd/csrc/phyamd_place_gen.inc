// phyamd_place_gen.inc: 20-state kernels of phyamd_placement_log_likelihoods_general -- lnL of query sequences placed on every edge
// of the engine's tree in one call -- included by phyamd_engine.hip inside its anonymous namespace, behind phyamd_place4.inc, whose
// scheme this is (see its head for the definition and the finish).
//
// The tree side comes from the partials a keep-partials gradient leaves resident: u_n, the message at the top of edge n's branch
// (d_upper; it carries pi when the gradient folded it in), and p_n, the node's own partial (a tip: its code; an internal node:
// true_lower_gen's partial in a temporary, because a stored lower is P_n p_n: k_classplace_own).  Per (edge, category c, 16-pattern tile), with
// P_lo = P(sigma t_n r_c) and P_hi = P((1 - sigma) t_n r_c),
//   hi = P_hi^T (pi o u_n),   lo = P_lo p_n,   E_c = hi o lo
// and the site likelihood of a query whose cell has CLASS k (a state 0..19, 20 = unknown, 21 + q = the call's set q) on a pendant
// branch of length l is Y[k] = sum_c sum_z R_{l,c}[k][z] E_c,z with R_{l,c}[k][z] = w_c sum_{j in class k} P(l r_c)[z][j]: three
// 20-wide products on v_mfma_f64_16x16x4_f64, the last one accumulated over the categories in category order in the accumulator.
// w_k log Y[k] goes to table [length][edge][pattern][32]; padded patterns, patterns of weight 0 and classes without members store 0.
// k_classplace_score is k_place_score4's gather with 256-byte rows, and k_place_finish serves as it is.  No atomics.
// (The kernels are named k_classplace_*, not k_place_*: tests/test_placement_abi.py counts the kernels whose names hold "k_place"
// and expects the 4-state call's four.)

constexpr int PLACE_GEN_CLASSES = 32, PLACE_GEN_STATES = 20, PLACE_GEN_MAX_SETS = PLACE_GEN_CLASSES - PLACE_GEN_STATES - 1;
constexpr int PLACE_GEN_CLASS_IMAGE = 2 * 5 * 64;                       // doubles of a class image: two full 16-row tiles, 5 k-steps
constexpr int PLACE_GEN_BLOCK = GenGeo<2>::WAVES * 16;                  // patterns of a workgroup of the table kernel: a tile per wave
constexpr int PLACE_GEN_LENGTHS = 4;                                    // pendant lengths a workgroup holds accumulators and images for

// images of the transposes of `count` row-major 20 x 20 matrices (grid: count): stage_matrix's layout, the row sums unused
__global__ __launch_bounds__(256) void k_classplace_transposed_images(const double *__restrict__ mats, double *__restrict__ imgs) {
	constexpr int S = PLACE_GEN_STATES, KT = 5;
	const double *M = mats + (size_t)blockIdx.x * S * S;
	double *img = imgs + (size_t)blockIdx.x * MatImage<2, 5>::SIZE;
	for (int idx = threadIdx.x; idx < MatImage<2, 5>::SIZE; idx += 256) {
		double v = 0.0;
		if (idx < MatImage<2, 5>::FRAG) {
			const int lane = idx & 63, ks = (idx >> 6) % KT, t = (idx >> 6) / KT;
			const int i = t == 1 ? 16 + (lane & 3) : (lane & 15), j = 4 * ks + (lane >> 4);  // (the tail tile: stage_matrix)
			v = M[(size_t)j * S + i];
		}
		img[idx] = v;
	}
}

// class images of `count` = lengths x categories row-major matrices P(l r_c) (grid: count): A fragments of the 32 x 20 matrix
// R[k][z] = w_c sum_{j in class k} P[z][j], the members added in state order; a class no set stands for: a zero row
__global__ __launch_bounds__(256) void k_classplace_images(int C, const double *__restrict__ mats, const double *__restrict__ props, const unsigned long long *__restrict__ sets,
                                                           int set_count, double *__restrict__ imgs) {
	constexpr int S = PLACE_GEN_STATES, KT = 5;
	const double *M = mats + (size_t)blockIdx.x * S * S;
	const double w = props[blockIdx.x % C];
	double *img = imgs + (size_t)blockIdx.x * PLACE_GEN_CLASS_IMAGE;
	for (int idx = threadIdx.x; idx < PLACE_GEN_CLASS_IMAGE; idx += 256) {
		const int lane = idx & 63, ks = (idx >> 6) % KT, t = (idx >> 6) / KT;
		const int k = 16 * t + (lane & 15), z = 4 * ks + (lane >> 4);
		const unsigned long long members = k < S ? 1ull << k : k == S ? (1ull << S) - 1 : k - S - 1 < set_count ? sets[k - S - 1] : 0ull;
		double s = 0.0;
		for (int j = 0; j < S; j++)
			if ((members >> j) & 1ull) s += M[(size_t)z * S + j];
		img[idx] = w * s;
	}
}

// p_n of the internal nodes of a chunk into their temporaries: true_lower_gen's kernel (k_node_lower_gen, whose sums these are,
// child by child in state order) for many nodes in one launch instead of one launch of two workgroups per node -- 198 launches
// were 33 ms of a 33.5 ms call at 200 taxa x 512 patterns.  A child is a tip (its code row and its matrices [C][S][S]) or a stored
// node (src = P p, used as it is); a keep-partials engine has no fused cherries
struct PlaceGenOwn {
	const double *mat_l, *src_l, *mat_r, *src_r;  // src null: a tip
	const uint8_t *row_l, *row_r;
	double *out;  // planes [C][S][Pp]
};

// grid (blocks of 256 patterns, nodes, categories)
__global__ __launch_bounds__(256) void k_classplace_own(const PlaceGenOwn *__restrict__ nodes, int P, int Pp, const unsigned long long *__restrict__ tipsets) {
	constexpr int S = PLACE_GEN_STATES;
	const int k = blockIdx.x * 256 + threadIdx.x, c = blockIdx.z;
	if (k >= P) return;
	const PlaceGenOwn o = nodes[blockIdx.y];
	const int code_l = o.src_l ? 0 : o.row_l[k], code_r = o.src_r ? 0 : o.row_r[k];
	const double *Ml = o.mat_l + (size_t)c * S * S, *Mr = o.mat_r + (size_t)c * S * S;
	const double *sl = o.src_l ? o.src_l + (size_t)c * S * Pp + k : nullptr, *sr = o.src_r ? o.src_r + (size_t)c * S * Pp + k : nullptr;
	for (int i = 0; i < S; i++) {
		double a = 0.0, b = 0.0;
		if (sl) a = sl[(size_t)i * Pp];
		else
			for (int j = 0; j < S; j++) a += Ml[i * S + j] * tip_indicator(code_l, S, tipsets, j);
		if (sr) b = sr[(size_t)i * Pp];
		else
			for (int j = 0; j < S; j++) b += Mr[i * S + j] * tip_indicator(code_r, S, tipsets, j);
		o.out[((size_t)c * S + i) * Pp + k] = a * b;
	}
}

// an edge of a chunk: the node below it, its upper partial, and its own partial (null: a tip, whose codes are row n of tipcode)
struct PlaceGenEdge {
	const double *up, *own;
	int32_t n, pad[3];
};

struct PlaceTableGenArgs {
	const PlaceGenEdge *edges;  // [gridDim.y]: the chunk's
	int P, Pp, Ppad, C, L, fold, classes;  // classes: 21 + the call's sets
	const uint8_t *tipcode;     // [T][P]
	const unsigned long long *tipsets;  // the ENGINE's sets (the reference tips')
	const double *freqs, *weights;
	const double *lo, *hiT;     // [N][C][MatImage<2, 5>::SIZE]: images of P_lo and of P_hi^T
	const double *cls;          // [L][C][PLACE_GEN_CLASS_IMAGE]
	double *table;              // [L][gridDim.y][Ppad][32]
};

// grid (Ppad / PLACE_GEN_BLOCK, edges of the chunk, groups of PLACE_GEN_LENGTHS lengths), block 8 waves: a wave owns the 16-pattern
// tile blockIdx.x * 8 + wave; the categories run in order, their images staged in turn
__global__ __launch_bounds__(GenGeo<2>::WAVES * 64) void k_classplace_table(const PlaceTableGenArgs a) {
	constexpr int RT = 2, KT = 5, S = PLACE_GEN_STATES, LG = PLACE_GEN_LENGTHS;
	using Img = MatImage<RT, KT>;
	__shared__ double sh[2 * Img::SIZE + LG * PLACE_GEN_CLASS_IMAGE];
	double *imgLo = sh, *imgHi = sh + Img::SIZE, *imgR = sh + 2 * Img::SIZE;
	const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), rq = lane >> 4;
	const PlaceGenEdge ed = a.edges[blockIdx.y];
	const int l0 = blockIdx.z * LG, nl = min(LG, a.L - l0);
	const int pat = (blockIdx.x * GenGeo<RT>::WAVES + wave) * 16 + (lane & 15);
	const size_t Pp = (size_t)a.Pp;
	const TileAddr<RT, KT> ta(pat, a.P, (unsigned)a.Pp);  // (a pattern past the last reads pattern 0 and stores 0)
	const int code = !ed.own && ta.ok ? a.tipcode[(size_t)ed.n * a.P + pat] : S;
	f64x4 fpi[RT];
	load_state_weights<RT>(a.freqs, S, a.fold != 0, fpi);  // pi, or ones when the uppers carry it
	f64x4 Y[LG][RT];
#pragma unroll
	for (int l = 0; l < LG; l++)
#pragma unroll
		for (int t = 0; t < RT; t++) Y[l][t] = f64x4{0., 0., 0., 0.};
#pragma unroll 1
	for (int c = 0; c < a.C; c++) {
		__syncthreads();  // (the previous category's images have been read)
		stage_image<RT, KT>(imgLo, a.lo + ((size_t)ed.n * a.C + c) * Img::SIZE);
		stage_image<RT, KT>(imgHi, a.hiT + ((size_t)ed.n * a.C + c) * Img::SIZE);
		for (int l = 0; l < nl; l++) {
			const double *src = a.cls + ((size_t)(l0 + l) * a.C + c) * PLACE_GEN_CLASS_IMAGE;
			for (int i = threadIdx.x; i < PLACE_GEN_CLASS_IMAGE; i += GenGeo<RT>::WAVES * 64) imgR[l * PLACE_GEN_CLASS_IMAGE + i] = src[i];
		}
		__syncthreads();
		f64x4 hi[RT], lo[RT];
		double frag[KT];
		{
			load_b<RT, KT>(ed.up + (size_t)c * S * Pp, Pp, ta, frag);
			f64x4 u[RT];
			b_as_d<RT, KT>(frag, u);
#pragma unroll
			for (int t = 0; t < RT; t++) u[t] = u[t] * fpi[t];
			d_as_b<RT, KT>(u, frag);
			mfma_matvec<RT, KT>(imgHi, frag, hi);
		}
		if (ed.own) {
			load_b<RT, KT>(ed.own + (size_t)c * S * Pp, Pp, ta, frag);
			mfma_matvec<RT, KT>(imgLo, frag, lo);
		} else
			tip_matvec<RT, KT>(imgLo, S, code, a.tipsets, lo);
#pragma unroll
		for (int t = 0; t < RT; t++) hi[t] = hi[t] * lo[t];  // E_c (rows 20..31 are zero in both)
		d_as_b<RT, KT>(hi, frag);
#pragma unroll
		for (int l = 0; l < LG; l++) {
			if (l >= nl) break;  // (uniform over the workgroup)
#pragma unroll
			for (int t = 0; t < RT; t++)
#pragma unroll
				for (int ks = 0; ks < KT; ks++)
					Y[l][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(imgR[l * PLACE_GEN_CLASS_IMAGE + (t * KT + ks) * 64 + lane], frag[ks], Y[l][t], 0, 0, 0);
		}
		__builtin_amdgcn_sched_barrier(0);
	}
	const double w = ta.ok ? a.weights[pat] : 0.0;
#pragma unroll
	for (int l = 0; l < LG; l++) {
		if (l >= nl) break;
		double *row = a.table + (((size_t)(l0 + l) * gridDim.y + blockIdx.y) * a.Ppad + pat) * PLACE_GEN_CLASSES;
#pragma unroll
		for (int t = 0; t < RT; t++)
#pragma unroll
			for (int r = 0; r < 4; r++) {
				const int k = 16 * t + 4 * r + rq;  // the class of register r of tile t
				row[k] = k < a.classes && w != 0.0 ? w * log(Y[l][t][r]) : 0.0;
			}
	}
}

// raw [Q][P] (the caller's rows) -> packed [Ppad / 8][Q] as k_place_masks packs them; patterns past the last: 20 (their table rows
// hold 0)
__global__ __launch_bounds__(256) void k_classplace_codes(int Q, int P, int groups, const uint8_t *__restrict__ raw, unsigned long long *__restrict__ packed) {
	const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (idx >= (size_t)groups * Q) return;
	const int q = (int)(idx % Q), g = (int)(idx / Q);
	unsigned long long word = 0;
	for (int b = 0; b < 8; b++) {
		const int k = g * 8 + b;
		const unsigned long long m = k < P ? raw[(size_t)q * P + k] : (unsigned long long)PLACE_GEN_STATES;
		word |= m << (8 * b);
	}
	packed[idx] = word;
}

// grid (blocks of blockDim.x queries, groups of PLACE_EDGES edges, segments * L), block (64 .. 1024): a lane is a query.
// k_place_score4 with rows of 32 classes (PlaceScoreArgs: table [L][E][Ppad][32]); every lane of a wave reads inside the same
// 256-byte row
__global__ __launch_bounds__(PLACE_MAX_QUERIES) void k_classplace_score(const PlaceScoreArgs a) {
	constexpr int W = PLACE_GEN_CLASSES;
	__shared__ double tile[PLACE_EDGES * PLACE_TILE * W];
	const int seg = blockIdx.z % a.segments, l = blockIdx.z / a.segments;
	const int e0 = blockIdx.y * PLACE_EDGES;
	const int q = blockIdx.x * blockDim.x + threadIdx.x, qc = q < a.Q ? q : a.Q - 1;
	const int kbegin = seg * REWEIGHT_SEGMENT, kend = min(kbegin + REWEIGHT_SEGMENT, a.Ppad);
	double acc[PLACE_EDGES];
#pragma unroll
	for (int j = 0; j < PLACE_EDGES; j++) acc[j] = 0.0;
	for (int kt = kbegin; kt < kend; kt += PLACE_TILE) {
		__syncthreads();  // (the previous tile has been read)
#pragma unroll
		for (int j = 0; j < PLACE_EDGES; j++) {
			const int e = min(e0 + j, a.E - 1);  // (past the last edge: a copy of it, never stored)
			const double2 *src = reinterpret_cast<const double2 *>(a.table + (((size_t)l * a.E + e) * a.Ppad + kt) * W);
			double2 *dst = reinterpret_cast<double2 *>(tile + j * PLACE_TILE * W);
			for (int i = threadIdx.x; i < PLACE_TILE * W / 2; i += blockDim.x) dst[i] = src[i];
		}
		__syncthreads();
		const unsigned long long *words = a.packed + (size_t)(kt / 8) * a.Q + qc;
#pragma unroll 2
		for (int g = 0; g < PLACE_TILE / 8; g++) {
			const unsigned long long word = words[(size_t)g * a.Q];
#pragma unroll
			for (int b = 0; b < 8; b++) {
				const int m = (int)(word >> (8 * b)) & (W - 1);
#pragma unroll
				for (int j = 0; j < PLACE_EDGES; j++) acc[j] += tile[(j * PLACE_TILE + g * 8 + b) * W + m];
			}
		}
	}
	if (q >= a.Q) return;
#pragma unroll
	for (int j = 0; j < PLACE_EDGES; j++)
		if (e0 + j < a.E) a.slab[(((size_t)seg * a.L + l) * a.E + e0 + j) * a.Q + q] = acc[j];
}
