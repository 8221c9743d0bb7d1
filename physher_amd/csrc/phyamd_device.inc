// phyamd_device.inc: device helpers, matrix/table kernels, the 4-state context shared by every 4-state kernel, reductions -- included by phyamd_engine.hip inside its anonymous namespace.

// ------------------------------------------------------------------------------------------------
// device helpers
// ------------------------------------------------------------------------------------------------

struct d4 {
	double x, y, z, w;
};

__device__ __forceinline__ d4 load4(const double *p) {
	// 32 contiguous bytes per lane: two 16-byte loads (global_load_dwordx4)
	const double2 a = reinterpret_cast<const double2 *>(p)[0];
	const double2 b = reinterpret_cast<const double2 *>(p)[1];
	return d4{a.x, a.y, b.x, b.y};
}

__device__ __forceinline__ void store4(double *p, const d4 &v) {
	reinterpret_cast<double2 *>(p)[0] = double2{v.x, v.y};
	reinterpret_cast<double2 *>(p)[1] = double2{v.z, v.w};
}

// Once-read / once-written streams (stored partials in the tree-walk kernels and child_message): non-temporal accesses.
// A/B at 1000 x 1e6 x 4 x 4 (two runs each): plain 49.7 / 49.8 ms per evaluation, nt loads 49.1 / 49.6, nt stores 48.9,
// both 49.2 / 49.0 -- a per-cent, kept because these bytes are never re-read from cache
typedef double dv2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ d4 load4_stream(const double *p) {
	const dv2 a = __builtin_nontemporal_load(reinterpret_cast<const dv2 *>(p));
	const dv2 b = __builtin_nontemporal_load(reinterpret_cast<const dv2 *>(p) + 1);
	return d4{a.x, a.y, b.x, b.y};
}
__device__ __forceinline__ void store4_stream(double *p, const d4 &v) {
	__builtin_nontemporal_store(dv2{v.x, v.y}, reinterpret_cast<dv2 *>(p));
	__builtin_nontemporal_store(dv2{v.z, v.w}, reinterpret_cast<dv2 *>(p) + 1);
}

// tip vector from a 4-bit ambiguity mask (one-hot for a known state, 0xF for a gap: datatype.h:26-66)
__device__ __forceinline__ d4 mask4(unsigned m) {
	return d4{(m & 1u) ? 1.0 : 0.0, (m & 2u) ? 1.0 : 0.0, (m & 4u) ? 1.0 : 0.0, (m & 8u) ? 1.0 : 0.0};
}

// Pointer into the AMDGPU constant address space: loads through it with a wave-uniform address become
// s_load_dwordx* into SGPRs (kernel inputs that no kernel of the same launch writes: matrices, Q, pi, weights).
typedef const __attribute__((address_space(4))) double *cptr;
__device__ __forceinline__ cptr as_const(const double *p) { return (cptr)p; }

// y = M v, M row-major 4x4 at a wave-uniform address (scalar loads)
__device__ __forceinline__ d4 matvec4(cptr M, const d4 &v) {
	d4 r;
	r.x = M[0] * v.x + M[1] * v.y + M[2] * v.z + M[3] * v.w;
	r.y = M[4] * v.x + M[5] * v.y + M[6] * v.z + M[7] * v.w;
	r.z = M[8] * v.x + M[9] * v.y + M[10] * v.z + M[11] * v.w;
	r.w = M[12] * v.x + M[13] * v.y + M[14] * v.z + M[15] * v.w;
	// Fence the scheduler: without it every s_load_dwordx16 of a basic block is hoisted to its top (10 matrices = 320
	// SGPRs in the fringe paths) and the overflow is parked in VGPR lanes (v_writelane / v_readlane around every use).
	__builtin_amdgcn_sched_barrier(0);
	return r;
}
// FENCE = false: the plain pre-order tree walk keeps few scalars live and gains ~2 % from free scheduling (its
// parameter-gradient variant does not: more live scalars, SGPR spills again)
template <bool FENCE>
__device__ __forceinline__ d4 matvec4_opt(cptr M, const d4 &v) {
	d4 r;
	r.x = M[0] * v.x + M[1] * v.y + M[2] * v.z + M[3] * v.w;
	r.y = M[4] * v.x + M[5] * v.y + M[6] * v.z + M[7] * v.w;
	r.z = M[8] * v.x + M[9] * v.y + M[10] * v.z + M[11] * v.w;
	r.w = M[12] * v.x + M[13] * v.y + M[14] * v.z + M[15] * v.w;
	if (FENCE) __builtin_amdgcn_sched_barrier(0);
	return r;
}

__device__ __forceinline__ d4 mul4(const d4 &a, const d4 &b) { return d4{a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w}; }
__device__ __forceinline__ double max4(const d4 &a) { return fmax(fmax(a.x, a.y), fmax(a.z, a.w)); }
__device__ __forceinline__ double dot4(const d4 &a, const d4 &b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }

// fixed-order sum over the 64 lanes of a wave; every lane ends with the total
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
	return v;
}

// v + (the value of the lane whose index differs in bit 0 / bit 1), exchanged inside each quad with DPP quad_perm moves
// (two v_mov_b32_dpp + one v_add_f64) instead of a ds_bpermute round trip through the LDS crossbar
template <int PERM>  // quad_perm selector: 0xB1 = [1,0,3,2] (xor 1), 0x4E = [2,3,0,1] (xor 2)
__device__ __forceinline__ double quad_swap_add(double v) {
	const int lo = __double2loint(v), hi = __double2hiint(v);
	const int olo = __builtin_amdgcn_update_dpp(0, lo, PERM, 0xF, 0xF, true);
	const int ohi = __builtin_amdgcn_update_dpp(0, hi, PERM, 0xF, 0xF, true);
	return v + __hiloint2double(ohi, olo);
}

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also drains the vector-memory counter (s_waitcnt vmcnt(0)):
// inside the per-op exchange of the rescaled tree walks that made every op wait for its own stores to be acknowledged.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// Make a wave-uniform pointer opaque to the optimiser.  The matrices are loop-invariant inside the
// pattern-group loop; without this LLVM hoists all of them out of the loop, runs out of SGPRs and
// parks them in VGPR lanes (v_writelane/v_readlane pairs around every use).  Re-issuing the scalar
// loads per group costs a few s_load_dwordx16 from the scalar cache instead.
__device__ __forceinline__ cptr opaque(cptr p) {
	asm volatile("" : "+s"(p));
	return p;
}

// ------------------------------------------------------------------------------------------------
// M1/M2: P(t) and dP/dt for every (node, category) from the eigen system (substmodel.c:518-557, 695-723)
// ------------------------------------------------------------------------------------------------
// model layout: eval[S] | evec[S*S] | ivec[S*S]
__global__ void k_transition_matrices(int S, int C, int node_count, const double *__restrict__ model, const double *__restrict__ rates,
                                      const double *__restrict__ lengths, const uint8_t *__restrict__ is_explicit, int root,
                                      double *__restrict__ mats, double *__restrict__ dmats) {
	const size_t total = (size_t)node_count * C * S * S;
	const double *eval = model, *evec = model + S, *ivec = model + S + S * S;
	for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
		const int j = idx % S;
		const int i = (idx / S) % S;
		const int c = (idx / ((size_t)S * S)) % C;
		const int n = idx / ((size_t)S * S * C);
		if (n == root || is_explicit[n]) continue;
		const double t = lengths[n] * rates[c];
		double p = 0., dp = 0.;
		for (int k = 0; k < S; k++) {
			const double e = exp(eval[k] * t);
			const double w = ivec[k * S + j] * evec[i * S + k];
			p += w * e;
			dp += w * (eval[k] * e);
		}
		mats[idx] = fabs(p);  // substmodel.c:552
		dmats[idx] = dp;
	}
}

// Tip messages, 4 states: for every (tip, category) the 16 vectors  P(t) . mask  (mask = 4-bit ambiguity code) are
// tabulated once per evaluation, so "transition matrix times tip vector" is one 32-byte gather per (tip, pattern)
// instead of 16 multiply-adds: tiptab[tip][c][mask][i] = sum_j P[i][j] bit_j(mask).  2 MB at 1000 taxa x 4 categories.
__global__ void k_tip_tables(int T, int C, const double *__restrict__ mats, double *__restrict__ tiptab) {
	const int idx = blockIdx.x * blockDim.x + threadIdx.x;
	if (idx >= T * C * 64) return;
	const int i = idx & 3, m = (idx >> 2) & 15, tc = idx >> 6;  // tc = tip * C + c
	const double *M = mats + (size_t)tc * 16 + i * 4;
	double s = 0.0;
	if (m & 1) s += M[0];
	if (m & 2) s += M[1];
	if (m & 4) s += M[2];
	if (m & 8) s += M[3];
	tiptab[idx] = s;
}

// F_ab(t) = (e^{l_a t} - e^{l_b t}) / (l_a - l_b), the divided difference of exp(l t) that dP/dtheta weighs U^-1 dQ U with, and its
// limit t e^{l_a t} where l_a == l_b.  Formed as e^{hi t} (1 - e^{-(hi - lo) t}) / (hi - lo) with expm1: an eigen solver returns a
// repeated eigenvalue (K80, F81, any GTR near them) split by an ulp or so, where the quotient of the two differences is rounding
// noise -- the reference's form (dPdp_with_dQdp, substmodel.c:478) and its l_a == l_b test do not survive that.  With the larger
// eigenvalue in front nothing overflows on a saturated branch: e^{hi t} <= 1 and the bracket lies in [0, 1].
__device__ __forceinline__ double exp_divided_difference(double la, double lb, double t) {
	const double hi = fmax(la, lb), d = hi - fmin(la, lb), eh = exp(hi * t);
	return d != 0.0 ? eh * (-expm1(-d * t) / d) : t * eh;
}

// G2: dP/dtheta for every (parameter, node, category) from B_theta = U^-1 (dQ/dtheta) U:
//   dP = U ( B o F(t) ) U^-1,  F_ab = exp_divided_difference(l_a, l_b, t)
// (the structure of dPdp_with_dQdp, substmodel.c:469-489).  dpm: [NP][N][C][S][S]; root and explicit-matrix nodes get zeros.
__global__ void k_parameter_matrices(int S, int C, int node_count, int np, const double *__restrict__ model, const double *__restrict__ B,
                                     const double *__restrict__ rates, const double *__restrict__ lengths,
                                     const uint8_t *__restrict__ is_explicit, int root, double *__restrict__ dpm) {
	const size_t per = (size_t)node_count * C * S * S, total = per * np;
	const double *eval = model, *evec = model + S, *ivec = model + S + S * S;
	for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
		const int j = idx % S;
		const int i = (idx / S) % S;
		const int c = (idx / ((size_t)S * S)) % C;
		const int n = (idx / ((size_t)S * S * C)) % node_count;
		const int th = idx / per;
		double v = 0.0;
		if (n != root && !is_explicit[n]) {
			const double t = lengths[n] * rates[c];
			const double *Bt = B + (size_t)th * S * S;
			for (int a = 0; a < S; a++) {
				double row = 0.0;
				for (int b = 0; b < S; b++) row += Bt[a * S + b] * exp_divided_difference(eval[a], eval[b], t) * ivec[b * S + j];
				v += evec[i * S + a] * row;
			}
		}
		dpm[idx] = v;
	}
}

// tip tables of dP/dtheta, like k_tip_tables: dptab[th][tip][c][mask][i] = sum_j dP_th[tip][c][i][j] bit_j(mask)
__global__ void k_parameter_tip_tables(int T, int N, int C, int np, const double *__restrict__ dpm, double *__restrict__ dptab) {
	const int idx = blockIdx.x * blockDim.x + threadIdx.x;
	if (idx >= np * T * C * 64) return;
	const int i = idx & 3, m = (idx >> 2) & 15, tc = (idx >> 6) % (T * C), th = (idx >> 6) / (T * C);
	const double *M = dpm + ((size_t)th * N * C + tc) * 16 + i * 4;
	double s = 0.0;
	if (m & 1) s += M[0];
	if (m & 2) s += M[1];
	if (m & 4) s += M[2];
	if (m & 8) s += M[3];
	dptab[idx] = s;
}

// ------------------------------------------------------------------------------------------------
// 4-state kernels.  Workgroup = (64 lanes = patterns) x (C waves = categories) x (G pattern groups);
// a wave's category is uniform, so its 4x4 matrices live in SGPRs and feed v_fma_f64 directly.
// Cross-category quantities (rescaling max, mixture sums) go through a small LDS exchange.
//
// Fringe fusion: an internal node whose subtree is a cherry (tip, tip) or a cherry plus a tip is never written to
// HBM.  Wherever its partial is needed it is recomputed from 2-3 tip bytes in registers, and in the pre-order pass
// its upper partial is pushed down through it in registers, yielding the gradients of its 2-4 inner branches in the
// same kernel.  Half of the internal nodes of a random tree are of these two shapes, so both passes move about half
// the bytes.  (The unfused schedule of keep_partials runs the same kernels with only tip / stored children.)
// ------------------------------------------------------------------------------------------------
// lower: stored partials, array `core` at lower + core * C*P*4, layout [C][P][4] (the reference's)
// tipmask: [T][P] 4-bit ambiguity masks
// lscale: [cores][P] cumulative log scale factors (SCALE only)

struct Ctx4 {
	const uint8_t *__restrict__ tipmask;
	const double *__restrict__ mats;
	const double *__restrict__ tiptab;  // [T][C][16][4] tip messages, then the DeepDesc table [N]
	int P, C, c, k;
	int T;
	bool valu_tips = false;  // tip messages as P . mask in registers instead of a table gather (see tipmsg)
	__device__ __forceinline__ const DeepDesc *deep(int node) const { return reinterpret_cast<const DeepDesc *>(tiptab + (size_t)T * C * 64) + node; }
	// P_t . tip vector: one gather from the per-(tip, category) table of the 16 possible masks
	// valu_tips (post-order walk, whose vector ALU is three quarters idle): the same product from the tip's matrix in SGPRs --
	// bit for bit the table's entry (k_tip_tables forms it with the same matvec4) -- so the mask byte's round trip is not
	// followed by a second, divergent one (the gathers were 2.7 of that kernel's 15 ms at 1000 taxa x 1e6 patterns)
	__device__ __forceinline__ d4 tipmsg(int t) const {
		const unsigned m = tipmask[(size_t)t * P + k];
		if (valu_tips) return matvec4(M(t), mask4(m));
		return load4(tiptab + (((size_t)t * C + c) * 16 + m) * 4);
	}
	__device__ __forceinline__ cptr M(int node) const { return opaque(as_const(mats + ((size_t)node * C + c) * 16)); }
};

// partial of a fringe node itself (before its own branch's matrix): cherry = product of two tip messages, cherry + tip
__device__ __forceinline__ d4 fringe_partial(const Ctx4 &x, int kind, int t0, int t1, int t2, int inner) {
	d4 p = mul4(x.tipmsg(t0), x.tipmsg(t1));
	if (kind == CH_CHERRY_TIP) p = mul4(matvec4(x.M(inner), p), x.tipmsg(t2));
	return p;
}
// partial of a DEEP node: both children are tips or fringe nodes, described in the DeepDesc table
__device__ __forceinline__ d4 deep_partial(const Ctx4 &x, int node) {
	const DeepDesc *d = x.deep(node);  // wave-uniform: scalar loads
	const d4 a = d->kind_left == CH_TIP ? x.tipmsg(d->left) : matvec4(x.M(d->left), fringe_partial(x, d->kind_left, d->lt0, d->lt1, d->lt2, d->linner));
	const d4 b = d->kind_right == CH_TIP ? x.tipmsg(d->right) : matvec4(x.M(d->right), fringe_partial(x, d->kind_right, d->rt0, d->rt1, d->rt2, d->rinner));
	return mul4(a, b);
}

// message of one child to its parent, P_child . p_child, at (pattern k, category c): a tip (table gather), a stored
// array, or a fringe / DEEP subtree recomputed in registers
__device__ __forceinline__ d4 child_message(const Ctx4 &x, int kind, int node, int core, int t0, int t1, int t2, int inner,
                                            const double *__restrict__ lower, size_t plane) {
	if (kind == CH_TIP) return x.tipmsg(node);
	if (kind == CH_CORE) return matvec4(x.M(node), load4_stream(lower + ((size_t)core * x.C + x.c) * plane + (size_t)x.k * 4));
	if (kind == CH_DEEP) return matvec4(x.M(node), deep_partial(x, node));
	return matvec4(x.M(node), fringe_partial(x, kind, t0, t1, t2, inner));
}
// same, also handing back p_child itself, which the substitution-parameter gradient contracts with dP/dtheta
__device__ __forceinline__ d4 child_message_pre(const Ctx4 &x, int kind, int node, int core, int t0, int t1, int t2, int inner,
                                                const double *__restrict__ lower, size_t plane, d4 &pre) {
	if (kind == CH_TIP) return x.tipmsg(node);
	if (kind == CH_CORE) pre = load4(lower + ((size_t)core * x.C + x.c) * plane + (size_t)x.k * 4);
	else if (kind == CH_DEEP) pre = deep_partial(x, node);
	else pre = fringe_partial(x, kind, t0, t1, t2, inner);
	return matvec4(x.M(node), pre);
}


// fixed-order reduction of per-block slabs: one wave per row. out[row_offset + row] = sum_b part[row][b]
__global__ __launch_bounds__(64) void k_reduce_rows(const double *__restrict__ part, int nblk, const uint8_t *__restrict__ row_valid,
                                                   double *__restrict__ out) {
	const int row = blockIdx.x;
	double s = 0.0;
	if (row_valid == nullptr || row_valid[row]) {
		for (int b = threadIdx.x; b < nblk; b += 64) s += part[(size_t)row * nblk + b];
		s = wave_sum(s);
	}
	if (threadIdx.x == 0) out[row] = s;
}

// sum_k (w_k / L_k) sum_i pi_i ( p_root[0][k][i] - mean_{c >= 1} p_root[c][k][i] ): the d lnL / d(proportion of the
// invariant class) term that needs the root partials (treelikelihood.c:2943-3008).  root: stored root partial;
// cat_stride / pat_stride / state_stride describe its layout ([C][P][4] or planes [C][S][Pp]).  L_k is re-formed from the
// root partial itself (scale factors are per pattern), so the expression also serves rescaled evaluations.
// Ec: null, or the per-category exponents of a root partial in the streamed walks' power-of-two form (LowerForm::CarriedExp2,
// [C][P]: category c is in units of 2^Ec[c][k]).  Every category is then brought to the units of the largest exponent of its
// pattern before the categories are mixed (as k_root_finish64 forms L_k).
__global__ __launch_bounds__(256) void k_root_invariant_term(int P, int S, int C, const double *__restrict__ root, size_t cat_stride, size_t pat_stride,
                                                            size_t state_stride, const double *__restrict__ freqs, const double *__restrict__ props,
                                                            const double *__restrict__ weights, const int *__restrict__ Ec, double *__restrict__ part) {
	__shared__ double red[4];
	const int k = blockIdx.x * 256 + threadIdx.x;
	double acc = 0.0;
	if (k < P) {
		int E = 0;
		if (Ec) {
			E = Ec[k];
			for (int c = 1; c < C; c++) E = max(E, Ec[(size_t)c * P + k]);
		}
		double s = 0.0, like = 0.0;
		for (int i = 0; i < S; i++) {
			const double *p = root + (size_t)k * pat_stride + (size_t)i * state_stride;
			const double p0 = Ec ? ldexp(p[0], Ec[k] - E) : p[0];
			double others = 0.0, mix = props[0] * p0;
			for (int c = 1; c < C; c++) {
				const double v = p[(size_t)c * cat_stride], pc = Ec ? ldexp(v, Ec[(size_t)c * P + k] - E) : v;
				others += pc;
				mix += props[c] * pc;
			}
			s += freqs[i] * (p0 - others / (C - 1));
			like += freqs[i] * mix;
		}
		acc = s * (weights[k] / like);
	}
	const double t = wave_sum(acc);
	if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = t;
	__syncthreads();
	if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// The root term of d lnL / d pi_f (calculate_dlnl_dQ, treelikelihood.c:2370-2401): for every state f
//   sum_k w_k  ( sum_c w_c p_root[c][k][f] )  /  ( sum_i pi_i sum_c w_c p_root[c][k][i] ).
// Scale factors are per pattern, so the same expression serves rescaled evaluations.  part: [S][gridDim.x]
__global__ __launch_bounds__(256) void k_root_frequency_term(int P, int S, int C, const double *__restrict__ root, size_t cat_stride, size_t pat_stride,
                                                            size_t state_stride, const double *__restrict__ freqs, const double *__restrict__ props,
                                                            const double *__restrict__ weights, double *__restrict__ part) {
	__shared__ double red[4];
	const int k = blockIdx.x * 256 + threadIdx.x;
	double like = 0.0;
	if (k < P)
		for (int i = 0; i < S; i++) {
			const double *p = root + (size_t)k * pat_stride + (size_t)i * state_stride;
			double m = 0.0;
			for (int c = 0; c < C; c++) m += props[c] * p[(size_t)c * cat_stride];
			like += freqs[i] * m;
		}
	const double wl = k < P ? weights[k] / like : 0.0;
	for (int f = 0; f < S; f++) {
		double m = 0.0;
		if (k < P) {
			const double *p = root + (size_t)k * pat_stride + (size_t)f * state_stride;
			for (int c = 0; c < C; c++) m += props[c] * p[(size_t)c * cat_stride];
		}
		const double t = wave_sum(m * wl);
		__syncthreads();
		if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = t;
		__syncthreads();
		if (threadIdx.x == 0) part[(size_t)f * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
	}
}

// One step of the root-to-node path that rebuilds ONE upper partial (phyamd_branch_log_likelihood without resident uppers):
//   upper(child) = (step at the root ? 1 : P_parent . upper(parent)) o message(sibling)
struct PathStep {
	int32_t mat;                               // node whose matrix multiplies the incoming upper (-1: the parent is the root)
	int32_t kind, node, core, t0, t1, t2, inner;  // the sibling, as child_message takes it
};

// Upper partial of one node by walking down from the root, 4 states: workgroup = 64 patterns x C category waves.
// SCALE: the stored lower partials are rescaled per pattern, so the product shrinks step by step; it is divided by its
// per-pattern maximum over categories and states whenever that falls below the threshold (the factor itself is irrelevant:
// the caller forms log(L(t) / L(t0)), in which every per-pattern factor cancels).  out: [C][P][4]
template <bool SCALE>
__global__ void k_path_upper4(const PathStep *__restrict__ steps, int nsteps, int T, int P, int C, const uint8_t *__restrict__ tipmask,
                              const double *__restrict__ lower, const double *__restrict__ mats, const double *__restrict__ tiptab,
                              double *__restrict__ out) {
	extern __shared__ double sh[];  // SCALE: [C][64]
	const int lane = threadIdx.x, c = __builtin_amdgcn_readfirstlane(threadIdx.y);
	const int k0 = blockIdx.x * WAVE + lane;
	const bool valid = k0 < P;
	const int k = valid ? k0 : P - 1;
	const size_t plane = (size_t)P * 4;
	const Ctx4 x{tipmask, mats, tiptab, P, C, c, k, T};
	d4 u = d4{1., 1., 1., 1.};
	for (int j = 0; j < nsteps; j++) {
		const PathStep st = steps[j];  // wave-uniform: scalar loads
		const d4 a = st.mat < 0 ? u : matvec4(x.M(st.mat), u);
		u = mul4(a, child_message(x, st.kind, st.node, st.core, st.t0, st.t1, st.t2, st.inner, lower, plane));
		if (SCALE) {
			__syncthreads();
			sh[c * WAVE + lane] = max4(u);
			__syncthreads();
			double m = 0.0;
			for (int cc = 0; cc < C; cc++) m = fmax(m, sh[cc * WAVE + lane]);
			if (m < 1.0e-40 && m > 0.0) u = d4{u.x / m, u.y / m, u.z / m, u.w / m};
		}
	}
	if (valid) store4(out + (size_t)c * plane + (size_t)k * 4, u);
}

// lower partial of a node that is not stored (fringe or DEEP), recomputed from its tips: out [C][P][4]
__global__ void k_unstored_partial4(int kind, int node, int t0, int t1, int t2, int inner, int T, int P, int C, const uint8_t *__restrict__ tipmask,
                                    const double *__restrict__ mats, const double *__restrict__ tiptab, double *__restrict__ out) {
	const int lane = threadIdx.x, c = __builtin_amdgcn_readfirstlane(threadIdx.y);
	const int k = blockIdx.x * WAVE + lane;
	if (k >= P) return;
	const Ctx4 x{tipmask, mats, tiptab, P, C, c, k, T};
	const d4 p = kind == CH_DEEP ? deep_partial(x, node) : fringe_partial(x, kind, t0, t1, t2, inner);
	store4(out + ((size_t)c * P + k) * 4, p);
}

// Single-branch likelihood from the two partials that meet on the branch (the optimiser's fast path: _calculate_uppper,
// dlnldt_uppper, d2lnldt2_uppper, treelikelihood.c:2196-2335, 2592-2686), 4 states:
//   L_k(t) = sum_c w_c sum_i f_i u_i (P(t r_c) p)_i,  L' = sum_c w_c r_c sum_i f_i u_i (Q P p)_i,  L'' with Q Q P.
// pm: [C][3][16] = P, r Q P, r^2 Q Q P per category (host-built for the trial length).  Workgroup = 64 patterns x C waves;
// part: [3][gridDim.x] partial sums of w log L, w L'/L, w (L''/L - (L'/L)^2).
// Rescaled evaluations (plk != NULL): u and p carry per-pattern scale factors that nobody kept for the uppers, but they
// cancel in  log L_k(t) = plk[k] + log(L~_k(t) / L~_k(t0)),  L~ formed from the stored (scaled) partials and m0 = the
// branch's current matrices [C][16], plk = the per-pattern lnL of the evaluation the partials belong to.
__global__ void k_branch_eval4(int P, int C, const double *__restrict__ up, const double *__restrict__ low, const uint8_t *__restrict__ tipmask_row,
                               const double *__restrict__ pm, const double *__restrict__ freqs, int fold, const double *__restrict__ props,
                               const double *__restrict__ weights, const double *__restrict__ plk, const double *__restrict__ m0,
                               double *__restrict__ part) {
	extern __shared__ double sh[];  // [4][C][64]
	const int lane = threadIdx.x, c = __builtin_amdgcn_readfirstlane(threadIdx.y);
	const int k0 = blockIdx.x * WAVE + lane;
	const bool valid = k0 < P;
	const int k = valid ? k0 : P - 1;
	const size_t plane = (size_t)P * 4;
	const d4 u = load4(up + (size_t)c * plane + (size_t)k * 4);
	const d4 p = low ? load4(low + (size_t)c * plane + (size_t)k * 4) : mask4(tipmask_row[k]);
	const d4 fu = fold ? u : mul4(d4{freqs[0], freqs[1], freqs[2], freqs[3]}, u);
	const cptr M = as_const(pm + (size_t)c * 48);
	sh[(0 * C + c) * WAVE + lane] = props[c] * dot4(fu, matvec4(M, p));
	sh[(1 * C + c) * WAVE + lane] = props[c] * dot4(fu, matvec4(M + 16, p));
	sh[(2 * C + c) * WAVE + lane] = props[c] * dot4(fu, matvec4(M + 32, p));
	if (plk) sh[(3 * C + c) * WAVE + lane] = props[c] * dot4(fu, matvec4(as_const(m0 + (size_t)c * 16), p));
	__syncthreads();
	if (c == 0) {
		double L = 0.0, L1 = 0.0, L2 = 0.0, L0 = 0.0;
		for (int cc = 0; cc < C; cc++) {
			L += sh[(0 * C + cc) * WAVE + lane];
			L1 += sh[(1 * C + cc) * WAVE + lane];
			L2 += sh[(2 * C + cc) * WAVE + lane];
			if (plk) L0 += sh[(3 * C + cc) * WAVE + lane];
		}
		const double w = valid ? weights[k] : 0.0, r1 = L1 / L, r2 = L2 / L;
		const double logL = plk ? plk[k] + log(L / L0) : log(L);
		const double a = wave_sum(valid ? w * logL : 0.0), b = wave_sum(valid ? w * r1 : 0.0), d = wave_sum(valid ? w * (r2 - r1 * r1) : 0.0);
		if (lane == 0) {
			part[blockIdx.x] = a;
			part[(size_t)gridDim.x + blockIdx.x] = b;
			part[(size_t)2 * gridDim.x + blockIdx.x] = d;
		}
	}
}
