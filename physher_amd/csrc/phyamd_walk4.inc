// phyamd_walk4.inc: depth-first tree-walk 4-state kernels (k_lower4_walk, k_upper4_walk): two launches per pass (cut subtrees and the
// top of the tree: chunk_pre_order / chunk_post_order) -- included by phyamd_engine.hip inside its anonymous namespace.

// ------------------------------------------------------------------------------------------------
// Tree-walk form of the post-order pass (unscaled evaluations).  Patterns are independent, so instead of one launch
// per tree level a workgroup keeps its 64*G*PPT_WALK patterns (PPT_WALK = 1 or 2, by shard size) and walks ALL core nodes itself, in depth-first
// post-order (larger subtree first).  The op before a node is then always one of its children: that child's partial
// is taken from registers instead of being read back (it is still stored once for the pre-order pass), and the other
// child was written by this very thread a short subtree ago, often still in L2 / Infinity Cache.  No
// level barriers; the root's integration happens after the loop on the carried root partial.
// dynamic LDS: G*C*64 doubles (root exchange) + G doubles
// ------------------------------------------------------------------------------------------------
// LPARK: a stored child that is re-read after a subtree which re-reads nothing itself also waits in the wave's
// LDS slot (NodeOp::lds_park; one slot of 64 x 32 bytes per wave and pattern group behind the exchange buffers): the re-read is an
// LDS round trip instead of an HBM / L2 one.
// Post-order walk: the mask bytes of ALL tips under an op's two children (a tip, a cherry, a cherry + tip, or a DEEP node of two
// such halves: up to six per child) are requested together at the top of the op.  Taken one by one inside the nested child
// messages, each byte was its own memory round trip: up to twelve in a row per op.
// slot order per child: tip -> [0]; cherry -> [0, 1]; cherry + tip -> [0, 1, 2]; DEEP -> left half in [0..2], right half in [3..5]
__device__ __forceinline__ void load_half_masks(const uint8_t *__restrict__ tipmask, int P, int k, int kind, int node, int t0, int t1, int t2, unsigned *m) {
	if (kind == CH_TIP) m[0] = tipmask[(size_t)node * P + k];
	else {
		m[0] = tipmask[(size_t)t0 * P + k];
		m[1] = tipmask[(size_t)t1 * P + k];
		if (kind == CH_CHERRY_TIP) m[2] = tipmask[(size_t)t2 * P + k];
	}
}
__device__ __forceinline__ void load_child_masks(const Ctx4 &x, int kind, int node, int t0, int t1, int t2, unsigned (&m)[6]) {
	if (kind == CH_CORE) return;
	if (kind == CH_DEEP) {
		const DeepDesc *d = x.deep(node);  // wave-uniform: scalar loads
		load_half_masks(x.tipmask, x.P, x.k, d->kind_left, d->left, d->lt0, d->lt1, d->lt2, m);
		load_half_masks(x.tipmask, x.P, x.k, d->kind_right, d->right, d->rt0, d->rt1, d->rt2, m + 3);
	} else
		load_half_masks(x.tipmask, x.P, x.k, kind, node, t0, t1, t2, m);
}
__device__ __forceinline__ d4 tip_message(const Ctx4 &x, int t, unsigned m) {
	if (x.valu_tips) return matvec4(x.M(t), mask4(m));
	return load4(x.tiptab + (((size_t)t * x.C + x.c) * 16 + m) * 4);
}
// P_half . p_half of a tip / cherry / cherry + tip, masks in m[0..2]
__device__ __forceinline__ d4 half_message(const Ctx4 &x, int kind, int node, int t0, int t1, int t2, int inner, const unsigned *m) {
	if (kind == CH_TIP) return tip_message(x, node, m[0]);
	d4 p = mul4(tip_message(x, t0, m[0]), tip_message(x, t1, m[1]));
	if (kind == CH_CHERRY_TIP) p = mul4(matvec4(x.M(inner), p), tip_message(x, t2, m[2]));
	return matvec4(x.M(node), p);
}
// message of a child that is not carried (child_message with the masks already in registers)
__device__ __forceinline__ d4 child_message_hoisted(const Ctx4 &x, int kind, int node, int core, int t0, int t1, int t2, int inner,
                                                    const double *__restrict__ lower, size_t plane, const unsigned (&m)[6]) {
	if (kind == CH_CORE) return matvec4(x.M(node), load4_stream(lower + ((size_t)core * x.C + x.c) * plane + (size_t)x.k * 4));
	if (kind == CH_DEEP) {
		const DeepDesc *d = x.deep(node);
		const d4 a = half_message(x, d->kind_left, d->left, d->lt0, d->lt1, d->lt2, d->linner, m);
		const d4 b = half_message(x, d->kind_right, d->right, d->rt0, d->rt1, d->rt2, d->rinner, m + 3);
		return matvec4(x.M(node), mul4(a, b));
	}
	return half_message(x, kind, node, t0, t1, t2, inner, m);
}

constexpr int LOWER_MIN_WAVES = 7;  // waves per SIMD asked of the plain one-pattern-per-thread walk (67 VGPRs): 6 -> 12.97, 7 -> 12.55, 8 (4 spilled) -> 13.25 ms
template <int WAVES, int PPT_WALK, bool SCALE>
__global__ __launch_bounds__(WAVES *WAVE, (WAVES == 4 && PPT_WALK == 1 && !SCALE) ? LOWER_MIN_WAVES : 1) void k_lower4_walk(const NodeOp *__restrict__ ops, int nops, int T, int P, int C,
                                                             const uint8_t *__restrict__ tipmask, double *__restrict__ lower,
                                                             const double *__restrict__ mats, const double *__restrict__ tiptab,
                                                             double *__restrict__ lscale,
                                                             const double *__restrict__ freqs, const double *__restrict__ props,
                                                             const double *__restrict__ weights, double *__restrict__ pattern_lk,
                                                             double *__restrict__ w_over_L, double *__restrict__ lnl_part,
                                                             const int *__restrict__ chunk_off, int chunk_base, int with_root) {
	// dynamic LDS: root exchange G*C*64 + G doubles; SCALE: + two G*C*64 buffers for the per-op maximum over categories
	extern __shared__ double sh[];
	const int lane = threadIdx.x, c = __builtin_amdgcn_readfirstlane(threadIdx.y), g = __builtin_amdgcn_readfirstlane(threadIdx.z), G = blockDim.z;
	const size_t plane = (size_t)P * 4;
	const int xsz = G * C * WAVE;
	int kq[PPT_WALK];
	bool vq[PPT_WALK];
#pragma unroll
	for (int q = 0; q < PPT_WALK; q++) {
		const int k0 = ((blockIdx.x * PPT_WALK + q) * G + g) * WAVE + lane;
		vq[q] = k0 < P;
		kq[q] = vq[q] ? k0 : P - 1;
	}
	d4 carry[PPT_WALK];
	double sfc[PPT_WALK];  // SCALE: cumulative log scale factor of the carried partial
#pragma unroll
	for (int q = 0; q < PPT_WALK; q++) {
		carry[q] = d4{0., 0., 0., 0.};
		sfc[q] = 0.0;
	}
	int flip = 0;
	// LPARK: park slots behind the root exchange (xsz + G doubles) and the SCALE exchange: [wave][q][2 halves][64 lanes] of 16 bytes
	dv2 *park = reinterpret_cast<dv2 *>(sh + xsz + G + (G & 1) + (SCALE ? 2 * xsz : 0)) + (size_t)(g * C + c) * PPT_WALK * 2 * WAVE + lane;
	// chunked launches (chunk_post_order): ops [op_begin, op_end) of the list, chunk blockIdx.y of the launch
	const int op_begin = chunk_off ? chunk_off[chunk_base + blockIdx.y] : 0, op_end = chunk_off ? chunk_off[chunk_base + blockIdx.y + 1] : nops;
#pragma unroll 1
	for (int i = op_begin; i < op_end; i++) {
		const NodeOp *op = ops + i;  // wave-uniform: scalar loads
		const int cin = op->carry_in;
		const int lp = op->lds_park;
		double *dst = lower + ((size_t)op->core_parent * C + c) * plane;
#pragma unroll
		for (int q = 0; q < PPT_WALK; q++) {
			const Ctx4 x{tipmask, mats, tiptab, P, C, c, kq[q], T, true};
			d4 a, b;
			if (lp & 3) {  // both children stored: one carried, the other from the LDS slot
				const dv2 lo = park[q * 2 * WAVE], hi = park[(q * 2 + 1) * WAVE];
				const d4 parked = d4{lo.x, lo.y, hi.x, hi.y};
				a = matvec4(x.M(op->left), (lp & 1) ? parked : carry[q]);
				b = matvec4(x.M(op->right), (lp & 2) ? parked : carry[q]);
			} else if (SCALE) {  // (the rescaled walk measures 5 ms slower with the hoisted form: 21.2 vs 16.3)
				a = cin == 1 ? matvec4(x.M(op->left), carry[q])
				             : child_message(x, op->kind_left, op->left, op->core_left, op->lt0, op->lt1, op->lt2, op->linner, lower, plane);
				b = cin == 2 ? matvec4(x.M(op->right), carry[q])
				             : child_message(x, op->kind_right, op->right, op->core_right, op->rt0, op->rt1, op->rt2, op->rinner, lower, plane);
			} else {
				unsigned ml[6] = {0, 0, 0, 0, 0, 0}, mr[6] = {0, 0, 0, 0, 0, 0};
				__builtin_amdgcn_s_setprio(3);
				if (cin != 1) load_child_masks(x, op->kind_left, op->left, op->lt0, op->lt1, op->lt2, ml);
				if (cin != 2) load_child_masks(x, op->kind_right, op->right, op->rt0, op->rt1, op->rt2, mr);
				__builtin_amdgcn_s_setprio(0);
				a = cin == 1 ? matvec4(x.M(op->left), carry[q])
				             : child_message_hoisted(x, op->kind_left, op->left, op->core_left, op->lt0, op->lt1, op->lt2, op->linner, lower, plane, ml);
				b = cin == 2 ? matvec4(x.M(op->right), carry[q])
				             : child_message_hoisted(x, op->kind_right, op->right, op->core_right, op->rt0, op->rt1, op->rt2, op->rinner, lower, plane, mr);
			}
			d4 out = mul4(a, b);
			if (SCALE) {  // SingleTreeLikelihood_scalePartials (treelikelihood.c:1790-1836): max over categories and states
				double *xb = sh + xsz + G + (flip & 1) * xsz;
				flip++;
				xb[(g * C + c) * WAVE + lane] = max4(out);
				lds_barrier();
				double m = 0.0, sf = 0.0;
				for (int cc = 0; cc < C; cc++) m = fmax(m, xb[(g * C + cc) * WAVE + lane]);
				if (m < SCALING_THRESHOLD && m > 0.0) {  // (m == 0, an empty state mask below: see k_lower4)
					out = d4{out.x / m, out.y / m, out.z / m, out.w / m};
					sf = log(m);
				}
				if (op->kind_left == CH_CORE) sf += cin == 1 ? sfc[q] : lscale[(size_t)op->core_left * P + kq[q]];
				if (op->kind_right == CH_CORE) sf += cin == 2 ? sfc[q] : lscale[(size_t)op->core_right * P + kq[q]];
				if (c == 0 && vq[q]) lscale[(size_t)op->core_parent * P + kq[q]] = sf;
				sfc[q] = sf;
			}
			if (vq[q] && !(op->lds_park & 8)) store4_stream(dst + (size_t)kq[q] * 4, out);  // (bit 3: no longer set by the host)
			if (lp & 4) {
				park[q * 2 * WAVE] = dv2{out.x, out.y};
				park[(q * 2 + 1) * WAVE] = dv2{out.z, out.w};
			}
			carry[q] = out;
		}
	}
	if (!with_root) return;  // a cut subtree: its root's partial is in HBM for the top part
	// the last op is the root: integrate_partials + node_log_likelihoods + weighted sum (treelikelihood.c:1473-1487)
	// one entry per block of 64 patterns (block = pattern / 64, whatever the launch shape: the sums over blocks are then formed in
	// an order that depends on the pattern range alone, see reduce_block_sums)
#pragma unroll
	for (int q = 0; q < PPT_WALK; q++) {
		const d4 out = carry[q];
		__syncthreads();
		sh[(g * C + c) * WAVE + lane] = props[c] * (freqs[0] * out.x + freqs[1] * out.y + freqs[2] * out.z + freqs[3] * out.w);
		__syncthreads();
		if (c == 0) {
			double L = 0.0, term = 0.0;
			for (int cc = 0; cc < C; cc++) L += sh[(g * C + cc) * WAVE + lane];
			const double lk = log(L) + (SCALE ? sfc[q] : 0.0);
			if (vq[q]) {
				const double w = weights[kq[q]];
				pattern_lk[kq[q]] = lk;
				if (!SCALE) w_over_L[kq[q]] = w / L;
				term = lk * w;
			}
			const double s = wave_sum(term);
			if (lane == 0) lnl_part[(blockIdx.x * PPT_WALK + q) * G + g] = s;
		}
	}
}

// tree-walk kernel: one pattern per thread, so every branch term is written exactly once per op (no read-modify-write);
// Q is diag(pi) Q (or Q when the frequencies are folded into the uppers), so there is no separate state weight.
// PARAMS: every gradient site also feeds the substitution-parameter gradient, accumulated in the eigen basis:
//   d lnL / d theta = sum_ab B_theta,ab G_ab,   G_ab = sum_sites w_c F_ab(t r_c) (w_k / L_k) a_a b_b,
//   a = U^T (pi o u),  b = U^-1 p,  B_theta = U^-1 dQ_theta U,  F as in dPdp_with_dQdp (substmodel.c:469-489)
// -- 16 accumulators per thread whatever the number of parameters, two extra mat-vecs and 16 multiply-adds per site
// (the reference walks the tree once per parameter; the level kernels contract with one dP/dtheta per parameter).
struct ParamCtx {
	cptr UTpi, Uinv;     // (diag(pi) U)^T and U^-1, 4x4 row-major
	const double *utab;  // [16][4]: U^-1 . tip mask
	const double *Fw;    // [N][C][20]: w_c F_ab(t_n r_c), then l_a e^{l_a t_n r_c} (the branch term in the eigen basis)
};
// SCALE (rescaled evaluations): the branch term is (w_k / D_k) num with D_k the site likelihood in the op's scaled units, and the
// parameter sums weight with wl = w_k / D_k.
template <bool PARAMS, bool SCALE, bool COMPAT = false>
struct GradWT {
	static constexpr bool FENCE = PARAMS;
	cptr Q;
	double wl;
	double *col;  // this thread's NACC slots in LDS, stride WCOL
	ParamCtx pc;
	double *G;    // [16], registers of the kernel
	double wq;    // SCALE only: w_k / D_k (the mixture likelihood in the op's scaled units): one division per op, not one per site
	double w, d;  // SCALE + COMPAT: the reference divides each category's term by that category's own likelihood, which underflows
	              // to denormals where the ratio is still finite -- quotient first there
	__device__ __forceinline__ void add(int i, const d4 &u, const d4 &b) const {
		const double num = dot4(u, matvec4_opt<FENCE>(opaque(Q), b));
		col[i * WCOL] = SCALE ? (COMPAT ? w * (num / d) : wq * num) : wl * num;
	}
	// PARAMS: the branch term comes from the same two eigen-basis vectors as the parameter sums,
	//   sum_i (pi o u)_i (Q P p)_i = sum_a l_a e^{l_a t} a_a b_a   (Q P = U L e^{Lt} U^-1),
	// four multiply-adds instead of a mat-vec with Q and a dot product
	__device__ __forceinline__ void accumulate(const Ctx4 &x, int slot, int node, const d4 &a, const d4 &b) const {
		const cptr F = opaque(as_const(pc.Fw + ((size_t)node * x.C + x.c) * 20));
		const double num = ((F[16] * a.x) * b.x + (F[17] * a.y) * b.y) + ((F[18] * a.z) * b.z + (F[19] * a.w) * b.w);
		col[slot * WCOL] = SCALE ? (COMPAT ? w * (num / d) : wq * num) : wl * num;
		const double t0 = wl * a.x, t1 = wl * a.y, t2 = wl * a.z, t3 = wl * a.w;
		G[0] += (F[0] * t0) * b.x;
		G[1] += (F[1] * t0) * b.y;
		G[2] += (F[2] * t0) * b.z;
		G[3] += (F[3] * t0) * b.w;
		G[4] += (F[4] * t1) * b.x;
		G[5] += (F[5] * t1) * b.y;
		G[6] += (F[6] * t1) * b.z;
		G[7] += (F[7] * t1) * b.w;
		G[8] += (F[8] * t2) * b.x;
		G[9] += (F[9] * t2) * b.y;
		G[10] += (F[10] * t2) * b.z;
		G[11] += (F[11] * t2) * b.w;
		G[12] += (F[12] * t3) * b.x;
		G[13] += (F[13] * t3) * b.y;
		G[14] += (F[14] * t3) * b.z;
		G[15] += (F[15] * t3) * b.w;
		__builtin_amdgcn_sched_barrier(0);
	}
	// one gradient site = column `slot` of the op: upper u at the top of the branch, the child's message b = P p, and
	// either its computed lower partial p (stored node, cherry product, ...) or, for a tip, its mask m
	__device__ __forceinline__ void site_vec(const Ctx4 &x, int slot, int node, const d4 &u, const d4 &b, const d4 &p) const {
		if (PARAMS) accumulate(x, slot, node, matvec4_opt<FENCE>(opaque(pc.UTpi), u), matvec4_opt<FENCE>(opaque(pc.Uinv), p));
		else add(slot, u, b);
	}
	__device__ __forceinline__ void site_tip(const Ctx4 &x, int slot, int tip, const d4 &u, const d4 &b, unsigned m) const {
		if (PARAMS) accumulate(x, slot, tip, matvec4_opt<FENCE>(opaque(pc.UTpi), u), load4(pc.utab + m * 4));
		else add(slot, u, b);
	}
};

// Variants for the pre-order tree walk: the mask bytes of an op's (up to six) tips are all requested at the top of the op,
// together with the parent's upper, so the op pays one memory round trip for them instead of one per child.
__device__ __forceinline__ d4 tip_gather(const Ctx4 &x, int t, unsigned m) { return load4(x.tiptab + (((size_t)t * x.C + x.c) * 16 + m) * 4); }
// `pre` receives the child's own partial (what the parameter gradient contracts): untouched for tips
// P_half . p_half of one half of a DEEP node (a tip, a cherry or a cherry + tip), masks in m[0..2], messages from the tables
template <bool FENCE>
__device__ __forceinline__ d4 deep_half_m(const Ctx4 &x, int kind, int node, int t0, int t1, int t2, int inner, const unsigned *m) {
	if (kind == CH_TIP) return tip_gather(x, node, m[0]);
	d4 p = mul4(tip_gather(x, t0, m[0]), tip_gather(x, t1, m[1]));
	if (kind == CH_CHERRY_TIP) p = mul4(matvec4_opt<FENCE>(x.M(inner), p), tip_gather(x, t2, m[2]));
	return matvec4_opt<FENCE>(x.M(node), p);
}
template <bool FENCE>
__device__ __forceinline__ d4 child_message_m(const Ctx4 &x, int kind, int node, int core, int t0, int t1, int t2, int inner,
                                              const d4 &pcore, unsigned m0, unsigned m1, unsigned m2, d4 &pre, const unsigned (&dm)[6]) {
	if (kind == CH_TIP) return tip_gather(x, node, m0);
	if (kind == CH_CORE) pre = pcore;
	else if (kind == CH_DEEP) {
		const DeepDesc *d = x.deep(node);  // wave-uniform: scalar loads
		pre = mul4(deep_half_m<FENCE>(x, d->kind_left, d->left, d->lt0, d->lt1, d->lt2, d->linner, dm),
		           deep_half_m<FENCE>(x, d->kind_right, d->right, d->rt0, d->rt1, d->rt2, d->rinner, dm + 3));
	} else {
		const d4 g0 = tip_gather(x, t0, m0), g1 = tip_gather(x, t1, m1);
		d4 g2 = d4{1., 1., 1., 1.};
		if (kind == CH_CHERRY_TIP) g2 = tip_gather(x, t2, m2);  // requested with the other two, not behind the inner mat-vec
		pre = mul4(g0, g1);                                                                          // cherry
		if (kind == CH_CHERRY_TIP) pre = mul4(matvec4_opt<FENCE>(x.M(inner), pre), g2);              // cherry + tip
	}
	return matvec4_opt<FENCE>(x.M(node), pre);
}
template <typename GradT>
__device__ __forceinline__ void descend_fringe_m(const Ctx4 &x, const GradT &gr, int base, int kind, int node, int t0, int t1, int t2, int inner,
                                                 const d4 &u, unsigned m0, unsigned m1, unsigned m2) {
	const d4 b0 = tip_gather(x, t0, m0), b1 = tip_gather(x, t1, m1);
	d4 b2e = d4{1., 1., 1., 1.};
	if (kind == CH_CHERRY_TIP) b2e = tip_gather(x, t2, m2);
	d4 a2 = matvec4_opt<GradT::FENCE>(x.M(node), u);
	if (kind == CH_CHERRY_TIP) {
		const d4 pn = mul4(b0, b1);
		const d4 bn = matvec4_opt<GradT::FENCE>(x.M(inner), pn);
		const d4 b2 = b2e;
		const d4 un = mul4(a2, b2);
		gr.site_vec(x, base + 2, inner, un, bn, pn);
		gr.site_tip(x, base + 3, t2, mul4(a2, bn), b2, m2);
		a2 = matvec4_opt<GradT::FENCE>(x.M(inner), un);  // now the upper message entering the inner cherry
	}
	gr.site_tip(x, base + 0, t0, mul4(a2, b1), b0, m0);
	gr.site_tip(x, base + 1, t1, mul4(a2, b0), b1, m1);
}

// sum 16 per-lane values over the 64 lanes of a wave in 17 exchange steps (instead of 16 x 6): after the xor-32 step a
// lane keeps only half of the values, after xor-16 a quarter, ...  Returns, in every lane, the wave total of value
// index ((lane >> 2) & 15) with bits taken as (bit5, bit4, bit3, bit2) -> (8, 4, 2, 1).  Fixed order: deterministic.
__device__ __forceinline__ double wave_sum16(const double (&v)[16], int lane) {
	double a8[8], a4[4], a2[2];
	const bool h5 = lane & 32, h4 = lane & 16, h3 = lane & 8, h2 = lane & 4;
#pragma unroll
	for (int i = 0; i < 8; i++) a8[i] = (h5 ? v[i + 8] : v[i]) + __shfl_xor(h5 ? v[i] : v[i + 8], 32, 64);
#pragma unroll
	for (int i = 0; i < 4; i++) a4[i] = (h4 ? a8[i + 4] : a8[i]) + __shfl_xor(h4 ? a8[i] : a8[i + 4], 16, 64);
#pragma unroll
	for (int i = 0; i < 2; i++) a2[i] = (h3 ? a4[i + 2] : a4[i]) + __shfl_xor(h3 ? a4[i] : a4[i + 2], 8, 64);
	double a1 = (h2 ? a2[1] : a2[0]) + __shfl_xor(h2 ? a2[0] : a2[1], 4, 64);
	a1 += __shfl_xor(a1, 2, 64);
	a1 += __shfl_xor(a1, 1, 64);
	return a1;
}

// ------------------------------------------------------------------------------------------------
// Tree-walk form of the pre-order pass + branch gradient (unscaled evaluations), the counterpart of k_lower4_walk: a
// workgroup keeps its patterns (ONE per thread) and visits every core node in depth-first pre-order, smaller core subtree
// first.  The upper partial of the child visited next never leaves registers (no store, no load); the other core child's
// upper is parked in one of ~log2(core nodes) recycled slots and read back by the same thread after the small subtree.
// The branch terms of an op go to LDS columns (written once per op) and are reduced over the wave by wave_sum16, then
// written to the gradient slab: gpart[(node * C + c) * nblk + blockIdx.x * G + g], nblk = gridDim.x * G.
// Register-lean on purpose (<= 96 VGPRs, 5 waves per SIMD): the walk is bound by dependent latency chains (tip byte ->
// table gather -> mat-vec, scalar matrix loads), so resident waves matter more than per-op amortisation; a form with 4
// patterns per thread, carried uppers in LDS and accumulators in registers (126 VGPRs, 4 waves) measured 14 % slower.
// dynamic LDS: [waves][NACC][WCOL] doubles
// ------------------------------------------------------------------------------------------------
constexpr int WALK_UPPER_MIN_WAVES = 5;
constexpr int WALK_UPPER_SCALE_WAVES = 4;  // 5 spills (4-16 VGPRs) and needs the LDS park slots gone to fit: 41.0 vs 42.7 ms, not taken
// PARAMS: dynamic LDS holds 16 columns per wave (the eigen-basis sums are reduced once, after the walk); pbuf = [UTpi(16) |
// Uinv(16) | utab(64)], Fw as in ParamCtx, gacc [16][nblk] receives the per-wave sums.
// SCALE / COMPAT: rescaled evaluations (see k_upper4): one LDS exchange per op gives every category's wave the mixture
// denominator D_k and the maxima of the two new uppers; dynamic LDS grows by 4 * waves * 64 doubles (double-buffered).
// LPARK (every launch but the parameter walk, LPARK = !PARAMS): leaf parks (NodeOp::lds_park) wait in a per-wave LDS slot of 64 x
// 32 bytes behind the columns instead of HBM: at 1000 taxa 94 of the 140 parked uppers, i.e. 24 of the 91 GB the walk moves, and
// their re-reads cost an LDS round trip instead of an HBM one.
// CATBLK (unscaled launches only): the workgroup's waves are blockDim.z pattern groups of ONE category, blockIdx.x = group block * C +
// category -- the waves share matrices and tables in the scalar cache (the parameter sums load three 4 x 4 matrices and twenty
// doubles per branch: with one category per wave a fifth of those scalar loads missed)
template <int WAVES, bool FOLD, bool PARAMS, bool SCALE, bool COMPAT, bool CATBLK = false>
__global__ __launch_bounds__(WAVES *WAVE, WAVES == 4 ? (PARAMS ? 3 : (SCALE ? WALK_UPPER_SCALE_WAVES : WALK_UPPER_MIN_WAVES)) : 1) void k_upper4_walk(const NodeOp *__restrict__ ops, int nops, int T, int P, int C,
                                                              const uint8_t *__restrict__ tipmask, const double *__restrict__ lower,
                                                              double *__restrict__ upper, const double *__restrict__ mats,
                                                              const double *__restrict__ tiptab, const double *__restrict__ Q,
                                                              const double *__restrict__ freqs, const double *__restrict__ w_over_L,
                                                              double *__restrict__ gpart, int nblk, const double *__restrict__ pbuf,
                                                              const double *__restrict__ Fw, double *__restrict__ gacc,
                                                              const double *__restrict__ props, const double *__restrict__ weights,
                                                              const int *__restrict__ chunk_off, int chunk_base) {
	extern __shared__ double sh[];
	constexpr int NCOL = PARAMS ? 16 : NACC;
	constexpr bool LPARK = !PARAMS;  // (the parameter walk runs on the unchunked list, whose parks all have HBM slots)
	static_assert(!(CATBLK && SCALE), "rescaled launches exchange across the categories of a workgroup");
	const int lane = threadIdx.x, g = __builtin_amdgcn_readfirstlane(threadIdx.z), G = blockDim.z;
	const int c = CATBLK ? (int)(blockIdx.x % C) : __builtin_amdgcn_readfirstlane(threadIdx.y), bx = CATBLK ? (int)(blockIdx.x / C) : (int)blockIdx.x;
	const size_t plane = (size_t)P * 4;
	const d4 pi = d4{freqs[0], freqs[1], freqs[2], freqs[3]};
	const d4 one = d4{1., 1., 1., 1.};
	const int wv = CATBLK ? g : g * C + c;
	double *wave_cols = sh + (size_t)wv * NCOL * WCOL;  // this wave's columns of WCOL (= 64 + padding) doubles
	double *col = wave_cols + lane;                     // this thread's slot in each column, stride WCOL
	// reduction role of this lane: lanes 0..4*NACC-1 each add a quarter (16 entries) of one column
	const int my = lane >> 2, seg = lane & 3;
	const size_t slab = (size_t)bx * G + g;
	if (CATBLK && slab >= (size_t)nblk) return;  // (no workgroup-level synchronisation in the unscaled kernel)
	const int k0 = (bx * G + g) * WAVE + lane;
	const bool valid = k0 < P;
	const int k = valid ? k0 : P - 1;
	const Ctx4 x{tipmask, mats, tiptab, P, C, c, k, T};
	const double wl = SCALE ? 0.0 : (valid ? w_over_L[k] : 0.0);
	const double wk = SCALE ? (valid ? weights[k] : 0.0) : 0.0;
	const int xsz = G * C * WAVE;
	double *xbase = sh + (size_t)G * C * NCOL * WCOL;  // SCALE: exchange buffers behind the columns
	// LPARK: this wave's park slot behind the columns, two 16-byte halves per lane (conflict-free ds_*_b128)
	dv2 *park = reinterpret_cast<dv2 *>(sh + (size_t)G * C * NCOL * WCOL + (SCALE ? (size_t)4 * xsz : 0) + (size_t)wv * 4 * WAVE) + lane;
	d4 carry = one;
	double Gab[16] = {0., 0., 0., 0., 0., 0., 0., 0., 0., 0., 0., 0., 0., 0., 0., 0.};
	const ParamCtx pc{as_const(pbuf), as_const(pbuf + 16), pbuf + 32, Fw};
	// chunked launches (chunk_pre_order): this workgroup walks ops [op_begin, op_end) of the list, chunk blockIdx.y of the launch
	const int op_begin = chunk_off ? chunk_off[chunk_base + blockIdx.y] : 0, op_end = chunk_off ? chunk_off[chunk_base + blockIdx.y + 1] : nops;
#pragma unroll 1
	for (int i = op_begin; i < op_end; i++) {
		const NodeOp *op = ops + i;  // wave-uniform: scalar loads
		const int cin = op->carry_in, cout = op->carry_out;
		const bool proot = op->upper_slot_parent < 0 && !cin && !(op->lds_park & 1);  // the root: no upper comes in from anywhere
		const int kl = op->kind_left, kr = op->kind_right;
		GradWT<PARAMS, SCALE, COMPAT> gr{as_const(Q), wl, col, pc, Gab, 0.0, 0.0, 1.0};  // Q is diag(pi) Q unless FOLD
		// every tip mask byte of the op up front: all in flight together (a DEEP child's four to six bytes too: they are used
		// once, for its message, at the top of the op)
		__builtin_amdgcn_s_setprio(3);  // a wave about to request its operands goes first: the sooner they leave, the shorter its chain
		unsigned ml0 = 0, ml1 = 0, ml2 = 0, mr0 = 0, mr1 = 0, mr2 = 0;
		unsigned dl[6] = {0, 0, 0, 0, 0, 0}, dr[6] = {0, 0, 0, 0, 0, 0};
		if (kl == CH_DEEP) load_child_masks(x, kl, op->left, -1, -1, -1, dl);
		if (kr == CH_DEEP) load_child_masks(x, kr, op->right, -1, -1, -1, dr);
		if (kl == CH_TIP) ml0 = tipmask[(size_t)op->left * P + k];
		else if (kl >= CH_CHERRY) {
			ml0 = tipmask[(size_t)op->lt0 * P + k];
			ml1 = tipmask[(size_t)op->lt1 * P + k];
			if (kl == CH_CHERRY_TIP) ml2 = tipmask[(size_t)op->lt2 * P + k];
		}
		if (kr == CH_TIP) mr0 = tipmask[(size_t)op->right * P + k];
		else if (kr >= CH_CHERRY) {
			mr0 = tipmask[(size_t)op->rt0 * P + k];
			mr1 = tipmask[(size_t)op->rt1 * P + k];
			if (kr == CH_CHERRY_TIP) mr2 = tipmask[(size_t)op->rt2 * P + k];
		}
		d4 uin = carry;  // the parent's upper: carried in registers, or parked by an earlier op of this thread
		if (!proot && !cin) {
			if (LPARK && (op->lds_park & 1)) {
				const dv2 lo = park[0], hi = park[WAVE];
				uin = d4{lo.x, lo.y, hi.x, hi.y};
			} else
				uin = load4_stream(upper + ((size_t)op->upper_slot_parent * C + c) * plane + (size_t)k * 4);
		}
		d4 pl = one, pr = one;  // stored children
		if (kl == CH_CORE) pl = load4_stream(lower + ((size_t)op->core_left * C + c) * plane + (size_t)k * 4);
		if (kr == CH_CORE) pr = load4_stream(lower + ((size_t)op->core_right * C + c) * plane + (size_t)k * 4);
		__builtin_amdgcn_s_setprio(0);
		d4 prel = one, prer = one;  // the children's own partials (the parameter gradient contracts them)
		const d4 bl = child_message_m<PARAMS>(x, kl, op->left, op->core_left, op->lt0, op->lt1, op->lt2, op->linner, pl, ml0, ml1, ml2, prel, dl);
		const d4 br = child_message_m<PARAMS>(x, kr, op->right, op->core_right, op->rt0, op->rt1, op->rt2, op->rinner, pr, mr0, mr1, mr2, prer, dr);
		d4 a;
		if (proot) a = FOLD ? pi : one;
		else a = matvec4_opt<PARAMS>(x.M(op->parent), uin);
		d4 ul = mul4(a, br), ur = mul4(a, bl);
		double ml = 1.0, mr = 1.0;
		if (SCALE) {
			// the mixture likelihood in this op's scaled units from all categories (L_k itself underflows by construction)
			const double den = dot4(FOLD ? a : mul4(pi, a), mul4(bl, br));
			// The maxima travel as the high words of the doubles, rounded up (two per 8-byte slot: the exchange then leaves room
			// for the LDS park slots at four workgroups per CU).  An upper's factor cancels in every branch term, so any
			// divisor >= the maximum serves; this one is within 2^-20 of it.
			double *xb = xbase + (size_t)(i & 1) * 2 * xsz;
			int2 *xm = reinterpret_cast<int2 *>(xb + xsz);
			const int xi = wv * WAVE + lane;
			xb[xi] = props[c] * den;
			xm[xi] = int2{__double2hiint(max4(ul)) + 1, __double2hiint(max4(ur)) + 1};
			lds_barrier();
			double D = 0.0;
			int mlh = 0, mrh = 0;
			for (int cc = 0; cc < C; cc++) {
				D += xb[(g * C + cc) * WAVE + lane];
				const int2 m2 = xm[(g * C + cc) * WAVE + lane];
				mlh = max(mlh, m2.x);
				mrh = max(mrh, m2.y);
			}
			ml = __hiloint2double(mlh, 0);
			mr = __hiloint2double(mrh, 0);
			// (D is a product of three factors that rescaling keeps above 1e-40 each: its reciprocal is finite)
			gr.wq = wk / D;
			gr.w = wk;
			gr.d = den;
			gr.wl = wk / D;
		}
		if (kl == CH_TIP) gr.site_tip(x, 0, op->left, ul, bl, ml0);
		else gr.site_vec(x, 0, op->left, ul, bl, prel);
		if (kr == CH_TIP) gr.site_tip(x, 1, op->right, ur, br, mr0);
		else gr.site_vec(x, 1, op->right, ur, br, prer);
		// fringe children continue in registers with the un-rescaled uppers (they share this op's units and denominator)
		if (kl >= CH_CHERRY) descend_fringe_m(x, gr, 2, kl, op->left, op->lt0, op->lt1, op->lt2, op->linner, ul, ml0, ml1, ml2);
		if (kr >= CH_CHERRY) descend_fringe_m(x, gr, 6, kr, op->right, op->rt0, op->rt1, op->rt2, op->rinner, ur, mr0, mr1, mr2);
		if (SCALE) {  // uppers are rescaled like lowers (treelikelihood.c:1414, 1795-1796)
			if (ml < SCALING_THRESHOLD) ul = d4{ul.x / ml, ul.y / ml, ul.z / ml, ul.w / ml};
			if (mr < SCALING_THRESHOLD) ur = d4{ur.x / mr, ur.y / mr, ur.z / mr, ur.w / mr};
		}
		if (LPARK && (op->lds_park & 6)) {
			const d4 &v = (op->lds_park & 2) ? ul : ur;
			park[0] = dv2{v.x, v.y};
			park[WAVE] = dv2{v.z, v.w};
		}
		// (LPARK launches walk the chunked list, where a child parked in LDS has no HBM slot; a cut subtree's upper has one)
		// plain stores: a parked upper is re-read within a subtree's time, and the non-temporal form of these two-halves-per-
		// lane writes measured 2.5 ms slower here (it pays in the post-order walk, whose partials are read a whole pass later)
		if (op->upper_slot_left >= 0 && valid) store4(upper + ((size_t)op->upper_slot_left * C + c) * plane + (size_t)k * 4, ul);
		if (op->upper_slot_right >= 0 && valid) store4(upper + ((size_t)op->upper_slot_right * C + c) * plane + (size_t)k * 4, ur);
		carry = cout == 1 ? ul : ur;
		// Fixed-order sum of each column over the wave's 64 patterns: four lanes per column add 16 entries each in order,
		// then (s0 + s1) + (s2 + s3).  Slots an op did not write hold stale values; their rows are never stored.
		__builtin_amdgcn_wave_barrier();
		double tot = 0.0;
		if (my < NACC) {
			const double *src = wave_cols + my * WCOL + seg;
			tot = src[0];
#pragma unroll
			for (int j = 1; j < 16; j++) tot += src[4 * j];
		}
		tot = quad_swap_add<0xB1>(tot);  // s0 + s1 | s2 + s3
		tot = quad_swap_add<0x4E>(tot);  // (s0 + s1) + (s2 + s3)
		__builtin_amdgcn_wave_barrier();
		if (seg == 0 && my < NACC) {
			int node = -1;  // accumulator -> gradient row (node id); -1 = unused for this op
			switch (my) {
				case 0: node = op->left; break;
				case 1: node = op->right; break;
				case 2: node = kl >= CH_CHERRY ? op->lt0 : -1; break;
				case 3: node = kl >= CH_CHERRY ? op->lt1 : -1; break;
				case 4: node = kl == CH_CHERRY_TIP ? op->linner : -1; break;
				case 5: node = kl == CH_CHERRY_TIP ? op->lt2 : -1; break;
				case 6: node = kr >= CH_CHERRY ? op->rt0 : -1; break;
				case 7: node = kr >= CH_CHERRY ? op->rt1 : -1; break;
				case 8: node = kr == CH_CHERRY_TIP ? op->rinner : -1; break;
				case 9: node = kr == CH_CHERRY_TIP ? op->rt2 : -1; break;
			}
			if (node >= 0) gpart[((size_t)node * C + c) * nblk + slab] = tot;
		}
	}
	if (PARAMS) {  // the 16 eigen-basis sums of this wave (all categories add into the same G_ab: one slab entry per wave)
#pragma unroll
		for (int a = 0; a < 16; a++) col[a * WCOL] = Gab[a];
		__builtin_amdgcn_wave_barrier();
		const double *src = wave_cols + my * WCOL + seg;
		double tot = src[0];
#pragma unroll
		for (int j = 1; j < 16; j++) tot += src[4 * j];
		tot += __shfl_xor(tot, 1, 64);
		tot += __shfl_xor(tot, 2, 64);
		if (seg == 0) gacc[(size_t)my * nblk * C + slab * C + c] = tot;
	}
}

// G2 tables of the tree-walk kernel: Fw[n][c][20] = 16 entries w_c F_ab(t_n r_c) + 4 entries l_a e^{l_a t_n r_c}; F_ab = exp_divided_difference(l_a, l_b, t)
// (phyamd_device.inc: stable at repeated and nearly repeated eigenvalues); root and explicit-matrix nodes get zeros.  4 states.
__global__ void k_eigen_weights(int C, int node_count, const double *__restrict__ model, const double *__restrict__ rates,
                                const double *__restrict__ props, const double *__restrict__ lengths, const uint8_t *__restrict__ is_explicit, int root,
                                double *__restrict__ Fw) {
	const int idx = blockIdx.x * blockDim.x + threadIdx.x;
	if (idx >= node_count * C * 20) return;
	const int e = idx % 20, c = (idx / 20) % C, n = idx / (20 * C);
	double v = 0.0;
	if (n != root && !is_explicit[n]) {
		const double t = lengths[n] * rates[c];
		if (e < 16) {
			v = props[c] * exp_divided_difference(model[e >> 2], model[e & 3], t);
		} else {  // l_a e^{l_a t}: (Q P)'s eigenvalues; the category weight is applied by the caller's epilogue, not here
			const double la = model[e - 16];
			v = la * exp(la * t);
		}
	}
	Fw[idx] = v;
}

// d lnL / d theta = sum_ab B_theta,ab G_ab (B = U^-1 dQ U, [np][16])
__global__ void k_contract_parameters(int np, const double *__restrict__ B, const double *__restrict__ Gsum, double *__restrict__ out) {
	const int th = blockIdx.x * blockDim.x + threadIdx.x;
	if (th >= np) return;
	double s = 0.0;
	for (int ab = 0; ab < 16; ab++) s += B[(size_t)th * 16 + ab] * Gsum[ab];
	out[th] = s;
}

