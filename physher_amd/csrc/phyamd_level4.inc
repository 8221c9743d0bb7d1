// phyamd_level4.inc: level-batched 4-state kernels (k_lower4, k_upper4): one launch per tree level -- included by phyamd_engine.hip inside its anonymous namespace.

// dynamic LDS: 4 * G*C*64 doubles (two double-buffered exchanges) + G doubles (reduction)
template <int WAVES, bool SCALE, bool ROOT>
__global__ __launch_bounds__(WAVES *WAVE) void k_lower4(const NodeOp *__restrict__ ops, int T, int P, int C,
                                                        const uint8_t *__restrict__ tipmask, double *__restrict__ lower,
                                                        const double *__restrict__ mats, const double *__restrict__ tiptab,
                                                        double *__restrict__ lscale,
                                                        const double *__restrict__ freqs, const double *__restrict__ props,
                                                        const double *__restrict__ weights, double *__restrict__ pattern_lk,
                                                        double *__restrict__ w_over_L, double *__restrict__ lnl_part) {
	extern __shared__ double sh[];
	// blockDim.x == 64: threadIdx.y/z are wave-uniform; readfirstlane tells the compiler so (SGPR addressing)
	const int lane = threadIdx.x, c = __builtin_amdgcn_readfirstlane(threadIdx.y), g = __builtin_amdgcn_readfirstlane(threadIdx.z), G = blockDim.z;
	const NodeOp op = ops[blockIdx.y];
	const size_t plane = (size_t)P * 4;  // one category of one node
	double *dst = lower + ((size_t)op.core_parent * C + c) * plane;
	const int xsz = G * C * WAVE;  // one exchange buffer
	double acc = 0.0;

#pragma unroll 1
	for (int q = 0; q < PPT_LOWER; q++) {
		const int k0 = ((blockIdx.x * PPT_LOWER + q) * G + g) * WAVE + lane;
		const bool valid = k0 < P;
		const Ctx4 x{tipmask, mats, tiptab, P, C, c, valid ? k0 : P - 1, T};
		const int k = x.k;
		const d4 a = child_message(x, op.kind_left, op.left, op.core_left, op.lt0, op.lt1, op.lt2, op.linner, lower, plane);
		const d4 b = child_message(x, op.kind_right, op.right, op.core_right, op.rt0, op.rt1, op.rt2, op.rinner, lower, plane);
		d4 out = mul4(a, b);
		double sf = 0.0;
		if (SCALE) {  // SingleTreeLikelihood_scalePartials (treelikelihood.c:1790-1836): max over categories and states
			double *xb = sh + (q & 1) * xsz;
			xb[(g * C + c) * WAVE + lane] = max4(out);
			__syncthreads();
			double m = 0.0;
			for (int cc = 0; cc < C; cc++) m = fmax(m, xb[(g * C + cc) * WAVE + lane]);
			// (m == 0: a tip cell below has an empty state mask.  The reference divides by it -- 0 / 0, and NaN for the pattern and for
			// lnL; the partials stay 0 here and the root gives the pattern log 0 = -inf, as the unscaled evaluation does)
			if (m < SCALING_THRESHOLD && m > 0.0) {
				out = d4{out.x / m, out.y / m, out.z / m, out.w / m};
				sf = log(m);
			}
			if (op.kind_left == CH_CORE) sf += lscale[(size_t)op.core_left * P + k];
			if (op.kind_right == CH_CORE) sf += lscale[(size_t)op.core_right * P + k];
			if (c == 0 && valid) lscale[(size_t)op.core_parent * P + k] = sf;
		}
		if (valid) store4(dst + (size_t)k * 4, out);
		if (ROOT) {  // integrate_partials + node_log_likelihoods + weighted sum (treelikelihood.c:1473-1487)
			double *yb = sh + (2 + (q & 1)) * xsz;
			yb[(g * C + c) * WAVE + lane] = props[c] * (freqs[0] * out.x + freqs[1] * out.y + freqs[2] * out.z + freqs[3] * out.w);
			__syncthreads();
			if (c == 0) {
				double L = 0.0;
				for (int cc = 0; cc < C; cc++) L += yb[(g * C + cc) * WAVE + lane];
				const double lk = log(L) + sf;
				if (valid) {
					const double w = weights[k];
					pattern_lk[k] = lk;
					if (!SCALE) w_over_L[k] = w / L;  // the gradient's w_k / L_k (treelikelihood.c:2879), formed once per pattern
					acc += lk * w;
				}
			}
		}
	}
	if (ROOT) {
		double *red = sh + 4 * xsz;
		const double s = wave_sum(acc);
		if (lane == 0 && c == 0) red[g] = s;
		__syncthreads();
		if (lane == 0 && c == 0 && g == 0) {
			double t = red[0];
			for (int gg = 1; gg < G; gg++) t += red[gg];
			lnl_part[blockIdx.x] = t;
		}
	}
}


// ------------------------------------------------------------------------------------------------
// K7 + K8 fused, 4 states: one level of the pre-order pass
// ------------------------------------------------------------------------------------------------
// For a parent p with children l, r, per (pattern k, category c):
//   a   = P_p u_p                      (parent is the root: a = pi if FOLD else 1)
//   bl  = P_l p_l,  br = P_r p_r
//   u_l = a o br,   u_r = a o bl                                       (treelikelihood.c:2142-2147)
//   den_c  = sum_i f_i a_i bl_i br_i      = L_kc in this branch's (scaled) units
//   num_lc = sum_i f_i u_l,i (Q bl)_i     since (dP/dt) p = Q P p     (treelikelihood.c:2846-2939), f = 1 if FOLD else pi
//   g[l][c] += w_k num_lc / L_k.  Unscaled: w_k / L_k comes from the root kernel.  Rescaled: L_k in this branch's
//   units = sum_c' w_c' den_c' (COMPAT: den_c alone, treelikelihood.c:2851-2870)
// A fringe child continues in registers: its upper is pushed through its cherry (and inner cherry), producing the
// gradients of the 2-4 branches inside it (accumulators e[0..3]).
// upper: slot s at upper + s * C*P*4.  gpart: [(N*C)][nblk] per-block partial sums.
// dynamic LDS: SCALE: 6 * G*C*64 doubles (three double-buffered exchanges); then NACC * waves * 64 doubles (reduction)

constexpr int NACC = 10;  // gradient accumulators per thread: 2 children + 4 + 4 fringe branches
// tree-walk kernel: LDS column stride.  Four lanes add a column: lane s of the four takes entries s, s + 4, s + 8, ... and the stride
// of 68 doubles puts the 32 readers of a half-wave on 32 different bank pairs (contiguous quarters at stride 66 met two- and three-way)
constexpr int WCOL = WAVE + 4;

struct Grad4 {
	cptr Q;
	d4 f;
	double wl;
	double *acc;  // this thread's accumulators in LDS: acc[i * WAVE] (lane-interleaved, conflict-free)
	// substitution-parameter side (PARAMS kernels only): dP/dtheta per (parameter, node, category) and their tip tables
	const double *__restrict__ dpm;    // [NP][N][C][16]
	const double *__restrict__ dptab;  // [NP][T][C][16][4]
	int np, N, T;
	double wc;                         // category proportion: parameter terms are summed over categories
	// acc[i] += w_k / L_k * sum_i f_i u_i (Q b)_i
	__device__ __forceinline__ void add(int i, const d4 &u, const d4 &b) const {
		acc[i * WAVE] += wl * dot4(mul4(f, u), matvec4(opaque(Q), b));
	}
	// acc[NACC + th] += w_c w_k / L_k sum_i f_i u_i (dP_th,node p)_i   (calculate_dlnl_dQ, treelikelihood.c:2472-2580)
	__device__ __forceinline__ void addp_vec(const Ctx4 &x, int node, const d4 &u, const d4 &p) const {
		const d4 fu = mul4(f, u);
		for (int th = 0; th < np; th++) {
			const cptr D = opaque(as_const(dpm + (((size_t)th * N + node) * x.C + x.c) * 16));
			acc[(NACC + th) * WAVE] += wc * wl * dot4(fu, matvec4(D, p));
		}
	}
	__device__ __forceinline__ void addp_tip(const Ctx4 &x, int tip, const d4 &u) const {
		const d4 fu = mul4(f, u);
		const unsigned m = x.tipmask[(size_t)tip * x.P + x.k];
		for (int th = 0; th < np; th++)
			acc[(NACC + th) * WAVE] += wc * wl * dot4(fu, load4(dptab + ((((size_t)th * T + tip) * x.C + x.c) * 16 + m) * 4));
	}
};

// push upper `u` of a fringe child (node `node`) down to its inner branches; accumulators base..base+3:
//   CH_CHERRY     : +0 -> t0, +1 -> t1
//   CH_CHERRY_TIP : +0 -> t0, +1 -> t1 (inside the inner cherry), +2 -> inner, +3 -> t2
// Ordered so that few vectors are live at once (the kernel is register-limited).
// rescaled evaluations: the branch term is w_k num / D_k with D_k the site likelihood in the op's scaled units; the quotient
// is formed first (num and D can both be denormal when a category has underflowed)
struct GradS {
	cptr Q;
	d4 f;
	double w, d;
	double *acc;
	__device__ __forceinline__ void add(int i, const d4 &u, const d4 &b) const { acc[i * WAVE] += w * (dot4(mul4(f, u), matvec4(opaque(Q), b)) / d); }
	__device__ __forceinline__ void addp_vec(const Ctx4 &, int, const d4 &, const d4 &) const {}
	__device__ __forceinline__ void addp_tip(const Ctx4 &, int, const d4 &) const {}
};
// only the substitution-parameter terms of a Grad4 (used next to GradS)
struct GradPOnly {
	const Grad4 &g;
	__device__ __forceinline__ void add(int, const d4 &, const d4 &) const {}
	__device__ __forceinline__ void addp_vec(const Ctx4 &x, int node, const d4 &u, const d4 &p) const { g.addp_vec(x, node, u, p); }
	__device__ __forceinline__ void addp_tip(const Ctx4 &x, int tip, const d4 &u) const { g.addp_tip(x, tip, u); }
};

// HESS: this category's two branch terms, left in the exchange for the categories' mixture (x[i * xsz]: f.(u o Q b),
// x[(NACC + i) * xsz]: f.(u o Q Q b)); nothing is accumulated here
struct GradH {
	cptr Q;
	d4 f;
	double *x;
	int xsz;
	__device__ __forceinline__ void add(int i, const d4 &u, const d4 &b) const {
		const d4 fu = mul4(f, u), qb = matvec4(opaque(Q), b);
		x[i * xsz] = dot4(fu, qb);
		x[(NACC + i) * xsz] = dot4(fu, matvec4(opaque(Q), qb));
	}
	__device__ __forceinline__ void addp_vec(const Ctx4 &, int, const d4 &, const d4 &) const {}
	__device__ __forceinline__ void addp_tip(const Ctx4 &, int, const d4 &) const {}
};

// accumulator / branch term j of an op -> the node whose branch it belongs to (-1: the op has no such term)
__device__ __forceinline__ int term_node(const NodeOp &op, int j) {
	const int kl = op.kind_left, kr = op.kind_right;
	switch (j) {
		case 0: return op.left;
		case 1: return op.right;
		case 2: return kl >= CH_CHERRY ? op.lt0 : -1;
		case 3: return kl >= CH_CHERRY ? op.lt1 : -1;
		case 4: return kl == CH_CHERRY_TIP ? op.linner : -1;
		case 5: return kl == CH_CHERRY_TIP ? op.lt2 : -1;
		case 6: return kr >= CH_CHERRY ? op.rt0 : -1;
		case 7: return kr >= CH_CHERRY ? op.rt1 : -1;
		case 8: return kr == CH_CHERRY_TIP ? op.rinner : -1;
		case 9: return kr == CH_CHERRY_TIP ? op.rt2 : -1;
	}
	return -1;
}

template <bool PARAMS, typename GradT>
__device__ __forceinline__ void descend_fringe(const Ctx4 &x, const GradT &gr, int base, int kind, int node, int t0, int t1, int t2, int inner,
                                               const d4 &u) {
	const d4 b0 = x.tipmsg(t0), b1 = x.tipmsg(t1);
	d4 a2 = matvec4(x.M(node), u);
	if (kind == CH_CHERRY_TIP) {
		const d4 pn = mul4(b0, b1);
		const d4 bn = matvec4(x.M(inner), pn);
		const d4 b2 = x.tipmsg(t2);
		const d4 un = mul4(a2, b2);
		gr.add(base + 2, un, bn);
		gr.add(base + 3, mul4(a2, bn), b2);
		if (PARAMS) {
			gr.addp_vec(x, inner, un, pn);
			gr.addp_tip(x, t2, mul4(a2, bn));
		}
		a2 = matvec4(x.M(inner), un);  // now the upper message entering the inner cherry
	}
	gr.add(base + 0, mul4(a2, b1), b0);
	gr.add(base + 1, mul4(a2, b0), b1);
	if (PARAMS) {
		gr.addp_tip(x, t0, mul4(a2, b1));
		gr.addp_tip(x, t1, mul4(a2, b0));
	}
}

// HESS (phyamd_branch_hessian_diagonal): lnL's first and second derivative in every branch length.  G == 1; workgroup x takes the
// 64-pattern blocks [hwg[2x], hwg[2x + 1]) (never across a segment of reduce_block_sums' bisection: sums do not depend on the shard
// count).  Per pattern every category wave leaves its branch terms n1_jc = f.(u_j o Q b_j), n2_jc = f.(u_j o Q Q b_j) in LDS next to
// w_c den_c, and after one more barrier wave c mixes the terms j = c (mod C) over the categories:
//   A_j = sum_c w_c r_c n1_jc,  B_j = sum_c w_c r_c^2 n2_jc,  D = sum_c w_c den_c
//   d1 += w_k A_j / D,  d2 += w_k (B_j / D - (A_j / D)^2)
// D is the site likelihood in the op's units (rescaled or not), so the scale factors cancel in both ratios.
// hpart: [workgroup][2 N] -- node n's d1 at n, its d2 at N + n.
template <int WAVES, bool SCALE, bool FOLD, bool COMPAT, bool PARAMS, bool HESS>
__global__ __launch_bounds__(WAVES *WAVE, (WAVES == 4 && !PARAMS && !HESS) ? UPPER_MIN_WAVES : 1) void k_upper4(const NodeOp *__restrict__ ops, int T, int P, int C,
                                                        const uint8_t *__restrict__ tipmask, const double *__restrict__ lower,
                                                        double *__restrict__ upper, const double *__restrict__ mats,
                                                        const double *__restrict__ tiptab, const double *__restrict__ Q,
                                                        const double *__restrict__ freqs,
                                                        const double *__restrict__ props, const double *__restrict__ weights,
                                                        const double *__restrict__ w_over_L, double *__restrict__ gpart, int nblk,
                                                        const double *__restrict__ dpm, const double *__restrict__ dptab, int np, int N,
                                                        double *__restrict__ ppart, int op_base, int op_total,
                                                        const double *__restrict__ rates, const int *__restrict__ hwg, double *__restrict__ hpart) {
	static_assert(!HESS || (!FOLD && !COMPAT && !PARAMS), "the Hessian variant is the plain reference arithmetic");
	extern __shared__ double sh[];
	// blockDim.x == 64: threadIdx.y/z are wave-uniform; readfirstlane tells the compiler so (SGPR addressing)
	const int lane = threadIdx.x, c = __builtin_amdgcn_readfirstlane(threadIdx.y), g = __builtin_amdgcn_readfirstlane(threadIdx.z), G = blockDim.z;
	const NodeOp op = ops[blockIdx.y];
	const size_t plane = (size_t)P * 4;
	const bool proot = op.upper_slot_parent < 0;
	const int hc = (NACC + C - 1) / C;  // HESS: branch terms per category wave
	const int nacc = HESS ? 2 * hc : NACC + (PARAMS ? np : 0);  // accumulator columns per thread
	const double *up = proot ? nullptr : upper + ((size_t)op.upper_slot_parent * C + c) * plane;
	double *ul_dst = op.upper_slot_left < 0 ? nullptr : upper + ((size_t)op.upper_slot_left * C + c) * plane;
	double *ur_dst = op.upper_slot_right < 0 ? nullptr : upper + ((size_t)op.upper_slot_right * C + c) * plane;
	const d4 pi = d4{freqs[0], freqs[1], freqs[2], freqs[3]};
	const d4 one = d4{1., 1., 1., 1.};
	const int xsz = G * C * WAVE;
	// gradient accumulators live in LDS (one column per thread), not in registers: the kernel is VGPR-limited
	const int wv = g * C + c, nw = G * C;
	double *red = sh + (HESS ? (6 + 2 * NACC) * xsz : SCALE ? 6 * xsz : 0);
	Grad4 gr{as_const(Q), FOLD ? one : pi, 0.0, red + (size_t)wv * nacc * WAVE + lane, dpm, dptab, np, N, T, props[c]};
	for (int i = 0; i < nacc; i++) gr.acc[i * WAVE] = 0.0;

#pragma unroll 1
	for (int q = 0; q < PPT_UPPER; q++) {
		if (HESS && hwg[2 * blockIdx.x] + q >= hwg[2 * blockIdx.x + 1]) break;  // (the same for every wave of the workgroup)
		const int k0 = HESS ? (hwg[2 * blockIdx.x] + q) * WAVE + lane : ((blockIdx.x * PPT_UPPER + q) * G + g) * WAVE + lane;
		const bool valid = k0 < P;
		const Ctx4 x{tipmask, mats, tiptab, P, C, c, valid ? k0 : P - 1, T};
		const int k = x.k;
		d4 prel = one, prer = one;  // the children's own partials (PARAMS only)
		const d4 bl = PARAMS ? child_message_pre(x, op.kind_left, op.left, op.core_left, op.lt0, op.lt1, op.lt2, op.linner, lower, plane, prel)
		                     : child_message(x, op.kind_left, op.left, op.core_left, op.lt0, op.lt1, op.lt2, op.linner, lower, plane);
		const d4 br = PARAMS ? child_message_pre(x, op.kind_right, op.right, op.core_right, op.rt0, op.rt1, op.rt2, op.rinner, lower, plane, prer)
		                     : child_message(x, op.kind_right, op.right, op.core_right, op.rt0, op.rt1, op.rt2, op.rinner, lower, plane);
		const d4 a = proot ? (FOLD ? pi : one) : matvec4(x.M(op.parent), load4(up + (size_t)k * 4));
		d4 ul = mul4(a, br), ur = mul4(a, bl);
		if (!SCALE && !HESS) {
			// unscaled: divide by the site likelihood formed at the root, like the reference (treelikelihood.c:2879);
			// no cross-category exchange, no barrier, no division in this kernel
			gr.wl = valid ? w_over_L[k] : 0.0;
			gr.add(0, ul, bl);
			gr.add(1, ur, br);
			if (ul_dst && valid) store4(ul_dst + (size_t)k * 4, ul);
			if (ur_dst && valid) store4(ur_dst + (size_t)k * 4, ur);
			if (PARAMS) {
				if (op.kind_left == CH_TIP) gr.addp_tip(x, op.left, ul);
				else gr.addp_vec(x, op.left, ul, prel);
				if (op.kind_right == CH_TIP) gr.addp_tip(x, op.right, ur);
				else gr.addp_vec(x, op.right, ur, prer);
			}
			if (op.kind_left >= CH_CHERRY) descend_fringe<PARAMS>(x, gr, 2, op.kind_left, op.left, op.lt0, op.lt1, op.lt2, op.linner, ul);
			if (op.kind_right >= CH_CHERRY) descend_fringe<PARAMS>(x, gr, 6, op.kind_right, op.right, op.rt0, op.rt1, op.rt2, op.rinner, ur);
			continue;
		} else {
			// rescaled: L_k underflows by construction, so the mixture likelihood is re-formed
			// in this branch's scaled units from all categories' den (exchange through LDS); the scale factors cancel in num / D
			const double den = dot4(mul4(gr.f, a), mul4(bl, br));
			const double numl = HESS ? 0.0 : dot4(mul4(gr.f, ul), matvec4(opaque(gr.Q), bl));
			const double numr = HESS ? 0.0 : dot4(mul4(gr.f, ur), matvec4(opaque(gr.Q), br));
			double *xb = sh + (q & 1) * 3 * xsz;
			const int xi = (g * C + c) * WAVE + lane;
			xb[xi] = props[c] * den;
			xb[xsz + xi] = max4(ul);
			xb[2 * xsz + xi] = max4(ur);
			__syncthreads();
			double D = 0.0, ml = 0.0, mr = 0.0;
			for (int cc = 0; cc < C; cc++) {
				D += xb[(g * C + cc) * WAVE + lane];
				ml = fmax(ml, xb[xsz + (g * C + cc) * WAVE + lane]);
				mr = fmax(mr, xb[2 * xsz + (g * C + cc) * WAVE + lane]);
			}
			// num / L first: with COMPAT both can be denormal (a category that has underflowed) and 1 / den alone overflows
			const double w = valid ? weights[k] : 0.0, d = COMPAT ? den : D;
			if (HESS) {
				double *hx = sh + 6 * xsz;  // [2 NACC][waves][64] branch terms
				const GradH gh{gr.Q, gr.f, hx + xi, xsz};
				gh.add(0, ul, bl);
				gh.add(1, ur, br);
				if (op.kind_left >= CH_CHERRY) descend_fringe<false>(x, gh, 2, op.kind_left, op.left, op.lt0, op.lt1, op.lt2, op.linner, ul);
				if (op.kind_right >= CH_CHERRY) descend_fringe<false>(x, gh, 6, op.kind_right, op.right, op.rt0, op.rt1, op.rt2, op.rinner, ur);
				__syncthreads();
				for (int j = c, m = 0; j < NACC; j += C, m++) {
					if (term_node(op, j) < 0) continue;
					double A = 0.0, B = 0.0;
					for (int cc = 0; cc < C; cc++) {
						const double wr = props[cc] * rates[cc];
						A += wr * hx[j * xsz + (g * C + cc) * WAVE + lane];
						B += wr * rates[cc] * hx[(NACC + j) * xsz + (g * C + cc) * WAVE + lane];
					}
					const double a1 = A / D;
					gr.acc[m * WAVE] += w * a1;
					gr.acc[(hc + m) * WAVE] += w * (B / D - a1 * a1);
				}
			} else {
				gr.acc[0] += w * (numl / d);
				gr.acc[WAVE] += w * (numr / d);
				if (PARAMS) {  // mixture numerator over the mixture likelihood in this branch's units (treelikelihood.c:2545-2556)
					gr.wl = w / D;
					if (op.kind_left == CH_TIP) gr.addp_tip(x, op.left, ul);
					else gr.addp_vec(x, op.left, ul, prel);
					if (op.kind_right == CH_TIP) gr.addp_tip(x, op.right, ur);
					else gr.addp_vec(x, op.right, ur, prer);
				}
				// Fringe children (fused schedules run rescaled too): a cherry or cherry + tip never reaches the rescaling threshold
				// (products of two or three transition probabilities), so its likelihood is in this op's units and shares D
				if (op.kind_left >= CH_CHERRY || op.kind_right >= CH_CHERRY) {
					const GradS gs{gr.Q, gr.f, w, d, gr.acc};
					if (op.kind_left >= CH_CHERRY) descend_fringe<false>(x, gs, 2, op.kind_left, op.left, op.lt0, op.lt1, op.lt2, op.linner, ul);
					if (op.kind_right >= CH_CHERRY) descend_fringe<false>(x, gs, 6, op.kind_right, op.right, op.rt0, op.rt1, op.rt2, op.rinner, ur);
					if (PARAMS) {
						const GradPOnly gp{gr};  // gr.wl = w / D from above
						if (op.kind_left >= CH_CHERRY) descend_fringe<true>(x, gp, 2, op.kind_left, op.left, op.lt0, op.lt1, op.lt2, op.linner, ul);
						if (op.kind_right >= CH_CHERRY) descend_fringe<true>(x, gp, 6, op.kind_right, op.right, op.rt0, op.rt1, op.rt2, op.rinner, ur);
					}
				}
			}
			// uppers are rescaled like lowers (treelikelihood.c:1414, 1795-1796)
			if (SCALE && ml < SCALING_THRESHOLD) ul = d4{ul.x / ml, ul.y / ml, ul.z / ml, ul.w / ml};
			if (SCALE && mr < SCALING_THRESHOLD) ur = d4{ur.x / mr, ur.y / mr, ur.z / mr, ur.w / mr};
		}
		if (ul_dst && valid) store4(ul_dst + (size_t)k * 4, ul);
		if (ur_dst && valid) store4(ur_dst + (size_t)k * 4, ur);
	}
	// Fixed-order reduction over the workgroup's patterns: the accumulators sit in LDS as [wave][acc][lane];
	// one lane per (wave, accumulator) adds the 64 entries in lane order; wave 0 of each category adds the pattern groups.
	__syncthreads();
	if (lane < nacc) {
		const double *src = red + ((size_t)wv * nacc + lane) * WAVE;
		double s0 = src[0], s1 = src[16], s2 = src[32], s3 = src[48];  // four chains of 16, then a fixed combine
		for (int j = 1; j < 16; j++) {
			s0 += src[j];
			s1 += src[16 + j];
			s2 += src[32 + j];
			s3 += src[48 + j];
		}
		const double s = (s0 + s1) + (s2 + s3);
		red[(size_t)nw * nacc * WAVE + wv * nacc + lane] = s;
	}
	__syncthreads();
	const double *tot = red + (size_t)nw * nacc * WAVE;
	if (HESS) {  // G == 1: one slab entry per workgroup and node
		const int j = c + lane * C;
		const int node = lane < hc && j < NACC ? term_node(op, j) : -1;
		if (node >= 0) {
			hpart[(size_t)blockIdx.x * 2 * N + node] = tot[c * nacc + lane];
			hpart[(size_t)blockIdx.x * 2 * N + N + node] = tot[c * nacc + hc + lane];
		}
		return;
	}
	if (g == 0 && lane < NACC) {
		double s = tot[c * nacc + lane];
		for (int gg = 1; gg < G; gg++) s += tot[(gg * C + c) * nacc + lane];
		// accumulator -> gradient row (node id); -1 = unused for this op (the same map as term_node, kept written out: calling it here
		// changes the register allocation of the existing instantiations)
		const int kl = op.kind_left, kr = op.kind_right;
		int node = -1;
		switch (lane) {
			case 0: node = op.left; break;
			case 1: node = op.right; break;
			case 2: node = kl >= CH_CHERRY ? op.lt0 : -1; break;
			case 3: node = kl >= CH_CHERRY ? op.lt1 : -1; break;
			case 4: node = kl == CH_CHERRY_TIP ? op.linner : -1; break;
			case 5: node = kl == CH_CHERRY_TIP ? op.lt2 : -1; break;
			case 6: node = kr >= CH_CHERRY ? op.rt0 : -1; break;
			case 7: node = kr >= CH_CHERRY ? op.rt1 : -1; break;
			case 8: node = kr == CH_CHERRY_TIP ? op.rinner : -1; break;
			case 9: node = kr == CH_CHERRY_TIP ? op.rt2 : -1; break;
		}
		if (node >= 0) gpart[((size_t)node * C + c) * nblk + blockIdx.x] = s;
	}
	if (PARAMS && wv == 0 && lane < np) {  // parameter terms: sum over all waves (categories and pattern groups) in a fixed order
		double s = 0.0;
		for (int w = 0; w < nw; w++) s += tot[w * nacc + NACC + lane];
		ppart[((size_t)lane * op_total + op_base + blockIdx.y) * nblk + blockIdx.x] = s;
	}
}

