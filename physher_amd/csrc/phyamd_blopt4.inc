// phyamd_blopt4.inc: 4-state kernels of phyamd_optimize_branch_lengths -- every branch length of a batch of trees optimised one
// branch at a time, pass after pass, on the device -- included by phyamd_engine.hip inside its anonymous namespace.
//
// The start state is the tree batch's lnL-only walk (k_batch_walk4<false>, grad = 0): every internal lower p_n of every item in the
// batch scratch, the items' matrices beside them.  A pass is the depth-first tour of build_branch_sweep (phyamd_tree_schedule.h):
// for a non-root node n with parent m and sibling s
//   O_n = A_m o msg(s),   A_m = P_m O_m (ones when m is the root),   msg(x) = P_x p_x (P_x . mask for a tip),
// one plane per node, formed on the way down; p_n = msg(left) o msg(right) formed again on the way up, after both children's
// branches have moved; then the visit of n.  With O_n and p_n current the site likelihood is k_cbopt_coeff4's exponential sum in
// t_n, K[c][a] = w_c (V^T (pi o O_n))_a (V^-1 p_n)_a, and the visit is k_cbopt_solve4's iteration on it (cbopt_evaluate, the same
// fixed-order sums) followed by the accept test.  Every item has 2 (T - 1) visit slots; slot i of all items of a chunk runs in
// lockstep with two launches, k_blopt_step4 (the item's partial operations in front of the visit, then K) and k_blopt_solve4
// (the rule, the new length and matrices, at the pass's last slot the stop test).  A workgroup reads and writes cells of its own
// item only, and in k_blopt_step4 of its own lanes only: no workgroup waits for another, and an item's arithmetic depends on
// nothing but its own tree and lengths.

// an op of an item's tour (SweepOp without the visit index) and a visit slot: the node, its ops [begin, end), whether it ends a pass
struct BloptOp {
	int32_t kind, node, a, b;
	int32_t pad[4];
};
struct BloptVisit {
	int32_t node, begin, end, last;
	int32_t pad[4];
};

// an item's word of status: BLOPT_DONE != 0 ends it (both kernels return at their top)
enum { BLOPT_DONE = 0, BLOPT_PASSES = 1, BLOPT_VISITS = 2, BLOPT_ITERATIONS = 3, BLOPT_STATUS = 4 };

struct BloptStepArgs {
	const BloptOp *ops;         // [item][ops_stride]
	const BloptVisit *visits;   // [item][visits_stride]
	int ops_stride, visits_stride, step;
	int T, N, P, C, nblk;
	const uint8_t *tipmask;     // [T][P]
	const double *freqs, *props;
	const double *model;        // eval [4] | evec [4][4] | ivec [4][4]
	const uint8_t *optimise;    // [item][N]
	const int32_t *status;      // [item][BLOPT_STATUS]
	const double *mats;         // [item][N][C][16]
	double *lower;              // [item][T - 1][C][nblk * 64][4]
	double *O;                  // [item][N][C][nblk * 64][4]
	double *K;                  // [item][C][4][nblk * 64]
};

// grid (nblk, items), block (64, C): the C category waves of 64 patterns of one item (k_batch_walk4's shape)
__global__ __launch_bounds__(BATCH_MAX_CATEGORIES *WAVE) void k_blopt_step4(const BloptStepArgs a) {
	const int lane = threadIdx.x, c = __builtin_amdgcn_readfirstlane(threadIdx.y);  // this wave's category
	const int item = blockIdx.y;
	if (a.status[(size_t)item * BLOPT_STATUS + BLOPT_DONE]) return;
	const BloptVisit v = load_const_record<4>(a.visits + (size_t)item * a.visits_stride, a.step);
	const BloptOp *ops = a.ops + (size_t)item * a.ops_stride;
	const int k0 = blockIdx.x * WAVE + lane;  // the scratch is padded to whole blocks and the walk has written every lane's cells
	const int k = k0 < a.P ? k0 : a.P - 1;
	const size_t Pp = (size_t)a.nblk * WAVE, plane = Pp * 4, node_stride = (size_t)a.C * plane;
	const cptr mats_c = as_const(a.mats + ((size_t)item * a.N * a.C + c) * 16);
	double *lower_c = a.lower + (size_t)item * (a.T - 1) * node_stride + (size_t)c * plane + (size_t)k0 * 4;
	double *O_c = a.O + (size_t)item * a.N * node_stride + (size_t)c * plane + (size_t)k0 * 4;
	const auto message = [&](int child) { return child_message4(mats_c + (size_t)child * a.C * 16, a.tipmask + k, a.P, lower_c, node_stride, a.T, child); };
#pragma unroll 1
	for (int i = v.begin; i < v.end; i++) {
		const BloptOp op = load_const_record<4>(ops, i);
		if (op.kind == SWEEP_UPPER) {
			const d4 ms = message(op.b);
			d4 A = d4{1., 1., 1., 1.};
			if (op.a != BATCH_ROOT) A = matvec4(opaque(mats_c + (size_t)op.a * a.C * 16), load4(O_c + (size_t)op.a * node_stride));
			store4(O_c + (size_t)op.node * node_stride, mul4(A, ms));
		} else {
			const d4 l = message(op.a), r = message(op.b);
			store4(lower_c + (size_t)(op.node - a.T) * node_stride, mul4(l, r));
		}
	}
	if (!a.optimise[(size_t)item * a.N + v.node] && !v.last) return;  // nobody evaluates this branch
	const d4 fU = mul4(d4{a.freqs[0], a.freqs[1], a.freqs[2], a.freqs[3]}, load4(O_c + (size_t)v.node * node_stride));  // pi o O_n
	const d4 p = v.node < a.T ? mask4(a.tipmask[(size_t)v.node * a.P + k]) : load4(lower_c + (size_t)(v.node - a.T) * node_stride);
	const cptr V = as_const(a.model + 4), Vi = as_const(a.model + 20);
	const d4 q = matvec4(opaque(Vi), p);  // V^-1 p
	const cptr W = opaque(V);
	d4 g;                                 // V^T (pi o O_n)
	g.x = W[0] * fU.x + W[4] * fU.y + W[8] * fU.z + W[12] * fU.w;
	g.y = W[1] * fU.x + W[5] * fU.y + W[9] * fU.z + W[13] * fU.w;
	g.z = W[2] * fU.x + W[6] * fU.y + W[10] * fU.z + W[14] * fU.w;
	g.w = W[3] * fU.x + W[7] * fU.y + W[11] * fU.z + W[15] * fU.w;
	const double wc = a.props[c];
	double *Kc = a.K + ((size_t)item * a.C + c) * 4 * Pp + k0;  // one 512-byte row segment per wave each
	Kc[0] = wc * (g.x * q.x);
	Kc[Pp] = wc * (g.y * q.y);
	Kc[2 * Pp] = wc * (g.z * q.z);
	Kc[3 * Pp] = wc * (g.w * q.w);
}

struct BloptSolveArgs {
	const BloptVisit *visits;  // [item][visits_stride]
	int visits_stride, step, pass, max_passes;
	int N, P, C, Pp;
	int max_iterations;
	double lower, upper, tolerance, lnl_tolerance;
	const double *model;       // eval [4] | evec [4][4] | ivec [4][4]
	const double *rates, *weights;
	const uint8_t *optimise;   // [item][N]
	const double *K;           // [item][C][4][Pp]
	double *lengths;           // [item][N]: the item's state
	double *mats;              // [item][N][C][16]
	double *lnl;               // [item][2]: lnL after the previous pass (the start's before the first) | lnL now
	int32_t *status;           // [item][BLOPT_STATUS]
};

// grid (items), block 256: one visit of one item (the rule of include/physher_amd.h), every thread with the same bits
__global__ __launch_bounds__(CBOPT_THREADS) void k_blopt_solve4(const BloptSolveArgs a) {
	__shared__ double sh_e[3 * 4 * BATCH_MAX_CATEGORIES], sh_w[3 * CBOPT_WAVES];
	const int item = blockIdx.x;
	int32_t *status = a.status + (size_t)item * BLOPT_STATUS;
	if (status[BLOPT_DONE]) return;
	const BloptVisit v = load_const_record<4>(a.visits + (size_t)item * a.visits_stride, a.step);
	const bool visited = a.optimise[(size_t)item * a.N + v.node] != 0;
	if (!visited && !v.last) return;
	CboptSolveArgs ev{};  // what cbopt_evaluate reads
	ev.P = a.P, ev.C = a.C, ev.Pp = a.Pp, ev.model = a.model, ev.rates = a.rates, ev.weights = a.weights;
	const double *K = a.K + (size_t)item * a.C * 4 * a.Pp;
	double *length = a.lengths + (size_t)item * a.N + v.node;
	// (a node that is not visited is evaluated where it stands: the last slot of a pass gives the pass's lnL)
	const double t0 = visited ? fmin(fmax(*length, a.lower), a.upper) : *length;
	double t = t0, lo = a.lower, hi = a.upper;
	double lnl, d1, d2, lnl0 = 0.0;
	bool bad = false;
	int n = 0;
	while (n < (visited ? a.max_iterations : 1)) {
		cbopt_evaluate(ev, K, t, n == 0, sh_e, sh_w, &lnl, &d1, &d2, &bad);
		if (n == 0) lnl0 = lnl;
		n++;
		if (bad || !visited) break;  // lnL is not finite at this iterate: it ends the item
		const double next = newton_propose(t, d1, d2, lo, hi);
		const bool converged = fabs(next - t) <= a.tolerance;
		t = next;
		if (converged) break;
	}
	double now = lnl0;  // lnL at the length the visit leaves
	if (bad) {
		if (n > 1) cbopt_evaluate(ev, K, t, true, sh_e, sh_w, &lnl0, &d1, &d2, &bad);  // the value that is not finite
		if (threadIdx.x == 0) {
			a.lnl[(size_t)item * 2 + 1] = isnan(lnl0) || isinf(lnl0) ? lnl0 : NAN;
			status[BLOPT_PASSES] = -a.pass;
			status[BLOPT_ITERATIONS] += n;
			status[BLOPT_DONE] = 1;
		}
		return;
	}
	if (visited) {
		bool worse;
		cbopt_evaluate(ev, K, t, true, sh_e, sh_w, &lnl, &d1, &d2, &worse);
		const bool accept = !worse && !(isnan(lnl) || isinf(lnl)) && lnl >= lnl0;
		const double tn = accept ? t : t0;
		if (accept) now = lnl;
		if (threadIdx.x == 0) {
			*length = tn;
			status[BLOPT_VISITS] += 1;
			status[BLOPT_ITERATIONS] += n;
		}
		if (threadIdx.x < 16 * a.C) {  // P_n(t_n r_c) of every category: k_batch_matrices' arithmetic
			const int j = threadIdx.x & 3, i = (threadIdx.x >> 2) & 3, c = threadIdx.x >> 4;
			const double *eval = a.model, *evec = a.model + 4, *ivec = a.model + 20;
			const double x = tn * a.rates[c];
			double p = 0.;
			for (int s = 0; s < 4; s++) p += ivec[s * 4 + j] * evec[i * 4 + s] * exp(eval[s] * x);
			a.mats[(((size_t)item * a.N + v.node) * a.C + c) * 16 + i * 4 + j] = fabs(p);  // substmodel.c:552
		}
	}
	if (threadIdx.x == 0) {
		a.lnl[(size_t)item * 2 + 1] = now;
		if (v.last) {  // the stop test
			if (now - a.lnl[(size_t)item * 2] <= a.lnl_tolerance) status[BLOPT_PASSES] = a.pass, status[BLOPT_DONE] = 1;
			else if (a.pass == a.max_passes) status[BLOPT_PASSES] = -a.max_passes, status[BLOPT_DONE] = 1;
			a.lnl[(size_t)item * 2] = now;
		}
	}
}
