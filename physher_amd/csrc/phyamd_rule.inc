// phyamd_rule.inc: the branch-length rule of include/physher_amd.h on the device, written once -- included by phyamd_engine.hip inside
// its anonymous namespace, before the kernels that run it.  No kernel and no LDS of its own: a kernel passes lambdas that close
// over its own arguments and LDS arrays, and everything here is inlined into it.
//
// Every evaluation `evaluate(t, final, &lnl, &d1, &d2, &bad)` leaves the same bits in every thread of the workgroup (fixed-order
// sums: cbopt_evaluate and its kin), so every thread takes the same accept, bisect and stop decisions and the barriers inside the
// lambdas are met by all.  final: lnL is wanted too; bad: lnL at t is not finite.
//   newton_propose     the safeguarded step: all seven solve kernels (k_blopt_solve4 keeps its own loop, one visit per launch)
//   solve_one_length   one length from a start: k_cbopt_solve4, k_pairdist_solve4, k_classpair_solve
//   three_branch_rule  three lengths that meet at a node, one at a time, pass after pass: k_tripod_solve4, k_qopt_solve4,
//                      k_classopt_solve

// the root of d1 lies on the side of t that d1's sign names: the bracket (lo, hi) shrinks to it, and the next iterate is the
// Newton step where the curvature is negative and the step stays inside the bracket, else the bracket's middle
__device__ __forceinline__ double newton_propose(double t, double d1, double d2, double &lo, double &hi) {
	if (d1 > 0.0) lo = t;
	else hi = t;
	double next = t - d1 / d2;
	if (!(d2 < 0.0 && lo < next && next < hi)) next = 0.5 * (lo + hi);
	return next;
}

// the whole iteration of one length from `start` (clamped), and thread 0's record: out4 = t*, lnL, d1, d2 at t* (the derivatives NaN
// where lnL is not finite); *iterations = proposals made, negated where the iteration did not converge
template <class Evaluate>
__device__ __forceinline__ void solve_one_length(const Evaluate &evaluate, double start, double lower, double upper, double tolerance, int max_iterations, double *out4,
                                                 int32_t *iterations) {
	double t = fmin(fmax(start, lower), upper), lo = lower, hi = upper;
	double lnl, d1, d2;
	bool bad;
	int n = 0, converged = 0;
	while (n < max_iterations) {
		evaluate(t, false, &lnl, &d1, &d2, &bad);
		n++;
		if (bad) break;  // lnL is not finite at this iterate: it is the report
		const double next = newton_propose(t, d1, d2, lo, hi);
		converged = fabs(next - t) <= tolerance;
		t = next;
		if (converged) break;
	}
	evaluate(t, true, &lnl, &d1, &d2, &bad);
	if (threadIdx.x == 0) {
		const bool finite = !(isnan(lnl) || isinf(lnl));
		out4[0] = t;
		out4[1] = lnl;
		out4[2] = finite ? d1 : NAN;
		out4[3] = finite ? d2 : NAN;
		*iterations = converged && finite ? n : -n;
	}
}

enum { RULE_PASSES = 0, RULE_VISITS = 1, RULE_ITERATIONS = 2, RULE_STATUS = 4 };  // a candidate's status words

// Three lengths (t0, t1, t2), in the order of the caller's `lengths`, the last the branch above the node where the three meet.  One
// loop over the start (slot -1: lnl_0 in the length of branch 2, as it is given) and the visits of the slots 0, 1, 2 whose bit is set
// in `branches` (1..7), one over a visit's evaluations, so that `coefficients` and `evaluate` are expanded once each.  EVERY_SLOT:
// `branches` is 7 and no slot is looked for -- known when the template is expanded, not found out by the optimiser afterwards: the
// kernels sit at their register limits, and k_tripod_solve4 spills a scalar register once the loop below is folded away late.
// branch_of(slot): the branch a slot visits; coefficients(z, t0, t1, t2): the visit of branch z begins at these lengths.  Thread
// 0's record: out = t0, t1, t2, lnl, initial_lnl; status [RULE_*]
template <bool EVERY_SLOT, class Coefficients, class Evaluate, class BranchOf>
__device__ __forceinline__ void three_branch_rule(const Coefficients &coefficients, const Evaluate &evaluate, const BranchOf &branch_of, int branches, double t0, double t1,
                                                  double t2, double lower, double upper, double tolerance, int max_iterations, double lnl_tolerance, int max_passes,
                                                  double *out, int32_t *status) {
	const int first = branches & 1 ? 0 : branches & 2 ? 1 : 2;
	double initial = 0.0, previous = 0.0, result = 0.0;
	int passes = 0, visits = 0, iterations = 0;
	int pass = 1, slot = -1;
#pragma unroll 1
	while (passes == 0) {
		const int z = slot < 0 ? 2 : branch_of(slot);
		coefficients(z, t0, t1, t2);
		const double tz = z == 0 ? t0 : z == 1 ? t1 : t2;
		const double from = slot < 0 ? tz : fmin(fmax(tz, lower), upper);
		double t = from, lo = lower, hi = upper, lnl = 0.0, lnl0 = 0.0, d1, d2;
		int n = 0;
		bool last = slot < 0, bad = false, wrong;  // last: the evaluation that ends the visit (the start has no other)
#pragma unroll 1
		for (;;) {
			evaluate(t, n == 0 || last, &lnl, &d1, &d2, &wrong);
			if (last) break;
			if (n == 0) lnl0 = lnl;
			n++;
			if (wrong) {  // lnL is not finite at this iterate: it ends the candidate, with the value there
				bad = true;
				if (n == 1) break;
				last = true;
				continue;
			}
			const double next = newton_propose(t, d1, d2, lo, hi);
			last = fabs(next - t) <= tolerance || n == max_iterations;
			t = next;
		}
		if (slot < 0) {
			initial = previous = result = lnl;
			slot = first;
			continue;
		}
		iterations += n;
		if (bad) {
			result = isnan(lnl) || isinf(lnl) ? lnl : NAN;
			passes = -pass;
			break;
		}
		const bool accept = !wrong && !(isnan(lnl) || isinf(lnl)) && lnl >= lnl0;
		const double tn = accept ? t : from;
		result = accept ? lnl : lnl0;  // lnL at the length the visit leaves
		if (z == 0) t0 = tn;
		else if (z == 1) t1 = tn;
		else t2 = tn;
		visits++;
		do slot++;
		while (!EVERY_SLOT && slot < 3 && !(branches >> slot & 1));
		if (slot < 3) continue;
		if (result - previous <= lnl_tolerance) passes = pass;  // the stop test
		else if (pass == max_passes) passes = -max_passes;
		previous = result;
		slot = first, pass++;
	}
	if (threadIdx.x == 0) {
		out[0] = t0, out[1] = t1, out[2] = t2, out[3] = result, out[4] = initial;
		status[RULE_PASSES] = passes, status[RULE_VISITS] = visits, status[RULE_ITERATIONS] = iterations;
	}
}
