// phyamd_walk4s.inc -- the plain pre-order tree walk as a software pipeline (k_upper4_stream), included by phyamd_engine.hip inside
// its anonymous namespace after phyamd_walk4.inc.  Same schedule, park slots and chunking as k_upper4_walk<.., LPARK> (update_upper_partials
// + gradient_cat_branch_lengths + calculate_branch_partials, treelikelihood.c:2129-2161, 2793-2941), different plumbing:
//
//   * NOTHING AN OP READS IS REQUESTED BY THAT OP.  k_upper4_walk read a byte per (tip, pattern), then gathered a table row, then
//     loaded its stored operands: dependent memory round trips at the top of every op, and ~56 % of its wave time in s_waitcnt.
//     Here op i requests, while it computes, everything op i + 1 needs (descriptor fields nx_* of op i say what that is):
//       - MASK WORDS: the 4-bit tip codes of an op, packed per pattern into one dword per child that has tips (up to six nibbles),
//         laid out in walk order [word][pattern] -- one coalesced dword per lane;
//       - STORED OPERANDS (CORE children, an upper parked in HBM) into two register sets A / B;
//       - the op's TABLE BLOCK: its tips' messages P . e_s (and, for tips whose branch term is formed in this op, Qs P . e_s)
//         for every state and for "unknown", 2 KB per (op, category), rebuilt from the matrices once per evaluation
//         (k_op_tables) and copied into LDS by two LDS-DMA instructions (global_load_lds_dwordx4: no registers, no VALU).
//     An op then waits once, at its top (s_waitcnt vmcnt(0)), and a tip message is a 32-byte LDS read at [slot][code].
//   * REDUCTION ON THE MATRIX PIPE.  A branch term is one double per lane; v_mfma_f64_4x4x4_4b with a row selector as A and the
//     term as B adds the four 16-lane groups and drops the result in row r of an accumulator (D_blk[i][j] = sum_k A_blk[i][k]
//     B_blk[k][j]; lane = 16 k + 4 blk + j), so ten terms land in three registers without touching LDS; two DPP halving steps fold
//     the registers into one and two quad steps finish 16 -> 1.  Fixed order: results are reproducible run to run.
//   * TIP BRANCH TERMS WITHOUT THE MAT-VEC.  For a tip, Qs (P e_s) is a table row too (the block holds it), so half of all branch
//     terms cost a dot product instead of a 4 x 4 mat-vec and a dot product.
//   * w_k / L_k rides in the uppers (folded in at the root, everything below is linear in it): no per-term multiply.
//   * The host orders every op's children so that the child whose upper is carried to the next op is the LEFT one: the carried
//     upper is never copied or selected.
//   * SLAB IN WALK ORDER.  gslab[(wave, category)][q], q = the branch's position in the walk: the results of an op are
//     neighbours, successive ops fill successive lines (the [row][block] slab scattered every store into a line of its own).
//   * ONE descriptor per op (128 bytes, DEEP children flattened into it).
//
// Four waves per SIMD (<= 128 registers): the prefetch needs registers, and with its operands already there a wave is rarely
// parked on memory, so the fifth wave buys less than the registers do.

// (StreamOp, StreamDesc, StreamChunk, HK_* / SU_* and the table block's layout OPBLK_*: phyamd_types.h)

// Mask words (packed): one dword row per pattern, mstream[row * mstride + k] (mstride = patterns rounded up to whole waves; the tail
// holds gaps).  A GROUP = the tips of one child of one op: bit 0 = "a nibble of this group holds a partial ambiguity code", then
// nibble j (bits 1 + 4 j ...) = the ROW of the child's j-th tip in its table: 0..3 = that state, 4 = gap / unknown, 5..14 = the ten
// partial ambiguity masks (IUPAC R, Y, ... = 3, 5, 6, 7, 9, 10, 11, 12, 13, 14; the AMBIG instantiation of the walk forms such a tip's
// rows as the sum of its states' rows: P . mask is linear in the mask).  Groups are packed in walk order, several to a dword, none
// across a dword boundary (pack_mask_groups): an op names its groups by (row, shift), its second group sits in the first one's row
// or the next.  Each walk has a stream of its own in its own op order, so successive ops mostly re-read the row they already
// have: the pre-order walk fetches 0.9 GB of words per category at the headline shape, the post-order walk 0.7 (one dword per child
// and op: 1.7 GB each).  That matters because the four category workgroups of a block group each fetch the words, and reads mixed
// into the post-order pass's write stream cost it 0.37 ms per GB (profiles/microbench/lower_stream_replay.hip).
// A mask of 0 (no state possible) sets bit 0 of *flags: the engine keeps the table-gather kernel, whose 16-row tables cover it;
// bit 1: some group holds a partial ambiguity code.
// row_entries: [rows][8] tip | nibble's bit position << 20 | group's flag bit position << 25 (-1: unused)
__global__ __launch_bounds__(256) void k_build_mask_stream(int rows, int P, size_t mstride, const int *__restrict__ row_entries, const uint8_t *__restrict__ tipmask,
                                                           uint32_t *__restrict__ mstream, int *__restrict__ flags) {
	const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (k >= mstride) return;
	bool bad = false, amb = false;
	for (int w = blockIdx.y; w < rows; w += gridDim.y) {
		uint32_t v = 0;
		for (int j = 0; j < 8; j++) {
			const int ent = row_entries[w * 8 + j];  // wave-uniform
			if (ent < 0) continue;
			const int t = ent & 0xFFFFF, pos = (ent >> 20) & 31, fpos = (ent >> 25) & 31;
			const uint32_t m = (k < (size_t)P ? tipmask[(size_t)t * P + k] : 0xFu) & 0xFu;
			// code of mask m: one state -> 0..3, all -> 4, the partial masks in increasing order -> 5..14 (AMBIG_MASKS below)
			const uint32_t code = m == 1 ? 0 : m == 2 ? 1 : m == 4 ? 2 : m == 8 ? 3 : (m == 15 || m == 0) ? 4 : m == 3 ? 5 : m < 8 ? m + 1 : m;
			bad |= m == 0;
			if (code >= 5) {
				amb = true;
				v |= 1u << fpos;
			}
			v |= code << pos;
		}
		mstream[(size_t)w * mstride + k] = v;
	}
	if (bad || amb) atomicOr(flags, (bad ? 1 : 0) | (amb ? 2 : 0));
}

// the table blocks of one evaluation: grid (ops, C), 64 threads; op_tips: [ops][12] (left child's tips 0..5, right 6..11),
// op_deep: bit 0 / 1 = the left / right child is a DEEP node, bit 2 = a pair op's block (OPBLK_PAIR_SITES, phyamd_types.h; pair_tab:
// [ops][16], its position table), site_tab: [ops][16], Qs: 4 x 4 row-major
__global__ __launch_bounds__(64) void k_op_tables(int nops, int C, const int *__restrict__ op_tips, const int *__restrict__ op_deep, const int *__restrict__ site_tab,
                                                  const int *__restrict__ pair_tab, const double *__restrict__ mats, const double *__restrict__ Qs, double *__restrict__ optab) {
	const int op = blockIdx.x, c = blockIdx.y, t = threadIdx.x;
	double *blk = optab + ((size_t)c * nops + op) * (OPBLK_BYTES / 8);
	if (t < 16) reinterpret_cast<int *>(blk)[t] = site_tab[op * 16 + t];
	const int deep = op_deep[op];
	const bool pair = (deep >> 2) & 1;
	if (t >= 16 && t < 32) reinterpret_cast<int *>(blk)[OPBLK_PAIR_SITES / 4 + t - 16] = pair ? pair_tab[op * 16 + t - 16] : -1;
	const bool sib_tip = pair && op_tips[op * 12 + 6] >= 0;
	for (int e = t; e < 2 * 120; e += 64) {  // 2 sides x 120 doubles
		const int side = e / 120, f = e % 120;
		const bool dp = (deep >> side) & 1;
		// DEEP: slot = f / 20, rows of P; otherwise slot = f / 40, first 20 doubles rows of P, next 20 rows of Qs P
		int slot = dp ? f / 20 : f / 40, g = dp ? f % 20 : f % 40;
		bool qrow = !dp && g >= 20;
		int tip = op_tips[op * 12 + side * 6 + slot];
		if (pair && side == 1 && !(sib_tip && f < 40)) {  // rows of Qs P of the left child's tips
			const int q = (sib_tip ? f - 40 : f) / 20;
			g = f % 20;
			qrow = true;
			tip = -1;
			if (!sib_tip) tip = op_tips[op * 12 + q];
			else
				for (int j = 0, seen = 0; j < 6; j++) {  // the q-th tip slot in use
					const int tj = op_tips[op * 12 + j];
					if (tj >= 0 && seen++ == q) tip = tj;
				}
		}
		const int row = (g % 20) / 4, i = g % 4;
		double v = 0.0;
		if (tip >= 0) {
			const double *M = mats + ((size_t)tip * C + c) * 16;
			double col[4];  // P . e_row, or P . 1
			for (int r = 0; r < 4; r++) col[r] = row < 4 ? M[r * 4 + row] : ((M[r * 4] + M[r * 4 + 1]) + (M[r * 4 + 2] + M[r * 4 + 3]));
			v = !qrow ? col[i] : Qs ? Qs[i * 4] * col[0] + Qs[i * 4 + 1] * col[1] + Qs[i * 4 + 2] * col[2] + Qs[i * 4 + 3] * col[3] : 0.0;  // (no Qs: the post-order pass reads message rows only)
		}
		blk[(side ? OPBLK_RIGHT : OPBLK_LEFT) / 8 + f] = v;
	}
}

typedef const __attribute__((address_space(3))) char *lds_cptr;
typedef __attribute__((address_space(3))) dv2 lds_dv2;

__device__ __forceinline__ d4 lds_read4(lds_cptr p) {
	const lds_dv2 *q = (const lds_dv2 *)p;
	const dv2 lo = q[0], hi = q[1];
	return d4{lo.x, lo.y, hi.x, hi.y};
}

struct SX {
	const char *__restrict__ mats_c;  // this category's matrices: mats + c * 16 doubles
	lds_cptr tb;  // this op's table block in LDS
	// `off` = node * C * 128: the descriptors name a matrix by its byte offset (two scalar adds instead of a multiply, an add, a
	// 64-bit shift and two adds per matrix, five to eight matrices per op -- both walks are bound by instruction issue)
	__device__ __forceinline__ cptr M(int off) const { return opaque(as_const(reinterpret_cast<const double *>(mats_c + (unsigned)off))); }
	// byte offset of the row that nibble J of group w selects (bit 0 of a group is its ambiguity flag: nibble J = bits 1 + 4 J ...)
	template <int J>
	static __device__ __forceinline__ unsigned row(unsigned w) {
		return J == 0 ? (w << 4) & 0xE0u : J == 1 ? w & 0xE0u : (w >> (4 * J - 4)) & 0xE0u;
	}
	// wave-uniform: a word of this op holds a partial ambiguity code (set per op by the AMBIG instantiation, constant false otherwise)
	bool amb = false;
	// the five rows at `rows`, selected by nibble J of w.  Codes 5..14 (a partial ambiguity mask, k_build_mask_stream): the sum of the
	// mask's state rows -- a tip message P . mask and its Qs P . mask are linear in the mask
	// (`rows` = tb + a compile-time offset, tb 2 KB-aligned and the row offset < 256: the row is OR-ed into tb -- shift, v_and_or_b32 --
	// and the constant rides in the read's offset field; as a sum the address took one more vector instruction per tip)
	template <int J>
	__device__ __forceinline__ d4 tip_rows(unsigned rows_off, unsigned w) const {
		const unsigned code = (w >> (4 * J + 1)) & 15u;
		const unsigned tbu = (unsigned)(uintptr_t)tb;
		const lds_cptr rows = (lds_cptr)(uintptr_t)tbu + rows_off;
		d4 v = lds_read4((lds_cptr)(uintptr_t)(tbu | ((amb && code >= 5u) ? 0u : row<J>(w))) + rows_off);  // (row<J> keeps three bits of the nibble: codes 0..4 only)
		if (amb) {
			if (code >= 5u) {
				const unsigned m = (unsigned)(0xEDCBA97653ull >> (4u * (code - 5u))) & 15u;  // AMBIG_MASKS: 3, 5, 6, 7, 9, ..., 14
				v = d4{0., 0., 0., 0.};
#pragma unroll
				for (int st = 0; st < 4; st++)
					if (m >> st & 1u) {
						const d4 r = lds_read4(rows + 32 * st);
						v = d4{v.x + r.x, v.y + r.y, v.z + r.z, v.w + r.w};
					}
			}
		}
		return v;
	}
	// message of a DEEP child's tip: slot SLOT (0..5) of side SIDE, row = nibble SLOT of the side's word
	template <int SIDE, int SLOT>
	__device__ __forceinline__ d4 deep_tip(unsigned w) const {
		return tip_rows<SLOT>((SIDE ? OPBLK_RIGHT : OPBLK_LEFT) + SLOT * OPTIP_BYTES, w);
	}
	// message b = P e_s of the SLOT-th tip (0..2) of a tip / cherry / cherry + tip child
	template <int SIDE, int SLOT>
	__device__ __forceinline__ d4 site_tip(unsigned w) const {
		return tip_rows<SLOT>((SIDE ? OPBLK_RIGHT : OPBLK_LEFT) + SLOT * 2 * OPTIP_BYTES, w);
	}
	// ... and Qs P e_s of the same tip
	template <int SIDE, int SLOT>
	__device__ __forceinline__ d4 site_tip_q(unsigned w) const {
		return tip_rows<SLOT>((SIDE ? OPBLK_RIGHT : OPBLK_LEFT) + SLOT * 2 * OPTIP_BYTES + OPTIP_BYTES, w);
	}
	// pair op (stream_pairs): Qs P e_s of the DEEP left child's tip in slot SLOT (0..5), from the block's other side.  qb = the LDS
	// address of that half's rows (wave-uniform, not 256-aligned: the row is added, not OR-ed -- v_bfe, v_lshl_add)
	template <int SLOT>
	static __device__ __forceinline__ d4 pair_tip_q(unsigned qb, unsigned w) {
		return lds_read4((lds_cptr)(uintptr_t)(qb + (((w >> (4 * SLOT + 1)) & 7u) << 5)) + SLOT * OPTIP_BYTES);
	}
};

// P_half . p_half of one half of a DEEP child (a tip, a cherry or a cherry + tip in slots SB..); h = {node, t0, t1, t2, inner}
template <int SIDE, int SB>
__device__ __forceinline__ d4 s_half(const SX &x, int hk, int mnode, int minner, unsigned w) {
	if (hk == HK_TIP) return x.deep_tip<SIDE, SB>(w);
	d4 p = mul4(x.deep_tip<SIDE, SB>(w), x.deep_tip<SIDE, SB + 1>(w));
	if (hk == HK_CHERRY_TIP) p = mul4(matvec4_opt<false>(x.M(minner), p), x.deep_tip<SIDE, SB + 2>(w));
	return matvec4_opt<false>(x.M(mnode), p);
}

// the ten branch terms of an op -> three accumulators (see the header); sel_r: 1.0 in lanes with (lane & 3) == r
template <bool WEIGHTED>
struct SiteSum {
	double acc0, acc1, acc2;
	double sel0, sel1, sel2, sel3;
	cptr Q;  // diag(pi) Q, or Q when the frequencies are folded into the uppers
	double wq = 1.0;  // WEIGHTED (rescaled evaluations): w_k / D_k of this op (plain ones carry w_k / L_k in the uppers)
	template <int A, int R, bool FIRST>
	__device__ __forceinline__ void put(double num) {
		const double s = R == 0 ? sel0 : R == 1 ? sel1 : R == 2 ? sel2 : sel3;
		double &acc = A == 0 ? acc0 : A == 1 ? acc1 : acc2;
		acc = __builtin_amdgcn_mfma_f64_4x4x4f64(s, WEIGHTED ? wq * num : num, FIRST ? 0.0 : acc, 0, 0, 0);
	}
	// a branch whose lower end is not a tip: u . (Qs b)
	template <int A, int R, bool FIRST = false>
	__device__ __forceinline__ void add(const d4 &u, const d4 &b) {
		put<A, R, FIRST>(dot4(u, matvec4_opt<false>(opaque(Q), b)));
	}
	// a tip's branch: Qs b comes from the table
	template <int A, int R, bool FIRST = false>
	__device__ __forceinline__ void add_tip(const d4 &u, const d4 &qb) {
		put<A, R, FIRST>(dot4(u, qb));
	}
};

// message of a cherry / cherry + tip child of side SIDE; bn = the inner cherry's message (cherry + tip only), which the descent reuses
// KEEP_BN: the inner cherry's message of a cherry + tip child is handed to s_descend in `bn`; else s_descend forms it again (its two
// tip rows are read there anyway, its matrices are that branch's): kept, it crosses the whole op in eight registers per side and the
// join of the paths that do and do not write it costs every op eight v_mov_b64 -- the plain kernel has the registers and is 0.1 ms
// faster with them; the rescaled and ambiguity-code instantiations drop from 131-140 to 121-127 registers without: four waves per
// SIMD instead of three (rescaled evaluation 33.6 -> 31.7 ms)
template <int SIDE, bool KEEP_BN>
__device__ __forceinline__ d4 s_fringe_message(const SX &x, int kind, int node, int inner, unsigned w, d4 &bn) {
	d4 p = mul4(x.site_tip<SIDE, 0>(w), x.site_tip<SIDE, 1>(w));
	if (kind == CH_CHERRY_TIP) {
		const d4 inner_message = matvec4_opt<false>(x.M(inner), p);
		if (KEEP_BN) bn = inner_message;
		p = mul4(inner_message, x.site_tip<SIDE, 2>(w));
	}
	return matvec4_opt<false>(x.M(node), p);
}

// message of a child the post-order walk did not store (SK_CORE_TIP / SK_CORE_CHERRY, stream_elide): t_n = P_n (m_f o t_s), t_s = the
// stored child's array, which the op was handed in place of the node's own, m_f = the tip / cherry child's message from table slots
// 0 and 1 of the side (fm: the cherry's matrices)
template <int SIDE>
__device__ __forceinline__ d4 s_elided_message(const SX &x, int kind, int node, int fm, unsigned w, const d4 &ts) {
	d4 unused;
	const d4 mf = kind == SK_CORE_TIP ? x.site_tip<SIDE, 0>(w) : s_fringe_message<SIDE, false>(x, CH_CHERRY, fm, 0, w, unused);
	return matvec4_opt<false>(x.M(node), mul4(mf, ts));
}

// fringe child (cherry, cherry + tip) of an op: its upper u goes down in registers; SIDE = accumulator of this side (0 left, 1 right),
// rows 1, 2 = the cherry's tips, row 3 = the inner cherry node, accumulator 2 row SIDE = the outer tip.
// FIRST2: this descent makes the first entry of accumulator 2.
template <int SIDE, bool FIRST2, bool KEEP_BN, typename SS>
__device__ __forceinline__ void s_descend(const SX &x, SS &ss, int kind, int node, int inner, const d4 &u, unsigned w, const d4 &bn_kept) {
	d4 a2 = matvec4_opt<false>(x.M(node), u);
	if (kind == CH_CHERRY_TIP) {
		const d4 bn = KEEP_BN ? bn_kept : matvec4_opt<false>(x.M(inner), mul4(x.site_tip<SIDE, 0>(w), x.site_tip<SIDE, 1>(w)));
		const d4 un = mul4(a2, x.site_tip<SIDE, 2>(w));
		ss.template add<SIDE, 3>(un, bn);
		ss.template add_tip<2, SIDE, FIRST2>(mul4(a2, bn), x.site_tip_q<SIDE, 2>(w));
		a2 = matvec4_opt<false>(x.M(inner), un);
	}
	ss.template add_tip<SIDE, 1>(mul4(a2, x.site_tip<SIDE, 1>(w)), x.site_tip_q<SIDE, 0>(w));
	ss.template add_tip<SIDE, 2>(mul4(a2, x.site_tip<SIDE, 0>(w)), x.site_tip_q<SIDE, 1>(w));
}

// pair op (stream_pairs): the descent into half H (a cherry or a cherry + tip in slots 3 H ..) of the DEEP child whose own op runs
// inside its parent's.  s_descend with the child's tips where the parent's block has them: message rows in the left side's DEEP
// slots, Qs P rows behind `qb` on the other side; the inner cherry's message is formed again (the same instructions on the same
// rows as in s_half).  Accumulator H rows 1..3 and accumulator 2 row H, as in the child's own op.
template <int H, typename SS>
__device__ __forceinline__ void s_descend_pair(const SX &x, SS &ss, int hk, int node, int inner, const d4 &u, unsigned w, unsigned qb) {
	d4 a2 = matvec4_opt<false>(x.M(node), u);
	if (hk == HK_CHERRY_TIP) {
		const d4 bn = matvec4_opt<false>(x.M(inner), mul4(x.deep_tip<0, 3 * H>(w), x.deep_tip<0, 3 * H + 1>(w)));
		const d4 un = mul4(a2, x.deep_tip<0, 3 * H + 2>(w));
		ss.template add<H, 3>(un, bn);
		ss.template add_tip<2, H, false>(mul4(a2, bn), SX::pair_tip_q<3 * H + 2>(qb, w));
		a2 = matvec4_opt<false>(x.M(inner), un);
	}
	ss.template add_tip<H, 1>(mul4(a2, x.deep_tip<0, 3 * H + 1>(w)), SX::pair_tip_q<3 * H>(qb, w));
	ss.template add_tip<H, 2>(mul4(a2, x.deep_tip<0, 3 * H>(w)), SX::pair_tip_q<3 * H + 1>(qb, w));
}

__device__ __forceinline__ double dpp_f64(double old, double src, const int ctrl, const int bank) {
	// v_mov_b32_dpp x 2: lanes whose bank (lane & 15) >> 2 is not in `bank` keep `old`
	const int lo = __double2loint(src), hi = __double2hiint(src), olo = __double2loint(old), ohi = __double2hiint(old);
	int rlo, rhi;
	switch (ctrl * 16 + bank) {
#define PHYAMD_DPP_CASE(CT, BK)                                              \
	case (CT) * 16 + (BK):                                                   \
		rlo = __builtin_amdgcn_update_dpp(olo, lo, CT, 0xF, BK, false);      \
		rhi = __builtin_amdgcn_update_dpp(ohi, hi, CT, 0xF, BK, false);      \
		break;
		PHYAMD_DPP_CASE(0x140, 0x3)
		PHYAMD_DPP_CASE(0x140, 0xC)
		PHYAMD_DPP_CASE(0x140, 0xF)
		PHYAMD_DPP_CASE(0x141, 0x5)
		PHYAMD_DPP_CASE(0x141, 0xA)
		PHYAMD_DPP_CASE(0x141, 0xF)
		PHYAMD_DPP_CASE(0xE4, 0xC)
		PHYAMD_DPP_CASE(0xE4, 0xA)
		PHYAMD_DPP_CASE(0x1B, 0xF)
		PHYAMD_DPP_CASE(0xB1, 0xF)
#undef PHYAMD_DPP_CASE
		default: rlo = lo; rhi = hi;
	}
	return __hiloint2double(rhi, rlo);
}

// 16 -> 1 inside every row of 16 lanes.  On return, in row r: lanes 0..3 hold the total of (acc0, row r), lanes 8..11 of
// (acc1, row r), and with THREE accumulators lanes 4..7 and 12..15 that of (acc2, row r) (with two they repeat their neighbours').
template <bool THREE>
__device__ __forceinline__ double fold_sites(double acc0, double acc1, double acc2) {
	// row_mirror (n <-> 15 - n): lanes n < 8 keep acc0, lanes n >= 8 keep acc1
	const double y01 = dpp_f64(dpp_f64(0.0, acc0, 0x140, 0x3), acc1, 0x140, 0xC);
	const double x01 = dpp_f64(acc0, acc1, 0xE4, 0xC);
	const double s01 = x01 + y01;
	double z;
	if (THREE) {
		const double s2 = acc2 + dpp_f64(0.0, acc2, 0x140, 0xF);
		// row_half_mirror (n <-> n ^ 7): lanes with bit 2 clear keep s01, the others s2
		const double y = dpp_f64(dpp_f64(0.0, s01, 0x141, 0x5), s2, 0x141, 0xA);
		const double xk = dpp_f64(s01, s2, 0xE4, 0xA);
		z = xk + y;
	} else
		z = s01 + dpp_f64(0.0, s01, 0x141, 0xF);
	z += dpp_f64(0.0, z, 0x1B, 0xF);  // quad_perm [3,2,1,0]
	z += dpp_f64(0.0, z, 0xB1, 0xF);  // quad_perm [1,0,3,2]
	return z;
}

// Rescaling by powers of two (SCALE == 2, both streamed walks): a vector whose largest entry has fallen below the threshold is
// multiplied by 2^-e, e = that entry's binary exponent, and e joins an integer cumulative exponent.  Exact (no rounding), and a
// CATEGORY'S OWN affair: with integer exponents per (node, pattern, category) a branch term is brought to the units of the site
// likelihood by one ldexp, so the category waves of a pattern block never have to meet -- the reference's scheme (a maximum over
// categories and states, treelikelihood.c:1790-1836: SCALE == 1) costs both walks an LDS exchange behind a barrier per op.
// The stored partials then differ from the reference's by their scale factors: this form lives between the two streamed walks
// only (LowerForm::CarriedExp2); every other reader of stored partials gets the reference's (require_reference_form).
__device__ __forceinline__ int exp2_rescale(d4 &v) {
	const double m = max4(v);
	if (!(m < SCALING_THRESHOLD) || !(m > 0.0)) return 0;
	const int e = ((__double2hiint(m) >> 20) & 0x7FF) - 1023;  // (m is a normal number: far above 2^-1022 by construction)
	v = d4{__builtin_amdgcn_ldexp(v.x, -e), __builtin_amdgcn_ldexp(v.y, -e), __builtin_amdgcn_ldexp(v.z, -e), __builtin_amdgcn_ldexp(v.w, -e)};
	return e;
}

constexpr int STREAM_MIN_WAVES = 4;        // waves per SIMD the kernel is compiled for (<= 128 registers)
constexpr int STREAM_MIN_WAVES_SCALE = 3;  // ... its rescaled / ambiguity-code instantiations (<= 168 registers, so that nothing is spilled)

// one 1 KB piece of a table block: global -> LDS with no register in between (global_load_lds_dwordx4: LDS address = uniform base +
// 16 * lane, source address per lane); completion is counted on vmcnt like any vector load
__device__ __forceinline__ void dma_piece(const char *gsrc, lds_cptr dst) {
	__builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)gsrc, (__attribute__((address_space(3))) void *)dst, 16, 0, 0);
}

// The loop's prefetches as "uniform base in SGPRs + one 32-bit lane offset" loads, written out: left to the compiler each of them
// kept a loop-invariant 64-bit lane address in two registers and added the descriptor's offset to it on the vector ALU, and every
// load it tracks drew a conservative s_waitcnt vmcnt(0) behind the requests (the op waits once, explicitly, at its top).
// The results are consumed only behind that wait -- and must not be MOVED before it either: the compiler takes them for defined
// when the statement ends, so a spill of A / B / U across the loop edge would save registers the load has not written yet.  Every
// instantiation is therefore compiled for an occupancy at which nothing is spilled (STREAM_MIN_WAVES,
// STREAM_MIN_WAVES_SCALE; tests/test_kernel_resources.py pins the spill counts to zero).
typedef double dv4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ d4 prefetch4(const char *base, unsigned lane_off, bool nt) {
	dv2 lo, hi;
	if (nt) asm volatile("global_load_dwordx4 %0, %2, %3 nt\n\tglobal_load_dwordx4 %1, %2, %3 offset:16 nt" : "=&v"(lo), "=&v"(hi) : "v"(lane_off), "s"(base) : "memory");
	else asm volatile("global_load_dwordx4 %0, %2, %3\n\tglobal_load_dwordx4 %1, %2, %3 offset:16" : "=&v"(lo), "=&v"(hi) : "v"(lane_off), "s"(base) : "memory");
	return d4{lo.x, lo.y, hi.x, hi.y};
}
__device__ __forceinline__ unsigned prefetch1(const char *base, unsigned lane_off) {
	unsigned w;
	asm volatile("global_load_dword %0, %1, %2" : "=v"(w) : "v"(lane_off), "s"(base) : "memory");
	return w;
}

// dynamic LDS per wave: STREAM_PARK_SLOTS park slots of [2][64] x 16 bytes, then two table blocks (this op's and the next op's).
// Slot 0 holds leaf parks (nothing else is parked while they wait), slot 1 parks whose wait holds leaf parks only -- an upper parked
// in HBM is written and read back (7.4 GB per evaluation at the headline shape with one slot), and without those stores the pass is
// 1.4 ms shorter (a timing-only ablation, since retired).  8 KB per wave: four workgroups per CU use 128 KB of the 160.
constexpr int STREAM_PARK_BYTES = 2 * WAVE * 16;  // (STREAM_PARK_SLOTS: phyamd_types.h)
constexpr int STREAM_LDS_PER_WAVE = STREAM_PARK_SLOTS * STREAM_PARK_BYTES + 2 * OPBLK_BYTES;

// Workgroup = STREAM_WAVES waves = that many consecutive blocks of 64 patterns of ONE category (blockIdx.x = block group * C + category):
// the waves of a workgroup walk the same ops with the same matrices, descriptors and table blocks, so the scalar cache serves
// three of every four of their scalar loads (one category per wave made every CU juggle four matrix sets: the per-op scalar
// round trips were the largest remaining wait); consecutive workgroups are the categories of one block group and share its mask
// words while they are hot.  No workgroup-level synchronisation anywhere: a wave past the last block leaves at once.
constexpr int STREAM_WAVES = 4;

// Workgroups are dealt to the eight XCDs round-robin (observed, speed only: MI355X_MICROARCH.md, "Workgroup dispatch"), so ids x and
// x + 8 share an L2 and x, x + 1 never do.  The category workgroups of one block group read the same mask words -- with consecutive
// ids every one of them fetched the words from HBM, and those reads are what slows the post-order pass's write stream down
// (profiles/microbench/lower_stream_replay.hip: 8.4 ms without them, 12.5 with) -- so position v of the (group, category) list goes to
// the id whose residue class holds v: ids of class r take positions [r q + min(r, m), ...) with q = n / 8, m = n % 8.
__device__ __forceinline__ unsigned xcd_position(unsigned x, unsigned n, int on) {
	if (!on) return x;
	const unsigned r = x & 7u, q = n >> 3, m = n & 7u;
	return r * q + (r < m ? r : m) + (x >> 3);
}

// SCALE (rescaled evaluations, treelikelihood.c:1790-1836 for lowers and uppers alike): L_k underflows by construction, so a branch
// term is (w_k / D_k) num with D_k = the site likelihood in this op's scaled units, summed over the categories -- and an upper is
// divided by its maximum over categories and states when that falls below the threshold.  Both need the other categories once per
// op: the workgroup is then the C <= 4 category waves of ONE block (blockIdx.x = block), which meet in a double-buffered LDS
// exchange behind one LDS-only barrier per op; everything else is the plain kernel.  w_over_L is unused, weights / props are read.
// AMBIG: the tip data hold partial ambiguity codes (SX::tip_rows); chosen by the launcher from k_build_mask_stream's flag.
// SCALE == 2 (powers of two per category, see exp2_rescale): no exchange, the plain workgroup shape.  Every upper carries an integer
// exponent (registers; beside the LDS park slots; `uexp` for HBM parks), stored children bring theirs (`lexp`, requested with the
// operand), and a branch term num in the op's units is worth num 2^(e_op - Eroot[k]) (w_k / L_k): one ldexp per op.
// "Some value, never mind which": a definition without an instruction, for a variable that only some paths of a loop body write
// and read -- the register allocator then has nothing to preserve around the loop.
__device__ __forceinline__ void any_value(d4 &v) { asm volatile("" : "=v"(v.x), "=v"(v.y), "=v"(v.z), "=v"(v.w)); }
// A copy the register allocator cannot see through: the value gets registers of its own HERE.  (TF: a stored child is its own
// message and lives to the end of the op, while its operand registers A / B are overwritten by the next op's prefetch in the middle
// of it -- left to itself the compiler keeps the message in place and moves BOTH freshly fetched operands at the end of EVERY op:
// eight moves per op instead of four per stored child, measured as +5300 vector instructions per walk of 501 ops.)
__device__ __forceinline__ d4 own_registers(const d4 &v) {
	d4 r;
	asm volatile("v_mov_b64 %0, %1" : "=v"(r.x) : "v"(v.x));
	asm volatile("v_mov_b64 %0, %1" : "=v"(r.y) : "v"(v.y));
	asm volatile("v_mov_b64 %0, %1" : "=v"(r.z) : "v"(v.z));
	asm volatile("v_mov_b64 %0, %1" : "=v"(r.w) : "v"(v.w));
	return r;
}
// TF: the stored children arrive as t = P p (the streamed post-order walk's TF variant stored them so: k_lower4_stream) -- a CORE
// child's message is the stored array itself, sixteen multiply-adds and a matrix fewer per such child.  Its descriptors may name
// children that walk did not store (SK_CORE_TIP / SK_CORE_CHERRY, s_elided_message); a child of such a kind counts as one with
// tips (a mask group of its own, the second piece of the table block) and is a stored child in everything after its message.
template <bool FOLD, int SCALE, bool AMBIG = false, bool TF = false>
__global__ __launch_bounds__(STREAM_WAVES *WAVE, (SCALE || AMBIG) ? STREAM_MIN_WAVES_SCALE : STREAM_MIN_WAVES) void k_upper4_stream(
    const StreamDesc *__restrict__ ops, const StreamChunk *__restrict__ chunks, const int *__restrict__ chunk_off, int chunk_base, int nops, int P, int C, int nb,
    const uint32_t *__restrict__ mstream, size_t mstride, const double *__restrict__ lower, double *__restrict__ upper, const double *__restrict__ mats,
    const char *__restrict__ optab, const double *__restrict__ Q, const double *__restrict__ freqs, const double *__restrict__ w_over_L,
    double *__restrict__ gslab, int R, const double *__restrict__ props, const double *__restrict__ weights, int xcd_map, const int *__restrict__ lexp,
    int *__restrict__ uexp, const int *__restrict__ Eroot) {
	extern __shared__ double sh[];
	constexpr bool KEEP_BN = !SCALE && !AMBIG;  // (s_fringe_message)
	constexpr bool PAIRS = TF && !SCALE && !AMBIG;  // the one instantiation that reads descriptors with pair ops (stream_pairs)
	constexpr bool XCH = SCALE == 1, EXP2 = SCALE == 2;
	const int lane = threadIdx.x, wv = __builtin_amdgcn_readfirstlane(threadIdx.y);
	const unsigned vx = XCH ? blockIdx.x : xcd_position(blockIdx.x, gridDim.x, xcd_map);
	const int c = XCH ? wv : vx % C, blk = XCH ? (int)blockIdx.x : (int)(vx / C) * STREAM_WAVES + wv;
	if (blk >= nb) return;
	const size_t plane = (size_t)P * 4;
	const int k0 = blk * WAVE + lane;
	const bool valid = k0 < P;
	const unsigned k = valid ? k0 : P - 1;
	const unsigned poff = k * 32u;  // byte offset of this thread's pattern in a [P][4] plane
	const unsigned moff = (unsigned)k0 * 4u;  // ... and of its dword in a mask-word row (rows are padded to whole waves)
	const lds_cptr wave_lds = (lds_cptr)sh + (size_t)wv * STREAM_LDS_PER_WAVE;
	const lds_cptr blocks = wave_lds + STREAM_PARK_SLOTS * STREAM_PARK_BYTES;
	SX x{reinterpret_cast<const char *>(mats + (size_t)c * 16), blocks};
	const double wk = XCH ? (valid ? weights[k] : 0.0) : EXP2 ? (valid ? w_over_L[k] : 0.0) : 0.0;  // (SCALE == 2: w_k / L_k in units of 2^Eroot[k])
	const double pc = XCH ? props[c] : 0.0;
	const int eroot = EXP2 ? Eroot[k] : 0;
	// SCALE == 1: exchange buffers behind the waves' own LDS: two sets of [C][64] doubles (w_c den) + [C][64] int2 (maxima of the two uppers)
	// SCALE == 2: the exponents of the uppers parked in LDS, [wave][park slot][64] ints
	double *const xbase = sh + (size_t)blockDim.y * (STREAM_LDS_PER_WAVE / 8);
	const int xsz = blockDim.y * WAVE;
	int *const pexp = reinterpret_cast<int *>(xbase) + ((size_t)wv * STREAM_PARK_SLOTS) * WAVE + lane;
	// exponents of stored lowers / HBM-parked uppers: [array][C][P] ints -- a plane offset of the doubles (32 bytes per pattern) / 8
	const char *const lexp_c = EXP2 ? reinterpret_cast<const char *>(lexp) + (size_t)c * P * 4 : nullptr;
	char *const uexp_c = EXP2 ? reinterpret_cast<char *>(uexp) + (size_t)c * P * 4 : nullptr;
	const unsigned eoff = k * 4u;
	SiteSum<SCALE != 0> ss;
	ss.Q = as_const(Q);
	ss.sel0 = (lane & 3) == 0 ? 1.0 : 0.0;
	ss.sel1 = (lane & 3) == 1 ? 1.0 : 0.0;
	ss.sel2 = (lane & 3) == 2 ? 1.0 : 0.0;
	ss.sel3 = (lane & 3) == 3 ? 1.0 : 0.0;
	// which result this lane stores after fold_sites: row r = lane >> 4; lane n = 0 -> (acc0, r), n = 8 -> (acc1, r), n = 4 -> (acc2, r)
	const int n16 = lane & 15, r4 = lane >> 4;
	const unsigned cid4 = (unsigned)(n16 == 0 ? r4 : n16 == 8 ? 4 + r4 : n16 == 4 ? 8 + r4 : 15) * 4u;
	char *const slab = reinterpret_cast<char *>(gslab + ((size_t)blk * C + c) * R);
	__attribute__((address_space(3))) dv2 *park = (__attribute__((address_space(3))) dv2 *)wave_lds + lane;
	// w_k / L_k is folded into the root's message, so every upper below carries it.  One use per walk, by its first op: it waits in
	// the wave's first park slot, which nothing is parked in before that op, instead of two registers held through the whole walk
	if (!SCALE) park[0].x = valid ? w_over_L[k] : 0.0;
	const int chunk = chunk_base + blockIdx.y;
	const int op_begin = chunk_off[chunk], op_end = chunk_off[chunk + 1];
	const char *const optab_c = optab + (size_t)c * nops * OPBLK_BYTES + lane * 16;  // this category's blocks, this lane's 16 bytes of a piece

	// this category's planes / the mask rows as byte pointers: a descriptor's 64-bit offset is one scalar add away
	const char *const lower_c = reinterpret_cast<const char *>(lower + (size_t)c * plane);
	char *const upper_c = reinterpret_cast<char *>(upper + (size_t)c * plane);
	const char *const mstream_b = reinterpret_cast<const char *>(mstream);
	const size_t mrow = mstride * 4;
	constexpr bool ASM_PREFETCH = true;  // (every instantiation is built spill-free: tests/test_kernel_resources.py)
	auto lower_at = [&](int64_t off) -> d4 {
		return ASM_PREFETCH ? prefetch4(lower_c + off, poff, true) : load4_stream(reinterpret_cast<const double *>(lower_c + off + poff));
	};
	auto upper_at = [&](int64_t off) -> d4 { return ASM_PREFETCH ? prefetch4(upper_c + off, poff, false) : load4(reinterpret_cast<const double *>(upper_c + off + poff)); };
	// (the lane offset is hidden from the compiler here: it would otherwise add it to upper_c once per walk and hold the 64-bit
	// address in two registers for the few ops that store; as "uniform base + 32-bit lane offset" the store needs neither)
	auto store_upper_at = [&](int64_t off, const d4 &v) {
		unsigned po = poff;
		asm volatile("" : "+v"(po));
		store4(reinterpret_cast<double *>(upper_c + off + po), v);
	};
	auto word_at = [&](int64_t off) -> unsigned { return ASM_PREFETCH ? prefetch1(mstream_b + off, moff) : *reinterpret_cast<const unsigned *>(mstream_b + off + moff); };
	// (the prologue takes indices: once per chunk)
	auto fetch_lower = [&](int core) -> d4 { return load4_stream(reinterpret_cast<const double *>(reinterpret_cast<const char *>(lower + ((size_t)core * C + c) * plane) + poff)); };
	auto fetch_upper = [&](int slot) -> d4 { return load4(reinterpret_cast<const double *>(reinterpret_cast<const char *>(upper + ((size_t)slot * C + c) * plane) + poff)); };
	auto fetch_word = [&](int w) -> unsigned { return *reinterpret_cast<const unsigned *>(reinterpret_cast<const char *>(mstream + (size_t)w * mstride) + moff); };
	auto fetch_block = [&](int op_index, int buffer, bool two) {  // table block of an op -> one of the two LDS buffers
		const char *src = optab_c + (size_t)op_index * OPBLK_BYTES;
		const lds_cptr dst = blocks + buffer * OPBLK_BYTES;
		dma_piece(src, dst);
		if (two) dma_piece(src + 1024, dst + 1024);
	};

	// prologue: the first op's operands
	unsigned w0 = 0, w1 = 0;
	d4 A = d4{1., 1., 1., 1.}, B = A, U = A;
	int eA = 0, eB = 0, eU = 0;  // SCALE == 2: the exponents that come with A / B / U
	if (op_begin < op_end) {
		const StreamChunk ch = chunks[chunk];
		fetch_block(op_begin, 0, true);
		if (ch.mask_words > 0) w0 = fetch_word(ch.mask_word);
		if (ch.mask_words > 1) w1 = fetch_word(ch.mask_word + (ch.same_row ? 0 : 1));
		if (ch.a != -1) A = fetch_lower(ch.a);
		if (ch.b != -1) B = fetch_lower(ch.b);
		if (ch.u != -1) U = fetch_upper(ch.u);
		if (EXP2) {
			if (ch.a != -1) eA = *reinterpret_cast<const int *>(lexp_c + (size_t)ch.a * C * P * 4 + eoff);
			if (ch.b != -1) eB = *reinterpret_cast<const int *>(lexp_c + (size_t)ch.b * C * P * 4 + eoff);
			if (ch.u != -1) eU = *reinterpret_cast<const int *>(uexp_c + (size_t)ch.u * C * P * 4 + eoff);
		}
	}
	d4 ul = A;  // the left child's upper of the op in front: what SU_CARRY reads
	int e_ul = 0;  // SCALE == 2: ... and its exponent
	double prev_tot = 0.0;
	int prev_off = -1;
	int buf = 0;  // the LDS buffer that holds this op's table block (they alternate; op indices do not: a pair op steps over its child's)
#pragma unroll 1
	for (int i = op_begin; i < op_end; i++, buf ^= 1) {
		StreamDesc op;  // wave-uniform: scalar loads through the constant address space
		{
			typedef const __attribute__((address_space(4))) int32_t *ciptr;
			const ciptr raw = (ciptr)(ops + i);
			int32_t *dst = reinterpret_cast<int32_t *>(&op);
#pragma unroll
			for (int j = 0; j < 27; j++) dst[j] = raw[j];
		}
		// Everything this op reads from memory was requested one op ago: its words, A / B and its table block (LDS-DMA).  The one
		// vector-memory wait of the op; the compiler does not order LDS reads behind an LDS-DMA by itself.
		asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
		// the previous op's result leaves now, so that it is older than this op's prefetches when the next op waits
		if (prev_off >= 0) *reinterpret_cast<double *>(slab + (unsigned)prev_off) = prev_tot;
		const int fl = op.flags;
		const int kl = fl & 7, kr = (fl >> 3) & 7;
		const int usrc = (fl >> 9) & 7, pk = (fl >> 12) & 3, nxw = (fl >> 14) & 3;
		x.tb = blocks + buf * OPBLK_BYTES;
		// pair op (stream_pairs, phyamd_tree_schedule.h): the DEEP left child's own op runs inside this one, and the next op is the one
		// behind the child's; its twelve slab positions have a table of their own at the block's end
		const bool pair = PAIRS && (fl & (1 << 8));
		const int soff = *(const __attribute__((address_space(3))) int *)(x.tb + (pair ? OPBLK_PAIR_SITES : 0) + cid4);  // this lane's slab position (-1: none)
		// a child with tips has a mask group of its own, the left one's first (w0 / w1 hold the groups' rows: the same row twice when they share it)
		const unsigned g0 = w0 >> (op.wsh & 31), g1 = w1 >> ((op.wsh >> 5) & 31);
		const unsigned wL = g0, wR = (kl != CH_CORE) ? g1 : g0;
		if (AMBIG) x.amb = __any((int)((g0 | (kl != CH_CORE && kr != CH_CORE ? g1 : 0u)) & 1u)) != 0;  // (no group: w0 = 0)
		// a = P_parent . (the parent's upper), straight from wherever that upper waits
		d4 a;
		int ea = 0;  // SCALE == 2: the exponent of the parent's upper
		if (usrc == SU_CARRY) {
			a = matvec4_opt<false>(x.M(op.parent), ul);
			ea = e_ul;
		} else if (usrc == SU_LDS) {
			const int ps = STREAM_PARK_SLOTS > 1 ? ((fl >> 7) & 1) * (STREAM_PARK_BYTES / 16) : 0;
			const dv2 lo = park[ps], hi = park[ps + WAVE];
			a = matvec4_opt<false>(x.M(op.parent), d4{lo.x, lo.y, hi.x, hi.y});
			if (EXP2) ea = pexp[(STREAM_PARK_SLOTS > 1 ? (fl >> 7) & 1 : 0) * WAVE];
		} else if (usrc == SU_U) {
			ea = eU;
			// (lanes past the last pattern were never stored and read a real pattern's upper: their weight w_k / L_k = 0 rides in the
			// uppers here, so the message is cleared for them)
			a = matvec4_opt<false>(x.M(op.parent), U);
			if (!SCALE && !valid) a = d4{0., 0., 0., 0.};
		}
		else {  // the root
			const double wl = SCALE ? 1.0 : (double)park[0].x;
			a = FOLD ? d4{wl * freqs[0], wl * freqs[1], wl * freqs[2], wl * freqs[3]} : d4{wl, wl, wl, wl};
		}
		// the children's messages
		d4 bl, br, bnl, bnr;  // bn*: the inner cherry's message of a cherry + tip child
		// (written and read on the cherry + tip paths only.  Left uninitialised -- or made variables of the whole walk -- the compiler
		// carries "the previous op's value" around the loop through a second register set: sixteen v_mov_b64 per op, measured.  An
		// empty definition per op ends the round trip; eight per op are left, the copies into the merged registers on the other paths
		// -- defined at the merge instead, or as variables of the whole walk, the allocator answers with more copies, not fewer.)
		if (KEEP_BN) {
			any_value(bnl);
			any_value(bnr);
		}
		if (PAIRS && pair) {
			// the left child d is DEEP and its own op, the next of the walk, runs inside this one: its two half messages stay live
			// (in the registers a cherry + tip child's inner message has in other ops); the other child s is stored or a tip
			bnl = s_half<0, 0>(x, (fl >> 16) & 3, op.lm[0], op.lm[1], wL);
			bnr = s_half<0, 3>(x, (fl >> 18) & 3, op.lm[2], op.lm[3], wL);
			bl = matvec4_opt<false>(x.M(op.lnode), mul4(bnl, bnr));
		} else if (kl == CH_CORE) bl = TF ? own_registers(A) : matvec4_opt<false>(x.M(op.lnode), A);
		else if (kl == CH_TIP) bl = x.site_tip<0, 0>(wL);
		else if (kl == CH_DEEP)
			bl = matvec4_opt<false>(x.M(op.lnode), mul4(s_half<0, 0>(x, (fl >> 16) & 3, op.lm[0], op.lm[1], wL), s_half<0, 3>(x, (fl >> 18) & 3, op.lm[2], op.lm[3], wL)));
		else if (TF && kl >= SK_CORE_TIP) bl = s_elided_message<0>(x, kl, op.lnode, op.lm[0], wL, A);  // (A = its stored child's array)
		else bl = s_fringe_message<0, KEEP_BN>(x, kl, op.lnode, op.lm[4], wL, bnl);
		if (kr == CH_CORE) br = TF ? own_registers(B) : matvec4_opt<false>(x.M(op.rnode), B);
		else if (kr == CH_TIP) br = x.site_tip<1, 0>(wR);
		else if (kr == CH_DEEP)
			br = matvec4_opt<false>(x.M(op.rnode), mul4(s_half<1, 0>(x, (fl >> 20) & 3, op.rm[0], op.rm[1], wR), s_half<1, 3>(x, (fl >> 22) & 3, op.rm[2], op.rm[3], wR)));
		else if (TF && kr >= SK_CORE_TIP) br = s_elided_message<1>(x, kr, op.rnode, op.rm[0], wR, B);
		else br = s_fringe_message<1, KEEP_BN>(x, kr, op.rnode, op.rm[4], wR, bnr);
		// (messages rebuilt from tips: no exponent; a child formed from its stored child's array: that array's)
		const int e_bl = EXP2 && (kl == CH_CORE || kl >= SK_CORE_TIP) ? eA : 0, e_br = EXP2 && (kr == CH_CORE || kr >= SK_CORE_TIP) ? eB : 0;
		// the next op's table block, words and stored operands (A, B and U have been consumed; requesting them before the messages of
		// DEEP and fringe children -- a third of an op's arithmetic earlier -- was measured: the longer lives of A / B / U spill)
		unsigned nw0 = 0, nw1 = 0;
		const int nxt = i + 1 + (pair ? 1 : 0);
		__builtin_amdgcn_s_setprio(3);
		if (nxt < op_end) fetch_block(nxt, buf ^ 1, (fl >> 24) & 1);
		if (nxw > 0) nw0 = word_at(op.nx_words);
		if (nxw > 1) nw1 = word_at(op.nx_words + ((fl >> 25) & 1 ? (int64_t)0 : (int64_t)mrow));  // (the same row again: the dword just requested, an L1 hit)
		if (fl & (1 << 26)) A = lower_at(op.nx_a);
		if (fl & (1 << 27)) B = lower_at(op.nx_b);
		if (fl & (1 << 28)) U = upper_at(op.nx_u);
		if (EXP2) {
			// ... and their exponents, by ORDINARY loads: the compiler may copy a loop-carried integer between registers wherever it
			// likes, and for a load written out in assembly it would do so before the data are there (measured: wrong gradients in
			// one block of patterns in eight); tracked loads cost this instantiation a wait at the end of the op instead of the top
			if (fl & (1 << 26)) eA = *reinterpret_cast<const int *>(lexp_c + (op.nx_a >> 3) + eoff);
			if (fl & (1 << 27)) eB = *reinterpret_cast<const int *>(lexp_c + (op.nx_b >> 3) + eoff);
			if (fl & (1 << 28)) eU = *reinterpret_cast<const int *>(uexp_c + (op.nx_u >> 3) + eoff);
		}
		__builtin_amdgcn_s_setprio(0);
		ul = mul4(a, br);
		d4 ur = mul4(a, bl);
		d4 ul_terms = ul, ur_terms = ur;  // SCALE: the branch terms and the fringe descents take the uppers before they are rescaled
		int e_l = 0, e_r = 0;
		if (EXP2) {
			// every branch term of this op is in units of 2^(ea + e_bl + e_br): to those of w_k / L_k with one ldexp
			ss.wq = __builtin_amdgcn_ldexp(wk, ea + e_bl + e_br - eroot);
			e_l = ea + e_br + exp2_rescale(ul);
			e_r = ea + e_bl + exp2_rescale(ur);
		}
		if (XCH) {
			// the mixture likelihood in this op's scaled units from all categories, and the maxima of the two new uppers (as the
			// doubles' high words rounded up: an upper's factor cancels in every branch term, any divisor >= the maximum serves)
			const double den = dot4(FOLD ? a : d4{freqs[0] * a.x, freqs[1] * a.y, freqs[2] * a.z, freqs[3] * a.w}, mul4(bl, br));
			double *xb = xbase + (size_t)(i & 1) * 2 * xsz;
			int2 *xm = reinterpret_cast<int2 *>(xb + xsz);
			xb[wv * WAVE + lane] = pc * den;
			xm[wv * WAVE + lane] = int2{__double2hiint(max4(ul)) + 1, __double2hiint(max4(ur)) + 1};
			lds_barrier();
			double D = 0.0;
			int mlh = 0, mrh = 0;
			for (int cc = 0; cc < C; cc++) {
				D += xb[cc * WAVE + lane];
				const int2 m2 = xm[cc * WAVE + lane];
				mlh = max(mlh, m2.x);
				mrh = max(mrh, m2.y);
			}
			ss.wq = wk / D;  // (D is a product of three factors that rescaling keeps above 1e-40 each: its reciprocal is finite)
			const double ml = __hiloint2double(mlh, 0), mr = __hiloint2double(mrh, 0);
			if (ml < SCALING_THRESHOLD) ul = d4{ul.x / ml, ul.y / ml, ul.z / ml, ul.w / ml};
			if (mr < SCALING_THRESHOLD) ur = d4{ur.x / mr, ur.y / mr, ur.z / mr, ur.w / mr};
		}
		if (pk) {
			const d4 &v = pk == 1 ? ul : ur;
			const int ps = STREAM_PARK_SLOTS > 1 ? ((fl >> 6) & 1) * (STREAM_PARK_BYTES / 16) : 0;
			park[ps] = dv2{v.x, v.y};
			park[ps + WAVE] = dv2{v.z, v.w};
			if (EXP2) pexp[(STREAM_PARK_SLOTS > 1 ? (fl >> 6) & 1 : 0) * WAVE] = pk == 1 ? e_l : e_r;
		}
		if ((fl & (1 << 29)) && valid) store_upper_at(op.st_left, ul);
		if ((fl & (1 << 30)) && valid) store_upper_at(op.st_right, ur);
		if (EXP2) {
			if ((fl & (1 << 29)) && valid) *reinterpret_cast<int *>(uexp_c + (op.st_left >> 3) + eoff) = e_l;
			if ((fl & (1 << 30)) && valid) *reinterpret_cast<int *>(uexp_c + (op.st_right >> 3) + eoff) = e_r;
		}
		// branch terms
		if (kl == CH_TIP) ss.template add_tip<0, 0, true>(ul_terms, x.site_tip_q<0, 0>(wL));
		else ss.template add<0, 0, true>(ul_terms, bl);
		if (kr == CH_TIP) ss.template add_tip<1, 0, true>(ur_terms, x.site_tip_q<1, 0>(wR));
		else ss.template add<1, 0, true>(ur_terms, br);
		if (PAIRS && pair) {
			// d's op on the live halves: a = P_d u_d, its children's messages are the halves.  Every term keeps an accumulator row of
			// its own (this op's two: rows 0 of accumulators 0 and 1, above; d's two: rows 2 and 3 of accumulator 2; d's descents:
			// the rows of its own op).  Its tips' Qs P rows sit on this block's other side, behind s's own rows when s is a tip (d
			// then has four tips: its second half's rows follow its first half's).
			const int hk0 = (fl >> 16) & 3, hk1 = (fl >> 18) & 3;
			const d4 ad = matvec4_opt<false>(x.M(op.lnode), ul);
			const d4 uhl = mul4(ad, bnr), uhr = mul4(ad, bnl);
			const unsigned q0 = (unsigned)(uintptr_t)x.tb + OPBLK_RIGHT + (kr == CH_TIP ? 2 * OPTIP_BYTES : 0);
			const unsigned q1 = (unsigned)(uintptr_t)x.tb + OPBLK_RIGHT + (kr == CH_TIP ? hk0 * OPTIP_BYTES : 0);
			if (hk0 == HK_TIP) ss.template add_tip<2, 2, true>(uhl, SX::pair_tip_q<0>(q0, wL));
			else ss.template add<2, 2, true>(uhl, bnl);
			if (hk1 == HK_TIP) ss.template add_tip<2, 3>(uhr, SX::pair_tip_q<3>(q1, wL));
			else ss.template add<2, 3>(uhr, bnr);
			if (hk0 != HK_TIP) s_descend_pair<0>(x, ss, hk0, op.lm[0], op.lm[1], uhl, wL, q0);
			if (hk1 != HK_TIP) s_descend_pair<1>(x, ss, hk1, op.lm[2], op.lm[3], uhr, wL, q1);
			prev_tot = fold_sites<true>(ss.acc0, ss.acc1, ss.acc2);
			ul = ur;  // s's upper: the carry of the op behind d's when that is s's own
			i++;
		} else if (kl == CH_CHERRY_TIP) {
			s_descend<0, true, KEEP_BN>(x, ss, CH_CHERRY_TIP, op.lnode, op.lm[4], ul_terms, wL, bnl);
			if (kr == CH_CHERRY || kr == CH_CHERRY_TIP) s_descend<1, false, KEEP_BN>(x, ss, kr, op.rnode, op.rm[4], ur_terms, wR, bnr);
			prev_tot = fold_sites<true>(ss.acc0, ss.acc1, ss.acc2);
		} else if (kr == CH_CHERRY_TIP) {
			if (kl == CH_CHERRY) s_descend<0, false, KEEP_BN>(x, ss, CH_CHERRY, op.lnode, op.lm[4], ul_terms, wL, bnl);
			s_descend<1, true, KEEP_BN>(x, ss, CH_CHERRY_TIP, op.rnode, op.rm[4], ur_terms, wR, bnr);
			prev_tot = fold_sites<true>(ss.acc0, ss.acc1, ss.acc2);
		} else {
			if (kl == CH_CHERRY) s_descend<0, false, KEEP_BN>(x, ss, CH_CHERRY, op.lnode, op.lm[4], ul_terms, wL, bnl);
			if (kr == CH_CHERRY) s_descend<1, false, KEEP_BN>(x, ss, CH_CHERRY, op.rnode, op.rm[4], ur_terms, wR, bnr);
			prev_tot = fold_sites<false>(ss.acc0, ss.acc1, 0.0);
		}
		prev_off = soff;
		w0 = nw0;
		w1 = nw1;
		e_ul = e_l;
	}
	if (prev_off >= 0) *reinterpret_cast<double *>(slab + (unsigned)prev_off) = prev_tot;
}

// ---- the post-order walk on the same plumbing (k_lower4_stream) -------------------------------------------------------------
// An op of the post-order pass has the same children as the pre-order op of the same node, so it reads the SAME mask words and
// the SAME table block (the message rows; k_op_tables runs before the pass): a tip's message is an LDS row instead of sixteen
// multiply-adds, and no byte -> arithmetic chain starts at the top of an op.  A post-order op is short (two messages and a
// product), so the requests for op i + 1 leave at the TOP of op i and nothing in the common path is a load the compiler tracks
// (one tracked load and its conservative s_waitcnt vmcnt(0) would land behind the requests and serialise every op):
//   * table block and mask words: LDS-DMA into two-deep rings (the words as one dword per lane);
//   * the wave's parked partials stay in registers: two slots, the first for a wait that holds no other, the second for a wait
//     that holds waits of the first kind only (build_schedule); a deeper nesting goes through memory;
//   * an op's result is stored at the top of the next op, AFTER that op's requests: the wait at the top of an op then leaves
//     the two store instructions in flight (vmcnt(2)) instead of waiting for the write to be acknowledged;
//   * a stored child that is neither the previous op's result nor parked (next to a cut subtree: a handful per walk) is an ordinary
//     load where it is used; that op pays the round trip.
// Workgroup = four consecutive 64-pattern blocks of ONE category (shared descriptors, matrices and table blocks in the scalar
// cache and L2), no workgroup-level synchronisation; the root's sum over categories is k_root_finish64's.
// (LowerDesc, LowerChunk: phyamd_types.h)

constexpr int LSTREAM_MIN_WAVES = 5;  // (29 KB of LDS per workgroup allow five workgroups per CU: 96 registers)
// Park slots of an instantiation: the second one is eight more registers, which the AMBIG instantiations do not have at five
// workgroups per CU (they would spill); those read a second-slot child from memory like the one-slot schedule does -- the
// descriptor keeps its offsets (stream_post_order).
constexpr int lstream_park_slots(bool ambig) { return ambig ? 1 : 2; }
constexpr int LSTREAM_LDS_PER_WAVE = 2 * OPBLK_BYTES + 5 * WAVE * 4 + WAVE * 32;  // two table blocks, a ring of four mask rows + a scratch row, the store staging area

__device__ __forceinline__ void dma_dword(const char *gsrc, lds_cptr dst) {  // one dword per lane -> LDS base + 4 * lane
	__builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)gsrc, (__attribute__((address_space(3))) void *)dst, 4, 0, 0);
}

// AMBIG: the tip data hold partial ambiguity codes (SX::tip_rows), as in k_upper4_stream.
// SCALE (rescaled evaluations, SingleTreeLikelihood_scalePartials, treelikelihood.c:1790-1836): a result whose maximum over categories
// and states falls below the threshold is divided by it, and log(maximum) joins the children's cumulative factors in lscale
// [stored][P].  The maximum needs all categories of a pattern once per op: the workgroup is then the C <= 4 category waves of ONE
// block (blockIdx.x = block) and they meet in a double-buffered LDS exchange behind one LDS-only barrier per op; category 0 keeps
// the factors (one more store per op, counted in its wait).
// TF: what an op hands on -- carries, parks, stores -- is t_n = P_n p_n, the partial already carried through the node's own branch
// (the root: p_root).  The multiply-adds are the same in number (one mat-vec per op instead of one per stored child), but the
// pre-order walk reads a stored child as its message and drops that mat-vec: 16 of ~220 vector instructions per op.  This is a
// form BETWEEN the two streamed walks (LowerForm::Carried): every other reader of stored partials gets p_n back
// (require_reference_form: the pass runs again without TF and stays so).  Never with SCALE == 1, which IS the reference's form.
template <bool AMBIG, int SCALE, bool TF = false>  // SCALE: 0 plain, 1 the reference's rescaling (exchange), 2 powers of two per category (lscale = int exponents [stored][C][P])
__global__ __launch_bounds__(STREAM_WAVES *WAVE, SCALE == 1 ? 4 : LSTREAM_MIN_WAVES) void k_lower4_stream(
    const LowerDesc *__restrict__ ops, const LowerChunk *__restrict__ chunks, const int *__restrict__ chunk_off, int chunk_base, int nblocks, int P, int C, int nb,
    const uint32_t *__restrict__ mstream, size_t mstride, double *__restrict__ lower, const double *__restrict__ mats, const char *__restrict__ optab,
    const double *__restrict__ freqs, const double *__restrict__ props, double *__restrict__ Lc, int with_root, double *__restrict__ lscale, int xcd_map,
    int *__restrict__ Ec) {
	extern __shared__ double sh[];
	constexpr bool XCH = SCALE == 1, EXP2 = SCALE == 2, PARK2 = lstream_park_slots(AMBIG) > 1;
	const int lane = threadIdx.x, wv = __builtin_amdgcn_readfirstlane(threadIdx.y);
	const unsigned vx = XCH ? blockIdx.x : xcd_position(blockIdx.x, gridDim.x, xcd_map);
	const int c = XCH ? wv : vx % C, blk = XCH ? (int)blockIdx.x : (int)(vx / C) * STREAM_WAVES + wv;
	if (blk >= nb) return;
	const size_t plane = (size_t)P * 4;
	const int k0 = blk * WAVE + lane;
	const bool valid = k0 < P;
	const unsigned k = valid ? k0 : P - 1;
	const unsigned poff = k * 32u, moff = (unsigned)k0 * 4u;
	const lds_cptr blocks = (lds_cptr)sh + (size_t)wv * LSTREAM_LDS_PER_WAVE;
	const lds_cptr wrows = blocks + 2 * OPBLK_BYTES;  // [ring slot 0..3 | scratch][lane]
	SX x{reinterpret_cast<const char *>(mats + (size_t)c * 16), blocks};
	const int chunk = chunk_base + blockIdx.y;
	const int op_begin = chunk_off[chunk], op_end = chunk_off[chunk + 1];
	const char *const optab_c = optab + (size_t)c * nblocks * OPBLK_BYTES + lane * 16;
	char *const lower_c = reinterpret_cast<char *>(lower + (size_t)c * plane);
	const char *const mstream_b = reinterpret_cast<const char *>(mstream) + moff;
	const size_t mrow = mstride * 4;
	// `count` new mask rows from byte offset `off` into ring slots slot, slot + 1.  Always two instructions (the wait at the top counts
	// them); one that has no row to fetch reads a line every wave of the category keeps hot (the head of the table) into the scratch
	// row.  A row is requested ONCE per wave: every byte the pass reads costs its write stream time (see "Mask words").
	const char *const hot = optab + (size_t)c * nblocks * OPBLK_BYTES + lane * 4;
	auto request_words = [&](int64_t off, int count, int slot) {
		dma_dword(count > 0 ? mstream_b + off : hot, wrows + (count > 0 ? slot : 4) * (WAVE * 4));
		dma_dword(count > 1 ? mstream_b + off + mrow : hot, wrows + (count > 1 ? ((slot + 1) & 3) : 4) * (WAVE * 4));
	};
	// (two instructions always, as for the words; a piece whose child has no tips is not fetched: its instruction reads the hot line
	// into the scratch row -- a quarter of the bytes through the vector memory path, which the result stores need)
	auto request_block = [&](int parity, int block, int pieces) {
		const char *src = optab_c + (size_t)block * OPBLK_BYTES;
		const lds_cptr dst = blocks + parity * OPBLK_BYTES;
		if (pieces & 1) dma_piece(src, dst);
		else dma_dword(hot, wrows + 4 * (WAVE * 4));
		if (pieces & 2) dma_piece(src + 1024, dst + 1024);
		else dma_dword(hot, wrows + 4 * (WAVE * 4));
	};
	if (op_begin < op_end) {
		const LowerChunk ch = chunks[chunk];
		request_block(op_begin & 1, ch.block, ch.pieces);
		request_words(ch.words, ch.mask_rows, ch.slot);
	}
	// A result leaves as two instructions of 1 KB each that cover whole cache lines (lane l: bytes 16 l and 1024 + 16 l of the wave's
	// 2 KB), not as two interleaved halves per lane: the pass is bound by its 50 GB of writes, and a store instruction that fills
	// every other 16 bytes of sixteen lines leaves the memory system to merge the halves.  The transposition goes through LDS.
	const lds_cptr stage = wrows + 5 * WAVE * 4;
	const bool valid_lo = blk * WAVE + (lane >> 1) < P, valid_hi = blk * WAVE + 32 + (lane >> 1) < P, full_block = (blk + 1) * WAVE <= P;
	auto store_result = [&](int64_t off, const d4 &v) {
		__attribute__((address_space(3))) dv2 *w = (__attribute__((address_space(3))) dv2 *)(stage + lane * 32);
		w[0] = dv2{v.x, v.y};
		w[1] = dv2{v.z, v.w};
		const dv2 lo = *(const __attribute__((address_space(3))) dv2 *)(stage + lane * 16), hi = *(const __attribute__((address_space(3))) dv2 *)(stage + 1024 + lane * 16);
		char *dst = lower_c + off + (size_t)blk * (WAVE * 32) + lane * 16;
		if (valid_lo) __builtin_nontemporal_store(lo, reinterpret_cast<dv2 *>(dst));
		if (valid_hi) __builtin_nontemporal_store(hi, reinterpret_cast<dv2 *>(dst + 1024));
	};
	d4 carry = d4{1., 1., 1., 1.}, parked = carry, parked2 = carry;
	double sfc = 0.0, sfp = 0.0, sfp2 = 0.0;  // SCALE == 1: cumulative log factors of the carried / parked partials
	int efc = 0, efp = 0, efp2 = 0;           // SCALE == 2: ... cumulative binary exponents
	double *const xbase = sh + (size_t)blockDim.y * (LSTREAM_LDS_PER_WAVE / 8);  // SCALE == 1: [2][C][64] maxima
	char *const lscale_k = XCH ? reinterpret_cast<char *>(lscale) + (size_t)k * 8 : nullptr;
	// SCALE == 2: this category's exponents; a descriptor's ls_* (byte offset of [stored][P] doubles) x C / 2 = that of [stored][C][P] ints
	char *const lexp_k = EXP2 ? reinterpret_cast<char *>(lscale) + ((size_t)c * P + k) * 4 : nullptr;
	auto exp_at = [&](int64_t ls_off) -> int * { return reinterpret_cast<int *>(lexp_k + (ls_off >> 1) * C); };
	int64_t prev_store = 0, prev_ls = 0;
	bool have_prev = false, stored = false;  // stored: the youngest two vector-memory instructions are the previous op's result store
#pragma unroll 1
	for (int i = op_begin; i < op_end; i++) {
		LowerDesc op;
		{
			typedef const __attribute__((address_space(4))) int32_t *ciptr;
			const ciptr raw = (ciptr)(ops + i);
			int32_t *dst = reinterpret_cast<int32_t *>(&op);
#pragma unroll
			for (int j = 0; j < (SCALE ? 30 : TF ? 24 : 23); j++) dst[j] = raw[j];  // (TF: + self; SCALE: + ls_store, ls_l, ls_r)
		}
		// words and table block of this op were requested at the top of the op in front (or by the prologue), before that op's
		// result store: everything but those two store instructions has to be back
		if (!stored) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
		else if (EXP2 || (XCH && c == 0)) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");  // (+ the factor's store)
		else asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
		const int fl = op.flags;
		const int kl = fl & 7, kr = (fl >> 3) & 7, nxw = (fl >> 14) & 3;
		const int sl = !PARK2 && ((fl >> 6) & 3) == 3 ? 0 : (fl >> 6) & 3, sr = !PARK2 && ((fl >> 8) & 3) == 3 ? 0 : (fl >> 8) & 3;
		x.tb = blocks + (i & 1) * OPBLK_BYTES;
		// this op's mask groups, from the ring slots of their rows
		const unsigned w0 = *(const __attribute__((address_space(3))) unsigned *)(wrows + ((op.wsh >> 10) & 3) * (WAVE * 4) + lane * 4) >> (op.wsh & 31);
		const unsigned w1 = *(const __attribute__((address_space(3))) unsigned *)(wrows + ((op.wsh >> 12) & 3) * (WAVE * 4) + lane * 4) >> ((op.wsh >> 5) & 31);
		if (AMBIG) x.amb = __any((int)(((kl != CH_CORE || kr != CH_CORE ? w0 : 0u) | (kl != CH_CORE && kr != CH_CORE ? w1 : 0u)) & 1u)) != 0;
		// the next op's requests, then this wave's previous result
		if (i + 1 < op_end) {
			request_block((i + 1) & 1, op.nx_block, ((fl >> 25) & 1) | ((fl >> 23) & 2));
			request_words(op.nx_words, nxw, (fl >> 12) & 3);
		}
		stored = have_prev && full_block;  // (a ragged last block may skip the second instruction: it waits for everything)
		if (have_prev) store_result(prev_store, carry);  // (every wave has a valid lane 0: two instructions)
		if (XCH && have_prev && c == 0 && valid) *reinterpret_cast<double *>(lscale_k + prev_ls) = sfc;
		if (EXP2 && have_prev && valid) __builtin_nontemporal_store(efc, exp_at(prev_ls));  // (every wave has a valid lane: one instruction, always)
		const unsigned wL = w0, wR = (kl != CH_CORE) ? w1 : w0;
		d4 bl, br, bn;
		any_value(bn);  // (see k_upper4_stream)
		double sf_in = 0.0;  // SCALE == 1: the stored children's cumulative factors
		int ef_in = 0;       // SCALE == 2
		if (kl == CH_CORE) {
			d4 src = sl == 1 ? carry : sl == 3 ? parked2 : parked;
			if (sl == 0) {  // from memory (next to a cut subtree): this op pays the round trip
				src = load4(reinterpret_cast<const double *>(lower_c + op.mem_l + poff));
				if (XCH) sf_in += *reinterpret_cast<const double *>(lscale_k + op.ls_l);
				if (EXP2) ef_in += *exp_at(op.ls_l);
				stored = false;
			} else if (XCH) sf_in += sl == 1 ? sfc : sl == 3 ? sfp2 : sfp;
			else if (EXP2) ef_in += sl == 1 ? efc : sl == 3 ? efp2 : efp;
			bl = TF ? src : matvec4_opt<false>(x.M(op.lnode), src);
		} else if (kl == CH_TIP) bl = x.site_tip<0, 0>(wL);
		else if (kl == CH_DEEP)
			bl = matvec4_opt<false>(x.M(op.lnode), mul4(s_half<0, 0>(x, (fl >> 16) & 3, op.lm[0], op.lm[1], wL), s_half<0, 3>(x, (fl >> 18) & 3, op.lm[2], op.lm[3], wL)));
		else bl = s_fringe_message<0, false>(x, kl, op.lnode, op.lm[4], wL, bn);
		if (kr == CH_CORE) {
			d4 src = sr == 1 ? carry : sr == 3 ? parked2 : parked;
			if (sr == 0) {
				src = load4(reinterpret_cast<const double *>(lower_c + op.mem_r + poff));
				if (XCH) sf_in += *reinterpret_cast<const double *>(lscale_k + op.ls_r);
				if (EXP2) ef_in += *exp_at(op.ls_r);
				stored = false;
			} else if (XCH) sf_in += sr == 1 ? sfc : sr == 3 ? sfp2 : sfp;
			else if (EXP2) ef_in += sr == 1 ? efc : sr == 3 ? efp2 : efp;
			br = TF ? src : matvec4_opt<false>(x.M(op.rnode), src);
		} else if (kr == CH_TIP) br = x.site_tip<1, 0>(wR);
		else if (kr == CH_DEEP)
			br = matvec4_opt<false>(x.M(op.rnode), mul4(s_half<1, 0>(x, (fl >> 20) & 3, op.rm[0], op.rm[1], wR), s_half<1, 3>(x, (fl >> 22) & 3, op.rm[2], op.rm[3], wR)));
		else br = s_fringe_message<1, false>(x, kr, op.rnode, op.rm[4], wR, bn);
		carry = mul4(bl, br);
		if (EXP2) efc = ef_in + exp2_rescale(carry);
		if (XCH) {
			double *xb = xbase + (size_t)(i & 1) * blockDim.y * WAVE;
			xb[c * WAVE + lane] = max4(carry);
			lds_barrier();
			double m = 0.0;
			for (int cc = 0; cc < C; cc++) m = fmax(m, xb[cc * WAVE + lane]);
			sfc = sf_in;
			if (m < SCALING_THRESHOLD) {
				carry = d4{carry.x / m, carry.y / m, carry.z / m, carry.w / m};
				sfc += log(m);
			}
		}
		if (TF && op.self) carry = matvec4_opt<false>(x.M(op.self), carry);  // t_n (an exponent or factor of p_n is t_n's too)
		if (fl & (1 << 10)) {
			parked = carry;
			sfp = sfc;
			efp = efc;
		}
		if (PARK2 && (fl & (1 << 26))) {
			parked2 = carry;
			sfp2 = sfc;
			efp2 = efc;
		}
		// (bit 11, stream_elide: the pre-order walk forms this node from its stored child; only the forms that walk reads -- any other
		// reader's pass, the rerun of require_reference_form, stores every node from the same descriptors.  The op that follows
		// an unstored one issues no stores, so the op after it waits for everything: `stored` above)
		have_prev = !(TF && (fl & (1 << 11)));
		prev_store = op.store;
		prev_ls = op.ls_store;
	}
	if (have_prev) store_result(prev_store, carry);
	if (XCH && have_prev && c == 0 && valid) *reinterpret_cast<double *>(lscale_k + prev_ls) = sfc;
	if (EXP2 && have_prev && valid) *exp_at(prev_ls) = efc;
	// the last op of the top part is the root: this category's share of the site likelihood (integrate_partials, treelikelihood.c:1473-1487)
	if (with_root && valid) {
		Lc[(size_t)c * P + k] = props[c] * (freqs[0] * carry.x + freqs[1] * carry.y + freqs[2] * carry.z + freqs[3] * carry.w);
		if (EXP2) Ec[(size_t)c * P + k] = efc;  // ... in units of 2^efc
	}
}

// node_log_likelihoods + the weighted sum: L_k = sum_c Lc[c][k], lnL_k, w_k / L_k, and one partial sum of w_k lnL_k per block of
// 64 patterns (reduce_block_sums)
// Ec / Eroot (power-of-two rescaling): category c's share is in units of 2^Ec[c][k]; the sum is formed in units of the largest of
// them, 2^Eroot[k], which the pre-order walk brings its branch terms to.
__global__ __launch_bounds__(64) void k_root_finish64(int P, int C, const double *__restrict__ Lc, const double *__restrict__ weights, double *__restrict__ pattern_lk,
                                                     double *__restrict__ w_over_L, double *__restrict__ lnl_part, const double *__restrict__ lscale_root,
                                                     const int *__restrict__ Ec, int *__restrict__ Eroot) {
	const int k = blockIdx.x * 64 + threadIdx.x;
	double term = 0.0;
	if (k < P) {
		double L = 0.0, ls = lscale_root ? lscale_root[k] : 0.0;  // (the reference's rescaling: + the root's cumulative log factor)
		if (Ec) {
			int E = Ec[k];
			for (int c = 1; c < C; c++) E = max(E, Ec[(size_t)c * P + k]);
			for (int c = 0; c < C; c++) L += ldexp(Lc[(size_t)c * P + k], Ec[(size_t)c * P + k] - E);
			Eroot[k] = E;
			ls = (double)E * 0.69314718055994530942;
		} else
			for (int c = 0; c < C; c++) L += Lc[(size_t)c * P + k];
		const double lk = log(L) + ls, w = weights[k];
		pattern_lk[k] = lk;
		w_over_L[k] = w / L;
		term = lk * w;
	}
	const double s = wave_sum(term);
	if (threadIdx.x == 0) lnl_part[blockIdx.x] = s;
}

// Sums over pattern blocks whose value depends on the pattern range alone -- not on how many GPUs share it.
// The block range [0, nb) of an engine is bisected `levels` times (mid = lo + (hi - lo) / 2), each of the 2^levels segments is
// summed in block order (eight interleaved lanes, then pairwise), and the segment sums are added pairwise up the bisection tree.
// An engine that holds one half, quarter or eighth of a larger range (a shard cut by the same bisection) runs with one, two or
// three levels fewer, and the host adds the shards pairwise: every addition is the same in every split.
// slab: [nb][C][R] -> seg: [segments][C][R]
__global__ __launch_bounds__(256) void k_slab_segments(const double *__restrict__ slab, int C, int R, const int *__restrict__ seg_lo, double *__restrict__ seg) {
	__shared__ double red[8][33];
	const int q = blockIdx.x * 32 + (threadIdx.x & 31), bl = threadIdx.x >> 5, c = blockIdx.y, o = blockIdx.z;
	const int lo = seg_lo[o], hi = seg_lo[o + 1];
	double s = 0.0;
	if (q < R)
		for (int b = lo + bl; b < hi; b += 8) s += slab[((size_t)b * C + c) * R + q];
	red[bl][threadIdx.x & 31] = s;
	__syncthreads();
	if (bl == 0 && q < R) {
		const int t = threadIdx.x & 31;
		seg[((size_t)o * C + c) * R + q] = ((red[0][t] + red[1][t]) + (red[2][t] + red[3][t])) + ((red[4][t] + red[5][t]) + (red[6][t] + red[7][t]));
	}
}
// the segment sums pairwise up the tree, written to out[(row_of[q] or q) * C + c]
__global__ void k_slab_finish(const double *__restrict__ seg, int segments, int C, int R, const int *__restrict__ row_of, double *__restrict__ out) {
	const int idx = blockIdx.x * blockDim.x + threadIdx.x;
	if (idx >= C * R) return;
	const int c = idx / R, q = idx % R;
	const size_t st = (size_t)C * R;
	double v[8];
	for (int o = 0; o < segments; o++) v[o] = seg[(size_t)o * st + (size_t)c * R + q];
	for (int n = segments; n > 1; n >>= 1)
		for (int o = 0; o < n / 2; o++) v[o] = v[2 * o] + v[2 * o + 1];
	out[(size_t)(row_of ? row_of[q] : q) * C + c] = v[0];
}
