// phyamd_types.h -- the plain data the host builds and the kernels read: op lists, descriptors, their enums and the few constants
// both sides share.  Standard C++17: no HIP include, no device code, so a host compiler reads it (tests/cpp/schedule_sanitize.cpp).
// phyamd_engine.hip includes it inside its anonymous namespace like the .inc files, after the standard headers below.
#ifndef PHYAMD_TYPES_H
#define PHYAMD_TYPES_H

#include <cstddef>
#include <cstdint>

constexpr int WAVE = 64;             // lanes per wavefront (gfx950)

// how a child's lower partial is obtained: read (CORE), or recomputed in registers from tips (CHERRY, CHERRY_TIP: "fringe",
// which also has its inner branch gradients computed inside its parent's pre-order op) or from two fringe / tip children
// (DEEP: no stored lower either, but a pre-order op of its own)
enum { CH_TIP = 0, CH_CORE = 1, CH_DEEP = 2, CH_CHERRY = 3, CH_CHERRY_TIP = 4 };

// children of a DEEP node, by node id: what child_message needs to rebuild its partial
struct DeepDesc {
	int32_t kind_left, left, lt0, lt1, lt2, linner;
	int32_t kind_right, right, rt0, rt1, rt2, rinner;
};

struct NodeOp {
	int32_t parent;  // lower pass: destination node; upper pass: the node whose children are produced
	int32_t left, right;
	int32_t upper_slot_parent;  // upper pass: slot of the parent's upper (-1: parent is the root)
	int32_t upper_slot_left, upper_slot_right;  // slots to write (-1: nothing stored)
	int32_t core_parent, core_left, core_right;  // index of the stored lower array (-1: tip or fused fringe node)
	int32_t kind_left, kind_right;               // CH_*
	int32_t lt0, lt1, lt2, linner;               // left fringe: cherry tips, outer tip, inner cherry node
	int32_t rt0, rt1, rt2, rinner;               // right fringe
	// tree-walk kernels only (ops in depth-first order, values handed from one op to the next in registers):
	int32_t carry_in;   // lower walk: 1 / 2 = the left / right child's partial is the previous op's result;
	                    // upper walk: 1 = the parent's upper is the previous op's carried child upper
	int32_t carry_out;  // upper walk: 1 / 2 = the left / right child's upper goes to the next op in registers (not stored)
	// upper walk, plain kernel: a parked upper whose waiting time holds no other park ("leaf park": two thirds of them in a random
	// tree) can wait in the wave's LDS slot instead of HBM.  bit 0: the parent's upper is read from LDS; bit 1 / 2: the left /
	// right child's upper is parked in LDS.  The HBM slot stays assigned (the rescaling and parameter variants use it).
	// (bit 3 is no longer set by the host; k_lower4_walk still tests it)
	// lower walk: bit 0 / 1: the left / right child comes from the wave's park slot, bit 2: the result is kept there; the streamed
	// walk's second slot: bit 4 / 5 and bit 6 (walk_post_order, phyamd_tree_schedule.h)
	int32_t lds_park;
};

// the chunked walk lists cut the op list into a top part and subtrees of at most 1 / WALK_CHUNKS of the ops (chunk_pre_order)
constexpr int WALK_CHUNKS = 3;  // (3 measured best once a re-read beside a cut subtree cost the post-order pass its write rate)

// ---- the batched walks (phyamd_batch4.inc, phyamd_nni4.inc, phyamd_spr4.inc, phyamd_sitelnl.inc) -------------------------------
// post-order: node = (P_left p_left) o (P_right p_right); carry 1 / 2: the left / right child's partial is the previous op's result
// pre-order: the op of `node` forms its children's uppers.  src: where u_node is (BATCH_ROOT: node is the root; BATCH_CARRY: the
// previous op handed it on in registers; >= 0: upper slot); dst_left / dst_right: where a child's upper goes (BATCH_NONE: a tip's
// is not kept)
struct BatchOp {
	int32_t node, left, right;
	int32_t carry;
	int32_t src, dst_left, dst_right;
	int32_t pad;
};
enum { BATCH_NONE = -1, BATCH_CARRY = -2, BATCH_ROOT = -3, BATCH_GHOST = -4 };  // BATCH_GHOST: a pruned child (phyamd_spr4.inc), whose message is all ones

// ---- the streamed 4-state walks (phyamd_walk4s.inc) ----------------------------------------------------------------------------
enum { HK_TIP = 0, HK_CHERRY = 1, HK_CHERRY_TIP = 2 };
enum { SU_CARRY = 0, SU_LDS = 1, SU_U = 2, SU_ROOT = 3 };
// kinds of a child that only the streamed pre-order walk's descriptors know (stream_elide, phyamd_tree_schedule.h): a stored node
// that the post-order walk did not store, formed from its stored child (whose plane the op is handed) and its tip / cherry child
enum { SK_CORE_TIP = 5, SK_CORE_CHERRY = 6 };

// side: node, then a[10]: CH_CHERRY / CH_CHERRY_TIP: {t0, t1, t2, inner}; CH_DEEP: two halves {node, t0, t1, t2, inner}
struct StreamOp {
	int32_t flags;        // kl 0-2 | kr 3-5 | 6: LDS slot of the park | 7: LDS slot the parent's upper is read from | upper source 9-11 |
	                      // park 12-13 (1: left child's upper -> LDS, 2: right) | mask groups of the
	                      // NEXT op 14-15 | half kinds: left h0 16-17, h1 18-19, right h0 20-21, h1 22-23 | 24: the next op's block is two pieces |
	                      // 25: the next op's second group sits in its first group's row
	                      // 8 (descriptors only, stream_pairs): a pair op -- the left child is DEEP and its own op, the next in the list, runs inside this one
	int32_t parent;       // node whose matrix multiplies the incoming upper (this and every other matrix: byte offset node * C * 128, see SX::M)
	int32_t slot_parent, slot_left, slot_right;  // HBM upper slots (-1: none)
	int32_t nx_mask_word;  // row of the next op's first mask group (-1: none)
	int32_t nx_a, nx_b;   // stored lower arrays the next op wants in register sets A (its left child) / B (right): -1 nothing
	int32_t lnode, la[10];
	int32_t rnode, ra[10];
	int32_t nx_u;         // HBM upper slot the next op wants in register set U (its parent's upper): -1 nothing
	int32_t wsh;          // this op's mask groups: shift of the first 0-4 | of the second 5-9 (inside their rows)
};
static_assert(sizeof(StreamOp) == 128, "one StreamOp = 32 dwords");

// What the kernel reads (build_stream_tables converts the StreamOp rows, which keep node ids for the host's bookkeeping): every
// address an op needs is a byte offset the host has multiplied out -- both walks are bound by instruction issue, and 64-bit
// scalar multiplies for (array index x plane size) were a third of the scalar instructions of an op.
struct StreamDesc {
	int32_t flags;               // StreamOp::flags | 26 / 27 / 28: the next op wants register set A / B / U | 29 / 30: the left / right child's upper is stored
	int32_t parent, lnode, rnode;  // matrices (SX::M): byte offset node * C * 128
	int32_t lm[5], rm[5];        // matrices inside a child: DEEP halves {node, inner} x 2, then a fringe child's inner cherry
	int64_t nx_words;            // byte offset of the row of the next op's first mask group
	int64_t nx_a, nx_b, nx_u;    // byte offsets of the planes the next op wants (category 0; a wave adds its category's)
	int64_t st_left, st_right;   // ... of the upper slots this op stores
	int32_t wsh;                 // StreamOp::wsh
	int32_t pad[5];
};
static_assert(sizeof(StreamDesc) == 128 && offsetof(StreamDesc, nx_words) == 56, "one StreamDesc = 32 dwords");

struct StreamChunk {  // what the first op of a chunk wants fetched before the loop (same_row: its second group sits in the first one's row)
	int32_t mask_word, mask_words, a, b, u, same_row, pad[2];
};

// Per-(op, category) table block, 2048 bytes:
//   [0, 64)       16 ints: byte offset in a slab row of the branch each result lane stores (-1: none), see k_upper4_stream
//   [64, 1024)    the left child's tips, [1024, 1984) the right child's:
//                 a DEEP child: six slots of 160 bytes = 5 rows x 4 doubles, P_tip . e_s for s = 0..3, then P_tip . 1;
//                 any other child (its tips' branch terms are formed in this op): three slots of 320 bytes = those 5 rows, then the
//                 5 rows of Qs P_tip . e_s / Qs P_tip . 1, Qs = the matrix of the branch terms (diag(pi) Q, or Q under FOLD)
// A pair op's block (stream_pairs, phyamd_tree_schedule.h: the DEEP left child's own op runs inside its parent's) is the block above
// with more in it, so that every kernel that does not know pairs reads it as before:
//   [1024, 1984)  the sibling stored: six slots of 160 bytes, the rows Qs P_tip . e_s / Qs P_tip . 1 of the DEEP child's tip slots;
//                 the sibling a tip: its 320 bytes as above, then those rows of the DEEP child's four tips, packed in slot order
//   [1984, 2048)  16 ints: the slab positions of the pair's twelve terms by result lane (the parent's two at 0 and 4, the child's
//                 descents at 1-3, 5-7, 8, 9 as in its own op, the child's two children at 10 and 11)
constexpr int OPBLK_BYTES = 2048, OPBLK_LEFT = 64, OPBLK_RIGHT = 1024, OPTIP_BYTES = 160, OPBLK_PAIR_SITES = 1984;

// LDS park slots per wave of the streamed pre-order walk (their use and their cost: phyamd_walk4s.inc, "dynamic LDS per wave")
constexpr int STREAM_PARK_SLOTS = 2;

// one op of the streamed post-order walk (k_lower4_stream; the plumbing: phyamd_walk4s.inc, "the post-order walk on the same plumbing")
struct LowerDesc {
	int32_t flags;     // kl 0-2 | kr 3-5 | where a stored left child comes from 6-7 (0: memory, 1: the previous op's result, 2: the parked
	                   // partial, 3: the one in the second slot) | same for the right child 8-9 | 10: park the result | 11: no store
	                   // (stream_elide; the TF instantiations) | 12-13: ring slot of the first mask row to request for the NEXT op | 14-15: how many rows to request
	                   // for it (0..2: the rows it reads that no op before it has read) | half kinds 16-23 | 24 / 25: the next op's block
	                   // needs its second / first piece | 26: park the result in the second slot
	int32_t nx_block;  // table block of the next op
	int32_t lnode, rnode, lm[5], rm[5];  // matrices by byte offset, as in StreamDesc
	int64_t nx_words;  // byte offset of the first mask row to request for the next op (the post-order walk's own stream)
	int64_t store;     // ... of the plane (category 0) that receives the result
	int64_t mem_l, mem_r;  // ... of a child that comes from memory
	int32_t wsh;       // this op's mask groups: shift of the first 0-4 | of the second 5-9 | ring slots of their rows 10-11 | 12-13
	int32_t self;      // TF: the node's own matrices by byte offset (0: the root, which has no branch)
	int64_t ls_store, ls_l, ls_r;  // rescaled evaluations: the same three as byte offsets into the cumulative log scale factors [stored][P]
	int32_t pad[2];
};
static_assert(sizeof(LowerDesc) == 128 && offsetof(LowerDesc, nx_words) == 56, "one LowerDesc = 32 dwords");
struct LowerChunk {  // what the first op of a chunk wants requested before the loop: table block, mask rows (count, ring slot and byte offset of the first)
	int32_t block, pieces, mask_rows, slot;
	int64_t words;
};

#endif
