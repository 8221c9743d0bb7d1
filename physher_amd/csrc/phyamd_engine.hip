// phyamd_engine.hip -- MI355X (gfx950) tree-likelihood engine behind include/physher_amd.h.
//
// One translation unit, assembled from:
//   phyamd_types.h          plain data the host builds and the kernels read: op lists, descriptors, their enums and constants
//   phyamd_tree_schedule.h  the tree check and every host-built list as a value built by a pure function (standard C++, no engine)
//   phyamd_memory.inc       owning device arrays and the memory budget they are allocated through
//   phyamd_device.inc / _level4 / _walk4 / _walk4s / _general / _genwalk / _patterns / _batch4 / _nni4 / _nniopt4 / _blopt4 / _spr4 / _tripod4 / _post / _bhess / _reweight / _pairdist4 / _pairdist_gen / _place4 / _place_gen / _nni_gen / _spr_gen / _qopt4 / _qopt_gen / _nniopt_gen  device code (kernels; _rule: the branch-length rule they share)
//   phyamd_shard.inc        state of one engine on one GPU (= one shard of the site patterns), the form of its stored lowers
//   phyamd_schedule.inc     the engine's schedule on the device: storage, upload, readiness
//   phyamd_launch.inc       kernel launches per pass
//   phyamd_eval.inc         one evaluation (incremental updates, lazy rescaling, gradients, pattern tiling)
//   phyamd_shard_api.inc    per-device half of the C ABI: creation, setters, evaluations, single-branch calls, inspection
//   phyamd_queries.inc      ... and its whole-tree query calls: batches, NNI and SPR scores, posteriors, the full branch Hessian
//   phyamd_place_calls.inc  ... and the placement calls, 4 and 20 states over one frame
//   phyamd_abi.inc          extern "C" entry points: a handle is a group of 1..n shards on 1..n GPUs
//   phyamd_schedule_export.inc  ... and the host-only ones that export a tree's schedules (included by phyamd_abi.inc)
//
// Replaces the CPU hot path of physher's SingleTreeLikelihood (src/phyc/treelikelihood.c and the per-state-count kernel files)
// with hand-written HIP kernels.  The shipped design:
//   * 4 states: a wave keeps 64 site patterns of one rate category (one per lane) and WALKS THE TREE -- the post-order pass and
//     the pre-order pass + branch gradient are each one depth-first walk over a host-built op list (two launches: cut subtrees,
//     then the top of the tree), values handed from op to op in registers, short-lived ones parked in LDS.  Cherries, cherry +
//     tip nodes and nodes above them with 4-6 tips below are never stored: they are rebuilt from 4-bit tip codes wherever needed.
//     Both walks are software pipelines: packed mask words, per-op table blocks (LDS-DMA) and stored operands of op i + 1 are
//     requested while op i computes (phyamd_walk4s.inc; phyamd_walk4.inc = the table-gather form for parameter gradients and
//     rescaled evaluations with more than four categories; phyamd_level4.inc = one launch per tree level for incremental updates,
//     keep_partials and the reference-compatible rescaled gradients);
//   * 20 / 60 / 61 states: P . partial on v_mfma_f64_16x16x4 from LDS matrix images, one launch per tree level (pre-order) or a
//     depth-first walk (20-state post-order), cherries fused (phyamd_general.inc, phyamd_genwalk.inc);
//   * a stored node holds t_n = P_n p_n, its partial carried through its own branch: the pre-order pass reads it where it would
//     repeat that product (20 / 60 / 61 states: always; 4 states: between the two streamed walks -- every other reader of stored
//     partials gets p_n back, require_reference_form);
//   * transition matrices are built on the device from the cached eigen system and reach the 4-state kernels through
//     wave-uniform (scalar) loads;
//   * the pre-order pass computes BOTH children's uppers from one read of the parent's upper and fuses the branch-length
//     gradient into the same kernel: the reference's spare_partials array never exists;
//   * reductions are fixed-order (matrix-pipe cross-lane sums, per-block slabs, bisection-ordered segment sums), so results are
//     bitwise reproducible run to run and independent of how many GPUs share the patterns.
//
// gfx950 only; no CUDA/compat paths.

#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "physher_amd.h"

#define PHYAMD_ABI_VERSION 5

namespace {

// (inside the namespace like the .inc files: the types keep internal linkage and every kernel its symbol; the standard headers the
// two include are included above)
#include "phyamd_types.h"
#include "phyamd_tree_schedule.h"

thread_local std::string g_last_error;

int fail(int code, const char *fmt, ...) {
	char buf[512];
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(buf, sizeof buf, fmt, ap);
	va_end(ap);
	g_last_error = buf;
	return code;
}

#define HIP_TRY(expr)                                                                                       \
	do {                                                                                                    \
		hipError_t err__ = (expr);                                                                          \
		if (err__ != hipSuccess)                                                                            \
			return fail(err__ == hipErrorOutOfMemory ? PHYAMD_ENOMEM : PHYAMD_EDEVICE, "%s: %s (%s:%d)", #expr, \
			            hipGetErrorString(err__), __FILE__, __LINE__);                                      \
	} while (0)

// tuning constants (A/B measured on MI355X at 1000 taxa x 1e6 patterns): pattern groups swept
// sequentially by one workgroup, and the occupancy the pre-order kernel is compiled for
constexpr int PPT_LOWER = 2, PPT_UPPER = 8;
constexpr int UPPER_MIN_WAVES = 6;
// patterns per thread of the tree-walk kernels are chosen per engine from the shard size (phyamd_create)
constexpr int MAX_WAVES = 16;        // 1024 threads
constexpr double SCALING_THRESHOLD = 1.0e-40;  // treelikelihood.c:1121

#include "phyamd_memory.inc"

#include "phyamd_device.inc"
#include "phyamd_level4.inc"
#include "phyamd_walk4.inc"
#include "phyamd_walk4s.inc"
#include "phyamd_general.inc"
#include "phyamd_genwalk.inc"
#include "phyamd_patterns.inc"
#include "phyamd_batch4.inc"
#include "phyamd_nni4.inc"
#include "phyamd_rule.inc"
#include "phyamd_nniopt4.inc"
#include "phyamd_blopt4.inc"
#include "phyamd_spr4.inc"
#include "phyamd_tripod4.inc"
#include "phyamd_post.inc"
#include "phyamd_bhess.inc"
#include "phyamd_reweight.inc"
#include "phyamd_sitelnl.inc"
#include "phyamd_pairdist4.inc"
#include "phyamd_pairdist_gen.inc"
#include "phyamd_place4.inc"
#include "phyamd_place_gen.inc"
#include "phyamd_nni_gen.inc"
#include "phyamd_spr_gen.inc"
#include "phyamd_qopt4.inc"
#include "phyamd_qopt_gen.inc"
#include "phyamd_nniopt_gen.inc"
#include "phyamd_graft_gen.inc"

#include "phyamd_shard.inc"

#include "phyamd_schedule.inc"
#include "phyamd_launch.inc"
#include "phyamd_eval.inc"
#include "phyamd_shard_api.inc"
#include "phyamd_queries.inc"
#include "phyamd_place_calls.inc"

}  // namespace

#include "phyamd_abi.inc"
