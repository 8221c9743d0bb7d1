"""Loader for the in-tree C-ABI library (physher_amd/libphysher_amd.so).

There is no CPU fallback: if the HIP library is missing or does not load, importing the engine fails
loudly.  Build it with ``python -c "import __graft_entry__ as g; g.build()"`` or
``make -C physher_amd/csrc``.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# PHYAMD_LIB: load another build of the same ABI (A/B experiments with kernel variants); default = the in-tree library
LIB_PATH = os.environ.get("PHYAMD_LIB") or os.path.join(_HERE, "libphysher_amd.so")

ABI_VERSION = 5

OK, EINVAL, EDEVICE, ENOMEM, EUNSUPPORTED = 0, -1, -2, -3, -4
RESCALE_NEVER, RESCALE_ALWAYS, RESCALE_AUTO = 0, 1, 2
GRAD_FOLD_ROOT_FREQS, GRAD_COMPAT_SCALED = 1, 2


class Config(C.Structure):
    _fields_ = [
        ("tip_count", C.c_int32), ("pattern_count", C.c_int32), ("state_count", C.c_int32),
        ("category_count", C.c_int32), ("device", C.c_int32), ("rescale", C.c_int32),
        ("max_device_bytes", C.c_int64), ("stream", C.c_void_p),
    ]


class Profile(C.Structure):
    _fields_ = [
        ("matrices_ms", C.c_double), ("lower_ms", C.c_double), ("upper_ms", C.c_double), ("reduce_ms", C.c_double),
        ("lower_launches", C.c_int32), ("upper_launches", C.c_int32), ("device_bytes", C.c_int64), ("tiles", C.c_int32),
    ]


class NniProfile(C.Structure):
    _fields_ = [("candidates", C.c_int32), ("scratch_bytes", C.c_int64), ("ms", C.c_double)]


class NniOptimizeProfile(C.Structure):
    _fields_ = [("candidates", C.c_int32), ("chunks", C.c_int32), ("scratch_bytes", C.c_int64), ("iterations", C.c_int64), ("ms", C.c_double)]


class BranchOptimizeProfile(C.Structure):
    _fields_ = [("items", C.c_int32), ("chunks", C.c_int32), ("passes", C.c_int32), ("visits", C.c_int64), ("iterations", C.c_int64),
                ("scratch_bytes", C.c_int64), ("ms", C.c_double)]


class SprProfile(C.Structure):
    _fields_ = [("prunes", C.c_int32), ("chunks", C.c_int32), ("candidates", C.c_int64), ("scratch_bytes", C.c_int64), ("ms", C.c_double)]


class SprOptimizeProfile(C.Structure):
    _fields_ = [("prunes", C.c_int32), ("chunks", C.c_int32), ("candidates", C.c_int64), ("visits", C.c_int64), ("iterations", C.c_int64),
                ("scratch_bytes", C.c_int64), ("ms", C.c_double)]


class DistanceProfile(C.Structure):
    _fields_ = [("pairs", C.c_int32), ("chunks", C.c_int32), ("segments", C.c_int32), ("scratch_bytes", C.c_int64), ("iterations", C.c_int64),
                ("ms", C.c_double)]


class PlacementProfile(C.Structure):
    _fields_ = [("queries", C.c_int32), ("lengths", C.c_int32), ("edges", C.c_int32), ("edge_chunks", C.c_int32), ("query_chunks", C.c_int32),
                ("scratch_bytes", C.c_int64), ("ms", C.c_double)]


class PlacementOptimizeProfile(C.Structure):
    _fields_ = [("candidates", C.c_int32), ("edges", C.c_int32), ("chunks", C.c_int32), ("visits", C.c_int64), ("iterations", C.c_int64),
                ("scratch_bytes", C.c_int64), ("ms", C.c_double)]


class HessianProfile(C.Structure):
    _fields_ = [("chunks", C.c_int32), ("pairs", C.c_int64), ("scratch_bytes", C.c_int64), ("ms", C.c_double)]


class GeneralProfile(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("lower_family", "lower_slots", "lower_levels", "lower_tiles_min", "lower_tiles_max", "walk_units",
                                         "walk_workgroups", "upper_hess", "upper_slots", "upper_levels", "upper_tiles_min", "upper_tiles_max")]


class PassProfile(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("lower_family", "lower_form", "lower_scale", "lower_ambiguous", "lower_incremental", "lower_waves", "lower_ppt",
                                         "upper_family", "upper_scale", "upper_ambiguous", "upper_waves", "upper_tf", "upper_fold", "upper_compat",
                                         "upper_params", "upper_catblk", "upper_pair_ops")]


class BatchProfile(C.Structure):
    _fields_ = [
        ("items_fast", C.c_int32), ("items_sequential", C.c_int32), ("chunks", C.c_int32), ("scratch_bytes", C.c_int64), ("ms", C.c_double),
    ]


class WeightBatchProfile(C.Structure):
    _fields_ = [
        ("items_fast", C.c_int32), ("items_sequential", C.c_int32), ("item_chunks", C.c_int32), ("pattern_chunks", C.c_int32),
        ("walks", C.c_int32), ("scratch_bytes", C.c_int64), ("ms", C.c_double),
    ]


class SiteLnlProfile(C.Structure):
    _fields_ = [
        ("items", C.c_int32), ("chunks", C.c_int32), ("replicate_chunks", C.c_int32), ("lower_slots", C.c_int32),
        ("scratch_bytes", C.c_int64), ("ms", C.c_double),
    ]


# every symbol include/physher_amd.h declares: (name, restype, argtypes)
_P = C.c_void_p
SYMBOLS = [
    ("phyamd_create", C.c_int, [C.POINTER(Config), C.POINTER(_P)]),
    ("phyamd_create_sharded", C.c_int, [C.POINTER(Config), C.c_int32, _P, C.POINTER(_P)]),
    ("phyamd_shard_count", C.c_int, [_P]),
    ("phyamd_destroy", None, [_P]),
    ("phyamd_last_error", C.c_char_p, []),
    ("phyamd_abi_version", C.c_int, []),
    ("phyamd_set_tip_states", C.c_int, [_P, C.c_int, _P]),
    ("phyamd_set_tip_partials", C.c_int, [_P, C.c_int, _P]),
    ("phyamd_set_pattern_weights", C.c_int, [_P, _P]),
    ("phyamd_set_topology", C.c_int, [_P, _P, _P, C.c_int]),
    ("phyamd_set_branch_lengths", C.c_int, [_P, _P]),
    ("phyamd_set_branch_length", C.c_int, [_P, C.c_int, C.c_double]),
    ("phyamd_update_all_nodes", C.c_int, [_P]),
    ("phyamd_set_eigen", C.c_int, [_P, _P, _P, _P]),
    ("phyamd_set_frequencies", C.c_int, [_P, _P]),
    ("phyamd_set_category_rates", C.c_int, [_P, _P, _P]),
    ("phyamd_set_node_matrices", C.c_int, [_P, C.c_int, _P]),
    ("phyamd_set_matrices", C.c_int, [_P, _P]),
    ("phyamd_set_rate_matrix", C.c_int, [_P, _P]),
    ("phyamd_log_likelihood", C.c_int, [_P, C.POINTER(C.c_double)]),
    ("phyamd_gradient", C.c_int, [_P, C.c_int, C.POINTER(C.c_double), _P]),
    ("phyamd_branch_gradient", C.c_int, [_P, C.c_int, _P, C.POINTER(C.c_double), _P]),
    ("phyamd_gradient_device", C.c_int, [_P, C.c_int, _P]),
    ("phyamd_log_likelihood_device", C.c_int, [_P, _P]),
    ("phyamd_root_invariant_term", C.c_int, [_P, C.POINTER(C.c_double)]),
    ("phyamd_set_rate_matrix_derivatives", C.c_int, [_P, C.c_int, _P]),
    ("phyamd_parameter_gradient", C.c_int, [_P, C.c_int, C.POINTER(C.c_double), _P, _P]),
    ("phyamd_parameter_gradient_device", C.c_int, [_P, C.c_int, _P]),
    ("phyamd_root_frequency_term", C.c_int, [_P, _P]),
    ("phyamd_branch_log_likelihood", C.c_int, [_P, C.c_int, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ("phyamd_branch_hessian_diagonal", C.c_int, [_P, C.c_int, C.POINTER(C.c_double), _P, _P]),
    ("phyamd_branch_hessian_diagonal_device", C.c_int, [_P, C.c_int, _P]),
    ("phyamd_gradient_batch", C.c_int, [_P, C.c_int, C.c_int32, _P, _P, _P]),
    ("phyamd_gradient_batch_trees", C.c_int, [_P, C.c_int, C.c_int32, _P, _P, _P, _P, _P, _P]),
    ("phyamd_get_batch_profile", C.c_int, [_P, C.POINTER(BatchProfile)]),
    ("phyamd_nni_log_likelihoods", C.c_int, [_P, C.c_int, _P, _P, _P, _P]),
    ("phyamd_nni_log_likelihoods_general", C.c_int, [_P, C.c_int, _P, _P, _P, _P]),
    ("phyamd_get_nni_profile", C.c_int, [_P, C.POINTER(NniProfile)]),
    ("phyamd_nni_optimize", C.c_int, [_P, C.c_int, _P, C.c_double, C.c_double, C.c_double, C.c_int32, _P, _P, _P, _P, _P]),
    ("phyamd_nni_optimize_general", C.c_int, [_P, C.c_int, _P, C.c_double, C.c_double, C.c_double, C.c_int32, _P, _P, _P, _P, _P]),
    ("phyamd_get_nni_optimize_profile", C.c_int, [_P, C.POINTER(NniOptimizeProfile)]),
    ("phyamd_optimize_branch_lengths", C.c_int, [_P, C.c_int, C.c_int32, _P, _P, _P, _P, _P, C.c_double, C.c_double, C.c_double, C.c_int32, C.c_double,
                                                 C.c_int32, _P, _P, _P, _P]),
    ("phyamd_get_branch_optimize_profile", C.c_int, [_P, C.POINTER(BranchOptimizeProfile)]),
    ("phyamd_branch_sweep_schedule", C.c_int, [C.c_int32, _P, _P, C.c_int32, _P, C.c_int32]),
    ("phyamd_spr_log_likelihoods", C.c_int, [_P, C.c_int, C.c_int32, _P, _P]),
    ("phyamd_spr_log_likelihoods_general", C.c_int, [_P, C.c_int, C.c_int32, _P, _P]),
    ("phyamd_get_spr_profile", C.c_int, [_P, C.POINTER(SprProfile)]),
    ("phyamd_spr_optimize", C.c_int, [_P, C.c_int, C.c_int32, _P, C.c_double, C.c_double, C.c_double, C.c_int32, C.c_double, C.c_int32, _P, _P, _P, _P]),
    ("phyamd_spr_optimize_general", C.c_int, [_P, C.c_int, C.c_int32, _P, C.c_double, C.c_double, C.c_double, C.c_int32, C.c_double, C.c_int32, _P, _P, _P, _P]),
    ("phyamd_get_spr_optimize_profile", C.c_int, [_P, C.POINTER(SprOptimizeProfile)]),
    ("phyamd_pairwise_distances", C.c_int, [_P, C.c_int, C.c_int32, _P, _P, C.c_double, C.c_double, C.c_double, C.c_int32, _P, _P, _P, _P, _P, _P]),
    ("phyamd_pairwise_distances_general", C.c_int, [_P, C.c_int, C.c_int32, _P, _P, C.c_double, C.c_double, C.c_double, C.c_int32, _P, _P, _P, _P, _P, _P, _P]),
    ("phyamd_get_distance_profile", C.c_int, [_P, C.POINTER(DistanceProfile)]),
    ("phyamd_placement_log_likelihoods", C.c_int, [_P, C.c_int, C.c_int32, _P, C.c_int32, _P, C.c_double, _P, _P, _P]),
    ("phyamd_placement_log_likelihoods_general", C.c_int, [_P, C.c_int, C.c_int32, _P, C.c_int32, _P, C.c_int32, _P, C.c_double, _P, _P, _P]),
    ("phyamd_get_placement_profile", C.c_int, [_P, C.POINTER(PlacementProfile)]),
    ("phyamd_placement_optimize", C.c_int, [_P, C.c_int, C.c_int32, _P, C.c_int32, _P, _P, C.c_double, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_int32,
                                            C.c_double, C.c_int32, _P, _P, _P, _P]),
    ("phyamd_placement_optimize_general", C.c_int, [_P, C.c_int, C.c_int32, _P, C.c_int32, _P, C.c_int32, _P, _P, C.c_double, C.c_int32, C.c_double, C.c_double, C.c_double,
                                                    C.c_int32, C.c_double, C.c_int32, _P, _P, _P, _P]),
    ("phyamd_get_placement_optimize_profile", C.c_int, [_P, C.POINTER(PlacementOptimizeProfile)]),
    ("phyamd_state_posteriors", C.c_int, [_P, C.c_int, C.c_int32, _P, _P, _P]),
    ("phyamd_site_rate_posteriors", C.c_int, [_P, _P, _P]),
    ("phyamd_branch_hessian", C.c_int, [_P, C.c_int, _P, _P, _P]),
    ("phyamd_get_hessian_profile", C.c_int, [_P, C.POINTER(HessianProfile)]),
    ("phyamd_get_general_profile", C.c_int, [_P, C.POINTER(GeneralProfile)]),
    ("phyamd_get_pass_profile", C.c_int, [_P, C.POINTER(PassProfile)]),
    ("phyamd_gradient_batch_weights", C.c_int, [_P, C.c_int, C.c_int32, _P, _P, _P, _P]),
    ("phyamd_get_weight_batch_profile", C.c_int, [_P, C.POINTER(WeightBatchProfile)]),
    ("phyamd_pattern_log_likelihoods_trees", C.c_int, [_P, C.c_int, C.c_int32, _P, _P, _P, _P, _P, _P, C.c_int32, _P, _P]),
    ("phyamd_get_site_lnl_profile", C.c_int, [_P, C.POINTER(SiteLnlProfile)]),
    ("phyamd_synchronize", C.c_int, [_P]),
    ("phyamd_get_pattern_log_likelihoods", C.c_int, [_P, _P]),
    ("phyamd_get_partials", C.c_int, [_P, C.c_int, C.c_int, _P]),
    ("phyamd_get_node_matrices", C.c_int, [_P, C.c_int, C.c_int, _P]),
    ("phyamd_post_order_parks", C.c_int, [C.c_int32, _P, _P, C.c_int32, C.c_int32, _P, C.c_int32]),
    ("phyamd_post_order_slots", C.c_int, [C.c_int32, _P, _P, C.c_int32, _P, C.c_int32, _P]),
    ("phyamd_pre_order_schedule", C.c_int, [C.c_int32, _P, _P, C.c_int32, C.c_int32, _P, C.c_int32, _P]),
    ("phyamd_stream_elisions", C.c_int, [C.c_int32, _P, _P, C.c_int32, _P, C.c_int32]),
    ("phyamd_stream_pairs", C.c_int, [C.c_int32, _P, _P, C.c_int32, C.c_int32, _P, C.c_int32]),
    ("phyamd_stream_keeps", C.c_int, [C.c_int32, _P, _P, C.c_int32, C.c_int32, _P, C.c_int32]),
    ("phyamd_is_rescaling", C.c_int, [_P]),
    ("phyamd_set_rescaling", C.c_int, [_P, C.c_int]),
    ("phyamd_set_keep_partials", C.c_int, [_P, C.c_int]),
    ("phyamd_set_reduction_levels", C.c_int, [_P, C.c_int]),
    ("phyamd_set_profiling", C.c_int, [_P, C.c_int]),
    ("phyamd_get_profile", C.c_int, [_P, C.POINTER(Profile)]),
    ("phyamd_store", C.c_int, [_P]),
    ("phyamd_restore", C.c_int, [_P]),
    ("phyamd_compress_patterns", C.c_int, [C.c_int, C.c_int32, C.c_int64, _P, _P, C.POINTER(C.c_int32), _P, _P]),
]

_lib = None


def load():
    """dlopen the engine library and bind every declared symbol (raises if anything is missing)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build the HIP engine first (make -C physher_amd/csrc); there is no CPU fallback")
    lib = C.CDLL(LIB_PATH)
    for name, res, args in SYMBOLS:
        fn = getattr(lib, name)  # AttributeError if the .so does not export it
        fn.restype = res
        fn.argtypes = args
    if lib.phyamd_abi_version() != ABI_VERSION:
        raise ImportError(f"ABI mismatch: library {lib.phyamd_abi_version()} != binding {ABI_VERSION}")
    _lib = lib
    return lib


class EngineError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"physher_amd engine error {code}: {message}")
        self.code = code
