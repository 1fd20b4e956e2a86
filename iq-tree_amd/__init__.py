"""iq-tree_amd -- Python plumbing over the MI355X likelihood engine.

The product is two shared libraries built in-tree by `make` (see __graft_entry__.build):
  lib/libiqhip.so   HIP kernels + the C ABI of include/iqhip.h (the drop-in boundary)
  lib/libiqhost.so  C++ host mirror of the PhyloTree slice that drives the kernels
This package only loads them with ctypes; there is no Python or CPU implementation of the
likelihood path here, and loading fails loudly when the libraries are missing.

The directory name has a hyphen, so it is imported through `__graft_entry__.load_package()`
(or tests/conftest.py) under the module name `iqtree_amd`.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# IQHIP_LIB_DIR: alternative build directory (A/B timing of two builds on one GPU box)
LIB_DIR = os.environ.get("IQHIP_LIB_DIR") or os.path.join(_HERE, "lib")
REPO_ROOT = os.path.dirname(_HERE)

# every symbol include/iqhip.h declares (kept in sync by tests/test_abi.py)
IQHIP_SYMBOLS = [
    "iqhip_last_error", "iqhip_abi_version", "iqhip_device_count", "iqhip_create", "iqhip_destroy",
    "iqhip_set_stream", "iqhip_reserve", "iqhip_release", "iqhip_rekey", "iqhip_set_alignment",
    "iqhip_set_ptn_freq", "iqhip_set_ptn_invar", "iqhip_set_ascertainment", "iqhip_set_model", "iqhip_update_partials",
    "iqhip_branch_lnl", "iqhip_traverse_lnl", "iqhip_compute_theta", "iqhip_derv",
    "iqhip_lnl_from_theta", "iqhip_newton_branch", "iqhip_optimize_branch", "iqhip_bind_result_buffer", "iqhip_result_device_ptr",
    "iqhip_result_capacity", "iqhip_traverse_lnl_async", "iqhip_derv_async", "iqhip_result_read",
    "iqhip_synchronize", "iqhip_fetch_scale_num", "iqhip_fetch_pattern_lh", "iqhip_fetch_partial",
    "iqhip_fetch_theta", "iqhip_upload_partial", "iqhip_timing_enable", "iqhip_timing_read",
    "iqhip_fetch_pattern_lh_scaled", "iqhip_set_boot_samples", "iqhip_rell", "iqhip_rell_async",
    "iqhip_set_mixture_model", "iqhip_pattern_lh_cat", "iqhip_optimize_branch_batch",
    "iqhip_em_posteriors", "iqhip_em_fetch_posteriors", "iqhip_em_site_rates", "iqhip_em_objective", "iqhip_debug_em_timing",
    "iqhip_mix_class_lh", "iqhip_mix_weights_em", "iqhip_mix_posteriors", "iqhip_debug_mix_timing",
    "iqhip_class_lnl", "iqhip_debug_class_lnl_timing",
    "iqhip_create_sharded", "iqhip_num_shards", "iqhip_shard_range", "iqhip_comm_unique_id", "iqhip_comm_init_rank",
    "iqhip_comm_size", "iqhip_update_partials_async", "iqhip_lnl_from_theta_async",
    "iqhip_newton_host_init", "iqhip_newton_host_update", "iqhip_newton_host_result",
    "iqhip_debug_create_planner", "iqhip_debug_plan", "iqhip_timing_plan_bytes", "iqhip_timing_collective_read", "iqhip_optimize_sweep", "iqhip_debug_cherry_tables",
    "iqhip_debug_path_counts", "iqhip_debug_plan_shape", "iqhip_debug_plan_layout", "iqhip_debug_pair_children", "iqhip_debug_pair_rows", "iqhip_debug_planner_plain_taxa", "iqhip_debug_plan_removed",
    "iqhip_debug_fill_image", "iqhip_debug_plan_submit", "iqhip_debug_planner_event", "iqhip_debug_fill_image_chunks", "iqhip_debug_memory", "iqhip_debug_fail_alloc",
    "iqhip_ptnlh_reserve", "iqhip_ptnlh_put_current", "iqhip_ptnlh_fetch", "iqhip_optimize_branch_batch_rows",
    "iqhip_branch_tests", "iqhip_ptnlh_rell",
    "iqhip_ptnlh_upload", "iqhip_gen_boot_samples", "iqhip_ptnlh_diff_variance", "iqhip_tree_tests", "iqhip_multiscale_bp",
    "iqhip_pair_counts", "iqhip_pair_distances", "iqhip_debug_pair_timing",
    "iqhip_quartet_cells", "iqhip_quartet_likelihoods", "iqhip_debug_quartet_timing",
    "iqhip_pars_init", "iqhip_pars_update", "iqhip_pars_branch_scores", "iqhip_pars_insert_scores", "iqhip_pars_fetch", "iqhip_pars_shape",
    "iqhip_debug_pars_levels", "iqhip_debug_pars_timing",
    "iqhip_pars_insert_scores_batch", "iqhip_debug_pars_batch_timing",
    "iqhip_pars_spr_scan", "iqhip_debug_pars_spr_check", "iqhip_debug_pars_spr_timing",
    "iqhip_bionj", "iqhip_debug_bionj_timing",
    "iqhip_ufboot_init", "iqhip_ufboot_update", "iqhip_ufboot_fetch", "iqhip_debug_ufboot_timing",
    "iqhip_partition_create", "iqhip_partition_destroy", "iqhip_partition_set_rates", "iqhip_partition_newton_branch",
    "iqhip_partition_lnl_from_theta", "iqhip_partition_traverse_lnl", "iqhip_debug_partition_timing",
    "iqhip_partition_optimize_branch_batch",
    "iqhip_partition_ptnlh_reserve", "iqhip_partition_optimize_branch_batch_rows", "iqhip_partition_ptnlh_rell",
    "iqhip_partition_ufboot_init", "iqhip_partition_ufboot_update", "iqhip_partition_ufboot_fetch",
    "iqhip_partition_pair_distances", "iqhip_debug_partition_pair_timing",
    "iqhip_debug_partition_ufboot_timing",
]

# slots of iqhip_debug_path_counts (include/iqhip.h IQHIP_PATH_*)
# slots of iqhip_debug_plan_shape (include/iqhip.h IQHIP_PLAN_SHAPE_NSLOTS)
_LAUNCH_SLOTS = ("variant", "tab", "nfull", "ngroups", "grid", "lds_bytes", "hold_off")
PLAN_SHAPE_SLOTS = (("lds_budget", "lds_doubles", "state_slots", "nhold", "chunks", "stages") +
                    tuple("stage_units_%d" % s for s in range(8)) +
                    tuple("top_" + f for f in _LAUNCH_SLOTS) + tuple("unit_" + f for f in _LAUNCH_SLOTS))
PATH_SLOTS = ("newton_one_launch", "newton_chain", "sweep_persistent", "sweep_per_step", "sweep_sequential",
              "newton_fallback")


class NodeOp(C.Structure):
    """struct iqhip_node_op (include/iqhip.h)."""
    _fields_ = [("dst_key", C.c_uint64), ("left_key", C.c_uint64), ("right_key", C.c_uint64),
                ("left_leaf", C.c_int32), ("right_leaf", C.c_int32),
                ("left_len", C.c_double), ("right_len", C.c_double), ("flags", C.c_uint32), ("_pad", C.c_uint32)]


class BranchEnd(C.Structure):
    """struct iqhip_branch_end (include/iqhip.h)."""
    _fields_ = [("key", C.c_uint64), ("leaf", C.c_int32), ("_pad", C.c_int32)]


class ParsOp(C.Structure):
    """struct iqhip_pars_op (include/iqhip.h): slots."""
    _fields_ = [("dst", C.c_int32), ("left", C.c_int32), ("right", C.c_int32), ("_pad", C.c_int32)]


class BranchSupport(C.Structure):
    """struct iqhip_branch_support (include/iqhip.h)."""
    _fields_ = [("sh_alrt", C.c_double), ("lbp", C.c_double), ("abayes", C.c_double), ("alrt_stat", C.c_double)]


class TreeTest(C.Structure):
    """struct iqhip_tree_test (include/iqhip.h)."""
    _fields_ = [("rell_bp", C.c_double), ("kh_pvalue", C.c_double), ("sh_pvalue", C.c_double), ("wkh_pvalue", C.c_double),
                ("wsh_pvalue", C.c_double), ("elw_value", C.c_double), ("rell_confident", C.c_int32),
                ("elw_confident", C.c_int32)]


class UFBootTree(C.Structure):
    """struct iqhip_ufboot_tree (include/iqhip.h; 32 bytes)."""
    _fields_ = [("row", C.c_int32), ("_pad", C.c_int32), ("tree_id", C.c_int64), ("logl", C.c_double), ("rand", C.c_double)]


class BranchTask(C.Structure):
    """struct iqhip_branch_task (include/iqhip.h)."""
    _fields_ = [("ops", C.c_void_p), ("nops", C.c_int32), ("max_steps", C.c_int32), ("a", BranchEnd), ("b", BranchEnd),
                ("xguess", C.c_double), ("x1", C.c_double), ("x2", C.c_double), ("xacc", C.c_double)]


class BranchResult(C.Structure):
    """struct iqhip_branch_result (include/iqhip.h)."""
    _fields_ = [("optx", C.c_double), ("d2l", C.c_double), ("lnl", C.c_double), ("nsteps", C.c_int32), ("status", C.c_int32)]


# tree_tests / evaluate_trees: one record per tree
TREE_TEST_DTYPE = np.dtype([("logl", np.float64), ("rell_bp", np.float64), ("kh_pvalue", np.float64),
                            ("sh_pvalue", np.float64), ("wkh_pvalue", np.float64), ("wsh_pvalue", np.float64),
                            ("elw_value", np.float64), ("rell_confident", np.bool_), ("elw_confident", np.bool_)])
AU_SCALES = (0.5, 0.6, 0.7, 0.8, 0.9, 1.0, 1.1, 1.2, 1.3, 1.4)   # performAUTest, phylotesting.cpp:1920
# bionj / compute_bionj: one record per merge, the layout of struct iqhip_bionj_step (include/iqhip.h; 32 bytes)
BIONJ_STEP_DTYPE = np.dtype([("a", np.int32), ("b", np.int32), ("la", np.float64), ("lb", np.float64), ("lambda", np.float64)])
# test_all_branches: one record per internal branch
SUPPORT_DTYPE = np.dtype([("node1", np.int32), ("node2", np.int32), ("lh", np.float64, (3,)), ("sh_alrt", np.float64),
                          ("lbp", np.float64), ("abayes", np.float64), ("alrt_stat", np.float64)])


def leaf_end(leaf):
    return BranchEnd(0, int(leaf), 0)


def key_end(key):
    return BranchEnd(int(key), -1, 0)


ALLREDUCE_HOOK = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_void_p)

_libs = {}


def _load(name):
    if name in _libs:
        return _libs[name]
    path = os.path.join(LIB_DIR, name)
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: the HIP extension has not been built "
            "(run `python -c 'import __graft_entry__ as g; g.build()'` or `make`). "
            "There is no CPU fallback for the likelihood path.")
    lib = C.CDLL(path, mode=C.RTLD_GLOBAL)
    _libs[name] = lib
    return lib


def libiqhip():
    lib = _load("libiqhip.so")
    if getattr(lib, "_iq_typed", False):
        return lib
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int16)
    vp = C.c_void_p
    lib.iqhip_last_error.restype = C.c_char_p
    lib.iqhip_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int]
    lib.iqhip_destroy.argtypes = [vp]
    lib.iqhip_destroy.restype = None
    lib.iqhip_set_stream.argtypes = [vp, vp]
    lib.iqhip_reserve.argtypes = [vp, C.c_int]
    lib.iqhip_release.argtypes = [vp, C.c_uint64]
    lib.iqhip_rekey.argtypes = [vp, C.c_uint64, C.c_uint64]
    lib.iqhip_set_alignment.argtypes = [vp, C.POINTER(C.c_uint8), dp, dp]
    lib.iqhip_set_ptn_freq.argtypes = [vp, dp]
    lib.iqhip_set_ptn_invar.argtypes = [vp, dp]
    lib.iqhip_set_ascertainment.argtypes = [vp, C.c_int64, C.c_double]
    lib.iqhip_set_model.argtypes = [vp, dp, dp, dp, dp, dp, C.c_int, dp]
    lib.iqhip_set_mixture_model.argtypes = [vp, C.c_int, C.POINTER(C.c_int32), dp, dp, dp, dp, dp, C.c_int, dp]
    lib.iqhip_update_partials.argtypes = [vp, C.POINTER(NodeOp), C.c_int, dp]
    lib.iqhip_branch_lnl.argtypes = [vp, BranchEnd, BranchEnd, C.c_double, dp]
    lib.iqhip_traverse_lnl.argtypes = [vp, C.POINTER(NodeOp), C.c_int, BranchEnd, BranchEnd,
                                       C.c_double, dp, dp]
    lib.iqhip_compute_theta.argtypes = [vp, BranchEnd, BranchEnd]
    lib.iqhip_derv.argtypes = [vp, C.c_double, dp, dp]
    lib.iqhip_lnl_from_theta.argtypes = [vp, C.c_double, dp]
    lib.iqhip_optimize_branch.argtypes = [vp, C.POINTER(NodeOp), C.c_int, BranchEnd, BranchEnd, C.c_double,
                                          C.c_double, C.c_double, C.c_double, C.c_int, dp, dp, dp,
                                          C.POINTER(C.c_int)]
    lib.iqhip_newton_branch.argtypes = [vp, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, dp, dp,
                                        C.POINTER(C.c_int)]
    lib.iqhip_bind_result_buffer.argtypes = [vp, vp, C.c_int]
    lib.iqhip_result_device_ptr.argtypes = [vp]
    lib.iqhip_result_device_ptr.restype = vp
    lib.iqhip_result_capacity.argtypes = [vp]
    lib.iqhip_traverse_lnl_async.argtypes = [vp, C.POINTER(NodeOp), C.c_int, BranchEnd, BranchEnd,
                                             C.c_double]
    lib.iqhip_derv_async.argtypes = [vp, C.c_double]
    lib.iqhip_result_read.argtypes = [vp, dp, C.c_int]
    lib.iqhip_synchronize.argtypes = [vp]
    lib.iqhip_fetch_scale_num.argtypes = [vp, C.c_uint64, ip]
    lib.iqhip_fetch_pattern_lh.argtypes = [vp, dp]
    lib.iqhip_fetch_partial.argtypes = [vp, C.c_uint64, dp]
    lib.iqhip_fetch_theta.argtypes = [vp, dp]
    lib.iqhip_upload_partial.argtypes = [vp, C.c_uint64, dp, ip]
    lib.iqhip_fetch_pattern_lh_scaled.argtypes = [vp, BranchEnd, BranchEnd, dp]
    lib.iqhip_set_boot_samples.argtypes = [vp, C.POINTER(C.c_float), C.c_int]
    lib.iqhip_rell.argtypes = [vp, BranchEnd, BranchEnd, dp]
    lib.iqhip_rell_async.argtypes = [vp, BranchEnd, BranchEnd]
    lib.iqhip_create_sharded.argtypes = [C.POINTER(vp), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64,
                                         C.c_int]
    lib.iqhip_num_shards.argtypes = [vp]
    lib.iqhip_shard_range.argtypes = [vp, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int)]
    lib.iqhip_comm_unique_id.argtypes = [vp]
    lib.iqhip_comm_init_rank.argtypes = [vp, C.c_int, C.c_int, vp]
    lib.iqhip_comm_size.argtypes = [vp]
    lib.iqhip_update_partials_async.argtypes = [vp, C.POINTER(NodeOp), C.c_int]
    lib.iqhip_lnl_from_theta_async.argtypes = [vp, C.c_double]
    lib.iqhip_newton_host_init.argtypes = [vp, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, dp]
    lib.iqhip_em_posteriors.argtypes = [vp, C.c_double, dp]
    lib.iqhip_em_fetch_posteriors.argtypes = [vp, dp]
    lib.iqhip_debug_em_timing.argtypes = [vp, dp]
    lib.iqhip_em_site_rates.argtypes = [vp, dp, C.POINTER(C.c_int32)]
    lib.iqhip_em_objective.argtypes = [vp, BranchEnd, BranchEnd, C.c_double, dp, C.POINTER(C.c_int64)]
    lib.iqhip_mix_class_lh.argtypes = [vp, C.c_double, dp]
    lib.iqhip_mix_weights_em.argtypes = [vp, C.c_int, C.c_double, dp, dp, C.POINTER(C.c_int), C.POINTER(C.c_int), dp]
    lib.iqhip_mix_posteriors.argtypes = [vp, dp, dp, dp]
    lib.iqhip_debug_mix_timing.argtypes = [vp, dp, C.POINTER(C.c_int64)]
    lib.iqhip_class_lnl.argtypes = [vp, BranchEnd, BranchEnd, C.c_double, dp, dp, dp, C.POINTER(C.c_int64)]
    lib.iqhip_debug_class_lnl_timing.argtypes = [vp, dp]
    lib.iqhip_newton_host_update.argtypes = [vp, C.c_double, C.c_double, dp, C.POINTER(C.c_int)]
    lib.iqhip_newton_host_result.argtypes = [vp, dp, dp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.iqhip_timing_enable.argtypes = [vp, C.c_int]
    lib.iqhip_timing_read.argtypes = [vp, dp, C.POINTER(C.c_int64), C.c_int]
    lib.iqhip_debug_create_planner.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.iqhip_timing_plan_bytes.argtypes = [vp, dp, dp]
    lib.iqhip_timing_collective_read.argtypes = [vp, dp, C.POINTER(C.c_int64), C.c_int]
    lib.iqhip_debug_cherry_tables.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.iqhip_debug_path_counts.argtypes = [vp, C.POINTER(C.c_int64), C.c_int]
    lib.iqhip_debug_plan.argtypes = [vp, C.POINTER(NodeOp), C.c_int]
    lib.iqhip_debug_plan_shape.argtypes = [vp, C.POINTER(C.c_int64), C.c_int]
    lib.iqhip_debug_plan_layout.argtypes = [vp, C.POINTER(C.c_int32), C.c_int]
    lib.iqhip_debug_pair_rows.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.iqhip_debug_fill_image.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.iqhip_debug_plan_submit.argtypes = [vp, C.POINTER(NodeOp), C.c_int, C.POINTER(C.c_int32), C.c_int, C.c_int]
    lib.iqhip_debug_planner_event.argtypes = [vp, C.c_int]
    lib.iqhip_debug_fill_image_chunks.argtypes = [vp, C.POINTER(C.c_int64), C.c_int, C.POINTER(C.c_int)]
    lib.iqhip_debug_memory.argtypes = [C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.iqhip_debug_memory.restype = None
    lib.iqhip_debug_fail_alloc.argtypes = [C.c_int]
    lib.iqhip_debug_fail_alloc.restype = None
    i32p = C.POINTER(C.c_int32)
    lib.iqhip_ptnlh_reserve.argtypes = [vp, C.c_int]
    lib.iqhip_ptnlh_put_current.argtypes = [vp, C.c_int, BranchEnd, BranchEnd]
    lib.iqhip_ptnlh_fetch.argtypes = [vp, C.c_int, dp]
    lib.iqhip_optimize_branch_batch_rows.argtypes = [vp, C.POINTER(BranchTask), C.c_int, dp, C.POINTER(BranchResult), i32p]
    lib.iqhip_branch_tests.argtypes = [vp, i32p, dp, C.c_int, C.c_int, C.c_int, C.POINTER(BranchSupport)]
    lib.iqhip_ptnlh_rell.argtypes = [vp, i32p, C.c_int, C.c_int, dp]
    lib.iqhip_ptnlh_upload.argtypes = [vp, C.c_int, dp]
    lib.iqhip_gen_boot_samples.argtypes = [vp, C.c_int, C.c_int64, C.c_int64, C.c_uint64, C.c_uint32]
    lib.iqhip_ptnlh_diff_variance.argtypes = [vp, i32p, C.c_int, dp]
    lib.iqhip_tree_tests.argtypes = [vp, i32p, dp, C.c_int, C.c_int, C.c_double, C.c_int, C.c_uint64, C.POINTER(TreeTest)]
    lib.iqhip_multiscale_bp.argtypes = [vp, i32p, C.c_int, dp, C.c_int, C.c_int, C.c_uint64, dp]
    lib.iqhip_pair_counts.argtypes = [vp, i32p, C.c_int, dp]
    lib.iqhip_pair_distances.argtypes = [vp, dp, C.c_double, C.c_double, C.c_double, C.c_int, dp, dp, i32p]
    lib.iqhip_debug_pair_timing.argtypes = [vp, dp, dp]
    lib.iqhip_quartet_cells.argtypes = [vp, i32p, C.c_int, dp, i32p]
    lib.iqhip_quartet_likelihoods.argtypes = [vp, i32p, C.c_int, dp, C.c_double, C.c_double, C.c_double, C.c_int, C.c_double,
                                              C.c_int, C.c_double, vp]
    lib.iqhip_debug_quartet_timing.argtypes = [vp, dp, dp]
    u8p, u32p, i64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_int64)
    lib.iqhip_pars_init.argtypes = [vp, u8p, C.c_int, i64p]
    lib.iqhip_pars_update.argtypes = [vp, C.POINTER(ParsOp), C.c_int]
    lib.iqhip_pars_branch_scores.argtypes = [vp, i32p, C.c_int, i32p, i32p]
    lib.iqhip_pars_insert_scores.argtypes = [vp, i32p, C.c_int, C.c_int32, i32p, i32p, i32p]
    lib.iqhip_pars_fetch.argtypes = [vp, C.c_int32, u32p]
    lib.iqhip_pars_shape.argtypes = [vp, i64p, i64p, C.POINTER(C.c_int)]
    lib.iqhip_debug_pars_levels.argtypes = [C.c_int, C.c_int, u8p, C.POINTER(ParsOp), C.c_int, i32p]
    lib.iqhip_debug_pars_timing.argtypes = [vp, dp, i64p, C.c_int]
    lib.iqhip_pars_insert_scores_batch.argtypes = [vp, i32p, i32p, C.c_int, i32p, i32p, i32p, i32p]
    lib.iqhip_debug_pars_batch_timing.argtypes = [vp, dp, i64p, C.c_int]
    lib.iqhip_pars_spr_scan.argtypes = [vp, vp, C.c_int, vp, C.c_int, i32p, i32p, i32p, i32p]
    lib.iqhip_debug_pars_spr_check.argtypes = [C.c_int, C.c_int, u8p, vp, C.c_int, vp, C.c_int, i32p]
    lib.iqhip_debug_pars_spr_timing.argtypes = [vp, dp, i64p, C.c_int]
    lib.iqhip_bionj.argtypes = [vp, C.c_int, dp, dp, vp, i32p, dp]
    lib.iqhip_debug_bionj_timing.argtypes = [vp, dp, i64p]
    lib.iqhip_ufboot_init.argtypes = [vp, C.c_int]
    lib.iqhip_ufboot_update.argtypes = [vp, C.POINTER(UFBootTree), C.c_int, C.c_double, C.c_double, i64p, dp]
    lib.iqhip_ufboot_fetch.argtypes = [vp, dp, dp, i32p, i64p]
    lib.iqhip_debug_ufboot_timing.argtypes = [vp, dp, i64p]
    lib.iqhip_partition_create.argtypes = [C.POINTER(vp), C.POINTER(vp), C.c_int]
    lib.iqhip_partition_destroy.argtypes = [vp]
    lib.iqhip_partition_destroy.restype = None
    lib.iqhip_partition_set_rates.argtypes = [vp, dp]
    lib.iqhip_partition_newton_branch.argtypes = [vp, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, dp, dp,
                                                  C.POINTER(C.c_int), dp]
    lib.iqhip_partition_lnl_from_theta.argtypes = [vp, C.c_double, dp]
    lib.iqhip_partition_traverse_lnl.argtypes = [vp, C.POINTER(NodeOp), C.c_int, BranchEnd, BranchEnd, C.c_double, dp, dp]
    lib.iqhip_partition_optimize_branch_batch.argtypes = [vp, C.POINTER(BranchTask), C.c_int, C.POINTER(BranchResult), dp]
    lib.iqhip_debug_partition_timing.argtypes = [vp, dp, i64p]
    lib.iqhip_partition_ptnlh_reserve.argtypes = [vp, C.c_int]
    lib.iqhip_partition_optimize_branch_batch_rows.argtypes = [vp, C.POINTER(BranchTask), C.c_int, C.POINTER(BranchResult), dp,
                                                               i32p]
    lib.iqhip_partition_ptnlh_rell.argtypes = [vp, i32p, C.c_int, C.c_int, dp]
    lib.iqhip_partition_ufboot_init.argtypes = [vp, C.c_int]
    lib.iqhip_partition_ufboot_update.argtypes = [vp, C.POINTER(UFBootTree), C.c_int, C.c_double, C.c_double, i64p, dp]
    lib.iqhip_partition_ufboot_fetch.argtypes = [vp, dp, dp, i32p, i64p]
    lib.iqhip_partition_pair_distances.argtypes = [vp, dp, C.c_double, C.c_double, C.c_double, C.c_int, dp, dp, i32p]
    lib.iqhip_debug_partition_pair_timing.argtypes = [vp, dp, dp]
    lib.iqhip_debug_partition_ufboot_timing.argtypes = [vp, dp, i64p]
    lib._iq_typed = True
    return lib


def libiqhost():
    libiqhip()  # dependency, loaded RTLD_GLOBAL first
    lib = _load("libiqhost.so")
    if getattr(lib, "_iq_typed", False):
        return lib
    dp, vp = C.POINTER(C.c_double), C.c_void_p
    lib.iqhost_last_error.restype = C.c_char_p
    lib.iqhost_create.argtypes = [C.POINTER(vp), C.c_char_p, C.POINTER(C.c_char_p), C.c_int]
    lib.iqhost_destroy.argtypes = [vp]
    lib.iqhost_destroy.restype = None
    lib.iqhost_set_alignment.argtypes = [vp, C.c_int, C.c_int, C.c_int64, C.POINTER(C.c_uint8), dp, dp]
    lib.iqhost_set_ascertainment.argtypes = [vp, C.c_int64, C.c_double]
    lib.iqhost_set_ptn_freq.argtypes = [vp, dp]
    lib.iqhost_set_ptn_invar.argtypes = [vp, dp]
    lib.iqhost_set_model.argtypes = [vp, C.c_int, dp, dp, dp, dp, dp]
    lib.iqhost_set_mixture_model.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_int), dp, dp, dp, dp, dp]
    lib.iqhost_set_mem_mode.argtypes = [vp, C.c_int]
    lib.iqhost_set_kernel.argtypes = [vp, C.c_int]
    lib.iqhost_attach_engine.argtypes = [vp, C.c_int]
    lib.iqhost_attach_engine_sharded.argtypes = [vp, C.POINTER(C.c_int), C.c_int, C.c_int]
    lib.iqhost_attach_comm.argtypes = [vp, C.c_int, C.c_int, C.c_char_p]
    lib.iqhost_set_dry_run.argtypes = [vp, C.c_int]
    lib.iqhost_set_heavy_first.argtypes = [vp, C.c_int]
    lib.iqhost_set_device_newton.argtypes = [vp, C.c_int]
    lib.iqhost_set_device_sweep.argtypes = [vp, C.c_int]
    lib.iqhost_num_derv_calls.argtypes = [vp]
    lib.iqhost_num_derv_calls.restype = C.c_long
    lib.iqhost_engine.argtypes = [vp]
    lib.iqhost_engine.restype = vp
    lib.iqhost_set_allreduce_hook.argtypes = [vp, ALLREDUCE_HOOK, vp]
    for f in ("iqhost_num_nodes", "iqhost_num_leaves", "iqhost_root", "iqhost_state_unknown"):
        getattr(lib, f).argtypes = [vp]
    lib.iqhost_tip_partial_lh.argtypes = [vp, dp]
    lib.iqhost_neighbors.argtypes = [vp, C.c_int, C.POINTER(C.c_int), dp, C.c_int]
    lib.iqhost_set_branch_length.argtypes = [vp, C.c_int, C.c_int, C.c_double, C.c_int]
    lib.iqhost_neighbor_info.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_int),
                                         C.POINTER(C.c_uint64), dp, dp]
    lib.iqhost_initialize_all_partial_lh.argtypes = [vp]
    lib.iqhost_clear_all_partial_lh.argtypes = [vp]
    lib.iqhost_compute_likelihood.argtypes = [vp, dp, dp]
    lib.iqhost_clear_and_compute_likelihood.argtypes = [vp, dp]
    lib.iqhost_current_branch.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.iqhost_compute_partial.argtypes = [vp, C.c_int, C.c_int]
    lib.iqhost_compute_branch.argtypes = [vp, C.c_int, C.c_int, dp]
    lib.iqhost_compute_derv.argtypes = [vp, C.c_int, C.c_int, dp, dp]
    lib.iqhost_reset_theta.argtypes = [vp]
    lib.iqhost_compute_from_buffer.argtypes = [vp, dp]
    lib.iqhost_optimize_one_branch.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, dp]
    lib.iqhost_optimize_all_branches.argtypes = [vp, C.c_int, C.c_double, C.c_int, dp]
    lib.iqhost_set_branch_bounds.argtypes = [vp, C.c_double, C.c_double]
    lib.iqhost_nni_for_branch.argtypes = [vp, C.c_int, C.c_int, C.c_int, dp]
    lib.iqhost_evaluate_nnis_batch.argtypes = [vp, C.POINTER(C.c_int), dp, C.c_int, C.POINTER(C.c_int)]
    lib.iqhost_compute_all_partial_lh.argtypes = [vp]
    lib.iqhost_sync_inputs.argtypes = [vp]
    ipp = C.POINTER(C.c_int)
    lib.iqhost_compute_parsimony.argtypes = [vp, ipp]
    lib.iqhost_parsimony_branch.argtypes = [vp, C.c_int, C.c_int, ipp, ipp]
    lib.iqhost_initialize_all_partial_pars.argtypes = [vp]
    lib.iqhost_compute_all_partial_pars.argtypes = [vp]
    lib.iqhost_fix_negative_branch.argtypes = [vp, C.c_int, ipp]
    lib.iqhost_pars_nsites.argtypes = [vp]
    lib.iqhost_pars_nsites.restype = C.c_int64
    lib.iqhost_get_branches.argtypes = [vp, ipp, C.c_int]
    lib.iqhost_compute_parsimony_tree.argtypes = [vp, ipp, ipp, ipp, C.c_int, ipp, ipp]
    lib.iqhost_collect_spr_jobs.argtypes = [vp, C.c_int, ipp, C.c_int, ipp, ipp, C.c_int, ipp, ipp]
    lib.iqhost_apply_spr_move.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.iqhost_optimize_parsimony_spr.argtypes = [vp, C.c_int, C.c_int, ipp, ipp, C.c_int, ipp]
    lib.iqhost_parsimony_orders.argtypes = [C.c_uint64, C.c_int, C.c_int, ipp]
    lib.iqhost_pars_forest_build.argtypes = [vp, ipp, C.c_int, C.c_int, C.c_int, C.POINTER(vp), C.POINTER(C.c_int64)]
    lib.iqhost_pars_forest_free.argtypes = [vp]
    lib.iqhost_pars_forest_free.restype = None
    lib.iqhost_pars_forest_member.argtypes = [vp, C.c_int, ipp, ipp, ipp, C.c_char_p, C.c_int, ipp]
    lib.iqhost_pars_forest_trace.argtypes = [vp, C.c_int, ipp, C.c_int, ipp, ipp, C.c_int]
    lib.iqhost_compute_dist.argtypes = [vp, dp, dp, dp]
    lib.iqhost_pair_counts.argtypes = [vp, C.POINTER(C.c_int32), C.c_int, dp]
    i32q, i64q = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    lib.iqhost_quartet_cells.argtypes = [vp, i32q, C.c_int, dp, i32q]
    lib.iqhost_quartet_likelihoods.argtypes = [vp, i32q, C.c_int, C.c_int, C.c_double, dp, vp]
    lib.iqhost_likelihood_mapping.argtypes = [vp, C.c_int64, C.c_uint64, dp, C.c_int64, i64q, i32q, dp, dp, i32q, i32q, i64q,
                                              i64q]
    lib.iqhost_lmap_region.argtypes = [dp, dp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.iqhost_lmap_num_quartets.argtypes = [C.c_int]
    lib.iqhost_lmap_num_quartets.restype = C.c_int64
    lib.iqhost_lmap_all_quartets.argtypes = [C.c_int, i32q]
    lib.iqhost_lmap_draw_quartets.argtypes = [C.c_int, C.c_int64, C.c_uint64, i32q]
    lib.iqhost_bionj_newick.argtypes = [vp, C.c_int, C.POINTER(C.c_int32), dp, C.POINTER(C.c_char_p), C.c_char_p, C.c_int, ipp]
    lib.iqhost_compute_bionj.argtypes = [vp, dp, dp, vp, C.POINTER(C.c_int32), dp, C.c_char_p, C.c_int, ipp]
    lib.iqhost_evaluate_nnis5_batch.argtypes = [vp, C.POINTER(C.c_int), dp, C.c_int, C.POINTER(C.c_int)]
    lib.iqhost_tree_string.argtypes = [vp, C.c_char_p, C.c_int]
    lib.iqhost_super_create.argtypes = [C.POINTER(vp), C.c_char_p, C.POINTER(C.c_char_p), C.c_int]
    lib.iqhost_super_destroy.argtypes = [vp]
    lib.iqhost_super_destroy.restype = None
    lib.iqhost_super_add_partition.argtypes = [vp, C.c_char_p, C.POINTER(vp)]
    lib.iqhost_super_attach_engines.argtypes = [vp, C.c_int]
    lib.iqhost_super_num_parts.argtypes = [vp]
    lib.iqhost_super_group.argtypes = [vp]
    lib.iqhost_super_group.restype = vp
    lib.iqhost_super_set_fixed_rates.argtypes = [vp, C.c_int]
    lib.iqhost_super_set_rates.argtypes = [vp, dp]
    lib.iqhost_super_get_rates.argtypes = [vp, dp]
    lib.iqhost_super_part_lnl.argtypes = [vp, dp]
    lib.iqhost_super_set_branch_bounds.argtypes = [vp, C.c_double, C.c_double]
    lib.iqhost_super_compute_likelihood.argtypes = [vp, dp]
    lib.iqhost_super_optimize_one_branch.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, dp]
    lib.iqhost_super_optimize_all_branches.argtypes = [vp, C.c_int, C.c_double, C.c_int, dp]
    lib.iqhost_super_optimize_gene_rates.argtypes = [vp, C.c_double, dp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.iqhost_super_optimize_parameters.argtypes = [vp, C.c_int, C.c_double, C.c_double, dp]
    lib.iqhost_super_newton_branch.argtypes = [vp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int,
                                               dp, dp, C.POINTER(C.c_int), dp]
    lib.iqhost_super_branch_length.argtypes = [vp, C.c_int, C.c_int, dp]
    lib.iqhost_super_branch_order.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int]
    lib.iqhost_super_tree_string.argtypes = [vp, C.c_char_p, C.c_int]
    lib.iqhost_super_counters.argtypes = [vp, C.POINTER(C.c_long)]
    lib.iqhost_super_compute_dist.argtypes = [vp, dp, dp, dp]
    lib.iqhost_super_compute_bionj.argtypes = [vp, dp, dp, C.c_char_p, C.c_int, ipp]
    lib.iqhost_super_fix_negative_branch.argtypes = [vp, C.c_int, ipp]
    lib.iqhost_super_group_batches.argtypes = [vp]
    lib.iqhost_super_group_batches.restype = C.c_long
    lib.iqhost_super_set_all_branch_mode.argtypes = [vp]
    lib.iqhost_super_tree.argtypes = [vp]
    lib.iqhost_super_tree.restype = vp
    lib.iqhost_super_read_tree.argtypes = [vp, C.c_char_p]
    lib.iqhost_super_num_nodes.argtypes = [vp]
    lib.iqhost_super_num_leaves.argtypes = [vp]
    lib.iqhost_super_neighbors.argtypes = [vp, C.c_int, C.POINTER(C.c_int), dp, C.c_int]
    lib.iqhost_super_do_nni.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.iqhost_super_change_nni_brans.argtypes = [vp, C.c_int, C.c_int, dp, C.c_int]
    lib.iqhost_super_do_random_nni.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    lib.iqhost_super_save_branch_lengths.argtypes = [vp, dp, C.c_int, C.POINTER(C.c_int)]
    lib.iqhost_super_restore_branch_lengths.argtypes = [vp, dp, C.c_int]
    lib.iqhost_super_clear_all_partial_lh.argtypes = [vp]
    lib.iqhost_super_nni_for_branch.argtypes = [vp, C.c_int, C.c_int, C.c_int, dp]
    lib.iqhost_super_nni_for_branch_rows.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, dp]
    lib.iqhost_super_evaluate_nnis_list_rows.argtypes = [vp, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_int), dp,
                                                         C.c_int, C.POINTER(C.c_int)]
    lib.iqhost_super_gen_boot_samples.argtypes = [vp, C.c_int, C.c_uint64]
    lib.iqhost_super_evaluate_nnis_list.argtypes = [vp, C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int), dp, C.c_int,
                                                    C.POINTER(C.c_int)]
    lib.iqhost_evaluate_nnis5_batch_rows.argtypes = [vp, C.POINTER(C.c_int), dp, C.c_int, C.POINTER(C.c_int), C.c_int]
    lib.iqhost_test_all_branches.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), dp, C.c_int,
                                             C.POINTER(C.c_int), dp]
    lib.iqhost_gen_boot_samples.argtypes = [vp, C.c_int, C.c_int64, C.c_int64, C.c_uint64, C.c_uint32]
    lib.iqhost_evaluate_trees.argtypes = [vp, C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_int, C.c_int, dp, C.c_int,
                                          C.c_uint64, C.c_double, dp, dp]
    lib.iqhost_support_tree_string.argtypes = [vp, C.POINTER(C.c_int), dp, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int]
    lib.iqhost_fetch_scale_num.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_int16)]
    lib.iqhost_fetch_partial.argtypes = [vp, C.c_int, C.c_int, dp]
    lib.iqhost_fetch_pattern_lh.argtypes = [vp, dp]
    lib.iqhost_compute_pattern_likelihood.argtypes = [vp, dp]
    lib.iqhost_compute_pattern_lh_cat.argtypes = [vp, dp]
    lib.iqhost_set_boot_samples.argtypes = [vp, C.POINTER(C.c_float), C.c_int]
    lib.iqhost_brent_init.argtypes = [vp, C.c_double, C.c_double, C.c_double, C.c_double, dp]
    lib.iqhost_brent_update.argtypes = [vp, C.c_double, dp, C.POINTER(C.c_int)]
    lib.iqhost_brent_result.argtypes = [vp, dp, dp, C.POINTER(C.c_int)]
    lib.iqhost_modelopt_create.argtypes = [C.POINTER(vp), vp, vp, C.c_char_p, C.c_int]
    lib.iqhost_modelopt_destroy.argtypes = [vp]
    lib.iqhost_modelopt_destroy.restype = None
    lib.iqhost_modelopt_run.argtypes = [vp, C.c_int, C.c_int, C.c_double, C.c_double, dp, C.POINTER(C.c_int)]
    lib.iqhost_modelopt_string.argtypes = [vp, C.c_int, C.c_char_p, C.c_int]
    lib.iqhost_modelopt_values.argtypes = [vp, dp, dp, C.c_int]
    lib.iqhost_modelopt_trace_len.argtypes = [vp]
    lib.iqhost_modelopt_trace_row.argtypes = [vp, C.c_int, C.c_char_p, C.POINTER(C.c_int), dp, dp, dp, dp, dp, C.c_int]
    lib.iqhost_modelopt_describe.argtypes = [C.c_char_p, C.c_int, dp]
    lib.iqhost_bfgs_create.argtypes = [C.POINTER(vp), C.c_int, dp, dp, dp, C.POINTER(C.c_int), C.c_double]
    lib.iqhost_bfgs_destroy.argtypes = [vp]
    lib.iqhost_bfgs_destroy.restype = None
    lib.iqhost_bfgs_request.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.iqhost_bfgs_points.argtypes = [vp, dp, dp]
    lib.iqhost_bfgs_update.argtypes = [vp, dp, C.c_int]
    lib.iqhost_bfgs_result.argtypes = [vp, dp, dp, dp, C.POINTER(C.c_int)]
    lib.iqhost_free_rate_start.argtypes = [C.c_int, dp, dp]
    lib.iqhost_em_posteriors.argtypes = [vp, dp, dp]
    lib.iqhost_em_objective.argtypes = [vp, C.c_int, C.c_int, dp, C.POINTER(C.c_int64)]
    lib.iqhost_site_rates.argtypes = [vp, dp, C.POINTER(C.c_int)]
    lib.iqhost_optimize_free_rates_em.argtypes = [vp, dp, dp, dp, C.POINTER(C.c_int), dp, C.c_int]
    lib.iqhost_mix_class_lh.argtypes = [vp, dp]
    lib.iqhost_mix_weights_em.argtypes = [vp, C.c_int, dp, dp, C.POINTER(C.c_int), C.POINTER(C.c_int), dp]
    lib.iqhost_mix_posteriors.argtypes = [vp, dp, dp, dp]
    lib.iqhost_pattern_state_freq.argtypes = [vp, dp, dp]
    lib.iqhost_optimize_mixture_weights.argtypes = [vp, dp, dp, dp, dp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.iqhost_mix_timing.argtypes = [vp, dp, C.POINTER(C.c_int64)]
    lib.iqhost_class_lnl.argtypes = [vp, C.c_int, C.c_int, dp, dp, dp, C.POINTER(C.c_int64)]
    lib.iqhost_class_lnl_timing.argtypes = [vp, dp]
    lib.iqhost_compute_rell.argtypes = [vp, dp, C.c_int]
    i64p, cpp = C.POINTER(C.c_int64), C.POINTER(C.c_char_p)
    lib.iqhost_ufboot_init.argtypes = [vp, C.c_int, C.c_uint64]
    lib.iqhost_ufboot_params.argtypes = [vp, C.c_double, C.c_double]
    lib.iqhost_ufboot_next_iteration.argtypes = [vp]
    lib.iqhost_ufboot_info.argtypes = [vp, i64p, dp]
    lib.iqhost_save_current_tree.argtypes = [vp, C.c_double, i64p, dp]
    lib.iqhost_save_nni_trees.argtypes = [vp, i64p, dp]
    lib.iqhost_sorted_taxon_id_string.argtypes = [vp, C.c_char_p, C.c_int, ipp]
    lib.iqhost_summarize_bootstrap.argtypes = [vp, ipp, ipp, C.c_int, ipp, ipp, C.c_char_p, C.c_int, ipp]
    lib.iqhost_ufboot_newick_splits.argtypes = [C.c_char_p, C.c_int, cpp, C.POINTER(C.c_uint64), C.c_int, ipp]
    lib.iqhost_ufboot_split_supports.argtypes = [cpp, C.c_int, i64p, C.c_int, cpp, C.c_char_p, ipp, C.c_int, ipp]
    lib.iqhost_ufboot_consensus.argtypes = [cpp, C.c_int, i64p, C.c_int, cpp, C.c_char_p, C.c_int, ipp]
    # NNI tree search (search_host.h, tree_search_host.h)
    u64 = C.c_uint64
    lib.iqhost_do_nni.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.iqhost_change_nni_brans.argtypes = [vp, C.c_int, C.c_int, dp, C.c_int]
    lib.iqhost_do_random_nni.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, ipp]
    lib.iqhost_save_branch_lengths.argtypes = [vp, dp, C.c_int, ipp]
    lib.iqhost_restore_branch_lengths.argtypes = [vp, dp, C.c_int]
    lib.iqhost_evaluate_nnis_list.argtypes = [vp, C.c_int, ipp, C.c_int, C.c_int, ipp, dp, C.c_int, ipp]
    lib.iqhost_search_sort_moves.argtypes = [dp, C.c_int, ipp]
    lib.iqhost_search_select_non_conflicting.argtypes = [ipp, C.c_int, ipp, ipp]
    lib.iqhost_search_branches_for_nni.argtypes = [ipp, C.c_int, ipp, ipp, C.c_int, ipp, C.c_int, ipp]
    lib.iqhost_search_rand.argtypes = [u64, u64, u64]
    lib.iqhost_search_rand.restype = u64
    lib.iqhost_search_rand_int.argtypes = [u64, C.c_int]
    lib.iqhost_search_stop.argtypes = [C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int]
    lib.iqhost_search_bootstrap_correlation.argtypes = [C.c_int, C.c_int, ipp, C.POINTER(u64), i64p, dp]
    lib.iqhost_candset_create.argtypes = [C.POINTER(vp), C.c_int]
    lib.iqhost_candset_destroy.argtypes = [vp]
    lib.iqhost_candset_destroy.restype = None
    lib.iqhost_candset_update.argtypes = [vp, C.c_char_p, C.c_char_p, C.c_double, ipp]
    lib.iqhost_candset_size.argtypes = [vp]
    lib.iqhost_candset_exists.argtypes = [vp, C.c_char_p]
    lib.iqhost_candset_best_score.argtypes = [vp]
    lib.iqhost_candset_best_score.restype = C.c_double
    lib.iqhost_candset_rand_rank.argtypes = [vp, C.c_int, u64, ipp]
    lib.iqhost_candset_entry.argtypes = [vp, C.c_int, dp, C.c_char_p, C.c_int, ipp]
    lib.iqhost_search_create.argtypes = [C.POINTER(vp), vp]
    lib.iqhost_search_create_super.argtypes = [C.POINTER(vp), vp]
    lib.iqhost_search_destroy.argtypes = [vp]
    lib.iqhost_search_destroy.restype = None
    lib.iqhost_search_set_params.argtypes = [vp, ipp, dp, u64]
    lib.iqhost_search_optimize_nni.argtypes = [vp, dp, ipp, ipp]
    lib.iqhost_search_do_random_nnis.argtypes = [vp, C.c_int, u64, ipp, C.c_int, ipp]
    lib.iqhost_search_do_tree_search.argtypes = [vp, dp]
    lib.iqhost_search_trace_json.argtypes = [vp, C.c_char_p, C.c_int, ipp]
    lib.iqhost_last_plan.argtypes = [vp, C.POINTER(C.c_int), dp, C.POINTER(C.c_uint64), C.c_int]
    lib.iqhost_num_partial_lh_computations.argtypes = [vp]
    lib.iqhost_num_partial_lh_computations.restype = C.c_long
    lib.iqhost_num_submissions.argtypes = [vp]
    lib.iqhost_num_submissions.restype = C.c_long
    # model / alignment producers (iq-tree_amd/host/iqmodel_c.cpp)
    ip, u8p = C.POINTER(C.c_int), C.POINTER(C.c_uint8)
    lib.iqmodel_last_error.restype = C.c_char_p
    lib.iqmodel_decompose.argtypes = [dp, dp, C.c_int, C.c_int, dp, dp, dp]
    lib.iqmodel_gamma_rates.argtypes = [C.c_double, C.c_int, C.c_int, C.c_double, dp]
    for f, n in (("iqmodel_ln_gamma", 1), ("iqmodel_incomplete_gamma", 2), ("iqmodel_point_normal", 1),
                 ("iqmodel_point_chi2", 2)):
        getattr(lib, f).argtypes = [C.c_double] * n
        getattr(lib, f).restype = C.c_double
    lib.iqmodel_genetic_code.argtypes = [C.c_int]
    lib.iqmodel_genetic_code.restype = C.c_char_p
    lib.iqaln_read.argtypes = [C.POINTER(vp), C.c_char_p, C.c_char_p, C.c_char_p]
    lib.iqpart_spec_parse.argtypes = [C.POINTER(vp), C.c_char_p, C.c_int]
    lib.iqpart_spec_free.argtypes = [vp]
    lib.iqpart_spec_free.restype = None
    lib.iqpart_spec_count.argtypes = [vp]
    for f in ("iqpart_spec_model", "iqpart_spec_name", "iqpart_model", "iqpart_name"):
        getattr(lib, f).argtypes = [vp, C.c_int]
        getattr(lib, f).restype = C.c_char_p
    lib.iqpart_spec_nsites.argtypes = [vp, C.c_int]
    lib.iqpart_spec_sites.argtypes = [vp, C.c_int, C.POINTER(C.c_int)]
    lib.iqpart_read.argtypes = [C.POINTER(vp), C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p]
    lib.iqpart_free.argtypes = [vp]
    lib.iqpart_free.restype = None
    lib.iqpart_count.argtypes = [vp]
    lib.iqpart_alignment.argtypes = [vp, C.c_int, C.POINTER(vp)]
    lib.iqaln_destroy.argtypes = [vp]
    lib.iqaln_destroy.restype = None
    for f in ("iqaln_nseq", "iqaln_nsite", "iqaln_npattern", "iqaln_nstates", "iqaln_seq_type", "iqaln_state_unknown"):
        getattr(lib, f).argtypes = [vp]
    lib.iqaln_frac_const_sites.argtypes = [vp]
    lib.iqaln_frac_const_sites.restype = C.c_double
    lib.iqaln_seq_name.argtypes = [vp, C.c_int]
    lib.iqaln_seq_name.restype = C.c_char_p
    lib.iqaln_append_unobserved.argtypes = [vp, ip]
    lib.iqaln_get.argtypes = [vp, u8p, dp, ip, ip]
    lib.iqaln_ptn_invar.argtypes = [vp, C.c_double, dp, dp]
    lib.iqaln_num_informative_sites.argtypes = [vp]
    lib.iqaln_informative.argtypes = [vp, u8p]
    lib.iqaln_state_freq.argtypes = [vp, dp]
    lib.iqaln_codon_freq.argtypes = [vp, C.c_int, dp, dp]
    lib.iqaln_write_sitelh.argtypes = [vp, C.c_char_p, dp]
    lib.iqmodel_build.argtypes = [vp, C.c_char_p, ip, dp, ip, dp, dp, dp, dp, dp, dp]
    lib.iqmodel_mixture_dims.argtypes = [vp, C.c_char_p, ip, ip]
    lib.iqmodel_build_mixture.argtypes = [vp, C.c_char_p, dp, ip, dp, dp, dp, dp, dp, ip, dp, dp, dp, dp]
    lib._iq_typed = True
    return lib


def _dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


class HostError(RuntimeError):
    pass


class EngineError(HostError):
    """a raw engine call returned a status: .code is the IQHIP_ERR_* value"""

    def __init__(self, code, text):
        super().__init__("%s (status %d)" % (text, code))
        self.code = code


ERR_INVALID, ERR_UNSUPPORTED = 2, 3


def _echk(rc):
    if rc != 0:
        raise EngineError(rc, libiqhip().iqhip_last_error().decode())


def bionj_newick(steps, last, last_len, names):
    """The reference's Newick string of a BIONJ step log (PhyloTree::bionjNewick of the host mirror; no device): steps =
    records of BIONJ_STEP_DTYPE (or rows of (a, b, la, lb, lambda)), one per merge, for len(names) = len(steps) + 3 taxa;
    last / last_len = the three rows left, ascending, and their lengths.  Lengths are printed with %10.8f."""
    lib = libiqhost()
    st = np.asarray(steps)
    if st.dtype != BIONJ_STEP_DTYPE:
        rows = np.asarray(steps, dtype=np.float64).reshape(-1, 5)
        st = np.zeros(rows.shape[0], dtype=BIONJ_STEP_DTYPE)
        for k, f in enumerate(BIONJ_STEP_DTYPE.names):
            st[f] = rows[:, k]
    st = np.ascontiguousarray(st)
    n = len(names)
    if st.size != max(0, n - 3):
        raise HostError("bionj_newick: %d taxa need %d steps, not %d" % (n, max(0, n - 3), st.size))
    la = np.ascontiguousarray(last, dtype=np.int32)
    ll = np.ascontiguousarray(last_len, dtype=np.float64)
    assert la.size == 3 and ll.size == 3
    arr = (C.c_char_p * max(1, n))(*[str(x).encode() for x in names])
    need = C.c_int()
    args = (st.ctypes.data_as(C.c_void_p) if st.size else None, n, la.ctypes.data_as(C.POINTER(C.c_int32)), _dptr(ll), arr)
    if lib.iqhost_bionj_newick(*args, None, 0, C.byref(need)) != 0:
        raise HostError(lib.iqhost_last_error().decode())
    buf = C.create_string_buffer(need.value)
    if lib.iqhost_bionj_newick(*args, buf, need.value, C.byref(need)) != 0:
        raise HostError(lib.iqhost_last_error().decode())
    return buf.value.decode()


def _hchk(rc):
    if rc != 0:
        raise HostError(libiqhost().iqhost_last_error().decode())


# ---- likelihood mapping: the pure host pieces (iq-tree_amd/host/lmap_host.h)
# iqhip_quartet_result of include/iqhip.h
QUARTET_RESULT_DTYPE = np.dtype([("logl", np.float64, (3,)), ("len", np.float64, (3, 5)), ("nsweeps", np.int32, (3,)),
                                 ("neval", np.int32, (3,)), ("status", np.int32, (3,)), ("_pad", np.int32)])
assert QUARTET_RESULT_DTYPE.itemsize == 184


def lmap_region(logl3):
    """(weights[3], corner 0..2, region 0..6) of a quartet's three log-likelihoods: the Bayesian weights (differences beyond
    40 give weight 0), the corner of the best tree and the region of the triangle, ties as the reference breaks them"""
    l3 = np.ascontiguousarray(logl3, dtype=np.float64)
    assert l3.shape == (3,)
    w = np.zeros(3)
    corner, area = C.c_int(), C.c_int()
    _hchk(libiqhost().iqhost_lmap_region(_dptr(l3), _dptr(w), C.byref(corner), C.byref(area)))
    return w, corner.value, area.value


def lmap_weights(logl3):
    """the Bayesian weights of a quartet's three log-likelihoods"""
    return lmap_region(logl3)[0]


def all_quartets(n):
    """every unique quartet of n taxa, i0 < i1 < i2 < i3 in the reference's nested-loop order: int32 [C(n, 4), 4]"""
    lib = libiqhost()
    out = np.zeros((int(lib.iqhost_lmap_num_quartets(int(n))), 4), dtype=np.int32)
    _hchk(lib.iqhost_lmap_all_quartets(int(n), out.ctypes.data_as(C.POINTER(C.c_int32))))
    return out


def draw_quartets(n, count, seed):
    """count random quartets of n taxa (four distinct taxa each, in the order drawn): int32 [count, 4]; quartet q of a seed
    does not depend on count"""
    out = np.zeros((int(count), 4), dtype=np.int32)
    _hchk(libiqhost().iqhost_lmap_draw_quartets(int(n), int(count), int(seed), out.ctypes.data_as(C.POINTER(C.c_int32))))
    return out


def _c_strings(items):
    return None if items is None else (C.c_char_p * max(len(items), 1))(*[x.encode() for x in items])


def _c_weights(weights, n):
    if weights is None:
        return None, None
    w = np.ascontiguousarray(weights, dtype=np.int64)
    assert w.shape == (n,)
    return w, w.ctypes.data_as(C.POINTER(C.c_int64))


def newick_splits(newick, ntaxa, names=None):
    """The non-trivial splits of a Newick string (iq-tree_amd/host/ufboot_splits.h) in the post-order of the string, each a
    frozenset of taxon ids: the side WITHOUT taxon 0.  Leaf labels are taxon ids, or are looked up in names."""
    lib = libiqhost()
    words_per = (int(ntaxa) + 63) // 64
    cap = max(int(ntaxa), 1)
    words = np.zeros((cap, words_per), dtype=np.uint64)
    n = C.c_int()
    _hchk(lib.iqhost_ufboot_newick_splits(newick.encode(), int(ntaxa), _c_strings(names),
                                          words.ctypes.data_as(C.POINTER(C.c_uint64)), cap, C.byref(n)))
    assert n.value <= cap
    return [frozenset(t for t in range(int(ntaxa)) if (int(words[k, t >> 6]) >> (t & 63)) & 1) for k in range(n.value)]


def split_supports(trees, query, ntaxa, weights=None, names=None):
    """createBootstrapSupport's numbers: for every split of `query` (newick_splits order) round(100 count / sum of the
    weights) over `trees` (weights: one integer per tree, default 1 each); 0 for a split no tree has."""
    lib = libiqhost()
    trees = list(trees)
    cap = max(int(ntaxa), 1)
    out = np.zeros(cap, dtype=np.int32)
    n = C.c_int()
    w, wp = _c_weights(weights, len(trees))
    _hchk(lib.iqhost_ufboot_split_supports(_c_strings(trees), len(trees), wp, int(ntaxa), _c_strings(names), query.encode(),
                                           out.ctypes.data_as(C.POINTER(C.c_int)), cap, C.byref(n)))
    return [int(x) for x in out[:n.value]]


def consensus_tree(trees, ntaxa, weights=None, names=None):
    """The greedy consensus (findMaxCompatibleSplits) of `trees`: splits by descending weight, ties to the split that
    appeared first, the supports as labels; rooted at taxon 0's node, children by ascending smallest taxon."""
    lib = libiqhost()
    trees = list(trees)
    need = C.c_int()
    w, wp = _c_weights(weights, len(trees))
    args = (_c_strings(trees), len(trees), wp, int(ntaxa), _c_strings(names))
    _hchk(lib.iqhost_ufboot_consensus(*args, None, 0, C.byref(need)))
    buf = C.create_string_buffer(need.value)
    _hchk(lib.iqhost_ufboot_consensus(*args, buf, len(buf), C.byref(need)))
    return buf.value.decode()


def ufboot_rand(seed, tree_id):
    """The tie draw of tree `tree_id`: (z >> 11) 2^-53 with z of the generator of include/iqhip.h for (seed, stream 0xBB,
    rho = tree_id, j = 0)."""
    m64, g = (1 << 64) - 1, 0x9E3779B97F4A7C15

    def mix(z):
        z ^= z >> 30
        z = z * 0xBF58476D1CE4E5B9 & m64
        z ^= z >> 27
        z = z * 0x94D049BB133111EB & m64
        return z ^ (z >> 31)

    z = mix((mix((mix((int(seed) + g * (0xBB + 1)) & m64) + g * (int(tree_id) + 1)) & m64) + g) & m64)
    return (z >> 11) * 2.0 ** -53


# ---- NNI tree search: the decisions that need no likelihood (iq-tree_amd/host/search_host.h)
def _iptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def _move_field(m, key):
    return m[key] if isinstance(m, dict) else getattr(m, key)


def sort_moves(moves):
    """NNI moves (dicts with newloglh) in descending newloglh; equal scores keep their order (std::stable_sort)."""
    moves = list(moves)
    score = np.array([_move_field(m, "newloglh") for m in moves], dtype=np.float64)
    order = np.zeros(max(len(moves), 1), dtype=np.int32)
    _hchk(libiqhost().iqhost_search_sort_moves(_dptr(score), len(moves), _iptr(order)))
    return [moves[int(k)] for k in order[:len(moves)]]


def select_non_conflicting(moves):
    """genNonconfNNIs on moves (dicts with node1, node2) in sorted order: a move is kept unless one of its two nodes is an end
    of a move already kept."""
    moves = list(moves)
    nodes = np.array([[_move_field(m, "node1"), _move_field(m, "node2")] for m in moves], dtype=np.int32).reshape(-1)
    if not moves:
        nodes = np.zeros(2, dtype=np.int32)
    taken = np.zeros(max(len(moves), 1), dtype=np.int32)
    n = C.c_int()
    _hchk(libiqhost().iqhost_search_select_non_conflicting(_iptr(nodes), len(moves), _iptr(taken), C.byref(n)))
    return [moves[int(k)] for k in taken[:n.value]]


def branches_for_nni(applied, adjacency):
    """getBranchesForNNI: per applied move (node1, node2) its branch and the internal branches up to two steps away on
    either side, each once; adjacency[v] = the neighbours of node v in neighbour order, AFTER the moves were applied."""
    app = np.array([tuple(a)[:2] for a in applied], dtype=np.int32).reshape(-1)
    if app.size == 0:
        app = np.zeros(2, dtype=np.int32)
    off = np.zeros(len(adjacency) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(a) for a in adjacency])
    adj = np.array([x for a in adjacency for x in a] or [0], dtype=np.int32)
    cap = max(int(adj.size), 1)
    out = np.zeros(2 * cap, dtype=np.int32)
    n = C.c_int()
    _hchk(libiqhost().iqhost_search_branches_for_nni(_iptr(app), len(applied), _iptr(off), _iptr(adj), len(adjacency), _iptr(out),
                                                     cap, C.byref(n)))
    return [(int(out[2 * q]), int(out[2 * q + 1])) for q in range(n.value)]


def search_rand(seed, iteration, draw):
    """The search's random stream: the 64-bit splitmix value keyed by (seed, iteration, draw index)."""
    return int(libiqhost().iqhost_search_rand(int(seed), int(iteration), int(draw)))


def parsimony_orders(seed, k, ntaxa):
    """iqsearch::parsimonyOrders: the addition orders of the k parsimony starting trees of a search with `seed` -- order j is
    a Fisher-Yates shuffle of 0 .. ntaxa-1 on the draws search_rand(seed, 0, j * ntaxa + i) -> [k][ntaxa] lists"""
    out = np.zeros(max(1, int(k) * int(ntaxa)), dtype=np.int32)
    _hchk(libiqhost().iqhost_parsimony_orders(int(seed), int(k), int(ntaxa), _iptr(out)))
    return [[int(x) for x in out[j * int(ntaxa):(j + 1) * int(ntaxa)]] for j in range(int(k))]


def search_rand_int(z, n):
    """random_int(n) from a search_rand value: its top 53 bits scaled to [0, n)."""
    return int(libiqhost().iqhost_search_rand_int(int(z), int(n)))


SC_FIXED_ITERATION, SC_UNSUCCESS_ITERATION, SC_BOOTSTRAP_CORRELATION = 0, 1, 2


def stop_rule(condition, cur_iteration, cur_correlation=0.0, min_iteration=0, unsuccess_iteration=100, min_correlation=0.99,
              max_iteration=1000, last_improved=0):
    """StopRule::meetStopCondition for the three conditions the search uses."""
    return bool(libiqhost().iqhost_search_stop(int(condition), int(cur_iteration), float(cur_correlation), int(min_iteration),
                                               int(unsuccess_iteration), float(min_correlation), int(max_iteration),
                                               int(last_improved)))


def bootstrap_correlation(snapshots, ntaxa):
    """computeBootstrapCorrelation: snapshots = split-count tables {split (iterable of taxon ids): count} in the order they
    were taken; the table at index (n - 1) // 2 against the last one, a split missing on one side counting 0 there, trivial
    splits left out; the Pearson correlation.  0.0 with fewer than two snapshots."""
    wp = (int(ntaxa) + 63) // 64
    nsplits = np.array([len(s) for s in snapshots] or [0], dtype=np.int32)
    total = max(int(nsplits.sum()), 1)
    words = np.zeros((total, wp), dtype=np.uint64)
    weights = np.zeros(total, dtype=np.int64)
    at = 0
    for snap in snapshots:
        for split, w in snap.items():
            for t in split:
                words[at, t >> 6] |= np.uint64(1 << (t & 63))
            weights[at] = int(w)
            at += 1
    out = C.c_double()
    _hchk(libiqhost().iqhost_search_bootstrap_correlation(int(ntaxa), len(snapshots), _iptr(nsplits),
                                                          words.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                          weights.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(out)))
    return out.value


class CandidateSet:
    """candidateset.cpp's set of candidate trees: score -> tree, one entry per topology (the caller's topology string,
    PhyloTree.sorted_taxon_id_string)."""

    def __init__(self, max_candidates=1000):
        self.lib = libiqhost()
        self.h = C.c_void_p()
        _hchk(self.lib.iqhost_candset_create(C.byref(self.h), int(max_candidates)))

    def close(self):
        if self.h:
            self.lib.iqhost_candset_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def update(self, tree, topology, score):
        """-> True for a new topology; a known one is replaced only by a better score"""
        new = C.c_int()
        _hchk(self.lib.iqhost_candset_update(self.h, tree.encode(), topology.encode(), float(score), C.byref(new)))
        return bool(new.value)

    def __len__(self):
        return self.lib.iqhost_candset_size(self.h)

    def tree_topology_exist(self, topology):
        return bool(self.lib.iqhost_candset_exists(self.h, topology.encode()))

    @property
    def best_score(self):
        return self.lib.iqhost_candset_best_score(self.h)

    def entry(self, rank):
        """(score, tree, topology) of the rank-th best tree"""
        score, need = C.c_double(), C.c_int()
        _hchk(self.lib.iqhost_candset_entry(self.h, int(rank), C.byref(score), None, 0, C.byref(need)))
        buf = C.create_string_buffer(need.value)
        _hchk(self.lib.iqhost_candset_entry(self.h, int(rank), C.byref(score), buf, len(buf), C.byref(need)))
        tree, topo = buf.value.decode().split("\n")
        return score.value, tree, topo

    def top_trees(self, n=None):
        return [self.entry(k) for k in range(len(self) if n is None else min(n, len(self)))]

    def rand_cand_rank(self, pop_size, r):
        """getRandCandTree: the rank drawn by the search_rand value r among the best min(pop_size, size) trees"""
        rank = C.c_int()
        _hchk(self.lib.iqhost_candset_rand_rank(self.h, int(pop_size), int(r), C.byref(rank)))
        return rank.value


def _pars_ops(ops):
    a = np.ascontiguousarray(ops, dtype=np.int32).reshape(-1, 3)
    arr = (ParsOp * max(1, a.shape[0]))()
    for k, (d, l, r) in enumerate(a):
        arr[k] = ParsOp(int(d), int(l), int(r), 0)
    return arr, a.shape[0]


def pars_levels(ntaxa, nvectors, ops, valid=None):
    """iqhip_debug_pars_levels: the validation and the level of every op of an iqhip_pars_update list (ops: rows of
    (dst, left, right) slots; valid: None or nvectors flags of the slots written by earlier calls); no device needed"""
    arr, n = _pars_ops(ops)
    lev = np.zeros(max(1, n), dtype=np.int32)
    v = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint8)
    assert v is None or v.size == nvectors
    _echk(libiqhip().iqhip_debug_pars_levels(int(ntaxa), int(nvectors), None if v is None else v.ctypes.data_as(C.POINTER(C.c_uint8)),
                                            arr, n, lev.ctypes.data_as(C.POINTER(C.c_int32))))
    return lev[:n]


PARS_SPR_NO_SCORE = 1        # include/iqhip.h IQHIP_PARS_SPR_NO_SCORE
PARS_SPR_MAX_RADIUS = 10


def _spr_rows(rows, what):
    """rows of 4 int32 as the structs iqhip_pars_spr_job (subtree, first_step, nsteps[, 0]) / iqhip_pars_spr_step (parent,
    side, target[, flags]); a missing fourth column is 0"""
    a = np.asarray(rows, dtype=np.int32)
    a = a.reshape(-1, a.shape[-1] if a.ndim == 2 and a.size else 4)
    if a.shape[1] == 3:
        a = np.concatenate([a, np.zeros((a.shape[0], 1), np.int32)], axis=1)
    assert a.shape[1] == 4, what
    return np.ascontiguousarray(a)


def debug_pars_spr_check(ntaxa, nvectors, jobs, steps, valid=None):
    """iqhip_debug_pars_spr_check: the validation of an iqhip_pars_spr_scan program -> the depth of every step (-1 at steps
    of no job); jobs: rows of (subtree, first_step, nsteps), steps: rows of (parent, side, target, flags); valid: None or
    nvectors flags of the slots written so far; no device needed"""
    jb, st = _spr_rows(jobs, "jobs"), _spr_rows(steps, "steps")
    depth = np.zeros(max(1, st.shape[0]), dtype=np.int32)
    v = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint8)
    assert v is None or v.size == nvectors
    _echk(libiqhip().iqhip_debug_pars_spr_check(int(ntaxa), int(nvectors), None if v is None else v.ctypes.data_as(C.POINTER(C.c_uint8)),
                                               jb.ctypes.data_as(C.c_void_p), jb.shape[0], st.ctypes.data_as(C.c_void_p),
                                               st.shape[0], depth.ctypes.data_as(C.POINTER(C.c_int32))))
    return depth[:st.shape[0]]


LK_EIGEN, LK_EIGEN_SSE, LK_EIGEN_HIP = 0, 1, 2
REDUCE_RCCL, REDUCE_HOST = 0, 1


class NewtonStateMachine:
    """Optimization::minimizeNewton as the engine's step-at-a-time state machine (iqhip_newton_host_*)."""

    def __init__(self, xguess, x1, x2, xacc, max_steps):
        self.lib = libiqhip()
        self.buf = C.create_string_buffer(128)
        x = C.c_double()
        if self.lib.iqhip_newton_host_init(self.buf, xguess, x1, x2, xacc, max_steps, C.byref(x)) != 0:
            raise HostError(self.lib.iqhip_last_error().decode())
        self.x, self.done = x.value, False

    def update(self, df_sum, ddf_sum):
        x, d = C.c_double(), C.c_int()
        self.lib.iqhip_newton_host_update(self.buf, df_sum, ddf_sum, C.byref(x), C.byref(d))
        self.x, self.done = x.value, bool(d.value)
        return self.x

    def result(self):
        optx, d2l, n, st = C.c_double(), C.c_double(), C.c_int(), C.c_int()
        if self.lib.iqhip_newton_host_result(self.buf, C.byref(optx), C.byref(d2l), C.byref(n), C.byref(st)) != 0:
            raise HostError(self.lib.iqhip_last_error().decode())
        return optx.value, d2l.value, n.value, st.value


class BrentStateMachine:
    """Optimization::minimizeOneDimen over brent_opt as the host mirror's step-at-a-time state machine (iqhost_brent_*):
    evaluate the function at .x and feed the value to update() until .done; then result() -> (optx, fx, nevals)."""

    def __init__(self, xmin, xguess, xmax, tol):
        self.lib = libiqhost()
        self.buf = C.create_string_buffer(self.lib.iqhost_brent_state_bytes() + 8)
        self.state = C.c_void_p((C.addressof(self.buf) + 7) & ~7)
        x = C.c_double()
        if self.lib.iqhost_brent_init(self.state, xmin, xguess, xmax, tol, C.byref(x)) != 0:
            raise HostError(self.lib.iqhost_last_error().decode())
        self.x, self.done = x.value, False

    def update(self, f):
        x, d = C.c_double(), C.c_int()
        if self.lib.iqhost_brent_update(self.state, float(f), C.byref(x), C.byref(d)) != 0:
            raise HostError(self.lib.iqhost_last_error().decode())
        self.x, self.done = x.value, bool(d.value)
        return self.x

    def result(self):
        optx, fx, n = C.c_double(), C.c_double(), C.c_int()
        if self.lib.iqhost_brent_result(self.state, C.byref(optx), C.byref(fx), C.byref(n)) != 0:
            raise HostError(self.lib.iqhost_last_error().decode())
        return optx.value, fx.value, n.value


class BfgsStateMachine:
    """The first pass of Optimization::minimizeMultiDimen (dfpmin over lnsrch and the forward-difference derivativeFunk) as
    the host mirror's resumable machine (bfgs_host.h, iqhost_bfgs_*).  .kind is "stencil" (.points[ndim + 1, ndim]: the base
    point and its ndim forward points, .steps[ndim]; independent of each other, so they may be evaluated in one batch),
    "single" (.points[1, ndim]: a line-search trial) or "done".  Feed the function values, in the order of the points, to
    update() until .done; then result() -> dict(x, fret, iter, gradient, stencils, singles).  bound_check = True (the
    reference's random restart at the boundary) is refused."""
    KINDS = ("stencil", "single", "done")

    def __init__(self, guess, lower, upper, gtol, bound_check=None):
        self.lib = libiqhost()
        g, lo, up = (np.ascontiguousarray(v, dtype=np.float64) for v in (guess, lower, upper))
        self.ndim = g.size
        assert lo.size == self.ndim and up.size == self.ndim
        bc = None
        if bound_check is not None:
            bc = np.ascontiguousarray(bound_check, dtype=np.int32)
            assert bc.size == self.ndim
        self.h = C.c_void_p()
        if self.lib.iqhost_bfgs_create(C.byref(self.h), self.ndim, _dptr(g), _dptr(lo), _dptr(up),
                                       None if bc is None else bc.ctypes.data_as(C.POINTER(C.c_int)), float(gtol)) != 0:
            raise HostError(self.lib.iqhost_last_error().decode())
        self._fetch()

    def _fetch(self):
        kind, npts = C.c_int(), C.c_int()
        if self.lib.iqhost_bfgs_request(self.h, C.byref(kind), C.byref(npts)) != 0:
            raise HostError(self.lib.iqhost_last_error().decode())
        self.kind = self.KINDS[kind.value]
        self.done = self.kind == "done"
        self.points = np.zeros((npts.value, self.ndim))
        self.steps = np.zeros(self.ndim)
        if npts.value and self.lib.iqhost_bfgs_points(self.h, _dptr(self.points), _dptr(self.steps)) != 0:
            raise HostError(self.lib.iqhost_last_error().decode())
        if self.kind != "stencil":
            self.steps = None

    def update(self, values):
        v = np.ascontiguousarray(np.atleast_1d(values), dtype=np.float64)
        if self.lib.iqhost_bfgs_update(self.h, _dptr(v), v.size) != 0:
            raise HostError(self.lib.iqhost_last_error().decode())
        self._fetch()
        return self.kind

    def result(self):
        x, g, fret, cnt = np.zeros(self.ndim), np.zeros(self.ndim), C.c_double(), (C.c_int * 3)()
        if self.lib.iqhost_bfgs_result(self.h, _dptr(x), C.byref(fret), _dptr(g), cnt) != 0:
            raise HostError(self.lib.iqhost_last_error().decode())
        return dict(x=x, fret=fret.value, iter=cnt[0], gradient=g, stencils=cnt[1], singles=cnt[2])

    def close(self):
        if self.h:
            self.lib.iqhost_bfgs_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


GRADIENT_EPSILON = 0.0001   # the default of ModelFactory::optimizeParameters (model/modelfactory.h:169)
LOGL_EPSILON = 0.01         # params.modeps (tools.cpp:871)


def model_opt_describe(model_string, nstates=4):
    """No device: what ModelOptimizer would estimate for this -m string -> dict(ndim, K, lower, upper, has_gamma, has_invar,
    alpha_bounds, pinv_lower); raises HostError for what it refuses (MIX{}, +R, +ASC, +FO)."""
    lib = libiqhost()
    out = np.zeros(9)
    if lib.iqhost_modelopt_describe(model_string.encode(), int(nstates), _dptr(out)) != 0:
        raise HostError(lib.iqhost_last_error().decode())
    return dict(ndim=int(out[0]), K=int(out[1]), lower=out[2], upper=out[3], has_gamma=bool(out[4]), has_invar=bool(out[5]),
                alpha_bounds=(out[6], out[7]), pinv_lower=out[8])


class ModelOptimizer:
    """Estimation of model parameters on the device (model_opt_host.h): the DNA substitution rates by the reference's BFGS
    with the forward-difference stencil batched as the classes of a candidate mixture engine (batch=True: for alignments of
    at most BATCH_MAX_PATTERNS = 5 000 patterns, the measured crossover; batch="always": at every size), the Gamma shape
    and p-inv by Brent, inside the loop of ModelFactory::optimizeParameters.  tree: a PhyloTree holding aln's patterns
    (aln.states, aln.ptn_freq), its engine attached, with a model of the string's category count; model_string: the -m
    string, values in braces are starting values, a substitution model, +I or +G<k> without braces starts from the
    reference's defaults.  .trace: per optimiser call dict(what, requests, stencils, stencil_traversals, single_traversals,
    stencils_redone, K, lnl_before, lnl_after, x0, grad0, h0, values0 (the first stencil))."""

    def __init__(self, tree, aln, model_string, batch=True):
        self.lib = libiqhost()
        self.tree, self.aln = tree, aln          # (kept alive: the optimiser refers to both)
        self.h = C.c_void_p()
        mode = 2 if batch == "always" else int(bool(batch))
        if self.lib.iqhost_modelopt_create(C.byref(self.h), tree.h, aln.h, model_string.encode(), mode) != 0:
            raise HostError(self.lib.iqhost_last_error().decode())

    def _run(self, what, fixed_len=False, logl_epsilon=LOGL_EPSILON, gradient_epsilon=GRADIENT_EPSILON):
        lnl, rounds = C.c_double(), C.c_int()
        if self.lib.iqhost_modelopt_run(self.h, what, int(bool(fixed_len)), float(logl_epsilon), float(gradient_epsilon),
                                        C.byref(lnl), C.byref(rounds)) != 0:
            raise HostError(self.lib.iqhost_last_error().decode())
        self.rounds = rounds.value
        return lnl.value

    def optimize_model(self, gradient_epsilon=GRADIENT_EPSILON):
        """ModelGTR::optimizeParameters -> lnL (0.0: the model has no free rate parameter)"""
        return self._run(0, gradient_epsilon=gradient_epsilon)

    def optimize_rates(self, gradient_epsilon=GRADIENT_EPSILON):
        """RateGamma / RateInvar / RateGammaInvar::optimizeParameters -> lnL (0.0: neither +G nor +I)"""
        return self._run(1, gradient_epsilon=gradient_epsilon)

    def optimize_parameters(self, fixed_len=False, logl_epsilon=LOGL_EPSILON, gradient_epsilon=GRADIENT_EPSILON):
        """ModelFactory::optimizeParameters -> lnL; .rounds = the rounds taken"""
        return self._run(3, fixed_len, logl_epsilon, gradient_epsilon)

    def model_string(self):
        buf = C.create_string_buffer(4096)
        if self.lib.iqhost_modelopt_string(self.h, 0, buf, len(buf)) != 0:
            raise HostError(self.lib.iqhost_last_error().decode())
        return buf.value.decode()

    def write_info(self):
        buf = C.create_string_buffer(4096)
        if self.lib.iqhost_modelopt_string(self.h, 1, buf, len(buf)) != 0:
            raise HostError(self.lib.iqhost_last_error().decode())
        return buf.value.decode()

    def values(self):
        """-> dict(params, alpha (None without +G), p_invar (None without +I))"""
        v, p = np.zeros(5), np.zeros(8)
        if self.lib.iqhost_modelopt_values(self.h, _dptr(v), _dptr(p), p.size) != 0:
            raise HostError(self.lib.iqhost_last_error().decode())
        return dict(params=p[:int(v[0])].copy(), alpha=v[1] if v[3] else None, p_invar=v[2] if v[4] else None)

    @property
    def trace(self):
        out = []
        for k in range(self.lib.iqhost_modelopt_trace_len(self.h)):
            what, ints, lnl = C.create_string_buffer(16), (C.c_int * 7)(), np.zeros(2)
            x0, g0, h0, v0 = np.zeros(8), np.zeros(8), np.zeros(8), np.zeros(9)
            if self.lib.iqhost_modelopt_trace_row(self.h, k, what, ints, _dptr(lnl), _dptr(x0), _dptr(g0), _dptr(h0), _dptr(v0), 8) != 0:
                raise HostError(self.lib.iqhost_last_error().decode())
            n = ints[6]
            out.append(dict(what=what.value.decode(), requests=ints[0], stencils=ints[1], stencil_traversals=ints[2],
                            single_traversals=ints[3], stencils_redone=ints[4], K=ints[5], lnl_before=lnl[0], lnl_after=lnl[1],
                            x0=x0[:n].copy(), grad0=g0[:n].copy(), h0=h0[:n].copy(), values0=v0[:n + 1].copy() if n else v0[:0]))
        return out

    def close(self):
        if self.h:
            self.lib.iqhost_modelopt_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def free_rate_start(k):
    """RateFree::setNCategory: the +R<k> starting point -> (props, rates): equal weights, gamma_rates(1.0, k)."""
    lib = libiqhost()
    props, rates = np.zeros(max(1, int(k))), np.zeros(max(1, int(k)))
    if lib.iqhost_free_rate_start(int(k), _dptr(props), _dptr(rates)) != 0:
        raise HostError(lib.iqhost_last_error().decode())
    return props, rates


def comm_unique_id():
    """ncclGetUniqueId through the engine library (rank 0; broadcast the 128 bytes to the other ranks)."""
    lib = libiqhip()
    buf = C.create_string_buffer(128)
    if lib.iqhip_comm_unique_id(buf) != 0:
        raise HostError(lib.iqhip_last_error().decode())
    return buf.raw


def debug_memory():
    """iqhip_debug_memory: (device bytes, pinned / host staging bytes) live through the library's owners in this process."""
    dev, host = C.c_int64(0), C.c_int64(0)
    libiqhip().iqhip_debug_memory(C.byref(dev), C.byref(host))
    return dev.value, host.value


def debug_fail_alloc(nth):
    """iqhip_debug_fail_alloc: the nth allocation from now (1-based) fails with out-of-memory; 0 clears it."""
    libiqhip().iqhip_debug_fail_alloc(int(nth))


LM_PER_NODE, LM_ALL_BRANCH = 0, 1
SEQ_DNA, SEQ_PROTEIN, SEQ_CODON, SEQ_OTHER = 0, 1, 2, 3


class PhyloTree:
    """Thin OO view of iqhost::PhyloTree (iq-tree_amd/host/phylo_host.h)."""

    def __init__(self, newick, names=None):
        self.lib = libiqhost()
        self.h = C.c_void_p()
        if names:
            arr = (C.c_char_p * len(names))(*[n.encode() for n in names])
            rc = self.lib.iqhost_create(C.byref(self.h), newick.encode(), arr, len(names))
        else:
            rc = self.lib.iqhost_create(C.byref(self.h), newick.encode(), None, 0)
        self._chk(rc)
        self.nptn = 0
        self.block = 0

    def _chk(self, rc):
        if rc != 0:
            raise HostError(self.lib.iqhost_last_error().decode())

    def close(self):
        if self.h:
            self.lib.iqhost_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- inputs
    def set_alignment(self, nstates, seq_type, states, ptn_freq, ptn_invar=None):
        states = np.ascontiguousarray(states, dtype=np.uint8)
        self.nptn = states.shape[1]
        self.nstates = nstates
        f = np.ascontiguousarray(ptn_freq, dtype=np.float64)
        iv = np.zeros(self.nptn) if ptn_invar is None else np.ascontiguousarray(ptn_invar, dtype=np.float64)
        self._chk(self.lib.iqhost_set_alignment(self.h, nstates, seq_type, self.nptn,
                                                states.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                _dptr(f), _dptr(iv)))

    def set_ptn_freq(self, ptn_freq):
        f = np.ascontiguousarray(ptn_freq, dtype=np.float64)
        assert f.size == self.nptn
        self._chk(self.lib.iqhost_set_ptn_freq(self.h, _dptr(f)))

    def set_ptn_invar(self, ptn_invar):
        f = np.ascontiguousarray(ptn_invar, dtype=np.float64)
        assert f.size == self.nptn
        self._chk(self.lib.iqhost_set_ptn_invar(self.h, _dptr(f)))

    def set_ascertainment(self, n_unobserved, nsites):
        """+ASC: the last n_unobserved patterns of set_alignment are the unobserved constant patterns."""
        self._chk(self.lib.iqhost_set_ascertainment(self.h, int(n_unobserved), float(nsites)))

    def set_model(self, model):
        """model: object with eval, evec, inv_evec, rates, props (see synth.Model); a mixture model also
        has nclass > 1 and cat_class (component -> eigen-system), its arrays concatenated per class."""
        a = [np.ascontiguousarray(x, dtype=np.float64) for x in
             (model.eval, model.evec, model.inv_evec, model.rates, model.props)]
        self.ncat = len(a[3])
        self.block = self.nstates * self.ncat
        nclass = int(getattr(model, "nclass", 1))
        self.nclass = nclass
        if nclass > 1:
            cls = np.ascontiguousarray(model.cat_class, dtype=np.int32)
            self._chk(self.lib.iqhost_set_mixture_model(self.h, nclass, self.ncat, cls.ctypes.data_as(C.POINTER(C.c_int)),
                                                        *[_dptr(x) for x in a]))
        else:
            self._chk(self.lib.iqhost_set_model(self.h, self.ncat, *[_dptr(x) for x in a]))

    def set_mem_mode(self, lm):
        self._chk(self.lib.iqhost_set_mem_mode(self.h, lm))

    def set_likelihood_kernel(self, lk):
        self._chk(self.lib.iqhost_set_kernel(self.h, lk))

    def attach_engine(self, device=0):
        self._chk(self.lib.iqhost_attach_engine(self.h, device))

    def attach_engine_sharded(self, devices, reduce_mode=REDUCE_RCCL):
        """one engine handle over several GPUs of this process (iqhip_create_sharded)"""
        arr = (C.c_int * len(devices))(*[int(d) for d in devices])
        self._chk(self.lib.iqhost_attach_engine_sharded(self.h, arr, len(devices), int(reduce_mode)))

    def attach_comm(self, nranks, rank, unique_id):
        """one process per GPU: join this tree's engine to the other ranks' (iqhip_comm_init_rank);
        unique_id = the 128 bytes rank 0 got from comm_unique_id(), distributed by the caller"""
        assert len(unique_id) == 128
        self._chk(self.lib.iqhost_attach_comm(self.h, int(nranks), int(rank), bytes(unique_id)))

    def set_device_newton(self, on=True):
        self._chk(self.lib.iqhost_set_device_newton(self.h, int(on)))

    def set_device_sweep(self, on=True):
        """optimize_all_branches: every sweep as ONE engine submission (iqhip_optimize_sweep) instead of one per branch"""
        self._chk(self.lib.iqhost_set_device_sweep(self.h, int(on)))

    @property
    def num_derv_calls(self):
        return self.lib.iqhost_num_derv_calls(self.h)

    def set_heavy_first(self, on=True):
        self._chk(self.lib.iqhost_set_heavy_first(self.h, int(on)))

    def set_dry_run(self, on=True):
        self._chk(self.lib.iqhost_set_dry_run(self.h, int(on)))

    @property
    def engine(self):
        return self.lib.iqhost_engine(self.h)

    def path_counts(self):
        """{slot name: count} of the Newton / sweep forms the attached engine ran since it was created
        (iqhip_debug_path_counts)"""
        out = (C.c_int64 * len(PATH_SLOTS))()
        lib = libiqhip()
        if lib.iqhip_debug_path_counts(self.engine, out, len(PATH_SLOTS)) != 0:
            raise HostError(lib.iqhip_last_error().decode())
        return dict(zip(PATH_SLOTS, out))

    def set_allreduce_hook(self, fn):
        """fn(device_ptr:int, ndoubles:int) all-reduces the device result vector in place."""
        if fn is None:
            self._hook = None
            self._chk(self.lib.iqhost_set_allreduce_hook(self.h, ALLREDUCE_HOOK(0), None))
            return
        self._hook = ALLREDUCE_HOOK(lambda ptr, n, ctx: fn(ptr, n))
        self._chk(self.lib.iqhost_set_allreduce_hook(self.h, self._hook, None))

    # ---- structure
    @property
    def num_nodes(self):
        return self.lib.iqhost_num_nodes(self.h)

    @property
    def num_leaves(self):
        return self.lib.iqhost_num_leaves(self.h)

    @property
    def root(self):
        return self.lib.iqhost_root(self.h)

    @property
    def state_unknown(self):
        return self.lib.iqhost_state_unknown(self.h)

    def tip_partial_lh(self):
        out = np.zeros((self.state_unknown + 1) * self.nstates)
        self.lib.iqhost_tip_partial_lh(self.h, _dptr(out))
        return out.reshape(self.state_unknown + 1, self.nstates)

    def neighbors(self, node):
        ids = (C.c_int * 8)()
        lens = (C.c_double * 8)()
        d = self.lib.iqhost_neighbors(self.h, node, ids, lens, 8)
        return [(ids[i], lens[i]) for i in range(d)]

    def set_branch_length(self, a, b, length, clear_reverse=True):
        self._chk(self.lib.iqhost_set_branch_length(self.h, a, b, length, int(clear_reverse)))

    def neighbor_info(self, frm, to):
        comp, key = C.c_int(), C.c_uint64()
        sf, ln = C.c_double(), C.c_double()
        self._chk(self.lib.iqhost_neighbor_info(self.h, frm, to, C.byref(comp), C.byref(key),
                                                C.byref(sf), C.byref(ln)))
        return dict(computed=comp.value, key=key.value, lh_scale_factor=sf.value, length=ln.value)

    def tree_string(self):
        buf = C.create_string_buffer(1 << 20)
        self.lib.iqhost_tree_string(self.h, buf, len(buf))
        return buf.value.decode()

    # ---- the reference's call sequence
    def initialize_all_partial_lh(self):
        self._chk(self.lib.iqhost_initialize_all_partial_lh(self.h))

    def clear_all_partial_lh(self):
        self._chk(self.lib.iqhost_clear_all_partial_lh(self.h))

    def compute_likelihood(self, want_pattern_lh=False):
        lnl = C.c_double()
        if want_pattern_lh:
            plh = np.zeros(self.nptn)
            self._chk(self.lib.iqhost_compute_likelihood(self.h, C.byref(lnl), _dptr(plh)))
            return lnl.value, plh
        self._chk(self.lib.iqhost_compute_likelihood(self.h, C.byref(lnl), None))
        return lnl.value

    def clear_and_compute_likelihood(self):
        """clearAllPartialLH(); computeLikelihood() -- the model optimisers' target function"""
        lnl = C.c_double()
        self._chk(self.lib.iqhost_clear_and_compute_likelihood(self.h, C.byref(lnl)))
        return lnl.value

    def current_branch(self):
        a, b = C.c_int(), C.c_int()
        if self.lib.iqhost_current_branch(self.h, C.byref(a), C.byref(b)):
            return None
        return a.value, b.value

    def compute_partial_likelihood(self, dad, node):
        self._chk(self.lib.iqhost_compute_partial(self.h, dad, node))

    def compute_likelihood_branch(self, dad, node):
        lnl = C.c_double()
        self._chk(self.lib.iqhost_compute_branch(self.h, dad, node, C.byref(lnl)))
        return lnl.value

    def compute_likelihood_derv(self, dad, node):
        df, ddf = C.c_double(), C.c_double()
        self._chk(self.lib.iqhost_compute_derv(self.h, dad, node, C.byref(df), C.byref(ddf)))
        return df.value, ddf.value

    def reset_theta(self):
        self._chk(self.lib.iqhost_reset_theta(self.h))

    def compute_likelihood_from_buffer(self):
        lnl = C.c_double()
        self._chk(self.lib.iqhost_compute_from_buffer(self.h, C.byref(lnl)))
        return lnl.value

    def optimize_one_branch(self, a, b, clear_lh=True, max_nr_step=100):
        ln = C.c_double()
        self._chk(self.lib.iqhost_optimize_one_branch(self.h, a, b, int(clear_lh), max_nr_step, C.byref(ln)))
        return ln.value

    def optimize_all_branches(self, iterations=100, tolerance=0.001, max_nr_step=100):
        lnl = C.c_double()
        self._chk(self.lib.iqhost_optimize_all_branches(self.h, iterations, tolerance, max_nr_step, C.byref(lnl)))
        return lnl.value

    def nni_for_branch(self, a, b, nni5=False):
        """getBestNNIForBran: [(newloglh, swapped subtree at a, swapped subtree at b, [newLen...]), x2]"""
        out = np.zeros(16)
        self._chk(self.lib.iqhost_nni_for_branch(self.h, a, b, int(nni5), _dptr(out)))
        return [(out[8 * c], int(out[8 * c + 1]), int(out[8 * c + 2]), list(out[8 * c + 3:8 * c + 8])) for c in range(2)]

    def _evaluate_nnis_list(self, nni5, branches, first_row):
        if branches is None:
            br, nbr, cap = None, 0, 4 * self.num_nodes
        else:
            branches = [tuple(b) for b in branches]
            br = _iptr(np.array(branches or [(0, 0)], dtype=np.int32).reshape(-1))
            nbr, cap = len(branches), max(2 * len(branches), 1)
        w = 6 if nni5 else 2
        ids = np.zeros(4 * cap, dtype=np.int32)
        vals = np.zeros(w * cap)
        n = C.c_int()
        self._chk(self.lib.iqhost_evaluate_nnis_list(self.h, int(nni5), br, nbr, -1 if first_row is None else int(first_row),
                                                     _iptr(ids), _dptr(vals), cap, C.byref(n)))
        return ids, vals, n.value

    def evaluate_nnis_batch(self, branches=None):
        """all nni1 candidates (2 per internal branch) in one submission ->
        list of dict(node1, node2, node1_nei, node2_nei, new_len, newloglh); branches: only these internal branches
        [(a, b), ...], in list order, each with the entries the full call gives for it"""
        ids, vals, n = self._evaluate_nnis_list(False, branches, None)
        return [dict(node1=int(ids[4 * k]), node2=int(ids[4 * k + 1]), node1_nei=int(ids[4 * k + 2]),
                     node2_nei=int(ids[4 * k + 3]), new_len=float(vals[2 * k]), newloglh=float(vals[2 * k + 1]))
                for k in range(n)]

    def evaluate_nnis5_batch(self, first_row=None, branches=None):
        """all nni5 candidates in ten submissions -> list of dict(node1, node2, node1_nei, node2_nei, new_lens[5], newloglh);
        first_row: candidate k's per-pattern lnL is kept in row first_row + k of the engine's store (ptnlh_fetch);
        branches: only these internal branches, as evaluate_nnis_batch"""
        ids, vals, n = self._evaluate_nnis_list(True, branches, first_row)
        return [dict(node1=int(ids[4 * k]), node2=int(ids[4 * k + 1]), node1_nei=int(ids[4 * k + 2]),
                     node2_nei=int(ids[4 * k + 3]), new_lens=[float(x) for x in vals[6 * k:6 * k + 5]],
                     newloglh=float(vals[6 * k + 5])) for k in range(n)]

    # ---- tree edits of the NNI search (phylo_host.h) and optimizeNNI (tree_search_host.h)
    def do_nni(self, move, clear_lh=True):
        """doNNI: the subtrees at move's node1_nei and node2_nei change places wherever they hang on node1 / node2 now, so
        the same move a second time restores the tree.  move: dict(node1, node2, node1_nei, node2_nei)"""
        self._chk(self.lib.iqhost_do_nni(self.h, int(move["node1"]), int(move["node2"]), int(move["node1_nei"]),
                                         int(move["node2_nei"]), int(clear_lh)))

    def change_nni_brans(self, move, nni5=True):
        """changeNNIBrans: move's new_lens[0] (or new_len) to the central branch; with nni5 new_lens[1..4] to the other branches
        of node1, then node2, in neighbour order after the swap"""
        lens = np.zeros(5)
        if "new_lens" in move:
            lens[:len(move["new_lens"])] = move["new_lens"]
        else:
            lens[0] = move["new_len"]
        self._chk(self.lib.iqhost_change_nni_brans(self.h, int(move["node1"]), int(move["node2"]), _dptr(lens), int(nni5)))

    def do_random_nni(self, a, b, bit1, bit2):
        """doOneRandomNNI on the internal branch (a, b) with its two coin flips as arguments -> the move that was made.  No
        likelihood vector is cleared: clear_all_partial_lh() is the caller's"""
        out = np.zeros(4, dtype=np.int32)
        self._chk(self.lib.iqhost_do_random_nni(self.h, int(a), int(b), int(bit1), int(bit2), _iptr(out)))
        return dict(node1=int(out[0]), node2=int(out[1]), node1_nei=int(out[2]), node2_nei=int(out[3]))

    def save_branch_lengths(self):
        n = C.c_int()
        self._chk(self.lib.iqhost_save_branch_lengths(self.h, None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1))
        self._chk(self.lib.iqhost_save_branch_lengths(self.h, _dptr(out), n.value, C.byref(n)))
        return out[:n.value].copy()

    def restore_branch_lengths(self, lengths):
        """the lengths of save_branch_lengths back onto the same Neighbor objects (they keep their branch through do_nni);
        every likelihood vector is stale afterwards: clear_all_partial_lh()"""
        v = np.ascontiguousarray(lengths, dtype=np.float64)
        self._chk(self.lib.iqhost_restore_branch_lengths(self.h, _dptr(v), v.size))

    def optimize_nni(self, nni5=True, speed=True, batched=True, trace=False):
        """compute_likelihood(), then IQTree::optimizeNNI -> (lnL, NNIs applied, steps) or, with trace, (lnL, NNIs applied,
        steps, [per step dict(branches, all_branches, evaluated, positive, applied, score, rolled_back, submissions)])"""
        ts = TreeSearch(self, nni5=nni5, speed=speed, batched=batched)
        try:
            return ts.optimize_nni(trace=trace)
        finally:
            ts.close()

    # ---- SH-aLRT / local bootstrap (include/iqhip.h "branch supports")
    def _hip(self, rc):
        if rc != 0:
            raise HostError(libiqhip().iqhip_last_error().decode())

    def test_all_branches(self, reps, lbp_reps=0, batched=True):
        """PhyloTree::testAllBranches on the device with the samples of set_boot_samples: a SUPPORT_DTYPE record per
        internal branch (lh = lnL of the tree and of its two NNI neighbours; fractions over max(reps, lbp_reps)
        replicates).  Row 0 of the engine's store then holds the tree's per-pattern lnL, rows 1 + 2 q + cnt the
        neighbours'.  batched=False evaluates the neighbours branch by branch (getBestNNIForBran)."""
        cap = self.num_nodes
        ids = np.zeros(2 * cap, dtype=np.int32)
        vals = np.zeros(7 * cap)
        n, lnl = C.c_int(), C.c_double()
        self._chk(self.lib.iqhost_test_all_branches(self.h, int(reps), int(lbp_reps), int(bool(batched)),
                                                    ids.ctypes.data_as(C.POINTER(C.c_int)), _dptr(vals), cap, C.byref(n),
                                                    C.byref(lnl)))
        out = np.zeros(n.value, dtype=SUPPORT_DTYPE)
        v = vals[:7 * n.value].reshape(n.value, 7)
        out["node1"], out["node2"] = ids[0:2 * n.value:2], ids[1:2 * n.value:2]
        out["lh"] = v[:, 0:3]
        for k, f in enumerate(("sh_alrt", "lbp", "abayes", "alrt_stat")):
            out[f] = v[:, 3 + k]
        return out

    def support_tree_string(self, supports, with_sh=True, with_lbp=False):
        """the tree with `SH-aLRT[/LBP]` labels (percent) on its internal nodes, the reference's label order"""
        n = len(supports)
        ids = np.zeros(2 * max(n, 1), dtype=np.int32)
        vals = np.zeros(7 * max(n, 1))
        for q in range(n):
            ids[2 * q], ids[2 * q + 1] = supports["node1"][q], supports["node2"][q]
            vals[7 * q + 3], vals[7 * q + 4] = supports["sh_alrt"][q], supports["lbp"][q]
        buf = C.create_string_buffer(1 << 20)
        self._chk(self.lib.iqhost_support_tree_string(self.h, ids.ctypes.data_as(C.POINTER(C.c_int)), _dptr(vals), n,
                                                      int(with_sh), int(with_lbp), buf, len(buf)))
        return buf.value.decode()

    def ptnlh_reserve(self, nrows):
        self._hip(libiqhip().iqhip_ptnlh_reserve(self.engine, int(nrows)))

    def ptnlh_put_current(self, row, a, b):
        """row <- per-pattern lnL of the branch (a, b) (BranchEnd) the last lnL evaluation ran on"""
        self._hip(libiqhip().iqhip_ptnlh_put_current(self.engine, int(row), a, b))

    def ptnlh_fetch(self, row):
        out = np.zeros(self.nptn)
        self._hip(libiqhip().iqhip_ptnlh_fetch(self.engine, int(row), _dptr(out)))
        return out

    def ptnlh_rell(self, rows, nsamples):
        """R[i, s] = <store row rows[i], boot sample s> for the first nsamples samples (matrix-core product)"""
        r = np.ascontiguousarray(rows, dtype=np.int32)
        out = np.zeros((r.size, int(nsamples)))
        self._hip(libiqhip().iqhip_ptnlh_rell(self.engine, r.ctypes.data_as(C.POINTER(C.c_int32)), r.size, int(nsamples),
                                              _dptr(out)))
        return out

    def branch_tests(self, rows3, lh3, reps_sh, reps_lbp=0):
        """iqhip_branch_tests: rows3 [nbranch, 3] store rows, lh3 [nbranch, 3] total lnL -> [nbranch, 4] =
        sh_alrt, lbp, abayes, alrt_stat"""
        r = np.ascontiguousarray(rows3, dtype=np.int32).reshape(-1, 3)
        l = np.ascontiguousarray(lh3, dtype=np.float64).reshape(-1, 3)
        assert r.shape == l.shape
        out = (BranchSupport * max(r.shape[0], 1))()
        self._hip(libiqhip().iqhip_branch_tests(self.engine, r.ctypes.data_as(C.POINTER(C.c_int32)), _dptr(l), r.shape[0],
                                                int(reps_sh), int(reps_lbp), out))
        return np.array([[o.sh_alrt, o.lbp, o.abayes, o.alrt_stat] for o in out[:r.shape[0]]])

    # ---- tree topology tests (include/iqhip.h "tree topology tests")
    def ptnlh_upload(self, row, values):
        """store row <- nptn host doubles (the counterpart of ptnlh_fetch)"""
        v = np.ascontiguousarray(values, dtype=np.float64)
        assert v.size == self.nptn
        self._hip(libiqhip().iqhip_ptnlh_upload(self.engine, int(row), _dptr(v)))

    def gen_boot_samples(self, nsamples, ndraws, seed, stream=0xA0, first_replicate=0):
        """iqhip_gen_boot_samples: rows [0, nsamples) of the sample matrix drawn on the device (ndraws sites each)"""
        self._chk(self.lib.iqhost_gen_boot_samples(self.h, int(nsamples), int(first_replicate), int(ndraws), int(seed),
                                                   int(stream)))
        self._nboot = int(nsamples)

    def ptnlh_diff_variance(self, rows):
        """computeLogLDiffVariance for all pairs of store rows -> [nrows, nrows]"""
        r = np.ascontiguousarray(rows, dtype=np.int32)
        out = np.zeros((r.size, r.size))
        self._hip(libiqhip().iqhip_ptnlh_diff_variance(self.engine, r.ctypes.data_as(C.POINTER(C.c_int32)), r.size, _dptr(out)))
        return out

    def tree_tests(self, rows, lh, nsamples, epsilon=0.5, weighted=False, tie_seed=0):
        """iqhip_tree_tests -> TREE_TEST_DTYPE record per tree (logl = lh)"""
        r = np.ascontiguousarray(rows, dtype=np.int32)
        l = np.ascontiguousarray(lh, dtype=np.float64)
        assert r.shape == l.shape and r.ndim == 1
        res = (TreeTest * max(r.size, 1))()
        self._hip(libiqhip().iqhip_tree_tests(self.engine, r.ctypes.data_as(C.POINTER(C.c_int32)), _dptr(l), r.size,
                                              int(nsamples), float(epsilon), int(bool(weighted)), int(tie_seed), res))
        out = np.zeros(r.size, dtype=TREE_TEST_DTYPE)
        out["logl"] = l
        for f in TREE_TEST_DTYPE.names[1:]:
            out[f] = [getattr(o, f) for o in res[:r.size]]
        return out

    def multiscale_bp(self, rows, scales, nsamples, seed):
        """iqhip_multiscale_bp -> bp[nscales, ntrees], the bootstrap proportions of the AU test's STEP 2"""
        r = np.ascontiguousarray(rows, dtype=np.int32)
        sc = np.ascontiguousarray(scales, dtype=np.float64)
        out = np.zeros((sc.size, r.size))
        self._hip(libiqhip().iqhip_multiscale_bp(self.engine, r.ctypes.data_as(C.POINTER(C.c_int32)), r.size, _dptr(sc), sc.size,
                                                 int(nsamples), int(seed), _dptr(out)))
        return out

    def evaluate_trees(self, newicks, nsamples, fixed_lengths=False, weighted=False, au_scales=None, seed=1, epsilon=0.5):
        """evaluateTrees (-z trees -zb nsamples [-zw] [-au]) on the device: (TREE_TEST_DTYPE record per tree,
        bp[nscales, ntrees] of the AU scales or None).  Store row t holds tree t's per-pattern lnL afterwards."""
        n = len(newicks)
        arr = (C.c_char_p * n)(*[s.encode() for s in newicks])
        sc = np.ascontiguousarray([] if au_scales is None else au_scales, dtype=np.float64)
        vals = np.zeros(9 * max(n, 1))
        bp = np.zeros((max(sc.size, 1), max(n, 1)))
        self._chk(self.lib.iqhost_evaluate_trees(self.h, arr, n, int(bool(fixed_lengths)), int(nsamples), int(bool(weighted)),
                                                 _dptr(sc), sc.size, int(seed), float(epsilon), _dptr(vals), _dptr(bp)))
        self._nboot = int(nsamples)
        out = np.zeros(n, dtype=TREE_TEST_DTYPE)
        v = vals[:9 * n].reshape(n, 9)
        for k, f in enumerate(TREE_TEST_DTYPE.names):
            out[f] = v[:, k]
        return out, (bp[:sc.size, :n].copy() if sc.size else None)

    # ---- pairwise ML distances (include/iqhip.h "pairwise maximum-likelihood distances")
    def pair_counts(self, pairs):
        """iqhip_pair_counts: pairs [npairs, 2] taxon ids -> counts[npairs, nstates, nstates], the pair-state frequencies
        of AlignmentPairwise (patterns with an ambiguous or unknown state in either taxon are skipped)"""
        pr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        out = np.zeros((pr.shape[0], self.nstates, self.nstates))
        self._chk(self.lib.iqhost_pair_counts(self.h, pr.ctypes.data_as(C.POINTER(C.c_int32)), pr.shape[0], _dptr(out)))
        return out

    def compute_dist(self, init=None, want_d2l=False):
        """PhyloTree::computeDist(dist_mat, var_mat): the ML distance of every pair of sequences under the current model,
        dist[ntaxa, ntaxa] (symmetric, zero diagonal); with want_d2l also minimizeNewton's d2l per pair.  init: None or
        [ntaxa, ntaxa] initial distances, 0 = start from the pair's JC distance."""
        n = self.num_leaves
        dist, d2l = np.zeros((n, n)), np.zeros((n, n))
        ini = None if init is None else np.ascontiguousarray(init, dtype=np.float64)
        assert ini is None or ini.shape == (n, n)
        self._chk(self.lib.iqhost_compute_dist(self.h, None if ini is None else _dptr(ini), _dptr(dist), _dptr(d2l)))
        return (dist, d2l) if want_d2l else dist

    # ---- likelihood mapping (include/iqhip.h "Likelihood mapping")
    @staticmethod
    def _quartets(quartets):
        q = np.ascontiguousarray(quartets, dtype=np.int32).reshape(-1, 4)
        return q, q.ctypes.data_as(C.POINTER(C.c_int32))

    def quartet_cells(self, quartets):
        """iqhip_quartet_cells: quartets [nq, 4] taxon ids -> (cells [nq, 4, 4, 4, 4] indexed by the four unambiguous states in
        quartet order, nother [nq] = the patterns with an ambiguous or unknown state among the four)"""
        q, qp = self._quartets(quartets)
        cells = np.zeros((q.shape[0], 4, 4, 4, 4))
        nother = np.zeros(q.shape[0], dtype=np.int32)
        self._chk(self.lib.iqhost_quartet_cells(self.h, qp, q.shape[0], _dptr(cells), nother.ctypes.data_as(C.POINTER(C.c_int32))))
        return cells, nother

    def quartet_likelihoods(self, quartets, iterations=10, tolerance=0.1, const_invar=None):
        """PhyloTree::computeQuartetLikelihoods: per quartet the three trees 12|34, 13|24, 14|23 from Fitch starting lengths
        through optimizeAllBranches(iterations, tolerance), one engine call -> records of QUARTET_RESULT_DTYPE (logl[3],
        len[3, 5]: pendant branches of the tree's four taxa, then the internal one; nsweeps, neval, status).  const_invar:
        None or (p_inv pi[0..3], p_inv) of a +I model."""
        q, qp = self._quartets(quartets)
        out = np.zeros(q.shape[0], dtype=QUARTET_RESULT_DTYPE)
        ci = None if const_invar is None else np.ascontiguousarray(const_invar, dtype=np.float64)
        assert ci is None or ci.shape == (5,)
        self._chk(self.lib.iqhost_quartet_likelihoods(self.h, qp, q.shape[0], int(iterations), float(tolerance),
                                                      None if ci is None else _dptr(ci), out.ctypes.data_as(C.c_void_p)))
        return out

    def likelihood_mapping(self, nquartets=0, seed=0, const_invar=None):
        """PhyloTree::doLikelihoodMapping: nquartets = 0 (or >= C(ntaxa, 4)) evaluates every unique quartet, otherwise
        draw_quartets(ntaxa, nquartets, seed) -> AttrDict(seq_id [nq, 4], logl [nq, 3], qweight [nq, 3], corner [nq], area [nq],
        areacount [7], cornercount [3], seq_count [ntaxa + 1, 10]: regions 0..6 and corners 7..9 per sequence, last row all)"""
        ci = None if const_invar is None else np.ascontiguousarray(const_invar, dtype=np.float64)
        assert ci is None or ci.shape == (5,)
        cip = None if ci is None else _dptr(ci)
        nq = C.c_int64()
        i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
        self._chk(self.lib.iqhost_likelihood_mapping(self.h, int(nquartets), int(seed), cip, 0, C.byref(nq), None, None, None,
                                                     None, None, None, None))
        n = nq.value
        seq_id, logl, w = np.zeros((n, 4), dtype=np.int32), np.zeros((n, 3)), np.zeros((n, 3))
        corner, area = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        counts = np.zeros(10, dtype=np.int64)
        seq_count = np.zeros((self.num_leaves + 1, 10), dtype=np.int64)
        self._chk(self.lib.iqhost_likelihood_mapping(self.h, int(nquartets), int(seed), cip, n, C.byref(nq),
                                                     seq_id.ctypes.data_as(i32p), _dptr(logl), _dptr(w),
                                                     corner.ctypes.data_as(i32p), area.ctypes.data_as(i32p),
                                                     counts.ctypes.data_as(i64p), seq_count.ctypes.data_as(i64p)))
        return AttrDict(seq_id=seq_id, logl=logl, qweight=w, corner=corner, area=area, areacount=counts[:7].copy(),
                        cornercount=counts[7:].copy(), seq_count=seq_count)

    def quartet_timing(self):
        """(cells_ms, solve_ms): device time of the last quartet_likelihoods call's launches (with iqhip_timing_enable)"""
        a, b = C.c_double(), C.c_double()
        self._hip(libiqhip().iqhip_debug_quartet_timing(self.engine, C.byref(a), C.byref(b)))
        return a.value, b.value

    # ---- BIONJ (include/iqhip.h "BIONJ")
    def bionj(self, dist, var=None):
        """iqhip_bionj on the attached engine (it supplies the device and the stream only): dist [n, n], any n >= 3, var
        None (V = D) or [n, n] -> (steps of BIONJ_STEP_DTYPE [n - 3], last int32[3], last_len float64[3]).  A status other
        than OK raises EngineError with its code."""
        d = np.ascontiguousarray(dist, dtype=np.float64)
        assert d.ndim == 2 and d.shape[0] == d.shape[1]
        n = d.shape[0]
        v = None if var is None else np.ascontiguousarray(var, dtype=np.float64)
        assert v is None or v.shape == d.shape
        steps = np.zeros(max(0, n - 3), dtype=BIONJ_STEP_DTYPE)
        last, last_len = np.zeros(3, dtype=np.int32), np.zeros(3)
        _echk(libiqhip().iqhip_bionj(self.engine, n, _dptr(d), None if v is None else _dptr(v),
                                     steps.ctypes.data_as(C.c_void_p) if steps.size else None,
                                     last.ctypes.data_as(C.POINTER(C.c_int32)), _dptr(last_len)))
        return steps, last, last_len

    def bionj_timing(self):
        """iqhip_debug_bionj_timing -> (device milliseconds of the last bionj call, 0 unless timing is enabled; its launches)"""
        ms, launches = C.c_double(), C.c_int64()
        _echk(libiqhip().iqhip_debug_bionj_timing(self.engine, C.byref(ms), C.byref(launches)))
        return ms.value, launches.value

    def compute_bionj(self, dist=None, var=None):
        """PhyloTree::computeBioNJ: the BIONJ tree of dist [ntaxa, ntaxa] (None: compute_dist() first) replaces the tree
        -> (newick, steps, last, last_len); the Newick string is the reference's, leaf labels = the current ones."""
        n = self.num_leaves
        d = self.compute_dist() if dist is None else np.ascontiguousarray(dist, dtype=np.float64)
        v = None if var is None else np.ascontiguousarray(var, dtype=np.float64)
        assert d.shape == (n, n) and (v is None or v.shape == (n, n))
        steps = np.zeros(max(1, n - 3), dtype=BIONJ_STEP_DTYPE)
        last, last_len = np.zeros(3, dtype=np.int32), np.zeros(3)
        cap = 1 << 20
        while True:
            buf, need = C.create_string_buffer(cap), C.c_int()
            self._chk(self.lib.iqhost_compute_bionj(self.h, _dptr(d), None if v is None else _dptr(v),
                                                    steps.ctypes.data_as(C.c_void_p), last.ctypes.data_as(C.POINTER(C.c_int32)),
                                                    _dptr(last_len), buf, cap, C.byref(need)))
            if need.value <= cap:
                return buf.value.decode(), steps[:max(0, n - 3)].copy(), last, last_len
            cap = need.value   # (a string beyond 1 MB: the call is repeated with room for it and gives the same tree)

    def compute_all_partial_lh(self):
        self._chk(self.lib.iqhost_compute_all_partial_lh(self.h))

    # ---- Fitch parsimony (PhyloTree::computeParsimony ... computeParsimonyTree of the host mirror)
    def compute_parsimony(self):
        """the Fitch parsimony score of the tree over the parsimony-informative sites"""
        out = C.c_int()
        self._chk(self.lib.iqhost_compute_parsimony(self.h, C.byref(out)))
        return out.value

    def parsimony_branch(self, a, b):
        """computeParsimonyBranch at branch a-b -> (score, substitutions on the branch)"""
        sc, sb = C.c_int(), C.c_int()
        self._chk(self.lib.iqhost_parsimony_branch(self.h, int(a), int(b), C.byref(sc), C.byref(sb)))
        return sc.value, sb.value

    def initialize_all_partial_pars(self):
        self._chk(self.lib.iqhost_initialize_all_partial_pars(self.h))

    def compute_all_partial_pars(self):
        self._chk(self.lib.iqhost_compute_all_partial_pars(self.h))

    @property
    def pars_nsites(self):
        """parsimony-informative sites of the last initialisation"""
        return int(self.lib.iqhost_pars_nsites(self.h))

    def fix_negative_branch(self, force=True):
        """fixNegativeBranch: branch lengths from the per-branch substitution counts (Jukes-Cantor corrected) -> branches set"""
        out = C.c_int()
        self._chk(self.lib.iqhost_fix_negative_branch(self.h, int(force), C.byref(out)))
        return out.value

    def get_branches(self):
        """MTree::getBranches from the root: [(node1, node2)] with node1 < node2"""
        cap = 2 * self.num_leaves
        out = (C.c_int * (2 * cap))()
        n = self.lib.iqhost_get_branches(self.h, out, cap)
        return [(out[2 * k], out[2 * k + 1]) for k in range(n)]

    def compute_parsimony_tree(self, order, trace=False):
        """stepwise addition by maximum parsimony in the given taxon order (computeParsimonyTree without its shuffle): the
        tree is replaced, its branch lengths come from fix_negative_branch(True) -> score, or with trace
        (score, [per step dict(branches=[(node1, node2)], scores=[...], chosen=index)])"""
        T = self.num_leaves
        od = (C.c_int * T)(*[int(x) for x in order])
        assert len(order) == T
        score = C.c_int()
        if not trace:
            self._chk(self.lib.iqhost_compute_parsimony_tree(self.h, od, C.byref(score), None, 0, None, None))
            return score.value
        cap = max(1, T * T)
        rows, chosen, n = (C.c_int * (4 * cap))(), (C.c_int * max(1, T))(), C.c_int()
        self._chk(self.lib.iqhost_compute_parsimony_tree(self.h, od, C.byref(score), rows, cap, C.byref(n), chosen))
        steps = [dict(branches=[], scores=[], chosen=chosen[s]) for s in range(max(0, T - 3))]
        for k in range(n.value):
            st = steps[rows[4 * k]]
            st["branches"].append((rows[4 * k + 1], rows[4 * k + 2]))
            st["scores"].append(rows[4 * k + 3])
        return score.value, steps

    # ---- Fitch parsimony: thin wrappers of the raw calls (include/iqhip.h "Fitch parsimony"); a status other than OK
    #      raises EngineError with its code
    def _pars_engine(self):
        self._chk(self.lib.iqhost_sync_inputs(self.h))
        return self.engine

    def pars_init(self, informative=None, nvectors=None):
        """iqhip_pars_init -> number of sites; nvectors defaults to the reference's arena, 4 * (ntaxa - 1)"""
        inf = None if informative is None else np.ascontiguousarray(informative, dtype=np.uint8)
        assert inf is None or inf.size == self.nptn
        nv = 4 * (self.num_leaves - 1) if nvectors is None else int(nvectors)
        nsites = C.c_int64()
        _echk(libiqhip().iqhip_pars_init(self._pars_engine(), None if inf is None else inf.ctypes.data_as(C.POINTER(C.c_uint8)),
                                        nv, C.byref(nsites)))
        return nsites.value

    def pars_update(self, ops):
        """iqhip_pars_update: ops = rows of (dst, left, right) slots, one launch"""
        arr, n = _pars_ops(ops)
        _echk(libiqhip().iqhip_pars_update(self._pars_engine(), arr, n))

    def pars_branch_scores(self, ends):
        """iqhip_pars_branch_scores: ends [nbranch, 2] slots -> (score[nbranch], subst[nbranch])"""
        en = np.ascontiguousarray(ends, dtype=np.int32).reshape(-1, 2)
        sc, sb = np.zeros(max(1, en.shape[0]), dtype=np.int32), np.zeros(max(1, en.shape[0]), dtype=np.int32)
        i32p = C.POINTER(C.c_int32)
        _echk(libiqhip().iqhip_pars_branch_scores(self._pars_engine(), en.ctypes.data_as(i32p), en.shape[0],
                                                 sc.ctypes.data_as(i32p), sb.ctypes.data_as(i32p)))
        return sc[:en.shape[0]], sb[:en.shape[0]]

    def pars_insert_scores(self, ends, taxon, want_scores=True):
        """iqhip_pars_insert_scores: the scan of one stepwise-addition step -> (score[nbranch] or None, best, best_score)"""
        en = np.ascontiguousarray(ends, dtype=np.int32).reshape(-1, 2)
        sc = np.zeros(max(1, en.shape[0]), dtype=np.int32) if want_scores else None
        best, bs = C.c_int32(), C.c_int32()
        i32p = C.POINTER(C.c_int32)
        _echk(libiqhip().iqhip_pars_insert_scores(self._pars_engine(), en.ctypes.data_as(i32p), en.shape[0], int(taxon),
                                                 None if sc is None else sc.ctypes.data_as(i32p), C.byref(best), C.byref(bs)))
        return (None if sc is None else sc[:en.shape[0]]), best.value, bs.value

    def pars_insert_scores_batch(self, ends, seg_start, taxa, want_scores=True):
        """iqhip_pars_insert_scores_batch: one stepwise-addition step of many trees.  ends [nbranch, 2] slots, seg_start
        [nseg + 1] offsets into the branches, taxa [nseg] tip slots -> (score[nbranch] or None, best[nseg] as indices
        within the segments, best_score[nseg])"""
        en = np.ascontiguousarray(ends, dtype=np.int32).reshape(-1, 2)
        ss = np.ascontiguousarray(seg_start, dtype=np.int32).reshape(-1)
        tx = np.ascontiguousarray(taxa, dtype=np.int32).reshape(-1)
        nseg = tx.size
        if ss.size != nseg + 1:
            raise HostError("pars_insert_scores_batch: seg_start needs one entry more than taxa")
        if nseg >= 1 and ss[-1] != en.shape[0]:
            raise HostError("pars_insert_scores_batch: seg_start must end at the number of branches")
        sc = np.zeros(max(1, en.shape[0]), dtype=np.int32) if want_scores else None
        best, bs = np.zeros(max(1, nseg), dtype=np.int32), np.zeros(max(1, nseg), dtype=np.int32)
        i32p = C.POINTER(C.c_int32)
        _echk(libiqhip().iqhip_pars_insert_scores_batch(self._pars_engine(), en.ctypes.data_as(i32p), ss.ctypes.data_as(i32p), nseg,
                                                       tx.ctypes.data_as(i32p), None if sc is None else sc.ctypes.data_as(i32p),
                                                       best.ctypes.data_as(i32p), bs.ctypes.data_as(i32p)))
        return (None if sc is None else sc[:en.shape[0]]), best[:nseg], bs[:nseg]

    def pars_batch_timing(self, reset=True):
        """iqhip_debug_pars_batch_timing -> {scan_ms, launches, branches, segments} of the batch scans since the last reset"""
        ms, ln = C.c_double(), (C.c_int64 * 3)()
        _echk(libiqhip().iqhip_debug_pars_batch_timing(self.engine, C.byref(ms), ln, int(reset)))
        return dict(scan_ms=ms.value, launches=ln[0], branches=ln[1], segments=ln[2])

    def compute_parsimony_forest(self, orders, spr_radius=0, trace=False):
        """K stepwise-addition parsimony trees built in lockstep on this tree's engine (ParsimonyForest): per step ONE
        update and ONE batch scan for all of them.  orders: K permutations of the taxa.  This tree's topology stays.
        -> [dict(newick, score, topology, spr_moves, steps)], steps as compute_parsimony_tree's trace plus best_score (None
        without trace).  The engine calls of the run are in self.forest_calls."""
        T = self.num_leaves
        od = np.ascontiguousarray(orders, dtype=np.int32).reshape(-1, T) if len(orders) else np.zeros((0, T), dtype=np.int32)
        K = od.shape[0]
        res, calls = C.c_void_p(), (C.c_int64 * 5)()
        self._chk(self.lib.iqhost_pars_forest_build(self.h, _iptr(od) if K else None, K, int(spr_radius), int(trace),
                                                    C.byref(res), calls))
        self.forest_calls = dict(updates=calls[0], scans=calls[1], branch_scores=calls[2], spr_scans=calls[3], inits=calls[4])
        out = []
        try:
            for k in range(K):
                score, spr, nrows, need = C.c_int(), C.c_int(), C.c_int(), C.c_int()
                self._chk(self.lib.iqhost_pars_forest_member(res, k, C.byref(score), C.byref(spr), C.byref(nrows), None, 0, C.byref(need)))
                buf = C.create_string_buffer(need.value)
                self._chk(self.lib.iqhost_pars_forest_member(res, k, C.byref(score), C.byref(spr), C.byref(nrows), buf, len(buf), C.byref(need)))
                newick, topology = buf.value.decode().split("\n")
                steps = None
                if trace:
                    ns = max(0, T - 3)
                    rows = (C.c_int * (4 * max(1, nrows.value)))()
                    chosen, best = (C.c_int * max(1, ns))(), (C.c_int * max(1, ns))()
                    self._chk(self.lib.iqhost_pars_forest_trace(res, k, rows, nrows.value, chosen, best, ns))
                    steps = [dict(branches=[], scores=[], chosen=chosen[s], best_score=best[s]) for s in range(ns)]
                    for q in range(nrows.value):
                        st = steps[rows[4 * q]]
                        st["branches"].append((rows[4 * q + 1], rows[4 * q + 2]))
                        st["scores"].append(rows[4 * q + 3])
                out.append(dict(newick=newick, score=score.value, topology=topology, spr_moves=spr.value, steps=steps))
        finally:
            self.lib.iqhost_pars_forest_free(res)
        return out

    def pars_fetch(self, slot):
        """iqhip_pars_fetch -> (planes[nwords, nstates] uint32 in the reference's layout, subtree score)"""
        nwords = self.pars_shape()[1]
        out = np.zeros(nwords * self.nstates + 1, dtype=np.uint32)
        _echk(libiqhip().iqhip_pars_fetch(self._pars_engine(), int(slot), out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out[:-1].reshape(nwords, self.nstates).copy(), int(out[-1])

    def pars_shape(self):
        """iqhip_pars_shape -> (nsites, nwords, nvectors) of the engine's current parsimony state, whoever initialised it"""
        ns, nw, nv = C.c_int64(), C.c_int64(), C.c_int()
        _echk(libiqhip().iqhip_pars_shape(self._pars_engine(), C.byref(ns), C.byref(nw), C.byref(nv)))
        return ns.value, nw.value, nv.value

    def pars_timing(self, reset=True):
        """iqhip_debug_pars_timing -> {update_ms, scan_ms, update_launches, scan_launches, ops, branches} since the last reset"""
        ms, ln = (C.c_double * 2)(), (C.c_int64 * 4)()
        _echk(libiqhip().iqhip_debug_pars_timing(self.engine, ms, ln, int(reset)))
        return dict(update_ms=ms[0], scan_ms=ms[1], update_launches=ln[0], scan_launches=ln[1], ops=ln[2], branches=ln[3])

    # ---- parsimony SPR search (include/iqhip.h "Parsimony SPR scan"; PhyloTree::collectSprJobs / optimizeParsimonySPR)
    def pars_spr_scan(self, jobs, steps, want_scores=True):
        """iqhip_pars_spr_scan: jobs = rows of (subtree, first_step, nsteps), steps = rows of (parent, side, target, flags)
        -> (score[nsteps] or None, best_step[njobs], best_score[njobs], best_job)"""
        jb, st = _spr_rows(jobs, "jobs"), _spr_rows(steps, "steps")
        i32p = C.POINTER(C.c_int32)
        sc = np.zeros(max(1, st.shape[0]), dtype=np.int32) if want_scores else None
        bs, bsc = np.zeros(max(1, jb.shape[0]), dtype=np.int32), np.zeros(max(1, jb.shape[0]), dtype=np.int32)
        bj = C.c_int32()
        _echk(libiqhip().iqhip_pars_spr_scan(self._pars_engine(), jb.ctypes.data_as(C.c_void_p), jb.shape[0],
                                            st.ctypes.data_as(C.c_void_p), st.shape[0], None if sc is None else sc.ctypes.data_as(i32p),
                                            bs.ctypes.data_as(i32p), bsc.ctypes.data_as(i32p), C.byref(bj)))
        return (None if sc is None else sc[:st.shape[0]]), bs[:jb.shape[0]], bsc[:jb.shape[0]], bj.value

    def collect_spr_jobs(self, radius):
        """PhyloTree::collectSprJobs -> (jobs[njobs, 4], steps[nsteps, 4], moves[nsteps, 5] = (prune, subtree, node1, node2,
        depth)): one job per internal node and neighbour, its steps the branches within `radius` of the merged branch"""
        nj, ns = C.c_int(), C.c_int()
        self._chk(self.lib.iqhost_collect_spr_jobs(self.h, int(radius), None, 0, None, None, 0, C.byref(nj), C.byref(ns)))
        jobs = np.zeros((max(1, nj.value), 4), dtype=np.int32)
        steps = np.zeros((max(1, ns.value), 4), dtype=np.int32)
        moves = np.zeros((max(1, ns.value), 5), dtype=np.int32)
        ip = C.POINTER(C.c_int)
        self._chk(self.lib.iqhost_collect_spr_jobs(self.h, int(radius), jobs.ctypes.data_as(ip), jobs.shape[0], steps.ctypes.data_as(ip),
                                                   moves.ctypes.data_as(ip), steps.shape[0], C.byref(nj), C.byref(ns)))
        return jobs[:nj.value], steps[:ns.value], moves[:ns.value]

    def apply_spr_move(self, prune, subtree, node1, node2):
        """PhyloTree::applySprMove: cut the subtree at node `subtree` off its neighbour `prune` and regraft it, with node
        `prune`, into the branch node1 -- node2"""
        self._chk(self.lib.iqhost_apply_spr_move(self.h, int(prune), int(subtree), int(node1), int(node2)))

    def optimize_parsimony_spr(self, radius=6, max_rounds=None, trace=False):
        """PhyloTree::optimizeParsimonySPR: rounds of (all vectors, one SPR scan of every prune point within `radius`, the
        best move applied) until no move lowers the score or max_rounds moves -> score, or with trace (score, [per round
        dict(score_before, job, step, score, steps_scored, move=(prune, subtree, node1, node2), applied)])"""
        score, n = C.c_int(), C.c_int()
        mr = -1 if max_rounds is None else int(max_rounds)
        if not trace:
            self._chk(self.lib.iqhost_optimize_parsimony_spr(self.h, int(radius), mr, C.byref(score), None, 0, None))
            return score.value
        cap = 4096
        rows = np.zeros((cap, 10), dtype=np.int32)
        self._chk(self.lib.iqhost_optimize_parsimony_spr(self.h, int(radius), mr, C.byref(score), rows.ctypes.data_as(C.POINTER(C.c_int)),
                                                         cap, C.byref(n)))
        if n.value > cap:
            raise HostError("optimize_parsimony_spr: more than %d rounds; only the first ones were traced" % cap)
        out = [dict(score_before=int(r[0]), job=int(r[1]), step=int(r[2]), score=int(r[3]), steps_scored=int(r[4]),
                    move=tuple(int(x) for x in r[5:9]), applied=bool(r[9])) for r in rows[:n.value]]
        return score.value, out

    def pars_spr_timing(self, reset=True):
        """iqhip_debug_pars_spr_timing -> {scan_ms, launches, steps_scored} since the last reset"""
        ms, ln = (C.c_double * 1)(), (C.c_int64 * 2)()
        _echk(libiqhip().iqhip_debug_pars_spr_timing(self.engine, ms, ln, int(reset)))
        return dict(scan_ms=ms[0], launches=ln[0], steps_scored=ln[1])

    def set_branch_bounds(self, lo, hi):
        self._chk(self.lib.iqhost_set_branch_bounds(self.h, lo, hi))

    # ---- host views
    def fetch_scale_num(self, frm, to):
        out = np.zeros(self.nptn, dtype=np.int16)
        self._chk(self.lib.iqhost_fetch_scale_num(self.h, frm, to, out.ctypes.data_as(C.POINTER(C.c_int16))))
        return out

    def fetch_partial(self, frm, to):
        out = np.zeros(self.nptn * self.block)
        self._chk(self.lib.iqhost_fetch_partial(self.h, frm, to, _dptr(out)))
        return out.reshape(self.nptn, self.block)

    def fetch_pattern_lh(self):
        out = np.zeros(self.nptn)
        self._chk(self.lib.iqhost_fetch_pattern_lh(self.h, _dptr(out)))
        return out

    def compute_pattern_likelihood(self):
        """PhyloTree::computePatternLikelihood: per-pattern lnL with the scaling events put back."""
        out = np.zeros(self.nptn)
        self._chk(self.lib.iqhost_compute_pattern_likelihood(self.h, _dptr(out)))
        return out

    def compute_pattern_lh_cat(self):
        """_pattern_lh_cat[nptn, ncat] of the current branch (unscaled category likelihoods)."""
        out = np.zeros((self.nptn, self.ncat))
        self._chk(self.lib.iqhost_compute_pattern_lh_cat(self.h, _dptr(out)))
        return out

    def em_posteriors(self):
        """One E-step of the +R EM on the current branch (iqhip_em_posteriors) -> (W[nptn, ncat], cat_sum[ncat]):
        W[p, c] = ptn_freq[p] * L_pc / sum_c L_pc, cat_sum = its column sums as the device summed them."""
        W, s = np.zeros((self.nptn, self.ncat)), np.zeros(self.ncat)
        self._chk(self.lib.iqhost_em_posteriors(self.h, _dptr(W), _dptr(s)))
        return W, s

    def em_objective(self, a, b):
        """iqhip_em_objective for the branch a -> b with the model the tree holds now, after em_posteriors()
        -> (F[ncat], floored[ncat])."""
        f, fl = np.zeros(self.ncat), np.zeros(self.ncat, dtype=np.int64)
        self._chk(self.lib.iqhost_em_objective(self.h, a, b, _dptr(f), fl.ctypes.data_as(C.POINTER(C.c_int64))))
        return f, fl

    def site_rates(self):
        """RateGamma::computePatternRates -> (posterior mean rate[nptn], best category[nptn]; ties: the first)."""
        r, c = np.zeros(self.nptn), np.zeros(self.nptn, dtype=np.int32)
        self._chk(self.lib.iqhost_site_rates(self.h, _dptr(r), c.ctypes.data_as(C.POINTER(C.c_int))))
        return r, c

    def optimize_free_rates_em(self, trace=False):
        """PhyloTree::optimizeFreeRatesEM (RateFree::optimizeWithEM with the rate searches in lockstep on the device)
        -> dict(props, rates, lnl, steps[, trace: per EM step dict(lnl_before, rounds, props, rates, evals, floored)])."""
        k = self.ncat
        props, rates, lnl, n = np.zeros(k), np.zeros(k), C.c_double(), C.c_int()
        tr = np.zeros((max(1, k), 2 + 4 * k))
        self._chk(self.lib.iqhost_optimize_free_rates_em(self.h, _dptr(props), _dptr(rates), C.byref(lnl), C.byref(n),
                                                         _dptr(tr), tr.shape[0]))
        out = dict(props=props, rates=rates, lnl=lnl.value, steps=n.value)
        if trace:
            out["trace"] = [dict(lnl_before=row[0], rounds=int(row[1]), props=row[2:2 + k].copy(), rates=row[2 + k:2 + 2 * k].copy(),
                                 evals=row[2 + 2 * k:2 + 3 * k].astype(int), floored=row[2 + 3 * k:2 + 4 * k].astype(np.int64))
                            for row in tr[:n.value]]
        return out

    def mix_class_lh(self):
        """computePatternLhCat(WSL_MIXTURE) on the current branch (iqhip_mix_class_lh) -> Lc[nptn, nclass], the sum of the
        pattern likelihoods of every class's components, unscaled; the matrix also stays on the device for the calls below."""
        out = np.zeros((self.nptn, self.nclass))
        self._chk(self.lib.iqhost_mix_class_lh(self.h, _dptr(out)))
        return out

    def mix_weights_em(self, weights, max_steps=None, p_invar=None, trace=False):
        """The EM of ModelMixture::optimizeWeights on the matrix of the last mix_class_lh() (iqhip_mix_weights_em), at most
        max_steps steps (default: nclass, as the reference); the tree and its model are left as they are
        -> dict(weights, p_invar (None without +I), steps, converged[, trace: [steps, nclass + 1] rows {w, p_invar}])."""
        k = self.nclass
        w = np.array(weights, dtype=np.float64)
        assert w.size == k
        max_steps = k if max_steps is None else int(max_steps)
        n, conv = C.c_int(), C.c_int()
        pinv = C.c_double(0.0 if p_invar is None else float(p_invar))
        tr = np.zeros((max(1, max_steps), k + 1))
        self._chk(self.lib.iqhost_mix_weights_em(self.h, max_steps, _dptr(w), None if p_invar is None else C.byref(pinv),
                                                 C.byref(n), C.byref(conv), _dptr(tr) if trace else None))
        out = dict(weights=w, p_invar=None if p_invar is None else pinv.value, steps=n.value, converged=conv.value)
        if trace:
            out["trace"] = tr[:n.value].copy()
        return out

    def mix_posteriors(self, class_freq=None):
        """Class posteriors of the matrix of the last mix_class_lh() -> post[nptn, nclass], or with class_freq[nclass, nstates]
        (post, state_freq[nptn, nstates]) as PhyloTree::computePatternStateFreq."""
        post = np.zeros((self.nptn, self.nclass))
        if class_freq is None:
            self._chk(self.lib.iqhost_mix_posteriors(self.h, None, _dptr(post), None))
            return post
        cf = np.ascontiguousarray(class_freq, dtype=np.float64)
        assert cf.shape == (self.nclass, self.nstates)
        sf = np.zeros((self.nptn, self.nstates))
        self._chk(self.lib.iqhost_mix_posteriors(self.h, _dptr(cf), _dptr(post), _dptr(sf)))
        return post, sf

    def pattern_state_freq(self, class_freq):
        """PhyloTree::computePatternStateFreq on the current branch: the class likelihoods are rebuilt (as mix_class_lh()), then
        state_freq[nptn, nstates] = sum_m class_freq[m] * posterior of class m."""
        cf = np.ascontiguousarray(class_freq, dtype=np.float64)
        assert cf.shape == (self.nclass, self.nstates)
        sf = np.zeros((self.nptn, self.nstates))
        self._chk(self.lib.iqhost_pattern_state_freq(self.h, _dptr(cf), _dptr(sf)))
        return sf

    def optimize_mixture_weights(self, p_invar=None):
        """ModelMixture::optimizeWeights: class likelihoods on the current branch, the EM with nclass steps, the component
        weights (and with +I ptn_invar) rescaled and re-sent, all vectors cleared
        -> dict(weights, props, p_invar, lnl, steps, converged)."""
        w, props, lnl, n, conv = np.zeros(self.nclass), np.zeros(self.ncat), C.c_double(), C.c_int(), C.c_int()
        pinv = C.c_double(0.0 if p_invar is None else float(p_invar))
        self._chk(self.lib.iqhost_optimize_mixture_weights(self.h, None if p_invar is None else C.byref(pinv), _dptr(w),
                                                           _dptr(props), C.byref(lnl), C.byref(n), C.byref(conv)))
        return dict(weights=w, props=props, p_invar=None if p_invar is None else pinv.value, lnl=lnl.value, steps=n.value,
                    converged=conv.value)

    def mix_timing(self):
        """iqhip_debug_mix_timing -> dict(class_lh_ms, em_ms, launches) of the last calls (times while timing is enabled)."""
        ms, n = np.zeros(2), C.c_int64()
        self._chk(self.lib.iqhost_mix_timing(self.h, _dptr(ms), C.byref(n)))
        return dict(class_lh_ms=ms[0], em_ms=ms[1], launches=n.value)

    def class_lnl(self, a, b, class_weight, class_invar=None):
        """iqhip_class_lnl for the branch a -> b (theta is rebuilt): the log-likelihood of every class's model alone on this
        tree, K candidate models as the K classes of the mixture the tree holds.  class_weight[nclass]: the weight folded
        into each class's props (1 for candidates); class_invar: None (the resident ptn_invar for every class) or
        [nclass, nptn] -> (lnl[nclass], floored[nclass])."""
        k = self.nclass
        w = np.ascontiguousarray(class_weight, dtype=np.float64)
        assert w.shape == (k,)
        inv = None
        if class_invar is not None:
            inv = np.ascontiguousarray(class_invar, dtype=np.float64)
            assert inv.shape == (k, self.nptn)
        lnl, fl = np.zeros(k), np.zeros(k, dtype=np.int64)
        self._chk(self.lib.iqhost_class_lnl(self.h, a, b, _dptr(w), None if inv is None else _dptr(inv), _dptr(lnl),
                                            fl.ctypes.data_as(C.POINTER(C.c_int64))))
        return lnl, fl

    def class_lnl_timing(self):
        """iqhip_debug_class_lnl_timing -> the device time (ms) of the last class_lnl() launches (while timing is enabled)."""
        ms = C.c_double()
        self._chk(self.lib.iqhost_class_lnl_timing(self.h, C.byref(ms)))
        return ms.value

    # ---- ultrafast bootstrap bookkeeping (include/iqhip.h "ultrafast bootstrap")
    def ufboot_init(self, nsamples, seed=0):
        """iqhip_ufboot_init on the first nsamples rows of the sample matrix; seed: the tie draws of save_current_tree /
        save_nni_trees"""
        self._chk(self.lib.iqhost_ufboot_init(self.h, int(nsamples), int(seed)))
        self._ufboot = int(nsamples)

    def ufboot_update(self, rows, tree_ids, logl, rand, epsilon=0.5, logl_cutoff=0.0):
        """iqhip_ufboot_update: one entry per candidate tree, applied in list order ->
        (counts = [applied, dropped by the cutoff, replicate slots replaced], min_orig_logl)"""
        r = np.ascontiguousarray(rows, dtype=np.int32).ravel()
        ids = np.ascontiguousarray(tree_ids, dtype=np.int64).ravel()
        l = np.ascontiguousarray(logl, dtype=np.float64).ravel()
        u = np.ascontiguousarray(rand, dtype=np.float64).ravel()
        assert r.size == ids.size == l.size == u.size
        ent = (UFBootTree * max(r.size, 1))()
        for k in range(r.size):
            ent[k] = UFBootTree(int(r[k]), 0, int(ids[k]), float(l[k]), float(u[k]))
        counts = np.zeros(3, dtype=np.int64)
        mn = C.c_double()
        _echk(libiqhip().iqhip_ufboot_update(self.engine, ent, r.size, float(epsilon), float(logl_cutoff),
                                             counts.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(mn)))
        return counts, mn.value

    def ufboot_state(self):
        """iqhip_ufboot_fetch -> dict(boot_logl, boot_orig_logl, boot_counts, boot_tree), nsamples entries each"""
        n = self._ufboot
        st = dict(boot_logl=np.zeros(n), boot_orig_logl=np.zeros(n), boot_counts=np.zeros(n, dtype=np.int32),
                  boot_tree=np.zeros(n, dtype=np.int64))
        _echk(libiqhip().iqhip_ufboot_fetch(self.engine, _dptr(st["boot_logl"]), _dptr(st["boot_orig_logl"]),
                                            st["boot_counts"].ctypes.data_as(C.POINTER(C.c_int32)),
                                            st["boot_tree"].ctypes.data_as(C.POINTER(C.c_int64))))
        return st

    def ufboot_timing(self):
        """(device ms of the products, of the update kernels, kernels enqueued) of the last ufboot_update"""
        ms = np.zeros(2)
        n = C.c_int64()
        _echk(libiqhip().iqhip_debug_ufboot_timing(self.engine, _dptr(ms), C.byref(n)))
        return float(ms[0]), float(ms[1]), int(n.value)

    def ufboot_params(self, epsilon=0.5, logl_cutoff=0.0):
        """params.ufboot_epsilon and logl_cutoff of the following save_current_tree / save_nni_trees calls"""
        self._chk(self.lib.iqhost_ufboot_params(self.h, float(epsilon), float(logl_cutoff)))

    def ufboot_next_iteration(self):
        """the start of a search iteration (iqtree.cpp:1887-1888): logl_cutoff = min boot_orig_logl"""
        self._chk(self.lib.iqhost_ufboot_next_iteration(self.h))

    def ufboot_info(self):
        info = np.zeros(2, dtype=np.int64)
        vals = np.zeros(2)
        self._chk(self.lib.iqhost_ufboot_info(self.h, info.ctypes.data_as(C.POINTER(C.c_int64)), _dptr(vals)))
        return dict(trees_fed=int(info[0]), trees_kept=int(info[1]), logl_cutoff=float(vals[0]), min_orig_logl=float(vals[1]))

    def save_current_tree(self, logl):
        """IQTree::saveCurrentTree(logl) for the tree of the last compute_likelihood -> (counts, min_orig_logl)"""
        counts = np.zeros(3, dtype=np.int64)
        mn = C.c_double()
        self._chk(self.lib.iqhost_save_current_tree(self.h, float(logl), counts.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(mn)))
        return counts, mn.value

    def save_nni_trees(self):
        """all 2(n-3) NNI neighbours (evaluate_nnis5_batch with store rows) through ONE update -> (counts, min_orig_logl)"""
        counts = np.zeros(3, dtype=np.int64)
        mn = C.c_double()
        self._chk(self.lib.iqhost_save_nni_trees(self.h, counts.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(mn)))
        return counts, mn.value

    def sorted_taxon_id_string(self):
        """the topology as the reference prints it with WT_TAXON_ID + WT_SORT_TAXA"""
        need = C.c_int()
        self._chk(self.lib.iqhost_sorted_taxon_id_string(self.h, None, 0, C.byref(need)))
        buf = C.create_string_buffer(need.value)
        self._chk(self.lib.iqhost_sorted_taxon_id_string(self.h, buf, len(buf), C.byref(need)))
        return buf.value.decode()

    def summarize_bootstrap(self):
        """summarizeBootstrap -> dict(support_tree, supports = [(node1, node2, percent)], consensus_tree, boot_trees =
        the winner of every replicate (taxon ids, taxa sorted), distinct_trees)"""
        cap = self.num_nodes
        ids = np.zeros(2 * cap, dtype=np.int32)
        sup = np.zeros(cap, dtype=np.int32)
        n, distinct, need = C.c_int(), C.c_int(), C.c_int()
        ip = C.POINTER(C.c_int)
        self._chk(self.lib.iqhost_summarize_bootstrap(self.h, ids.ctypes.data_as(ip), sup.ctypes.data_as(ip), cap, C.byref(n),
                                                      C.byref(distinct), None, 0, C.byref(need)))
        buf = C.create_string_buffer(need.value)
        self._chk(self.lib.iqhost_summarize_bootstrap(self.h, ids.ctypes.data_as(ip), sup.ctypes.data_as(ip), cap, C.byref(n),
                                                      C.byref(distinct), buf, len(buf), C.byref(need)))
        lines = buf.value.decode().split("\n")
        return dict(support_tree=lines[0], consensus_tree=lines[1], boot_trees=lines[2:2 + self._ufboot],
                    supports=[(int(ids[2 * q]), int(ids[2 * q + 1]), int(sup[q])) for q in range(n.value)],
                    distinct_trees=distinct.value)

    def set_boot_samples(self, samples):
        """UFBoot boot_samples: float32 [nsamples, nptn] pattern weights, uploaded once."""
        s = np.ascontiguousarray(samples, dtype=np.float32)
        assert s.ndim == 2 and s.shape[1] == self.nptn
        self._nboot = s.shape[0]
        self._chk(self.lib.iqhost_set_boot_samples(self.h, s.ctypes.data_as(C.POINTER(C.c_float)), s.shape[0]))

    def compute_rell(self):
        out = np.zeros(self._nboot)
        self._chk(self.lib.iqhost_compute_rell(self.h, _dptr(out), out.size))
        return out

    def last_plan(self):
        cap = 4 * self.num_nodes + 8
        ints = (C.c_int * (7 * cap))()
        lens = (C.c_double * (2 * cap))()
        keys = (C.c_uint64 * (3 * cap))()
        n = self.lib.iqhost_last_plan(self.h, ints, lens, keys, cap)
        plan = []
        for k in range(n):
            plan.append(dict(dst=(ints[7 * k], ints[7 * k + 1]), left=ints[7 * k + 2], right=ints[7 * k + 3],
                             left_leaf=ints[7 * k + 4], right_leaf=ints[7 * k + 5], flags=ints[7 * k + 6],
                             left_len=lens[2 * k], right_len=lens[2 * k + 1],
                             dst_key=keys[3 * k], left_key=keys[3 * k + 1], right_key=keys[3 * k + 2]))
        return plan

    @property
    def num_partial_lh_computations(self):
        return self.lib.iqhost_num_partial_lh_computations(self.h)

    @property
    def num_submissions(self):
        return self.lib.iqhost_num_submissions(self.h)


def _trace_move(m):
    return dict(node1=m[0], node2=m[1], node1_nei=m[2], node2_nei=m[3], newloglh=m[4], new_lens=m[5:10])


def _trace_steps(steps):
    for st in steps:
        st["branches"] = [tuple(b) for b in st["branches"]]
        for key in ("evaluated", "positive", "applied"):
            st[key] = [_trace_move(m) for m in st[key]]
    return steps


class TreeSearch:
    """The NNI tree search on a PhyloTree with an attached engine (iq-tree_amd/host/tree_search_host.h): optimizeNNI and
    the stochastic loop of doTreeSearch.  iterations: a fixed number of search iterations after the starting tree's
    (SC_FIXED_ITERATION); None: stop after num_stop iterations without a better tree.  With tree.ufboot_init done before,
    every evaluated tree feeds the bootstrap and the correlation rule applies: every step_iterations iterations the split
    frequencies of the bootstrap winners are correlated (correlation_log); the search ends when the correlation reaches
    min_correlation and num_stop iterations brought no better tree, or after max_iterations (with `iterations` given: after
    min(iterations, max_iterations)).
    num_init_trees > 0: the reference's initCandidateTreeSet first -- the given tree plus num_init_trees - 1 parsimony trees
    built in lockstep on the orders of parsimony_orders(seed, ...) (with init_spr_radius > 0 followed by SPR rounds),
    duplicate topologies dropped (init_duplicates), each scored with optimize_all_branches(2) (init_trees), the best
    num_nni_trees optimised by NNI as the iterations 1 .. M; `iterations` counts the iterations after those (with UFBoot it
    caps max_iterations, which counts every iteration, as in the reference)."""

    def __init__(self, tree, seed=0, nni5=True, speed=True, pop_size=5, pers=0.5, iterations=None, num_stop=100, batched=True,
                 step_iterations=100, min_correlation=0.99, max_iterations=1000, num_init_trees=0, num_nni_trees=20,
                 init_spr_radius=0):
        self.lib = libiqhost()
        self.tree = tree
        self.h = C.c_void_p()
        if isinstance(tree, PhyloSuperTree):   # num_init_trees > 0 is refused; UFBoot: tree.ufboot_init (the group's state)
            _hchk(self.lib.iqhost_search_create_super(C.byref(self.h), tree.h))
        else:
            _hchk(self.lib.iqhost_search_create(C.byref(self.h), tree.h))
        self.params = dict(seed=seed, nni5=nni5, speed=speed, pop_size=pop_size, pers=pers, iterations=iterations,
                           num_stop=num_stop, batched=batched, step_iterations=step_iterations,
                           min_correlation=min_correlation, max_iterations=max_iterations, num_init_trees=num_init_trees,
                           num_nni_trees=num_nni_trees, init_spr_radius=init_spr_radius)
        self.init_trees = []        # after search(): [(score, tree, topology)] of the distinct starting trees, in generation order
        self.init_duplicates = 0    # parsimony trees that repeated an earlier topology
        self.best_score = None
        self.correlation_log = []
        self._trace = None

    def close(self):
        if self.h:
            self.lib.iqhost_search_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _set_params(self, trace):
        p = self.params
        boot = getattr(self.tree, "_ufboot", 0) > 0
        if p["iterations"] is not None and int(p["iterations"]) < 0:
            raise HostError("TreeSearch: iterations must be >= 0")
        if boot:   # the correlation rule; a fixed iteration count caps it
            cond = SC_BOOTSTRAP_CORRELATION
            max_it = p["max_iterations"] if p["iterations"] is None else min(p["max_iterations"], int(p["iterations"]))
        else:
            cond = SC_UNSUCCESS_ITERATION if p["iterations"] is None else SC_FIXED_ITERATION
            max_it = p["max_iterations"]
        iv = np.array([p["nni5"], p["speed"], p["batched"], p["pop_size"], cond,
                       int(p["iterations"] or 0), p["num_stop"], max_it, p["step_iterations"], trace,
                       p["num_init_trees"], p["num_nni_trees"], p["init_spr_radius"]], dtype=np.int32)
        dv = np.array([p["pers"], p["min_correlation"]], dtype=np.float64)
        _hchk(self.lib.iqhost_search_set_params(self.h, _iptr(iv), _dptr(dv), int(p["seed"])))

    def _fetch_trace(self):
        need = C.c_int()
        _hchk(self.lib.iqhost_search_trace_json(self.h, None, 0, C.byref(need)))
        buf = C.create_string_buffer(need.value)
        _hchk(self.lib.iqhost_search_trace_json(self.h, buf, len(buf), C.byref(need)))
        import json
        t = json.loads(buf.value.decode())
        _trace_steps(t["nni_steps"])
        for it in t["iterations"]:
            _trace_steps(it["steps"])
            it["random_nnis"] = [tuple(x) for x in it["random_nnis"]]
        t["boot_splits"] = [{frozenset(s): w for s, w in snap} for snap in t["boot_splits"]]
        return t

    def optimize_nni(self, trace=False):
        """compute_likelihood(), then optimizeNNI on the tree -> (lnL, NNIs applied, steps[, per-step trace])"""
        self._set_params(trace)
        lnl, cnt, steps = C.c_double(), C.c_int(), C.c_int()
        _hchk(self.lib.iqhost_search_optimize_nni(self.h, C.byref(lnl), C.byref(cnt), C.byref(steps)))
        if trace:
            return lnl.value, cnt.value, steps.value, self._fetch_trace()["nni_steps"]
        return lnl.value, cnt.value, steps.value

    def do_random_nnis(self, num_nni, iteration):
        """doRandomNNIs with the draws of `iteration` -> [(node1, node2, bit1, bit2)]; all vectors go stale"""
        self._set_params(False)
        out = np.zeros(4 * max(int(num_nni), 1), dtype=np.int32)
        n = C.c_int()
        _hchk(self.lib.iqhost_search_do_random_nnis(self.h, int(num_nni), int(iteration), _iptr(out), int(num_nni), C.byref(n)))
        return [tuple(int(x) for x in out[4 * k:4 * k + 4]) for k in range(n.value)]

    def search(self, trace=False):
        """doTreeSearch -> the best score (with trace: (best score, [per iteration dict(iteration, parent, random_nnis,
        perturb_score, steps, score, new_best, nni_count)])); the best tree is loaded into the PhyloTree"""
        self._set_params(trace)
        best = C.c_double()
        _hchk(self.lib.iqhost_search_do_tree_search(self.h, C.byref(best)))
        self.best_score = best.value
        t = self._fetch_trace()
        self._trace = t
        self.correlation_log = [(int(i), float(c)) for i, c in t["correlation_log"]]
        self.boot_splits = t["boot_splits"]
        self._candidates = [(c[0], c[1], c[2]) for c in t["candidates"]]
        self.init_trees = [(c[0], c[1], c[2]) for c in t["init_trees"]]
        self.init_duplicates = int(t["init_duplicates"])
        return (best.value, t["iterations"]) if trace else best.value

    def candidates(self):
        """the candidate set after search(): [(score, tree, topology)], the best first"""
        return list(self._candidates)


# ---------------------------------------------------------------------------------------------
# model / alignment producers: C++ in iq-tree_amd/host/{model,alignment}_host.cpp
# ---------------------------------------------------------------------------------------------

class PartitionGroup:
    """A group of engines, one per partition of an edge-linked partition model (iqhip_partition_*, include/iqhip.h).
    `members`: PhyloTree objects with attached engines, or raw engine handles.  The group owns nothing of them."""

    def __init__(self, members):
        self.lib = libiqhip()
        self.members = list(members)
        handles = [m.engine if isinstance(m, PhyloTree) else m for m in self.members]
        self.nparts = len(handles)
        arr = (C.c_void_p * max(1, self.nparts))(*handles)
        self.h = C.c_void_p()
        self._chk(self.lib.iqhip_partition_create(C.byref(self.h), arr, self.nparts))

    def _chk(self, rc):
        if rc != 0:
            raise EngineError(rc, self.lib.iqhip_last_error().decode())

    def close(self):
        if getattr(self, "h", None) is not None and self.h.value:
            self.lib.iqhip_partition_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_rates(self, rates):
        r = np.ascontiguousarray(rates, dtype=np.float64)
        if r.shape != (self.nparts,):
            raise ValueError("one rate per member")
        self._chk(self.lib.iqhip_partition_set_rates(self.h, r.ctypes.data_as(C.POINTER(C.c_double))))

    def newton_branch(self, xguess, x1, x2, xacc, max_steps, want_lnl=True):
        """-> (optx, d2l, derivative evaluations, part_lnl or None)"""
        optx, d2l, ns = C.c_double(), C.c_double(), C.c_int()
        out = np.zeros(self.nparts) if want_lnl else None
        self._chk(self.lib.iqhip_partition_newton_branch(
            self.h, xguess, x1, x2, xacc, max_steps, C.byref(optx), C.byref(d2l), C.byref(ns),
            out.ctypes.data_as(C.POINTER(C.c_double)) if want_lnl else None))
        return optx.value, d2l.value, ns.value, out

    def lnl_from_theta(self, x):
        out = np.zeros(self.nparts)
        self._chk(self.lib.iqhip_partition_lnl_from_theta(self.h, x, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def traverse_lnl(self, ops, a, b, length, scale=None):
        """ops: a ctypes array of NodeOp (or None); a, b: BranchEnd; -> part_lnl"""
        out = np.zeros(self.nparts)
        sc = None if scale is None else np.ascontiguousarray(scale, dtype=np.float64)
        self._chk(self.lib.iqhip_partition_traverse_lnl(
            self.h, ops, 0 if ops is None else len(ops), a, b, length,
            None if sc is None else sc.ctypes.data_as(C.POINTER(C.c_double)), out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def optimize_branch_batch(self, tasks, want_part_lnl=True, rows=None):
        """tasks: a ctypes array of BranchTask (their ops arrays must stay alive for the call), or a list of them;
        rows (optional, one per task; < 0: none): the row of every member's per-pattern store that takes the task's values
        (iqhip_partition_optimize_branch_batch_rows);
        -> (results, part_lnl): a list of dicts {optx, d2l, lnl, nsteps, status} and an array [task][member] or None"""
        if tasks is not None and not isinstance(tasks, C.Array):
            tasks = (BranchTask * max(1, len(tasks)))(*tasks) if len(tasks) else None
        n = 0 if tasks is None else len(tasks)
        res = (BranchResult * max(1, n))()
        out = np.zeros((max(1, n), self.nparts)) if want_part_lnl else None
        outp = out.ctypes.data_as(C.POINTER(C.c_double)) if want_part_lnl else None
        if rows is None:
            self._chk(self.lib.iqhip_partition_optimize_branch_batch(self.h, tasks, n, res, outp))
        else:
            r = np.ascontiguousarray(rows, dtype=np.int32)
            if r.shape != (n,):
                raise ValueError("one row per task")
            self._chk(self.lib.iqhip_partition_optimize_branch_batch_rows(self.h, tasks, n, res, outp, _iptr(r)))
        results = [dict(optx=r.optx, d2l=r.d2l, lnl=r.lnl, nsteps=r.nsteps, status=r.status) for r in res[:n]]
        return results, out

    def pair_distances(self, init=None, x1=1e-6, x2=9.0, xacc=1e-6, max_steps=100, ntaxa=None):
        """iqhip_partition_pair_distances: every pair of taxa solved jointly over the members at the group's rates
        -> (dist, d2l, nsteps), each [ntaxa, ntaxa] symmetric.  init: None or [ntaxa, ntaxa], 0 = the pooled JC start; a start
        of exactly 9 is returned without a solve.  ntaxa: the members' taxon count (taken from a PhyloTree member if None)."""
        n = int(ntaxa if ntaxa is not None else self.members[0].num_leaves)
        dist, d2l, ns = np.zeros((n, n)), np.zeros((n, n)), np.zeros((n, n), dtype=np.int32)
        ini = None if init is None else np.ascontiguousarray(init, dtype=np.float64)
        if ini is not None and ini.shape != (n, n):
            raise ValueError("init must be [ntaxa, ntaxa]")
        self._chk(self.lib.iqhip_partition_pair_distances(self.h, None if ini is None else _dptr(ini), x1, x2, xacc, max_steps,
                                                          _dptr(dist), _dptr(d2l), _iptr(ns)))
        return dist, d2l, ns

    def pair_timing(self):
        """iqhip_debug_partition_pair_timing -> (device ms of the members' count launches, of the solve launches) of the last
        pair_distances (0 unless timing is enabled on member 0)"""
        return _group_pair_timing(self.lib, self.h)

    def timing(self):
        """-> {"derv_ms", "update_ms", "launches"} of the last call (the times need iqhip_timing_enable on member 0)"""
        ms = (C.c_double * 2)()
        n = C.c_int64()
        self._chk(self.lib.iqhip_debug_partition_timing(self.h, ms, C.byref(n)))
        return {"derv_ms": ms[0], "update_ms": ms[1], "launches": n.value}

    # ---- per-pattern rows, RELL sums and UFBoot of the group: row r is row r of every member's store, every member keeps
    #      its own sample matrix (set_boot_samples / gen_boot_samples on the member)
    def ptnlh_reserve(self, nrows):
        self._chk(self.lib.iqhip_partition_ptnlh_reserve(self.h, int(nrows)))

    def ptnlh_rell(self, rows, nsamples):
        """-> [len(rows), nsamples]: the members' RELL sums added in member order"""
        return _group_ptnlh_rell(self.lib, self.h, rows, nsamples)

    def ufboot_init(self, nsamples):
        self._chk(self.lib.iqhip_partition_ufboot_init(self.h, int(nsamples)))
        self._ufboot = int(nsamples)

    def ufboot_update(self, rows, tree_ids, logl, rand, epsilon=0.5, logl_cutoff=0.0):
        """iqhip_partition_ufboot_update -> as PhyloTree.ufboot_update"""
        return _group_ufboot_update(self.lib, self.h, rows, tree_ids, logl, rand, epsilon, logl_cutoff)

    def ufboot_state(self):
        """iqhip_partition_ufboot_fetch -> dict(boot_logl, boot_orig_logl, boot_counts, boot_tree)"""
        return _group_ufboot_state(self.lib, self.h, getattr(self, "_ufboot", 0))

    def ufboot_timing(self):
        """(device ms of the members' products, of the update kernels, kernels enqueued) of the last ufboot_update"""
        return _group_ufboot_timing(self.lib, self.h)


def _gchk(lib, rc):
    if rc != 0:
        raise EngineError(rc, lib.iqhip_last_error().decode())


def _group_ptnlh_rell(lib, g, rows, nsamples):
    r = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1)
    out = np.zeros((max(1, r.size), max(1, int(nsamples))))
    _gchk(lib, lib.iqhip_partition_ptnlh_rell(g, _iptr(r), r.size, int(nsamples), _dptr(out)))
    return out[:r.size, :int(nsamples)]


def _group_ufboot_update(lib, g, rows, tree_ids, logl, rand, epsilon, logl_cutoff):
    r = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1)
    assert r.size == len(tree_ids) == len(logl) == len(rand)
    ent = (UFBootTree * max(1, r.size))()
    for k in range(r.size):
        ent[k] = UFBootTree(int(r[k]), 0, int(tree_ids[k]), float(logl[k]), float(rand[k]))
    counts = np.zeros(3, dtype=np.int64)
    mn = C.c_double()
    _gchk(lib, lib.iqhip_partition_ufboot_update(g, ent, r.size, float(epsilon), float(logl_cutoff),
                                                 counts.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(mn)))
    return counts, mn.value


def _group_ufboot_state(lib, g, n):
    n = max(1, int(n))
    st = dict(boot_logl=np.zeros(n), boot_orig_logl=np.zeros(n), boot_counts=np.zeros(n, dtype=np.int32),
              boot_tree=np.zeros(n, dtype=np.int64))
    _gchk(lib, lib.iqhip_partition_ufboot_fetch(g, _dptr(st["boot_logl"]), _dptr(st["boot_orig_logl"]), _iptr(st["boot_counts"]),
                                                st["boot_tree"].ctypes.data_as(C.POINTER(C.c_int64))))
    return st


def _group_ufboot_timing(lib, g):
    ms = (C.c_double * 2)()
    n = C.c_int64()
    _gchk(lib, lib.iqhip_debug_partition_ufboot_timing(g, ms, C.byref(n)))
    return ms[0], ms[1], n.value


def _group_pair_timing(lib, g):
    a, b = C.c_double(), C.c_double()
    _gchk(lib, lib.iqhip_debug_partition_pair_timing(g, C.byref(a), C.byref(b)))
    return a.value, b.value


def parse_partition_spec(text, nsite):
    """RAxML-style partition file text (host/partition_spec.h) -> [(model string verbatim, name, [0-based sites])]"""
    lib = libiqhost()
    h = C.c_void_p()
    _mchk(lib, lib.iqpart_spec_parse(C.byref(h), text.encode(), int(nsite)))
    try:
        out = []
        for k in range(lib.iqpart_spec_count(h)):
            sites = (C.c_int * lib.iqpart_spec_nsites(h, k))()
            _mchk(lib, lib.iqpart_spec_sites(h, k, sites))
            out.append((lib.iqpart_spec_model(h, k).decode(), lib.iqpart_spec_name(h, k).decode(), list(sites)))
        return out
    finally:
        lib.iqpart_spec_free(h)


def read_partition_file(aln, path, aln_content=None, part_content=None):
    """One alignment file + a RAxML-style partition file `MODEL, name = 1-100, 250-400, 401-500\\3` (readPartitionRaxml):
    -> (sequence names, parts), one dict per partition ready for PhyloSuperTree: name, model_string, alignment (an
    Alignment), nstates, seq_type, pat, freq, invar, model, nsite.  Every taxon is kept (all-unknown rows)."""
    lib = libiqhost()
    h = C.c_void_p()
    if aln_content is not None:
        _mchk(lib, lib.iqpart_read(C.byref(h), None, aln_content.encode(), None, part_content.encode()))
    else:
        _mchk(lib, lib.iqpart_read(C.byref(h), str(aln).encode(), None, str(path).encode(), None))
    try:
        parts, names = [], None
        for k in range(lib.iqpart_count(h)):
            a = Alignment.__new__(Alignment)
            a.lib, a.h, a.n_unobserved = lib, C.c_void_p(), 0
            _mchk(lib, lib.iqpart_alignment(h, k, C.byref(a.h)))
            ms = lib.iqpart_model(h, k).decode()
            model = a.build_model(ms)
            pat, freq, _, _ = a.arrays()
            names = a.seq_names
            parts.append(dict(name=lib.iqpart_name(h, k).decode(), model_string=ms, alignment=a, nstates=a.nstates,
                              seq_type=a.seq_type, pat=pat, freq=freq, invar=a.ptn_invar(model.p_invar, model.state_freq),
                              model=model, nsite=a.nsite))
        return names, parts
    finally:
        lib.iqpart_free(h)


class _MemberTree(PhyloTree):
    """a PhyloTree owned by a PhyloSuperTree: every method works, destruction is the super tree's"""

    def __init__(self, handle):
        self.lib = libiqhost()
        self.h = handle
        self.nptn = 0
        self.block = 0

    def close(self):
        self.h = C.c_void_p()


class PhyloSuperTree:
    """Edge-linked partition model (-q / -spp; host/supertree_host.h): P trees of the super tree's topology, member p's
    lengths the super tree's times part_rates[p].  parts: dicts with nstates, seq_type, pat, freq, model and optionally
    invar, name.  Every member keeps every taxon (all-unknown rows where a partition has no data)."""

    def __init__(self, newick, parts, names=None, device=0, fixed_rates=True, attach=True, all_branch=False):
        self.lib = libiqhost()
        self.h = C.c_void_p()
        if names:
            arr = (C.c_char_p * len(names))(*[n.encode() for n in names])
            rc = self.lib.iqhost_super_create(C.byref(self.h), newick.encode(), arr, len(names))
        else:
            rc = self.lib.iqhost_super_create(C.byref(self.h), newick.encode(), None, 0)
        self._chk(rc)
        self.members = []
        for k, d in enumerate(parts):
            mh = C.c_void_p()
            self._chk(self.lib.iqhost_super_add_partition(self.h, str(d.get("name", "part%d" % (k + 1))).encode(), C.byref(mh)))
            t = _MemberTree(mh)
            t.set_alignment(d["nstates"] if "nstates" in d else d["n"], d["seq_type"], d["pat"], d["freq"], d.get("invar"))
            t.set_model(d["model"])
            self.members.append(t)
        self.nparts = len(self.members)
        self.nsites = [float(np.sum(d["freq"])) for d in parts]
        self._chk(self.lib.iqhost_super_set_fixed_rates(self.h, int(fixed_rates)))
        if all_branch:   # a buffer per directed vector on every member: what the batched NNI evaluations need
            self._chk(self.lib.iqhost_super_set_all_branch_mode(self.h))
        if attach:
            self._chk(self.lib.iqhost_super_attach_engines(self.h, device))

    def _chk(self, rc):
        if rc != 0:
            raise HostError(self.lib.iqhost_last_error().decode())

    def close(self):
        if self.h:
            for t in self.members:
                t.close()
            self.lib.iqhost_super_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def part_rates(self):
        out = np.zeros(self.nparts)
        self._chk(self.lib.iqhost_super_get_rates(self.h, _dptr(out)))
        return out

    @part_rates.setter
    def part_rates(self, rates):
        r = np.ascontiguousarray(rates, dtype=np.float64)
        if r.shape != (self.nparts,):
            raise ValueError("one rate per partition")
        self._chk(self.lib.iqhost_super_set_rates(self.h, _dptr(r)))

    def set_fixed_rates(self, on=True):
        self._chk(self.lib.iqhost_super_set_fixed_rates(self.h, int(on)))

    def set_branch_bounds(self, lo, hi):
        self._chk(self.lib.iqhost_super_set_branch_bounds(self.h, lo, hi))

    def part_lnl(self):
        """every member's log-likelihood as of the last call (part_info[part].cur_score)"""
        out = np.zeros(self.nparts)
        self._chk(self.lib.iqhost_super_part_lnl(self.h, _dptr(out)))
        return out

    def compute_likelihood(self):
        v = C.c_double()
        self._chk(self.lib.iqhost_super_compute_likelihood(self.h, C.byref(v)))
        return v.value

    def optimize_one_branch(self, a, b, clear_lh=True, max_nr_step=100):
        v = C.c_double()
        self._chk(self.lib.iqhost_super_optimize_one_branch(self.h, a, b, int(clear_lh), max_nr_step, C.byref(v)))
        return v.value

    def optimize_all_branches(self, iterations=100, tolerance=0.001, max_nr_step=100):
        v = C.c_double()
        self._chk(self.lib.iqhost_super_optimize_all_branches(self.h, iterations, tolerance, max_nr_step, C.byref(v)))
        return v.value

    def optimize_gene_rates(self, gradient_epsilon=0.001):
        """-> dict(lnl, rates, evals per member, rounds = group traversals)"""
        v, rounds = C.c_double(), C.c_int()
        evals = (C.c_int * self.nparts)()
        self._chk(self.lib.iqhost_super_optimize_gene_rates(self.h, gradient_epsilon, C.byref(v), evals, C.byref(rounds)))
        return dict(lnl=v.value, rates=self.part_rates, evals=list(evals), rounds=rounds.value)

    def optimize_parameters(self, fixed_len=False, logl_epsilon=0.001, gradient_epsilon=0.001):
        v = C.c_double()
        self._chk(self.lib.iqhost_super_optimize_parameters(self.h, int(fixed_len), logl_epsilon, gradient_epsilon, C.byref(v)))
        return v.value

    def partition_newton_branch(self, a, b, xguess, x1, x2, xacc, max_steps):
        """theta of (a, b) on every member, then iqhip_partition_newton_branch -> (optx, d2l, evaluations, part_lnl)"""
        optx, d2l, ns = C.c_double(), C.c_double(), C.c_int()
        out = np.zeros(self.nparts)
        self._chk(self.lib.iqhost_super_newton_branch(self.h, a, b, xguess, x1, x2, xacc, max_steps, C.byref(optx), C.byref(d2l),
                                                      C.byref(ns), _dptr(out)))
        return optx.value, d2l.value, ns.value, out

    def branch_length(self, a, b):
        v = C.c_double()
        self._chk(self.lib.iqhost_super_branch_length(self.h, a, b, C.byref(v)))
        return v.value

    def branch_order(self):
        """the branches in optimize_all_branches' order"""
        cap = 4 * self.members[0].num_nodes
        n1, n2 = (C.c_int * cap)(), (C.c_int * cap)()
        n = self.lib.iqhost_super_branch_order(self.h, n1, n2, cap)
        if n < 0:
            raise HostError(self.lib.iqhost_last_error().decode())
        return [(n1[k], n2[k]) for k in range(n)]

    def tree_string(self):
        buf = C.create_string_buffer(1 << 20)
        self._chk(self.lib.iqhost_super_tree_string(self.h, buf, len(buf)))
        return buf.value.decode()

    def counters(self):
        out = (C.c_long * 3)()
        self.lib.iqhost_super_counters(self.h, out)
        return dict(group_solves=out[0], group_traversals=out[1], diverged=out[2],
                    group_batches=self.lib.iqhost_super_group_batches(self.h))

    # ---- NNI on the super tree: the plain tree's surface (PhyloTree above), moves and lengths in super-tree units
    @property
    def num_nodes(self):
        return self.lib.iqhost_super_num_nodes(self.h)

    @property
    def num_leaves(self):
        return self.lib.iqhost_super_num_leaves(self.h)

    def neighbors(self, node):
        ids = (C.c_int * 8)()
        lens = (C.c_double * 8)()
        d = self.lib.iqhost_super_neighbors(self.h, node, ids, lens, 8)
        return [(ids[i], lens[i]) for i in range(d)]

    def nni_for_branch(self, a, b, nni5=False, first_row=None):
        """the branch-by-branch path: both swaps made on every tree, joint optimize_one_branch solves, the summed lnL ->
        [(newloglh, swapped subtree at a, swapped subtree at b, [newLen...]), x2]; first_row: the two neighbours'
        per-pattern values are kept in rows first_row, first_row + 1 of every member's store (ptnlh_fetch)"""
        out = np.zeros(16)
        self._chk(self.lib.iqhost_super_nni_for_branch_rows(self.h, a, b, int(nni5), -1 if first_row is None else int(first_row),
                                                            _dptr(out)))
        return [(out[8 * c], int(out[8 * c + 1]), int(out[8 * c + 2]), list(out[8 * c + 3:8 * c + 8])) for c in range(2)]

    def _evaluate_nnis_list(self, nni5, branches, first_row=None):
        if branches is None:
            br, nbr, cap = None, 0, 4 * self.num_nodes
        else:
            branches = [tuple(b) for b in branches]
            br = _iptr(np.array(branches or [(0, 0)], dtype=np.int32).reshape(-1))
            nbr, cap = len(branches), max(2 * len(branches), 1)
        w = 6 if nni5 else 2
        ids = np.zeros(4 * cap, dtype=np.int32)
        vals = np.zeros(w * cap)
        n = C.c_int()
        self._chk(self.lib.iqhost_super_evaluate_nnis_list_rows(self.h, int(nni5), br, nbr, -1 if first_row is None else int(first_row),
                                                                _iptr(ids), _dptr(vals), cap, C.byref(n)))
        return ids, vals, n.value

    def evaluate_nnis_batch(self, branches=None):
        """all nni1 candidates in two batches of joint solves (needs all_branch=True) -> as PhyloTree.evaluate_nnis_batch"""
        ids, vals, n = self._evaluate_nnis_list(False, branches)
        return [dict(node1=int(ids[4 * k]), node2=int(ids[4 * k + 1]), node1_nei=int(ids[4 * k + 2]),
                     node2_nei=int(ids[4 * k + 3]), new_len=float(vals[2 * k]), newloglh=float(vals[2 * k + 1]))
                for k in range(n)]

    def evaluate_nnis5_batch(self, first_row=None, branches=None):
        """all nni5 candidates in ten batches of joint solves (needs all_branch=True) -> as PhyloTree.evaluate_nnis5_batch;
        first_row: candidate k's per-pattern values are kept in row first_row + k of every member's store (ptnlh_fetch)"""
        ids, vals, n = self._evaluate_nnis_list(True, branches, first_row)
        return [dict(node1=int(ids[4 * k]), node2=int(ids[4 * k + 1]), node1_nei=int(ids[4 * k + 2]),
                     node2_nei=int(ids[4 * k + 3]), new_lens=[float(x) for x in vals[6 * k:6 * k + 5]],
                     newloglh=float(vals[6 * k + 5])) for k in range(n)]

    def do_nni(self, move):
        """the move on the super tree and on every member, their stale vectors cleared; twice restores the tree"""
        self._chk(self.lib.iqhost_super_do_nni(self.h, int(move["node1"]), int(move["node2"]), int(move["node1_nei"]),
                                               int(move["node2_nei"])))

    def change_nni_brans(self, move, nni5=True):
        lens = np.zeros(5)
        if "new_lens" in move:
            lens[:len(move["new_lens"])] = move["new_lens"]
        else:
            lens[0] = move["new_len"]
        self._chk(self.lib.iqhost_super_change_nni_brans(self.h, int(move["node1"]), int(move["node2"]), _dptr(lens), int(nni5)))

    def do_random_nni(self, a, b, bit1, bit2):
        out = np.zeros(4, dtype=np.int32)
        self._chk(self.lib.iqhost_super_do_random_nni(self.h, int(a), int(b), int(bit1), int(bit2), _iptr(out)))
        return dict(node1=int(out[0]), node2=int(out[1]), node1_nei=int(out[2]), node2_nei=int(out[3]))

    def save_branch_lengths(self):
        n = C.c_int()
        self._chk(self.lib.iqhost_super_save_branch_lengths(self.h, None, 0, C.byref(n)))
        out = np.zeros(n.value)
        self._chk(self.lib.iqhost_super_save_branch_lengths(self.h, _dptr(out), n.value, C.byref(n)))
        return out

    def restore_branch_lengths(self, lengths):
        v = np.ascontiguousarray(lengths, dtype=np.float64)
        self._chk(self.lib.iqhost_super_restore_branch_lengths(self.h, _dptr(v), v.size))

    def clear_all_partial_lh(self):
        self._chk(self.lib.iqhost_super_clear_all_partial_lh(self.h))

    def sorted_taxon_id_string(self):
        """the super tree's topology as the reference prints it with WT_TAXON_ID + WT_SORT_TAXA"""
        sup = self.lib.iqhost_super_tree(self.h)
        need = C.c_int()
        self._chk(self.lib.iqhost_sorted_taxon_id_string(sup, None, 0, C.byref(need)))
        buf = C.create_string_buffer(need.value)
        self._chk(self.lib.iqhost_sorted_taxon_id_string(sup, buf, len(buf), C.byref(need)))
        return buf.value.decode()

    def read_tree(self, newick):
        """a candidate tree on the same taxa: re-read by the super tree and every member; engines, models and rates stay,
        member lengths are rate x super lengths, every vector is dropped"""
        self._chk(self.lib.iqhost_super_read_tree(self.h, newick.encode()))

    def optimize_nni(self, nni5=True, speed=True, batched=True, trace=False):
        """compute_likelihood(), then IQTree::optimizeNNI on the super tree -> as PhyloTree.optimize_nni; the partition rates
        and models are taken as given"""
        ts = TreeSearch(self, nni5=nni5, speed=speed, batched=batched)
        try:
            return ts.optimize_nni(trace=trace)
        finally:
            ts.close()

    # ---- UFBoot on the super tree: sites are resampled within partitions (every member keeps its own sample matrix), the
    #      per-replicate state is the group's, the bookkeeping is the plain tree's run on the super tree
    @property
    def _group(self):
        return self.lib.iqhost_super_group(self.h)

    @property
    def _super(self):
        return self.lib.iqhost_super_tree(self.h)

    def gen_boot_samples(self, nsamples, seed):
        """member p: nsamples replicates of its own site count drawn on the device with stream p"""
        self._chk(self.lib.iqhost_super_gen_boot_samples(self.h, int(nsamples), int(seed)))

    def set_boot_samples(self, list_of_W):
        """one float32 [nsamples, member's nptn] matrix of pattern weights per member"""
        if len(list_of_W) != self.nparts:
            raise ValueError("one sample matrix per partition")
        for t, W in zip(self.members, list_of_W):
            t.set_boot_samples(W)

    def ptnlh_reserve(self, nrows):
        _gchk(libiqhip(), libiqhip().iqhip_partition_ptnlh_reserve(self._group, int(nrows)))

    def ptnlh_fetch(self, row):
        """-> the row of every member's store, a list of per-member arrays"""
        return [t.ptnlh_fetch(row) for t in self.members]

    def ptnlh_rell(self, rows, nsamples):
        """-> [len(rows), nsamples]: sum_p L_p[row] . W_p[s], the members' sums added in member order"""
        return _group_ptnlh_rell(libiqhip(), self._group, rows, nsamples)

    def ufboot_init(self, nsamples, seed=0):
        """iqhip_partition_ufboot_init on the first nsamples rows of every member's sample matrix; seed: the tie draws"""
        self._chk(self.lib.iqhost_ufboot_init(self._super, int(nsamples), int(seed)))
        self._ufboot = int(nsamples)

    def ufboot_update(self, rows, tree_ids, logl, rand, epsilon=0.5, logl_cutoff=0.0):
        """iqhip_partition_ufboot_update -> (counts = [applied, dropped by the cutoff, slots replaced], min_orig_logl)"""
        return _group_ufboot_update(libiqhip(), self._group, rows, tree_ids, logl, rand, epsilon, logl_cutoff)

    def ufboot_state(self):
        return _group_ufboot_state(libiqhip(), self._group, getattr(self, "_ufboot", 0))

    def ufboot_timing(self):
        return _group_ufboot_timing(libiqhip(), self._group)

    def ufboot_params(self, epsilon=0.5, logl_cutoff=0.0):
        self._chk(self.lib.iqhost_ufboot_params(self._super, float(epsilon), float(logl_cutoff)))

    def ufboot_next_iteration(self):
        self._chk(self.lib.iqhost_ufboot_next_iteration(self._super))

    def ufboot_info(self):
        info = np.zeros(2, dtype=np.int64)
        vals = np.zeros(2)
        self._chk(self.lib.iqhost_ufboot_info(self._super, info.ctypes.data_as(C.POINTER(C.c_int64)), _dptr(vals)))
        return dict(trees_fed=int(info[0]), trees_kept=int(info[1]), logl_cutoff=float(vals[0]), min_orig_logl=float(vals[1]))

    def save_current_tree(self, logl):
        """the current tree's row on every member (row 0), then one update -> (counts, min_orig_logl)"""
        counts = np.zeros(3, dtype=np.int64)
        mn = C.c_double()
        self._chk(self.lib.iqhost_save_current_tree(self._super, float(logl), counts.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(mn)))
        return counts, mn.value

    def save_nni_trees(self):
        """all 2(n-3) NNI neighbours (evaluate_nnis5_batch with rows 1 ..) through ONE update -> (counts, min_orig_logl)"""
        counts = np.zeros(3, dtype=np.int64)
        mn = C.c_double()
        self._chk(self.lib.iqhost_save_nni_trees(self._super, counts.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(mn)))
        return counts, mn.value

    def summarize_bootstrap(self):
        """as PhyloTree.summarize_bootstrap, on the super tree"""
        cap = self.num_nodes
        ids = np.zeros(2 * cap, dtype=np.int32)
        sup = np.zeros(cap, dtype=np.int32)
        n, distinct, need = C.c_int(), C.c_int(), C.c_int()
        ip = C.POINTER(C.c_int)
        args = (self._super, ids.ctypes.data_as(ip), sup.ctypes.data_as(ip), cap, C.byref(n), C.byref(distinct))
        self._chk(self.lib.iqhost_summarize_bootstrap(*args, None, 0, C.byref(need)))
        buf = C.create_string_buffer(need.value)
        self._chk(self.lib.iqhost_summarize_bootstrap(*args, buf, len(buf), C.byref(need)))
        lines = buf.value.decode().split("\n")
        return dict(support_tree=lines[0], consensus_tree=lines[1], boot_trees=lines[2:2 + self._ufboot],
                    supports=[(int(ids[2 * q]), int(ids[2 * q + 1]), int(sup[q])) for q in range(n.value)],
                    distinct_trees=distinct.value)

    # ---- the starting tree of a partitioned alignment: joint ML distances, BIONJ, fixNegativeBranch
    def compute_dist(self, init=None, want_d2l=False):
        """PhyloSuperTreePlen::computeDist for all pairs (iqhip_partition_pair_distances at the current rates): dist[ntaxa,
        ntaxa], symmetric with a zero diagonal; with want_d2l also minimizeNewton's d2l per pair.  init: None or [ntaxa,
        ntaxa], 0 = the pooled JC start (SuperAlignment::computeDist); a start of 9 is returned without a solve."""
        n = self.num_leaves
        dist, d2l = np.zeros((n, n)), np.zeros((n, n))
        ini = None if init is None else np.ascontiguousarray(init, dtype=np.float64)
        if ini is not None and ini.shape != (n, n):
            raise ValueError("init must be [ntaxa, ntaxa]")
        self._chk(self.lib.iqhost_super_compute_dist(self.h, None if ini is None else _dptr(ini), _dptr(dist), _dptr(d2l)))
        return (dist, d2l) if want_d2l else dist

    def compute_bionj(self, dist=None, var=None):
        """PhyloTree::computeBioNJ on the super tree: the BIONJ tree of dist (None: compute_dist() first) is read into the
        super tree and every member -> the reference's Newick string (lengths may be negative: fix_negative_branch(False))"""
        n = self.num_leaves
        d = self.compute_dist() if dist is None else np.ascontiguousarray(dist, dtype=np.float64)
        v = None if var is None else np.ascontiguousarray(var, dtype=np.float64)
        if d.shape != (n, n) or (v is not None and v.shape != (n, n)):
            raise ValueError("dist and var must be [ntaxa, ntaxa]")
        cap = 1 << 20
        while True:
            buf, need = C.create_string_buffer(cap), C.c_int()
            self._chk(self.lib.iqhost_super_compute_bionj(self.h, _dptr(d), None if v is None else _dptr(v), buf, cap, C.byref(need)))
            if need.value <= cap:
                return buf.value.decode()
            cap = need.value   # (the call is repeated with room for the string and gives the same tree)

    def fix_negative_branch(self, force=True):
        """PhyloSuperTreePlen::fixNegativeBranch: every member's fixNegativeBranch(force) on its own lengths; if any branch
        was fixed the super-tree lengths become the site-weighted means of the members' and the members get rate x super
        length again -> the number of fixed member branches"""
        out = C.c_int()
        self._chk(self.lib.iqhost_super_fix_negative_branch(self.h, int(force), C.byref(out)))
        return out.value

    def partition_pair_timing(self):
        """iqhip_debug_partition_pair_timing of the last compute_dist -> (counts_ms, solve_ms); the times need
        iqhip_timing_enable on member 0"""
        return _group_pair_timing(libiqhip(), self.lib.iqhost_super_group(self.h))

    def partition_timing(self):
        """iqhip_debug_partition_timing of the group's last call (times need iqhip_timing_enable on member 0)"""
        hip = libiqhip()
        ms = (C.c_double * 2)()
        n = C.c_int64()
        if hip.iqhip_debug_partition_timing(self.lib.iqhost_super_group(self.h), ms, C.byref(n)) != 0:
            raise HostError(hip.iqhip_last_error().decode())
        return {"derv_ms": ms[0], "update_ms": ms[1], "launches": n.value}


class AttrDict(dict):
    """dict whose keys also read as attributes (so it can stand where a synth.Model is expected)."""
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)


def _mchk(lib, rc):
    if rc != 0:
        raise HostError(lib.iqmodel_last_error().decode())


def decompose_rate_matrix(rate_matrix, state_freq, ignore_state_freq=False):
    """ModelGTR::decomposeRateMatrix -> dict(eval, evec, inv_evec) (row-major, reference layout)."""
    lib = libiqhost()
    r = np.ascontiguousarray(rate_matrix, dtype=np.float64)
    f = np.ascontiguousarray(state_freq, dtype=np.float64)
    n = f.size
    ev, U, Ui = np.zeros(n), np.zeros((n, n)), np.zeros((n, n))
    _mchk(lib, lib.iqmodel_decompose(_dptr(r), _dptr(f), n, int(ignore_state_freq), _dptr(ev), _dptr(U), _dptr(Ui)))
    return AttrDict(eval=ev, evec=U, inv_evec=Ui)


def gamma_rates(shape, ncat, median=False, p_invar=0.0):
    """RateGamma::computeRates."""
    lib = libiqhost()
    out = np.zeros(ncat)
    _mchk(lib, lib.iqmodel_gamma_rates(float(shape), int(ncat), int(median), float(p_invar), _dptr(out)))
    return out


class Alignment:
    """iqhost::Alignment: PHYLIP/FASTA reader + site->pattern compression."""

    def __init__(self, filename=None, content=None, seq_type=""):
        self.lib = libiqhost()
        self.h = C.c_void_p()
        rc = self.lib.iqaln_read(C.byref(self.h), filename.encode() if filename else None,
                                 content.encode() if content is not None else None, seq_type.encode())
        _mchk(self.lib, rc)
        self.n_unobserved = 0

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.iqaln_destroy(self.h)
            self.h = None

    nseq = property(lambda s: s.lib.iqaln_nseq(s.h))
    nsite = property(lambda s: s.lib.iqaln_nsite(s.h))
    npattern = property(lambda s: s.lib.iqaln_npattern(s.h))
    nstates = property(lambda s: s.lib.iqaln_nstates(s.h))
    seq_type = property(lambda s: s.lib.iqaln_seq_type(s.h))
    state_unknown = property(lambda s: s.lib.iqaln_state_unknown(s.h))
    frac_const_sites = property(lambda s: s.lib.iqaln_frac_const_sites(s.h))

    @property
    def seq_names(self):
        return [self.lib.iqaln_seq_name(self.h, i).decode() for i in range(self.nseq)]

    def append_unobserved_const_patterns(self):
        n = C.c_int()
        _mchk(self.lib, self.lib.iqaln_append_unobserved(self.h, C.byref(n)))
        self.n_unobserved = n.value
        return n.value

    def arrays(self):
        """-> states[nseq, nptn] uint8, ptn_freq[nptn], site_pattern[nsite], const_char[nptn] (-1 = not constant)"""
        ns, npt, nsite = self.nseq, self.npattern, self.nsite
        st = np.zeros((ns, npt), dtype=np.uint8)
        fr = np.zeros(npt)
        sp = np.zeros(nsite, dtype=np.int32)
        cc = np.zeros(npt, dtype=np.int32)
        _mchk(self.lib, self.lib.iqaln_get(self.h, st.ctypes.data_as(C.POINTER(C.c_uint8)), _dptr(fr),
                                           sp.ctypes.data_as(C.POINTER(C.c_int)), cc.ctypes.data_as(C.POINTER(C.c_int))))
        return st, fr, sp, cc

    def informative(self):
        """-> is_informative[nptn] uint8 (Alignment::computeConst's parsimony-informative flag per pattern)"""
        out = np.zeros(self.npattern, dtype=np.uint8)
        _mchk(self.lib, self.lib.iqaln_informative(self.h, out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    @property
    def num_informative_sites(self):
        return int(self.lib.iqaln_num_informative_sites(self.h))

    def ptn_invar(self, p_invar, state_freq):
        out = np.zeros(self.npattern)
        f = np.ascontiguousarray(state_freq, dtype=np.float64)
        _mchk(self.lib, self.lib.iqaln_ptn_invar(self.h, float(p_invar), _dptr(f), _dptr(out)))
        return out

    def state_freq(self):
        out = np.zeros(self.nstates)
        _mchk(self.lib, self.lib.iqaln_state_freq(self.h, _dptr(out)))
        return out

    def codon_freq(self, f3x4=False):
        out, nt = np.zeros(self.nstates), np.zeros(12)
        _mchk(self.lib, self.lib.iqaln_codon_freq(self.h, int(f3x4), _dptr(out), _dptr(nt)))
        return out, nt

    def write_sitelh(self, filename, pattern_lh):
        p = np.ascontiguousarray(pattern_lh, dtype=np.float64)
        _mchk(self.lib, self.lib.iqaln_write_sitelh(self.h, filename.encode(), _dptr(p)))

    def build_model(self, model_string):
        """-m string -> the dict PhyloTree.set_model() takes (+ state_freq, p_invar, asc)."""
        n = self.nstates
        ncat, asc, pinv = C.c_int(), C.c_int(), C.c_double()
        if model_string.upper().startswith("MIX{"):
            # a mixture: + nclass, cat_class, class_freq[nclass, n], class_rates, class_weights; state_freq = their weighted mean
            M = C.c_int()
            _mchk(self.lib, self.lib.iqmodel_mixture_dims(self.h, model_string.encode(), C.byref(M), C.byref(ncat)))
            M, k = M.value, ncat.value
            ev, U, Ui, cf, fr = np.zeros((M, n)), np.zeros((M, n, n)), np.zeros((M, n, n)), np.zeros((M, n)), np.zeros(n)
            cls, rates, props, cr, cw = np.zeros(k, dtype=np.int32), np.zeros(k), np.zeros(k), np.zeros(M), np.zeros(M)
            _mchk(self.lib, self.lib.iqmodel_build_mixture(self.h, model_string.encode(), C.byref(pinv), C.byref(asc), _dptr(ev),
                                                           _dptr(U), _dptr(Ui), _dptr(cf), _dptr(fr),
                                                           cls.ctypes.data_as(C.POINTER(C.c_int)), _dptr(rates), _dptr(props),
                                                           _dptr(cr), _dptr(cw)))
            return AttrDict(nstates=n, ncat=k, nclass=M, cat_class=cls, eval=ev, evec=U, inv_evec=Ui, state_freq=fr,
                            class_freq=cf, class_rates=cr, class_weights=cw, rates=rates, props=props, p_invar=pinv.value,
                            asc=bool(asc.value))
        ev, U, Ui, fr = np.zeros(n), np.zeros((n, n)), np.zeros((n, n)), np.zeros(n)
        rates, props = np.zeros(64), np.zeros(64)
        _mchk(self.lib, self.lib.iqmodel_build(self.h, model_string.encode(), C.byref(ncat), C.byref(pinv), C.byref(asc),
                                               _dptr(ev), _dptr(U), _dptr(Ui), _dptr(fr), _dptr(rates), _dptr(props)))
        k = ncat.value
        return AttrDict(nstates=n, ncat=k, eval=ev, evec=U, inv_evec=Ui, state_freq=fr, rates=rates[:k].copy(),
                    props=props[:k].copy(), p_invar=pinv.value, asc=bool(asc.value))
