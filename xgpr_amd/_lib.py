"""ctypes binding of libxgpr_hip.so (the C ABI declared in include/xgpr_hip.h).

There is no CPU fallback: if the library is missing the import of any product module
fails loudly, and every compute entry point needs a HIP device.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# XGPR_HIP_LIB: development aid (ablation builds of the same library); never a fallback
LIB_PATH = os.environ.get("XGPR_HIP_LIB", os.path.join(_HERE, "libxgpr_hip.so"))

_vp, _l, _i, _d, _sz = C.c_void_p, C.c_long, C.c_int, C.c_double, C.c_size_t

# name -> argtypes; mirrors include/xgpr_hip.h one to one (tests/test_cabi.py checks that
# every function declared in the header is listed here and exported by the library).
SIGNATURES = {
    "xgpr_fht_f32": [_vp, _l, _l, _l, _vp],
    "xgpr_fht_f64": [_vp, _l, _l, _l, _vp],
    "xgpr_srht_f32": [_vp, _vp, _l, _l, _l, _vp],
    "xgpr_srht_f64": [_vp, _vp, _l, _l, _l, _vp],
    "xgpr_srht_sample_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _l, _l, _l, _l, _l, _vp, _sz, _vp],
    "xgpr_srht_sample_f64": [_vp, _vp, _vp, _vp, _vp, _vp, _l, _l, _l, _l, _l, _vp, _sz, _vp],
    "xgpr_rbf_feature_gen_f32": [_vp, _vp, _vp, _vp, _l, _l, _l, _l, _l, _l, _i, _vp, _sz, _vp],
    "xgpr_rbf_feature_gen_f64": [_vp, _vp, _vp, _vp, _l, _l, _l, _l, _l, _l, _i, _vp, _sz, _vp],
    "xgpr_rbf_grad_f32": [_vp, _vp, _vp, _vp, _vp, _l, _l, _l, _l, _l, _l, _l, _l, _d, _i, _vp, _sz, _vp],
    "xgpr_rbf_grad_f64": [_vp, _vp, _vp, _vp, _vp, _l, _l, _l, _l, _l, _l, _l, _l, _d, _i, _vp, _sz, _vp],
    "xgpr_rbf_grad_rows_f32": [_vp, _vp, _vp, _vp, _vp, _l, _l, _l, _l, _l, _d, _i, _vp, _sz, _vp],
    "xgpr_mini_ard_grad_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _l, _l, _l, _l, _l, _l, _l, _l, _l, _l, _l, _i, _vp],
    "xgpr_mini_ard_grad_f64": [_vp, _vp, _vp, _vp, _vp, _vp, _l, _l, _l, _l, _l, _l, _l, _l, _l, _l, _l, _i, _vp],
    "xgpr_conv1d_fgen_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _l, _l, _l, _l, _l, _l, _l, _l, _i, _i, _vp, _sz, _vp],
    "xgpr_conv1d_fgen_f64": [_vp, _vp, _vp, _vp, _vp, _vp, _l, _l, _l, _l, _l, _l, _l, _l, _i, _i, _vp, _sz, _vp],
    "xgpr_conv_feature_rows_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _l, _l, _l, _l, _l, _l, _l, _i, _i, _i, _vp, _sz, _vp],
    "xgpr_conv_grad_rows_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _l, _l, _l, _l, _l, _l, _l, _d, _i, _i, _i, _vp, _sz, _vp],
    "xgpr_conv_token_rows_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _l, _l, _l, _l, _l, _l, _l, _l, _i, _i, _i, _vp, _sz, _vp],
    "xgpr_conv_token_grad_rows_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _l, _l, _l, _l, _l, _l, _l, _l, _d, _i, _i, _i,
                                      _vp, _sz, _vp],
    "xgpr_conv_token_rows_ok": [_l, _l, _l],
    "xgpr_conv_grad_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _l, _l, _l, _l, _l, _l, _l, _l, _l, _l, _d, _i, _i,
                           _vp, _sz, _vp],
    "xgpr_conv_grad_f64": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _l, _l, _l, _l, _l, _l, _l, _l, _l, _l, _d, _i, _i,
                           _vp, _sz, _vp],
    "xgpr_conv1d_maxpool_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _l, _l, _l, _l, _l, _l, _l, _l, _i, _vp, _sz, _vp],
    "xgpr_conv1d_maxpool_f64": [_vp, _vp, _vp, _vp, _vp, _vp, _l, _l, _l, _l, _l, _l, _l, _l, _i, _vp, _sz, _vp],
    "xgpr_ztz_matvec_f32": [_vp, _vp, _vp, _vp, _vp, _l, _l, _l, _l, _l, _i, _vp, _sz, _vp],
    "xgpr_zty_f32": [_vp, _vp, _vp, _vp, _vp, _l, _l, _l, _l, _l, _i, _vp, _sz, _vp],
    "xgpr_cg_step1_f64": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _d, _d, _l, _d, _vp, _vp],
    "xgpr_cg_step2_f64": [_vp, _vp, _vp, _vp, _vp, _l, _d, _vp],
    "xgpr_softmax_residual_f64": [_vp, _vp, _l, _l, _vp, _vp],
    "xgpr_precond_utr_block_f64": [_vp, _vp, _vp, _l, _l, _l, _vp, _sz, _vp],
    "xgpr_precond_apply_block_f64": [_vp, _vp, _d, _vp, _vp, _l, _l, _l, _vp, _sz, _vp],
    "xgpr_cg_step1_block_f64": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _d, _l, _l, _vp, _sz, _vp],
    "xgpr_cg_step2_block_f64": [_vp, _vp, _vp, _vp, _vp, _vp, _l, _l, _vp, _sz, _vp],
    "xgpr_precond_apply_f64": [_vp, _vp, _d, _vp, _vp, _l, _l, _vp, _sz, _vp],
    "xgpr_rbf_feature_cache_f32": [_vp, _vp, _vp, _vp, _l, _l, _l, _l, _l, _vp, _sz, _vp],
    "xgpr_zcache_matvec_f32": [_vp, _vp, _vp, _l, _l, _i, _vp, _sz, _vp],
    "xgpr_zcache_matvec_scaled_f32": [_vp, _vp, _vp, _l, _l, _d, _vp, _sz, _vp],
    "xgpr_rows_pack_f16": [_vp, _vp, _l, _vp],
    "xgpr_zcache_matvec_f16": [_vp, _vp, _vp, _l, _l, _i, _vp, _sz, _vp],
    "xgpr_zcache_matvec_scaled_f16": [_vp, _vp, _vp, _l, _l, _d, _vp, _sz, _vp],
    "xgpr_zcache_zty_f32": [_vp, _vp, _vp, _l, _l, _i, _d, _vp, _sz, _vp],
    "xgpr_zcache_block_matvec_f32": [_vp, _vp, _vp, _l, _l, _l, _i, _d, _i, _vp, _sz, _vp],
    "xgpr_zcache_block_project_f32": [_vp, _vp, _vp, _l, _l, _l, _i, _d, _vp, _sz, _vp],
    "xgpr_zcache_block_backproject_f32": [_vp, _vp, _vp, _l, _l, _l, _i, _d, _i, _vp, _sz, _vp],
    "xgpr_srht_sample_rows_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _l, _l, _l, _l, _l, _d, _i, _vp, _sz, _vp],
    "xgpr_sketch_gemm_f64": [_vp, _l, _vp, _l, _l, _vp, _l, _l, _i, _i, _d, _i, _i, _vp, _sz, _vp],
    "xgpr_ztz_gram_f64": [_vp, _l, _l, _vp, _l, _l, _d, _i, _i, _vp, _sz, _vp],
    "xgpr_cross_gram_f64": [_vp, _vp, _l, _l, _vp, _l, _i, _vp, _sz, _vp],
    "xgpr_selftest_lane_xor": [_vp, _vp],
    "xgpr_ztz_matvec_plan": [_l, _l],
    "xgpr_rccl_load": [C.c_char_p],
    "xgpr_rccl_unique_id": [_vp],
    "xgpr_rccl_comm_init": [_vp, _i, _vp, _i],
    "xgpr_allreduce_sum_f64": [_vp, _vp, _l, _vp],
    "xgpr_rccl_comm_destroy": [_vp],
}
SIZE_FUNCS = {
    "xgpr_rbf_workspace_bytes": [_l],
    "xgpr_sorf_workspace_bytes": [_l, _l, _i],
    "xgpr_conv_workspace_bytes": [_l, _l, _i, _l],
    "xgpr_conv_feature_rows_workspace_bytes": [_l, _l, _l, _l],
    "xgpr_conv_grad_rows_workspace_bytes": [_l, _l, _l, _l],
    "xgpr_precond_apply_workspace_bytes": [_l],
    "xgpr_precond_utr_block_workspace_bytes": [_l, _l, _l],
    "xgpr_precond_apply_block_workspace_bytes": [_l, _l, _l],
    "xgpr_cg_block_workspace_bytes": [_l, _l],
    "xgpr_ztz_matvec_workspace_bytes": [_l, _l],
    "xgpr_zcache_block_workspace_bytes": [_l, _l, _l],
    "xgpr_zcache_block_project_workspace_bytes": [_l, _l, _l],
    "xgpr_srht_sample_workspace_bytes": [_l],
    "xgpr_sketch_gemm_workspace_bytes": [_l, _l, _l, _l, _i],
    "xgpr_ztz_gram_workspace_bytes": [_l, _l],
    "xgpr_cross_gram_workspace_bytes": [_l, _l],
}
# ... and include/xgpr_hip_pool.h, the second public header (tests/test_pool_header_host.py checks it the same way)
POOL_SIGNATURES = {
    "xgpr_conv_token_maxpool_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _l, _l, _l, _l, _l, _l, _l, _l, _l, _i, _vp, _sz, _vp],
}
# ... and include/xgpr_hip_input_grad.h, the third (tests/test_input_grad_host.py)
INPUT_GRAD_SIGNATURES = {
    "xgpr_rbf_input_grad_ok": [_l, _l],
    "xgpr_rbf_input_grad_f32": [_vp, _vp, _vp, _vp, _vp, _l, _l, _l, _l, _l, _l, _d, _i, _vp, _sz, _vp],
}
# ... and include/xgpr_hip_seq_input_grad.h, the fourth (tests/test_seq_input_grad_host.py)
SEQ_INPUT_GRAD_SIGNATURES = {
    "xgpr_conv_input_grad_ok": [_l, _l],
    "xgpr_conv_token_input_grad_ok": [_l, _l, _l],
    "xgpr_conv_input_grad_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _l, _l, _l, _l, _l, _l, _l, _d, _i, _i, _i, _vp, _sz, _vp],
    "xgpr_conv_token_input_grad_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _l, _l, _l, _l, _l, _l, _l, _l, _d, _i, _i, _i, _vp,
                                       _sz, _vp],
}
# ... and include/xgpr_hip_pool_input_grad.h, the fifth (tests/test_pool_input_grad_host.py)
POOL_INPUT_GRAD_SIGNATURES = {
    "xgpr_conv_maxpool_input_grad_ok": [_l],
    "xgpr_conv_token_maxpool_input_grad_ok": [_l, _l, _l],
    "xgpr_conv_maxpool_input_grad_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _l, _l, _l, _l, _l, _l, _i, _vp, _sz, _vp],
    "xgpr_conv_token_maxpool_input_grad_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _l, _l, _l, _l, _l, _l, _l, _i, _vp,
                                               _sz, _vp],
}
# ... and include/xgpr_hip_cluster.h, the sixth (tests/test_cluster_host.py); its two *_workspace_bytes functions return size_t
CLUSTER_SIGNATURES = {
    "xgpr_kmeans_ok": [_l, _l],
    "xgpr_kmeans_assign_workspace_bytes": [_l, _l, _l],
    "xgpr_kmeans_assign_f32": [_vp, _vp, _vp, _vp, _l, _l, _l, _vp, _sz, _vp],
    "xgpr_kmeans_update_workspace_bytes": [_l, _l, _l],
    "xgpr_kmeans_update_f32": [_vp, _vp, _vp, _vp, _l, _l, _l, _i, _vp, _sz, _vp],
}
# ... and include/xgpr_hip_subst_scan.h, the seventh (tests/test_subst_scan_host.py)
SUBST_SCAN_SIGNATURES = {
    "xgpr_conv_token_subst_scan_ok": [_l, _l, _l, _l],
    "xgpr_conv_token_subst_scan_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _l, _l, _l, _l, _l, _l, _i, _i, _i, _vp, _sz, _vp],
}
# ... and include/xgpr_hip_indel_scan.h, the eighth (tests/test_indel_scan_host.py)
INDEL_SCAN_SIGNATURES = {
    "xgpr_conv_token_indel_scan_ok": [_l, _l, _l, _l],
    "xgpr_conv_token_window_scores_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _l, _l, _l, _l, _l, _l, _i, _i, _vp, _sz, _vp],
    "xgpr_conv_token_indel_scan_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _l, _l, _l, _l, _l, _l, _i, _i, _i, _vp, _sz, _vp],
}
# ... and include/xgpr_hip_subst_var_scan.h, the ninth (tests/test_subst_var_scan_host.py); its *_workspace_bytes function returns size_t
SUBST_VAR_SCAN_SIGNATURES = {
    "xgpr_conv_token_subst_var_scan_ok": [_l, _l, _l, _l, _l],
    "xgpr_conv_token_subst_var_scan_workspace_bytes": [_l, _l, _l],
    "xgpr_conv_token_subst_var_scan_f32": [_vp, _vp, _vp, _l, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _l, _l, _l, _l, _l, _l, _l, _i, _i, _i, _l,
                                           _vp, _sz, _vp],
}
# ... and include/xgpr_hip_indel_var_scan.h, the tenth (tests/test_indel_var_scan_host.py); its *_workspace_bytes function returns size_t
INDEL_VAR_SCAN_SIGNATURES = {
    "xgpr_conv_token_indel_var_scan_ok": [_l, _l, _l, _l, _l],
    "xgpr_conv_token_indel_var_scan_workspace_bytes": [_l, _l, _l],
    "xgpr_conv_token_indel_var_scan_f32": [_vp, _vp, _vp, _l, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _l, _l, _l, _l, _l, _l, _l,
                                           _i, _i, _i, _l, _vp, _sz, _vp],
}
# ... and include/xgpr_hip_pair_scan.h, the eleventh (tests/test_pair_scan_host.py)
PAIR_SCAN_SIGNATURES = {
    "xgpr_conv_token_pair_scan_ok": [_l, _l, _l, _l],
    "xgpr_conv_token_pair_scan_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _l, _l, _l, _l, _l, _l, _i, _i, _i, _vp, _sz, _vp],
}
# ... and include/xgpr_hip/pool_edits.h, the twelfth (tests/test_pool_edits_host.py); why its name does not end like the others': see
# that header's opening comment
POOL_EDITS_ABI = {
    "xgpr_conv_token_maxpool_edits_ok": [_l, _l, _l, _l],
    "xgpr_conv_token_maxpool_tables_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _l, _l, _l, _l, _l, _l, _l, _i, _vp, _sz, _vp],
    "xgpr_conv_token_maxpool_edits_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _l, _l, _l, _l, _l, _l, _l, _i, _i, _l, _l, _vp,
                                          _sz, _vp],
}
# ... and include/xgpr_hip/edit_proj.h, the thirteenth (tests/test_edit_proj_host.py); named like the twelfth's table, for its reason; its
# *_workspace_bytes function returns size_t
EDIT_PROJ_ABI = {
    "xgpr_conv_token_edit_proj_ok": [_l, _l, _l, _l, _l, _l],
    "xgpr_conv_token_edit_proj_workspace_bytes": [_l, _l, _l],
    "xgpr_conv_token_subst_proj_f32": [_vp, _vp, _vp, _l, _vp, _vp, _vp, _vp, _vp, _vp, _l, _l, _l, _l, _l, _l, _l, _l, _i, _i, _i, _l,
                                       _vp, _sz, _vp],
    "xgpr_conv_token_indel_proj_f32": [_vp, _vp, _vp, _l, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _l, _l, _l, _l, _l, _l, _l, _l, _i, _i,
                                       _i, _l, _vp, _sz, _vp],
}
# ... and include/xgpr_hip/site_scan.h, the fourteenth (tests/test_site_scan_host.py); named like the twelfth's table, for its reason; its
# *_workspace_bytes function returns size_t and its *_layout function long
SITE_SCAN_ABI = {
    "xgpr_conv_token_site_scan_ok": [_l, _l, _l, _l, _i],
    "xgpr_conv_token_site_scan_layout": [_vp, _i, _l, _i, _l, _vp, _vp, _vp, _vp, _vp, _i],
    "xgpr_conv_token_site_scan_workspace_bytes": [_l, _l, _i],
    "xgpr_conv_token_site_scan_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _l, _l, _l, _l, _l, _l, _i, _i, _i, _vp, _sz, _vp],
}
STRING_FUNCS = ["xgpr_last_error", "xgpr_build_arch", "xgpr_build_id"]

_lib = None


def load():
    """Load libxgpr_hip.so.  Raises ImportError (loudly) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    # torch first: it ships its own libamdhip64 and must be the HIP runtime of the process; loading this
    # library before torch would bind it to the system copy, and the second runtime then sees no device
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: the HIP extension has not been built "
            "(run `python xgpr_amd/build.py`); xgpr_amd has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, args in (list(SIGNATURES.items()) + list(POOL_SIGNATURES.items()) + list(INPUT_GRAD_SIGNATURES.items())
                       + list(SEQ_INPUT_GRAD_SIGNATURES.items()) + list(POOL_INPUT_GRAD_SIGNATURES.items()) + list(CLUSTER_SIGNATURES.items())
                       + list(SUBST_SCAN_SIGNATURES.items()) + list(INDEL_SCAN_SIGNATURES.items())
                       + list(SUBST_VAR_SCAN_SIGNATURES.items()) + list(INDEL_VAR_SCAN_SIGNATURES.items())
                       + list(PAIR_SCAN_SIGNATURES.items()) + list(POOL_EDITS_ABI.items()) + list(EDIT_PROJ_ABI.items())
                       + list(SITE_SCAN_ABI.items())):
        fn = getattr(lib, name)
        fn.argtypes = args
        sized = (name in CLUSTER_SIGNATURES or name in SUBST_VAR_SCAN_SIGNATURES or name in INDEL_VAR_SCAN_SIGNATURES
                 or name in EDIT_PROJ_ABI or name in SITE_SCAN_ABI)
        fn.restype = (C.c_size_t if sized and name.endswith("_workspace_bytes")
                      else C.c_long if name == "xgpr_conv_token_site_scan_layout" else C.c_int)
    for name, args in SIZE_FUNCS.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = C.c_size_t
    for name in STRING_FUNCS:
        fn = getattr(lib, name)
        fn.argtypes = []
        fn.restype = C.c_char_p
    _lib = lib
    return lib


def build_id():
    """sha256 of the sources and flags the loaded library was compiled from (xgpr_amd/build.py source_id())."""
    return load().xgpr_build_id().decode()


def last_error():
    return load().xgpr_last_error().decode()


def check(rc):
    """Map a negative return code to the RuntimeError the reference would have thrown."""
    if rc != 0:
        raise RuntimeError(last_error() or f"xgpr_hip error {rc}")
    return 0
