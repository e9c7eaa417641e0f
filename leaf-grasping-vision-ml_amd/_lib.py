"""ctypes binding of liblgrasp.so (include/leafgrasp.h).  The library is REQUIRED: there is no CPU or
PyTorch fallback anywhere in this package -- a missing/unloadable library raises at import."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LG_LIB_PATH") or os.path.join(_HERE, "liblgrasp.so")  # override: kernel experiments only

LG_NUM_MAPS = 8
MAP_NAMES = ("sdf_score", "approach_score", "flatness_map", "isolation_map", "distance_map",
             "accessibility_map", "stem_penalty", "traditional_score")  # grasp_point_selector.py:258-280
MAP_INDEX = {n: i for i, n in enumerate(MAP_NAMES)}

LG_OK, LG_ERR_INVALID, LG_ERR_HIP, LG_ERR_NOMEM, LG_ERR_NO_MODEL, LG_ERR_UNSUPPORTED, LG_ERR_BUSY = 0, -1, -2, -3, -4, -5, -6


class LgParams(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("cx", "cy", "f")] + [(n, C.c_float) for n in (
        "w_approach", "w_sdf", "w_flat", "w_access", "sdf_w_interior", "sdf_w_align",
        "sdf_w_sdf", "optimal_distance", "access_w_dist", "access_w_dir", "flat_scale", "iso_w_close",
        "iso_w_wide", "iso_ramp_top", "iso_ramp_bottom", "min_edge_distance", "stem_valid_thresh")] + \
        [(n, C.c_int32) for n in ("stem_se", "stem_bottom_div", "top_k", "nms_min_distance",
                                  "pregrasp_clearance", "mask_is_bool", "gaussian_size", "chamfer_init_dist0", "label_aware")]


_FP = C.POINTER(C.c_float)


class LgCnnWeights(C.Structure):
    _fields_ = [("conv_w", _FP * 8), ("conv_b", _FP * 8), ("bn_g", _FP * 8), ("bn_b", _FP * 8),
                ("bn_m", _FP * 8), ("bn_v", _FP * 8), ("att_w", _FP), ("att_b", _FP),
                ("fc_w", _FP * 4), ("fc_b", _FP * 4), ("fbn_g", _FP * 3), ("fbn_b", _FP * 3),
                ("fbn_m", _FP * 3), ("fbn_v", _FP * 3), ("bn_eps", C.c_float), ("attention_type", C.c_int32),
                ("ca_w1", _FP), ("ca_b1", _FP), ("ca_w2", _FP), ("ca_b2", _FP),
                ("n_blocks", C.c_int32), ("filters", C.c_int32 * 4)]


class LgGraspResult(C.Structure):
    _fields_ = [("found", C.c_int32), ("x", C.c_int32), ("y", C.c_int32), ("X", C.c_float), ("Y", C.c_float),
                ("Z", C.c_float), ("has_pre", C.c_int32), ("pX", C.c_float), ("pY", C.c_float),
                ("pZ", C.c_float), ("n_candidates", C.c_int32), ("ml_used", C.c_int32),
                ("best_score", C.c_float), ("theta", C.c_float)]


class LgGraspCandidate(C.Structure):
    """lg_grasp_candidate: one ranked candidate of lg_select_grasp_candidates (17 four-byte fields)."""
    _fields_ = [("index", C.c_int32), ("x", C.c_int32), ("y", C.c_int32), ("traditional", C.c_float), ("ml_score", C.c_float),
                ("ml_confidence", C.c_float), ("combined", C.c_float), ("scored", C.c_int32), ("pick_score", C.c_float),
                ("by_ml", C.c_int32), ("X", C.c_float), ("Y", C.c_float), ("Z", C.c_float), ("has_pre", C.c_int32),
                ("pX", C.c_float), ("pY", C.c_float), ("pZ", C.c_float)]


LG_ML_SAMPLE_NTH, LG_ML_SAMPLE_GRID = 0, 1


class LgMlSampling(C.Structure):
    """lg_ml_sampling: how lg_select_grasp_ml* picks the leaf pixels it scores (chunk 0 = the library's default)."""
    _fields_ = [("mode", C.c_int32), ("target", C.c_int32), ("stride", C.c_int32), ("max_samples", C.c_int32),
                ("chunk", C.c_int32)]


class LgMlSample(C.Structure):
    """lg_ml_sample: one row of the sample table of lg_select_grasp_ml* (20 bytes)."""
    _fields_ = [("x", C.c_int32), ("y", C.c_int32), ("scored", C.c_int32), ("logit", C.c_float), ("ml_score", C.c_float)]


class LgCollectParams(C.Structure):
    """lg_collect_params: the constants of the collecting selector (lg_select_grasp_collect)."""
    _fields_ = [("erosion_kernel_size", C.c_int32), ("erosion_iterations", C.c_int32), ("tip_se", C.c_int32),
                ("tip_aware", C.c_int32), ("w_tip", C.c_float)]


class LgTrainHparams(C.Structure):
    """lg_train_hparams; defaults = scripts/train_model.py:221-222,256."""
    _fields_ = [("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
                ("weight_decay", C.c_float), ("max_grad_norm", C.c_float), ("pos_weight", C.c_float)]


class LgLeafStat(C.Structure):
    _fields_ = [("id", C.c_int32), ("area", C.c_int32), ("touches_border", C.c_int32), ("pad_", C.c_int32),
                ("sum_x", C.c_double), ("sum_y", C.c_double), ("sum_depth", C.c_double), ("sum_ray", C.c_double),
                ("median_depth", C.c_float), ("pad2_", C.c_float)]


class LgEvalResult(C.Structure):
    """lg_eval_result: validation loss and confusion counts of lg_eval_logits / lg_cnn_evaluate (64 bytes)."""
    _fields_ = [("loss", C.c_double), ("n", C.c_int64), ("n_chunks", C.c_int64), ("correct", C.c_int64),
                ("tp", C.c_int64), ("fp", C.c_int64), ("fn", C.c_int64), ("tn", C.c_int64)]


# lg_debug_cnn_weights: the buffers of the loaded CNN (include/leafgrasp.h LG_CNNW_*)
CNNW = {"bconv": 0, "wconv": 1, "uwino": 2, "uwino4": 3, "fcw": 4, "fcb": 5, "att_w": 6, "ca_w1": 7, "ca_b1": 8, "ca_w2": 9,
        "ca_b2": 10, "zeros": 11, "scalars": 12, "allocs": 13}


# every symbol include/leafgrasp.h declares: (restype, argtypes)
_VP = C.c_void_p
SYMBOLS = {
    "lg_create": (C.c_int, [C.c_int, C.POINTER(_VP)]),
    "lg_destroy": (C.c_int, [_VP]),
    "lg_last_error": (C.c_char_p, [_VP]),
    "lg_orientation_note": (C.c_char_p, [_VP]),
    "lg_version": (C.c_char_p, []),
    "lg_default_params": (None, [C.POINTER(LgParams)]),
    "lg_score_maps": (C.c_int, [_VP, _VP, _VP, C.c_int, C.c_int, C.c_int, C.POINTER(LgParams),
                                C.POINTER(_VP * LG_NUM_MAPS), _VP, _FP, _VP]),
    "lg_smooth_depth": (C.c_int, [_VP, _VP, C.c_int, C.c_int, C.c_int, C.c_int, _VP, _VP]),
    "lg_gaussian_taps": (C.c_int, [C.c_int, _FP]),
    "lg_topk_nms": (C.c_int, [_VP, _VP, _VP, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _VP, _VP, _VP]),
    "lg_gather_patches": (C.c_int, [_VP, _VP, _VP, C.POINTER(_VP * LG_NUM_MAPS), C.c_int, C.c_int, C.c_int,
                                    C.c_int, _VP, _VP, _VP, _VP]),
    "lg_cnn_load": (C.c_int, [_VP, C.POINTER(LgCnnWeights)]),
    "lg_cnn_unload": (C.c_int, [_VP]),
    "lg_cnn_forward": (C.c_int, [_VP, _VP, C.c_int, _VP, _VP]),
    "lg_select_grasp": (C.c_int, [_VP, _VP, _VP, C.c_int, C.c_int, C.c_int, C.POINTER(LgParams),
                                  C.POINTER(_VP * LG_NUM_MAPS), _VP, C.POINTER(LgGraspResult), _VP]),
    "lg_select_grasp_labels": (C.c_int, [_VP, _VP, _VP, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.POINTER(LgParams),
                                         C.POINTER(_VP * LG_NUM_MAPS), _VP, C.POINTER(LgGraspResult), _VP]),
    "lg_select_grasp_candidates": (C.c_int, [_VP, _VP, _VP, C.c_int, C.c_int, C.c_int, C.POINTER(LgParams),
                                             C.POINTER(LgGraspResult), C.POINTER(LgGraspCandidate), _VP]),
    "lg_select_grasp_candidates_labels": (C.c_int, [_VP, _VP, _VP, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int,
                                                    C.POINTER(LgParams), C.POINTER(LgGraspResult), C.POINTER(LgGraspCandidate), _VP]),
    "lg_default_ml_sampling": (None, [C.POINTER(LgMlSampling)]),
    "lg_select_grasp_ml": (C.c_int, [_VP, _VP, _VP, C.c_int, C.c_int, C.c_int, C.POINTER(LgParams), C.POINTER(LgMlSampling),
                                     C.POINTER(LgGraspResult), _VP, C.POINTER(C.c_int32), _VP]),
    "lg_select_grasp_ml_labels": (C.c_int, [_VP, _VP, _VP, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.POINTER(LgParams),
                                            C.POINTER(LgMlSampling), C.POINTER(LgGraspResult), _VP, C.POINTER(C.c_int32), _VP]),
    "lg_ml_sample_points_host": (C.c_int, [_VP, C.c_int, C.c_int, C.c_int, C.POINTER(LgMlSampling), _VP, _VP, C.c_int,
                                           C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "lg_debug_ml_planes": (C.c_int, [_VP, C.c_int, C.POINTER(C.c_int32)]),
    "lg_default_collect_params": (None, [C.POINTER(LgCollectParams)]),
    "lg_collect_params_check": (C.c_int, [C.POINTER(LgParams), C.POINTER(LgCollectParams)]),
    "lg_erode_ellipse": (C.c_int, [_VP, _VP, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _VP, _VP]),
    "lg_erode_words_host": (C.c_int, [_VP, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _VP]),
    "lg_tip_penalty": (C.c_int, [_VP, _VP, C.c_int, C.c_int, C.c_int, C.POINTER(LgParams), C.POINTER(LgCollectParams), _VP, _VP,
                                 _VP]),
    "lg_tip_fix_host": (C.c_int, [C.c_int, C.c_int, C.c_int32, _VP, C.POINTER(C.c_uint32)]),
    "lg_argmax_first": (C.c_int, [_VP, _VP, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), _FP, C.POINTER(C.c_int32), _VP]),
    "lg_select_grasp_collect": (C.c_int, [_VP, _VP, _VP, C.c_int, C.c_int, C.c_int, C.POINTER(LgParams), C.POINTER(LgCollectParams),
                                          C.POINTER(_VP * LG_NUM_MAPS), _VP, _VP, _VP, C.POINTER(LgGraspResult), _VP]),
    "lg_rank_grasp_candidates": (C.c_int, [_VP, _VP, _VP, C.c_int, C.c_int, _VP, _VP, _VP]),
    "lg_ml_combined_score": (C.c_int, [C.c_double, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                       C.POINTER(C.c_double)]),
    "lg_cnn_candidate_cannot_win": (C.c_int, [C.c_double, C.c_double]),
    "lg_leaf_stats": (C.c_int, [_VP, _VP, _VP, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float,
                                C.POINTER(LgLeafStat), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int32), _VP]),
    "lg_leaf_stats_batch": (C.c_int, [_VP, _VP, _VP, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float,
                                      C.POINTER(LgLeafStat), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int32),
                                      C.POINTER(C.c_int), _VP]),
    "lg_leaf_select_batch": (C.c_int, [_VP, _VP, _VP, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double,
                                       C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int, _VP]),
    "lg_leaf_select_from_stats": (C.c_int, [C.POINTER(LgLeafStat), C.c_int, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_double,
                                            C.c_double, C.c_double, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int,
                                            C.POINTER(C.c_int32)]),
    "lg_leaf_orientation": (C.c_int, [_VP, _VP, C.c_int, C.c_int, _FP, C.POINTER(C.c_int), _VP]),
    "lg_profile_enable": (C.c_int, [_VP, C.c_int]),
    "lg_profile_read": (C.c_int, [_VP, C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_double)]),
    "lg_debug_dt_max": (C.c_int, [_VP, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_int32)]),
    "lg_format_grasp_results": (C.c_int, [_VP, C.c_int, C.c_char_p, C.c_int64, C.POINTER(C.c_int64)]),
    "lg_debug_dt_form": (C.c_int, [_VP, C.c_int, C.POINTER(C.c_int32)]),
    "lg_debug_orient_redo": (C.c_int, [_VP, C.POINTER(C.c_int32)]),
    "lg_options_text": (C.c_int, [C.c_int, C.c_char_p, C.c_int]),
    "lg_debug_options": (C.c_int, [_VP, C.c_char_p, C.c_int]),
    "lg_debug_dt_search_form": (C.c_int, [_VP, C.POINTER(C.c_int32)]),
    "lg_dt_form_host": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "lg_near_tile_rect": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32)]),
    "lg_stem_words_host": (C.c_int, [_VP, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _VP]),
    "lg_stem_words_host_spans": (C.c_int, [_VP, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int8),
                                           C.POINTER(C.c_int8), C.c_int, _VP]),
    "lg_stem_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int8), C.POINTER(C.c_int8), C.POINTER(C.c_int32),
                               C.POINTER(C.c_int8), C.POINTER(C.c_int8), C.POINTER(C.c_int8), C.POINTER(C.c_int8)]),
    "lg_window_from_box": (C.c_int, [C.POINTER(C.c_uint32), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32)]),
    "lg_border_line_max": (C.c_int, [C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint32)]),
    "lg_debug_near_tiles":(C.c_int, [_VP, C.POINTER(C.c_int32), C.c_int]),
    "lg_tail_lane_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "lg_debug_tail_lanes": (C.c_int, [_VP, C.c_int, C.POINTER(C.c_int32)]),
    "lg_debug_cnn_scored": (C.c_int, [_VP, C.POINTER(C.c_int64)]),
    "lg_debug_leaf_fallback": (C.c_int, [_VP, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "lg_debug_cnn_survivors": (C.c_int, [_VP, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int32,
                                         C.POINTER(C.c_int32), C.POINTER(C.c_int32), _FP, C.c_int64, C.POINTER(C.c_int64)]),
    "lg_debug_patch": (C.c_int, [_VP, C.c_int64, _FP]),
    "lg_debug_isolation_fields": (C.c_int, [_VP, C.c_int, _VP, _VP, C.POINTER(C.c_uint32)]),
    "lg_label_aware_check": (C.c_int, [C.POINTER(LgParams), C.c_int]),
    "lg_norm3_host": (C.c_int, [_VP, _VP, C.c_int, _VP]),
    "lg_dilate_words_host": (C.c_int, [_VP, C.c_int, C.c_int, C.c_int, C.c_int, _VP]),
    "lg_debug_ws_plane_bytes": (C.c_int, [_VP, C.POINTER(C.c_int64)]),
    "lg_wave_rows_on_mask": (C.c_int, [_VP, C.c_int, C.c_int, C.c_int, C.c_int]),
    "lg_harvest_patches": (C.c_int, [_VP, _VP, _VP, _VP, C.c_int, C.c_int, C.c_int, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "lg_negative_masks": (C.c_int, [_VP, _VP, _VP, C.c_int, C.c_int, _VP, _VP, _VP]),
    "lg_leaf_contour": (C.c_int, [_VP, _VP, C.c_int, C.c_int, _VP, C.c_int, C.POINTER(C.c_int), _VP]),
    "lg_train_create": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int, C.c_int, C.POINTER(_VP)]),
    "lg_train_destroy": (C.c_int, [_VP]),
    "lg_train_last_error": (C.c_char_p, [_VP]),
    "lg_train_sizes": (C.c_int, [_VP, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "lg_train_set_state": (C.c_int, [_VP, _FP, _FP, _FP, _FP, C.c_int64]),
    "lg_train_get_state": (C.c_int, [_VP, _FP, _FP, _FP, _FP, _FP, C.POINTER(C.c_int64)]),
    "lg_train_step": (C.c_int, [_VP, _VP, _VP, C.c_int, _VP, C.c_uint64, C.POINTER(LgTrainHparams), C.c_int, _FP, _FP, _VP]),
    "lg_train_epoch": (C.c_int, [_VP, _VP, _VP, C.c_int64, C.POINTER(C.c_int32), C.c_int64, C.c_int, C.c_uint64,
                                 C.POINTER(LgTrainHparams), _FP, _FP, C.POINTER(C.c_int64), _VP, C.POINTER(C.c_int32)]),
    "lg_train_epoch_plan": (C.c_int, [C.c_int64, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "lg_train_sync": (C.c_int, [_VP]),
    "lg_train_grad_buffer": (C.c_int, [_VP, C.POINTER(_FP), C.POINTER(C.c_int64)]),
    "lg_train_apply": (C.c_int, [_VP, C.POINTER(LgTrainHparams), _FP]),
    "lg_clahe": (C.c_int, [_VP, _VP, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, _VP, _VP]),
    "lg_detect_midrib": (C.c_int, [_VP, _VP, C.c_int, _VP, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32),
                                   C.POINTER(C.c_int32), _VP]),
    "lg_cnn_load_from_trainer": (C.c_int, [_VP, _VP]),
    "lg_eval_logits": (C.c_int, [_VP, _VP, _VP, C.c_int, C.c_int, C.c_double, C.c_float, C.POINTER(LgEvalResult), _VP]),
    "lg_eval_logits_host": (C.c_int, [_FP, _FP, C.c_int, C.c_int, C.c_double, C.c_float, C.POINTER(LgEvalResult)]),
    "lg_cnn_evaluate": (C.c_int, [_VP, _VP, _VP, C.c_int, C.c_int, C.c_double, C.c_float, _VP, C.POINTER(LgEvalResult), _VP]),
    "lg_debug_cnn_weights": (C.c_int, [_VP, C.c_int, C.c_int, _FP, C.c_int64, C.POINTER(C.c_int64)]),
    "lg_midrib_walk": (C.c_int, [_VP, _VP, C.c_int, C.c_int, C.c_int, _FP, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
}


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  This package has no CPU fallback.")
    # PyTorch-ROCm ships its own libamdhip64 and every device pointer this package passes comes from torch: torch must be
    # the one that brings the HIP runtime into the process.  Loaded the other way round, liblgrasp.so binds the system
    # runtime in /opt/rocm, torch then loads its bundled copy, and the second runtime finds no device
    # ("lg_create: hipGetDeviceCount -> no ROCm-capable device is detected").
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the library does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    return lib


lib = _load()


class LgError(RuntimeError):
    pass


def check(handle, rc, what):
    if rc == LG_ERR_BUSY:
        raise LgError(f"{what}: another thread is inside a call on this handle (one call in flight per selector instance)")
    if rc != LG_OK:
        msg = lib.lg_last_error(handle if handle else None).decode()   # NULL handle: the reason lg_create failed
        raise LgError(f"{what} failed with status {rc}: {msg}")


def default_params():
    p = LgParams()
    lib.lg_default_params(C.byref(p))
    return p
