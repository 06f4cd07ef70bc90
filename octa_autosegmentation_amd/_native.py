"""ctypes binding of liboctahip.so (include/octa_hip.h). Fails loudly when the library is missing."""
import contextlib
import ctypes
import os
import random as _random
import threading

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("OCTA_HIP_LIB") or os.path.join(HERE, "liboctahip.so")    # OCTA_HIP_LIB: experiment builds (tools/build_sim_variant.py)

_lib = None
_ctxs = {}
_lock = threading.Lock()

c_void_p, c_int, c_double, c_size_t = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_size_t


def _struct(name, ints, ptrs):
    """ctypes mirror of an argument struct of include/octa_hip.h: uint32 struct_size, the int fields, float slope, the pointer fields."""
    fields = [("struct_size", ctypes.c_uint32)] + [(k, c_int) for k in ints.split()] + [("slope", ctypes.c_float)] + [(k, c_void_p) for k in ptrs.split()]
    return type(name, (ctypes.Structure,), {"_fields_": fields})


# zero = absent, except stride / in_dilation / tap_mask / out_scale: no hidden default, the plain layer is 1 / 1 / 0x1ff / 1
Conv3x3Args = _struct("Conv3x3Args", "N H W Cin Cout stride in_dilation tap_mask out_scale out_off_y out_off_x C1 CY1 nslot",
                      "d_x d_x2 d_w d_y d_y2 d_scale1 d_shift1 d_scale2 d_shift2 d_stat_partials d_stat_slots d_residual")
Conv3x3WgradArgs = _struct("Conv3x3WgradArgs", "N H W Cin Cout stride tap_mask C1 out_mode", "d_x d_x2 d_dy d_dw d_scale1 d_shift1 d_scale2 d_shift2")
WGRAD_TAP_MAJOR, WGRAD_PARAM_ADD, WGRAD_PARAM_SET = 0, 1, 2     # out_mode

# symbol -> (restype, argtypes); must list every function include/octa_hip.h declares
SIGNATURES = {
    "octa_abi_version": (c_int, []),
    "octa_last_error": (ctypes.c_char_p, []),
    "octa_ctx_create": (c_int, [c_int, ctypes.POINTER(c_void_p)]),
    "octa_ctx_destroy": (None, [c_void_p]),
    "octa_ctx_scratch_bytes": (c_size_t, [c_void_p]),
    "octa_rasterize_2d": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_double,
                                  c_double, c_void_p, c_void_p]),
    "octa_rasterize_2d_plan": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_double, c_double, c_void_p]),
    "octa_rasterize_2d_draw": (c_int, [c_void_p, c_void_p, c_void_p]),
    "octa_raster_prof": (c_int, [c_void_p, c_void_p]),
    "octa_fs_dither": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "octa_voxel_padded_dims": (c_int, [c_void_p, c_void_p]),
    "octa_voxelize_3d": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_double, c_double, c_int, c_void_p, c_void_p]),
    "octa_edges_read_back": (c_int, [c_void_p, c_void_p, c_void_p, ctypes.c_int64, c_void_p, c_void_p]),
    "octa_max_u8": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "octa_bif_native_init": (c_int, [ctypes.c_char_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "octa_bif_native": (None, [c_int, c_void_p, c_void_p, c_void_p]),
    "octa_bif_native_counts": (c_int, [c_void_p]),
    "octa_instnorm_lrelu_fwd": (c_int, [c_void_p] * 7 + [c_int, c_int, ctypes.c_int64, c_int, ctypes.c_float, ctypes.c_float, c_void_p]),
    "octa_instnorm_lrelu_bwd": (c_int, [c_void_p] * 10 + [c_int, c_int, ctypes.c_int64, c_int, ctypes.c_float, c_void_p]),
    "octa_csv_bytes_bound": (ctypes.c_int64, [ctypes.c_int64]),
    "octa_csv_format_edges": (ctypes.c_int64, [c_void_p, ctypes.c_int64, c_void_p, ctypes.c_int64]),
    "octa_csv_write_file": (c_int, [ctypes.c_char_p, c_void_p, ctypes.c_int64]),
    "octa_csv_count_rows": (ctypes.c_int64, [c_void_p, ctypes.c_int64]),
    "octa_csv_parse_edges": (ctypes.c_int64, [c_void_p, ctypes.c_int64, c_void_p, ctypes.c_int64]),
    "octa_py_random_advance": (c_int, [c_void_p, ctypes.c_int64]),
    "octa_png_write_gray8": (c_int, [ctypes.c_char_p, c_void_p, c_int, c_int, c_int]),
    "octa_png_write_bits": (c_int, [ctypes.c_char_p, c_void_p, c_int, c_int, c_int]),
    "octa_write_sample_files": (c_int, [ctypes.c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int,
                                        ctypes.c_char_p, ctypes.c_int64, c_int, c_int]),
    "octa_pack_bits": (c_int, [c_void_p, c_void_p, c_void_p, ctypes.c_int64, c_int, c_void_p]),
    "octa_background_noise": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_int64, c_void_p, c_void_p, c_void_p]),
    "octa_speckle_brightness": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "octa_menten_vessel_noise": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_double, c_double, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "octa_menten_floater_mask": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "octa_menten_floater": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "octa_menten_motion": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "octa_noise_model": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, ctypes.c_uint64, ctypes.c_uint32, c_double, c_double, c_double,
                                 c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "octa_noise_model_backward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, ctypes.c_uint64, ctypes.c_uint32,
                                          c_double, c_double, c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "octa_philox4x32_10": (None, [c_void_p, c_void_p, c_void_p]),
    "octa_sim_create": (c_int, [c_void_p, c_void_p, c_int, ctypes.POINTER(c_void_p)]),
    "octa_sim_create_ex": (c_int, [c_void_p, c_void_p, c_int, c_int, ctypes.POINTER(c_void_p)]),
    "octa_sim_destroy": (None, [c_void_p]),
    "octa_sim_run": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "octa_sim_run_states": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "octa_sim_np_state": (c_int, [c_void_p, c_int, c_void_p]),
    "octa_thinconv_expand": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, ctypes.c_float, c_void_p]),
    "octa_thinconv_squeeze": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "octa_lrelu_bwd_bf16": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_int64, ctypes.c_float, c_void_p]),
    "octa_thinconv_wgrad_scratch_floats": (ctypes.c_longlong, [c_int, c_int, c_int, c_int]),
    "octa_thinconv_wgrad": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "octa_sim_spans": (c_int, [c_void_p, c_void_p]),
    "octa_sim_edge_offsets": (c_int, [c_void_p, c_void_p, c_void_p]),
    "octa_sim_export_edges": (c_int, [c_void_p, c_void_p]),
    "octa_sim_export_edges_device": (c_int, [c_void_p, c_void_p, c_void_p]),
    "octa_sim_trace": (c_int, [c_void_p, c_void_p]),
    "octa_sim_stats": (c_int, [c_void_p, c_void_p]),
    "octa_sim_kd_paths": (c_int, [c_void_p, c_void_p]),
    "octa_sim_assign_paths": (c_int, [c_void_p, c_void_p]),
    "octa_sim_timing": (c_int, [c_void_p, c_void_p]),
    "octa_sim_service_stats": (c_int, [c_void_p, c_void_p]),
    "octa_sim_geometry": (c_int, [c_int, c_void_p]),
    "octa_sim_is_large": (c_int, [c_void_p]),
    "octa_conv2d_f32_nchw": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p] + [c_int] * 14 + [c_void_p]),
    "octa_convtranspose2x2_f32_nchw": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "octa_conv2d_f32_dgrad_nchw": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p] + [c_int] * 11 + [c_void_p]),
    "octa_conv2d_f32_wgrad_workspace": (c_int, [c_int] * 10 + [ctypes.POINTER(c_size_t)]),
    "octa_conv2d_f32_wgrad_nchw": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t] + [c_int] * 10 + [c_void_p]),
    "octa_sim_fields": (c_int, [c_void_p, c_int, c_void_p, ctypes.c_int64, c_void_p, c_void_p, ctypes.c_int64, c_void_p]),
    "octa_instnorm_lrelu_nhwc_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, ctypes.c_int64, ctypes.c_float, c_void_p]),
    "octa_pack_conv_weights": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "octa_head1_nhwc_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "octa_instnorm_nhwc_stats": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, ctypes.c_int64, ctypes.c_float, c_void_p]),
    "octa_scale_shift_lrelu_nhwc": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, ctypes.c_int64, ctypes.c_float, c_void_p]),
    "octa_resize_bilinear": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "octa_resize_bilinear_bwd": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "octa_flip_rot90_rotate": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, ctypes.c_float, c_int, c_void_p]),
    "octa_flip_rot90_rotate_window": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, ctypes.c_float, c_int, c_int, c_int,
                                              c_void_p, c_void_p, c_void_p]),
    "octa_remove_small_objects": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, ctypes.c_uint8, c_void_p, c_void_p]),
    "octa_cc3d_filter": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, ctypes.c_uint8, c_void_p, c_void_p, c_void_p]),
    "octa_skeletonize": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, ctypes.POINTER(c_int), c_void_p]),
    "octa_reflect_pad_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "octa_reflect_pad_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "octa_blur_down_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "octa_blur_down_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "octa_blur_up_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "octa_blur_up_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "octa_conv4x4_nhwc_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "octa_conv4x4_nhwc_wgrad": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "octa_dice_bce_fwd": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, ctypes.c_int64, c_void_p, c_void_p]),
    "octa_dice_bce_finish": (c_int, [c_void_p, c_void_p, c_int, ctypes.c_int64, c_double, c_double, c_void_p, c_void_p]),
    "octa_dice_bce_bwd": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, ctypes.c_int64, c_void_p, c_void_p, ctypes.c_float, ctypes.c_float, c_void_p, c_void_p]),
    "octa_l1_pairs_fwd": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "octa_l1_pairs_finish": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "octa_l1_pairs_bwd": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "octa_lsgan_fwd": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "octa_lsgan_bwd": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "octa_mix_max_fwd": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, ctypes.c_int64, c_void_p, c_void_p]),
    "octa_mix_max_bwd": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, ctypes.c_int64, c_void_p, c_void_p, c_void_p]),
    "octa_pool_exchange": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, ctypes.c_int64, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "octa_sim_launch_count": (ctypes.c_longlong, []),
    "octa_order_wait_launch": (c_int, [c_void_p, ctypes.c_longlong, c_int, c_int, c_void_p, c_void_p]),
    "octa_conv3x3_c1_wgrad": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "octa_conv_stat_tiles": (c_int, [c_int, c_int]),
    "octa_instnorm_lrelu_head1_nhwc_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, ctypes.c_int64, ctypes.c_float, c_void_p]),
    "octa_conv3x3_s2t_nhwc": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "octa_conv3x3_nhwc_fwd": (c_int, [c_void_p, ctypes.POINTER(Conv3x3Args), c_void_p]),
    "octa_conv3x3_nhwc_wgrad": (c_int, [c_void_p, ctypes.POINTER(Conv3x3WgradArgs), c_void_p]),
    "octa_conv3x3_nhwc_fwd_pad": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p]),
    "octa_conv3x3_nhwc_wgrad_pad": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "octa_instnorm_lrelu_nhwc_fwd": (c_int, [c_void_p] * 7 + [c_int, c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_float, c_void_p, c_int, c_void_p, c_int, c_void_p]),
    "octa_instnorm_lrelu_head1_nhwc_fwd": (c_int, [c_void_p] * 9 + [c_int, c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_float, c_void_p, c_int, c_void_p]),
    "octa_head1_nhwc_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_int64, c_int, c_void_p, c_void_p]),
    "octa_headn_nhwc_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, ctypes.c_int64, c_int, c_int, c_void_p, c_void_p]),
    "octa_headn_nhwc_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, ctypes.c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "octa_conv3x3_c1_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p]),
    "octa_fft2_c2c_f64_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "octa_fft2_c2c_f64": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "octa_oof_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "octa_oof_2d": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "octa_oof_2d_response": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "octa_frangi_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "octa_frangi_2d": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, ctypes.c_float, c_double, c_double, c_int, c_void_p, c_void_p]),
    "octa_frangi_hessian": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, ctypes.c_float, c_int, c_void_p, c_void_p]),
    "octa_frangi_eigenvalues": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, ctypes.c_float, c_int, c_void_p, c_void_p]),
    "octa_skr_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "octa_area_opening": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "octa_skr_filter": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "octa_sim_kat_kd_order": (c_int, [c_void_p, c_void_p, ctypes.c_int64, c_void_p, c_void_p]),
    "octa_sim_kat_kd_order_signflag": (c_int, [c_void_p, c_void_p, ctypes.c_int64, c_void_p, ctypes.c_int32, c_void_p]),
    "octa_sim_kat_sample": (c_int, [c_void_p, c_void_p, ctypes.c_int64, c_void_p, c_void_p, ctypes.c_int64, c_void_p, ctypes.c_int64, ctypes.c_int64,
                                    c_double, c_double, c_double, c_void_p, c_void_p]),
}


class OctaHipError(RuntimeError):
    pass


def lib():
    """Load liboctahip.so once. Raises if it has not been built (no fallback path exists)."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise OctaHipError(
                        f"{LIB_PATH} is missing: build it with `python -m octa_autosegmentation_amd.build` "
                        "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
                # torch bundles its own libamdhip64 (same soname as /opt/rocm's): import it first so that
                # liboctahip.so binds to the runtime torch's allocator and streams live in.
                import torch  # noqa: F401
                l = ctypes.CDLL(LIB_PATH)
                for name, (res, args) in SIGNATURES.items():
                    fn = getattr(l, name)
                    fn.restype = res
                    fn.argtypes = args
                _lib = l
    return _lib


_SYNC_DEBUG = bool(os.environ.get("OCTA_SYNC_DEBUG"))


def check(rc, what):
    if _SYNC_DEBUG and rc == 0:     # development aid: wait for the launch and name it, so that an asynchronous fault has an owner
        import sys
        import torch
        torch.cuda.current_stream().synchronize()
        print(f"[octa-sync] {threading.current_thread().name} {what} ok", file=sys.stderr, flush=True)
    if rc != 0:
        msg = lib().octa_last_error().decode("utf-8", "replace")
        raise OctaHipError(f"{what} failed (rc={rc}): {msg}")


_tls = threading.local()


def _device_index(device_index):
    """The GPU to use (None: torch's current device); raises when torch sees none."""
    import torch
    if not torch.cuda.is_available():
        raise OctaHipError("no ROCm GPU visible to torch; the HIP path cannot run (no CPU fallback)")
    return int(torch.cuda.current_device() if device_index is None else device_index)


def _create_ctx(device_index):
    out = c_void_p()
    call("octa_ctx_create", device_index, ctypes.byref(out))
    return out


def new_ctx(device_index=None):
    """A private context (own grow-only scratch); the owner frees it with free_ctx()."""
    return _create_ctx(_device_index(device_index))


def free_ctx(h):
    if h is not None:
        lib().octa_ctx_destroy(h)


@contextlib.contextmanager
def use_ctx(h):
    """Route every ctx() lookup of the calling thread to `h` (a pipeline slot keeps its own scratch, whichever
    pool thread happens to run it)."""
    prev = getattr(_tls, "ctx", None)
    _tls.ctx = h
    try:
        yield h
    finally:
        _tls.ctx = prev


def ctx(device_index=None):
    """Context (grow-only device scratch) for one GPU, one per calling THREAD and current STREAM unless use_ctx() is active: an
    octa_ctx must not be used from two threads at once (include/octa_hip.h), pipelines keep several steps in flight from a thread
    pool, and its scratch is stream-ordered (common.h: one context = one stream at a time) -- the autograd thread runs the backward
    nodes of a step that used two streams on those two streams, interleaved (models/gan_seg_model.py)."""
    import torch
    if getattr(_tls, "ctx", None) is not None:
        return _tls.ctx
    device_index = _device_index(device_index)
    key = (device_index, threading.get_ident(), torch.cuda.current_stream(device_index).cuda_stream)
    with _lock:
        h = _ctxs.get(key)
    if h is None:
        h = _create_ctx(device_index)
        with _lock:
            _ctxs[key] = h
    return h


def current_stream_ptr():
    import torch
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def addr(t):
    """Device (or host) address of a tensor for a pointer field of an argument struct; None stays None."""
    return t.data_ptr() if t is not None else None


def _ctx_of(device):       # launch() has a parameter called ctx
    return ctx(device.index)


# The marshalling rule of launch() and call(): an argument with a data_ptr attribute (a torch tensor) becomes its address; everything
# else -- None, Python numbers, ctypes.byref(), ctypes structs, bytes, numpy `.ctypes.data` ints -- goes through untouched and the
# declared argtypes (SIGNATURES) convert it.

def launch(name, device, *args, what=None, ctx=None, stream=None):
    """Call `int name(octa_ctx*, args..., void* stream)` and check its return code. The context is the one of `device` for the
    calling thread and current stream (ctx()) and the stream is torch's current one; ctx= / stream= name another (a private context
    from new_ctx(), a stream of the caller's own). what= replaces the symbol's name in the error message."""
    argv = [_ctx_of(device) if ctx is None else ctx]
    for a in args:
        argv.append(a.data_ptr() if hasattr(a, "data_ptr") else a)
    argv.append(current_stream_ptr() if stream is None else stream)
    check(getattr(lib(), name)(*argv), what or name)


def call(name, *args, what=None):
    """Call `int name(args...)` -- an entry point that is not of launch()'s form: no context and no stream, or only one of the two,
    which then is an ordinary argument -- and check its return code. Entry points that return a VALUE are called through lib()."""
    check(getattr(lib(), name)(*[a.data_ptr() if hasattr(a, "data_ptr") else a for a in args]), what or name)


def advance_python_random(n):
    """`random.random()` n times, natively (same final state of the global generator as the Python loop)."""
    if n <= 0:
        return
    if n < 64:
        for _ in range(n):
            _random.random()
        return
    ver, state, gauss = _random.getstate()
    arr = np.array(state, dtype=np.uint32)
    call("octa_py_random_advance", arr.ctypes.data, int(n))
    _random.setstate((ver, tuple(arr.tolist()), gauss))
