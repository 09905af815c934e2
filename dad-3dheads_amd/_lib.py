"""ctypes binding of libdad3d_hip.so (the C ABI declared in include/dad3d.h).

There is NO CPU fallback: if the library is missing or a call fails, the caller gets an exception.
Build it with `python __graft_entry__.py build` (or `make -C dad-3dheads_amd/csrc`).
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DAD3D_LIB_PATH") or os.path.join(_HERE, "libdad3d_hip.so")  # override: diagnostics builds

OK, E_INVALID, E_HIP, E_UNSUPPORTED, E_NOMEM = range(5)
ZERO_ROTATION, TO_2D, MUTATE_PARAMS, FLIP_Z, COMPAT_CROSS_B3 = 0x1, 0x2, 0x4, 0x8, 0x10
NORMAL_ACCUMULATE = 0x1
PLAN_GET_NORMAL, PLAN_PHONG, PLAN_RENDER = 0, 1, 2
FORM_REFUSED, FORM_TABLE, FORM_LDS, FORM_GLOBAL = 0, 1, 2, 3
TEX_INDEX_CORNER, TEX_INDEX_REFERENCE = 0, 1
DTYPE_F32, DTYPE_U8 = 0, 1
EVAL_SELF_EXCLUDE, EVAL_MAX_K, EVAL_MAX_HEAD, EVAL_MAX_ANCHORS = 0x1, 8, 4096, 8
HEATMAP_RAW, HEATMAP_UINT8, HEATMAP_FLOAT = 0, 1, 2
OBJ_MAX_LINE_BYTES, OBJ_FLAG_NONFINITE, OBJ_FLAG_LARGE = 71, 0x1, 0x2
JSON_MAX_NUMBER_BYTES, JSON_MAX_LITERAL_BYTES, JSON_FLAG_NONFINITE = 23, 64, 0x1
JSON_PARSE_TILE_BYTES, JSON_PARSE_RECORD_INTS = 4096, 6
(JSON_PARSE_FLAG_GRAMMAR, JSON_PARSE_FLAG_DIGITS, JSON_PARSE_FLAG_BIG_INT, JSON_PARSE_FLAG_SUBNORMAL, JSON_PARSE_FLAG_OVERFLOW,
 JSON_PARSE_FLAG_AMBIGUOUS) = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20
(ANNOTATION_FLAG_GRAMMAR, ANNOTATION_FLAG_KEYS, ANNOTATION_FLAG_SHAPE, ANNOTATION_FLAG_NUMBER, ANNOTATION_FLAG_STRING,
 ANNOTATION_FLAG_RANGE) = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20
ANNOTATION_MAX_BACKSLASH_RUN, ANNOTATION_MAX_WORD_BYTES, ANNOTATION_MAX_KEY_BYTES, ANNOTATION_MAX_KEYS = 64, 32, 64, 128
PNG_SEGMENT_BYTES, ZLIB_SECOND_DISTANCE, PNG_FLAG_INTERNAL, DEFLATE_HEADER_BYTES = 8192, 4, 0x1, 640
PNG_DECODE_DESC_INTS, ZLIB_DECODE_DESC_INTS, PNG_DECODE_INFO_SEGMENTED = 12, 4, 0x1
PNG_DECODE_FLAG_MALFORMED, PNG_DECODE_FLAG_UNSUPPORTED, PNG_DECODE_FLAG_OVERFLOW = 0x1, 0x2, 0x4
JPEG_DECODE_DESC_INTS, JPEG_DECODE_GRID_INTS, JPEG_DECODE_FLAG_MALFORMED, JPEG_DECODE_FLAG_UNSUPPORTED = 12, 3, 0x1, 0x2
JPEG_DECODE_SYNC_DESC_INTS, JPEG_DECODE_SYNC_GRID_INTS = 16, 4
JPEG_DECODE_SYNC_MODE_SEGMENTS, JPEG_DECODE_SYNC_MODE_VERIFIED, JPEG_DECODE_SYNC_MODE_SERIAL = 0, 1, 2
JPEG_ENCODE_FLAG_INTERNAL = 0x1
OVERLAY_MAX_COORD = 8192
DTYPE_F16, DTYPE_BF16, HEATMAP_DTYPE_U8 = 1, 2, 3
LAYOUT_NCHW, LAYOUT_NHWC = 0, 1
POINTS_SRC_XY_F32, POINTS_SRC_YX_I32 = 0, 1
BOX_DTYPE_I32, BOX_DTYPE_I64, BOX_DTYPE_F32, BOX_DTYPE_F64 = 0, 1, 2, 3
PREPROCESS_OUT_F32_NCHW, PREPROCESS_OUT_F16_NHWC, PREPROCESS_OUT_BF16_NHWC = 0, 1, 2
BOX_FLAG_EMPTY, BOX_FLAG_COLLAPSED, BOX_FLAG_RANGE = 0x1, 0x2, 0x4
TRACK_FLAG_PREVIOUS, TRACK_FLAG_RANGE, TRACK_FLAG_NONFINITE, TRACK_FLAG_SMALL, TRACK_FLAG_OUTSIDE = 0x1, 0x2, 0x4, 0x8, 0x10
TRACK_FLAG_DUPLICATE, TRACK_MAX_SLOTS = 0x20, 1024
TRACK_FLAG_RETIRED, TRACK_MAX_DETECTIONS = 0x40, 1024
ASSIGN_FLAG_PADDING, ASSIGN_FLAG_INVALID, ASSIGN_FLAG_COVERED, ASSIGN_FLAG_SPAWNED, ASSIGN_FLAG_FULL = 0x1, 0x2, 0x4, 0x8, 0x10
FRAME_FLAG_INDEX, FRAME_FLAG_CAPACITY, FRAME_MAX_TILES, FRAME_MAX_COUNT = 0x1, 0x2, 4096, 65535
RENDER_REVERSE, RENDER_CLEAR = 1, 2
BAKE_FLAG_INDEX, BAKE_FLAG_DEPTH_WINDOW, BAKE_FLAG_NONFINITE, BAKE_MAX_DEPTH_SIDE = 0x1, 0x2, 0x4, 4096
POSE_FLAG_NONFINITE, POSE_FLAG_DEGENERATE, POSE_FLAG_GIMBAL, POSE_FLAG_INDEX = 0x1, 0x2, 0x4, 0x8
HEADS_MAX, HEAD_ACT_NONE, HEAD_ACT_RELU, HEAD_ACT_TANH = 4, 0, 1, 2
KERNEL_AUTO, KERNEL_TWO_ROLE, KERNEL_PIPELINED, KERNEL_SPLIT_BF16, KERNEL_SPLIT_F16 = 0, 1, 2, 3, 4


class Dad3dError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(f"libdad3d_hip status {status}: {message}")
        self.status = status


class UnsupportedError(Dad3dError):
    pass


class FlameModelC(C.Structure):
    _fields_ = [
        ("n_verts", C.c_int32),
        ("n_betas", C.c_int32),
        ("n_joints", C.c_int32),
        ("v_template", C.c_void_p),
        ("shapedirs", C.c_void_p),
        ("posedirs", C.c_void_p),
        ("j_regressor", C.c_void_p),
        ("parents", C.c_void_p),
        ("lbs_weights", C.c_void_p),
    ]


class FlameConstsC(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("shape", "expression", "jaw", "rotation", "eyeballs", "neck", "translation", "scale")]


class LightC(C.Structure):
    _fields_ = [
        ("intensity_ambient", C.c_float),
        ("intensity_directional", C.c_float),
        ("intensity_specular", C.c_float),
        ("specular_exp", C.c_float),
        ("color_ambient", C.c_float * 3),
        ("color_directional", C.c_float * 3),
        ("light_pos", C.c_float * 3),
        ("view_pos", C.c_float * 3),
    ]


class HeadDescC(C.Structure):
    _fields_ = [
        ("w1", C.c_void_p),
        ("b1", C.c_void_p),
        ("w2", C.c_void_p),
        ("b2", C.c_void_p),
        ("dst", C.c_void_p),
        ("dst_row_stride", C.c_int64),
        ("dst_col_offset", C.c_int64),
        ("hidden", C.c_int32),
        ("out_dim", C.c_int32),
        ("act", C.c_int32),
        ("limit", C.c_float),
    ]


# name -> (restype, argtypes); mirrors include/dad3d.h one to one
_P, _I, _U, _F = C.c_void_p, C.c_int, C.c_uint, C.c_float
SIGNATURES = {
    "dad3d_last_error": (C.c_char_p, []),
    "dad3d_clear_error": (None, []),
    "dad3d_version": (_I, []),
    "dad3d_build_info": (C.c_char_p, []),
    "dad3d_device_count": (_I, []),
    "dad3d_flame_create": (_I, [C.POINTER(FlameModelC), C.POINTER(FlameConstsC), _F, _I, C.POINTER(_P)]),
    "dad3d_flame_destroy": (None, [_P]),
    "dad3d_flame_fork": (_I, [_P, C.POINTER(_P)]),
    "dad3d_flame_num_params": (_I, [_P]),
    "dad3d_flame_num_verts": (_I, [_P]),
    "dad3d_flame_set_landmarks": (_I, [_P, _P, _I]),
    "dad3d_flame_num_landmarks": (_I, [_P]),
    "dad3d_flame_num_landmark_vertices": (_I, [_P]),
    "dad3d_flame_decode": (_I, [_P, _P, _I, _U, _P, _P, _P, _P, _P]),
    "dad3d_flame_decode_posed": (_I, [_P, _P, _I, _U, _P, _P, _P, _P]),
    "dad3d_flame_decode_backward": (_I, [_P, _I, _U, _P, _P, _P, _P, _P, _P, _P]),
    "dad3d_flame_grad_inputs": (_I, [_P, _P, _I, _P, _P]),
    "dad3d_flame_num_chain_inputs": (_I, [_P]),
    "dad3d_flame_pose_chain": (_I, [_P, _P, _I, _P, _P, _P]),
    "dad3d_flame_pose_chain_backward": (_I, [_P, _P, _I, _P, _P, _P, _P]),
    "dad3d_flame_decode_host": (_I, [_P, _P, _I, _U, _P, _P, _P, _P]),
    "dad3d_flame_readjust_params": (_I, [_P, _P, _I, _P, _F, _F, _F, _P]),
    "dad3d_flame_profile_begin": (_I, [_P, _P]),
    "dad3d_flame_profile_end": (_I, [_P, _P, C.POINTER(C.c_double), C.POINTER(_I)]),
    "dad3d_flame_select_kernel": (_I, [_P, _I]),
    "dad3d_flame_handoff_timeouts": (_I, [_P, C.POINTER(C.c_uint)]),
    "dad3d_flame_debug_trace": (_I, [_P, _P, C.c_uint64]),
    "dad3d_flame_debug_trace_entries": (C.c_uint64, [_P, _I]),
    "dad3d_mesh_create": (_I, [_P, _I, _I, _I, C.POINTER(_P)]),
    "dad3d_mesh_destroy": (None, [_P]),
    "dad3d_mesh_get_normal": (_I, [_P, _P, _P, _I, _U, _P]),
    "dad3d_mesh_get_tri_normal": (_I, [_P, _P, _P, _I, _I, _P]),
    "dad3d_mesh_get_ver_normal": (_I, [_P, _P, _P, _I, _U, _P]),
    "dad3d_mesh_rasterize": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _F, _I, _P]),
    "dad3d_mesh_rasterize_triangles": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "dad3d_mesh_phong_light": (_I, [_P, _P, _P, _P, _I, C.POINTER(LightC), _P]),
    "dad3d_mesh_normal_phong_light": (_I, [_P, _P, _P, _P, _I, C.POINTER(LightC), _P]),
    "dad3d_mesh_render": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, C.POINTER(LightC), _I, _P]),
    "dad3d_mesh_rasterize_frames": (_I, [_P, _P, _P, _I, _P, _P, _P, _I, _I, _P, _P]),
    "dad3d_mesh_render_frames": (_I, [_P, _P, _P, _I, _P, _P, _P, _I, C.POINTER(LightC), _I, _P, _P]),
    "dad3d_mesh_render_texture_frames": (_I, [_P, _P, _P, _I, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _I, _P, _P]),
    "dad3d_mesh_frames_scratch_bytes": (_I, [_P, C.POINTER(C.c_size_t)]),
    "dad3d_mesh_normal_plan": (_I, [_P, _I, _I, _I, _I, C.POINTER(_I), C.POINTER(_I), C.POINTER(_I)]),
    "dad3d_mesh_debug_trace": (_I, [_P, _P]),
    "dad3d_mesh_set_texcoords": (_I, [_P, _P, _I, _I, _P]),
    "dad3d_mesh_render_texture": (_I, [_P, _P, _I, _P, _P, _I, _I, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "dad3d_project_vertices": (_I, [_P, _P, _P, _P, _I, _I, _P, _P, _P, _I, _P]),
    "dad3d_gt_keypoints": (_I, [_P, _P, _P, _P, _I, _I, _P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _I, _P]),
    "dad3d_preprocess_images": (_I, [_P, _I, _I, C.POINTER(C.c_float), C.POINTER(C.c_float), _P, _I, _P]),
    "dad3d_nhwc_bias_act": (_I, [_P, _P, _P, C.c_int64, _I, _I, _I, _I, _P]),
    "dad3d_nhwc_resize_sum": (_I, [_P, _I, _I, _I, _I, _I, _I, C.POINTER(_P), C.POINTER(_I), C.POINTER(_I), C.POINTER(C.c_float), _I, _P]),
    "dad3d_nhwc_fusion_concat": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "dad3d_nhwc_bias_mul": (_I, [_P, _P, _P, C.c_int64, _I, _I, _I, _P]),
    "dad3d_regression_heads": (_I, [_P, _I, _I, _I, _I, C.POINTER(HeadDescC), _I, _P, _P, _P, _I, _P]),
    "dad3d_heatmap_argmax": (_I, [_P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _I, _P]),
    "dad3d_points_readjust": (_I, [_P, _I, _I, _I, _F, _F, _P, _I, _I, C.c_double, _P, _I, _P]),
    "dad3d_preprocess_boxes": (_I, [_P, _I, _P, _I, _P, _I, C.POINTER(C.c_double), _I, C.POINTER(C.c_float), C.POINTER(C.c_float), _I, _P, _P, _P, _P,
                                    _I, _P]),
    "dad3d_flame_readjust_params_frame": (_I, [_P, _P, _I, _P, _P]),
    "dad3d_points_readjust_frame": (_I, [_P, _I, _I, _I, _F, _F, _P, _P, _I, _P]),
    "dad3d_boxes_from_heads": (_I, [_P, _I, _I, C.c_int64, _I, _P, _I, _P, _I, _P, _P, _I, C.c_double, _P, _P, _I, _P]),
    "dad3d_one_euro_rows": (_I, [_P, C.c_int64, _P, C.c_int64, _I, _I, _P, _P, _P, _F, _F, _F, _P, _P, _P, _I, _P]),
    "dad3d_track_suppress_duplicates": (_I, [_P, _P, _P, _I, C.c_double, _I, _P]),
    "dad3d_track_assign_detections": (_I, [_P, _P, _P, _P, _I, _P, _P, _P, _I, _P, _I, C.c_double, _I, _I, _P, _P, _P, _I, _P]),
    "dad3d_cube_region_loss": (_I, [_P, _P, _I, _I, _P, _P, _P, _I, _P, _P, _P, _I, _P, _P, _P, _I, _P]),
    "dad3d_point_loss_terms": (_I, [_I]),
    "dad3d_weighted_point_loss": (_I, [_P, _P, _I, _I, _I, _P, _F, _I, _P, _P, _I, _P]),
    "dad3d_eval_nearest": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _I, _P]),
    "dad3d_eval_z5_ranks": (_I, [_P, _P, _I, _I, C.POINTER(C.c_int32), _I, _P, _P, _I, _P]),
    "dad3d_heatmap_encode": (_I, [_P, _I, _P, _P, _I, _I, _F, _I, _I, _P, _P, _I, _P]),
    "dad3d_heatmap_iou": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _I, _P]),
    "dad3d_heatmap_iou_grad": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P, _I, _P]),
    "dad3d_visibility_point_loss": (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _P, _I, _P]),
    "dad3d_keypoint_errors": (_I, [_P, _P, _I, _I, _I, _P, _I, _P, _F, _F, _I, _P, C.POINTER(C.c_double), _I, _I, _P, _P, _P, _I, _P]),
    "dad3d_uvmap_create": (_I, [_P, _I, _I, _P, _P, _P, _I, _I, _I, C.POINTER(_P)]),
    "dad3d_uvmap_destroy": (None, [_P]),
    "dad3d_uvmap_size": (_I, [_P]),
    "dad3d_uvmap_vertex_normals": (_I, [_P, _P, _P, _I, _P]),
    "dad3d_uvmap_bake": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "dad3d_uvmap_bake_frames": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _P, _I, _P, _P]),
    "dad3d_uvmap_depth_frames": (_I, [_P, _P, _P, _P, _P, _P, _I, _P, _I, _I, _P, _P]),
    "dad3d_uvmap_bake_frames_occluded": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _P, _I, _P, _P, _P, _I, C.c_double, C.c_double, _P, _P]),
    "dad3d_obj_format_scratch_bytes": (C.c_size_t, [_I, _I]),
    "dad3d_obj_format_vertices": (_I, [_P, _I, _I, _P, C.c_size_t, _P, _P, _P, C.c_size_t, _I, _P]),
    "dad3d_json_format_scratch_bytes": (C.c_size_t, [_I, _I]),
    "dad3d_json_format_values": (_I, [_P, _I, _I, _P, _P, _P, C.c_size_t, _P, _P, _P, C.c_size_t, _I, _P]),
    "dad3d_json_number_host": (_I, [_P, C.c_size_t, _P, C.c_size_t, _P]),
    "dad3d_json_parse_scratch_bytes": (C.c_size_t, [C.c_int64]),
    "dad3d_json_parse_index": (_I, [_P, C.c_int64, _P, C.c_size_t, _P, _I, _P]),
    "dad3d_json_parse_lists": (_I, [_P, C.c_int64, _P, C.c_size_t, _P, _P, C.c_int64, _P, _P, _P, _P, C.c_int64, _I, _P]),
    "dad3d_json_parse_check_arrays": (_I, [_P, C.c_int64, _P, _P, C.c_int64, _P, _P, _P, C.c_int64, _P, _P, _P, C.c_int64, _I, _P]),
    "dad3d_json_parse_extract": (_I, [_P, C.c_int64, _P, C.c_int64, _P, C.c_int64, C.c_int64, _P, _P, C.c_int64, _I, _P]),
    "dad3d_json_parse_number_host": (_I, [_P, _P, _P, C.c_size_t, _P, _P, _P]),
    "dad3d_annotation_parse": (_I, [_P, C.c_int64, _P, _P, _I, _I, _P, _P, _P, _P, _I, _P]),
    "dad3d_png_max_bytes": (C.c_size_t, [_I, _I, _I]),
    "dad3d_png_scratch_bytes": (C.c_size_t, [_I, _I, _I, _I]),
    "dad3d_png_encode": (_I, [_P, _I, _I, _I, _I, _P, C.c_size_t, _P, _P, _P, C.c_size_t, _I, _P]),
    "dad3d_zlib_max_bytes": (C.c_size_t, [C.c_int64]),
    "dad3d_zlib_scratch_bytes": (C.c_size_t, [_I, C.c_int64]),
    "dad3d_zlib_compress": (_I, [_P, _I, C.c_int64, _P, C.c_size_t, _P, _P, _P, C.c_size_t, _I, _P]),
    "dad3d_deflate_tables_host": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "dad3d_png_decode_scratch_bytes": (C.c_size_t, [_P, _I, _P]),
    "dad3d_png_decode": (_I, [_P, C.c_size_t, _P, _I, _I, _P, C.c_size_t, _P, _P, _P, C.c_size_t, _I, _I, _P]),
    "dad3d_zlib_decompress": (_I, [_P, C.c_size_t, _P, _I, _P, C.c_size_t, _P, _P, _I, _P]),
    "dad3d_inflate_host": (_I, [_P, _P, _I, _P, C.c_int64, _P, _P]),
    "dad3d_jpeg_decode_scratch_bytes": (C.c_size_t, [_P, _I, _P]),
    "dad3d_jpeg_decode": (_I, [_P, C.c_size_t, _P, _I, _P, _P, C.c_size_t, _P, _P, C.c_size_t, _I, _P]),
    "dad3d_jpeg_decode_host": (_I, [_P, C.c_int64, _I, _P, C.c_int64, _P, _P, _P, _P]),
    "dad3d_jpeg_decode_sync_scratch_bytes": (C.c_size_t, [_P, _I, _P, _I]),
    "dad3d_jpeg_decode_sync": (_I, [_P, C.c_size_t, _P, _I, _P, _I, _P, C.c_size_t, _P, _P, _P, C.c_size_t, _I, _P]),
    "dad3d_jpeg_decode_sync_host": (_I, [_P, C.c_int64, _I, _I, _P, C.c_int64, _P, _P, _P, _P, _P]),
    "dad3d_jpeg_max_bytes": (C.c_size_t, [_I, _I, _I, _I]),
    "dad3d_jpeg_encode_scratch_bytes": (C.c_size_t, [_I, _I, _I, _I, _I]),
    "dad3d_jpeg_encode": (_I, [_P, _I, _I, _I, _I, _I, _I, _I, _P, C.c_size_t, _P, _P, _P, C.c_size_t, _I, _P]),
    "dad3d_jpeg_encode_host": (_I, [_P, _I, _I, _I, _I, _I, _I, _P, C.c_int64, _P, _P]),
    "dad3d_overlay_segments": (_I, [_P, _P, _I, _I, _I, _P, _I, _P, _I, _P, _U, _I, _I, _P]),
    "dad3d_overlay_discs": (_I, [_P, _P, _I, _I, _I, _P, _I, _P, _I, _I, _U, _I, _P]),
    "dad3d_head_pose": (_I, [_P, _I, C.c_int64, _I, _P, _I, _P, _I, _I, _P, _P, _P, _P, _I, _P]),
    "dad3d_head_pose_host": (_I, [_P, _I, C.c_int64, _I, _P, _I, _P, _I, _I, _P, _P, _P, _P]),
    "dad3d_procrustes": (_I, [_P, _P, _I, _I, _P, _P, _P, _P, _I, _P]),
    "dad3d_procrustes_host": (_I, [_P, _P, _I, _I, _P, _P, _P, _P]),
    "dad3d_sim3dr_get_tri_normal": (None, [_P, _P, _P, _I, _I]),
    "dad3d_sim3dr_get_ver_normal": (None, [_P, _P, _P, _I, _I]),
    "dad3d_sim3dr_get_normal": (None, [_P, _P, _P, _I, _I]),
    "dad3d_sim3dr_rasterize_triangles": (None, [_P, _P, _P, _P, _P, _I, _I, _I]),
    "dad3d_sim3dr_rasterize": (None, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _F, _I]),
}

_lib = None


def load() -> C.CDLL:
    """Load the HIP library or raise. Never falls back to a CPU implementation."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: the HIP extension has not been built "
            "(run `python __graft_entry__.py build`). There is no CPU fallback."
        )
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(status: int) -> None:
    if status != OK:
        msg = load().dad3d_last_error().decode("utf-8", "replace")
        raise (UnsupportedError if status == E_UNSUPPORTED else Dad3dError)(status, msg)


def require_gpu() -> None:
    if load().dad3d_device_count() < 1:
        raise RuntimeError("no HIP device visible: the dad-3dheads_amd hot path runs on an MI355X only (no CPU fallback)")
