"""ctypes binding of libposerisk_hip.so (the C ABI declared in include/poserisk_hip.h).

The product path has no CPU fallback: if the library is missing or fails to load, importing
any compute entry point raises.  `python -m poserisk_release_amd.build` (or
`__graft_entry__.build()`) produces the library in-tree.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# The shipped library.  POSERISK_LIB_PATH selects another build for A/B and ablation runs (scripts/ab_libs.sh builds them
# beside the tree with `python -m poserisk_release_amd.build --out ...`): nothing ever overwrites the shipped file, and
# pr_build_info() -- printed by bench.py as `library` -- says which build a record came from.
LIB_PATH = os.environ.get("POSERISK_LIB_PATH") or os.path.join(HERE, "libposerisk_hip.so")

ABI_VERSION = 16


class PoseRiskHipError(RuntimeError):
    pass


class RebaInfo(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("legs_bilateral", "sitting", "load_force", "arm_supported_l",
                                          "arm_supported_r", "coupling", "activity")]


class RulaInfo(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("arm_supported_l", "arm_supported_r", "a_muscle_l", "a_muscle_r",
                                          "a_load_l", "a_load_r", "legs_bilateral", "b_muscle", "b_load")]


class RenderArgs(C.Structure):
    """pr_render_args (include/poserisk_hip.h, the mesh overlay)."""
    _fields_ = [(n, C.c_void_p) for n in ("verts", "faces", "cam", "bboxes", "frames", "frame_idx", "face_part", "part_rgb",
                                           "out", "face_id", "vert_fx", "status")] + \
               [(n, C.c_int) for n in ("N", "V", "F", "P", "n_frames", "H", "W", "bgr")] + \
               [("scale", C.c_float), ("alpha", C.c_float)]


class RenderPeopleArgs(C.Structure):
    """pr_render_people_args (include/poserisk_hip.h, the people mesh overlay)."""
    _fields_ = [(n, C.c_void_p) for n in ("verts", "faces", "cam", "bboxes", "frames", "canvas", "src_idx", "z_step", "face_part",
                                           "part_rgb", "out", "face_id", "vert_fx", "status", "canvas_status")] + \
               [(n, C.c_int) for n in ("N", "M", "V", "F", "P", "n_frames", "H", "W", "bgr")] + \
               [("scale", C.c_float), ("alpha", C.c_float)]


class ComposeArgs(C.Structure):
    """pr_compose_args (include/poserisk_hip.h, the annotated score video)."""
    _fields_ = [(n, C.c_void_p) for n in ("frames", "src_idx", "box", "lines", "text", "atlas", "out", "status")] + \
               [(n, C.c_int) for n in ("N", "n_frames", "H", "W", "dst_h", "dst_w", "panel_w", "L", "C", "S", "CH", "CW")] + \
               [("adv", C.c_int * 4), ("ascent", C.c_int * 4), ("box_rgb", C.c_uint8 * 4)]


class ComposePeopleArgs(C.Structure):
    """pr_compose_people_args (include/poserisk_hip.h, the people video)."""
    _fields_ = [(n, C.c_void_p) for n in ("frames", "src_idx", "box", "box_rgb", "lines", "text", "atlas", "out", "status")] + \
               [(n, C.c_int) for n in ("N", "n_frames", "H", "W", "dst_h", "dst_w", "panel_w", "K", "L", "L_img", "C", "S", "CH", "CW")] + \
               [("adv", C.c_int * 4), ("ascent", C.c_int * 4)]


class JpegArgs(C.Structure):
    """pr_jpeg_args (include/poserisk_hip.h, the JPEG decoder)."""
    _fields_ = [(n, C.c_void_p) for n in ("data", "frames", "segments", "huff", "out", "status")] + [("data_bytes", C.c_int64)] + \
               [(n, C.c_int) for n in ("F", "H", "W", "n_segments", "n_huff", "bgr")]


class JpegScansArgs(C.Structure):
    """pr_jpeg_scans_args (include/poserisk_hip.h, pr_jpeg_decode_scans)."""
    _fields_ = [("base", JpegArgs), ("scans", C.c_void_p), ("segment_scan", C.c_void_p), ("n_scans", C.c_int32), ("n_levels", C.c_int32)]


class JpegSyncOpts(C.Structure):
    """pr_jpeg_sync_opts (include/poserisk_hip.h, pr_jpeg_decode_sync): subseq_bytes 0 = the build's default; max_rounds is 1..64
    (0 is an error: pass no opts at all for both defaults)."""
    _fields_ = [("subseq_bytes", C.c_int32), ("max_rounds", C.c_int32)]


class JpegEncArgs(C.Structure):
    """pr_jpeg_enc_args (include/poserisk_hip.h, the JPEG encoder)."""
    _fields_ = [(n, C.c_void_p) for n in ("frames", "plan", "out", "nbytes", "status")] + [("capacity", C.c_int64)] + \
               [(n, C.c_int) for n in ("F", "H", "W", "hs", "vs", "restart_interval", "bgr")]


class PngArgs(C.Structure):
    """pr_png_args (include/poserisk_hip.h, the PNG decoder)."""
    _fields_ = [(n, C.c_void_p) for n in ("data", "frames", "idat", "palettes", "out", "status")] + [("data_bytes", C.c_int64)] + \
               [(n, C.c_int) for n in ("F", "H", "W", "n_idat", "n_palettes", "bgr")]


class PngEncArgs(C.Structure):
    """pr_png_enc_args (include/poserisk_hip.h, the PNG encoder)."""
    _fields_ = [(n, C.c_void_p) for n in ("frames", "plan", "out", "nbytes", "status")] + [("capacity", C.c_int64)] + \
               [(n, C.c_int) for n in ("F", "H", "W", "filter", "mode", "bgr")]


class Y4mInfo(C.Structure):
    """pr_y4m_info (include/poserisk_hip.h, the YUV4MPEG2 reader)."""
    _fields_ = [(n, C.c_int32) for n in ("width", "height", "fps_num", "fps_den", "chroma", "full_range", "header_bytes", "reserved")] + \
               [("frame_bytes", C.c_int64)]


class YuvCoeffs(C.Structure):
    """pr_yuv_coeffs (include/poserisk_hip.h, pr_yuv_plan)."""
    _fields_ = [(n, C.c_int32) for n in ("cy", "crv", "cbu", "cgu", "cgv", "yo")]


class YuvArgs(C.Structure):
    """pr_yuv_args (include/poserisk_hip.h, pr_yuv_frames)."""
    _fields_ = [(n, C.c_void_p) for n in ("data", "offsets", "dst", "xofs", "xcoef", "yofs", "ycoef")] + [("data_bytes", C.c_int64)] + \
               [("plan", YuvCoeffs)] + [(n, C.c_int) for n in ("F", "H", "W", "chroma", "bgr", "h", "w", "mode")]


class YuvEncCoeffs(C.Structure):
    """pr_yuv_enc_coeffs (include/poserisk_hip.h, pr_yuv_enc_plan)."""
    _fields_ = [(n, C.c_int32) for n in ("kyr", "kyg", "kyb", "kc", "kur", "kug", "kvb", "kvg", "yo")]


class YuvEncArgs(C.Structure):
    """pr_yuv_enc_args (include/poserisk_hip.h, pr_yuv_encode)."""
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("plan", YuvEncCoeffs)] + \
               [(n, C.c_int) for n in ("F", "H", "W", "out_H", "out_W", "chroma", "bgr")]


class DetLayer(C.Structure):
    """pr_det_layer (include/poserisk_hip.h, section j8: the detector's topology table)."""
    _fields_ = [(n, C.c_int32) for n in ("type", "cin", "cout", "ksize", "stride", "bn", "from0", "from1", "down", "cin_pad", "cout_pad",
                                          "kpad")] + [("weight_offset", C.c_int64), ("pack_offset", C.c_int64)]


class SmoothParams(C.Structure):
    """pr_smooth_params (include/poserisk_hip.h, section s1)."""
    _fields_ = [("median_radius", C.c_int32), ("reserved", C.c_int32), ("sigma", C.c_double)]


class SmoothInputs(C.Structure):
    """pr_smooth_inputs (include/poserisk_hip.h, section s1)."""
    _fields_ = [(n, C.c_void_p) for n in ("rotmat", "betas", "cam")]


class SmoothOutputs(C.Structure):
    """pr_smooth_outputs (include/poserisk_hip.h, section s1)."""
    _fields_ = [(n, C.c_void_p) for n in ("rotmat", "betas", "cam", "replaced")]


class ActivityParams(C.Structure):
    """pr_activity_params (include/poserisk_hip.h, section t1)."""
    _fields_ = [(n, C.c_int32) for n in ("hold_frames", "rapid_frames", "gap_frames", "rep_events")] + \
               [(n, C.c_double) for n in ("dot_static", "dot_move", "dot_rapid")]


class FramesOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("rotmat", "betas", "cam", "axis_angle", "euler_deg", "joint_cam",
                                           "verts", "reba", "rula", "status")]


_P = C.c_void_p
_I = C.c_int
# name -> (restype, argtypes); every symbol include/poserisk_hip.h declares
SIGNATURES = {
    "pr_last_error": (C.c_char_p, []),
    "pr_abi_version": (_I, []),
    "pr_build_info": (C.c_char_p, []),
    "pr_declare_stream": (_I, [_P, _I]),
    "pr_fence_check": (_I, [C.c_char_p, C.c_size_t]),
    "pr_fence_list": (_I, [C.c_char_p, C.c_size_t]),
    "pr_fence_payload_fill": (_I, [C.c_char_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "pr_fence_selftest": (_I, []),
    "pr_hmr_weight_floats": (C.c_size_t, []),
    "pr_hmr_create": (_I, [_I, _P, C.c_size_t, _I, _I, _I, C.POINTER(_P)]),
    "pr_hmr_destroy": (_I, [_P]),
    "pr_hmr_forward": (_I, [_P, _P, _I, _P, _P, _P, _P, _P, _P]),
    "pr_hmr_set_streams": (_I, [_P, _I]),
    "pr_hmr_set_concurrency": (_I, [_P, _I]),
    "pr_hmr_profile_enable": (_I, [_P, _I]),
    "pr_hmr_profile_read": (_I, [_P, _P, _P, _P, _P, _I]),
    "pr_hmr_num_conv_layers": (_I, []),
    "pr_hmr_conv_form": (_I, [_P]),
    "pr_hmr_plan_counts": (_I, [_P, _I, C.POINTER(_I), C.POINTER(_I)]),
    "pr_hmr_encode_until": (_I, [_P, _P, _I, _I, _P, _P]),
    "pr_hmr_regress_until": (_I, [_P, _P, _I, _I, _P, _P]),
    "pr_conv_num_tile_cfgs": (_I, []),
    "pr_conv2d_nhwc": (_I, [_I, _P, _P, _P, _P, _P] + [_I] * 14 + [_P, _P]),
    "pr_conv1x1_dual_nhwc": (_I, [_I, _P, _P, _P, _P, _P, _P] + [_I] * 12 + [_P]),
    "pr_conv3x3_conv1x1_nhwc": (_I, [_I, _P, _P, _P, _P, _P, _P, _P] + [_I] * 7 + [_P]),
    "pr_conv3x3_wino64_nhwc": (_I, [_I, _P, _P, _P, _P, _P, _P, _P] + [_I] * 9 + [_P]),
    "pr_bottleneck_nhwc": (_I, [_I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P]),
    "pr_bottleneck128_nhwc": (_I, [_I, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P]),
    "pr_bottleneck256_nhwc": (_I, [_I, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P]),
    "pr_stem_pool_nhwc": (_I, [_I, _P, _P, _P, _P, _I, _I, _I, _P, _P]),
    "pr_stem_pool_f32_nhwc": (_I, [_I, _P, _P, _P, _P, _I, _I, _P, _P]),
    "pr_crop_frames": (_I, [_P, _I, _I, _I, _I, _P, _P, _I, C.c_float, _P, _P, _P]),
    "pr_rot6d_to_rotmat": (_I, [_P, _I, _P, _P]),
    "pr_pose_to_euler": (_I, [_P, _I, _P, _P, _P, _P]),
    "pr_axis_angle_to_euler": (_I, [_P, _I, _P, _P, _P]),
    "pr_smpl_create": (_I, [_I, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, C.POINTER(_P)]),
    "pr_smpl_destroy": (_I, [_P]),
    "pr_smpl_forward": (_I, [_P, _P, _P, _P, _I, _I, _P, _P, _P]),
    "pr_smpl_joint_cam": (_I, [_P, _P, _I, _P, _P, _P]),
    "pr_reba": (_I, [_P, _I, C.POINTER(RebaInfo), _P, _P]),
    "pr_rula": (_I, [_P, _I, C.POINTER(RulaInfo), _P, _P]),
    "pr_frames_forward": (_I, [_P, _P, _P, _I, C.POINTER(RebaInfo), C.POINTER(RulaInfo),
                               C.POINTER(FramesOut), _P]),
    "pr_render_workspace_bytes": (C.c_size_t, [_I, _I, _I, _I, _I]),
    "pr_render_overlay": (_I, [C.POINTER(RenderArgs), _P, C.c_size_t, _P]),
    "pr_render_people_workspace_bytes": (C.c_size_t, [_I, _I, _I, _I, _I, _I]),
    "pr_render_people": (_I, [C.POINTER(RenderPeopleArgs), _P, C.c_size_t, _P]),
    "pr_compose_video": (_I, [C.POINTER(ComposeArgs), _P]),
    "pr_compose_people": (_I, [C.POINTER(ComposePeopleArgs), _P]),
    "pr_jpeg_parse": (_I, [_P, _P, _I, _I, _I, _P, _P, _I, _P, _I, _P, _P]),
    "pr_jpeg_refusal_name": (C.c_char_p, [_I]),
    "pr_jpeg_workspace_bytes": (C.c_size_t, [_I, _I, _I]),
    "pr_jpeg_decode": (_I, [C.POINTER(JpegArgs), _P, C.c_size_t, _P]),
    "pr_jpeg_sync_workspace_bytes": (C.c_size_t, [_I, _I, _I, C.c_int64, _I, C.POINTER(JpegSyncOpts)]),
    "pr_jpeg_decode_sync": (_I, [C.POINTER(JpegArgs), C.POINTER(JpegSyncOpts), _P, _P, C.c_size_t, _P]),
    "pr_jpeg_parse_scans": (_I, [_P, _P, _I, _I, _I, _P, _P, _P, _I, _P, _I, _P, _I, _P, _P]),
    "pr_jpeg_scan_refusal_name": (C.c_char_p, [_I]),
    "pr_jpeg_scans_workspace_bytes": (C.c_size_t, [_I, _I, _I]),
    "pr_jpeg_decode_scans": (_I, [C.POINTER(JpegScansArgs), _P, C.c_size_t, _P]),
    "pr_jpeg_encode_plan": (_I, [_I, _I, _I, _I, _I, _I, _P]),
    "pr_jpeg_encode_bound": (C.c_size_t, [_I, _I, _I, _I, _I]),
    "pr_jpeg_encode_workspace_bytes": (C.c_size_t, [_I, _I, _I, _I, _I, _I, C.c_int64]),
    "pr_jpeg_encode": (_I, [C.POINTER(JpegEncArgs), _P, C.c_size_t, _P]),
    "pr_png_parse": (_I, [_P, _P, _I, _I, _I, _P, _P, _I, _P, _I, _P, _P]),
    "pr_png_refusal_name": (C.c_char_p, [_I]),
    "pr_png_workspace_bytes": (C.c_size_t, [_I, _I, _I, C.c_int64]),
    "pr_png_decode": (_I, [C.POINTER(PngArgs), _P, C.c_size_t, _P]),
    "pr_png_encode_plan": (_I, [_I, _I, _I, _I, _P]),
    "pr_png_encode_bound": (C.c_size_t, [_I, _I]),
    "pr_png_encode_workspace_bytes": (C.c_size_t, [_I, _I, _I]),
    "pr_png_encode": (_I, [C.POINTER(PngEncArgs), _P, C.c_size_t, _P]),
    "pr_resize_plan": (_I, [_I, _I, _I, _I, _P, _P, _P, _P, _P]),
    "pr_resize_frames": (_I, [_P, _I, _I, _I, _P, _I, _I, _P, _P, _P, _P, _I, _P]),
    "pr_y4m_parse_header": (_I, [_P, C.c_int64, C.POINTER(Y4mInfo)]),
    "pr_y4m_refusal_name": (C.c_char_p, [_I]),
    "pr_y4m_index": (_I, [_P, C.c_int64, C.POINTER(Y4mInfo), _P, _I, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "pr_yuv_plan": (_I, [_I, _I, C.POINTER(YuvCoeffs)]),
    "pr_yuv_frames": (_I, [C.POINTER(YuvArgs), _P]),
    "pr_yuv_enc_plan": (_I, [_I, _I, C.POINTER(YuvEncCoeffs)]),
    "pr_yuv_encode": (_I, [C.POINTER(YuvEncArgs), _P]),
    "pr_det_topology": (_I, [_I, C.POINTER(DetLayer)]),
    "pr_det_weight_floats": (C.c_size_t, [_I]),
    "pr_det_packed_floats": (C.c_size_t, [_I]),
    "pr_det_fold_pack": (_I, [_I, _P, C.c_size_t, C.c_double, _P, C.c_size_t]),
    "pr_det_packed_bytes_bf16": (C.c_size_t, [_I]),
    "pr_det_fold_pack_bf16": (_I, [_I, _P, C.c_size_t, C.c_double, _P, C.c_size_t]),
    "pr_det_create_p": (_I, [_I, _P, C.c_size_t, _I, _I, _I, C.c_double, _I, C.POINTER(_P)]),
    "pr_det_precision": (_I, [_P]),
    "pr_det_elem_bytes": (_I, [_P, _I]),
    "pr_det_conv_nhwc_bf16": (_I, [_P, _P, _P, _P] + [_I] * 9 + [_P]),
    "pr_det_create": (_I, [_I, _P, C.c_size_t, _I, _I, _I, C.c_double, C.POINTER(_P)]),
    "pr_det_destroy": (_I, [_P]),
    "pr_det_input_size": (_I, [_P, C.POINTER(_I), C.POINTER(_I)]),
    "pr_det_max_batch": (_I, [_P]),
    "pr_det_grid": (_I, [_P, _I, C.POINTER(_I), C.POINTER(_I), C.POINTER(_I)]),
    "pr_det_conv_nhwc": (_I, [_P, _P, _P, _P] + [_I] * 8 + [_P]),
    "pr_det_letterbox": (_I, [_P, _P, _I, _I, _I, _I, _P, _P]),
    "pr_det_network": (_I, [_P, _P, _I, _P, _P, _P, _P]),
    "pr_det_network_until": (_I, [_P, _P, _I, _I, _P, _P]),
    "pr_det_postprocess": (_I, [_P, _P, _P, _P, _I, C.c_float, C.c_float, _I, _P, _P, _P, _P, _P]),
    "pr_det_detect": (_I, [_P, _P, _I, _I, _I, _I, C.c_float, C.c_float, _I, _P, _P, _P, _P, _P]),
    "pr_det_unmap": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "pr_smooth_tile_rows": (_I, []),
    "pr_smooth_workspace_bytes": (C.c_size_t, [_I, _I, _I]),
    "pr_smooth_tracks": (_I, [C.POINTER(SmoothParams), C.POINTER(SmoothInputs), _P, C.POINTER(_I), _I, _I, C.POINTER(SmoothOutputs),
                              _P, _P, _P]),
    "pr_activity_tile_rows": (_I, []),
    "pr_activity_chunk_rows": (_I, []),
    "pr_activity_workspace_bytes": (C.c_size_t, [_I]),
    "pr_activity_tracks": (_I, [C.POINTER(ActivityParams), _P, _P, C.POINTER(_I), _I, _I, _P, _P, _P, _P]),
    "pr_reba_rows": (_I, [_P, _I, C.POINTER(RebaInfo), _P, _P, _P]),
    "pr_rula_rows": (_I, [_P, _I, C.POINTER(RulaInfo), _P, _P, _P]),
}

_lib = None


def load():
    """Load (once) and return the ctypes library; raises PoseRiskHipError if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PoseRiskHipError(
            f"{LIB_PATH} is missing: build it with `python -m poserisk_release_amd.build` "
            "(there is no CPU fallback for the hot path)")
    # PyTorch-ROCm bundles its own HIP runtime (libamdhip64): it has to be in the process BEFORE this library resolves the
    # same soname, or the two copies each try to own the device and the second one sees none ("no HIP device visible" from
    # pr_hmr_create when the library was loaded first, e.g. by __graft_entry__.build() followed by smoke() in one process).
    import torch  # noqa: F401
    try:
        lib = C.CDLL(LIB_PATH)
    except OSError as e:
        raise PoseRiskHipError(f"cannot load {LIB_PATH}: {e}") from e
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.pr_abi_version() != ABI_VERSION:
        raise PoseRiskHipError(f"ABI version mismatch: library {lib.pr_abi_version()}, binding {ABI_VERSION}")
    _lib = lib
    return lib


def declare_stream(device=None):
    """Tell the library which stream this thread enqueues on (torch's current one) before a call that allocates -- create,
    set_streams, destroy -- so that it can refuse instead of invalidating a hipGraph capture in progress
    (include/poserisk_hip.h, pr_declare_stream)."""
    import torch
    lib = load()
    if torch.cuda.is_available():
        lib.pr_declare_stream(torch.cuda.current_stream(device).cuda_stream, 1)
    return lib


def check(status, what=""):
    if status != 0:
        msg = load().pr_last_error().decode("utf-8", "replace")
        raise PoseRiskHipError(f"{what} failed (status {status}): {msg}")


def reba_info_struct(info):
    """add_info["REBA"] dict (example/additional_information.json:2-11) -> RebaInfo."""
    return RebaInfo(int(info["Legs_bilateral_weight_bearing/walking"]), int(info["Sitting"]),
                    int(info["Load/Force Score"]), int(info["Arm_supported_leaning_L"]),
                    int(info["Arm_supported_leaning_R"]), int(info["Coupling"]), int(info["Activity_Score"]))


def rula_info_struct(info):
    """add_info["RULA"] dict (example/additional_information.json:13-24) -> RulaInfo."""
    return RulaInfo(int(info["Arm_supported_leaning_L"]), int(info["Arm_supported_leaning_R"]),
                    int(info["A_Muscle_use_L"]), int(info["A_Muscle_use_R"]), int(info["A_Load/Force_L"]),
                    int(info["A_Load/Force_R"]), int(info["Legs_bilateral_weight_bearing"]),
                    int(info["B_Muscle_use"]), int(info["B_Load/Force"]))
