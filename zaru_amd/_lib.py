"""ctypes binding of the C ABI in include/zaru_hip.h (zaru_amd/lib/libzaru_hip.so).

The library is built in-tree by ``__graft_entry__.build()`` (``make -C zaru_amd/csrc``).
There is no fallback: if the shared object is missing or has no GPU to run on, every
entry point raises.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(HERE, "lib")
LIB_PATH = os.path.join(LIB_DIR, "libzaru_hip.so")
HEADER = os.path.join(os.path.dirname(HERE), "include", "zaru_hip.h")

ZR_OK = 0
ERRORS = {-1: "invalid argument", -2: "model", -3: "device", -4: "shape", -5: "internal"}


class ZaruError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"{ERRORS.get(code, code)} error: {msg}")
        self.code = code


class View(C.Structure):
    """zr_view: RotatedRect in root-image coordinates (centre, size, clockwise radians)."""
    _fields_ = [("cx", C.c_float), ("cy", C.c_float), ("w", C.c_float), ("h", C.c_float),
                ("rad", C.c_float)]


class Frame(C.Structure):
    _fields_ = [("rgba", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32),
                ("row_stride", C.c_uint64)]


class TrackState(C.Structure):
    """zr_track_state: one tracked ROI in HBM."""
    _fields_ = [("roi", C.c_float * 5), ("view_rect", C.c_float * 5), ("local", C.c_float * 3),
                ("active", C.c_uint32), ("frame_w", C.c_uint32), ("frame_h", C.c_uint32),
                ("tracked", C.c_uint32), ("confidence", C.c_float), ("updated", C.c_float * 5)]


class TrackCfg(C.Structure):
    """zr_track_cfg."""
    _fields_ = [("kind", C.c_int), ("num_landmarks", C.c_int), ("in_w", C.c_int), ("in_h", C.c_int),
                ("aspect_w", C.c_int), ("aspect_h", C.c_int), ("loss_thresh", C.c_float),
                ("padding", C.c_float), ("rois_per_frame", C.c_int)]


class MultiCfg(C.Structure):
    """zr_multi_cfg: the K-objects-per-stream bookkeeping (zr_multi_manage_async)."""
    _fields_ = [("slots", C.c_int), ("iou_thresh", C.c_float), ("det_grow", C.c_float), ("use_angle", C.c_int),
                ("interval_ms", C.c_double), ("aspect_w", C.c_int), ("aspect_h", C.c_int)]


class DetMergeCfg(C.Structure):
    """zr_detmerge_cfg: tiled detection's merge (zr_detect_merge_async); mode 0 Average, 1 Remove."""
    _fields_ = [("tiles", C.c_int), ("tile_cap", C.c_int), ("keypoints", C.c_int), ("iou", C.c_float),
                ("mode", C.c_int)]


class LmFilter(C.Structure):
    """zr_lm_filter: kind 0 none, 1 EMA {alpha}, 2 alpha-beta {alpha, beta}, 3 1 euro
    {min_cutoff, beta, d_cutoff}."""
    _fields_ = [("kind", C.c_int), ("p", C.c_float * 3)]

    @classmethod
    def make(cls, kind: int, *p: float):
        f = cls()
        f.kind = kind
        for i, v in enumerate(p):
            f.p[i] = v
        return f


class Pose(C.Structure):
    """zr_pose: the Procrustes result of one point set (84 bytes).  `quat` is {i, j, k, w}, `rot`
    row-major; valid == 0: the set was not analysed and every float is NaN."""
    _fields_ = [("centroid", C.c_float * 3), ("scale", C.c_float), ("translation", C.c_float * 3),
                ("valid", C.c_uint32), ("quat", C.c_float * 4), ("rot", C.c_float * 9)]


class IdentityState(C.Structure):
    """zr_identity_state: what the multi-object loop knows of one object's identity (24 bytes).
    The default state is {-1, +inf, 0, 0, 0.0}."""
    _fields_ = [("row", C.c_int32), ("distance", C.c_float), ("embeddings", C.c_uint32), ("flags", C.c_uint32),
                ("next_ms", C.c_double)]


class GalleryLink(C.Structure):
    """zr_gallery_link: one gallery row's link record (16 bytes).  The default record of row r is
    {r, -1, 0, 0}."""
    _fields_ = [("alias", C.c_int32), ("partner", C.c_int32), ("seen", C.c_uint32), ("reserved", C.c_uint32)]


class IdentityCfg(C.Structure):
    """zr_identity_cfg."""
    _fields_ = [("slots", C.c_int), ("num_landmarks", C.c_int), ("aspect_w", C.c_int), ("aspect_h", C.c_int),
                ("crop_grow", C.c_float), ("threshold", C.c_float), ("interval_ms", C.c_double)]


class EyeCfg(C.Structure):
    """zr_eye_cfg."""
    _fields_ = [("slots", C.c_int), ("num_landmarks", C.c_int), ("aspect_w", C.c_int), ("aspect_h", C.c_int),
                ("in_w", C.c_int), ("in_h", C.c_int), ("crop_grow", C.c_float)]


class FaceQuality(C.Structure):
    """zr_face_quality: the quality gate's record of one object (32 bytes); the default is all zero."""
    _fields_ = [("size", C.c_float), ("inside", C.c_float), ("sharpness", C.c_float), ("frontal", C.c_float),
                ("flags", C.c_uint32), ("rejected", C.c_uint32), ("samples", C.c_uint32), ("reserved", C.c_uint32)]


class QualityTier(C.Structure):
    """zr_quality_tier: four minima; -inf skips a criterion."""
    _fields_ = [("min_size", C.c_float), ("min_inside", C.c_float), ("min_sharpness", C.c_float),
                ("min_frontal", C.c_float)]


class QualityCfg(C.Structure):
    """zr_quality_cfg."""
    _fields_ = [("slots", C.c_int), ("ow", C.c_int), ("oh", C.c_int), ("embed", QualityTier), ("learn", QualityTier)]


QUALITY_MEASURED, QUALITY_EMBED, QUALITY_LEARN = 1, 2, 4
QUALITY_FAIL_SIZE, QUALITY_FAIL_INSIDE, QUALITY_FAIL_SHARPNESS, QUALITY_FAIL_FRONTAL = 16, 32, 64, 128


class AlignCfg(C.Structure):
    """zr_align_cfg: the aligned identity crop's template, landmark groups (-1 ends a group) and limit."""
    _fields_ = [("num_points", C.c_int32), ("ow", C.c_int32), ("oh", C.c_int32), ("tmpl", C.c_float * 2 * 8),
                ("group", C.c_int32 * 4 * 8), ("max_residual", C.c_float)]

    @classmethod
    def make(cls, template, groups, ow=112, oh=112, max_residual=float("inf")):
        """template: P points (x, y); groups: P lists of 1..4 landmark indices.  Nothing is checked
        here: the entry points refuse what they refuse."""
        c = cls(len(template), ow, oh)
        c.max_residual = max_residual
        for p in range(8):
            for j in range(4):
                c.group[p][j] = -1
        for p, (t, g) in enumerate(zip(template[:8], groups[:8])):
            c.tmpl[p][0], c.tmpl[p][1] = float(t[0]), float(t[1])
            for j, idx in enumerate(list(g)[:4]):
                c.group[p][j] = int(idx)
        return c


class FaceAlignment(C.Structure):
    """zr_face_alignment: the record of one fit (16 bytes)."""
    _fields_ = [("scale", C.c_float), ("rad", C.c_float), ("residual", C.c_float), ("flags", C.c_uint32)]


ALIGN_ALIGNED, ALIGN_FALLBACK, ALIGN_FAIL_DEGENERATE, ALIGN_FAIL_RESIDUAL = 1, 2, 16, 32


class ExportHeader(C.Structure):
    """zr_export_header: the fixed part of one record of zr_multi_export_async (48 bytes)."""
    _fields_ = [("id", C.c_uint64), ("stream", C.c_int32), ("slot", C.c_int32), ("roi", C.c_float * 5),
                ("confidence", C.c_float), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class ExportIdentity(C.Structure):
    """zr_export_identity: an exported object's identity (16 bytes); all zero when it has none."""
    _fields_ = [("row", C.c_int32), ("distance", C.c_float), ("embeddings", C.c_uint32), ("flags", C.c_uint32)]


EXPORT_POSE, EXPORT_IDENTITY, EXPORT_EYE_LEFT, EXPORT_EYE_RIGHT, EXPORT_QUALITY = 1, 2, 4, 8, 16


class MultiExportArgs(C.Structure):
    """zr_multi_export_args: the tracker's arrays and the packed outputs, device pointers.  An optional
    group (pose; identity; eyes) is left None when its feature is off.  (The quality gate's group travels
    beside it: zr_multi_export_quality_async.)"""
    INPUTS = ("d_nobjects", "d_src", "d_ids", "d_roi", "d_state", "d_landmarks")
    POSE = ("d_pose", "d_out_pose")
    IDENTITY = ("d_id_state", "d_id_emb", "d_out_identity", "d_out_emb")
    EYES = ("d_eye_valid", "d_eye_diam", "d_eye_crop", "d_eye_lm", "d_out_eye_valid", "d_out_eye_diam",
            "d_out_eye_crop", "d_out_eye_lm")
    _fields_ = [(n, C.c_void_p) for n in (
        "d_nobjects", "d_src", "d_ids", "d_roi", "d_state", "d_landmarks", "d_pose", "d_id_state", "d_id_emb",
        "d_eye_valid", "d_eye_diam", "d_eye_crop", "d_eye_lm", "d_count", "d_stream_offsets", "d_header",
        "d_out_landmarks", "d_out_pose", "d_out_identity", "d_out_emb", "d_out_eye_valid", "d_out_eye_diam",
        "d_out_eye_crop", "d_out_eye_lm")]


def lm_filter_state_size(f: LmFilter, num_landmarks: int) -> int:
    n = C.c_size_t(0)
    check(lib().zr_lm_filter_state_size(C.byref(f), num_landmarks, C.byref(n)))
    return n.value


_LIB = None

# (name, restype, argtypes) for every exported entry point of include/zaru_hip.h
_P, _SZ, _F, _U32, _I = C.c_void_p, C.c_size_t, C.c_float, C.c_uint32, C.c_int
SIGNATURES = [
    ("zr_session_create", _I, [_P, _SZ, _P, _SZ, _I, C.POINTER(_P)]),
    ("zr_session_destroy", None, [_P]),
    ("zr_session_num_io", _I, [_P, _I, C.POINTER(_SZ)]),
    ("zr_session_io", _I, [_P, _I, _SZ, C.POINTER(C.c_char_p), _P, C.POINTER(_SZ)]),
    ("zr_session_run", _I, [_P, _SZ, _P, _SZ, _P, _SZ]),
    ("zr_session_run_async", _I, [_P, _SZ, _P, _P, _SZ, _P]),
    ("zr_cnn_estimate_views", _I, [_P, _P, _U32, _U32, _SZ, _P, _SZ, _F, _F, _P]),
    ("zr_cnn_estimate_views_async", _I, [_P, _P, _SZ, _P, _P, _SZ, _F, _F, _P, _P]),
    ("zr_preprocess_views_async", _I, [_P, _SZ, _P, _P, _SZ, _U32, _U32, _F, _F, _P, _P]),
    ("zr_detection_candidates_async", _I, [_P, _P, _U32, _U32, _U32, _F, _U32, _P, _P, _P]),
    ("zr_track_seed_async", _I, [_P, _SZ, _P, _P, _P]),
    ("zr_track_update_async", _I, [_P, _SZ, _P, _P, _SZ, _P, _SZ, _P, _P, _P]),
    ("zr_lm_filter_state_size", _I, [_P, _SZ, C.POINTER(_SZ)]),
    ("zr_lm_filter_async", _I, [_P, _P, _P, _SZ, _P, _SZ, _P, _SZ, _F, _P, _P, _P]),
    ("zr_track_update_positions_async", _I, [_P, _SZ, _P, _P, _P, _SZ, _P, _P, _P]),
    ("zr_lm_filter_indexed_async", _I, [_P, _P, _P, _SZ, _SZ, _P, _SZ, _P, _SZ, _P, _P, _F, _P, _P, _P, _P]),
    ("zr_track_update_positions_indexed_async", _I, [_P, _SZ, _P, _P, _P, _SZ, _P, _P, _P, _P]),
    ("zr_procrustes_create", _I, [_P, _SZ, C.POINTER(_P)]),
    ("zr_procrustes_destroy", None, [_P]),
    ("zr_procrustes_analyze_async", _I, [_P, _P, _SZ, _SZ, _I, _P, _P, _P]),
    ("zr_procrustes_analyze_tracked_async", _I, [_P, _P, _SZ, _SZ, _I, _P, _P, _P]),
    ("zr_view_describe", _I, [_P, _SZ, _U32, _P]),
    ("zr_detect_post_async", _I, [_P, _P, _P, _P, _SZ, _P, _P, _P, _SZ, _P, _SZ, _U32, _U32, _P, _P]),
    ("zr_detect_post_mapped_async", _I, [_P, _P, _P, _P, _SZ, _P, _P, _P, _P, _P, _SZ, _P, _P]),
    ("zr_due_compact_async", _I, [_P, _SZ, _P, _P, _P, _P, _P, _P]),
    ("zr_due_compact_tiles_async", _I, [_P, _SZ, _P, _SZ, _P, _P, _P, _P, _P, _P, _P, _P]),
    ("zr_detect_merge_async", _I, [_P, _P, _P, _P, _SZ, _P, _P, _P, _SZ, _P, _P, _P]),
    ("zr_track_lost_compact_async", _I, [_P, _SZ, _P, _P, _P, _P, _P, _P]),
    ("zr_track_reseed_best_async", _I, [_P, _P, _SZ, _P, _SZ, _P, _P, _P, _P, _P]),
    ("zr_cnn_estimate_device_views_count_async", _I, [_P, _P, _SZ, _P, _SZ, _P, _F, _F, _P, _P]),
    ("zr_track_seed_detections_async", _I, [_P, _P, _SZ, _P, _P, _P, _SZ, _P, _F, _I, _P, _P, _P, _P]),
    ("zr_hand_manage_async", _I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _SZ, _P, _SZ, _P, C.c_double, _I,
                                  _P, _P, _P]),
    ("zr_multi_manage_async", _I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _SZ, _P, _SZ, _P, C.c_double, _I,
                                   _P, _P, _P]),
    ("zr_slot_compact_async", _I, [_P, _SZ, _SZ, _P, _P, _P, _P, _P, _P]),
    ("zr_track_update_indexed_async", _I, [_P, _SZ, _P, _P, _SZ, _P, _SZ, _P, _P, _P, _P]),
    ("zr_embed_match_async", _I, [_P, _SZ, _P, _SZ, _SZ, _P, _P, _P, _P, _P]),
    ("zr_identity_select_async", _I, [_P, _P, _SZ, _P, _P, C.c_double, _P, _P, _P, _P, _P, _P, _P]),
    ("zr_identity_compact_async", _I, [_P, _P, _SZ, _P, _P, _P, _P, _P, _P]),
    ("zr_identity_commit_async", _I, [_P, _SZ, _P, _P, _P, _P, C.c_double, _P, _P, _P]),
    ("zr_identity_enrol_async", _I, [_P, _SZ, _P, _P, _P, _P, _P, _P, _P, _SZ, _SZ, _U32, _P, _P, _P]),
    ("zr_identity_link_async", _I, [_P, _P, _SZ, _P, _P, _P, _P, _P, _P, _SZ, _U32, C.c_float, _P, _P]),
    ("zr_identity_blend_async", _I, [_P, _SZ, _P, _P, _P, _P, _U32, _P, _P]),
    ("zr_identity_refine_async", _I, [_P, _SZ, _P, _P, _P, _P, _P, _P, _SZ, _SZ, _U32, C.c_float, _P, _P]),
    ("zr_identity_quality_async", _I, [_P, _P, _SZ, _P, _SZ, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    ("zr_identity_quality_mask_async", _I, [_SZ, _P, _P, _P, _P, _P]),
    ("zr_face_quality_host", _I, [_P, _P, _P, _P, _P]),
    ("zr_identity_align_async", _I, [_P, _P, _SZ, _P, _SZ, _P, _P, _P, _P, _P]),
    ("zr_face_align_host", _I, [_P, _P, _SZ, _SZ, _U32, _U32, _U32, _P, _P]),
    ("zr_embed_match_count_async", _I, [_P, _SZ, _P, _SZ, _P, _SZ, _P, _P, _P, _P]),
    ("zr_eye_select_async", _I, [_P, _P, _SZ, _P, _P, _P, _P, _P]),
    ("zr_eye_crop_async", _I, [_P, _SZ, _P, _P, _SZ, _P, _P, _U32, _U32, _P]),
    ("zr_eye_commit_async", _I, [_P, _SZ, _P, _P, _P, _SZ, _SZ, _P, _P, _P, _P, _P]),
    ("zr_multi_export_async", _I, [_P, _SZ, _SZ, _SZ, _P]),
    ("zr_multi_export_quality_async", _I, [_P, _P, _P, _SZ, _SZ, _SZ, _P]),
    ("zr_comm_unique_id", _I, [_P]),
    ("zr_comm_create", _I, [_P, _I, _I, _I, C.POINTER(_P)]),
    ("zr_comm_destroy", None, [_P]),
    ("zr_comm_size", _I, [_P, C.POINTER(_I)]),
    ("zr_comm_all_gather_async", _I, [_P, _P, _P, _SZ, _P]),
    ("zr_debug_glibc_math", _I, [_I, _P, _P, _P, _SZ, _P]),
    ("zr_cnn_estimate_device_views_async", _I, [_P, _P, _SZ, _P, _SZ, _F, _F, _P, _P]),
    ("zr_jpeg_decoder_create", _I, [C.c_int, _P]),
    ("zr_jpeg_decoder_destroy", None, [_P]),
    ("zr_jpeg_info", _I, [_P, _SZ, _P, _P]),
    ("zr_jpeg_decode_async", _I, [_P, _P, _SZ, _P, _SZ, _P]),
    ("zr_jpeg_decode_batch_async", _I, [_P, _SZ, _P, _P, _P, _P, _P]),
    ("zr_jpeg_coefficients", _I, [_P, _SZ, _P, _SZ, _P]),
    ("zr_jpeg_decoder_status", _I, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(_I)]),
    ("zr_jpeg_frame_errors", _I, [_P, _P, _SZ, C.POINTER(_SZ)]),
    ("zr_session_stats", _I, [_P, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(_SZ)]),
    ("zr_plan_describe", _I, [_P, _SZ, _P, _SZ, _P, _SZ, C.POINTER(_SZ)]),
    ("zr_profile_enable", _I, [_P, _I]),
    ("zr_profile_read", _I, [_P, _P, _SZ, C.POINTER(_SZ)]),
    ("zr_last_error", C.c_char_p, []),
    ("zr_device_count", _I, [C.POINTER(_I)]),
    ("zr_malloc", _I, [C.POINTER(_P), _SZ]),
    ("zr_free", _I, [_P]),
    ("zr_host_alloc", _I, [C.POINTER(_P), _SZ]),
    ("zr_host_free", _I, [_P]),
    ("zr_memcpy_async", _I, [_P, _P, _SZ, _I, _P]),
    ("zr_memset_async", _I, [_P, _I, _SZ, _P]),
    ("zr_memcpy2d_async", _I, [_P, _SZ, _P, _SZ, _SZ, _SZ, _I, _P]),
    ("zr_stream_create", _I, [C.POINTER(_P)]),
    ("zr_stream_destroy", _I, [_P]),
    ("zr_stream_synchronize", _I, [_P]),
    ("zr_event_create", _I, [C.POINTER(_P)]),
    ("zr_event_create_timing", _I, [C.POINTER(_P)]),
    ("zr_event_elapsed", _I, [C.POINTER(_F), _P, _P]),
    ("zr_stream_wait_event", _I, [_P, _P]),
    ("zr_event_destroy", _I, [_P]),
    ("zr_event_record", _I, [_P, _P]),
    ("zr_event_synchronize", _I, [_P]),
    ("zr_event_query", _I, [_P]),
]


def lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise ZaruError(-3, f"HIP extension not built: {LIB_PATH} missing "
                            "(run __graft_entry__.build())")
    L = C.CDLL(LIB_PATH)
    for name, res, args in SIGNATURES:
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _LIB = L
    return L


def check(rc: int):
    if rc != ZR_OK:
        raise ZaruError(rc, lib().zr_last_error().decode(errors="replace"))


def device_count() -> int:
    n = C.c_int(0)
    check(lib().zr_device_count(C.byref(n)))
    return n.value


def plan_describe(onnx: bytes, outputs=None) -> str:
    sel = (C.c_uint32 * len(outputs))(*outputs) if outputs else None
    need = C.c_size_t(0)
    check(lib().zr_plan_describe(onnx, len(onnx), sel, len(outputs or []), None, 0,
                                 C.byref(need)))
    buf = C.create_string_buffer(need.value)
    check(lib().zr_plan_describe(onnx, len(onnx), sel, len(outputs or []), buf, need.value,
                                 C.byref(need)))
    return buf.value.decode()


class DeviceBuffer:
    """Owning device allocation (through the C ABI helpers, no HIP/torch import needed)."""

    def __init__(self, nbytes: int):
        p = C.c_void_p()
        check(lib().zr_malloc(C.byref(p), max(4, int(nbytes))))
        self.ptr = p.value
        self.nbytes = int(nbytes)

    @classmethod
    def from_array(cls, a, stream=None):
        import numpy as np
        a = np.ascontiguousarray(a)
        b = cls(a.nbytes)
        b.upload(a, stream)
        return b

    def upload(self, a, stream=None):
        import numpy as np
        a = np.ascontiguousarray(a)
        check(lib().zr_memcpy_async(self.ptr, a.ctypes.data, a.nbytes, 0, stream))
        check(lib().zr_stream_synchronize(stream))

    def download(self, shape, dtype, stream=None):
        import numpy as np
        out = np.empty(shape, dtype)
        check(lib().zr_memcpy_async(out.ctypes.data, self.ptr, out.nbytes, 1, stream))
        check(lib().zr_stream_synchronize(stream))
        return out

    def free(self):
        if getattr(self, "ptr", None) and _LIB is not None:
            _LIB.zr_free(self.ptr)
            self.ptr = None

    def __del__(self):
        self.free()


class Procrustes:
    """zr_procrustes: a reference point set ((n, 3) float32, n >= 2) on the device, and the batched
    analysis of device-resident point sets against it (kernels/procrustes.hip)."""

    def __init__(self, reference):
        import numpy as np
        ref = np.ascontiguousarray(reference, np.float32)
        if ref.ndim != 2 or ref.shape[1] != 3:
            raise ZaruError(-4, "reference must be (n, 3) float32")
        p = C.c_void_p()
        check(lib().zr_procrustes_create(ref.ctypes.data, ref.shape[0], C.byref(p)))
        self.ptr, self.n_ref = p.value, ref.shape[0]

    def analyze_async(self, d_points: int, n_sets: int, d_out: int, stride=None, flip_y=False, d_valid=None,
                      stream=None):
        """Enqueue the analysis of n_sets sets (`stride` floats apart, default 3 n_ref) into n_sets
        zr_pose records at d_out."""
        check(lib().zr_procrustes_analyze_async(self.ptr, d_points, n_sets,
                                                3 * self.n_ref if stride is None else stride,
                                                int(bool(flip_y)), d_valid, d_out, stream))

    def analyze(self, points, flip_y=False, valid=None):
        """Host arrays in, a numpy record array (dtype of `Pose`) out: points is (n_sets, m, 3)
        float32 with m >= n_ref; valid an optional int32 mask."""
        import numpy as np
        pts = np.ascontiguousarray(points, np.float32)
        if pts.ndim != 3 or pts.shape[2] != 3:
            raise ZaruError(-4, "points must be (n_sets, m, 3) float32")
        d_pts = DeviceBuffer.from_array(pts)
        d_valid = None if valid is None else DeviceBuffer.from_array(np.ascontiguousarray(valid, np.int32))
        d_out = DeviceBuffer(pts.shape[0] * C.sizeof(Pose))
        self.analyze_async(d_pts.ptr, pts.shape[0], d_out.ptr, 3 * pts.shape[1], flip_y,
                           None if d_valid is None else d_valid.ptr)
        return d_out.download((pts.shape[0],), np.dtype(Pose))

    def close(self):
        if getattr(self, "ptr", None) and _LIB is not None:
            _LIB.zr_procrustes_destroy(self.ptr)
            self.ptr = None

    def __del__(self):
        self.close()


def synchronize(stream=None):
    check(lib().zr_stream_synchronize(stream))


class _StdoutToStderr:
    """RCCL prints a version banner on stdout when it initialises; bench.py's one JSON line on
    stdout must stay the only thing there, so fd 1 points at stderr meanwhile."""

    def __enter__(self):
        import os
        import sys
        sys.stdout.flush()
        self.saved = os.dup(1)
        os.dup2(2, 1)

    def __exit__(self, *exc):
        import os
        os.dup2(self.saved, 1)
        os.close(self.saved)


class Comm:
    """The node communicator of the multi-GPU path (zr_comm_*): RCCL over xGMI,
    one rank per GPU.  `unique_id()` on one rank; its 128 bytes reach the others by any side
    channel (bench.py: the gloo control group); `Comm(uid, world, rank, device)` joins."""

    @staticmethod
    def unique_id() -> bytes:
        buf = (C.c_uint8 * 128)()
        with _StdoutToStderr():
            check(lib().zr_comm_unique_id(buf))
        return bytes(buf)

    def __init__(self, uid: bytes, world: int, rank: int, device: int):
        if len(uid) != 128:
            raise ValueError("a communicator id is 128 bytes")
        p = C.c_void_p()
        buf = (C.c_uint8 * 128).from_buffer_copy(uid)
        with _StdoutToStderr():
            check(lib().zr_comm_create(buf, world, rank, device, C.byref(p)))
        self.ptr, self.world, self.rank = p.value, world, rank

    def size(self) -> int:
        n = C.c_int()
        check(lib().zr_comm_size(self.ptr, C.byref(n)))
        return n.value

    def all_gather_async(self, d_send: int, d_recv: int, nbytes: int, stream=None):
        check(lib().zr_comm_all_gather_async(self.ptr, d_send, d_recv, nbytes, stream))

    def close(self):
        if getattr(self, "ptr", None) and _LIB is not None:
            _LIB.zr_comm_destroy(self.ptr)
            self.ptr = None

    def __del__(self):
        self.close()
