"""ctypes binding of libfaceid.so (include/faceid.h).  There is NO fallback: if the shared library
is missing or a call fails, this raises -- the product never computes on the CPU."""
from __future__ import annotations

import ctypes as C
import os
import sys
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# FID_LIB names another build of the same library in this directory (libfaceid_asan.so from `make asan`); never a CPU fallback
LIB_PATH = os.path.join(_HERE, os.path.basename(os.environ.get("FID_LIB") or "libfaceid.so"))

c_void_pp = C.POINTER(C.c_void_p)
c_int_p = C.POINTER(C.c_int)
c_i32_p = C.POINTER(C.c_int32)
c_i64_p = C.POINTER(C.c_int64)
c_f32_p = C.POINTER(C.c_float)
c_f64_p = C.POINTER(C.c_double)
c_u8_p = C.POINTER(C.c_uint8)

# name -> (restype, argtypes); every symbol include/faceid.h declares
class GateConfig(C.Structure):
    """fid_gate_config (include/faceid.h): the reference's config.json blocks face_quality / side_face_detection / face_detection, flattened;
    the defaults are the reference's own values"""
    _fields_ = ([("size_normalization", C.c_float)]
                + [(n, C.c_float) for n in ("w_detection", "w_size", "w_blur", "w_pose", "w_lighting",
                                            "ar_extreme_profile", "ar_very_strong_profile", "ar_strong_profile", "ar_very_wide", "ar_wide", "ar_moderately_wide",
                                            "area_extremely_small", "area_very_small", "area_small", "area_very_large", "area_large",
                                            "compactness_very_low", "compactness_low", "confidence_very_low", "confidence_low", "edge_position_threshold")]
                + [("decision_threshold", C.c_int32)]
                + [(n, C.c_float) for n in ("yaw_threshold", "pitch_threshold", "confidence_threshold", "min_quality_threshold")])

    DEFAULTS = dict(size_normalization=10000.0, w_detection=0.4, w_size=0.2, w_blur=0.2, w_pose=0.1, w_lighting=0.1,
                    ar_extreme_profile=0.2, ar_very_strong_profile=0.3, ar_strong_profile=0.5, ar_very_wide=2.5, ar_wide=2.0, ar_moderately_wide=1.6,
                    area_extremely_small=1200.0, area_very_small=1800.0, area_small=2500.0, area_very_large=400000.0, area_large=300000.0,
                    compactness_very_low=0.10, compactness_low=0.6, confidence_very_low=0.15, confidence_low=0.7,
                    edge_position_threshold=30.0, decision_threshold=4, yaw_threshold=35.0, pitch_threshold=35.0,
                    confidence_threshold=0.6, min_quality_threshold=0.05)

    def __init__(self, **kw):
        super().__init__()
        vals = dict(self.DEFAULTS)
        unknown = set(kw) - set(vals)
        if unknown:
            raise TypeError(f"unknown gate thresholds: {sorted(unknown)}")
        vals.update(kw)
        for k, v in vals.items():
            setattr(self, k, v)

    @classmethod
    def from_reference_json(cls, cfg: dict) -> "GateConfig":
        """the reference's config.json (the three blocks the gates read; missing keys keep the defaults)"""
        q, s, d = cfg.get("face_quality", {}), cfg.get("side_face_detection", {}), cfg.get("face_detection", {})
        kw = {}
        if "size_normalization" in q:
            kw["size_normalization"] = float(q["size_normalization"])
        for src, dst in (("detection_score", "w_detection"), ("size_score", "w_size"), ("blur_score", "w_blur"), ("pose_score", "w_pose"),
                         ("lighting_score", "w_lighting")):
            if src in q.get("weights", {}):
                kw[dst] = float(q["weights"][src])
        for block, prefix in (("aspect_ratio_thresholds", "ar_"), ("area_thresholds", "area_"), ("compactness_thresholds", "compactness_"),
                              ("confidence_thresholds", "confidence_")):
            for k, v in s.get(block, {}).items():
                if prefix + k in cls.DEFAULTS:
                    kw[prefix + k] = float(v)
        for k in ("edge_position_threshold", "decision_threshold"):
            if k in s:
                kw[k] = int(s[k]) if k == "decision_threshold" else float(s[k])
        for k in ("yaw_threshold", "pitch_threshold", "confidence_threshold", "min_quality_threshold"):
            if k in d:
                kw[k] = float(d[k])
        return cls(**kw)


class TrackConfig(C.Structure):
    """fid_track_config (include/faceid.h): overlap threshold of the association, frames a track survives unmatched, matches between two
    embeddings of a named track (refresh) and of one without a name (retry)"""
    _fields_ = [("iou_thresh", C.c_float), ("max_age", C.c_int32), ("refresh", C.c_int32), ("retry", C.c_int32)]


TRACK_SLOT_WORDS = 10            # FID_TRACK_SLOT_WORDS
TRACK_STARTED, TRACK_EMBED = 1 << 8, 1 << 9
TRACK_COASTED = 1 << 10          # FID_TRACK_COASTED: a row the coaster appended; the word's bits 16 .. are the track's missed frames
COAST_WORDS = 16                 # FID_COAST_WORDS: id, missed, has_vel, ident_idx, ident_score, box[4], vel[4], conf, 0 x 2


class CoastConfig(C.Structure):
    """fid_coast_config (include/faceid.h): missed frames a track's box is held for (0 .. 1023), whether the held box moves along the track's
    last velocity, and the share of its width and height the box grows by on every side per missed frame ([0, 0.5]).
    The defaults (5 frames, prediction on, 5 % per frame) are UNCALIBRATED: nobody has measured them on real video.  They are starting
    points for a user's own calibration."""
    _fields_ = [("hold", C.c_int32), ("predict", C.c_int32), ("grow", C.c_float), ("reserved", C.c_int32)]

    def __init__(self, hold=5, predict=True, grow=0.05):
        super().__init__(int(hold), int(bool(predict)), float(grow), 0)


TRACK_RELINKED = 1 << 11         # FID_TRACK_RELINKED: the detection's person id is an earlier track's, not its own track id
RELINK_WORDS = 8                 # FID_RELINK_WORDS: live = id, person, has_q, link score, seen, missed, linked-from, 0; pool = person, id, seen, 0 x 5
RELINK_MAX_POOL = 64             # FID_RELINK_MAX_POOL


class RelinkConfigC(C.Structure):
    """fid_relink_config (include/faceid.h)"""
    _fields_ = [("thresh", C.c_float), ("window", C.c_int32), ("max_age", C.c_int32)]


class RelinkConfig:
    """What a relinker is built with: the cosine a new track's first embedding must exceed against a pooled, ended track to inherit its
    person id ([0, 1)), the frames an ended track waits in the pool, and the pool's entries per stream (1 .. 64).  max_age is not here: it
    is the tracker's (c(max_age) gives the fid_relink_config).
    thresh defaults to the reference's grouping_threshold (0.45) and, like it, is UNCALIBRATED for this use; window and pool are
    uncalibrated too.  They are starting points for a user's own calibration (engine.VectorGallery.score_distribution measures the score
    distributions of a labelled store)."""

    def __init__(self, thresh=0.45, window=300, pool=32):
        self.thresh, self.window, self.pool = float(thresh), int(window), int(pool)

    def c(self, max_age) -> RelinkConfigC:
        return RelinkConfigC(self.thresh, self.window, int(max_age))

    def __repr__(self):
        return f"RelinkConfig(thresh={self.thresh}, window={self.window}, pool={self.pool})"


FID_LABEL_MAX = 32               # name bytes a label shows
DRAW_TRACK_ID = 1                # FID_DRAW_TRACK_ID


class DrawStyle(C.Structure):
    """fid_draw_style (include/faceid.h): corner length as a fraction of min(w, h) (a double, like the reference's Python float), thickness
    of the corner arms (odd, 1 .. 15), text scale (0 = no text, 1 .. 4), similarity bar on / off, flags (DRAW_TRACK_ID), colour of an unknown
    face; the defaults are the reference's (draw_bbox's 0.2 and 3, main.py:148's (255, 0, 0))"""
    _fields_ = [("proportion", C.c_double), ("thickness", C.c_int32), ("text_scale", C.c_int32), ("bar", C.c_int32), ("flags", C.c_int32),
                ("unknown_bgr", C.c_uint8 * 4)]

    def __init__(self, proportion=0.2, thickness=3, text_scale=2, bar=1, flags=0, unknown_bgr=(255, 0, 0)):
        super().__init__()
        self.proportion, self.thickness, self.text_scale = float(proportion), int(thickness), int(text_scale)
        self.bar, self.flags = int(bar), int(flags)
        self.unknown_bgr[:3] = [int(v) for v in unknown_bgr]


REDACT_MOSAIC, REDACT_FILL = 0, 1          # FID_REDACT_MOSAIC, FID_REDACT_FILL
REDACT_UNKNOWN, REDACT_KNOWN = 1, 2        # FID_REDACT_UNKNOWN, FID_REDACT_KNOWN (bits of `who`)


class RedactStyle(C.Structure):
    """fid_redact_style (include/faceid.h): mosaic or solid fill, whom to redact (REDACT_UNKNOWN | REDACT_KNOWN), mosaic cells along the
    longer side of the box (1 .. 16), margin as a share of the box's width and height ([0, 0.5]), FILL colour.  The default hides every face
    that is not in the gallery behind an 8-cell mosaic."""
    _fields_ = [("mode", C.c_int32), ("who", C.c_int32), ("cells", C.c_int32), ("reserved", C.c_int32), ("expand", C.c_double),
                ("fill_bgr", C.c_uint8 * 4)]

    def __init__(self, mode=REDACT_MOSAIC, who=REDACT_UNKNOWN, cells=8, expand=0.1, fill_bgr=(0, 0, 0)):
        super().__init__()
        self.mode, self.who, self.cells, self.reserved, self.expand = int(mode), int(who), int(cells), 0, float(expand)
        self.fill_bgr[:3] = [int(v) for v in fill_bgr]


MEASURE_KEYS = ("sharpness", "mean", "contrast", "clipped", "yaw", "pitch", "residual")       # words 0 .. 6 of a fid_face_measure row
MEASURE_PIXELS_VALID, MEASURE_POSE_VALID = 1, 2                                                # stats word 7

SHOT_META_WORDS = 16             # FID_SHOT_META_WORDS: stream, track id, ident_idx, ident_score, shot score, frame, rows, box[4], det score, 0 x 4


class MeasureConfig(C.Structure):
    """fid_measure_config (include/faceid.h): what fid_face_gates_measured divides the measured sharpness (variance of the Laplacian), contrast
    (standard deviation of the luma) and landmark residual (crop pixels) by, and the |yaw| / |pitch| ratios above which a face is a side face.
    The defaults are UNCALIBRATED: nobody has measured them on real faces.  They are starting points for a user's own calibration."""
    _fields_ = [(n, C.c_float) for n in ("sharpness_normalization", "contrast_normalization", "residual_normalization",
                                         "yaw_ratio_threshold", "pitch_ratio_threshold")]

    def __init__(self, sharpness_normalization=100.0, contrast_normalization=40.0, residual_normalization=8.0, yaw_ratio_threshold=0.25,
                 pitch_ratio_threshold=0.25):
        super().__init__(float(sharpness_normalization), float(contrast_normalization), float(residual_normalization),
                         float(yaw_ratio_threshold), float(pitch_ratio_threshold))


YUV_STANDARDS = {"bt601": 0, "bt709": 1, "bt601_full": 2}     # FID_YUV_BT601_LIMITED, FID_YUV_BT709_LIMITED, FID_YUV_BT601_FULL


class Nv12Desc(C.Structure):
    """fid_nv12_desc (include/faceid.h): bytes per row of both planes, bytes from a frame's first Y byte to its first UV byte, bytes from one
    frame to the next, colour standard"""
    _fields_ = [("pitch", C.c_int32), ("uv_offset", C.c_int64), ("frame_stride", C.c_int64), ("standard", C.c_int32)]


def nv12_desc(H, W, pitch=None, uv_offset=None, frame_stride=None, standard="bt601") -> Nv12Desc:
    """the layout of H x W NV12 frames; the defaults are the dense one: pitch = W, uv_offset = W*H, frame_stride = W*H*3//2"""
    H, W = int(H), int(W)
    pitch = W if pitch is None else int(pitch)
    uv_offset = pitch * H if uv_offset is None else int(uv_offset)
    frame_stride = uv_offset + pitch * (H // 2) if frame_stride is None else int(frame_stride)
    if isinstance(standard, str):
        if standard not in YUV_STANDARDS:
            raise ValueError(f"unknown colour standard {standard!r}: one of {sorted(YUV_STANDARDS)}")
        standard = YUV_STANDARDS[standard]
    return Nv12Desc(pitch, uv_offset, frame_stride, int(standard))


class Nv12Frames:
    """A batch of NV12 video frames on the device, as the *_nv12 entry points take it: `buf` (a DeviceBuffer, a torch tensor or a raw device
    pointer) holds the frames, H x W is the picture, the rest is fid_nv12_desc -- by default the dense layout ([B, H*3//2, W] uint8: H rows
    of Y, then H/2 rows of interleaved U, V).  FacePipeline.detect / embed / run_step / draw take one wherever they take BGR frames.
    `.args()` = the two leading arguments (nv12_dev, desc) of those entry points."""

    def __init__(self, buf, H, W, pitch=None, uv_offset=None, frame_stride=None, standard="bt601"):
        self.buf, self.H, self.W = buf, int(H), int(W)
        self.desc = nv12_desc(H, W, pitch, uv_offset, frame_stride, standard)

    def args(self):
        return (_ptr(self.buf), C.byref(self.desc))


def label_arrays(names, colors=None):
    """names (str or bytes per gallery row), colors (BGR triple per row, or None) as fid_labels_create / fid_draw_faces_host take them:
    (name bytes, int32 [G+1] offsets, uint8 [G,3] or None).  A str is encoded as UTF-8; the table keeps FID_LABEL_MAX bytes of it."""
    raw = [n if isinstance(n, (bytes, bytearray)) else str(n).encode("utf-8") for n in names]
    offsets = np.zeros(len(raw) + 1, np.int32)
    offsets[1:] = np.cumsum([len(r) for r in raw])
    bgr = None
    if colors is not None:
        bgr = np.ascontiguousarray(np.asarray(colors).reshape(len(raw), 3), dtype=np.uint8)
    return b"".join(bytes(r) for r in raw), offsets, bgr

TEMPLATE_MAX_ROWS = 1 << 20       # FID_TEMPLATE_MAX_ROWS: positions of one fid_gallery_templates call
TEMPLATE_CHUNK = 256             # FID_TEMPLATE_CHUNK: the members one wave sums; a person with more is split over several waves

SIGNATURES = {
    "fid_labels_create": (C.c_int, [C.c_void_p, C.c_char_p, c_i32_p, C.c_void_p, C.c_int, c_void_pp]),
    "fid_labels_destroy": (C.c_int, [C.c_void_p, C.c_void_p]),
    "fid_draw_faces": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                 C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fid_draw_faces_host": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                      C.c_void_p, C.c_int, C.c_void_p, C.c_char_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "fid_draw_faces_nv12": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                      C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fid_draw_faces_nv12_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                           C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_char_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "fid_draw_glyphs": (C.c_int, [C.c_void_p]),
    "fid_redact_faces": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                   C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "fid_redact_faces_host": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                        C.c_void_p, C.c_int, C.c_void_p]),
    "fid_redact_faces_nv12": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                        C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "fid_redact_faces_nv12_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                             C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "fid_abi_version": (C.c_int, []),
    "fid_last_error": (C.c_char_p, []),
    "fid_device_count": (C.c_int, [c_int_p]),
    "fid_ctx_create": (C.c_int, [C.c_int, C.c_void_p, c_void_pp]),
    "fid_ctx_destroy": (C.c_int, [C.c_void_p]),
    "fid_sync": (C.c_int, [C.c_void_p]),
    "fid_device_name": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    "fid_malloc": (C.c_int, [C.c_void_p, C.c_size_t, c_void_pp]),
    "fid_free": (C.c_int, [C.c_void_p, C.c_void_p]),
    "fid_memcpy_h2d": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "fid_memcpy_d2h": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "fid_memset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t]),
    "fid_pinned_alloc": (C.c_int, [C.c_void_p, C.c_size_t, c_void_pp]),
    "fid_pinned_free": (C.c_int, [C.c_void_p, C.c_void_p]),
    "fid_upload_async": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "fid_upload_wait": (C.c_int, [C.c_void_p]),
    "fid_upload_release": (C.c_int, [C.c_void_p, C.c_int]),
    "fid_upload_async_slot": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]),
    "fid_upload_wait_slot": (C.c_int, [C.c_void_p, C.c_int]),
    "fid_event_record": (C.c_int, [C.c_void_p, C.c_int]),
    "fid_event_elapsed_ms": (C.c_int, [C.c_void_p, C.c_int, C.c_int, c_f32_p]),
    "fid_net_create": (C.c_int, [C.c_void_p, c_i32_p, C.c_int, c_i32_p, C.c_int, C.c_void_p, C.c_size_t,
                                 C.c_int, C.c_int, C.c_int, c_void_pp]),
    "fid_net_destroy": (C.c_int, [C.c_void_p, C.c_void_p]),
    "fid_net_run": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "fid_net_set_sub_batch": (C.c_int, [C.c_void_p, C.c_int]),
    "fid_net_tensor": (C.c_int, [C.c_void_p, C.c_int, c_void_pp, c_int_p, c_int_p]),
    "fid_net_run_profiled": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, c_f32_p]),
    "fid_net_plan_save": (C.c_int, [C.c_void_p, C.c_char_p]),
    "fid_net_plan_load": (C.c_int, [C.c_void_p, C.c_char_p, c_int_p]),
    "fid_net_macs": (C.c_int, [C.c_void_p, c_f64_p]),
    "fid_letterbox": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                c_f64_p]),
    "fid_letterbox_ragged": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, c_i32_p, c_i64_p, C.c_int, C.c_void_p, C.c_int, C.c_int, c_f64_p]),
    "fid_nv12_to_bgr": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "fid_nv12_to_bgr_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "fid_bgr_to_nv12": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "fid_bgr_to_nv12_host": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "fid_letterbox_nv12": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, c_f64_p]),
    "fid_tile_cut_nv12": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, c_i32_p, C.c_int, C.c_void_p, C.c_int,
                                    C.c_int]),
    "fid_align_crops_nv12": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                       C.c_void_p, C.c_void_p]),
    "fid_align_crops_packed_nv12": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                              C.c_int, C.c_void_p, C.c_void_p]),
    "fid_scrfd_postprocess_ragged": (C.c_int, [C.c_void_p, c_void_pp, c_i32_p, c_i32_p, c_i64_p, C.c_int, C.c_int, C.c_int, C.c_int, c_i32_p,
                                               C.c_float, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "fid_align_crops_ragged": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, c_i32_p, c_i64_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                         C.c_void_p, C.c_void_p]),
    "fid_align_crops_packed_ragged": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, c_i32_p, c_i64_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                                C.c_int, C.c_void_p, C.c_void_p]),
    "fid_tile_cut": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, c_i32_p, C.c_int, C.c_void_p, C.c_int, C.c_int]),
    "fid_scrfd_postprocess_tiled": (C.c_int, [C.c_void_p, c_void_pp, c_i32_p, c_i32_p, c_i64_p, c_i32_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                              C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_int]),
    "fid_scrfd_postprocess": (C.c_int, [C.c_void_p, c_void_pp, c_i32_p, c_i32_p, c_i64_p, C.c_int, C.c_int,
                                        C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int,
                                        C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "fid_scrfd_set_candidate_capacity": (C.c_int, [C.c_void_p, C.c_int]),
    "fid_scrfd_check": (C.c_int, [C.c_void_p, c_int_p]),
    "fid_scrfd_decode": (C.c_int, [C.c_void_p, c_void_pp, c_i32_p, c_i32_p, c_i64_p, C.c_int, C.c_int, C.c_int,
                                   C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
    "fid_distance2bbox": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "fid_distance2kps": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "fid_nms": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
    "fid_align_crops": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                  C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "fid_l2_normalize_f16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "fid_l2_normalize_f16_slots": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "fid_face_pack": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int]),
    "fid_align_crops_packed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                         C.c_void_p, C.c_void_p]),
    "fid_l2_normalize_f16_packed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "fid_tracker_create": (C.c_int, [C.c_void_p, C.c_int, C.c_int, c_void_pp]),
    "fid_tracker_destroy": (C.c_int, [C.c_void_p, C.c_void_p]),
    "fid_tracker_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "fid_tracker_read": (C.c_int, [C.c_void_p, C.c_void_p, c_i32_p, c_i32_p]),
    "fid_track_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, c_i32_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_int]),
    "fid_track_identify": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, c_i32_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                     C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "fid_coaster_create": (C.c_int, [C.c_void_p, C.c_int, C.c_int, c_void_pp]),
    "fid_coaster_destroy": (C.c_int, [C.c_void_p, C.c_void_p]),
    "fid_coaster_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "fid_coaster_read": (C.c_int, [C.c_void_p, C.c_void_p, c_i32_p]),
    "fid_track_coast": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, c_i32_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fid_track_coast_host": (C.c_int, [c_i32_p, C.c_int, C.c_int, c_i32_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fid_relinker_create": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, c_void_pp]),
    "fid_relinker_destroy": (C.c_int, [C.c_void_p, C.c_void_p]),
    "fid_relinker_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "fid_relinker_read": (C.c_int, [C.c_void_p, C.c_void_p, c_i32_p, c_i32_p, c_i32_p, C.c_void_p, C.c_void_p]),
    "fid_track_relink": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, c_i32_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fid_track_relink_host": (C.c_int, [c_i32_p, C.c_void_p, c_i32_p, C.c_void_p, c_i32_p, C.c_int, C.c_int, C.c_int, C.c_int, c_i32_p, C.c_int,
                                        C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
    "fid_face_gates": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p]),
    "fid_face_measure": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fid_face_measure_host": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fid_face_gates_measured": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fid_shot_score": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "fid_shot_score_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "fid_shots_create": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_void_pp]),
    "fid_shots_destroy": (C.c_int, [C.c_void_p, C.c_void_p]),
    "fid_track_keep": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, c_i32_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                 C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fid_shots_flush": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "fid_shots_finished": (C.c_int, [C.c_void_p, C.c_void_p, c_i32_p, c_i32_p, c_void_pp, c_void_pp, c_void_pp]),
    "fid_shots_clear_finished": (C.c_int, [C.c_void_p, C.c_void_p]),
    "fid_shots_read": (C.c_int, [C.c_void_p, C.c_void_p, c_i32_p]),
    "fid_gallery_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, c_void_pp]),
    "fid_gallery_destroy": (C.c_int, [C.c_void_p, C.c_void_p]),
    "fid_gallery_info": (C.c_int, [C.c_void_p, c_int_p, c_int_p, c_int_p]),
    "fid_gallery_data": (C.c_int, [C.c_void_p, c_void_pp]),
    "fid_gallery_topk": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
    "fid_gallery_search": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
    "fid_topk_keys": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "fid_topk_merge": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
    "fid_quantize_rows_i8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "fid_quantize_rows_i8_host": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "fid_gallery_quantize": (C.c_int, [C.c_void_p, C.c_void_p]),
    "fid_gallery_quant_data": (C.c_int, [C.c_void_p, c_void_pp, c_void_pp]),
    "fid_coarse_keys": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "fid_rerank_keys": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "fid_gallery_search_coarse": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
    "fid_gallery_set_rows": (C.c_int, [C.c_void_p, C.c_void_p, c_i32_p, C.c_void_p, C.c_int]),
    "fid_gallery_range": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]),
    "fid_gallery_group": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_int,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fid_gallery_dedup": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fid_gallery_cluster": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p]),
    "fid_cluster_host": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p]),
    "fid_gallery_score_hist": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p]),
    "fid_score_hist_host": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p]),
    "fid_gallery_templates": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fid_templates_host": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fid_gallery_put_rows_f16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "fid_pair_verify": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_float,
                                  C.c_void_p, C.c_void_p, C.c_void_p]),
    "fid_match": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
    "fid_match_keys": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "fid_match_merge": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
    "fid_comm_unique_id": (C.c_int, [C.c_void_p, C.c_size_t]),
    "fid_comm_init_rank": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, c_void_pp]),
    "fid_comm_destroy": (C.c_int, [C.c_void_p, C.c_void_p]),
    "fid_comm_info": (C.c_int, [C.c_void_p, c_int_p, c_int_p]),
    "fid_allgather": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "fid_cosine_matrix": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
}

_lib = None
_lock = threading.Lock()


class FaceIdError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libfaceid error {code}: {msg}")
        self.code = code


def load():
    """dlopen libfaceid.so and attach the prototypes.  Raises if it has not been built
    (python __graft_entry__.py / make -C scrfd_arcface_facerecognition_amd/csrc)."""
    global _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise FileNotFoundError(
                    f"{LIB_PATH} not built: run `make -C {os.path.join(_HERE, 'csrc')}`; there is no CPU fallback")
            if os.environ.get("FID_LIB"):                 # never silently: a forgotten FID_LIB would test another build's kernels
                print(f"[faceid] FID_LIB={os.environ['FID_LIB']}: loading {LIB_PATH} instead of libfaceid.so", file=sys.stderr, flush=True)
            lib = C.CDLL(LIB_PATH)
            for name, (res, args) in SIGNATURES.items():
                fn = getattr(lib, name)      # AttributeError if the library lacks a declared symbol
                fn.restype = res
                fn.argtypes = args
            if lib.fid_abi_version() != 2:
                raise RuntimeError("libfaceid ABI version mismatch")
            _lib = lib
    return _lib


def check(rc):
    if rc != 0:
        raise FaceIdError(rc, load().fid_last_error().decode("utf-8", "replace"))


def device_count() -> int:
    n = C.c_int(0)
    check(load().fid_device_count(C.byref(n)))
    return n.value


def _ptr(x):
    """device pointer (int / c_void_p / DeviceBuffer / torch tensor) -> c_void_p"""
    if x is None:
        return C.c_void_p(0)
    if isinstance(x, DeviceBuffer):
        return C.c_void_p(x.ptr)
    if isinstance(x, int):
        return C.c_void_p(x)
    if hasattr(x, "data_ptr"):
        return C.c_void_p(x.data_ptr())
    return x


def pack_images(images):
    """A mixed-size batch as the *_ragged entry points take it (include/faceid.h): the images, each uint8 [H,W,3] with H, W >= 1, concatenated
    in input order without padding.  -> (buffer uint8 1-D, hw int32 [B,2], offsets int64 [B]); pure numpy."""
    images = list(images)
    if not images:
        raise ValueError("pack_images: no images")
    hw = np.empty((len(images), 2), np.int32)
    for i, im in enumerate(images):
        shape, dtype = getattr(im, "shape", None), getattr(im, "dtype", None)
        if dtype != np.uint8 or shape is None or len(shape) != 3 or shape[2] != 3 or shape[0] < 1 or shape[1] < 1:
            raise ValueError(f"pack_images: image {i} is {dtype} {shape}, expected uint8 [H,W,3] with H, W >= 1")
        hw[i] = shape[:2]
    sizes = hw[:, 0].astype(np.int64) * hw[:, 1].astype(np.int64) * 3
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    buf = np.empty(int(sizes.sum()), np.uint8)
    for im, o, n in zip(images, offsets, sizes):
        buf[o:o + n] = np.asarray(im).reshape(-1)
    return buf, hw, offsets


class ImageBatch:
    """A mixed-size batch on the device (Context.image_batch): `.frames` the one allocation, `.hw` / `.offsets` the host arrays the
    *_ragged entry points read, `.nbytes` the allocation's size, `.B` the number of images.  `.args()` = the four leading arguments
    (frames_dev, frames_bytes, hw, offsets) of those entry points."""

    def __init__(self, ctx: "Context", images):
        buf, self.hw, self.offsets = pack_images(images)
        self.frames = ctx.to_device(buf)
        self.nbytes, self.B = int(buf.nbytes), len(self.hw)

    def args(self):
        return (C.c_void_p(self.frames.ptr), C.c_size_t(self.nbytes), self.hw.ctypes.data_as(c_i32_p), self.offsets.ctypes.data_as(c_i64_p))


class DeviceBuffer:
    """A typed view of device memory owned by the library's allocator (or borrowed)."""

    def __init__(self, ctx: "Context", shape, dtype, ptr=None):
        self.ctx = ctx
        self.shape = tuple(int(s) for s in shape)
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        self.owned = ptr is None
        if ptr is None:
            p = C.c_void_p()
            check(ctx.lib.fid_malloc(ctx.handle, max(self.nbytes, 16), C.byref(p)))
            ptr = p.value
        self.ptr = int(ptr)

    def upload(self, arr):
        arr = np.ascontiguousarray(arr, dtype=self.dtype)
        assert arr.nbytes == self.nbytes, (arr.shape, self.shape)
        check(self.ctx.lib.fid_memcpy_h2d(self.ctx.handle, C.c_void_p(self.ptr), arr.ctypes.data_as(C.c_void_p), self.nbytes))
        self.ctx._keepalive = arr      # the copy is asynchronous with respect to the host
        self.ctx.sync()
        return self

    def download(self, count_bytes=None):
        out = np.empty(self.shape, dtype=self.dtype)
        n = self.nbytes if count_bytes is None else count_bytes
        check(self.ctx.lib.fid_memcpy_d2h(self.ctx.handle, out.ctypes.data_as(C.c_void_p), C.c_void_p(self.ptr), n))
        return out

    def zero(self):
        check(self.ctx.lib.fid_memset(self.ctx.handle, C.c_void_p(self.ptr), 0, self.nbytes))
        return self

    def free(self):
        if self.owned and self.ptr:
            self.ctx.lib.fid_free(self.ctx.handle, C.c_void_p(self.ptr))
            self.ptr = 0

    def __del__(self):
        try:
            if self.ctx.handle:
                self.free()
        except Exception:
            pass


class Context:
    """fid_ctx: one HIP device + stream.  `stream` may be a raw hipStream_t (e.g.
    torch.cuda.current_stream().cuda_stream) so library work is ordered with torch/RCCL work."""

    def __init__(self, device: int = 0, stream: int | None = None):
        self.lib = load()
        h = C.c_void_p()
        check(self.lib.fid_ctx_create(int(device), C.c_void_p(stream or 0), C.byref(h)))
        self.handle = h
        self.device = int(device)
        self._keepalive = None

    def sync(self):
        check(self.lib.fid_sync(self.handle))

    def name(self) -> str:
        buf = C.create_string_buffer(256)
        check(self.lib.fid_device_name(self.handle, buf, 256))
        return buf.value.decode()

    def empty(self, shape, dtype) -> DeviceBuffer:
        return DeviceBuffer(self, shape, dtype)

    def to_device(self, arr) -> DeviceBuffer:
        arr = np.ascontiguousarray(arr)
        return DeviceBuffer(self, arr.shape, arr.dtype).upload(arr)

    def image_batch(self, images) -> ImageBatch:
        """images of differing sizes, uploaded once as one allocation (pack_images)"""
        return ImageBatch(self, images)

    def borrow(self, ptr, shape, dtype) -> DeviceBuffer:
        return DeviceBuffer(self, shape, dtype, ptr=ptr)

    def event_record(self, slot: int):
        check(self.lib.fid_event_record(self.handle, slot))

    def elapsed_ms(self, a: int, b: int) -> float:
        ms = C.c_float()
        check(self.lib.fid_event_elapsed_ms(self.handle, a, b, C.byref(ms)))
        return ms.value

    def close(self):
        if self.handle:
            self.lib.fid_ctx_destroy(self.handle)
            self.handle = None


_default_ctx = {}


def default_context(device: int = 0) -> Context:
    """Process-wide context per device (the reference keeps one global ORT session per model)."""
    if device not in _default_ctx:
        _default_ctx[device] = Context(device)
    return _default_ctx[device]
