"""BGR -> NV12 and the overlay on NV12 frames (fid_bgr_to_nv12, fid_draw_faces_nv12; include/faceid.h), restated in numpy from the header's
text -- not from csrc/yuv_core.h or csrc/draw.hip: the forward tables from (kr, kb) by the formula, int64 arithmetic, box-filtered chroma; the
overlay from draw_oracle.face_mask per face in order: Y where the mask is set, a pair where the mask's 2 x 2 OR is set."""
import math

import numpy as np

import draw_oracle as O

# standard -> (kr, kb, limited range)
STANDARDS = {"bt601": (0.299, 0.114, True), "bt709": (0.2126, 0.0722, True), "bt601_full": (0.299, 0.114, False)}
MACRO = {"bt601": "FID_YUV_BT601_LIMITED_FWD_TABLE", "bt709": "FID_YUV_BT709_LIMITED_FWD_TABLE", "bt601_full": "FID_YUV_BT601_FULL_FWD_TABLE"}
SHIFT = 20


def table(standard):
    """(YB, YG, YR, UB, UG, UR, VB, VG, VR, Y offset): floor(c * 2^20 + 0.5) of the standard's matrix, rows on (B, G, R)"""
    kr, kb, limited = STANDARDS[standard]
    kg = 1.0 - kr - kb
    ys, cs = (219.0 / 255.0, 224.0 / 255.0) if limited else (1.0, 1.0)
    rows = [ys * kb, ys * kg, ys * kr,
            cs * 0.5, cs * 0.5 * (-kg / (1.0 - kb)), cs * 0.5 * (-kr / (1.0 - kb)),
            cs * 0.5 * (-kb / (1.0 - kr)), cs * 0.5 * (-kg / (1.0 - kr)), cs * 0.5]
    return tuple(int(math.floor(c * (1 << SHIFT) + 0.5)) for c in rows) + (16 if limited else 0,)


def luma(bgr, standard="bt601"):
    """uint8 [..., 3] -> int64 [...]"""
    t = table(standard)
    p = np.asarray(bgr).astype(np.int64)
    return np.clip((t[0] * p[..., 0] + t[1] * p[..., 1] + t[2] * p[..., 2] + (t[9] << SHIFT) + (1 << (SHIFT - 1))) >> SHIFT, 0, 255)


def chroma(sums, standard="bt601"):
    """the sums of a group's four pixels, int [..., 3] -> int64 [..., 2] (U, V)"""
    t = table(standard)
    s = np.asarray(sums).astype(np.int64)
    bias = (128 << (SHIFT + 2)) + (1 << (SHIFT + 1))
    u = (t[3] * s[..., 0] + t[4] * s[..., 1] + t[5] * s[..., 2] + bias) >> (SHIFT + 2)
    v = (t[6] * s[..., 0] + t[7] * s[..., 1] + t[8] * s[..., 2] + bias) >> (SHIFT + 2)
    return np.clip(np.stack([u, v], axis=-1), 0, 255)


def colour_yuv(bgr, standard="bt601"):
    """one solid colour -> (Y, U, V): Y(c) and the pair of the flat group S = 4 * c"""
    c = np.asarray(bgr[:3], np.int64)
    u, v = chroma(4 * c, standard)
    return int(luma(c, standard)), int(u), int(v)


def layout(H, W, pitch=None, uv_offset=None, frame_stride=None):
    pitch = W if pitch is None else pitch
    uv_offset = pitch * H if uv_offset is None else uv_offset
    frame_stride = uv_offset + pitch * (H // 2) if frame_stride is None else frame_stride
    return pitch, uv_offset, frame_stride


def planes(buf, b, H, W, pitch=None, uv_offset=None, frame_stride=None):
    """writable views of frame b of the flat allocation buf: (Y [H, W], UV [H/2, W/2, 2])"""
    pitch, uv_offset, frame_stride = layout(H, W, pitch, uv_offset, frame_stride)
    f = b * frame_stride
    y = np.lib.stride_tricks.as_strided(buf[f:], (H, W), (pitch, 1))
    uv = np.lib.stride_tricks.as_strided(buf[f + uv_offset:], (H // 2, W // 2, 2), (pitch, 2, 1))
    return y, uv


def bgr_to_nv12(frames, out, standard="bt601", **lay):
    """frames uint8 [B,H,W,3] -> written into the flat allocation `out` (uint8 1-D, modified in place and returned): only the first W bytes
    of every Y row and of every UV row change"""
    frames = np.asarray(frames, np.uint8)
    B, H, W = frames.shape[:3]
    for b in range(B):
        y, uv = planes(out, b, H, W, **lay)
        y[...] = luma(frames[b], standard)
        s = frames[b].astype(np.int64).reshape(H // 2, 2, W // 2, 2, 3).sum(axis=(1, 3))
        uv[...] = chroma(s, standard)
    return out


def faces_in_order(B, H, W, det, counts, cap, glyphs, idx=None, score=None, id_stride=0, offsets=None, n_rows=0, track=None, names=None, bgr=None,
                   style=None):
    """(frame, face, bool [H,W] mask, (b, g, r)) of every face that draws something, in draw order: the records of draw_oracle.draw"""
    style = style or O.Style()
    det = np.asarray(det, np.float32).reshape(B, cap, 5)
    G = len(names) if names is not None else 0
    for b, n in enumerate(O.face_counts(B, counts, cap, idx, id_stride, offsets, n_rows)):
        for f in range(n):
            i, sc = -1, 0.0
            if idx is not None:
                j = int(offsets[b]) + f if offsets is not None else b * id_stride + f
                i, sc = int(np.asarray(idx).reshape(-1)[j]), np.asarray(score, np.float32).reshape(-1)[j]
            known = 0 <= i < G
            tid = int(np.asarray(track).reshape(B, cap, 2)[b, f, 0]) if track is not None else -1
            colour = (tuple(bgr[i]) if bgr is not None else O.default_bgr(i)) if known else style.unknown_bgr
            text = O.label_text(known, names[i] if known else None, sc, tid, style.flags)
            m = O.face_mask(H, W, det[b, f], known, sc, text, style, glyphs)
            if m is not None:
                yield b, f, m, tuple(int(c) for c in colour[:3])


def draw_nv12(buf, B, H, W, det, counts, cap, glyphs, standard="bt601", pitch=None, uv_offset=None, frame_stride=None, **faces):
    """-> the annotated copy of the flat allocation buf; faces: the keywords of faces_in_order (those of draw_oracle.draw)"""
    out = np.array(buf, dtype=np.uint8, copy=True).reshape(-1)
    for b, _, m, colour in faces_in_order(B, H, W, det, counts, cap, glyphs, **faces):
        y, uv = planes(out, b, H, W, pitch, uv_offset, frame_stride)
        yc, uc, vc = colour_yuv(colour, standard)
        y[m] = yc                                                 # ascending f: the highest face index shows
        uv[m.reshape(H // 2, 2, W // 2, 2).any(axis=(1, 3))] = (uc, vc)
    return out


def last_face(B, H, W, det, counts, cap, glyphs, **faces):
    """int [B,H,W]: per pixel the index of the last face whose set contains it, -1 where none does"""
    out = np.full((B, H, W), -1, np.int64)
    for b, f, m, _ in faces_in_order(B, H, W, det, counts, cap, glyphs, **faces):
        out[b][m] = f
    return out


def header_tables(path):
    """the ten integers of each FID_YUV_*_FWD_TABLE macro of include/faceid.h"""
    import re
    src = open(path).read()
    out = {}
    for std, macro in MACRO.items():
        m = re.search(r"#define\s+" + macro + r"\s+\{([^}]*)\}", src)
        assert m, macro
        out[std] = tuple(int(v) for v in m.group(1).split(","))
    return out
