"""The overlay of fid_draw_faces / fid_draw_faces_host (include/faceid.h), restated in numpy from the raster rules -- not from csrc/draw_core.h:
text pixels are filled block by block per glyph bit, the arms corner by corner, everything through boolean masks over the whole frame.  The
glyph bits come from the library (fid_draw_glyphs), so the font exists once.  Also the case list the CPU and the GPU tests share."""
import numpy as np

LABEL_MAX = 32
TRACK_ID = 1


class Style:
    def __init__(self, proportion=0.2, thickness=3, text_scale=2, bar=1, flags=0, unknown_bgr=(255, 0, 0)):
        self.proportion, self.thickness, self.text_scale, self.bar, self.flags = float(proportion), thickness, text_scale, bar, flags
        self.unknown_bgr = tuple(unknown_bgr)


def default_bgr(g):
    h = ((g + 1) * 2654435761) & 0xFFFFFFFF
    return (h >> 24, (h >> 16) & 255, (h >> 8) & 255)


def clean_score(score):
    s = np.float32(score)
    return s if np.isfinite(s) and s > 0 else np.float32(0)


def cents_of(scores):
    """hundredths of fp32 scores (any shape), nearest with ties to even on the exact double product, at most 999; not finite or <= 0 -> 0"""
    s = np.asarray(scores, np.float32)
    with np.errstate(invalid="ignore"):
        s = np.where(np.isfinite(s) & (s > 0), s, np.float32(0)).astype(np.float32)
    return np.minimum(np.rint(s.astype(np.float64) * 100.0), 999).astype(np.int64)


def two_decimals(score):
    cents = int(cents_of(score))
    return f"{cents // 100}.{(cents // 10) % 10}{cents % 10}"


def corner_length(m, proportion=0.2):
    return int(proportion * float(m))


def shown_name(name):
    raw = name if isinstance(name, (bytes, bytearray)) else str(name).encode("utf-8")
    return "".join(chr(c) if 0x20 <= c <= 0x7E else "?" for c in raw[:LABEL_MAX])


def label_text(known, name, score, track_id=-1, flags=0):
    tag = f"#{track_id}" if (flags & TRACK_ID) and track_id >= 0 else ""
    if not known:
        return tag
    return (tag + " " if tag else "") + shown_name(name) + ": " + two_decimals(score)


def face_mask(H, W, box, known, score, text, style, glyphs):
    """bool [H,W]: the pixel set of one face, or None when it draws nothing"""
    v = np.asarray(box[:4], np.float32)
    if not np.all(np.isfinite(v)) or not np.all(np.abs(v) < 2.0 ** 23):
        return None
    x1, y1, x2, y2 = (int(c) for c in v)                    # int(): toward zero
    w, h = x2 - x1, y2 - y1
    if not (w > 0 and h > 0):
        return None
    Y, X = np.mgrid[0:H, 0:W]
    L = corner_length(min(w, h), style.proportion)
    r = (style.thickness - 1) // 2
    m = ((X >= x1) & (X <= x2) & ((Y == y1) | (Y == y2))) | ((Y >= y1) & (Y <= y2) & ((X == x1) | (X == x2)))
    for cx, cy, sx, sy in ((x1, y1, 1, 1), (x2, y1, -1, 1), (x1, y2, 1, -1), (x2, y2, -1, -1)):
        xa, xb = sorted((cx, cx + sx * L))
        ya, yb = sorted((cy, cy + sy * L))
        m |= (X >= xa - r) & (X <= xb + r) & (np.abs(Y - cy) <= r)
        m |= (Y >= ya - r) & (Y <= yb + r) & (np.abs(X - cx) <= r)
    if known and style.bar:
        with np.errstate(over="ignore"):
            p = clean_score(score) * np.float32(h)          # fp32 product
        bh = int(min(float(p), 2.0 ** 24))                  # (2^24 rows or more: above every frame either way)
        m |= (X >= x2 + 10) & (X <= x2 + 20) & (Y >= y2 - bh) & (Y <= y2)
    t = style.text_scale
    if t > 0:
        for k, ch in enumerate(text):
            g = glyphs[ord(ch) - 0x20]
            left, bottom = x1 + 6 * t * k, y1 - 10
            for row in range(7):
                for col in range(5):
                    if (int(g[row]) >> (4 - col)) & 1:
                        xs, ye = left + col * t, bottom - (6 - row) * t
                        m[max(ye - t + 1, 0):max(ye + 1, 0), max(xs, 0):max(xs + t, 0)] = True
    return m


def face_counts(B, counts, cap, idx, id_stride, offsets, n_rows):
    out = []
    for b in range(B):
        if idx is None:
            n = min(max(int(counts[b]), 0), cap)
        elif offsets is None:
            n = min(max(int(counts[b]), 0), cap, id_stride)
        else:
            n = min(max(min(int(offsets[b + 1]), n_rows) - int(offsets[b]), 0), cap)
        out.append(n)
    return out


def draw(frames, det, counts, cap, glyphs, idx=None, score=None, id_stride=0, offsets=None, n_rows=0, track=None, names=None, bgr=None,
         style=None):
    """-> the annotated copy of frames uint8 [B,H,W,3]"""
    style = style or Style()
    out = np.array(frames, dtype=np.uint8, copy=True)
    B, H, W = out.shape[:3]
    det = np.asarray(det, np.float32).reshape(B, cap, 5)
    G = len(names) if names is not None else 0
    for b, n in enumerate(face_counts(B, counts, cap, idx, id_stride, offsets, n_rows)):
        for f in range(n):
            i, sc = -1, 0.0
            if idx is not None:
                j = int(offsets[b]) + f if offsets is not None else b * id_stride + f
                i, sc = int(np.asarray(idx).reshape(-1)[j]), np.asarray(score, np.float32).reshape(-1)[j]
            known = 0 <= i < G
            tid = int(np.asarray(track).reshape(B, cap, 2)[b, f, 0]) if track is not None else -1
            colour = (tuple(bgr[i]) if bgr is not None else default_bgr(i)) if known else style.unknown_bgr
            text = label_text(known, names[i] if known else None, sc, tid, style.flags)
            m = face_mask(H, W, det[b, f], known, sc, text, style, glyphs)
            if m is not None:
                out[b][m] = np.array(colour[:3], np.uint8)  # ascending f: the highest face index shows
    return out


# ---- the shared case list ------------------------------------------------------------------------------------

NAMES = [b"ann", b"Bob_the_builder_with_a_very_long_name_xy", "Zoë".encode("utf-8"), b"d"]      # 3, 40 and 4 bytes (two of them one letter), 1
G = len(NAMES)
B, CAP = 3, 8


def scene(H, W):
    """det [3,8,5]: frame 0 two overlapping faces, a fractional box and an out-of-range one; frame 1 a face across each of the four edges;
    frame 2 text cut at the top, bar cut at the right, edges on columns 63 | 64 and rows 15 | 16, w = 1, h = 1, w = 0, a NaN"""
    nan = np.nan
    boxes = [
        [(10, 20, 40, 44), (25, 22, 60, 46), (3.7, 30.2, 20.9, 44.5), (3e7, 5, 3.00001e7, 30), (40, 2, 62, 18), (5, 5, 15, 14), (44, 25, 60, 36),
         (1, 1, 9, 8)],
        [(-10, 15, 12, 40), (W - 15, 10, W + 9, 35), (20, -8, 45, 14), (30, H - 12, 52, H + 10), (-30, -30, -5, -5), (18, 18, 40, 33),
         (W - 30, H - 20, W - 6, H - 3), (2, 2, 30, 12)],
        [(5, 12, 30, 33), (W - 40, 14, W - 12, 36), (50, 5, 63, 15), (64, 16, 66, 30), (10.2, 20, 11.9, 34), (20, 30, 40, 31.5),
         (30.1, 20, 30.9, 34), (nan, 5, 20, 20)],
    ]
    det = np.zeros((B, CAP, 5), np.float32)
    for b, fr in enumerate(boxes):
        for f, bx in enumerate(fr):
            det[b, f, :4] = bx
            det[b, f, 4] = 0.5 + 0.05 * f
    return det


IDX = np.array([0, -1, 1, G, 2, G + 5, 3, 0], np.int32)
SCORE = np.array([0.125, 0.999, 1.0000001, 0.5, np.nan, -0.3, 0.73, 0.25], np.float32)


def cases(H, W):
    """[(name, kwargs of draw() / of the entry points)]: det, counts, idx, score, id_stride, offsets, n_rows, track, names, bgr, style"""
    det = scene(H, W)
    full = np.full(B, CAP, np.int32)
    idx = np.stack([np.roll(IDX, b) for b in range(B)])
    score = np.stack([np.roll(SCORE, 2 * b) for b in range(B)])
    base = dict(det=det, counts=full, idx=idx, score=score, id_stride=CAP, offsets=None, n_rows=0, track=None, names=NAMES, bgr=None, style=Style())
    out = [("slots", dict(base))]
    sw = det.copy()
    sw[0, [0, 1]] = sw[0, [1, 0]]
    out.append(("slots, the two overlapping faces swapped", dict(base, det=sw)))
    out.append(("detections only", dict(base, idx=None, score=None)))
    out.append(("no label table", dict(base, names=None)))
    row_idx, row_score = np.resize(IDX, 24), np.resize(SCORE, 24)
    out.append(("rows", dict(base, idx=row_idx, score=row_score, offsets=np.array([0, 3, 7, 15], np.int32), n_rows=12)))
    out.append(("rows cut inside frame 1", dict(base, idx=row_idx, score=row_score, offsets=np.array([0, 3, 7, 15], np.int32), n_rows=5)))
    out.append(("counts 0, -2, cap + 3", dict(base, counts=np.array([0, -2, CAP + 3], np.int32))))
    out.append(("an empty frame between two drawn ones", dict(base, counts=np.array([3, 0, CAP], np.int32))))
    out.append(("two slots per frame", dict(base, idx=idx[:, :2].copy(), score=score[:, :2].copy(), id_stride=2)))
    track = np.full((B, CAP, 2), -1, np.int32)
    track[:, :, 0] = np.array([0, 1234567, -1, 5, 42, 7, 2147483647, 9], np.int32)
    track[:, :, 1] = np.arange(CAP)
    out.append(("track ids", dict(base, track=track, style=Style(flags=TRACK_ID, text_scale=1))))
    out.append(("track ids given, flag off", dict(base, track=track)))
    colours = np.array([(1, 2, 3), (250, 128, 0), (0, 255, 255), (90, 90, 200)], np.uint8)
    out.append(("thickness 1, no text", dict(base, style=Style(thickness=1, text_scale=0), bgr=colours)))
    out.append(("thickness 7, text 3, no bar", dict(base, style=Style(thickness=7, text_scale=3, bar=0, unknown_bgr=(7, 8, 9)))))
    out.append(("thickness 3, text 1, proportion 0.35", dict(base, style=Style(thickness=3, text_scale=1, proportion=0.35))))
    out.append(("thickness 15, text 4, proportion 1", dict(base, style=Style(thickness=15, text_scale=4, proportion=1.0))))
    return out
