"""The redaction of fid_redact_faces / fid_redact_faces_nv12 (include/faceid.h), restated in plain numpy loops from the header's text -- not
from csrc/redact_core.h: per face in ascending order, cell by cell from the anchor, every mean from a snapshot of the frame taken before the
first write, every write over whatever an earlier face left.  Also the case list the CPU and the GPU tests share."""
import numpy as np

import draw_nv12_oracle as N
import draw_oracle as O

MOSAIC, FILL = 0, 1
UNKNOWN, KNOWN = 1, 2


class Style:
    def __init__(self, mode=MOSAIC, who=UNKNOWN, cells=8, expand=0.1, fill_bgr=(0, 0, 0)):
        self.mode, self.who, self.cells, self.expand, self.fill_bgr = mode, who, cells, float(expand), tuple(fill_bgr)


def geometry(box, style):
    """the unclipped region and the cell edge of one det row: dict(x1, y1, x2, y2, w, h, rx0, ry0, rx1, ry1, c), or None for a skipped face"""
    v = np.asarray(box[:4], np.float32)
    if not np.all(np.isfinite(v)) or not np.all(np.abs(v) < 2.0 ** 23):
        return None
    x1, y1, x2, y2 = (int(c) for c in v)                    # int(): toward zero
    w, h = x2 - x1, y2 - y1
    if not (w > 0 and h > 0):
        return None
    mx, my = int(style.expand * float(w)), int(style.expand * float(h))
    rx0, ry0 = ((x1 - mx) // 2) * 2, ((y1 - my) // 2) * 2   # //: floor, also for negatives
    rx1, ry1 = (x2 + mx) | 1, (y2 + my) | 1
    q = max(w, h) // style.cells
    c = max(2, q + (q & 1))
    return dict(x1=x1, y1=y1, x2=x2, y2=y2, w=w, h=h, rx0=rx0, ry0=ry0, rx1=rx1, ry1=ry1, c=c)


def clipped(g, H, W):
    """the region intersected with the frame, inclusive (x0, y0, x1, y1), or None when nothing is left"""
    x0, y0, x1, y1 = max(g["rx0"], 0), max(g["ry0"], 0), min(g["rx1"], W - 1), min(g["ry1"], H - 1)
    return (x0, y0, x1, y1) if x0 <= x1 and y0 <= y1 else None


def disjoint(regions):
    """do no two of the inclusive rectangles (x0, y0, x1, y1) share a pixel?"""
    for i, a in enumerate(regions):
        for b in regions[i + 1:]:
            if max(a[0], b[0]) <= min(a[2], b[2]) and max(a[1], b[1]) <= min(a[3], b[3]):
                return False
    return True


def cell_rects(g, H, W):
    """the non-empty clipped cells of one face, each inclusive (xa, ya, xb, yb)"""
    r = clipped(g, H, W)
    if r is None:
        return
    c = g["c"]
    top = g["ry0"]
    while top <= g["ry1"]:
        left = g["rx0"]
        while left <= g["rx1"]:
            xa, ya, xb, yb = max(left, r[0]), max(top, r[1]), min(left + c - 1, r[2]), min(top + c - 1, r[3])
            if xa <= xb and ya <= yb:
                yield xa, ya, xb, yb
            left += c
        top += c


def cells_per_face(g):
    """cells of the unclipped region"""
    c = g["c"]
    return -(-(g["rx1"] - g["rx0"] + 1) // c) * -(-(g["ry1"] - g["ry0"] + 1) // c)


def mean(values):
    n = int(values.size)
    s = int(values.astype(np.int64).sum())
    return (s + n // 2) // n, (2 * (s % n) == n)


def selected_faces(B, det, counts, cap, idx=None, id_stride=0, offsets=None, n_rows=0, style=None, **_):
    """(frame, face, geometry) of every selected face that is not skipped, in ascending order"""
    style = style or Style()
    det = np.asarray(det, np.float32).reshape(B, cap, 5)
    for b, n in enumerate(O.face_counts(B, counts, cap, idx, id_stride, offsets, n_rows)):
        for f in range(n):
            known = False
            if idx is not None:
                j = int(offsets[b]) + f if offsets is not None else b * id_stride + f
                known = int(np.asarray(idx).reshape(-1)[j]) >= 0
            if not (style.who & (KNOWN if known else UNKNOWN)):
                continue
            g = geometry(det[b, f], style)
            if g is not None:
                yield b, f, g


def redact(frames, det, counts, cap, idx=None, score=None, id_stride=0, offsets=None, n_rows=0, style=None, sequential=False, stats=None):
    """-> the redacted copy of frames uint8 [B,H,W,3].  sequential=True is NOT the definition: it takes each face's means from what the
    faces before it left (what applying the faces one after another would give).  stats: a dict that receives halfway (cells x channels
    whose sum is exactly half-way) and cells."""
    style = style or Style()
    out = np.array(frames, dtype=np.uint8, copy=True)
    B, H, W = out.shape[:3]
    before = out.copy()
    half = cells = 0
    for b, f, g in selected_faces(B, det, counts, cap, idx, id_stride, offsets, n_rows, style):
        src = out[b].copy() if sequential else before[b]
        for xa, ya, xb, yb in cell_rects(g, H, W):
            if style.mode == FILL:
                out[b, ya:yb + 1, xa:xb + 1] = np.array(style.fill_bgr[:3], np.uint8)
                continue
            cells += 1
            for ch in range(3):
                m, hw = mean(src[ya:yb + 1, xa:xb + 1, ch])
                half += hw
                out[b, ya:yb + 1, xa:xb + 1, ch] = m
    if stats is not None:
        stats.update(halfway=half, cells=cells)
    return out


def redact_nv12(buf, B, H, W, det, counts, cap, standard="bt601", pitch=None, uv_offset=None, frame_stride=None, idx=None, score=None,
                id_stride=0, offsets=None, n_rows=0, style=None, stats=None):
    """-> the redacted copy of the flat allocation buf"""
    style = style or Style()
    out = np.array(buf, dtype=np.uint8, copy=True).reshape(-1)
    before = out.copy()
    half = 0
    for b, f, g in selected_faces(B, det, counts, cap, idx, id_stride, offsets, n_rows, style):
        y, uv = N.planes(out, b, H, W, pitch, uv_offset, frame_stride)
        y0, uv0 = N.planes(before, b, H, W, pitch, uv_offset, frame_stride)
        for xa, ya, xb, yb in cell_rects(g, H, W):
            assert xa % 2 == 0 and ya % 2 == 0 and xb % 2 == 1 and yb % 2 == 1      # whole 2 x 2 groups
            ga, gb, ha, hb = xa // 2, xb // 2, ya // 2, yb // 2
            if style.mode == FILL:
                yc, uc, vc = N.colour_yuv(style.fill_bgr, standard)
            else:
                (yc, h0), (uc, h1), (vc, h2) = mean(y0[ya:yb + 1, xa:xb + 1]), mean(uv0[ha:hb + 1, ga:gb + 1, 0]), mean(uv0[ha:hb + 1, ga:gb + 1, 1])
                half += h0 + h1 + h2
            y[ya:yb + 1, xa:xb + 1] = yc
            uv[ha:hb + 1, ga:gb + 1, 0] = uc
            uv[ha:hb + 1, ga:gb + 1, 1] = vc
    if stats is not None:
        stats.update(halfway=half)
    return out


# ---- the shared case list ------------------------------------------------------------------------------------

B, CAP = 3, 8
BIG = 8388608.0                                              # 2^23: a box that reaches it is skipped


def scene(H, W):
    """det [3,8,5].  Frame 0: two overlapping faces, a fractional box, a 2^23 box, w = h = 1, a 20-pixel face.  Frame 1: a face across each
    of the four edges (the left one with a negative odd x1 - mx), one wholly outside.  Frame 2: edges on columns 63 | 64 and rows 15 | 16,
    h = 1, w = 0, a NaN"""
    nan = np.nan
    boxes = [
        [(10, 20, 40, 44), (25, 22, 60, 46), (3.7, 30.2, 20.9, 44.5), (BIG, 5, BIG + 64, 30), (40, 2, 62, 18), (5, 5, 6, 6), (30, 26, 50, 40),
         (1, 1, 9, 8)],
        [(-9, 15, 12, 40), (W - 15, 10, W + 9, 35), (20, -8, 45, 14), (30, H - 12, 52, H + 10), (-30, -30, -5, -5), (18, 18, 40, 33),
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


IDX = np.array([0, -1, 1, 7, -1, 12, -1, 0], np.int32)      # (no label table is involved: 7 and 12 are known like 0 and 1)
SCORE = np.array([0.125, 0.999, 1.0000001, 0.5, np.nan, -0.3, 0.73, 0.25], np.float32)
ROW_OFFSETS = np.array([0, 3, 7, 15], np.int32)
FILL_COLOUR = (200, 30, 90)


def cases(H, W):
    """[(name, kwargs of redact() / of the entry points)]: det, counts, idx, score, id_stride, offsets, n_rows, style"""
    det = scene(H, W)
    full = np.full(B, CAP, np.int32)
    idx = np.stack([np.roll(IDX, b) for b in range(B)])
    score = np.stack([np.roll(SCORE, 2 * b) for b in range(B)])
    row_idx, row_score = np.resize(IDX, 24), np.resize(SCORE, 24)
    forms = {"detections only": dict(idx=None, score=None, id_stride=0, offsets=None, n_rows=0),
             "slots": dict(idx=idx, score=score, id_stride=CAP, offsets=None, n_rows=0),
             "rows": dict(idx=row_idx, score=row_score, id_stride=0, offsets=ROW_OFFSETS, n_rows=12)}
    out = []
    for form, ident in forms.items():
        for who in (UNKNOWN, KNOWN, UNKNOWN | KNOWN):
            out.append((f"{form}, who {who}", dict(det=det, counts=full, style=Style(who=who), **ident)))
    everyone = dict(det=det, counts=full, **forms["slots"])
    both = UNKNOWN | KNOWN
    sw = det.copy()
    sw[0, [0, 1]] = sw[0, [1, 0]]
    out.append(("the two overlapping faces swapped", dict(everyone, det=sw, style=Style(who=both))))
    out.append(("rows cut inside frame 1", dict(everyone, **dict(forms["rows"], n_rows=5), style=Style(who=both))))
    out.append(("two slots per frame", dict(everyone, idx=idx[:, :2].copy(), score=score[:, :2].copy(), id_stride=2, style=Style(who=both))))
    out.append(("counts 0, -2, cap + 3", dict(everyone, counts=np.array([0, -2, CAP + 3], np.int32), style=Style(who=both))))
    out.append(("an empty frame between two redacted ones", dict(everyone, counts=np.array([3, 0, CAP], np.int32), style=Style(who=both))))
    whole = det.copy()
    whole[2, 0, :4] = (0, 0, W - 1, H - 1)
    out.append(("one box covers the frame, cells 1", dict(everyone, det=whole, counts=np.array([CAP, CAP, 1], np.int32),
                                                          style=Style(who=both, cells=1, expand=0.0))))
    apart = det.copy()
    apart[:, :4, :4] = [(2, 2, 14, 14), (30, 4, 50, 20), (4, 24, 24, 44), (40, 26, 60, 40)]
    out.append(("four faces apart", dict(everyone, det=apart, counts=np.full(B, 4, np.int32), style=Style(who=both))))
    out.append(("cells 16, expand 0.5", dict(everyone, style=Style(who=both, cells=16, expand=0.5))))
    out.append(("cells 3, expand 0", dict(everyone, style=Style(who=both, cells=3, expand=0.0))))
    out.append(("fill, a colour that is not grey", dict(everyone, style=Style(mode=FILL, who=both, fill_bgr=FILL_COLOUR))))
    out.append(("fill, unknown faces only, expand 0.25", dict(everyone, style=Style(mode=FILL, who=UNKNOWN, expand=0.25, fill_bgr=(255, 255, 255)))))
    return out
