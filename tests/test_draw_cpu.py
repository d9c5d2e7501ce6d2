"""CPU: the overlay's arithmetic and fid_draw_faces_host (include/faceid.h) against tests/draw_oracle.py, byte for byte over the whole buffer;
the font table's shape; every refusal; the utils/helpers shims on a host without OpenCV.  libfaceid.so loads without a GPU."""
import ctypes as C
import sys

import numpy as np
import pytest

import draw_oracle as O
from draw_calls import c_style, host_draw


@pytest.fixture(scope="module")
def lib():
    from scrfd_arcface_facerecognition_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def glyphs(lib):
    out = np.zeros(95 * 7, np.uint8)
    assert lib.fid_draw_glyphs(out.ctypes.data_as(C.c_void_p)) == 0
    return out.reshape(95, 7)


def frames_of(H, W, seed=3):
    return np.random.default_rng(seed).integers(0, 256, (O.B, H, W, 3), dtype=np.uint8)


def one_face_text(lib, glyphs, name, score, track_id=-1, flags=0, idx=0, scale=1):
    """the text fid_draw_faces_host draws for one face, read back from the image: the cell columns compared with every glyph"""
    H, W = 24, 6 * scale * 60
    det = np.array([[[0, 18, 5, 22, 0.9]]], np.float32)
    style = O.Style(thickness=1, text_scale=scale, bar=0, flags=flags)
    track = np.array([[[track_id, 0]]], np.int32)
    rc, img = host_draw(lib, np.zeros((1, H, W, 3), np.uint8), 1, det, np.array([1], np.int32), idx=np.array([idx], np.int32),
                        score=np.array([score], np.float32), id_stride=1, track=track, names=[name], bgr=[(9, 9, 9)], style=style)
    assert rc == 0
    lit = img[0, 8 - 7 * scale + 1:9, :, 0] != 0                         # the text rows: y1 - 10 = 8 is the bottom row
    text = ""
    for k in range(W // (6 * scale)):
        cell = lit[::scale, 6 * scale * k:6 * scale * (k + 1):scale]
        rows = [sum(int(cell[r, c]) << (4 - c) for c in range(5)) for r in range(7)]
        hit = [g for g in range(95) if glyphs[g].tolist() == rows]
        assert len(hit) == 1 and not cell[:, 5].any()
        text += chr(0x20 + hit[0])
    return text.rstrip(" ")


# ---- formatting -----------------------------------------------------------------------------------------------

def test_two_decimals_equal_python_formatting():
    rng = np.random.default_rng(11)
    v = np.concatenate([(rng.random(1_000_000) * 1.2).astype(np.float32), np.arange(0, 10, dtype=np.float32) / 8,
                        np.arange(0, 160, dtype=np.float32) / 128])
    cents = O.cents_of(v)
    want = np.array([int(f"{x:.2f}".replace(".", "")) for x in v], np.int64)
    assert np.array_equal(cents, want), np.flatnonzero(cents != want)[:8]
    for x in v[-170::7]:
        assert O.two_decimals(x) == f"{np.float32(x):.2f}"
    assert [O.two_decimals(x) for x in (np.nan, -0.3, -np.inf, np.inf)] == ["0.00"] * 4
    assert O.two_decimals(0.125) == "0.12" and O.two_decimals(0.375) == "0.38" and O.two_decimals(123.0) == "9.99"


def test_library_formats_like_the_oracle(lib, glyphs):
    for s in (0.125, 0.375, 0.999, 1.0000001, 0.005, 0.015, np.nan, -0.3, -np.inf, 57.0):
        assert one_face_text(lib, glyphs, b"a", s) == "a: " + O.two_decimals(s), s


def test_corner_length_is_the_double_product():
    for m in range(5000):
        assert O.corner_length(m) == int(0.2 * m)
    assert O.corner_length(100, 0.29) == 28 and int(np.float32(0.29) * np.float32(100)) == 29      # an fp32 product is another number


def test_corner_length_in_the_library(lib):
    """w = h = m: the outline hides an arm of thickness 1, so thickness 3 and the row y1 - 1, where the top-left arm covers x1 - 1 .. x1 + L + 1"""
    for m, prop in ((10, 0.2), (14, 0.2), (15, 0.2), (35, 0.2), (70, 0.2), (115, 0.2), (4995, 0.2), (4999, 0.2), (100, 0.29), (50, 0.0)):
        L = int(prop * m)
        det = np.array([[[2, 2, 2 + m, 2 + m, 1]]], np.float32)
        rc, img = host_draw(lib, np.zeros((1, 6, m + 8, 3), np.uint8), 1, det, np.array([1], np.int32), style=O.Style(text_scale=0, proportion=prop))
        assert rc == 0
        row = np.flatnonzero(img[0, 1, :m // 2 + 3, 0])
        assert row.tolist() == list(range(1, 2 + L + 2)), (m, row)


def test_label_strings(lib, glyphs):
    long_name = O.NAMES[1]
    assert len(long_name) == 40
    assert O.label_text(True, b"ann", 0.5) == "ann: 0.50"
    assert O.label_text(True, b"ann", 0.5, 7, O.TRACK_ID) == "#7 ann: 0.50" and O.label_text(True, b"ann", 0.5, 7, 0) == "ann: 0.50"
    assert O.label_text(False, None, 0.5, 7, O.TRACK_ID) == "#7" and O.label_text(False, None, 0.5, -1, O.TRACK_ID) == ""
    assert O.label_text(True, long_name, 1.0) == long_name[:32].decode() + ": 1.00"
    assert O.label_text(True, "Zoë", 0.25) == "Zo??: 0.25"
    for name, score, tid, flags, idx in ((b"ann", 0.5, -1, 0, 0), (b"ann", 0.5, 7, O.TRACK_ID, 0), (b"ann", 0.5, 7, 0, 0), (b"ann", 0.5, 0, O.TRACK_ID, 0),
                                         (b"ann", 0.5, 1234567, O.TRACK_ID, -1), (b"ann", 0.5, -1, O.TRACK_ID, -1), (b"ann", 0.5, 5, O.TRACK_ID, 1),
                                         (long_name, 1.0, 2147483647, O.TRACK_ID, 0), ("Zoë".encode(), 0.25, -1, 0, 0), (b"a\x7f\x1f~ ", 0.3, -1, 0, 0)):
        assert one_face_text(lib, glyphs, name, score, tid, flags, idx) == O.label_text(idx == 0, name, score, tid, flags), (name, tid, flags, idx)


# ---- font -----------------------------------------------------------------------------------------------------

def test_font_table(glyphs):
    assert not glyphs[0].any()                                             # space
    assert len({bytes(g) for g in glyphs}) == 95
    assert not (glyphs & 0xE0).any()
    pixels = [sum(bin(int(r)).count("1") for r in g) for g in glyphs]
    for ch in "0123456789.:#?" + "".join(chr(c) for c in range(ord("a"), ord("z") + 1)) + "".join(chr(c) for c in range(ord("A"), ord("Z") + 1)):
        assert pixels[ord(ch) - 0x20] >= 5, ch


# ---- the host rasteriser against the oracle -------------------------------------------------------------------

@pytest.mark.parametrize("H, W", [(48, 80), (37, 67)])
def test_host_rasteriser_equals_the_oracle(lib, glyphs, H, W):
    frames = frames_of(H, W)
    images = {}
    for name, kw in O.cases(H, W):
        rc, got = host_draw(lib, frames, O.CAP, **kw)
        assert rc == 0, (name, lib.fid_last_error())
        want = O.draw(frames, cap=O.CAP, glyphs=glyphs, **kw)
        assert np.array_equal(got, want), (name, np.argwhere(got != want)[:6])
        images[name] = want
    assert (images["slots"] != frames).any()
    assert (images["slots"][0] != images["slots, the two overlapping faces swapped"][0]).any()          # the later face shows
    assert np.array_equal(images["an empty frame between two drawn ones"][1], frames[1])
    assert np.array_equal(images["counts 0, -2, cap + 3"][:2], frames[:2]) and (images["counts 0, -2, cap + 3"][2] != frames[2]).any()
    assert np.array_equal(images["rows cut inside frame 1"][2], frames[2])
    assert (images["track ids"] != images["track ids given, flag off"]).any()


def test_one_face_per_rule(lib, glyphs):
    """each degenerate box alone: what draws nothing leaves the frame as it was"""
    frames = frames_of(40, 72, seed=5)[:1]
    for box, draws in (((10.2, 20, 11.9, 34), True), ((20, 30, 40, 31.5), True), ((30.1, 20, 30.9, 34), False), ((np.nan, 5, 20, 20), False),
                       ((5, 5, 3e7, 20), False), ((5, 5, np.inf, 20), False), ((20, 20, 10, 30), False), ((-9.5, -9.5, -0.5, -0.5), True),
                       ((-9.5, -9.5, -2.5, -2.5), False),
                       ((-0.9, -0.9, 5, 5), True), ((8388607, 0, 8388609, 5), False)):
        det = np.array([[list(box) + [1]]], np.float32)
        rc, got = host_draw(lib, frames, 1, det, np.array([1], np.int32), style=O.Style(text_scale=0))
        want = O.draw(frames, det, np.array([1]), 1, glyphs, style=O.Style(text_scale=0))
        assert rc == 0 and np.array_equal(got, want) and (got != frames).any() == draws, box


# ---- refusals --------------------------------------------------------------------------------------------------

def test_refusals_leave_the_image_untouched(lib):
    H, W = 20, 30
    frames = frames_of(H, W)
    det = O.scene(H, W)
    good = dict(det=det, counts=np.full(O.B, 3, np.int32), idx=np.zeros((O.B, O.CAP), np.int32), score=np.ones((O.B, O.CAP), np.float32),
                id_stride=O.CAP, names=O.NAMES, style=O.Style())
    rc, img = host_draw(lib, frames, O.CAP, **good)
    assert rc == 0 and (img != frames).any()
    S = O.Style
    bad = [dict(style=S(thickness=2)), dict(style=S(thickness=0)), dict(style=S(thickness=17)), dict(style=S(thickness=-1)),
           dict(style=S(text_scale=-1)), dict(style=S(text_scale=5)), dict(style=S(proportion=np.nan)), dict(style=S(proportion=-0.01)),
           dict(style=S(proportion=1.01)), dict(score=None), dict(id_stride=0), dict(id_stride=-3), dict(n_rows=-1), dict(det=None),
           dict(counts=None)]
    for kw in bad:
        rc, img = host_draw(lib, frames, O.CAP, **dict(good, **kw))
        assert rc == -1 and len(lib.fid_last_error()) > 0 and np.array_equal(img, frames), kw
    rc, img = host_draw(lib, frames, 0, **good)
    assert rc == -1 and np.array_equal(img, frames)
    # sizes and NULL pointers that host_draw cannot express
    img = frames.copy()
    st = c_style(O.Style())
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    counts = good["counts"]

    def call(frames_p=p(img), Bn=O.B, h=H, w=W, cap=O.CAP, style=C.byref(st)):
        return lib.fid_draw_faces_host(frames_p, Bn, h, w, p(det), p(counts), cap, None, None, 0, None, 0, None, None, None, None, 0, style)

    for kw in (dict(frames_p=None), dict(style=None), dict(Bn=0), dict(Bn=-1), dict(h=0), dict(w=0), dict(w=-5), dict(cap=-1),
               dict(h=1 << 15, w=1 << 15), dict(h=(1 << 31) - 1, w=(1 << 31) - 1), dict(Bn=1 << 20, cap=1 << 12)):
        assert call(**kw) == -1, kw
    assert np.array_equal(img, frames)
    assert call() == 0 and (img != frames).any()
    assert lib.fid_draw_glyphs(None) == -1


# ---- the shims -------------------------------------------------------------------------------------------------

def test_helpers_draw_without_opencv(lib, glyphs, monkeypatch):
    monkeypatch.setitem(sys.modules, "cv2", None)                          # `import cv2` raises ImportError, as on a host without OpenCV
    from utils import helpers
    rng = np.random.default_rng(8)
    image = rng.integers(0, 256, (60, 90, 3), dtype=np.uint8)
    bbox = np.array([12.7, 25.2, 50.9, 55.5], np.float32)
    det = np.concatenate([bbox, [1.0]]).astype(np.float32).reshape(1, 1, 5)
    one = np.array([1], np.int32)
    # draw_bbox: one unknown face in the given colour, no text, no bar
    got = image.copy()
    assert helpers.draw_bbox(got, bbox, color=(0, 200, 50), thickness=5, proportion=0.3) is got
    want = O.draw(image[None], det, one, 1, glyphs, style=O.Style(proportion=0.3, thickness=5, text_scale=0, bar=0, unknown_bgr=(0, 200, 50)))[0]
    assert np.array_equal(got, want) and (got != image).any()
    got = image.copy()
    helpers.draw_bbox(got, bbox)
    want = O.draw(image[None], det, one, 1, glyphs, style=O.Style(text_scale=0, bar=0, unknown_bgr=(0, 255, 0)))[0]
    assert np.array_equal(got, want)
    # draw_bbox_info: name, similarity and bar
    got = image.copy()
    assert helpers.draw_bbox_info(got, bbox, np.float32(0.625), "ann", (10, 20, 250)) is got
    want = O.draw(image[None], det, one, 1, glyphs, idx=np.array([0]), score=np.array([0.625], np.float32), id_stride=1, names=[b"ann"],
                  bgr=[(10, 20, 250)], style=O.Style())[0]
    assert np.array_equal(got, want)
    # draw_faces: one results() list
    faces = [(np.array([5, 20, 30, 50], np.float32), 0.9, np.zeros((5, 2), np.float32), "ann", 0.5),
             (np.array([20, 24, 70, 58], np.float32), 0.8, np.zeros((5, 2), np.float32), "Unknown", 0.0),
             (np.array([40, 18, 80, 40], np.float32), 0.7, np.zeros((5, 2), np.float32), "bob", 0.75)]
    got = image.copy()
    assert helpers.draw_faces(got, faces, colors={"ann": (1, 2, 3), "bob": (200, 100, 0)}) is got
    det3 = np.zeros((1, 3, 5), np.float32)
    det3[0, :, :4] = [f[0] for f in faces]
    want = O.draw(image[None], det3, np.array([3]), 3, glyphs, idx=np.array([0, -1, 1]), score=np.array([0.5, 0.0, 0.75], np.float32), id_stride=3,
                  names=[b"ann", b"bob"], bgr=[(1, 2, 3), (200, 100, 0)], style=O.Style())[0]
    assert np.array_equal(got, want)
