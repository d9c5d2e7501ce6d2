"""CPU: fid_redact_faces_host and fid_redact_faces_nv12_host against tests/redact_oracle.py, byte for byte over whole allocations; the cases
the list must hold, each shown not to be vacuous; the per-face cell bound over an enumeration of boxes; idempotence; and every refused call
leaving the frames as they were."""
import ctypes as C

import numpy as np
import pytest

import redact_oracle as R
from draw_nv12_calls import GUARD, STANDARDS, background, layouts
from redact_calls import host_redact, host_redact_nv12, invalid_calls

INVALID = -1
BGR_SHAPES = [(48, 80), (37, 67)]
NV12_SHAPES = [(48, 80), (38, 68)]


@pytest.fixture(scope="module")
def lib():
    from scrfd_arcface_facerecognition_amd import _lib
    return _lib.load()


def frames_for(H, W):
    return np.random.default_rng(100 * H + W).integers(0, 256, (R.B, H, W, 3), dtype=np.uint8)


def idempotent_frames(H, W, kw, first, second, name, frame_of=lambda a, b: a[b]):
    """Idempotence: a second application changes nothing -- a cell of constant v has mean v -- in every frame whose selected regions do not
    overlap, and under FILL always.  (Where two regions overlap, a cell of the lower face is part its own mean and part the upper face's
    values after the first application, and its mean moves: the definition's, not the code's -- the oracle does the same, asserted by the
    callers.)  -> the number of frames with two or more redacted faces that were checked"""
    regions = {}
    for b, f, g in R.selected_faces(R.B, cap=R.CAP, **kw):
        if R.clipped(g, H, W) is not None:
            regions.setdefault(b, []).append(R.clipped(g, H, W))
    checked = 0
    for b in range(R.B):
        if kw["style"].mode == R.FILL or R.disjoint(regions.get(b, [])):
            assert np.array_equal(frame_of(second, b), frame_of(first, b)), (name, b)
            checked += len(regions.get(b, [])) >= 2
    return checked


@pytest.mark.parametrize("H, W", BGR_SHAPES)
def test_host_twin_equals_the_oracle_bgr(lib, H, W):
    frames = frames_for(H, W)
    changed = idem = 0
    for name, kw in R.cases(H, W):
        rc, got = host_redact(lib, frames, R.CAP, **kw)
        want = R.redact(frames, cap=R.CAP, **kw)
        assert rc == 0 and np.array_equal(got, want), (name, np.argwhere(got != want)[:6])
        changed += int((got != frames).any())
        rc2, again = host_redact(lib, got, R.CAP, **kw)
        assert rc2 == 0 and np.array_equal(again, R.redact(got, cap=R.CAP, **kw)), name
        idem += idempotent_frames(H, W, kw, got, again, name)
    assert changed >= len(R.cases(H, W)) - 1                               # ("detections only, who 2" selects nobody)
    assert idem >= 10


@pytest.mark.parametrize("standard", STANDARDS)
@pytest.mark.parametrize("H, W", NV12_SHAPES)
def test_host_twin_equals_the_oracle_nv12(lib, standard, H, W):
    for lname, lay in layouts(H, W).items():
        buf = background(H + W, R.B, H, W, lay, exact=True)
        idem = 0
        for name, kw in R.cases(H, W):
            rc, got = host_redact_nv12(lib, buf, R.B, H, W, lay, standard, R.CAP, **kw)
            want = R.redact_nv12(buf, R.B, H, W, cap=R.CAP, standard=standard, **lay, **kw)
            assert rc == 0 and np.array_equal(got, want), (lname, name, np.argwhere(got != want)[:6])
            rc2, again = host_redact_nv12(lib, got, R.B, H, W, lay, standard, R.CAP, **kw)
            assert rc2 == 0 and np.array_equal(again, R.redact_nv12(got, R.B, H, W, cap=R.CAP, standard=standard, **lay, **kw)), (lname, name)
            stride = lay["frame_stride"]
            idem += idempotent_frames(H, W, kw, got, again, name, lambda a, b: a[b * stride:(b + 1) * stride])
        assert idem >= 10
        # padding is never written: GUARD bytes of the background are GUARD bytes of every result (compared above over the whole allocation),
        # and they exist in the padded layouts
        if lname != "dense":
            owned = np.zeros(buf.size, bool)
            for b in range(R.B):
                for plane in R.N.planes(owned, b, H, W, **lay):
                    plane[...] = True
            assert (~owned).sum() > 0 and (buf[~owned] == GUARD).all()


def case(H, W, name):
    return dict(R.cases(H, W))[name]


def faces_of(H, W, name):
    kw = case(H, W, name)
    return {(b, f): g for b, f, g in R.selected_faces(R.B, cap=R.CAP, **kw)}, kw


@pytest.mark.parametrize("H, W", BGR_SHAPES + NV12_SHAPES[1:])
def test_the_case_list_is_not_vacuous(H, W):
    frames = frames_for(H, W)
    names = [n for n, _ in R.cases(H, W)]
    assert len(set(names)) == len(names)
    # two overlapping selected regions: the snapshot rule and one-face-after-another give different bytes
    faces, kw = faces_of(H, W, "slots, who 3")
    a, b = R.clipped(faces[(0, 0)], H, W), R.clipped(faces[(0, 1)], H, W)
    assert max(a[0], b[0]) <= min(a[2], b[2]) and max(a[1], b[1]) <= min(a[3], b[3])
    stats = {}
    snap, seq = R.redact(frames, cap=R.CAP, stats=stats, **kw), R.redact(frames, cap=R.CAP, sequential=True, **kw)
    assert (snap[0] != seq[0]).any()
    # a cell whose sum is exactly half-way: truncation and round-half-up differ there
    assert stats["halfway"] > 0 and stats["cells"] > 100
    if H % 2 == 0 and W % 2 == 0:
        lay = layouts(H, W)["w+6"]
        st2 = {}
        R.redact_nv12(background(H + W, R.B, H, W, lay), R.B, H, W, cap=R.CAP, stats=st2, **lay, **kw)
        assert st2["halfway"] > 0
    # a box partly outside each of the four edges, one wholly outside
    left, right, top, bottom, outside = (faces[(1, f)] for f in range(5))
    assert left["rx0"] < 0 <= left["rx1"] and right["rx0"] <= W - 1 < right["rx1"] and top["ry0"] < 0 <= top["ry1"]
    assert bottom["ry0"] <= H - 1 < bottom["ry1"] and R.clipped(outside, H, W) is None
    # a negative odd x1 - mx: the floor to even is one below the truncation
    mx = int(kw["style"].expand * left["w"])
    assert left["x1"] - mx < 0 and (left["x1"] - mx) % 2 == 1 and left["rx0"] == left["x1"] - mx - 1
    # w = h = 1
    one = faces[(0, 5)]
    assert one["w"] == 1 and one["h"] == 1 and one["c"] == 2
    # a NaN box and a 2^23 box are skipped; h = 1 is not, w = 0 is
    assert (0, 3) not in faces and (2, 7) not in faces and (2, 6) not in faces and (2, 5) in faces
    assert kw["det"][0, 3, 0] == 2.0 ** 23 and np.isnan(kw["det"][2, 7, 0])
    # one box covering the frame with cells = 1: one cell per frame-sized region
    faces1, kw1 = faces_of(H, W, "one box covers the frame, cells 1")
    g = faces1[(2, 0)]
    rects = list(R.cell_rects(g, H, W))
    assert R.clipped(g, H, W) == (0, 0, W - 1, H - 1) and len([k for k in faces1 if k[0] == 2]) == 1
    # (c = the box's side rounded up to even: an even frame is one cell; in an odd one the box is a pixel short of the frame's last column)
    assert len(rects) == (1 if W % 2 == 0 and H % 2 == 0 else 2) and rects[0][:2] == (0, 0) and rects[0][2] >= W - 2 and rects[0][3] == H - 1
    # cells = 16 on a 20-pixel face
    faces16, _ = faces_of(H, W, "cells 16, expand 0.5")
    assert max(faces16[(0, 6)]["w"], faces16[(0, 6)]["h"]) == 20 and faces16[(0, 6)]["c"] == 2
    # counts > cap; an empty frame between two redacted ones
    assert case(H, W, "counts 0, -2, cap + 3")["counts"][2] > R.CAP
    e = R.redact(frames, cap=R.CAP, **case(H, W, "an empty frame between two redacted ones"))
    assert (e[0] != frames[0]).any() and np.array_equal(e[1], frames[1]) and (e[2] != frames[2]).any()
    # who = 1, 2, 3 under each of the three identity forms: the selections differ as the classes say
    for form in ("detections only", "slots", "rows"):
        sel = {who: set(faces_of(H, W, f"{form}, who {who}")[0]) for who in (1, 2, 3)}
        assert sel[1] | sel[2] == sel[3] and not (sel[1] & sel[2]) and sel[3]
        assert (not sel[2]) == (form == "detections only") and sel[1]
    assert set(faces_of(H, W, "slots, who 3")[0]) != set(faces_of(H, W, "rows, who 3")[0])
    # FILL with a colour that is not grey: its chroma is not 128 under any standard
    fill = case(H, W, "fill, a colour that is not grey")["style"]
    assert fill.mode == R.FILL and len(set(fill.fill_bgr)) == 3
    for std in STANDARDS:
        _, u, v = R.N.colour_yuv(fill.fill_bgr, std)
        assert u != 128 and v != 128
    assert len({R.N.colour_yuv(fill.fill_bgr, std) for std in STANDARDS}) == 3


def test_cell_bound_holds_over_an_enumeration(lib):
    """the most cells one face can have, from (cells, expand) alone: (floor(1.5 * (1 + 2 * expand) * cells) + 3)^2 (csrc/redact_core.h), against
    the oracle's count for every w, h in 1 .. 200, at an even and at an odd corner (the alignment can add a cell on either side)"""
    w = np.arange(1, 201, dtype=np.int64)
    for cells in range(1, 17):
        for expand in (0.0, 0.1, 0.25, 0.5):
            per_axis = int(1.5 * (1.0 + 2.0 * expand) * cells) + 3
            m = (expand * w.astype(np.float64)).astype(np.int64)
            s = np.maximum(w[:, None], w[None, :])
            q = s // cells
            c = np.maximum(2, q + (q & 1))
            worst = 0
            for x1 in (10, 11, -11):
                r0 = ((x1 - m) // 2) * 2
                r1 = (x1 + w + m) | 1
                n = -(-(r1 - r0 + 1)[:, None] // c)                        # cells along the axis of side w[i] when the other side is w[j]
                worst = max(worst, int(n.max()))
                assert (n * n.T).max() <= per_axis * per_axis
            assert worst <= per_axis, (cells, expand, worst, per_axis)
    # ... and the vectorised count is the oracle's own, on a sample
    for wv, hv, cells, expand in ((1, 1, 16, 0.5), (200, 3, 7, 0.25), (37, 111, 16, 0.5), (2, 199, 1, 0.1), (5, 5, 2, 0.5)):
        st = R.Style(cells=cells, expand=expand)
        g = R.geometry((1011, 1010, 1011 + wv, 1010 + hv), st)
        assert R.cells_per_face(g) <= (int(1.5 * (1.0 + 2.0 * expand) * cells) + 3) ** 2
        assert R.cells_per_face(g) == len(list(R.cell_rects(g, 4096, 4096)))
    st = R.Style()
    assert (int(1.5 * (1.0 + 2.0 * st.expand) * st.cells) + 3) ** 2 == 289


def test_every_refused_call_leaves_the_frames_untouched(lib):
    H, W = 48, 80
    frames = frames_for(H, W)
    base = case(H, W, "slots, who 3")
    lay = layouts(H, W)["w+6"]
    buf = background(7, R.B, H, W, lay, exact=True)
    for what, over, style in invalid_calls(base["style"]):
        kw = dict(base, **over, style=style)
        cap = kw.pop("cap", R.CAP)
        rc, got = host_redact(lib, frames, cap, **kw)
        assert rc == INVALID and np.array_equal(got, frames), what
        rc, got = host_redact_nv12(lib, buf, R.B, H, W, lay, "bt601", cap, **kw)
        assert rc == INVALID and np.array_equal(got, buf), what
    for what, bad in (("pitch below W", dict(lay, pitch=W - 2)), ("overlapping planes", dict(lay, uv_offset=lay["pitch"] * H - 1)),
                      ("overlapping frames", dict(lay, frame_stride=lay["uv_offset"]))):
        rc, got = host_redact_nv12(lib, buf, R.B, H, W, bad, "bt601", R.CAP, **base)
        assert rc == INVALID and np.array_equal(got, buf), what
    rc, got = host_redact_nv12(lib, buf, R.B, H, W, lay, 3, R.CAP, **base)                    # an unknown standard
    assert rc == INVALID and np.array_equal(got, buf)
    rc, got = host_redact_nv12(lib, buf, R.B, H - 1, W, lay, "bt601", R.CAP, **base)          # an odd H
    assert rc == INVALID and np.array_equal(got, buf)
    null = C.c_void_p(None)
    assert lib.fid_redact_faces_host(null, 1, 8, 8, null, null, 1, null, null, 0, null, 0, null) == INVALID


def test_helper_redact_faces_is_the_host_twin(lib):
    from utils.helpers import redact_faces
    from scrfd_arcface_facerecognition_amd._lib import RedactStyle
    H, W = 48, 80
    image = frames_for(H, W)[0]
    kw = case(H, W, "slots, who 3")
    faces = [tuple(row) for row in kw["det"][0]]
    known = [int(i) >= 0 for i in kw["idx"][0]]
    for who in (1, 2, 3):
        want = R.redact(image[None], kw["det"][:1], np.array([R.CAP]), R.CAP, idx=kw["idx"][:1], id_stride=R.CAP, style=R.Style(who=who))[0]
        got = redact_faces(image.copy(), faces, known, RedactStyle(who=who))
        assert np.array_equal(got, want)
    want = R.redact(image[None], kw["det"][:1], np.array([R.CAP]), R.CAP)[0]
    assert np.array_equal(redact_faces(image.copy(), faces), want)
