"""CPU: the way out as NV12 -- the forward colour tables, fid_bgr_to_nv12_host and fid_draw_faces_nv12_host (helpers.bgr_to_nv12 /
draw_faces_nv12) against tests/draw_nv12_oracle.py, byte for byte over whole allocations; the round trip through the existing inverse; and
csrc/yuv_core.h + csrc/draw_nv12_core.h under AddressSanitizer + UBSan in a stand-alone program (tests/draw_nv12_host_driver.cpp; nothing is
preloaded and nothing is loaded into Python)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import draw_nv12_oracle as N
import draw_oracle as O
import nv12_oracle
from draw_nv12_calls import GUARD, STANDARDS, background, desc_of, host_draw, layouts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("clang++")


@pytest.fixture(scope="module")
def lib():
    from scrfd_arcface_facerecognition_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def glyphs(lib):
    out = np.zeros(95 * 7, np.uint8)
    assert lib.fid_draw_glyphs(out.ctypes.data_as(C.c_void_p)) == 0
    return out.reshape(95, 7)


# ---- the tables ----
def test_tables_equal_the_header():
    """the integers the formula gives from (kr, kb) are the ones written out in include/faceid.h; every chroma row sums to 0"""
    head = N.header_tables(os.path.join(ROOT, "include", "faceid.h"))
    issue = {"bt601": (102662, 528618, 269262, 460551, -305128, -155423, -74897, -385654, 460551, 16),
             "bt709": (65019, 644067, 191455, 460551, -355018, -105533, -42230, -418321, 460551, 16),
             "bt601_full": (119538, 615514, 313524, 524288, -347356, -176932, -85262, -439026, 524288, 0)}
    for std in STANDARDS:
        t = N.table(std)
        assert t == head[std] == issue[std], std
        assert sum(t[3:6]) == 0 and sum(t[6:9]) == 0
        grey = np.arange(256)[:, None].repeat(3, axis=1)
        assert (N.chroma(4 * grey, std) == 128).all()                      # every grey maps to U = V = 128 exactly
        # the int32 range of the chroma sum: one positive coefficient against 1020, or the two negative ones
        worst = max(1020 * max(abs(t[3]), abs(t[4] + t[5]), abs(t[8]), abs(t[6] + t[7])) + (128 << 22) + (1 << 21), 0)
        assert worst < 1.08e9


# ---- the conversion ----
@pytest.mark.parametrize("standard", STANDARDS)
@pytest.mark.parametrize("H, W", [(16, 18), (32, 64)])
def test_bgr_to_nv12_host_equals_the_oracle(lib, standard, H, W):
    frames = np.random.default_rng(H + W).integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    for name, lay in layouts(H, W).items():
        n = nv12_oracle.needed_bytes(2, H, W, **lay)
        got = np.full(n, GUARD, np.uint8)
        rc = lib.fid_bgr_to_nv12_host(frames.ctypes.data_as(C.c_void_p), 2, H, W, got.ctypes.data_as(C.c_void_p), C.byref(desc_of(H, W, lay, standard)))
        want = N.bgr_to_nv12(frames, np.full(n, GUARD, np.uint8), standard, **lay)
        assert rc == 0 and np.array_equal(got, want), (name, np.argwhere(got != want)[:6])
        owned = np.zeros(n, np.uint8)                                      # every byte outside the rows' first W bytes keeps its fill
        for b in range(2):
            for plane in N.planes(owned, b, H, W, **lay):
                plane[...] = 1
        assert (got[owned == 0] == GUARD).all() and int(owned.sum()) == 2 * H * W * 3 // 2


def test_helper_bgr_to_nv12_is_the_twin_of_nv12_to_bgr():
    from utils.helpers import bgr_to_nv12, nv12_to_bgr
    frames = np.random.default_rng(1).integers(0, 256, (2, 12, 20, 3), dtype=np.uint8)
    dense = bgr_to_nv12(frames, "bt709")
    assert dense.shape == (2, 18, 20) and np.array_equal(dense.reshape(-1), N.bgr_to_nv12(frames, np.zeros(2 * 18 * 20, np.uint8), "bt709"))
    assert np.array_equal(bgr_to_nv12(frames[1], "bt709"), dense[1])
    lay = layouts(12, 20)["w+6"]
    flat = bgr_to_nv12(frames, pitch=lay["pitch"], uv_offset=lay["uv_offset"], frame_stride=lay["frame_stride"])
    assert flat.size == 2 * lay["frame_stride"] and np.array_equal(flat, N.bgr_to_nv12(frames, np.zeros(flat.size, np.uint8), **lay))
    assert nv12_to_bgr(dense, 12, 20, "bt709").shape == (2, 12, 20, 3)
    with pytest.raises(RuntimeError):
        bgr_to_nv12(frames[:, :11])                                        # odd H


@pytest.mark.parametrize("standard, bound", [("bt601", 2), ("bt709", 2), ("bt601_full", 2)])
def test_round_trip_through_the_inverse(standard, bound):
    """flat 2 x 2 blocks of 64 K random colours and the eight cube corners: nv12_to_bgr(bgr_to_nv12(x)) is within 2 levels of x per channel
    (over all 2^24 colours the maxima are 2, 2 and 1).  The inverse is tests/nv12_oracle.py's -- a yardstick of its own, so a swapped
    U / V or a wrong row cannot cancel out."""
    rng = np.random.default_rng(9)
    corners = np.array([[b, g, r] for b in (0, 255) for g in (0, 255) for r in (0, 255)], np.uint8)
    colours = np.concatenate([corners, rng.integers(0, 256, (65536, 3), dtype=np.uint8)])
    Y = N.luma(colours, standard)
    uv = N.chroma(4 * colours.astype(np.int64), standard)
    back = nv12_oracle.yuv_to_bgr(Y, uv[:, 0], uv[:, 1], standard)
    err = np.abs(back.astype(np.int64) - colours.astype(np.int64))
    print(f"\n{standard}: max round-trip error {err.max()} per channel {err.max(axis=0).tolist()}")
    assert err.max() <= bound
    # ... and through the library's own two host calls, as frames of flat blocks
    from utils.helpers import bgr_to_nv12, nv12_to_bgr
    side = 2 * 64
    blocks = colours[:64 * 64].reshape(64, 64, 3).repeat(2, axis=0).repeat(2, axis=1)
    assert blocks.shape == (side, side, 3)
    back = nv12_to_bgr(bgr_to_nv12(blocks, standard), side, side, standard)
    assert np.abs(back.astype(np.int64) - blocks.astype(np.int64)).max() <= bound


# ---- the overlay ----
@pytest.mark.parametrize("standard", STANDARDS)
@pytest.mark.parametrize("H, W", [(48, 80), (38, 68)])
def test_host_draw_equals_the_oracle(lib, glyphs, standard, H, W):
    for lname, lay in layouts(H, W).items():
        buf = background(H, O.B, H, W, lay)
        for name, kw in O.cases(H, W):
            rc, got = host_draw(lib, buf, O.B, H, W, lay, standard, O.CAP, **kw)
            want = N.draw_nv12(buf, O.B, H, W, cap=O.CAP, glyphs=glyphs, standard=standard, **kw, **lay)
            assert rc == 0 and np.array_equal(got, want), (lname, name, np.argwhere(got != want)[:6])
            if name == "slots":
                assert (got != buf).any()


def test_helper_draw_faces_nv12(glyphs):
    from utils.helpers import bgr_to_nv12, draw_faces_nv12
    H, W = 48, 80
    frame = bgr_to_nv12(np.random.default_rng(2).integers(0, 256, (H, W, 3), dtype=np.uint8))
    faces = [(np.array([10, 20, 40, 44], np.float32), 0.9, None, "ann", 0.5), (np.array([25, 22, 60, 46], np.float32), 0.8, None, "Unknown", 0.0)]
    got = draw_faces_nv12(frame.copy(), H, W, faces, colors={"ann": (10, 200, 30)})
    det = np.zeros((1, 2, 5), np.float32)
    det[0, :, :4] = [f[0] for f in faces]
    want = N.draw_nv12(frame.reshape(-1), 1, H, W, det, np.array([2]), 2, glyphs, idx=np.array([0, -1]), score=np.array([0.5, 0.0], np.float32),
                       id_stride=2, names=[b"ann"], bgr=[(10, 200, 30)])
    assert got.shape == (H * 3 // 2, W) and np.array_equal(got.reshape(-1), want) and (got != frame).any()
    with pytest.raises(ValueError):
        draw_faces_nv12(frame[:-1], H, W, faces)


def test_host_calls_refuse(lib):
    from scrfd_arcface_facerecognition_amd._lib import nv12_desc
    H, W = 20, 32
    buf = np.full(H * W * 3 // 2, GUARD, np.uint8)
    bgr = np.zeros((1, H, W, 3), np.uint8)
    det, counts = np.zeros((1, 2, 5), np.float32), np.array([2], np.int32)
    det[0, :, :4] = (3, 3, 15, 15)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    st = O.Style()
    from draw_calls import c_style
    bad = [nv12_desc(H, W, pitch=W - 2, uv_offset=W * H, frame_stride=W * H * 3 // 2), nv12_desc(H, W, pitch=W, uv_offset=W * H - 1, frame_stride=W * H * 3),
           nv12_desc(H, W, pitch=W, uv_offset=W * H, frame_stride=W * H * 3 // 2 - 1), nv12_desc(H, W, standard=3)]
    good = nv12_desc(H, W)
    for d in bad:
        assert lib.fid_draw_faces_nv12_host(p(buf), C.byref(d), 1, H, W, p(det), p(counts), 2, None, None, 0, None, 0, None, None, None, None, 0,
                                            C.byref(c_style(st))) == -1 and lib.fid_last_error()
        assert lib.fid_bgr_to_nv12_host(p(bgr), 1, H, W, p(buf), C.byref(d)) == -1
    assert lib.fid_draw_faces_nv12_host(p(buf), C.byref(good), 1, H - 1, W, p(det), p(counts), 2, None, None, 0, None, 0, None, None, None, None, 0,
                                        C.byref(c_style(st))) == -1
    assert lib.fid_draw_faces_nv12_host(p(buf), None, 1, H, W, p(det), p(counts), 2, None, None, 0, None, 0, None, None, None, None, 0,
                                        C.byref(c_style(st))) == -1
    assert lib.fid_draw_faces_nv12_host(p(buf), C.byref(good), 1, H, W, p(det), p(counts), 2, None, None, 0, None, 0, None, None, None, None, 0,
                                        C.byref(c_style(O.Style(thickness=2)))) == -1
    assert lib.fid_bgr_to_nv12_host(None, 1, H, W, p(buf), C.byref(good)) == -1 and lib.fid_bgr_to_nv12_host(p(bgr), 1, H, W, None, C.byref(good)) == -1
    assert lib.fid_bgr_to_nv12_host(p(bgr), 1, H, W + 1, p(buf), C.byref(good)) == -1
    assert (buf == GUARD).all()


# ---- the headers under the sanitizers ----
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if CXX is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("draw_nv12_driver") / "draw_nv12_host_driver"
    cmd = [CXX, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "scrfd_arcface_facerecognition_amd", "csrc"), os.path.join(ROOT, "tests", "draw_nv12_host_driver.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True)
    return str(exe)


def run_case(driver, tmp_path, H, W, lay, standard, buf, bgr, det, counts, idx, score, names, style):
    Bn, cap = det.shape[:2]
    offsets = np.zeros(len(names) + 1, np.int32)
    offsets[1:] = np.cumsum([len(n) for n in names])
    src, dst = tmp_path / "case.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.array([Bn, H, W, cap, len(names), style.thickness, style.text_scale, style.bar, lay["pitch"], nv12_oracle.STANDARD_ID[standard]],
                         np.int32).tobytes())
        f.write(np.array([lay["uv_offset"], lay["frame_stride"], buf.size], np.int64).tobytes())
        f.write(np.array([style.proportion], np.float64).tobytes())
        for a, dt in ((det, np.float32), (counts, np.int32), (idx, np.int32), (score, np.float32), (offsets, np.int32)):
            f.write(np.ascontiguousarray(a, dt).tobytes())
        f.write(b"".join(names))
        f.write(buf.tobytes())
        f.write(np.ascontiguousarray(bgr, np.uint8).tobytes())
    p = subprocess.run([driver, str(src), str(dst)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    out = np.fromfile(dst, np.uint8)
    return out[:buf.size], out[buf.size:], int(p.stdout)


@pytest.mark.parametrize("H, W", [(48, 80), (38, 68)])
def test_headers_under_the_sanitizers(driver, tmp_path, glyphs, H, W):
    """the pitched layout (pitch = W + 6, a gap, a tail) in an allocation that ends with the last UV byte of the last frame: one byte further
    is a heap overflow"""
    lay = layouts(H, W)["w+6"]
    buf = background(3, O.B, H, W, lay, exact=True)
    assert buf.size == (O.B - 1) * lay["frame_stride"] + lay["uv_offset"] + lay["pitch"] * (H // 2 - 1) + W
    bgr = np.random.default_rng(4).integers(0, 256, (O.B, H, W, 3), dtype=np.uint8)
    ran = 0
    for std in STANDARDS:
        for name, kw in O.cases(H, W):
            if kw["idx"] is None or kw["offsets"] is not None or kw["id_stride"] != O.CAP or kw["track"] is not None or kw["bgr"] is not None \
                    or kw["names"] is None or kw["style"].unknown_bgr != (255, 0, 0):
                continue                                                   # (the driver speaks the slot form with default colours)
            drawn, conv, lit = run_case(driver, tmp_path, H, W, lay, std, buf, bgr, kw["det"], kw["counts"], kw["idx"], kw["score"], kw["names"], kw["style"])
            want = N.draw_nv12(buf, O.B, H, W, cap=O.CAP, glyphs=glyphs, standard=std, **kw, **lay)
            assert np.array_equal(drawn, want), (std, name, np.argwhere(drawn != want)[:6])
            assert np.array_equal(conv, N.bgr_to_nv12(bgr, np.full(buf.size, GUARD, np.uint8), std, **lay)), (std, name)
            ran += 1
    assert ran >= 15
    # boxes whose geometry reaches the limits of int: nothing may overflow, nothing may be written outside
    big = 8388607.0
    det = np.zeros((1, 6, 5), np.float32)
    det[0, :, :4] = [(-big, -big, big, big), (-big, 3, 5, big), (big - 1, big - 1, big, big), (0, 0, big, 1), (-big, -big, -big + 1, -big + 1), (2, 2, 9, 9)]
    idx, score = np.zeros((1, 6), np.int32), np.full((1, 6), 3.0e38, np.float32)
    style = O.Style(thickness=15, text_scale=4, proportion=1.0)
    one = background(5, 1, H, W, lay, exact=True)
    drawn, _, lit = run_case(driver, tmp_path, H, W, lay, "bt601", one, bgr[:1], det, np.array([6], np.int32), idx, score, [b"x" * 40], style)
    want = N.draw_nv12(one, 1, H, W, det, np.array([6]), 6, glyphs, idx=idx, score=score, id_stride=6, names=[b"x" * 40], style=style, **lay)
    assert np.array_equal(drawn, want) and lit > 0
