"""CPU: csrc/draw_core.h under AddressSanitizer + UBSan.  tests/draw_host_driver.cpp -- a stand-alone program that includes only that header --
rasterises the clipping cases of tests/draw_oracle.py into heap buffers of exactly H * W * 3 bytes; a pixel outside a frame, a read past an
input array or a signed overflow in the geometry ends the program.  Its frames are then compared with the oracle's, byte for byte.
Nothing is preloaded and nothing is loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import draw_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("clang++")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if CXX is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("draw_driver") / "draw_host_driver"
    cmd = [CXX, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "scrfd_arcface_facerecognition_amd", "csrc"), os.path.join(ROOT, "tests", "draw_host_driver.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True)
    return str(exe)


def run_case(driver, tmp_path, H, W, det, counts, idx, score, names, style):
    Bn, cap = det.shape[:2]
    offsets = np.zeros(len(names) + 1, np.int32)
    offsets[1:] = np.cumsum([len(n) for n in names])
    src, dst = tmp_path / "case.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.array([Bn, H, W, cap, len(names), style.thickness, style.text_scale, style.bar], np.int32).tobytes())
        f.write(np.array([style.proportion], np.float64).tobytes())
        for a, dt in ((det, np.float32), (counts, np.int32), (idx, np.int32), (score, np.float32), (offsets, np.int32)):
            f.write(np.ascontiguousarray(a, dt).tobytes())
        f.write(b"".join(names))
    p = subprocess.run([driver, str(src), str(dst)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    return np.fromfile(dst, np.uint8).reshape(Bn, H, W, 3), int(p.stdout)


@pytest.mark.parametrize("H, W", [(48, 80), (37, 67)])
def test_clipping_cases_under_the_sanitizers(driver, tmp_path, H, W):
    import ctypes as C
    from scrfd_arcface_facerecognition_amd import _lib
    glyphs = np.zeros(95 * 7, np.uint8)
    assert _lib.load().fid_draw_glyphs(glyphs.ctypes.data_as(C.c_void_p)) == 0
    glyphs = glyphs.reshape(95, 7)
    black = np.zeros((O.B, H, W, 3), np.uint8)
    ran = 0
    for name, kw in O.cases(H, W):
        if kw["idx"] is None or kw["offsets"] is not None or kw["id_stride"] != O.CAP or kw["track"] is not None or kw["bgr"] is not None \
                or kw["names"] is None or kw["style"].unknown_bgr != (255, 0, 0):
            continue                                                       # (the driver speaks the slot form with default colours)
        got, lit = run_case(driver, tmp_path, H, W, kw["det"], kw["counts"], kw["idx"], kw["score"], kw["names"], kw["style"])
        want = O.draw(black, cap=O.CAP, glyphs=glyphs, **kw)
        assert np.array_equal(got, want), (name, np.argwhere(got != want)[:6])
        assert lit > 0
        ran += 1
    assert ran >= 5
    # boxes whose geometry reaches the limits of int: nothing may overflow, nothing may be written outside
    big = 8388607.0
    det = np.zeros((1, 6, 5), np.float32)
    det[0, :, :4] = [(-big, -big, big, big), (-big, 3, 5, big), (big - 1, big - 1, big, big), (0, 0, big, 1), (-big, -big, -big + 1, -big + 1), (2, 2, 9, 9)]
    idx, score = np.zeros((1, 6), np.int32), np.full((1, 6), 3.0e38, np.float32)
    style = O.Style(thickness=15, text_scale=4, proportion=1.0)
    got, _ = run_case(driver, tmp_path, H, W, det, np.array([6], np.int32), idx, score, [b"x" * 40], style)
    want = O.draw(black[:1], det, np.array([6]), 6, glyphs, idx=idx, score=score, id_stride=6, names=[b"x" * 40], style=style)
    assert np.array_equal(got, want)
