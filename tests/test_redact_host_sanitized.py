"""CPU: csrc/redact_core.h under AddressSanitizer + UBSan.  tests/redact_host_driver.cpp -- a stand-alone program that includes only that
header -- redacts the slot-form cases of tests/redact_oracle.py, and boxes whose geometry reaches the limits of the format, in heap buffers of
exactly B * H * W * 3 bytes or of exactly the NV12 allocation; a byte outside a frame, a read past an input array or a signed overflow in
the geometry ends the program.  Its frames are then compared with the oracle's, byte for byte.  One 4200 x 4200 frame of solid 255 under one
cell sums to 4 498 200 000 per channel, past 2^32: every byte must stay 255.  Nothing is preloaded and nothing is loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import nv12_oracle
import redact_oracle as R
from draw_nv12_calls import background, layouts
from draw_nv12_oracle import STANDARDS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("clang++")
STANDARD_ID = {"bt601": 0, "bt709": 1, "bt601_full": 2}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if CXX is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("redact_driver") / "redact_host_driver"
    cmd = [CXX, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "scrfd_arcface_facerecognition_amd", "csrc"), os.path.join(ROOT, "tests", "redact_host_driver.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True)
    return str(exe)


def run_case(driver, tmp_path, Bn, H, W, cap, det, counts, idx, style, frames=None, solid=-1, lay=None, standard="bt601", n_bytes=None):
    """frames: uint8 of exactly the allocation (BGR [B,H,W,3] or the flat NV12 buffer), or None with solid = the byte every frame holds"""
    nv12 = lay is not None
    lay = lay or dict(pitch=0, uv_offset=0, frame_stride=0)
    n_bytes = int(frames.size if frames is not None else n_bytes)
    src, dst = tmp_path / "case.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.array([Bn, H, W, cap, style.mode, style.who, style.cells, int(nv12), lay["pitch"], STANDARD_ID[standard], solid,
                          *style.fill_bgr[:3]], np.int32).tobytes())
        f.write(np.array([lay["uv_offset"], lay["frame_stride"], n_bytes], np.int64).tobytes())
        f.write(np.array([style.expand], np.float64).tobytes())
        for a, dt in ((det, np.float32), (counts, np.int32), (idx, np.int32)):
            f.write(np.ascontiguousarray(a, dt).tobytes())
        if frames is not None:
            f.write(np.ascontiguousarray(frames, np.uint8).tobytes())
    p = subprocess.run([driver, str(src), str(dst)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    return np.fromfile(dst, np.uint8)


def slot_cases(H, W):
    return [(name, kw) for name, kw in R.cases(H, W) if kw["idx"] is not None and kw["offsets"] is None and kw["id_stride"] == R.CAP]


def limit_boxes():
    big = 8388607.0
    det = np.zeros((1, 7, 5), np.float32)
    det[0, :, :4] = [(-big, -big, big, big), (-big, 3, 5, big), (big - 1, big - 1, big, big), (0, 0, big, 1), (-big, -big, -big + 1, -big + 1),
                     (2, 2, 9, 9), (-big, -big, 7, 7)]
    return det, np.array([7], np.int32), np.full((1, 7), -1, np.int32)


@pytest.mark.parametrize("H, W", [(48, 80), (37, 67)])
def test_bgr_cases_under_the_sanitizers(driver, tmp_path, H, W):
    frames = np.random.default_rng(H * W).integers(0, 256, (R.B, H, W, 3), dtype=np.uint8)
    ran = 0
    for name, kw in slot_cases(H, W):
        got = run_case(driver, tmp_path, R.B, H, W, R.CAP, kw["det"], kw["counts"], kw["idx"], kw["style"], frames)
        want = R.redact(frames, cap=R.CAP, **kw)
        assert np.array_equal(got.reshape(frames.shape), want), (name, np.argwhere(got.reshape(frames.shape) != want)[:6])
        ran += 1
    assert ran >= 10
    # boxes whose geometry reaches the limits of int: nothing may overflow, nothing may be written outside
    det, counts, idx = limit_boxes()
    for style in (R.Style(cells=1, expand=0.5), R.Style(cells=16, expand=0.5), R.Style(cells=16, expand=0.0), R.Style(mode=R.FILL, fill_bgr=(1, 2, 3))):
        got = run_case(driver, tmp_path, 1, H, W, 7, det, counts, idx, style, frames[:1])
        want = R.redact(frames[:1], det, counts, 7, idx=idx, id_stride=7, style=style)
        assert np.array_equal(got.reshape(want.shape), want), (style.cells, style.expand)
        assert (want != frames[:1]).any()


@pytest.mark.parametrize("standard", sorted(STANDARDS))
@pytest.mark.parametrize("H, W", [(48, 80), (38, 68)])
def test_nv12_cases_under_the_sanitizers(driver, tmp_path, standard, H, W):
    for lname, lay in layouts(H, W).items():
        buf = background(H * W, R.B, H, W, lay, exact=True)                # ends with the last UV byte of the last frame
        assert buf.size == nv12_oracle.needed_bytes(R.B, H, W, **lay)
        for name, kw in slot_cases(H, W):
            got = run_case(driver, tmp_path, R.B, H, W, R.CAP, kw["det"], kw["counts"], kw["idx"], kw["style"], buf, lay=lay, standard=standard)
            want = R.redact_nv12(buf, R.B, H, W, cap=R.CAP, standard=standard, **lay, **kw)
            assert np.array_equal(got, want), (lname, name, np.argwhere(got != want)[:6])
        det, counts, idx = limit_boxes()
        one = buf[:nv12_oracle.needed_bytes(1, H, W, **lay)]
        for style in (R.Style(cells=1, expand=0.5), R.Style(cells=16, expand=0.5), R.Style(mode=R.FILL, fill_bgr=(200, 30, 90))):
            got = run_case(driver, tmp_path, 1, H, W, 7, det, counts, idx, style, one, lay=lay, standard=standard)
            want = R.redact_nv12(one, 1, H, W, det, counts, 7, standard=standard, **lay, idx=idx, id_stride=7, style=style)
            assert np.array_equal(got, want), (lname, style.cells)


def test_a_sum_past_32_bits(driver, tmp_path):
    """4200 x 4200 of solid 255 under one cell: 17 640 000 pixels x 255 = 4 498 200 000 > 2^32 per channel"""
    S = 4200
    assert S * S * 255 == 4_498_200_000 > 2 ** 32
    det = np.zeros((1, 1, 5), np.float32)
    det[0, 0, :4] = (0, 0, S - 1, S - 1)
    style = R.Style(cells=1, expand=0.0)
    g = R.geometry(det[0, 0], style)
    assert g["c"] == S and R.clipped(g, S, S) == (0, 0, S - 1, S - 1)      # one cell, the whole frame
    got = run_case(driver, tmp_path, 1, S, S, 1, det, np.array([1], np.int32), np.full((1, 1), -1, np.int32), style, solid=255, n_bytes=S * S * 3)
    assert np.array_equal(got, np.full(S * S * 3, 255, np.uint8))
    lay = nv12_oracle.dense_layout(S, S)
    got = run_case(driver, tmp_path, 1, S, S, 1, det, np.array([1], np.int32), np.full((1, 1), -1, np.int32), style, solid=255, lay=lay,
                   n_bytes=S * S * 3 // 2)
    assert np.array_equal(got, np.full(S * S * 3 // 2, 255, np.uint8))
