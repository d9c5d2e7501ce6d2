"""CPU: NV12 -> BGR on the host (fid_nv12_to_bgr_host, utils.helpers.nv12_to_bgr) against tests/nv12_oracle.py byte for byte: the three
standards, pitched layouts, the bytes that must never be read, hand-computed corners of the formula, every validation failure, and
csrc/yuv_core.h under AddressSanitizer + UBSan in a stand-alone program (tests/nv12_host_driver.cpp; nothing is preloaded)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import nv12_oracle as oracle
from scrfd_arcface_facerecognition_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("clang++")
SHAPES = [(2, 2), (46, 62), (48, 64)]
STANDARDS = list(oracle.COEFFS)


def layouts(H, W):
    """the issue's layout cases: dense, pitch = W + 2, four padding rows in front of the UV plane, slack between the frames"""
    return {
        "dense": dict(pitch=W, uv_offset=W * H, frame_stride=W * H * 3 // 2),
        "pitch+2": dict(pitch=W + 2, uv_offset=(W + 2) * H, frame_stride=(W + 2) * H * 3 // 2),
        "uv_padding": dict(pitch=W, uv_offset=W * (H + 4), frame_stride=W * (H + 4) + W * (H // 2)),
        "frame_slack": dict(pitch=W + 2, uv_offset=(W + 2) * (H + 4), frame_stride=(W + 2) * (H + 4) + (W + 2) * (H // 2) + 37),
    }


def host_convert(buf, B, H, W, standard, **layout):
    lib = _lib.load()
    desc = _lib.nv12_desc(H, W, standard=standard, **layout)
    out = np.full((max(B, 1), H, W, 3), 0xA5, np.uint8)
    rc = lib.fid_nv12_to_bgr_host(buf.ctypes.data_as(C.c_void_p), C.byref(desc), B, H, W, out.ctypes.data_as(C.c_void_p))
    return rc, out


def test_struct_matches_the_header():
    """fid_nv12_desc: int32 pitch, int64 uv_offset, int64 frame_stride, int32 standard with natural alignment"""
    d = _lib.Nv12Desc
    assert (d.pitch.offset, d.uv_offset.offset, d.frame_stride.offset, d.standard.offset, C.sizeof(d)) == (0, 8, 16, 24, 32)
    hdr = open(os.path.join(ROOT, "include", "faceid.h")).read()
    for std, macro in (("bt601", "FID_YUV_BT601_LIMITED_TABLE"), ("bt709", "FID_YUV_BT709_LIMITED_TABLE"), ("bt601_full", "FID_YUV_BT601_FULL_TABLE")):
        assert f"#define {macro} {{{', '.join(str(v) for v in oracle.table(std))}}}" in hdr, macro       # the header IS the rounding rule's result
    assert oracle.table("bt601") == (1220542, 2116026, -409993, -852492, 1673527, 16)                  # the issue's constants


@pytest.mark.parametrize("standard", STANDARDS)
@pytest.mark.parametrize("hw", SHAPES)
def test_host_twin_equals_the_oracle(hw, standard):
    H, W = hw
    for name, lay in layouts(H, W).items():
        outs = []
        for fill in (0xFF, 0x00):                       # every byte that must never be read, set both ways: the result may not move
            buf, _ = oracle.random_batch(7, 3, H, W, fill=fill, exact_end=False, **lay)
            rc, got = host_convert(buf, 3, H, W, standard, **lay)
            assert rc == 0, (name, _lib.load().fid_last_error())
            assert np.array_equal(got, oracle.nv12_to_bgr(buf, 3, H, W, standard=standard, **lay)), (name, fill)
            outs.append(got)
        assert np.array_equal(outs[0], outs[1]), name


def test_helper_wraps_the_host_twin():
    from scrfd_arcface_facerecognition_amd.utils.helpers import nv12_to_bgr
    H, W = 46, 62
    buf, _ = oracle.random_batch(3, 2, H, W)
    one = nv12_to_bgr(buf[:W * H * 3 // 2].reshape(H * 3 // 2, W), H, W)
    both = nv12_to_bgr(buf.reshape(2, H * 3 // 2, W), H, W, "bt709")
    assert one.shape == (H, W, 3) and both.shape == (2, H, W, 3)
    assert np.array_equal(one, oracle.nv12_to_bgr(buf, 1, H, W)[0])
    assert np.array_equal(both, oracle.nv12_to_bgr(buf, 2, H, W, standard="bt709"))
    with pytest.raises(ValueError):
        nv12_to_bgr(buf, H, W, "bt2020")


def one_pixel(Y, U, V, standard="bt601"):
    """a 2 x 2 frame of one colour through the library -> its BGR"""
    buf = np.array([Y, Y, Y, Y, U, V], np.uint8)
    rc, got = host_convert(buf, 1, 2, 2, standard)
    assert rc == 0
    assert (got == got[0, 0, 0]).all()
    return tuple(int(v) for v in got[0, 0, 0])


def test_hand_computed_corners():
    cy, cub, cug, cvg, cvr, _ = (1220542, 2116026, -409993, -852492, 1673527, 16)
    half, sat = 1 << 19, lambda v: min(max(v, 0), 255)
    assert one_pixel(16, 128, 128) == (0, 0, 0)
    white = sat(((235 - 16) * cy + half) >> 20)          # neutral chroma: all three channels are the luma term alone
    assert one_pixel(235, 128, 128) == (white, white, white) and white == 255
    assert one_pixel(0, 128, 128) == (0, 0, 0)            # max(0, Y - 16): below black is black, not negative
    assert one_pixel(0, 128, 128) == one_pixel(16, 128, 128) == one_pixel(7, 128, 128)
    yy = (255 - 16) * cy
    hi = one_pixel(255, 255, 255)
    assert hi == (sat((yy + cub * 127 + half) >> 20), sat((yy + cug * 127 + cvg * 127 + half) >> 20), sat((yy + cvr * 127 + half) >> 20))
    assert hi[0] == 255 and hi[2] == 255
    lo = one_pixel(255, 0, 0)
    assert lo == (sat((yy - cub * 128 + half) >> 20), sat((yy - cug * 128 - cvg * 128 + half) >> 20), sat((yy - cvr * 128 + half) >> 20))
    # With these constants Y = 255 is too bright for zero chroma to reach the lower clamp: (239 * CY - 128 * CUB + 2^19) >> 20 = 20 and
    # (239 * CY - 128 * CVR + 2^19) >> 20 = 74.  The formula is the definition, so those are the bytes; the lower clamp is pinned where it
    # does engage, at black-level luma, where the raw B and R sums are negative.
    assert lo == (20, 255, 74)
    assert one_pixel(16, 0, 0) == (0, sat((-cug * 128 - cvg * 128 + half) >> 20), 0)
    assert (-cub * 128 + half) >> 20 < 0 and (-cvr * 128 + half) >> 20 < 0
    # a negative sum must shift arithmetically: Y = 16, U = 0 gives B = sat8(-(cub * 128 - half) >> 20) = 0, G > 0
    assert one_pixel(16, 0, 128) == (0, sat((-cug * 128 + half) >> 20), 0)
    # full range: no luma offset, Y = 255 stays 255
    assert one_pixel(255, 128, 128, "bt601_full") == (255, 255, 255) and one_pixel(1, 128, 128, "bt601_full") == (1, 1, 1)


@pytest.mark.parametrize("what,B,H,W,layout", [
    ("odd H", 1, 3, 4, dict(pitch=4, uv_offset=16, frame_stride=32)),
    ("odd W", 1, 4, 3, dict(pitch=4, uv_offset=16, frame_stride=32)),
    ("pitch below W", 1, 4, 4, dict(pitch=3, uv_offset=16, frame_stride=32)),
    ("planes overlap", 1, 4, 4, dict(pitch=4, uv_offset=15, frame_stride=32)),
    ("frames overlap", 2, 4, 4, dict(pitch=4, uv_offset=16, frame_stride=23)),
    ("unknown standard", 1, 4, 4, dict(pitch=4, uv_offset=16, frame_stride=24, standard=3)),
    ("negative standard", 1, 4, 4, dict(pitch=4, uv_offset=16, frame_stride=24, standard=-1)),
    ("no frames", 0, 4, 4, dict(pitch=4, uv_offset=16, frame_stride=24)),
])
def test_validation_is_all_or_nothing(what, B, H, W, layout):
    lib = _lib.load()
    layout = dict(layout)
    rc, out = host_convert(np.zeros(256, np.uint8), B, H, W, layout.pop("standard", "bt601"), **layout)
    assert rc == -1 and lib.fid_last_error(), what              # FID_E_INVALID with a message
    assert (out == 0xA5).all(), what                              # nothing written


def test_null_arguments_are_refused():
    lib = _lib.load()
    desc = _lib.nv12_desc(4, 4)
    buf = np.zeros(64, np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    assert lib.fid_nv12_to_bgr_host(None, C.byref(desc), 1, 4, 4, p) == -1
    assert lib.fid_nv12_to_bgr_host(p, None, 1, 4, 4, p) == -1 and b"layout" in lib.fid_last_error()
    assert lib.fid_nv12_to_bgr_host(p, C.byref(desc), 1, 4, 4, None) == -1
    # the device entry points with a NULL context: FID_E_INVALID on a host without a GPU too
    assert lib.fid_nv12_to_bgr(None, p, C.byref(desc), 1, 4, 4, p) == -1
    assert lib.fid_letterbox_nv12(None, p, C.byref(desc), 1, 4, 4, p, 4, 4, None) == -1
    assert lib.fid_tile_cut_nv12(None, p, C.byref(desc), 1, 4, 4, None, 1, p, 4, 4) == -1
    assert lib.fid_align_crops_nv12(None, p, C.byref(desc), 1, 4, 4, p, p, 1, 1, p, None) == -1
    assert lib.fid_align_crops_packed_nv12(None, p, C.byref(desc), 1, 4, 4, p, 1, p, 1, p, None) == -1


def test_nv12_frames_holder_defaults_to_the_dense_layout():
    fr = _lib.Nv12Frames(0x1000, 1080, 1920)
    assert (fr.desc.pitch, fr.desc.uv_offset, fr.desc.frame_stride, fr.desc.standard) == (1920, 1920 * 1080, 1920 * 1080 * 3 // 2, 0)
    fr = _lib.Nv12Frames(0x1000, 1080, 1920, pitch=2048, uv_offset=2048 * 1088, standard="bt709")
    assert (fr.desc.pitch, fr.desc.uv_offset, fr.desc.frame_stride, fr.desc.standard) == (2048, 2048 * 1088, 2048 * 1088 + 2048 * 540, 1)
    with pytest.raises(ValueError):
        _lib.Nv12Frames(0x1000, 4, 4, standard="rec2020")


# ---- csrc/yuv_core.h under the sanitizers, as a program of its own ----
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if CXX is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("nv12_driver") / "nv12_host_driver"
    cmd = [CXX, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "scrfd_arcface_facerecognition_amd", "csrc"), os.path.join(ROOT, "tests", "nv12_host_driver.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True)
    return str(exe)


def run_driver(driver, tmp_path, buf, B, H, W, standard, pitch, uv_offset, frame_stride):
    case, dst = tmp_path / "case.bin", tmp_path / "out.bin"
    with open(case, "wb") as f:
        f.write(np.array([B, H, W, pitch, standard], np.int32).tobytes())
        f.write(np.array([uv_offset, frame_stride, buf.size], np.int64).tobytes())
        f.write(buf.tobytes())
    p = subprocess.run([driver, str(case), str(dst)], capture_output=True, text=True)
    return p, dst


@pytest.mark.parametrize("layout", ["dense", "pitch+2", "frame_slack"])
@pytest.mark.parametrize("hw", SHAPES)
def test_bounds_under_the_sanitizers(driver, tmp_path, hw, layout):
    """the allocation ends with the last byte the layout lets the library read: the last UV row of the last frame, W bytes of it"""
    H, W = hw
    lay = layouts(H, W)[layout]
    full, _ = oracle.random_batch(11, 2, H, W, **lay)
    buf = full[:oracle.needed_bytes(2, H, W, **lay)].copy()
    if layout == "dense":
        assert buf.size == full.size == 2 * W * H * 3 // 2          # pitch = W: the exact size of two dense frames
    for std in STANDARDS:
        p, dst = run_driver(driver, tmp_path, buf, 2, H, W, oracle.STANDARD_ID[std], **lay)
        assert p.returncode == 0, p.stderr[-2000:]
        got = np.frombuffer(open(dst, "rb").read(), np.uint8).reshape(2, H, W, 3)
        assert np.array_equal(got, oracle.nv12_to_bgr(full, 2, H, W, standard=std, **lay)), std


def test_driver_refuses_a_bad_layout(driver, tmp_path):
    p, _ = run_driver(driver, tmp_path, np.zeros(24, np.uint8), 1, 4, 4, 0, 4, 15, 24)
    assert p.returncode == 3 and "overlap" in p.stderr
