"""CPU: fid_face_measure_host (csrc/measure.hip over csrc/measure_core.h) against tests/measure_oracle.py, word for word: 8 int64 and 8 float32
words per row, compared as bytes.  No device involved."""
import ctypes as C

import numpy as np
import pytest

import measure_oracle as O


def host(crops, kps=None, src=None, M=None, n=None):
    from scrfd_arcface_facerecognition_amd import _lib
    lib = _lib.load()
    crops = np.ascontiguousarray(crops, np.uint8)
    n = len(crops) if n is None else n
    stats, meas = np.full((max(n, 1), 8), -7, np.int64), np.full((max(n, 1), 8), -7.0, np.float32)
    p = lambda a, dt: None if a is None else np.ascontiguousarray(a, dt).ctypes.data_as(C.c_void_p)
    keep = [p(kps, np.float32), p(src, np.int32), p(M, np.float64)]
    rc = lib.fid_face_measure_host(crops.ctypes.data_as(C.c_void_p), n, keep[0], keep[1], keep[2], stats.ctypes.data_as(C.c_void_p),
                                   meas.ctypes.data_as(C.c_void_p))
    return rc, stats[:n], meas[:n]


def same(got, want, names=None):
    (gs, gm), (ws, wm) = got, want
    for i in range(len(ws)):
        assert gs[i].tolist() == ws[i].tolist(), (i, names[i] if names else None)
        assert gm[i].tobytes() == wm[i].tobytes(), (i, names[i] if names else None, gm[i], wm[i])


def test_pixel_cases_equal_the_oracle():
    names, crops = zip(*O.pixel_cases())
    crops = np.stack(crops)
    rc, stats, meas = host(crops)
    assert rc == 0
    same((stats, meas), O.measure(crops), names)
    by = dict(zip(names, range(len(names))))
    # the checkerboard is the case a 32-bit accumulator breaks on
    i = by["checkerboard"]
    assert stats[i, 4] == 6400 * 1020 ** 2 > 2 ** 32 and stats[i, 3] == 0 and meas[i, 0] == np.float32(1040400.0)
    assert stats[by["zeros"]].tolist() == [6400, 0, 0, 0, 0, 6400, 0, 1] and meas[by["zeros"], 3] == 1.0
    assert stats[by["ones"]].tolist() == [6400, 6400 * 255, 6400 * 255 ** 2, 0, 0, 0, 6400, 1]
    for name, y in (("blue", 29), ("green", 149), ("red", 77)):          # the weights and the rounding
        assert stats[by[name], 1] == 6400 * y and meas[by[name], 1] == np.float32(y), name
    # a single bright pixel: inside the window, reached only as a neighbour, out of reach
    assert stats[by["dot_16_16"], 1:5].tolist() == [255, 255 ** 2, 255 * 2, 1020 ** 2 + 2 * 255 ** 2]
    assert stats[by["dot_95_95"], 1:5].tolist() == [255, 255 ** 2, 255 * 2, 1020 ** 2 + 2 * 255 ** 2]
    assert stats[by["dot_15_16"], 1:5].tolist() == [0, 0, -255, 255 ** 2] and stats[by["dot_96_95"], 1:5].tolist() == [0, 0, -255, 255 ** 2]
    assert stats[by["dot_14_50"]].tolist() == stats[by["zeros"]].tolist() == stats[by["dot_0_0"]].tolist()
    assert meas[:, 4:].tobytes() == bytes(4 * 4 * len(names))             # no pose input: words 4 .. 7 are 0, flag bit 1 clear


def test_pose_cases_equal_the_oracle():
    ps = O.pose_cases()
    names = [p[0] for p in ps]
    kps = np.stack([p[1].reshape(10) for p in ps])
    M = np.stack([p[2] for p in ps])
    crops = np.random.default_rng(3).integers(0, 256, (len(ps), 112, 112, 3), dtype=np.uint8)
    rc, stats, meas = host(crops, kps=kps, M=M)
    assert rc == 0
    same((stats, meas), O.measure(crops, kps=kps, M=M), names)
    by = dict(zip(names, range(len(names))))
    assert meas[by["template"], 4:].tobytes() == bytes(16) and stats[by["template"], 7] == 3          # exactly 0, 0, 0 and valid
    i = by["nose_shifted"]
    assert stats[i, 7] == 3 and meas[i, 4] > 0 and meas[i, 5] < 0 and meas[i, 6] > 0
    i = by["rotated_scaled"]
    assert stats[i, 7] == 3 and abs(meas[i, 4]) < 1e-5 and abs(meas[i, 5]) < 1e-5 and meas[i, 6] < 1e-4
    for name in ("w_negative", "w_zero", "h_negative", "h_zero", "nan_in_M", "inf_in_M", "zero_M", "nan_landmark"):
        assert stats[by[name], 7] == 1 and meas[by[name], 4:].tobytes() == bytes(16), name
    assert all(stats[by[f"random_{k}"], 7] == 3 for k in range(4))


def test_row_table_picks_landmarks_and_zeroes_holes():
    c = O.cases()
    rc, stats, meas = host(c["crops"], kps=c["kps"], src=c["src"], M=c["M"])
    assert rc == 0
    want = O.measure(c["crops"], kps=c["kps"], src=c["src"], M=c["M"])
    same((stats, meas), want, c["names"])
    holes = c["src"] < 0
    assert holes.sum() >= 3 and not stats[holes].any() and meas[holes].tobytes() == bytes(32 * int(holes.sum()))
    assert (stats[~holes, 0] == 6400).all() and (stats[~holes, 7] & 1).all() and (stats[~holes, 7] == 3).sum() >= 8
    # the same rows with the landmark table shuffled give other pose words: src really picks the row
    rc, _, other = host(c["crops"], kps=c["kps"][::-1], src=c["src"], M=c["M"])
    assert rc == 0 and other[:, 4:7].tobytes() != meas[:, 4:7].tobytes() and other[:, :4].tobytes() == meas[:, :4].tobytes()
    # pixel part only, with the table
    rc, s2, m2 = host(c["crops"], src=c["src"])
    assert rc == 0
    same((s2, m2), O.measure(c["crops"], src=c["src"]))


def test_arguments():
    from scrfd_arcface_facerecognition_amd import _lib
    assert C.sizeof(_lib.MeasureConfig) == 20
    assert _lib.MEASURE_KEYS == O.KEYS == ("sharpness", "mean", "contrast", "clipped", "yaw", "pitch", "residual")
    crops = np.zeros((2, 112, 112, 3), np.uint8)
    kps, M = np.zeros((2, 10), np.float32), np.zeros((2, 6))
    rc, stats, meas = host(crops, kps=kps)                                # exactly one of the two: refused, nothing written
    assert rc == -1 and (stats == -7).all() and (meas == -7).all()
    assert b"together" in _lib.load().fid_last_error()
    assert host(crops, M=M)[0] == -1
    assert host(crops, n=-1)[0] == -1
    rc, stats, meas = host(crops, n=0)
    assert rc == 0 and stats.shape == (0, 8)
    lib = _lib.load()
    out = np.zeros(16, np.int64).ctypes.data_as(C.c_void_p)
    assert lib.fid_face_measure_host(None, 1, None, None, None, out, out) == -1
    assert lib.fid_face_measure_host(crops.ctypes.data_as(C.c_void_p), 1, None, None, None, None, out) == -1
    assert lib.fid_face_measure(None, crops.ctypes.data_as(C.c_void_p), 1, None, None, None, out, out) == -1         # NULL context: before any device call


def test_helper_measure_crops():
    from utils.helpers import measure_crops
    c = O.cases()
    faces = c["src"] >= 0
    crops, kps, M = c["crops"][faces], c["kps"][c["src"][faces]], c["M"][faces]
    got = measure_crops(crops, kps=kps.reshape(-1, 5, 2), M=M.reshape(-1, 2, 3))
    _, want = O.measure(crops, kps=kps, M=M)
    assert len(got) == len(crops)
    for i, d in enumerate(got):
        assert list(d) == list(O.KEYS) + ["pose_valid"]
        assert [np.float32(d[k]).tobytes() for k in O.KEYS] == [want[i, j].tobytes() for j in range(7)]
    one = measure_crops(crops[0])                                         # a single crop, pixel part only
    assert len(one) == 1 and one[0]["pose_valid"] is False and one[0]["sharpness"] == float(want[0, 0])
