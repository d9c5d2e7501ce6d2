"""CPU: csrc/relink_core.h under AddressSanitizer + UBSan.  tests/relink_host_driver.cpp -- a stand-alone program that includes only that
header -- runs the relinker's walk over the tracked walks of tests/relink_calls.py and over hand-made limits in heap buffers of exactly the
specified sizes: a read past a frame's last detection, past the last row or the last pool entry, a write past a table's last word, or a
signed overflow ends the program.  Its person tables and its state after every step are then compared with tests/relink_oracle.py, byte
for byte.  Nothing is preloaded and nothing is loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import relink_oracle as O
from relink_calls import SHAPES, THRESH, WALKS, WINDOW, differs, walk_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("clang++")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if CXX is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("relink_driver") / "relink_host_driver"
    cmd = [CXX, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "scrfd_arcface_facerecognition_amd", "csrc"), os.path.join(ROOT, "tests", "relink_host_driver.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True)
    return str(exe)


def run_case(driver, tmp_path, S, T, L, dim, steps, thresh, window, max_age, n_rows=None):
    """-> per step (person, [live, pool, frames, live_q, pool_q])"""
    B, cap = steps[0][2].shape[:2]
    src_f, dst_f = tmp_path / "case.bin", tmp_path / "out.bin"
    with open(src_f, "wb") as f:
        f.write(np.array([S, T, L, dim, B, cap, len(steps), window, max_age], np.int32).tobytes())
        f.write(np.array([thresh], np.float32).tobytes())
        for stream, counts, track, offsets, src, q in steps:
            n = len(q) if n_rows is None else n_rows
            f.write(np.array([len(src), n], np.int32).tobytes())
            for a in (stream, counts, track, offsets, src):
                f.write(np.ascontiguousarray(a, np.int32).tobytes())
            f.write(np.ascontiguousarray(q[:n], np.float16).tobytes())
    p = subprocess.run([driver, str(src_f), str(dst_f)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    raw = np.fromfile(dst_f, np.uint8)
    shapes = [((B, cap, 2), np.int32), ((S, T, 8), np.int32), ((S, L, 8), np.int32), ((S,), np.int32), ((S, T, dim), np.float16),
              ((S, L, dim), np.float16)]
    out, at = [], 0
    for _ in steps:
        arrays = []
        for shape, dt in shapes:
            n = int(np.prod(shape)) * np.dtype(dt).itemsize
            arrays.append(raw[at:at + n].view(dt).reshape(shape))
            at += n
        out.append((arrays[0], arrays[1:]))
    assert at == raw.size
    return out


@pytest.mark.parametrize("T, cap, L", SHAPES)
def test_walks_under_the_sanitizers(driver, tmp_path, T, cap, L):
    for dim in (8, 40):
        steps, want, _ = walk_case(T, cap, L, dim)
        got = run_case(driver, tmp_path, WALKS[(T, cap)][1], T, L, dim, steps, THRESH, WINDOW, 1)
        for call in range(len(steps)):
            assert np.array_equal(got[call][0], want[call][0]), (dim, call)
            assert not differs(got[call][1], want[call][1]), (dim, call)


def test_limits_under_the_sanitizers(driver, tmp_path):
    """counts far outside [0, cap], src entries and offsets far outside their tables, n_rows below the row table, all 64 slots retiring
    into a pool of 64 in one frame and 64 new tracks linking in one later frame"""
    T = L = cap = 64
    dim, B = 64, 5
    rows = np.zeros((T, dim), np.float16)
    rows[np.arange(T), np.arange(T)] = 1
    NEW = (1 << 8) | (1 << 9)
    track = np.full((B, cap, 2), -1, np.int32)
    track[0, :, 0], track[0, :, 1] = np.arange(T), np.arange(T) | NEW
    track[3, :, 0], track[3, :, 1] = 64 + np.arange(T), np.arange(T)[::-1] | NEW
    counts = np.array([2 ** 31 - 1, -2 ** 31, 0, 64, 70], np.int32)
    offsets = np.array([-5, 64, 64, 64, 128, 2 ** 31 - 1], np.int32)
    src = np.full(140, -1, np.int32)
    src[:64] = np.arange(64)
    src[64:128] = 3 * cap + np.arange(64)
    src[128:] = (2 ** 31 - 1, -2 ** 31, 4 * cap, 5 * cap, 0, 3 * cap + 1, -1, -1, -1, -1, -1, -1)
    q = np.concatenate([rows, rows[::-1], np.ones((12, dim), np.float16)])
    step = (np.zeros(B, np.int32), counts, track, offsets, src, q)
    for n_rows in (140, 100):
        ref = O.Relinker(1, T, L, dim)
        want = ref.step(*step[:5], len(src), n_rows, q, 0.5, 10, 1)
        got = run_case(driver, tmp_path, 1, T, L, dim, [step], 0.5, 10, 1, n_rows=n_rows)
        assert np.array_equal(got[0][0], want) and not differs(got[0][1], ref.state())
        assert len(ref.links) == (64 if n_rows == 140 else 36) and (ref.pool[0, :, 0] == -1).sum() == len(ref.links)
