"""CPU: csrc/cluster_core.h under AddressSanitizer + UBSan.  tests/cluster_host_driver.cpp -- a stand-alone program that includes only that
header -- clusters the stores of tests/cluster_cases.py in heap buffers of exactly the specified sizes: a read past the last gallery row or the
last position, a write past an output's last entry, or a signed overflow ends the program.  Its outputs are then compared with
tests/cluster_oracle.py, bit for bit.  Nothing is preloaded and nothing is loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import cluster_cases as K
import cluster_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("clang++")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if CXX is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("cluster_driver") / "cluster_host_driver"
    cmd = [CXX, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "scrfd_arcface_facerecognition_amd", "csrc"), os.path.join(ROOT, "tests", "cluster_host_driver.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True)
    return str(exe)


def run_case(driver, tmp_path, g16, rows, thresh, min_pts):
    src, dst = tmp_path / "case.bin", tmp_path / "out.bin"
    src.write_bytes(K.pack_case(g16, rows, thresh, min_pts))
    p = subprocess.run([driver, str(src), str(dst)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    n = len(g16) if rows is None else len(rows)
    raw = np.fromfile(dst, np.int32)
    assert raw.size == 4 * n + 6
    return raw[:n], raw[n:2 * n], raw[2 * n:3 * n], raw[3 * n:4 * n].view(np.float32), tuple(int(v) for v in raw[4 * n:])


@pytest.mark.parametrize("n, dim", [(1, 32), (17, 512), (129, 32), (300, 32)])
def test_probe_stores_under_the_sanitizers(driver, tmp_path, n, dim):
    g, rows, _ = K.probe_case(n, dim)
    g16 = K.unit_f16(g)
    for thresh in (0.75, K.ABOVE):
        for min_pts in (1, 2, 3):
            assert K.same(run_case(driver, tmp_path, g16, rows, thresh, min_pts), O.cluster(g16, rows, thresh, min_pts)) is None, (thresh, min_pts)
    assert K.same(run_case(driver, tmp_path, g16, None, 0.75, 2), O.cluster(g16, None, 0.75, 2)) is None


def test_rows_outside_the_gallery_and_zero_rows_under_the_sanitizers(driver, tmp_path):
    """every position but seven names a row outside [0, G), a zero row or nothing at all; one entry is the largest int32"""
    for equal in (True, False):
        g, rows, pos = K.tie_case(equal, p_low=False)
        rows = rows.copy()
        rows[1], rows[4] = 2 ** 31 - 1, -2 ** 31
        g16 = K.unit_f16(g)
        np.ascontiguousarray(g16).view(np.uint16)[38, 0] = 0x8000          # a -0.0 marker row
        rows[6] = 38
        got = run_case(driver, tmp_path, g16, rows, 0.625, 4)
        assert K.same(got, O.cluster(g16, rows, 0.625, 4)) is None
        assert got[4] == (2, 2, 5, 0, 7, 0) and got[2][pos["x"]] == (pos["Q"] if equal else pos["P"])


def test_a_path_under_the_sanitizers(driver, tmp_path):
    g, rows, _ = K.path_case(29, 32)
    g16 = K.unit_f16(g)
    got = run_case(driver, tmp_path, g16, rows, 0.75, 3)
    assert K.same(got, O.cluster(g16, rows, 0.75, 3)) is None and got[4] == (1, 27, 2, 0, 29, 0)
