"""CPU: csrc/calib_core.h under AddressSanitizer + UBSan.  tests/calib_host_driver.cpp -- a stand-alone program that includes only that header --
runs the stores of tests/calib_cases.py in heap buffers of exactly the specified sizes: a read past the last gallery row, position or label, a
write past an output's last entry, an out-of-range float-to-int conversion or a signed overflow ends the program.  Its outputs are then compared
with tests/calib_oracle.py, bit for bit.  Nothing is preloaded and nothing is loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import calib_cases as K
import calib_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("clang++")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if CXX is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("calib_driver") / "calib_host_driver"
    cmd = [CXX, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "scrfd_arcface_facerecognition_amd", "csrc"), os.path.join(ROOT, "tests", "calib_host_driver.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True)
    return str(exe)


def run_case(driver, tmp_path, g16, rows, labels, bins, expect=0):
    src, dst = tmp_path / "case.bin", tmp_path / "out.bin"
    src.write_bytes(K.pack_case(g16, rows, labels, bins))
    p = subprocess.run([driver, str(src), str(dst)], capture_output=True, text=True)
    assert p.returncode == expect, p.stderr[-2000:]
    if expect:
        return p.stderr
    n = len(g16) if rows is None else len(rows)
    raw = dst.read_bytes()
    assert len(raw) == 16 * bins + 16 * n + 32
    hist = np.frombuffer(raw, np.uint64, 2 * bins).reshape(2, bins)
    per = np.frombuffer(raw, np.int32, 4 * n, 16 * bins)
    summary = np.frombuffer(raw, np.uint64, 4, 16 * bins + 16 * n)
    return hist, per[:n], per[n:2 * n].view(np.float32), per[2 * n:3 * n], per[3 * n:].view(np.float32), tuple(int(v) for v in summary)


@pytest.mark.parametrize("n, dim", [(1, 32), (17, 512), (129, 32), (300, 32)])
def test_exact_stores_under_the_sanitizers(driver, tmp_path, n, dim):
    g, rows, labels, plants = K.exact_case(n, dim)
    g16 = K.with_marker(K.unit_f16(g), plants)
    for bins in K.BINS:
        assert K.same(run_case(driver, tmp_path, g16, rows, labels, bins), O.score_hist(g16, rows, labels, bins)) is None, bins
    all_labels = (np.arange(len(g16)) % 3).astype(np.int32)
    assert K.same(run_case(driver, tmp_path, g16, None, all_labels, 64), O.score_hist(g16, None, all_labels, 64)) is None


def test_rows_far_outside_and_extreme_labels_under_the_sanitizers(driver, tmp_path):
    g, rows, labels, plants = K.exact_case(129, 32)
    rows, labels = rows.copy(), labels.copy()
    rows[6], rows[9] = 2 ** 31 - 1, -2 ** 31
    labels[20], labels[21], labels[22] = 2 ** 31 - 1, 2 ** 31 - 1, -2 ** 31
    g16 = K.with_marker(K.unit_f16(g), plants)
    got = run_case(driver, tmp_path, g16, rows, labels, 100)
    assert K.same(got, O.score_hist(g16, rows, labels, 100)) is None
    assert got[3][20] == 21 and got[3][21] == 20 and got[1][22] == -1


def test_scores_far_outside_the_bins_and_non_finite_ones_under_the_sanitizers(driver, tmp_path):
    """rows that are not unit rows: finite scores of +-1.7e10 (past int32 before and after the multiply with bins / 2: the clamp is done on the
    float), infinite ones and NaNs"""
    g16 = np.zeros((5, 32), np.float16)
    g16[0, :4] = 65504
    g16[1, :4] = -65504
    g16[2, :] = 65504
    g16[3, 0] = np.inf
    g16[4, 1] = np.nan
    labels = np.int32([0, 0, 1, 1, 0])
    for bins in (2, 4096):
        got = run_case(driver, tmp_path, g16, None, labels, bins)
        assert K.same(got, O.score_hist(g16, None, labels, bins)) is None
        assert got[0][0][0] == 1 and got[0].sum() == 3 and got[5] == (5, 1, 2, 7) and got[0][1][bins - 1] == 1 and got[0][1][0] == 1


def test_the_check_refuses_before_anything_is_written(driver, tmp_path):
    g, rows, labels, plants = K.exact_case(17, 32)
    for bins in (0, 3, 4098, -4):
        assert "refused" in run_case(driver, tmp_path, K.unit_f16(g), rows, labels, bins, expect=3)
