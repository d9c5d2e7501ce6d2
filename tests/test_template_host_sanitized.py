"""CPU: csrc/template_core.h under AddressSanitizer + UBSan.  tests/template_host_driver.cpp -- a stand-alone program that includes only that
header -- runs the cases of tests/template_cases.py in heap buffers of exactly the specified sizes: a read past the last gallery row, position,
label or weight, a write past an output's last entry, a shift or a signed overflow ends the program.  Its outputs are then compared with
tests/template_oracle.py, byte for byte.  Nothing is preloaded and nothing is loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import template_cases as K
import template_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("clang++")
CASES = K.all_cases()


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if CXX is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("template_driver") / "template_host_driver"
    cmd = [CXX, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "scrfd_arcface_facerecognition_amd", "csrc"), os.path.join(ROOT, "tests", "template_host_driver.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True)
    return str(exe)


def run_case(driver, tmp_path, c, expect=0):
    src, dst = tmp_path / "case.bin", tmp_path / "out.bin"
    src.write_bytes(K.pack_case(c))
    p = subprocess.run([driver, str(src), str(dst)], capture_output=True, text=True)
    assert p.returncode == expect, p.stderr[-2000:]
    if expect:
        return p.stderr
    n, P, dim = K.n_of(c), c["P"], c["g16"].shape[1]
    raw = dst.read_bytes()
    assert len(raw) == 2 * P * dim + 8 * n + 20 * P + 48
    at = 0

    def take(dtype, count):
        nonlocal at
        a = np.frombuffer(raw, dtype, count, at)
        at += a.nbytes
        return a
    return (take(np.float16, P * dim).reshape(P, dim), take(np.float32, n), take(np.int32, n), take(np.int32, 4 * P).reshape(P, 4),
            take(np.float32, P), tuple(int(v) for v in take(np.int64, 6)))


@pytest.mark.parametrize("name", sorted(CASES))
def test_cases_under_the_sanitizers(driver, tmp_path, name):
    c = CASES[name]
    assert K.same(run_case(driver, tmp_path, c), O.templates(c["g16"], c["rows"], c["labels"], c["weights"], c["P"], c["min_score"])) is None


def test_the_check_refuses_before_anything_is_written(driver, tmp_path):
    c = CASES["seven_dim32"]
    for bad in (dict(P=0), dict(P=K.n_of(c) + 1), dict(P=-2), dict(min_score=float("nan")), dict(min_score=float("inf"))):
        assert "refused" in run_case(driver, tmp_path, dict(c, **bad), expect=3)
