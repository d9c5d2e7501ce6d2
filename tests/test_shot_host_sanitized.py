"""CPU: csrc/shot_core.h under AddressSanitizer + UBSan.  tests/shot_host_driver.cpp -- a stand-alone program that includes only that header --
scores the rows of tests/shot_oracle.py from heap buffers of exactly the stated sizes; its scores are then compared with the oracle's to the
bit.  Nothing is preloaded and nothing is loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from shot_oracle import measure_rows, shot_score

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("clang++")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if CXX is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("shot_driver") / "shot_host_driver"
    cmd = [CXX, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "scrfd_arcface_facerecognition_amd", "csrc"), os.path.join(ROOT, "tests", "shot_host_driver.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True)
    return str(exe)


@pytest.mark.parametrize("norms", [(100.0, 40.0, 8.0), (37.5, 11.0, 3.25)])
def test_scores_under_the_sanitizers(driver, tmp_path, norms):
    stats, measure = measure_rows(5, n=200, norms=norms)
    case, dst = tmp_path / "case.bin", tmp_path / "out.bin"
    with open(case, "wb") as f:
        f.write(np.array([len(stats)], np.int32).tobytes())
        f.write(np.array(norms, np.float32).tobytes())
        f.write(stats.tobytes())
        f.write(measure.tobytes())
    p = subprocess.run([driver, str(case), str(dst)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    assert int(p.stdout) == len(stats)
    got = np.frombuffer(open(dst, "rb").read(), np.float32)
    assert got.tobytes() == shot_score(stats, measure, *norms).tobytes()


def test_a_bad_normalisation_is_refused(driver, tmp_path):
    case = tmp_path / "case.bin"
    with open(case, "wb") as f:
        f.write(np.array([0], np.int32).tobytes())
        f.write(np.array([100.0, 0.0, 8.0], np.float32).tobytes())
    p = subprocess.run([driver, str(case), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert p.returncode == 3 and "normalisation" in p.stderr
