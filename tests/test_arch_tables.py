"""The architecture tables against the only model facts the reference holds: the file sizes of its five ONNX weights (reference
README.md:57-61).  oracle/nets.py interprets the SAME archs.py graph the product lowers, so a wrong table is invisible
to every parity test -- the size of the file the table claims to describe is not.  fp32 parameter bytes of a table (every array an
insightface-style export stores: conv / FC weights and biases, BatchNorm gamma / beta / mean / var, PReLU slopes, the head's scale) must
be within 3 % of the listed size.  GitHub's release page prints MiB as "MB": 166 "MB" of w600k_r50 are 174.5e6 bytes = 43.6 M values,
the IResNet-50 of SURVEY B.2 exactly.

Round 5 outcome: det_10g needs per-stride head towers (shared: -7 %), w600k_mbf the (2, 8, 12, 4)-block MobileFaceNet (the (1, 4, 6, 2)
table of rounds 1-4: -39 %); both were changed (archs.scrfd_10g / archs.mobilefacenet docstrings)."""
import os
import re

import pytest

from scrfd_arcface_facerecognition_amd import archs

# reference README.md:57-61 (data, not code): basename -> listed size
README_SIZES_MIB = {"det_500m": 2.41, "det_2.5g": 3.14, "det_10g": 16.1, "w600k_mbf": 12.99, "w600k_r50": 166.0}
# the weights table of that README (README.md:55-61), stored verbatim as a fixture
README_TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "weights_table.md")


def table_mib(arch):
    net = archs.ARCHS[arch]()
    return sum(v.size for v in archs.synth_params(net, 0).values()) * 4 / 2 ** 20


@pytest.mark.parametrize("basename", sorted(README_SIZES_MIB))
def test_table_parameter_bytes_match_the_listed_file_size(basename):
    arch = archs.ONNX_BASENAMES[basename]
    got, want = table_mib(arch), README_SIZES_MIB[basename]
    assert abs(got / want - 1) < 0.03, f"{arch}: {got:.2f} MiB of fp32 parameters vs {want} listed for {basename}.onnx"


def test_the_rejected_tables_do_not_match():
    """what the check is worth: the two tables rounds 1-4 used fail it"""
    small = table_mib("arcface_mbf_small")
    assert abs(small / README_SIZES_MIB["w600k_mbf"] - 1) > 0.3
    shared = archs.scrfd_resnet("scrfd_10g", (640, 640), head_shared=True)
    mib = sum(v.size for v in archs.synth_params(shared, 0).values()) * 4 / 2 ** 20
    assert abs(mib / README_SIZES_MIB["det_10g"] - 1) > 0.05


def test_fixture_equals_the_reference_readme():
    rows = dict(re.findall(r"\[(\w[\w.]*)\.onnx\]\([^)]*\)\s*\|\s*([\d.]+)\s*MB", open(README_TABLE).read()))
    assert {k: float(v) for k, v in rows.items()} == README_SIZES_MIB
