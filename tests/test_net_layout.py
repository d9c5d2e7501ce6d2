"""CPU: net_layout.py, the Python mirror of the layer-table format, says what the headers say: every OP_* / W_* / T_* enumerator of csrc/net.h,
every CF_* / ACT_* of csrc/conv.h and the record sizes of include/faceid.h, name by name and value by value, both ways."""
import os
import re

from conftest import ROOT
from scrfd_arcface_facerecognition_amd import lower, net_layout

CSRC = os.path.join(ROOT, "scrfd_arcface_facerecognition_amd", "csrc")


def header_enumerators(path, prefixes):
    """{NAME: value} of every `NAME = <int>` enumerator with one of the prefixes in a header (comments stripped)"""
    src = open(path).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    pairs = re.findall(r"\b((?:" + "|".join(prefixes) + r")_[A-Z0-9_]+)\s*=\s*(-?\d+)\s*[,}]", src)
    assert len(pairs) == len({n for n, _ in pairs}), "an enumerator is defined twice"
    return {n: int(v) for n, v in pairs}


def mirror(prefixes):
    return {k: v for k, v in vars(net_layout).items() if k.split("_")[0] in prefixes and k.isupper() and isinstance(v, int)}


def test_op_and_tensor_words_match_net_h():
    want = header_enumerators(os.path.join(CSRC, "net.h"), ("OP", "W", "T"))
    by = lambda p: {k for k in want if k.startswith(p + "_")}
    assert len(by("OP")) >= 10 and len(by("W")) >= 60 and len(by("T")) >= 7, sorted(want)     # (a regex that stops matching fails here)
    have = mirror(("OP", "W", "T"))
    del have["OP_WORDS"]                                            # (a record size, checked below)
    assert have == want, sorted(set(have.items()) ^ set(want.items()))
    assert all(0 <= v < net_layout.OP_WORDS for k, v in want.items() if k.startswith("W_"))
    assert all(0 <= v < net_layout.TENSOR_WORDS for k, v in want.items() if k.startswith("T_"))


def test_flags_and_activations_match_conv_h():
    want = header_enumerators(os.path.join(CSRC, "conv.h"), ("CF", "ACT"))
    assert sum(k.startswith("CF_") for k in want) >= 4 and sum(k.startswith("ACT_") for k in want) >= 3, sorted(want)
    assert mirror(("CF", "ACT")) == want
    assert net_layout.ACT == {k[4:].lower(): v for k, v in want.items() if k.startswith("ACT_")}


def test_record_sizes_match_faceid_h():
    src = open(os.path.join(ROOT, "include", "faceid.h")).read()
    sizes = {n: int(v) for n, v in re.findall(r"^#define\s+FID_(OP_WORDS|TENSOR_WORDS)\s+(\d+)\s*$", src, flags=re.M)}
    assert sizes == {"OP_WORDS": net_layout.OP_WORDS, "TENSOR_WORDS": net_layout.TENSOR_WORDS}


def test_lower_reexports_the_layout():
    names = [k for k in vars(net_layout) if k.isupper()] + ["record_tensors"]
    assert len(names) > 90 and all(getattr(lower, k) is getattr(net_layout, k) for k in names) and lower.CPAD == 32


def test_record_tensors_by_op_type():
    """the second-tensor words count only for their own op type (the same word means a blob offset in another)"""
    L = net_layout
    rec = [0] * L.OP_WORDS
    rec[L.W_SRC], rec[L.W_DST], rec[L.W_RES] = 3, 4, -1
    rec[L.W_X_DST2], rec[L.W_L_LAT], rec[L.W_X_SRC2], rec[L.W_S_DST2] = 8, 9, 6, 7
    want = {L.OP_CONV: ([3, 5], [4, 7]), L.OP_LATFPN: ([3], [4, 8]), L.OP_STEMBLOCK: ([3], [4, 6]), L.OP_BBLOCK: ([3], [4]), L.OP_MBBLOCK: ([3], [4])}
    for kind, rw in want.items():
        rec[L.W_TYPE] = kind
        assert L.record_tensors(rec) == rw, kind
    rec[L.W_TYPE], rec[L.W_SRC], rec[L.W_RES] = L.OP_CONV, -1, 2
    assert L.record_tensors(rec) == ([2, 5], [4, 7])
