"""CPU: the host half of the two-stage gallery search (tests/test_gpu_coarse.py runs the device half) -- the quantisation rule on hand-made rows,
the host twin fid_quantize_rows_i8_host and a sanitized stand-alone build of csrc/quant_core.h against the numpy oracle (tests/coarse_oracle.py),
and the fixtures of the device tests with the conditions that keep those tests from passing vacuously.

Fixtures:
  recall-1   the probe galleries of tests/test_match_exact_cpu.py: unit rows of +-0.5, +-0.25, +-0.125 quantise without error, so the coarse order
             IS the exact order, ties included, and the two-stage search must return the exact search's answer for every k <= R.
  reorder    rows of small integers whose squares sum to 256^2 (the norm is a power of two, so the unit fp16 rows are exact and known here).  Against
             the query e_0: row A = (23, 127 x 4, 22, 1 x 7) / 256 lies on the grid 2^-8 and keeps its 23/256; row B = (22, 255, 1 x 27) / 256 has the
             grid 2^-6, where 22/256 = 5.5 steps rounds (to even) to 6 = 24/256.  Exact: A > B.  Coarse: B > A.  R - 1 rows at exactly 0.5 fill the
             shortlist, so its last place goes to B and the exact search's k-th answer, A, is missed: a device that ran the exact search fails.
  tie        copies of one such row on both sides of the 128-row tile borders and of the borders of three slices (rows 384 and 768 of 1 000)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import coarse_oracle as O
from test_gpu_range_join import probe_rows, prototypes, unit_f16
from test_match_exact_cpu import BELOW, cosines, ref_topk, small_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("clang++")

ROW_A = [23, 127, 127, 127, 127, 22] + [1] * 7
ROW_B = [22, 255] + [1] * 27
SEARCH_SHAPES = ((129, 64, 17), (300, 64, 129), (1000, 512, 17))            # (G, dim, n) of the recall-1 searches on the device
SEARCH_KR = ((1, 1), (5, 5), (5, 32), (10, 16), (32, 32))
THRESHOLDS = (0.0, 0.75, BELOW)
TIE_ROWS = (127, 128, 383, 384, 767, 768, 999)


def f16(bits):
    return np.asarray(bits, np.uint16).view(np.float16)


def planted(values, dim, cols=None):
    r = np.zeros(dim, np.float32)
    r[np.arange(len(values)) if cols is None else cols[:len(values)]] = values
    assert float((r.astype(np.float64) ** 2).sum()) == 65536.0
    return r


def reorder_case(R, G=300, dim=64, n=17):
    """-> (gallery fp32 [G, dim], queries fp32 [n, dim], (row of A, row of B)); see the module docstring"""
    rng = np.random.default_rng(100 * R + dim)
    protos = prototypes(rng, dim)
    g = probe_rows(rng, G, dim, protos, {})
    g[g[:, 0] > 0] *= -1                                                     # no other row is positive against e_0
    rows = rng.permutation(G)[:R + 1]
    a, b = int(rows[0]), int(rows[1])
    g[a], g[b] = planted(ROW_A, dim), planted(ROW_B, dim)
    for r in rows[2:]:
        g[r] = 0
        g[r, [0, 7, 19, 33]] = [1, -1, 1, -1]                                # 0.5 against e_0, coarse and exact
    q = probe_rows(rng, n, dim, protos, {})
    q[0] = 0
    q[0, 0] = 1.0
    if n > 4:
        q[1], q[2], q[3], q[4] = g[a], g[b], -q[0], 0
    return g, q, (a, b)


def tie_case(G=1000, dim=64, n=17):
    """-> (gallery, queries): query 0 copies the row planted at TIE_ROWS, query 1 the one planted at rows 255 | 256"""
    rng = np.random.default_rng(77)
    protos = prototypes(rng, dim)
    g = probe_rows(rng, G, dim, protos, {})
    cols = rng.permutation(dim)
    t = planted(np.array(ROW_A) * rng.choice([-1, 1], len(ROW_A)), dim, cols)
    u = planted(np.array(ROW_B) * rng.choice([-1, 1], len(ROW_B)), dim, cols[::-1])
    g[list(TIE_ROWS)] = t
    g[[255, 256]] = u
    q = probe_rows(rng, n, dim, protos, {})
    q[0], q[1] = t, u
    if n > 3:
        q[2], q[3] = -t, 0
    return g, q


def lane_probe():
    """-> (gallery fp32 [16, 64] = e_i, queries fp16 [16, 64] = (17 a + j) / 512): asymmetric, so a row / column slip of the fragments shows"""
    q = (17 * np.arange(16)[:, None] + np.arange(64)[None, :]) / 512.0
    assert np.array_equal(q.astype(np.float16).astype(np.float64), q)
    return np.eye(16, 64, dtype=np.float32), q.astype(np.float16)


def hand_rows(dim=64):
    """name -> fp16 row [dim]"""
    def row(vals):
        r = np.zeros(dim, np.float16)
        r[:len(vals)] = vals
        return r
    edge = np.float16(127.0 / 128.0)
    above = np.nextafter(edge, np.float16(2.0))
    sub = f16([1, 2, 3, 126, 127, 0x8005, 0x8001]).tolist()                                       # fp16 subnormals: multiples of 2^-24
    marker = np.zeros(dim, np.uint16)
    marker[0] = 0x8000
    return {"edge": row([edge, 0.25, -edge]), "above": row([above, 0.25, -0.25]), "small_edge": row([127 * 2.0 ** -20, 2.0 ** -20]),
            "ties": row([1.0] + [x / 64.0 for x in (0.5, 1.5, 2.5, 3.5, -0.5, -1.5, -2.5, 126.5)]), "subnormal": row(sub),
            "zero": row([]), "nan": row([0.5, np.nan]), "inf": row([0.5, -np.inf]), "marker": marker.view(np.float16), "largest": row([65504.0, 1024.0, 511.0])}


def host_twin(rows16):
    from scrfd_arcface_facerecognition_amd import _lib
    lib = _lib.load()
    rows16 = np.ascontiguousarray(rows16, np.float16)
    n, dim = rows16.shape
    codes, exps = np.full((n, dim), 99, np.int8), np.full(n, 99, np.int8)
    rc = lib.fid_quantize_rows_i8_host(rows16.ctypes.data_as(C.c_void_p), n, dim, codes.ctypes.data_as(C.c_void_p), exps.ctypes.data_as(C.c_void_p))
    assert rc == 0
    return codes, exps


def random_rows16(n=1000, dim=128):
    rng = np.random.default_rng(5)
    x = rng.standard_normal((n, dim)) * 10.0 ** rng.uniform(-7, 4, (n, 1))                        # subnormal rows to rows near fp16's largest
    x[::50, 3] = np.nan
    x[7::50] = 0
    return np.clip(x, -65504, 65504).astype(np.float16)


# ---- the rule --------------------------------------------------------------------------------------------------------------------------------------
def test_rule_on_hand_made_rows():
    rows = hand_rows()
    codes, exps = O.quantise(np.stack(list(rows.values())))
    got = {name: (codes[i], int(exps[i])) for i, name in enumerate(rows)}
    assert got["edge"][1] == -7 and got["edge"][0][:3].tolist() == [127, 32, -127]               # m = 127 * 2^-7 exactly: still e = -7
    assert got["above"][1] == -6 and got["above"][0][:3].tolist() == [64, 16, -16]               # one ulp above: e steps, 63.53 rounds to 64
    assert got["small_edge"][1] == -20 and got["small_edge"][0][:2].tolist() == [127, 1]
    assert got["ties"][1] == -6 and got["ties"][0][:9].tolist() == [64, 0, 2, 2, 4, 0, -2, -2, 126]   # x.5 goes to the even neighbour
    assert got["subnormal"][1] == -24 and got["subnormal"][0][:7].tolist() == [1, 2, 3, 126, 127, -5, -1]
    assert got["largest"][1] == 10 and got["largest"][0][:3].tolist() == [64, 1, 0]              # 65504 / 1024 = 63.97; 511 / 1024 = 0.499
    for name in ("zero", "nan", "inf", "marker"):
        assert got[name][1] == 0 and not got[name][0].any(), name
    d, s = O.coarse_scores(np.stack([rows["edge"], rows["nan"]]), np.stack([rows["edge"], rows["above"], rows["zero"]]))
    assert d.tolist() == [[2 * 127 * 127 + 32 * 32, 127 * 64 + 32 * 16 + 127 * 16, 0], [0, 0, 0]]
    assert s[0, 0] == np.float32(33282 / 16384.0) and s[0, 1] == np.float32(10672 / 8192.0)


def test_host_twin_equals_the_oracle():
    for rows in (np.stack(list(hand_rows().values())), np.stack(list(hand_rows(512).values())), random_rows16()):
        want, got = O.quantise(rows), host_twin(rows)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    r = random_rows16()
    assert (np.abs(r.astype(np.float64)).max(1) < 2.0 ** -14).any() and (np.abs(np.nan_to_num(r.astype(np.float64))).max(1) > 1024).any()
    from scrfd_arcface_facerecognition_amd import _lib
    lib = _lib.load()
    buf = np.zeros((2, 96), np.int8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.fid_quantize_rows_i8_host(p(np.zeros((2, 96), np.float16)), 2, 96, p(buf), p(buf)) == -1          # dim % 64
    assert lib.fid_quantize_rows_i8_host(p(np.zeros((2, 64), np.float16)), 0, 64, p(buf), p(buf)) == -1
    assert lib.fid_quantize_rows_i8_host(None, 2, 64, p(buf), p(buf)) == -1


def test_host_rule_under_the_sanitizers(tmp_path):
    """tests/quant_host_driver.cpp includes only csrc/quant_core.h; every row, code row and exponent is a heap allocation of its exact size"""
    if CXX is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "quant_host_driver"
    subprocess.run([CXX, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "scrfd_arcface_facerecognition_amd", "csrc"), os.path.join(ROOT, "tests", "quant_host_driver.cpp"),
                    "-o", str(exe)], check=True)
    for k, rows in enumerate((np.stack(list(hand_rows().values())), random_rows16(200, 64), random_rows16(50, 1024))):
        case, dst = tmp_path / ("case%d.bin" % k), tmp_path / ("out%d.bin" % k)
        with open(case, "wb") as f:
            f.write(np.array(rows.shape, np.int32).tobytes())
            f.write(rows.tobytes())
        p = subprocess.run([str(exe), str(case), str(dst)], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-2000:]
        assert int(p.stdout) == len(rows)
        raw = np.frombuffer(open(dst, "rb").read(), np.int8)
        codes, exps = O.quantise(rows)
        assert raw.size == rows.size + len(rows)
        assert raw[:rows.size].tobytes() == codes.tobytes() and raw[rows.size:].tobytes() == exps.tobytes()


# ---- the fixtures' conditions -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,dim,n", SEARCH_SHAPES)
def test_recall_1_fixture_coarse_equals_exact(G, dim, n):
    g, q, _ = small_case(G, dim, n)
    g16, q16 = unit_f16(g), unit_f16(q)
    S = cosines(q16, g16)
    assert np.array_equal(O.coarse_scores(q16, g16)[1], S.astype(np.float32))                    # probe rows quantise without error
    for k, R in SEARCH_KR:
        for thresh in THRESHOLDS:
            got, want = O.search_coarse(q16, g16, k, R, thresh), ref_topk(S, k, thresh)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (k, R, thresh)


@pytest.mark.parametrize("R", [1, 5, 32])
def test_reorder_fixture_coarse_differs_from_exact(R):
    g, q, (a, b) = reorder_case(R)
    g16, q16 = unit_f16(g), unit_f16(q)
    assert np.array_equal(g16[[a, b]].astype(np.float64) * 256, g[[a, b]])                       # the planted unit rows are exact
    S = cosines(q16, g16)
    C_ = O.coarse_scores(q16, g16)[1]
    assert (S[0] > 0).sum() == R + 1 > R                                                          # more positive rows than the shortlist holds
    assert S[0, a] == 23 / 256 > S[0, b] == 22 / 256 and C_[0, a] == np.float32(23 / 256) < C_[0, b] == np.float32(24 / 256)
    got, want = O.search_coarse(q16, g16, R, R, 0.0), ref_topk(S, R, 0.0)
    assert got[0][0, -1] == b and got[1][0, -1] == np.float32(22 / 256) and want[0][0, -1] == a   # the shortlist's last place: B, at its exact score
    assert not np.array_equal(got[0], want[0])
    assert np.array_equal(got[0][0, :-1], want[0][0, :-1])


def test_tie_fixture_lowest_row_first():
    g, q = tie_case()
    g16, q16 = unit_f16(g), unit_f16(q)
    scores = O.coarse_scores(q16, g16)
    assert (scores[1][0, list(TIE_ROWS)] == 1.0).all() and (np.delete(scores[1][0], list(TIE_ROWS)) < 1.0).all()
    for R in (1, 5, 32):
        rows, s = O.unpack(O.coarse_keys(q16, g16, R, 4096, scores))
        assert rows[0, :min(R, 7)].tolist() == [4096 + r for r in TIE_ROWS[:R]] and (s[0, :min(R, 7)] == 1.0).all()
        assert rows[1, :min(R, 2)].tolist() == [4096 + 255, 4096 + 256][:R]
    assert 127 // 128 != 128 // 128 and 383 // 384 != 384 // 384 and 767 // 384 != 768 // 384      # a tile border, the borders of three slices
    K = O.coarse_keys(q16, g16, 32, 0, scores)
    assert not K[2].any() or O.unpack(K[2:3])[1].max() < 1.0
    assert not K[3].any()                                                                         # the zero query has no candidate


def test_a_full_shortlist_is_the_exact_search():
    """R >= the number of rows with dot > 0: nothing is cut, so the rerank restores the exact order"""
    rng = np.random.default_rng(3)
    g16, q16 = unit_f16(rng.standard_normal((20, 64))), unit_f16(rng.standard_normal((6, 64)))
    dot, _ = O.coarse_scores(q16, g16)
    assert (dot > 0).sum(1).max() <= 20
    S = (q16.astype(np.float64) @ g16.astype(np.float64).T).astype(np.float32)
    assert ((S > 0.02) == (dot > 0))[np.abs(S) > 0.02].all()
    got, want = O.search_coarse(q16, g16, 5, 20, 0.02), ref_topk(S, 5, 0.02)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    cut = O.search_coarse(q16, g16, 5, 5, 0.02)
    assert (cut[0] >= -1).all() and set(cut[0][cut[0] >= 0].tolist()) <= set(range(20))


def test_sharded_oracle_never_finds_fewer():
    g, q, _ = small_case(1000, 64, 17)
    g16, q16 = unit_f16(g), unit_f16(q)
    S = cosines(q16, g16)
    for bounds in ([0, 437, 1000], [0, 301, 650, 1000]):
        got, want = O.search_coarse(q16, g16, 5, 5, 0.0, bounds), ref_topk(S, 5, 0.0)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
