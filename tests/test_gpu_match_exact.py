"""GPU: the gallery match family to the bit -- fid_match, fid_match_keys + fid_match_merge, fid_gallery_topk, fid_cosine_matrix on every kernel path
(the 256 x 256 scan of csrc/match_gemm.hip, the register-staged 128 x 128 x 64 override and the LDS-DMA ring plans of csrc/match.hip / conv.hip),
and the rows fid_l2_normalize_f16* and fid_gallery_set_rows store.

The fixtures, the float64 reference, the dispatch mirror and the conditions the fixtures meet are tests/test_match_exact_cpu.py's: probe rows whose
cosines are exact multiples of 1/64 in any summation order, with exact copies planted on both sides of every 128- / 256-row seam, every workgroup-range
border of the scan, the shard borders and in the last real row.  Such rows tie all the time: "the first index of the maximum wins" and the strict
'>' against a threshold that a score attains decide most answers here.  All comparisons are bit for bit.  The large shapes are built from the
device's CU count, the smallest that reach each path; the largest allocation is the 256 x CUs-row gallery."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_range_join import gallery_rows, probe_rows, prototypes, unit_f16
from test_match_exact_cpu import (CF_ARGMAX, CF_OUT_F32, KS, NAN_QUERY, SMALL_DIMS, SMALL_GS, SMALL_NS, SLOT_COUNTS, SLOT_F, THRESHOLDS, build_queries,
                                  cosines, degenerate_rows, expected_path, f16_nan_row, klog_path, large_case, marker_row,
                                  normal_rows, normalise_rule, ref_cosine_matrix, ref_match, ref_topk, shard_bounds, small_case)

pytestmark = pytest.mark.gpu

CANARY = 0x7B
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    from scrfd_arcface_facerecognition_amd._lib import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cus(ctx):
    return int(re.search(r"\|cus=(\d+)", ctx.name()).group(1))


@pytest.fixture(scope="module")
def large(ctx, cus):
    """name -> (Gallery, fp32 rows, fp16 unit rows, info, Gp, dim, ns) of test_match_exact_cpu.large_shapes, each built once"""
    from scrfd_arcface_facerecognition_amd.engine import Gallery
    made = {}

    def get(name):
        if name not in made:
            g, info, Gp, dim, ns = large_case(name, cus)
            gal = Gallery(ctx, g)
            assert (gal.G, gal.Gp) == (len(g), Gp)
            made[name] = (gal, g, unit_f16(g), info, Gp, dim, ns)
        return made[name]
    yield get
    for entry in made.values():
        entry[0].close()


# ---- the entry points ------------------------------------------------------------------------------------------------------------------------------
def filled(ctx, shape, dtype):
    from scrfd_arcface_facerecognition_amd._lib import check
    b = ctx.empty(shape, dtype)
    check(ctx.lib.fid_memset(ctx.handle, C.c_void_p(b.ptr), CANARY, b.nbytes))
    return b


def run_match(ctx, gal, qd, n, thresh):
    idx, sc = filled(ctx, (n,), np.int32), filled(ctx, (n,), np.float32)
    gal.match_device(qd, n, thresh, idx, sc)
    return idx.download(), sc.download()


def run_topk(ctx, gal, qd, n, k, thresh):
    from scrfd_arcface_facerecognition_amd._lib import check
    idx, sc = filled(ctx, (n, k), np.int32), filled(ctx, (n, k), np.float32)
    check(ctx.lib.fid_gallery_topk(ctx.handle, gal.handle, C.c_void_p(qd.ptr), n, k, thresh, C.c_void_p(idx.ptr), C.c_void_p(sc.ptr)))
    return idx.download(), sc.download()


def run_cosine_matrix(ctx, gal, qd, n):
    from scrfd_arcface_facerecognition_amd._lib import check
    out = filled(ctx, (n, gal.Gp), np.float32)
    check(ctx.lib.fid_cosine_matrix(ctx.handle, gal.handle, C.c_void_p(qd.ptr), n, C.c_void_p(out.ptr)))
    return out.download()


def same(got, want):
    """indices equal, scores equal as floats"""
    return np.array_equal(got[0], want[0]) and got[1].dtype == np.float32 and np.array_equal(got[1], want[1])


def with_nan_query(q16):
    q16 = q16.copy()
    if len(q16) > NAN_QUERY:
        q16[NAN_QUERY] = f16_nan_row(q16.shape[1])
    return q16


def set_env(monkeypatch, env):
    for name in ("FID_NO_MATCH256", "FID_MATCH_DMA"):                              # (both are read per call)
        if name in env:
            monkeypatch.setenv(name, "1")
        else:
            monkeypatch.delenv(name, raising=False)


# ---- a. the generic GEMM plans on small galleries --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", SMALL_DIMS)
@pytest.mark.parametrize("G", SMALL_GS)
def test_small_galleries_every_entry_point(ctx, cus, G, dim):
    """Every (G, dim) of the list with n = 1, 17, 128, 129: one K-step (dim 32 and, at bk = 64, dim 64), three of 32 in a four-slot ring (dim 96), the
    96-wide column tile (G = 96, 288 at dim 32 / 96), 32- and 64-wide ones, a second query tile of one row, zero padding behind the last real row."""
    from scrfd_arcface_facerecognition_amd.engine import Gallery
    g, _, info = small_case(G, dim, 1)
    g16 = unit_f16(g)
    gal = Gallery(ctx, g)
    try:
        stored = gallery_rows(ctx, gal).download()
        assert np.array_equal(stored[:G], g16) and not stored[G:].view(np.uint16).any()
        for n in SMALL_NS:
            if cus > 3:
                assert expected_path(n, gal.Gp, dim, cus, CF_ARGMAX)[0] == expected_path(n, gal.Gp, dim, cus, CF_OUT_F32)[0] == "dma"
            q16 = unit_f16(build_queries(n, g, info, 10 * n + dim))
            S = cosines(q16, g16)
            qd = ctx.to_device(q16)
            assert np.array_equal(run_cosine_matrix(ctx, gal, qd, n), ref_cosine_matrix(S, gal.Gp)), n
            for k in KS:
                for thresh in (0.05, 0.75):
                    assert same(run_topk(ctx, gal, qd, n, k, thresh), ref_topk(S, k, thresh)), (n, k, thresh)
            qn = with_nan_query(q16)
            Sn, qd = cosines(qn, g16), ctx.to_device(qn)
            for thresh in THRESHOLDS:
                got, want = run_match(ctx, gal, qd, n, thresh), ref_match(Sn, thresh)
                assert same(got, want), (n, thresh, np.flatnonzero(got[0] != want[0])[:8])
            if n > NAN_QUERY:
                assert got[0][NAN_QUERY] == -1 and got[1][NAN_QUERY] == 0.0
    finally:
        gal.close()


# ---- b. the large-gallery paths --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["full64", "full96", "full512", "half64", "half96", "half512", "ragged_tile", "ragged_range"])
def test_large_gallery_argmax_paths(ctx, cus, large, monkeypatch, name):
    """n > 128: the 256 x 256 scan with one gallery tile per workgroup (dim 64 / 96: two / three K-steps, fewer than the loaders' prologue issues),
    a last tile of 32 real rows, a last workgroup range of one tile (each holding a query's only maximum and the lower row of a tie); n <= 128: the 128 x 128 x 64 override (dim 64: one K-step) or, at dim 96, the ring
    plan on a large gallery.  Every shape again with the scan and with the override switched off: same answers as the default and the reference."""
    gal, g, g16, info, Gp, dim, ns = large(name)
    for n in ns:
        default = expected_path(n, Gp, dim, cus, CF_ARGMAX)
        assert default == (("scan256",) if n > 128 else ("rs", 128, 128, 64) if dim % 64 == 0 else ("dma", 128, 128, 32))
        q16 = with_nan_query(unit_f16(build_queries(n, g, info, 10 * n + dim)))
        S = cosines(q16, g16)
        qd = ctx.to_device(q16)
        want = {t: ref_match(S, t) for t in THRESHOLDS}
        assert n == 1 or (want[0.0][0] >= info["tail"]).sum() >= 2                # answers only the last workgroup range (tile) can give
        envs = [{}, {"FID_NO_MATCH256": "1"}, {"FID_MATCH_DMA": "1"}] + ([{"FID_NO_MATCH256": "1", "FID_MATCH_DMA": "1"}] if n > 128 else [])
        for env in envs:
            set_env(monkeypatch, env)
            for t in THRESHOLDS:
                got = run_match(ctx, gal, qd, n, t)
                assert same(got, want[t]), (n, sorted(env), t, np.flatnonzero(got[0] != want[t][0])[:8])
            if n > NAN_QUERY:
                assert got[0][NAN_QUERY] == -1 and got[1][NAN_QUERY] == 0.0
        set_env(monkeypatch, {})


@pytest.mark.parametrize("name", ["full64", "full96", "full512"])
def test_large_gallery_score_matrix_and_topk(ctx, cus, large, monkeypatch, name):
    """the CF_OUT_F32 epilogue on the override (dim 64: a single K-step) and on the ring plan of a large gallery (dim 96, and FID_MATCH_DMA)"""
    gal, g, g16, info, Gp, dim, ns = large(name)
    assert expected_path(3, Gp, dim, cus, CF_OUT_F32) == (("rs", 128, 128, 64) if dim % 64 == 0 else ("dma", 128, 128, 32))
    assert np.array_equal(gallery_rows(ctx, gal).download()[:gal.G], g16)
    q16 = unit_f16(build_queries(5, g, info, 50 + dim))
    S = cosines(q16, g16)
    qd = ctx.to_device(q16)
    for env in ({}, {"FID_MATCH_DMA": "1"}):
        set_env(monkeypatch, env)
        assert np.array_equal(run_cosine_matrix(ctx, gal, qd, 3), ref_cosine_matrix(S[:3], Gp))
        for k in KS:
            for thresh in (0.05, 0.75):
                assert same(run_topk(ctx, gal, qd, 5, k, thresh), ref_topk(S, k, thresh)), (sorted(env), k, thresh)
    set_env(monkeypatch, {})


# ---- c. shards -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parts", [3, 8])
def test_sharded_keys_merge_equals_the_whole_scan(ctx, cus, large, parts):
    """fid_match_keys over contiguous shards whose borders are no multiple of 128 (first_row != 0), planted copies on both sides of every border;
    with three shards the first two take the scan and the last, 201 rows, the generic GEMM"""
    from scrfd_arcface_facerecognition_amd._lib import check
    from scrfd_arcface_facerecognition_amd.engine import Gallery
    gal, g, g16, info, Gp, dim, ns = large("full64")
    n, b = 257, shard_bounds(gal.G, parts)
    q16 = with_nan_query(unit_f16(build_queries(n, g, info, 10 * n + dim)))
    S = cosines(q16, g16)
    qd = ctx.to_device(q16)
    keys = filled(ctx, (parts, n), np.uint64)
    paths = []
    for r, (lo, hi) in enumerate(zip(b, b[1:])):
        shard = Gallery(ctx, g[lo:hi])
        paths.append(expected_path(n, shard.Gp, dim, cus, CF_ARGMAX)[0])
        check(ctx.lib.fid_match_keys(ctx.handle, shard.handle, C.c_void_p(qd.ptr), n, lo, C.c_void_p(keys.ptr + r * n * 8)))
        ctx.sync()
        shard.close()
    assert parts != 3 or paths == ["scan256", "scan256", "dma"]
    for t in THRESHOLDS:
        idx, sc = filled(ctx, (n,), np.int32), filled(ctx, (n,), np.float32)
        check(ctx.lib.fid_match_merge(ctx.handle, C.c_void_p(keys.ptr), parts, n, gal.G, t, C.c_void_p(idx.ptr), C.c_void_p(sc.ptr)))
        merged, want = (idx.download(), sc.download()), ref_match(S, t)
        assert same(merged, want), (t, np.flatnonzero(merged[0] != want[0])[:8])
        assert same(run_match(ctx, gal, qd, n, t), want)


# ---- d. the kernels the shapes above are about are the ones that run -----------------------------------------------------------------------------
CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from scrfd_arcface_facerecognition_amd._lib import Context
from scrfd_arcface_facerecognition_amd.engine import Gallery
ctx = Context(0)
print(ctx.name())
for name, n, G, dim in json.loads(sys.argv[2]):
    gal = Gallery(ctx, np.ones((G, dim), np.float32))
    q = ctx.to_device(np.zeros((n, dim), np.float16))
    idx, sc = ctx.empty((n,), np.int32), ctx.empty((n,), np.float32)
    ctx.sync()
    sys.stderr.write("[klog] case %s\n" % name)
    sys.stderr.flush()
    gal.match_device(q, n, 0.0, idx, sc)
    ctx.sync()
    gal.close()
ctx.close()
"""


def test_each_path_launches_the_kernel_the_mirror_names(cus):
    cases = [("scan", 129, 256 * cus - 31, 64), ("override", 128, 256 * cus - 31, 64), ("ring_large", 128, 256 * cus - 31, 96), ("ring_96wide", 17, 96, 32)]
    env = {k: v for k, v in os.environ.items() if k not in ("FID_NO_MATCH256", "FID_MATCH_DMA")}
    p = subprocess.run([sys.executable, "-c", CHILD, ROOT, json.dumps(cases)], env=dict(env, FID_KLOG="1"), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "|cus=%d" % cus in p.stdout
    seen, case = {}, None
    for line in p.stderr.splitlines():
        m = re.match(r"\[klog\] (case|kernel) (.*)", line)
        if m and m.group(1) == "case":
            case = m.group(2).strip()
        elif m and case and klog_path(m.group(2)):
            seen.setdefault(case, []).append(klog_path(m.group(2)))
    want = {name: [expected_path(n, (G + 31) // 32 * 32, dim, cus, CF_ARGMAX)] for name, n, G, dim in cases}
    assert seen == want
    assert [w[0][0] for w in want.values()] == ["scan256", "rs", "dma", "dma"] and want["override"][0] == ("rs", 128, 128, 64)


# ---- e. the rows fid_l2_normalize_f16* and fid_gallery_set_rows store ----------------------------------------------------------------------------
def normalise(ctx, x, counts=None, F=1, src=None, spare=3):
    """-> uint16 [n + spare, dim]: the n rows the call writes and `spare` canary rows behind them"""
    from scrfd_arcface_facerecognition_amd._lib import check
    n, dim = x.shape
    e, out = ctx.to_device(x), filled(ctx, (n + spare, dim), np.uint16)
    if counts is not None:
        c = ctx.to_device(np.asarray(counts, np.int32))
        check(ctx.lib.fid_l2_normalize_f16_slots(ctx.handle, C.c_void_p(e.ptr), n, dim, C.c_void_p(c.ptr), F, C.c_void_p(out.ptr)))
    elif src is not None:
        s = ctx.to_device(np.asarray(src, np.int32))
        check(ctx.lib.fid_l2_normalize_f16_packed(ctx.handle, C.c_void_p(e.ptr), n, dim, C.c_void_p(s.ptr), C.c_void_p(out.ptr)))
    else:
        check(ctx.lib.fid_l2_normalize_f16(ctx.handle, C.c_void_p(e.ptr), n, dim, C.c_void_p(out.ptr)))
    got = out.download()
    assert (got[n:] == CANARY * 0x0101).all()                                      # nothing behind the last row, whatever the block holds
    return got


def bits(x16):
    return np.ascontiguousarray(x16).view(np.uint16)


@pytest.mark.parametrize("dim", [32, 96, 500, 512])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023])
def test_l2_normalize_rows(ctx, n, dim):
    """probe rows to the bit, random normal rows by the rounding rule, the documented degenerate rows as all-+0.0 rows -- four rows per block, so
    n = 1, 3, 5, 1023 end inside one; dim 32 leaves half a wave idle, 96 and 500 end inside a pass of 64 lanes"""
    rng = np.random.default_rng(100 * n + dim)
    x = probe_rows(rng, n, dim, prototypes(rng, dim), {})
    assert np.array_equal(normalise(ctx, x)[:n], bits(unit_f16(x)))
    y = normal_rows(1023, dim)[:n]
    bad, excepted = normalise_rule(normalise(ctx, y)[:n].view(np.float16), y)
    assert bad == 0 and excepted < 0.01, (bad, excepted)
    h = n // 2
    got = normalise(ctx, np.concatenate([x[:h], degenerate_rows(dim), x[h:]]))     # the degenerate rows wherever in a block n puts them
    assert not got[h:h + 5].any()                                                  # 0x0000 everywhere: +0.0
    assert np.array_equal(np.concatenate([got[:h], got[h + 5:n + 5]]), bits(unit_f16(x)))


@pytest.mark.parametrize("dim", [32, 96, 500, 512])
def test_empty_slots_are_marker_rows_and_leave_their_neighbours_alone(ctx, dim):
    F, counts = SLOT_F, list(SLOT_COUNTS)                                          # 45 rows: the last block holds one
    n = F * len(counts)
    rng = np.random.default_rng(dim)
    x = probe_rows(rng, n, dim, prototypes(rng, dim), {})
    x[[2, 21, 44]] = degenerate_rows(dim)[[0, 1, 3]]                               # degenerate rows of DETECTED faces: +0.0 rows, not markers
    valid = np.concatenate([np.arange(F) < c for c in counts])
    assert valid[[2, 21]].all() and not valid[44] and valid.sum() == sum(counts)
    finite = x.copy()
    finite[[2, 21, 44]] = 0.0
    want = np.where(valid[:, None], bits(unit_f16(finite)), marker_row(dim)[None])
    assert not want[[2, 21]].any()
    assert (want[~valid, 0] == 0x8000).all() and not want[~valid, 1:].any()
    assert np.array_equal(normalise(ctx, x, counts=counts, F=F)[:n], want)
    y = normal_rows(n, dim)
    got = normalise(ctx, y, counts=counts, F=F)[:n]
    bad, excepted = normalise_rule(got[valid].view(np.float16), y[valid])
    assert bad == 0 and excepted < 0.01 and np.array_equal(got[~valid], want[~valid])
    src = np.where(valid, rng.integers(0, 1000, n), -1 - rng.integers(0, 5, n))    # packed table: only the sign of an entry says "no face"
    assert np.array_equal(normalise(ctx, x, src=src)[:n], want)
    for m in (1, 2, 3, 6, 7):                                                      # row counts that end inside a block; 6, 7: behind a marker
        assert np.array_equal(normalise(ctx, x[:m], src=src[:m])[:m], want[:m])


@pytest.mark.parametrize("dim", [32, 96, 512])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023])
def test_set_rows_stores_exact_rows(ctx, n, dim):
    from scrfd_arcface_facerecognition_amd._lib import c_i32_p, check
    from scrfd_arcface_facerecognition_amd.engine import Gallery
    G = 1100
    rng = np.random.default_rng(7 * n + dim)
    protos = prototypes(rng, dim)
    g0 = probe_rows(rng, G, dim, protos, {})
    gal = Gallery(ctx, g0)
    try:
        want = np.zeros((gal.Gp, dim), np.uint16)
        want[:G] = bits(unit_f16(g0))

        def upsert(rows, emb):
            rows, emb = np.ascontiguousarray(rows, np.int32), np.ascontiguousarray(emb, np.float32)
            check(ctx.lib.fid_gallery_set_rows(ctx.handle, gal.handle, rows.ctypes.data_as(c_i32_p), emb.ctypes.data_as(C.c_void_p), len(rows)))
            return gallery_rows(ctx, gal).download().view(np.uint16)
        rows = rng.permutation(G - 2)[:n] + 1
        rows[0], rows[-1] = G - 1, (0 if n > 1 else G - 1)                         # the last and the first real row among them
        x = probe_rows(rng, n, dim, protos, {})
        want[rows] = bits(unit_f16(x))
        assert np.array_equal(upsert(rows, x), want)                               # the new rows to the bit, every other row untouched
        y = normal_rows(1023, dim)[:n]
        got = upsert(rows, y)
        bad, excepted = normalise_rule(got[rows].view(np.float16), y)
        assert bad == 0 and excepted < 0.01, (bad, excepted)
        want[rows] = got[rows]
        assert np.array_equal(got, want)
        d = degenerate_rows(dim)[:min(n, 5)]
        want[rows[:len(d)]] = 0                                                    # zero / NaN / inf / overflowing / underflowing norm: a deleted row
        assert np.array_equal(upsert(rows[:len(d)], d), want)
    finally:
        gal.close()
