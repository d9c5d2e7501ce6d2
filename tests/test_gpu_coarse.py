"""GPU: the two-stage gallery search to the bit -- fid_quantize_rows_i8 / fid_gallery_quantize, fid_coarse_keys, fid_rerank_keys,
fid_gallery_search_coarse and VectorGallery.search(via="coarse") against tests/coarse_oracle.py.

The quantisation rule is integer arithmetic and power-of-two scaling, so codes, exponents and coarse keys are compared byte for byte on every
input, real-valued rows included.  Reranked scores are compared bit for bit where the fp32 sums are exact (the probe rows and the planted rows of
tests/test_coarse_cpu.py, which also asserts what the fixtures have to offer) and within the project's cosine tolerance on random rows.
The shortlist is per shard: a sharded search keeps up to parts * R candidates per query and may find more than the unsharded one, never fewer;
the oracle is run over the same shards."""
import ctypes as C

import numpy as np
import pytest

import coarse_oracle as O
from test_coarse_cpu import (SEARCH_KR, SEARCH_SHAPES, THRESHOLDS, TIE_ROWS, hand_rows, lane_probe, random_rows16, reorder_case, tie_case)
from test_gpu_range_join import gallery_rows, probe_rows, prototypes, unit_f16
from test_gpu_topk_fused import CANARY, canary_words, filled, run_search, set_slices, split
from test_match_exact_cpu import NAN_QUERY, cosines, f16_nan_row, ref_topk, small_case
from test_topk_fused_cpu import same

pytestmark = pytest.mark.gpu

FID_E_INVALID, FID_E_STATE = -1, -5
TOPK_MAX = 32


@pytest.fixture(scope="module")
def ctx():
    from scrfd_arcface_facerecognition_amd._lib import Context
    c = Context(0)
    yield c
    c.close()


def quantised(ctx, g):
    """a Gallery of the fp32 rows g with its int8 copy"""
    from scrfd_arcface_facerecognition_amd._lib import check
    from scrfd_arcface_facerecognition_amd.engine import Gallery
    gal = Gallery(ctx, g)
    check(ctx.lib.fid_gallery_quantize(ctx.handle, gal.handle))
    return gal


def quant_copy(ctx, gal):
    """-> (codes int8 [Gp, dim], exps int8 [Gp]) of the gallery's int8 copy"""
    from scrfd_arcface_facerecognition_amd._lib import check
    pc, pe = C.c_void_p(), C.c_void_p()
    check(ctx.lib.fid_gallery_quant_data(gal.handle, C.byref(pc), C.byref(pe)))
    return ctx.borrow(pc.value, (gal.Gp, gal.dim), np.int8).download(), ctx.borrow(pe.value, (gal.Gp,), np.int8).download()


def device_rows(ctx, gal):
    return gallery_rows(ctx, gal).download()[:gal.G]


def run_coarse_keys(ctx, gal, qd, n, R, first_row=0):
    from scrfd_arcface_facerecognition_amd._lib import check
    keys = filled(ctx, n * R * 8)
    check(ctx.lib.fid_coarse_keys(ctx.handle, gal.handle, C.c_void_p(qd.ptr), n, R, first_row, C.c_void_p(keys.ptr)))
    K, whole = split(keys, (n, R), np.uint64)
    assert whole, "bytes behind the keys were written"
    return K


def run_search_coarse(ctx, gal, qd, n, k, R, thresh):
    from scrfd_arcface_facerecognition_amd._lib import check
    idx, sc = filled(ctx, n * k * 4), filled(ctx, n * k * 4)
    check(ctx.lib.fid_gallery_search_coarse(ctx.handle, gal.handle, C.c_void_p(qd.ptr), n, k, R, thresh, C.c_void_p(idx.ptr), C.c_void_p(sc.ptr)))
    (i, gi), (s, gs) = split(idx, (n, k), np.int32), split(sc, (n, k), np.float32)
    assert gi and gs, "bytes behind an output were written"
    assert not (i == canary_words((n, k), np.int32)).any() and not (s.view(np.int32) == canary_words((n, k), np.int32)).any()     # every entry written
    return i, s


def bytes_equal(got, want):
    return got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()


# ---- a. the rule -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [64, 128, 512])
@pytest.mark.parametrize("G", [1, 33, 129, 300])
def test_quantise_equals_the_oracle(ctx, G, dim):
    from scrfd_arcface_facerecognition_amd._lib import check
    rng = np.random.default_rng(1000 * G + dim)
    x = rng.standard_normal((G, dim)).astype(np.float32) * np.float32(10.0) ** rng.integers(-3, 4, (G, 1)).astype(np.float32)
    if G > 2:
        x[2] = 0                                                                                  # a deleted row
    gal = quantised(ctx, x)
    try:
        rows16 = gallery_rows(ctx, gal).download()                                                # all Gp rows: the padding quantises to zeros too
        assert bytes_equal(quant_copy(ctx, gal), O.quantise(rows16))
        # the table entry point, on rows a gallery never holds: the hand-made rows, subnormal rows, NaN rows, rows up to fp16's largest value
        table = np.concatenate([np.stack(list(hand_rows(dim).values())), random_rows16(G, dim)])
        td = ctx.to_device(table)
        codes, exps = filled(ctx, table.size), filled(ctx, len(table))
        check(ctx.lib.fid_quantize_rows_i8(ctx.handle, C.c_void_p(td.ptr), len(table), dim, C.c_void_p(codes.ptr), C.c_void_p(exps.ptr)))
        (c, gc), (e, ge) = split(codes, table.shape, np.int8), split(exps, (len(table),), np.int8)
        assert gc and ge and bytes_equal((c, e), O.quantise(table))
        if G >= 33:                                                                               # upsert two rows, delete one: exactly those change
            before = quant_copy(ctx, gal)
            rows = np.array([G - 1, 0, 17], np.int32)
            emb = rng.standard_normal((3, dim)).astype(np.float32)
            emb[1] = 0
            check(ctx.lib.fid_gallery_set_rows(ctx.handle, gal.handle, rows.ctypes.data_as(C.POINTER(C.c_int32)), emb.ctypes.data_as(C.c_void_p), 3))
            after, want = quant_copy(ctx, gal), O.quantise(gallery_rows(ctx, gal).download())
            assert bytes_equal(after, want)
            changed = np.flatnonzero((after[0] != before[0]).any(1) | (after[1] != before[1]))
            assert sorted(changed.tolist()) == sorted(rows.tolist())
            assert not after[0][0].any() and after[1][0] == 0
            check(ctx.lib.fid_gallery_quantize(ctx.handle, gal.handle))                           # a second call refreshes: the same copy
            assert bytes_equal(quant_copy(ctx, gal), want)
    finally:
        gal.close()


def test_lane_map_probe(ctx):
    """gallery row i = e_i, query a = (17 a + j) / 512: key (a, i) carries the code of element i of query a.  A row / column swap or a wrong
    fragment index of the int8 MFMA puts another element there."""
    g, q16 = lane_probe()
    gal, qd = quantised(ctx, g), ctx.to_device(q16)
    try:
        g16 = device_rows(ctx, gal)
        assert np.array_equal(g16, g.astype(np.float16))
        for first_row in (0, 4096):
            got, want = run_coarse_keys(ctx, gal, qd, 16, 16, first_row), O.coarse_keys(q16, g16, 16, first_row)
            assert got.tobytes() == want.tobytes()
        rows, s = O.unpack(want)
        assert (want[1:] != 0).all() and (want[0] != 0).sum() == 15                               # every (query, row) but 0 x 0 has a key
        dot, S = O.coarse_scores(q16, g16)
        assert not np.array_equal(S, S.T) and len(np.unique(S)) > 100                             # asymmetric, and hardly two alike
    finally:
        gal.close()


# ---- b. the coarse keys ----------------------------------------------------------------------------------------------------------------------------
def keys_all_ways(ctx, monkeypatch, gal, q16, g16, Rs=(1, 5, 32)):
    """every R, first_row and slicing against the oracle (the coarse scores computed once)"""
    n = len(q16)
    qd = ctx.to_device(q16)
    scores = O.coarse_scores(q16, g16)
    for R in Rs:
        for first_row in (0, 4096):
            want = O.coarse_keys(q16, g16, R, first_row, scores)
            for s in ("1", "3"):
                set_slices(monkeypatch, s)
                got = run_coarse_keys(ctx, gal, qd, n, R, first_row)
                assert got.tobytes() == want.tobytes(), (n, R, first_row, s, np.flatnonzero((got != want).any(1))[:8])
    set_slices(monkeypatch, None)
    got = run_coarse_keys(ctx, gal, qd, n, Rs[-1])
    assert got.tobytes() == O.coarse_keys(q16, g16, Rs[-1], 0, scores).tobytes()                  # ... and the library's own choice of slices
    return got


@pytest.mark.parametrize("dim", [64, 512])
@pytest.mark.parametrize("G", [1, 127, 128, 129, 300, 1000])
def test_coarse_keys_equal_the_oracle(ctx, monkeypatch, G, dim):
    """the recall-1 fixture: one partly filled tile, a tile border with a planted pair, several tiles (so three slices cut for real), one K-step
    (dim 64) and eight; one query, 17, and two query tiles of which the second holds one row; a zero query and a NaN query"""
    g = small_case(G, dim, 129)[0]
    gal = quantised(ctx, g)
    try:
        g16 = device_rows(ctx, gal)
        assert np.array_equal(g16, unit_f16(g))
        for n in (1, 17, 129):
            q16 = unit_f16(small_case(G, dim, n)[1])
            if n > NAN_QUERY:
                q16[NAN_QUERY] = f16_nan_row(dim)
            K = keys_all_ways(ctx, monkeypatch, gal, q16, g16)
            if n > NAN_QUERY:
                assert not K[NAN_QUERY].any() and not K[2].any()                                  # the NaN query and the zero query: no candidate
    finally:
        gal.close()


def test_coarse_keys_on_the_reorder_and_tie_fixtures(ctx, monkeypatch):
    for R in (1, 5, 32):
        g, q, _ = reorder_case(R)
        gal = quantised(ctx, g)
        try:
            g16 = device_rows(ctx, gal)
            assert np.array_equal(g16, unit_f16(g))
            keys_all_ways(ctx, monkeypatch, gal, unit_f16(q), g16, Rs=(R,))
        finally:
            gal.close()
    g, q = tie_case()
    gal = quantised(ctx, g)
    try:
        g16 = device_rows(ctx, gal)
        K = keys_all_ways(ctx, monkeypatch, gal, unit_f16(q), g16)
        assert O.unpack(K)[0][0, :7].tolist() == list(TIE_ROWS)                                   # equal scores across tile and slice borders: lowest row first
    finally:
        gal.close()


# ---- c. the search ---------------------------------------------------------------------------------------------------------------------------------
def search_cases():
    for G, dim, n in SEARCH_SHAPES:
        g, q, _ = small_case(G, dim, n)
        yield "recall-1 %d x %d" % (G, dim), g, q, SEARCH_KR, True
    for R in (1, 5, 32):
        g, q, _ = reorder_case(R)
        yield "reorder R = %d" % R, g, q, ((R, R), (1, R)), False
    g, q = tie_case()
    yield "tie", g, q, SEARCH_KR, False


def test_search_coarse_equals_the_oracle(ctx):
    for name, g, q, krs, exact_too in search_cases():
        gal = quantised(ctx, g)
        try:
            g16, q16 = device_rows(ctx, gal), unit_f16(q)
            assert np.array_equal(g16, unit_f16(g))
            if len(q16) > NAN_QUERY:
                q16[NAN_QUERY] = f16_nan_row(q16.shape[1])
            qd, n = ctx.to_device(q16), len(q16)
            for k, R in krs:
                for thresh in THRESHOLDS:
                    got, want = run_search_coarse(ctx, gal, qd, n, k, R, thresh), O.search_coarse(q16, g16, k, R, thresh)
                    assert same(got, want), (name, k, R, thresh, np.flatnonzero((got[0] != want[0]).any(1))[:8])
                    if len(q16) > NAN_QUERY:
                        assert (got[0][NAN_QUERY] == -1).all() and not got[1][NAN_QUERY].view(np.uint32).any()
                    if exact_too:                                                                 # recall 1: the exact search's answer, bit for bit
                        assert same(got, run_search(ctx, gal, qd, n, k, thresh)), (name, k, R, thresh)
                        assert same(got, ref_topk(cosines(q16, g16), k, thresh))
            if name.startswith("reorder"):
                R = krs[0][1]
                assert not same(run_search_coarse(ctx, gal, qd, n, R, R, 0.0), run_search(ctx, gal, qd, n, R, 0.0))   # the rule, not the exact search
        finally:
            gal.close()


def test_invalid_arguments_leave_the_outputs_untouched(ctx):
    from scrfd_arcface_facerecognition_amd._lib import check
    from scrfd_arcface_facerecognition_amd.engine import Gallery
    g, q, _ = small_case(33, 64, 17)
    gal, qd = Gallery(ctx, g), ctx.to_device(unit_f16(q))
    g96 = Gallery(ctx, small_case(33, 96, 17)[0])
    q96 = ctx.to_device(unit_f16(small_case(33, 96, 17)[1]))
    idx, sc, keys, keys2 = filled(ctx, 17 * 33 * 4), filled(ctx, 17 * 33 * 4), filled(ctx, 17 * 33 * 8), filled(ctx, 17 * 33 * 8)
    lib, h = ctx.lib, ctx.handle
    p = lambda b: C.c_void_p(b.ptr)
    try:
        # no quantised copy yet
        assert lib.fid_gallery_search_coarse(h, gal.handle, p(qd), 17, 5, 16, 0.05, p(idx), p(sc)) == FID_E_STATE
        assert lib.fid_coarse_keys(h, gal.handle, p(qd), 17, 5, 0, p(keys)) == FID_E_STATE
        pc, pe = C.c_void_p(), C.c_void_p()
        assert lib.fid_gallery_quant_data(gal.handle, C.byref(pc), C.byref(pe)) == FID_E_STATE
        assert lib.fid_gallery_quantize(h, g96.handle) == FID_E_INVALID and lib.fid_gallery_quantize(h, None) == FID_E_INVALID
        check(lib.fid_gallery_quantize(h, gal.handle))
        nan = float("nan")
        bad = [lib.fid_gallery_search_coarse(h, gal.handle, p(qd), 17, 6, 5, 0.05, p(idx), p(sc)),                  # k > R
               lib.fid_gallery_search_coarse(h, gal.handle, p(qd), 17, 5, TOPK_MAX + 1, 0.05, p(idx), p(sc)),
               lib.fid_gallery_search_coarse(h, gal.handle, p(qd), 17, 0, 5, 0.05, p(idx), p(sc)),
               lib.fid_gallery_search_coarse(h, g96.handle, p(q96), 17, 5, 16, 0.05, p(idx), p(sc)),                # dim 96
               lib.fid_gallery_search_coarse(h, gal.handle, p(qd), 17, 5, 16, nan, p(idx), p(sc)),
               lib.fid_gallery_search_coarse(h, gal.handle, None, 17, 5, 16, 0.05, p(idx), p(sc)),
               lib.fid_gallery_search_coarse(h, None, p(qd), 17, 5, 16, 0.05, p(idx), p(sc)),
               lib.fid_gallery_search_coarse(h, gal.handle, p(qd), 17, 5, 16, 0.05, None, p(sc)),
               lib.fid_gallery_search_coarse(h, gal.handle, p(qd), 17, 5, 16, 0.05, p(idx), None),
               lib.fid_gallery_search_coarse(h, gal.handle, p(qd), 0, 5, 16, 0.05, p(idx), p(sc)),
               lib.fid_gallery_search_coarse(h, gal.handle, p(qd), -1, 5, 16, 0.05, p(idx), p(sc)),
               lib.fid_coarse_keys(h, gal.handle, p(qd), 17, 0, 0, p(keys)),
               lib.fid_coarse_keys(h, gal.handle, p(qd), 17, TOPK_MAX + 1, 0, p(keys)),
               lib.fid_coarse_keys(h, gal.handle, p(qd), 0, 5, 0, p(keys)),
               lib.fid_coarse_keys(h, gal.handle, p(qd), 17, 5, -1, p(keys)),
               lib.fid_coarse_keys(h, gal.handle, p(qd), 17, 5, 2 ** 31 - 40, p(keys)),
               lib.fid_coarse_keys(h, g96.handle, p(q96), 17, 5, 0, p(keys)),
               lib.fid_coarse_keys(h, gal.handle, None, 17, 5, 0, p(keys)),
               lib.fid_coarse_keys(h, gal.handle, p(qd), 17, 5, 0, None),
               lib.fid_rerank_keys(h, gal.handle, p(qd), 17, 0, 0, p(keys), p(keys2)),
               lib.fid_rerank_keys(h, gal.handle, p(qd), 17, TOPK_MAX + 1, 0, p(keys), p(keys2)),
               lib.fid_rerank_keys(h, gal.handle, p(qd), 0, 5, 0, p(keys), p(keys2)),
               lib.fid_rerank_keys(h, gal.handle, p(qd), 17, 5, -1, p(keys), p(keys2)),
               lib.fid_rerank_keys(h, gal.handle, p(qd), 17, 5, 0, p(keys), p(keys)),                                # in place
               lib.fid_rerank_keys(h, gal.handle, p(qd), 17, 5, 0, None, p(keys2)),
               lib.fid_rerank_keys(h, gal.handle, p(qd), 17, 5, 0, p(keys), None),
               lib.fid_quantize_rows_i8(h, p(q96), 17, 96, p(keys), p(keys2)),
               lib.fid_quantize_rows_i8(h, p(qd), 0, 64, p(keys), p(keys2)),
               lib.fid_quantize_rows_i8(h, None, 17, 64, p(keys), p(keys2))]
        assert bad == [FID_E_INVALID] * len(bad), bad
        ctx.sync()
        for b in (idx, sc, keys, keys2):
            assert (b.download() == CANARY).all()
    finally:
        gal.close()
        g96.close()


# ---- d. shards -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bounds", [[0, 437, 1000], [0, 301, 650, 1000]])
def test_sharded_coarse_rerank_merge(ctx, bounds):
    """per shard fid_coarse_keys + fid_rerank_keys with the shard's first row, one fid_topk_merge over [parts, n, R].  The shortlist is per shard:
    up to parts * R candidates per query, so the oracle is run over the same shards (on the recall-1 gallery both equal the exact search)."""
    from scrfd_arcface_facerecognition_amd._lib import check
    parts, n, G = len(bounds) - 1, 129, 1000
    for fixture in ("recall-1", "tie"):
        g, q = small_case(G, 64, n)[:2] if fixture == "recall-1" else tie_case(G, 64, n)
        g16, q16 = unit_f16(g), unit_f16(q)
        q16[NAN_QUERY] = f16_nan_row(64)
        qd = ctx.to_device(q16)
        shards = [quantised(ctx, g[lo:hi]) for lo, hi in zip(bounds, bounds[1:])]
        try:
            for k, R in ((5, 5), (5, 16)):
                coarse, exact = filled(ctx, parts * n * R * 8), filled(ctx, parts * n * R * 8)
                for r, shard in enumerate(shards):
                    off = r * n * R * 8
                    check(ctx.lib.fid_coarse_keys(ctx.handle, shard.handle, C.c_void_p(qd.ptr), n, R, bounds[r], C.c_void_p(coarse.ptr + off)))
                    check(ctx.lib.fid_rerank_keys(ctx.handle, shard.handle, C.c_void_p(qd.ptr), n, R, bounds[r], C.c_void_p(coarse.ptr + off),
                                                  C.c_void_p(exact.ptr + off)))
                (Kc, gc), (Ke, ge) = split(coarse, (parts, n, R), np.uint64), split(exact, (parts, n, R), np.uint64)
                assert gc and ge
                for r, (lo, hi) in enumerate(zip(bounds, bounds[1:])):
                    want_c = O.coarse_keys(q16, g16[lo:hi], R, lo)
                    assert Kc[r].tobytes() == want_c.tobytes() and Ke[r].tobytes() == O.rerank(q16, g16[lo:hi], want_c, lo).tobytes(), (fixture, r)
                assert (Ke[:, :, :-1] >= Ke[:, :, 1:]).all() and not Ke[:, NAN_QUERY].any()       # descending; the NaN query has no candidate
                for thresh in (0.0, 0.75):                                                        # the merge takes [parts, n, R] at k = R
                    idx, sc = filled(ctx, n * R * 4), filled(ctx, n * R * 4)
                    check(ctx.lib.fid_topk_merge(ctx.handle, C.c_void_p(exact.ptr), parts, n, R, G, thresh, C.c_void_p(idx.ptr), C.c_void_p(sc.ptr)))
                    (i, gi), (s, gs) = split(idx, (n, R), np.int32), split(sc, (n, R), np.float32)
                    assert gi and gs and same((i, s), O.search_coarse(q16, g16, R, R, thresh, bounds)), (fixture, R, thresh)
                    want_k = O.search_coarse(q16, g16, k, R, thresh, bounds)
                    assert same((i[:, :k], s[:, :k]), want_k)                                     # ... and its first k columns are the best k
                    if fixture == "recall-1":
                        assert same(want_k, ref_topk(cosines(q16, g16), k, thresh))
        finally:
            for shard in shards:
                shard.close()


# ---- e. real-valued rows ---------------------------------------------------------------------------------------------------------------------------
def test_random_rows_keys_to_the_bit_scores_within_the_cosine_tolerance(ctx):
    """64 random normal queries x 5 000 random rows, dim 512, k = 10, R = 32.  The coarse keys still equal the oracle bit for bit: that is the
    point of the rule.  The reported scores are fp32 sums of fp16 products; 1e-3 is the project's stated cosine tolerance."""
    from scrfd_arcface_facerecognition_amd._lib import check
    rng = np.random.default_rng(2024)
    n, G, dim, k, R = 64, 5000, 512, 10, 32
    gal = quantised(ctx, rng.standard_normal((G, dim)).astype(np.float32))
    try:
        e = ctx.to_device(rng.standard_normal((n, dim)).astype(np.float32))
        qd = ctx.empty((n, dim), np.float16)
        check(ctx.lib.fid_l2_normalize_f16(ctx.handle, C.c_void_p(e.ptr), n, dim, C.c_void_p(qd.ptr)))
        q16, g16 = qd.download(), device_rows(ctx, gal)
        want_keys = O.coarse_keys(q16, g16, R)
        assert run_coarse_keys(ctx, gal, qd, n, R).tobytes() == want_keys.tobytes()
        ref = q16.astype(np.float64) @ g16.astype(np.float64).T
        idx, sc = run_search_coarse(ctx, gal, qd, n, k, R, 0.0)
        short = O.unpack(want_keys)[0]
        assert (idx >= 0).all() and all(set(idx[r].tolist()) <= set(short[r].tolist()) for r in range(n))
        err = np.abs(sc.astype(np.float64) - np.take_along_axis(ref, idx.astype(np.int64), 1)).max()
        print("max |score - float64| = %.3g" % err)
        assert err <= 1e-3 and (np.diff(sc, axis=1) <= 0).all()
        fi, fs = run_search(ctx, gal, qd, n, k, 0.0)
        exact = {(r, int(j)): fs[r, c] for r in range(n) for c, j in enumerate(fi[r]) if j >= 0}
        both = [(sc[r, c], exact[(r, int(j))]) for r in range(n) for c, j in enumerate(idx[r]) if (r, int(j)) in exact]
        diff = max(abs(float(a) - float(b)) for a, b in both)
        recall = len(both) / float((fi >= 0).sum())
        print("pairs reported by both searches: %d, largest |coarse-path score - fid_gallery_search score| = %.3g, recall@%d = %.4f"
              % (len(both), diff, k, recall))
        assert diff <= 1e-3
    finally:
        gal.close()


# ---- f. Python -------------------------------------------------------------------------------------------------------------------------------------
def test_vector_gallery_search_via_coarse(ctx):
    """the 300-row probe store of test_vector_gallery_search_any_k: via="coarse" equals via="fused", and stays equal after a delete of a hit, an
    upsert of a new best row and a growth of the store"""
    from scrfd_arcface_facerecognition_amd.engine import VectorGallery
    rng = np.random.default_rng(9)
    G, dim = 300, 64
    emb = probe_rows(rng, G, dim, prototypes(rng, dim), {})
    ids = ["p%d" % i for i in range(G)]
    vg = VectorGallery(ctx, dim=dim, capacity=G)
    vg.upsert(ids, emb)
    q = emb[[7, 130, 299, 12]]
    for k, rerank in ((5, 32), (3, 3), (32, 32), (1, 8)):
        assert vg.search(q, k=k, via="coarse", rerank=rerank) == vg.search(q, k=k, via="fused"), (k, rerank)
    assert vg.search(q, k=10, score_threshold=0.5, via="coarse") == vg.search(q, k=10, score_threshold=0.5, via="fused")
    assert vg._gal._quant is True
    with pytest.raises(ValueError):
        vg.search(q, k=5, via="coarse", rerank=4)
    with pytest.raises(ValueError):
        vg.search(q, k=5, via="coarse", rerank=33)
    best = vg.search(q[:1], k=3, via="coarse")[0][0][0]
    vg.delete([best])                                                                             # a hit goes
    after = vg.search(q, k=5, via="coarse")
    assert best not in [i for i, _ in after[0]] and after == vg.search(q, k=5, via="fused")
    vg.upsert(["new"], q[1:2])                                                                    # a new best row (a copy of query 1) takes the freed row
    after = vg.search(q, k=5, via="coarse")
    assert "new" in [i for i, _ in after[1][:2]] and after == vg.search(q, k=5, via="fused")
    vg.upsert(["grown"], q[2:3])                                                                  # no free row left: the store grows
    assert vg._gal.G == 2 * G and vg._gal._quant is True
    after = vg.search(q, k=5, via="coarse")
    assert "grown" in [i for i, _ in after[2][:2]] and after == vg.search(q, k=5, via="fused")
    merges = vg.find_and_merge_duplicates(0.8, via="device")                                      # rows cleared on the device: the copy is stale ...
    assert merges and vg._gal._quant is False
    after = vg.search(q, k=5, via="coarse")                                                       # ... and rebuilt by the next coarse search
    assert vg._gal._quant is True and after == vg.search(q, k=5, via="fused")
    gone = {dead for _, dead, _ in merges}
    assert not gone & {i for row in after for i, _ in row}
    assert vg.search(q, k=5) == vg.search(q, k=5, via="matrix")                                   # via=None still chooses what it chose
