"""GPU: the fused top-k search to the bit -- fid_gallery_search for any k up to 32, fid_topk_keys + fid_topk_merge over row shards, and
VectorGallery.search on top of them.

Fixtures, reference and the conditions they meet are tests/test_match_exact_cpu.py's and tests/test_topk_fused_cpu.py's: probe rows whose cosines
are exact multiples of 1/64 in any summation order and which tie all the time, so indices and fp32 scores are compared bit for bit and the
"lowest row among equal scores" rule decides most lists.  Every search runs with the number of gallery slices forced to 1, to 3 and left to the
library: the answer must not depend on how the scan is cut."""
import ctypes as C
import re
import types

import numpy as np
import pytest

from test_gpu_range_join import probe_rows, prototypes, unit_f16
from test_match_exact_cpu import NAN_QUERY, ZERO_ROW, build_queries, cosines, f16_nan_row, large_case, ref_topk, shard_bounds, small_case
from test_topk_fused_cpu import KS, SHAPES, same, unpack

pytestmark = pytest.mark.gpu

CANARY = 0x7B
GUARD = 64                                          # bytes behind every output that must stay untouched
OLD_KS = (1, 2, 4, 5, 8)                            # what fid_gallery_topk serves
FID_E_INVALID = -1
SLICES = ("1", "3", None)


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
    """name -> (Gallery, fp32 rows, fp16 unit rows, info, dim), each built once"""
    from scrfd_arcface_facerecognition_amd.engine import Gallery
    made = {}

    def get(name):
        if name not in made:
            g, info, Gp, dim, _ = large_case(name, cus)
            gal = Gallery(ctx, g)
            assert (gal.G, gal.Gp) == (len(g), Gp)
            made[name] = (gal, g, unit_f16(g), info, dim)
        return made[name]
    yield get
    for entry in made.values():
        entry[0].close()


def filled(ctx, nbytes):
    """a byte buffer of nbytes + GUARD canary bytes"""
    from scrfd_arcface_facerecognition_amd._lib import check
    b = ctx.empty((nbytes + GUARD,), np.uint8)
    check(ctx.lib.fid_memset(ctx.handle, C.c_void_p(b.ptr), CANARY, b.nbytes))
    return b


def split(buf, shape, dtype):
    """-> (the array, True if the guard bytes behind it are whole)"""
    raw = buf.download()
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    return raw[:n].view(dtype).reshape(shape), bool((raw[n:] == CANARY).all())


def set_slices(monkeypatch, s):
    if s is None:
        monkeypatch.delenv("FID_TOPK_SLICES", raising=False)
    else:
        monkeypatch.setenv("FID_TOPK_SLICES", s)                                    # (read per call)


def run_search(ctx, gal, qd, n, k, thresh):
    from scrfd_arcface_facerecognition_amd._lib import check
    idx, sc = filled(ctx, n * k * 4), filled(ctx, n * k * 4)
    check(ctx.lib.fid_gallery_search(ctx.handle, gal.handle, C.c_void_p(qd.ptr), n, k, thresh, C.c_void_p(idx.ptr), C.c_void_p(sc.ptr)))
    (i, gi), (s, gs) = split(idx, (n, k), np.int32), split(sc, (n, k), np.float32)
    assert gi and gs, "bytes behind an output were written"
    return i, s


def run_old_topk(ctx, gal, qd, n, k, thresh):
    from scrfd_arcface_facerecognition_amd._lib import check
    idx, sc = ctx.empty((n, k), np.int32), ctx.empty((n, k), np.float32)
    check(ctx.lib.fid_gallery_topk(ctx.handle, gal.handle, C.c_void_p(qd.ptr), n, k, thresh, C.c_void_p(idx.ptr), C.c_void_p(sc.ptr)))
    return idx.download(), sc.download()


def search_all_slicings(ctx, monkeypatch, gal, qd, n, k, thresh):
    """the search under FID_TOPK_SLICES = 1, 3 and unset: byte-identical, returned once"""
    got = []
    for s in SLICES:
        set_slices(monkeypatch, s)
        got.append(run_search(ctx, gal, qd, n, k, thresh))
    set_slices(monkeypatch, None)
    for other in got[1:]:
        assert got[0][0].tobytes() == other[0].tobytes() and got[0][1].tobytes() == other[1].tobytes()
    return got[0]


def canary_words(shape, dtype):
    return np.frombuffer(bytes([CANARY]) * (int(np.prod(shape)) * np.dtype(dtype).itemsize), dtype).reshape(shape)


# ---- a. small shapes, every k, every slicing; e. the old entry point agrees where it exists -----------------------------------------------------
@pytest.mark.parametrize("G,dim,n", SHAPES + ((1, 32, 17), (33, 32, 17), (300, 32, 129)))
def test_small_shapes_equal_the_reference(ctx, monkeypatch, G, dim, n):
    """one partly filled tile (G = 1, 33), a zero row (row 3), padding rows behind the last real row, two query tiles of which the second holds one
    row (n = 129) or two (130), several gallery tiles (so S = 3 cuts for real), dim 32 = a single K-step and dim 512 = sixteen"""
    from scrfd_arcface_facerecognition_amd.engine import Gallery
    g, q, _ = small_case(G, dim, n)
    g16, q16 = unit_f16(g), unit_f16(q)
    S = cosines(q16, g16)
    gal, qd = Gallery(ctx, g), ctx.to_device(q16)
    try:
        for k in KS:
            for thresh in (0.05, 0.75):
                got, want = search_all_slicings(ctx, monkeypatch, gal, qd, n, k, thresh), ref_topk(S, k, thresh)
                assert same(got, want), (k, thresh, np.flatnonzero((got[0] != want[0]).any(1))[:8])
                assert G < 33 or not (got[0] == ZERO_ROW).any()
        for k in OLD_KS:
            for thresh in (0.05, 0.75):
                assert same(run_search(ctx, gal, qd, n, k, thresh), run_old_topk(ctx, gal, qd, n, k, thresh)), (k, thresh)
    finally:
        gal.close()


# ---- b. outputs and arguments ----------------------------------------------------------------------------------------------------------------------
def test_every_entry_is_written_and_nothing_behind(ctx):
    from scrfd_arcface_facerecognition_amd.engine import Gallery
    G, dim, n = 300, 96, 129
    g, q, _ = small_case(G, dim, n)
    q16 = unit_f16(q)
    q16[NAN_QUERY] = f16_nan_row(dim)
    S = cosines(q16, unit_f16(g))
    gal, qd = Gallery(ctx, g), ctx.to_device(q16)
    try:
        for k in (1, 7, 32):
            i, s = run_search(ctx, gal, qd, n, k, 0.05)                             # (run_search checks the guard bytes)
            assert not (i == canary_words((n, k), np.int32)).any() and not (s.view(np.int32) == canary_words((n, k), np.int32)).any()
            assert same((i, s), ref_topk(S, k, 0.05))
            assert (i[NAN_QUERY] == -1).all() and not s[NAN_QUERY].view(np.uint32).any()          # k x (-1, +0.0)
            assert (i[2] == -1).all() and not s[2].view(np.uint32).any()                          # the zero query
    finally:
        gal.close()


def test_invalid_arguments_leave_the_outputs_untouched(ctx):
    from scrfd_arcface_facerecognition_amd.engine import Gallery
    g, q, _ = small_case(33, 32, 17)
    gal, qd = Gallery(ctx, g), ctx.to_device(unit_f16(q))
    try:
        for n, k, thresh in ((17, 0, 0.05), (17, 33, 0.05), (0, 5, 0.05), (17, 5, float("nan")), (-1, 5, 0.05), (17, -1, 0.05)):
            idx, sc = filled(ctx, 17 * 33 * 4), filled(ctx, 17 * 33 * 4)
            rc = ctx.lib.fid_gallery_search(ctx.handle, gal.handle, C.c_void_p(qd.ptr), n, k, thresh, C.c_void_p(idx.ptr), C.c_void_p(sc.ptr))
            assert rc == FID_E_INVALID, (n, k, thresh, rc)
            ctx.sync()
            assert (idx.download() == CANARY).all() and (sc.download() == CANARY).all(), (n, k, thresh)
        keys = filled(ctx, 3 * 17 * 33 * 8)
        idx, sc = filled(ctx, 17 * 33 * 4), filled(ctx, 17 * 33 * 4)
        lib, h = ctx.lib, ctx.handle
        bad = [lib.fid_topk_keys(h, gal.handle, C.c_void_p(qd.ptr), 17, 0, 0, C.c_void_p(keys.ptr)),
               lib.fid_topk_keys(h, gal.handle, C.c_void_p(qd.ptr), 17, 33, 0, C.c_void_p(keys.ptr)),
               lib.fid_topk_keys(h, gal.handle, C.c_void_p(qd.ptr), 0, 5, 0, C.c_void_p(keys.ptr)),
               lib.fid_topk_keys(h, gal.handle, C.c_void_p(qd.ptr), 17, 5, -1, C.c_void_p(keys.ptr)),
               lib.fid_topk_keys(h, gal.handle, C.c_void_p(qd.ptr), 17, 5, 2 ** 31 - 40, C.c_void_p(keys.ptr)),
               lib.fid_topk_keys(h, gal.handle, None, 17, 5, 0, C.c_void_p(keys.ptr)),
               lib.fid_topk_keys(h, gal.handle, C.c_void_p(qd.ptr), 17, 5, 0, None),
               lib.fid_topk_merge(h, C.c_void_p(keys.ptr), 0, 17, 5, 33, 0.05, C.c_void_p(idx.ptr), C.c_void_p(sc.ptr)),
               lib.fid_topk_merge(h, C.c_void_p(keys.ptr), 3, 0, 5, 33, 0.05, C.c_void_p(idx.ptr), C.c_void_p(sc.ptr)),
               lib.fid_topk_merge(h, C.c_void_p(keys.ptr), 3, 17, 33, 33, 0.05, C.c_void_p(idx.ptr), C.c_void_p(sc.ptr)),
               lib.fid_topk_merge(h, C.c_void_p(keys.ptr), 3, 17, 0, 33, 0.05, C.c_void_p(idx.ptr), C.c_void_p(sc.ptr)),
               lib.fid_topk_merge(h, C.c_void_p(keys.ptr), 3, 17, 5, 33, float("nan"), C.c_void_p(idx.ptr), C.c_void_p(sc.ptr)),
               lib.fid_topk_merge(h, None, 3, 17, 5, 33, 0.05, C.c_void_p(idx.ptr), C.c_void_p(sc.ptr)),
               lib.fid_topk_merge(h, C.c_void_p(keys.ptr), 3, 17, 5, 33, 0.05, None, C.c_void_p(sc.ptr)),
               lib.fid_gallery_search(h, gal.handle, None, 17, 5, 0.05, C.c_void_p(idx.ptr), C.c_void_p(sc.ptr)),
               lib.fid_gallery_search(h, None, C.c_void_p(qd.ptr), 17, 5, 0.05, C.c_void_p(idx.ptr), C.c_void_p(sc.ptr))]
        assert bad == [FID_E_INVALID] * len(bad), bad
        ctx.sync()
        assert (keys.download() == CANARY).all() and (idx.download() == CANARY).all() and (sc.download() == CANARY).all()
    finally:
        gal.close()


# ---- c. the large path: default S leaves each slice more than one tile, planted pairs on the slice seams --------------------------------------------
@pytest.mark.parametrize("name,ns,ks", [("full64", (1, 129), (5, 32)), ("full512", (1, 129), (5, 32)), ("ragged_tile", (129,), (8,))])
def test_large_galleries(ctx, cus, large, monkeypatch, name, ns, ks):
    """256 x CUs rows = 2 x CUs gallery tiles.  Two query tiles (n = 129) get CUs slices of two tiles each by default, so every slice carries its
    lists across a tile border and the pairs planted in front of every 256-row border lie on the slice seams; one query tile gets a slice per
    gallery tile; S = 1 and S = 3 walk hundreds of tiles per workgroup.  ragged_tile: the last tile has 32 rows."""
    gal, g, g16, info, dim = large(name)
    assert 2 * cus - 1 <= -(-gal.G // 128) <= 2 * cus
    for n in ns:
        q16 = unit_f16(build_queries(n, g, info, 10 * n + dim))
        S = cosines(q16, g16)
        qd = ctx.to_device(q16)
        for k in ks:
            for thresh in (0.05, 0.75):
                got, want = search_all_slicings(ctx, monkeypatch, gal, qd, n, k, thresh), ref_topk(S, k, thresh)
                assert same(got, want), (n, k, thresh, np.flatnonzero((got[0] != want[0]).any(1))[:8])
        if n > 1:
            assert (ref_topk(S, ks[0], 0.05)[0] >= info["tail"]).any()               # answers only the last gallery tile can give


# ---- d. shards -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parts", [3, 8])
def test_sharded_keys_merge_equals_the_whole_search(ctx, large, parts):
    from scrfd_arcface_facerecognition_amd._lib import check
    from scrfd_arcface_facerecognition_amd.engine import Gallery
    from scrfd_arcface_facerecognition_amd.pipeline import FacePipeline
    gal, g, g16, info, dim = large("full64")
    n, b = 129, shard_bounds(gal.G, parts)
    q16 = unit_f16(build_queries(n, g, info, 10 * n + dim))
    q16[NAN_QUERY] = f16_nan_row(dim)
    S = cosines(q16, g16)
    qd = ctx.to_device(q16)
    shards = [Gallery(ctx, g[lo:hi]) for lo, hi in zip(b, b[1:])]
    try:
        for k in (5, 16):
            keys = filled(ctx, parts * n * k * 8)
            for r, shard in enumerate(shards):
                check(ctx.lib.fid_topk_keys(ctx.handle, shard.handle, C.c_void_p(qd.ptr), n, k, b[r], C.c_void_p(keys.ptr + r * n * k * 8)))
            K, whole = split(keys, (parts, n, k), np.uint64)
            assert whole
            assert (K[:, :, :-1] >= K[:, :, 1:]).all()                               # descending, so 0 only behind the last candidate
            assert ((K[:, :, :-1] > K[:, :, 1:]) | (K[:, :, 1:] == 0)).all()         # ... and no key twice
            rows, scores = unpack(K)
            for r in range(parts):
                live = K[r] != 0
                assert ((rows[r][live] >= b[r]) & (rows[r][live] < b[r + 1])).all() and (scores[r][live] > 0).all()
            assert not K[:, NAN_QUERY].any() and not K[:, 2].any()                   # the NaN query and the zero query have no candidate
            for thresh in (0.05, 0.75):
                idx, sc = filled(ctx, n * k * 4), filled(ctx, n * k * 4)
                check(ctx.lib.fid_topk_merge(ctx.handle, C.c_void_p(keys.ptr), parts, n, k, gal.G, thresh, C.c_void_p(idx.ptr), C.c_void_p(sc.ptr)))
                (i, gi), (s, gs) = split(idx, (n, k), np.int32), split(sc, (n, k), np.float32)
                want = ref_topk(S, k, thresh)
                assert gi and gs and same((i, s), want), (k, thresh, np.flatnonzero((i != want[0]).any(1))[:8])
                assert same(run_search(ctx, gal, qd, n, k, thresh), want)
        # the thin wrappers of the pipeline are the same calls
        k = 5
        keys2 = ctx.empty((parts, n, k), np.uint64)
        pipe = types.SimpleNamespace(ctx=ctx)                                        # (the wrappers use the pipeline's context and nothing else)
        for r, shard in enumerate(shards):
            FacePipeline.topk_keys(pipe, shard, qd, n, k, b[r], keys2.ptr + r * n * k * 8)
        idx, sc = ctx.empty((n, k), np.int32), ctx.empty((n, k), np.float32)
        FacePipeline.topk_merge(pipe, keys2, parts, n, k, gal.G, 0.05, idx, sc)
        assert same((idx.download(), sc.download()), ref_topk(S, k, 0.05))
    finally:
        for shard in shards:
            shard.close()


# ---- f. real-valued rows ---------------------------------------------------------------------------------------------------------------------------
def test_random_rows_within_the_cosine_tolerance(ctx):
    """64 random normal queries x 5 000 random rows, dim 512, k = 10, threshold 0, against a float64 product of the fp16 unit rows.  1e-3 is the
    project's stated cosine tolerance (README); the fp32 sums themselves differ from float64 by at most 511 * 2^-24 ~ 3e-5."""
    from scrfd_arcface_facerecognition_amd._lib import check
    from scrfd_arcface_facerecognition_amd.engine import Gallery
    from test_gpu_range_join import gallery_rows
    rng = np.random.default_rng(2024)
    n, G, dim, k = 64, 5000, 512, 10
    gal = Gallery(ctx, rng.standard_normal((G, dim)).astype(np.float32))
    try:
        e = ctx.to_device(rng.standard_normal((n, dim)).astype(np.float32))
        qd = ctx.empty((n, dim), np.float16)
        check(ctx.lib.fid_l2_normalize_f16(ctx.handle, C.c_void_p(e.ptr), n, dim, C.c_void_p(qd.ptr)))
        ref = qd.download().astype(np.float64) @ gallery_rows(ctx, gal).download()[:G].astype(np.float64).T
        idx, sc = run_search(ctx, gal, qd, n, k, 0.0)
        assert (idx >= 0).all() and (idx < G).all()                                  # 5 000 random rows: every query has ten positive scores
        for r in range(n):
            assert len(set(idx[r].tolist())) == k
            err = np.abs(sc[r].astype(np.float64) - ref[r, idx[r]]).max()
            print("query %d: max |score - float64| = %.3g" % (r, err))
            assert err <= 1e-3
            assert (np.diff(sc[r]) <= 0).all()
            for j in np.argsort(-ref[r])[:k]:
                assert j in idx[r] or abs(ref[r, j] - float(sc[r, -1])) <= 1e-3, (r, j)
    finally:
        gal.close()


# ---- g. Python -------------------------------------------------------------------------------------------------------------------------------------
def test_vector_gallery_search_any_k(ctx):
    from scrfd_arcface_facerecognition_amd.engine import VectorGallery
    rng = np.random.default_rng(9)
    G, dim = 300, 64
    emb = probe_rows(rng, G, dim, prototypes(rng, dim), {})
    ids = ["p%d" % i for i in range(G)]
    vg = VectorGallery(ctx, dim=dim, capacity=G)
    vg.upsert(ids, emb)
    assert [vg.row_of[i] for i in ids] == list(range(G))                             # rows in id order: the argsort below breaks ties the same way
    q = emb[[7, 130, 299, 12]]
    S = (unit_f16(q).astype(np.float64) @ unit_f16(emb).astype(np.float64).T)

    def want(S, k, thresh=0.0, gone=()):
        out = []
        for s in S:
            order = [int(j) for j in np.argsort(-s, kind="stable") if s[j] > thresh and j not in gone][:k]
            out.append([(ids[j], float(np.float32(s[j]))) for j in order])
        return out
    for k in (3, 10, 5, 32):
        assert vg.search(q, k=k) == want(S, k), k                                    # k = 3, 10: FID_E_INVALID before
    assert vg.search(q, k=10, score_threshold=0.5) == want(S, 10, 0.5)
    assert vg.search(q, k=5, via="fused") == vg.search(q, k=5, via="matrix") == want(S, 5)
    with pytest.raises(ValueError, match="range_search"):
        vg.search(q, k=33)
    with pytest.raises(ValueError):
        vg.search(q, k=0)
    with pytest.raises(ValueError):
        vg.search(q, k=3, via="matrix")
    best = vg.search(q[:1], k=3)[0][0][0]
    vg.delete([best])
    after = vg.search(q[:1], k=3)
    assert best not in [i for i, _ in after[0]] and after == want(S[:1], 3, gone={ids.index(best)})
