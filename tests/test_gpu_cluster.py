"""GPU: fid_gallery_cluster (density clusters on the device, csrc/cluster.hip), VectorGallery.cluster and FaceAnalysis.cluster_faces.

Exact probes (tests/cluster_cases.py): rows of +-1 / 0 whose unit entries fp16 holds exactly, so every cosine is an exact multiple of 1/64 in fp32
whatever the summation order: label, degree, via, score (as uint32) and summary must equal tests/cluster_oracle.py bit for bit, also at a
threshold that is itself attained, with canary bytes behind every output.  Positions are cut into tiles of 128: the planted pairs sit inside a
tile, across the 127 | 128 seam and two tiles apart, the gallery has free holes and `rows` is deliberately not ascending."""
import ctypes as C

import numpy as np
import pytest

import cluster_cases as K
import cluster_oracle as O
from test_gpu_range_join import CANARY, canary_i32, gallery_rows, near_copy_store, shuffled_store
from test_range_join_cpu import duplicate_store

pytestmark = pytest.mark.gpu

PAGE = 4096


@pytest.fixture(scope="module")
def ctx():
    from scrfd_arcface_facerecognition_amd._lib import default_context
    return default_context(0)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


# ---- the entry point -----------------------------------------------------------------------------------------------------------------------------
def cluster_call(ctx, gal, rows_dev, n, thresh, min_pts, outputs, null_ctx=False):
    """fid_gallery_cluster's return code; outputs = (label, degree, via, score, summary) device buffers (or None)"""
    from scrfd_arcface_facerecognition_amd._lib import _ptr
    return ctx.lib.fid_gallery_cluster(None if null_ctx else ctx.handle, None if gal is None else gal.handle, _ptr(rows_dev), int(n),
                                       C.c_float(thresh), int(min_pts), *[_ptr(o) for o in outputs])


def canary_outputs(ctx, n):
    from scrfd_arcface_facerecognition_amd._lib import check
    bufs = [ctx.empty((n + PAGE // 4,), dt) for dt in (np.int32, np.int32, np.int32, np.float32)] + [ctx.empty((6 + PAGE // 4,), np.int32)]
    for b in bufs:
        check(ctx.lib.fid_memset(ctx.handle, C.c_void_p(b.ptr), CANARY, b.nbytes))
    return bufs


def fetch(bufs, n):
    """-> label, degree, via, score [n], summary (6); nothing beyond n entries (6 for the summary) may have been written"""
    host = [b.download() for b in bufs]
    for h, m in zip(host, (n, n, n, n, 6)):
        assert (h[m:].view(np.int32) == canary_i32()).all()
    return host[0][:n], host[1][:n], host[2][:n], host[3][:n], tuple(int(v) for v in host[4][:6])


def run_cluster(ctx, gal, rows, thresh, min_pts, n=None):
    """rows: int32 array, or None = every gallery row"""
    from scrfd_arcface_facerecognition_amd._lib import check
    m = gal.G if rows is None else len(rows)
    bufs = canary_outputs(ctx, m)
    rows_dev = None if rows is None else ctx.to_device(np.ascontiguousarray(rows, dtype=np.int32))
    check(cluster_call(ctx, gal, rows_dev, m if n is None else n, thresh, min_pts, bufs))
    return fetch(bufs, m)


class Store:
    """a gallery of exact rows and its stored bytes on the host"""

    def __init__(self, ctx, g):
        from scrfd_arcface_facerecognition_amd.engine import Gallery
        self.ctx, self.gal = ctx, Gallery(ctx, g)
        self.before = gallery_rows(ctx, self.gal).download()
        assert np.array_equal(bits(self.before[:len(g)]), bits(K.unit_f16(g)))      # the stored rows are the exact ones

    def check(self, rows, thresh, min_pts, what=""):
        want = O.cluster(self.before[:self.gal.G], rows, thresh, min_pts)
        got = run_cluster(self.ctx, self.gal, rows, thresh, min_pts)
        assert K.same(got, want) is None, (what, thresh, min_pts, K.same(got, want))
        return want

    def unchanged(self):
        return np.array_equal(bits(gallery_rows(self.ctx, self.gal).download()), bits(self.before))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.gal.close()


# ---- planted probe stores ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, dim", K.PROBE_SHAPES)
def test_cluster_exact_probes(ctx, n, dim):
    g, rows, plants = K.probe_case(n, dim)
    assert n < 3 or not np.array_equal(rows, np.sort(rows))
    with Store(ctx, g) as st:
        clusters = 0
        for thresh in (0.75, K.ABOVE):
            for min_pts in (1, 2, 3):
                want = st.check(rows, thresh, min_pts)
                assert want[4][4] == n
                clusters += want[4][0]
                label, degree, via, score, _ = want
                if "seam" in plants and min_pts <= 2:
                    assert label[127] == label[128] >= 0 and score[128] >= 0.875     # 0.875 across the 127 | 128 seam
                if "far" in plants and min_pts <= 2:
                    if thresh == 0.75:
                        assert label[290] == label[5] >= 0 and score[290] >= 0.75    # two tiles apart, exactly at the threshold
                    else:
                        assert score[290] != 0.75
        assert n == 1 or clusters > 0
        assert st.unchanged()                                                        # the gallery is never written


@pytest.mark.parametrize("n, dim", [(300, 512), (29, 32)])
def test_a_shuffled_path_is_one_cluster_to_any_depth(ctx, n, dim):
    g, rows, t_of = K.path_case(n, dim)
    with Store(ctx, g) as st:
        label, degree, via, score, summary = st.check(rows, 0.75, 3)
        assert summary == (1, n - 2, 2, 0, n, 0)
        ends = np.nonzero((t_of == 0) | (t_of == n - 1))[0]
        assert ends[0] == 0 and (degree[ends] == 2).all() and (np.delete(degree, ends) == 3).all()
        lowest_core = int(np.nonzero(degree >= 3)[0][0])
        assert lowest_core > 0 and (label == lowest_core).all()                      # the lowest CORE position, not the lowest position
        assert (score == 0.75).all()
        assert st.check(rows, 0.75, 2)[4] == (1, n, 0, 0, n, 0)
        assert st.check(rows, K.ABOVE, 3)[4] == (0, 0, 0, n, n, 0)
        assert st.check(rows, 0.5, 1)[4] == (1, n, 0, 0, n, 0)
        assert st.unchanged()


@pytest.mark.parametrize("equal", [True, False])
@pytest.mark.parametrize("p_low", [True, False])
def test_a_border_between_two_clusters_takes_the_best_score_then_the_lower_position(ctx, equal, p_low):
    g, rows, pos = K.tie_case(equal, p_low)
    with Store(ctx, g) as st:
        label, degree, via, score, summary = st.check(rows, 0.625, 4)
        assert summary == (2, 2, 5, 0, 7, 0) and degree[pos["x"]] == 3 and degree[pos["P"]] == degree[pos["Q"]] == 4
        assert label[pos["P"]] == pos["P"] and label[pos["Q"]] == pos["Q"]
        winner = min(pos["P"], pos["Q"]) if equal else pos["P"]
        assert via[pos["x"]] == label[pos["x"]] == winner and score[pos["x"]] == (0.75 if equal else 0.875)


def test_a_dense_store_is_one_cluster(ctx):
    """300 identical rows: every pair hits, every wave of every tile hooks into the same tree and raises the same keys at once"""
    row = np.zeros(64, np.float32)
    row[::4] = [1, -1] * 8
    with Store(ctx, np.tile(row, (300, 1))) as st:
        for min_pts in (2, 300, 301):
            label, degree, via, score, summary = st.check(None, 0.9, min_pts)
            assert (degree == 300).all()
            if min_pts <= 300:
                assert summary == (1, 300, 0, 0, 300, 0) and (label == 0).all() and via[0] == 1 and (via[1:] == 0).all() and (score == 1.0).all()
            else:
                assert summary == (0, 0, 0, 300, 300, 0) and (label == -1).all() and (via == -1).all()


def test_more_tiles_than_one_super_tile(ctx):
    """2 200 positions are 18 tiles: two super-tiles of 16 per side, the second ragged, and the skipped lower half of the diagonal ones"""
    from test_gpu_range_join import gallery_special, probe_rows, prototypes
    n, dim = 2200, 32
    rng = np.random.default_rng(n)
    g = probe_rows(rng, n, dim, prototypes(rng, dim), gallery_special(n))
    rows = rng.permutation(n).astype(np.int32)
    with Store(ctx, g) as st:
        for min_pts in (1, 3):
            label, degree, via, score, summary = st.check(rows, 0.75, min_pts)
            tiles = {(min(k, v) // 128, max(k, v) // 128) for k, v in enumerate(via) if v >= 0}
            assert summary[0] >= 20 and len(tiles) > 100
            # best cores in the first diagonal super-tile, in the off-diagonal one and in the ragged second diagonal one
            assert any(b < 16 for a, b in tiles) and any(a < 16 <= b for a, b in tiles) and (min_pts > 1 or any(a >= 16 for a, b in tiles))


# ---- rows that take no part ------------------------------------------------------------------------------------------------------------------------
def test_zero_marker_and_outside_rows_take_no_part(ctx):
    n, dim = 200, 32
    g, rows, plants = K.probe_case(n, dim)
    zero, marker, outside = [0, 64, 130, 199], [1, 127, 129], [3, 128, 150]
    with Store(ctx, g) as st:
        view = gallery_rows(ctx, st.gal)
        host = st.before.copy()
        host[rows[zero + marker]] = 0
        bits(host)[rows[marker], 0] = 0x8000                                         # the -0.0-first marker row of an empty slot
        view.upload(host)
        st.before = host
        bad = rows.copy()
        bad[outside] = [-1, st.gal.G, 2 ** 31 - 1]
        for min_pts in (1, 2):
            label, degree, via, score, summary = st.check(bad, 0.75, min_pts)
            off = zero + marker + outside
            assert (label[off] == -1).all() and (degree[off] == 0).all() and (via[off] == -1).all() and (score[off] == 0).all()
            assert summary[4] == n - 10 and not np.isin(via, off).any() and not np.isin(label, off).any()
        assert st.check(rows, 0.75, 2)[0][9] >= 0                                    # (with its partner inside the gallery, position 9 is clustered)
        assert st.unchanged()


def test_null_rows_means_every_gallery_row(ctx):
    g, rows, _ = K.probe_case(300, 32)
    with Store(ctx, g) as st:
        G = st.gal.G
        for min_pts in (1, 3):
            want = st.check(np.arange(G, dtype=np.int32), 0.75, min_pts)
            got = run_cluster(ctx, st.gal, None, 0.75, min_pts, n=-5)                # (n is ignored)
            assert K.same(got, want) is None and want[4][4] == 300 and want[4][0] > 0


def test_the_bitmap_skip_does_not_change_the_answer(ctx, monkeypatch):
    g, rows, _ = K.probe_case(300, 512)
    gp, rows_p, _ = K.path_case(300, 512)
    for store, r in ((g, rows), (gp, rows_p)):
        with Store(ctx, store) as st:
            monkeypatch.delenv("FID_CLUSTER_SKIP", raising=False)
            on = run_cluster(ctx, st.gal, r, 0.75, 2)
            monkeypatch.setenv("FID_CLUSTER_SKIP", "0")
            off = run_cluster(ctx, st.gal, r, 0.75, 2)
            assert K.same(off, on) is None and K.same(on, O.cluster(st.before[:st.gal.G], r, 0.75, 2)) is None


def test_two_calls_back_to_back(ctx):
    """no synchronise between them; the second call reuses the scratch arena of the first"""
    from scrfd_arcface_facerecognition_amd._lib import check
    g, rows, _ = K.probe_case(300, 32)
    with Store(ctx, g) as st:
        rows_dev = ctx.to_device(rows)
        first, second = canary_outputs(ctx, 300), canary_outputs(ctx, 300)
        check(cluster_call(ctx, st.gal, rows_dev, 300, 0.75, 2, first))
        check(cluster_call(ctx, st.gal, rows_dev, 300, K.ABOVE, 1, second))
        assert K.same(fetch(first, 300), O.cluster(st.before[:st.gal.G], rows, 0.75, 2)) is None
        assert K.same(fetch(second, 300), O.cluster(st.before[:st.gal.G], rows, K.ABOVE, 1)) is None


def test_argument_checks_enqueue_nothing(ctx):
    g, rows, _ = K.probe_case(17, 32)
    with Store(ctx, g) as st:
        gal = st.gal
        rows_dev = ctx.to_device(rows)
        outs = canary_outputs(ctx, 17)
        for thr in (float("nan"), 0.0, -0.5):
            assert cluster_call(ctx, gal, rows_dev, 17, thr, 2, outs) == -1, thr
            assert ctx.lib.fid_last_error() != b""
        for n in (0, -3, (1 << 20) + 1):
            assert cluster_call(ctx, gal, rows_dev, n, 0.75, 2, outs) == -1, n
        assert b"1048576" in ctx.lib.fid_last_error()
        for min_pts in (0, -1):
            assert cluster_call(ctx, gal, rows_dev, 17, 0.75, min_pts, outs) == -1, min_pts
        # (dim % 32 != 0 cannot be reached from here: fid_gallery_create refuses such a gallery)
        assert cluster_call(ctx, gal, rows_dev, 17, 0.75, 2, outs, null_ctx=True) == -1
        assert cluster_call(ctx, None, rows_dev, 17, 0.75, 2, outs) == -1
        for i in range(5):
            assert cluster_call(ctx, gal, rows_dev, 17, 0.75, 2, [None if j == i else o for j, o in enumerate(outs)]) == -1, i
        ctx.sync()
        assert all((b.download().view(np.int32) == canary_i32()).all() for b in outs)
        assert st.unchanged()


# ---- realistic values, through the Python layer ------------------------------------------------------------------------------------------------
def union_find_clusters(ids, pairs):
    parent = {i: i for i in ids}

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i
    for a, b, _ in pairs:
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    out = {}
    for i in sorted(ids):
        out.setdefault(find(i), []).append(i)
    return [out[k] for k in sorted(out)]


# (the seeds were picked on the CPU, with the fp16 rounding emulated, so that no pair lies within 1e-4 of the threshold; asserted below on the rows
# the device actually stores)
@pytest.mark.parametrize("which, seed, capacity", [("duplicates120", 55, 128), ("copies700", 11, 1024)])
def test_realistic_values_through_vector_gallery(ctx, which, seed, capacity):
    """The reference is float64 on the fp16 unit rows as stored, so the only difference left is the order of the fp32 sums, bounded by
    (K - 1) * 2^-24 * sum|a_i b_i| <= 511 * 6e-8 ~ 3e-5 for unit rows (test_gpu_range_join): with no pair within 1e-4 of the threshold the hit
    graph is the oracle's, so labels, degrees and counts are equal; via where the two best core scores are more than 1e-4 apart; scores within 1e-4."""
    rng = np.random.default_rng(seed)
    emb = duplicate_store(rng) if which == "duplicates120" else near_copy_store(rng)
    vg, ids = shuffled_store(ctx, rng, emb, capacity)
    stored = gallery_rows(ctx, vg._gal).download()
    order = sorted(ids)
    rows = np.asarray([vg.row_of[i] for i in order])
    x = stored[rows].astype(np.float64)
    S = x @ x.T
    thresh = 0.8
    assert np.abs(S[np.triu_indices(len(order), 1)] - thresh).min() > 1e-4
    for min_samples in (1, 2, 3):
        label, degree, via, score, summary = O.cluster_scores(S.astype(np.float32), np.ones(len(order), bool), thresh, min_samples)
        res = vg.cluster(thresh, min_samples)
        assert np.array_equal(res.label_pos, label) and np.array_equal(res.degree_pos, degree)
        assert tuple(res.summary) == summary and summary[0] >= 2
        core = degree >= min_samples
        for k in range(len(order)):
            cand = np.sort(np.where((S[k] >= thresh) & core & (np.arange(len(order)) != k), S[k], -1.0))[::-1]
            if cand[0] > 0 and cand[0] - max(cand[1], 0.0) > 1e-4:
                assert res.via_pos[k] == via[k], k
            assert (res.via_pos[k] >= 0) == (via[k] >= 0)
            if via[k] >= 0:
                assert abs(float(res.score_pos[k]) - S[k, res.via_pos[k]]) < 1e-4
        # the result object speaks ids
        assert res.labels == {order[k]: (order[label[k]] if label[k] >= 0 else None) for k in range(len(order))}
        assert [c[0] for c in res.clusters] == sorted(c[0] for c in res.clusters) and all(c == sorted(c) for c in res.clusters)
        assert res.counts["clusters"] == len(res.clusters) and len(res.noise) == res.counts["noise"]
        if min_samples == 1:                                                         # plain connected components of today's only route
            assert res.clusters == union_find_clusters(order, vg.similar_pairs(thresh)) and res.noise == []
    sub = order[::3]
    res = vg.cluster(thresh, 1, ids=sub)
    rows = np.asarray([vg.row_of[i] for i in sub])
    assert np.array_equal(res.label_pos, O.cluster(stored[:vg._gal.G], rows, thresh, 1)[0])
    assert np.array_equal(bits(gallery_rows(ctx, vg._gal).download()), bits(stored))


def test_cluster_of_an_empty_store_and_the_size_limit(ctx, monkeypatch):
    from scrfd_arcface_facerecognition_amd import engine
    vg = engine.VectorGallery(ctx, 512, capacity=8)
    res = vg.cluster()
    assert res.clusters == [] and res.labels == {} and res.counts["took_part"] == 0
    vg.upsert([4, 2, 9], np.eye(3, 512, dtype=np.float32))
    res = vg.cluster(0.5, 1)
    assert res.clusters == [[2], [4], [9]] and res.via == {}
    monkeypatch.setattr(engine, "CLUSTER_MAX_ROWS", 2)
    with pytest.raises(ValueError):
        vg.cluster()


def test_cluster_faces_is_get_batch_plus_cluster(ctx, monkeypatch):
    """glue only: get_batch is stubbed to return chosen embeddings"""
    from scrfd_arcface_facerecognition_amd.app import Face, FaceAnalysis
    x = np.zeros((5, 512), np.float32)
    for t in range(4):
        x[t, t:t + 4] = 1                                                            # a path of four: 0.75 between neighbours
    x[4, 100:104] = 1                                                                # on its own
    faces = [[Face(embedding=x[0] * 2.0), Face(embedding=x[4])], [], [Face(embedding=x[2]), Face(embedding=x[1] * 0.5), Face(embedding=x[3])]]
    app = FaceAnalysis.__new__(FaceAnalysis)
    app.ctx = ctx
    seen = {}
    monkeypatch.setattr(FaceAnalysis, "get_batch", lambda self, images, max_num=0: seen.update(images=images, max_num=max_num) or faces)
    res = app.cluster_faces(["a", "b", "c"], similarity_threshold=0.75, min_samples=3, max_num=7)
    assert seen == {"images": ["a", "b", "c"], "max_num": 7}
    # path order: (0,0) - (2,1) - (2,0) - (2,2); the two inner faces are cores, the ends borders, (0,1) is noise
    assert res.clusters == [[(0, 0), (2, 0), (2, 1), (2, 2)]] and res.noise == [(0, 1)]
    assert res.labels[(0, 0)] == (2, 0) and res.via[(0, 0)] == ((2, 1), 0.75) and res.degree[(2, 0)] == 3
    assert res.counts == {"clusters": 1, "cores": 2, "borders": 2, "noise": 1, "took_part": 5}
