"""GPU: fid_gallery_score_hist (genuine / impostor score distributions on the device, csrc/calib.hip), VectorGallery.score_distribution and
FaceAnalysis.calibrate_faces.

Exact stores (tests/calib_cases.py): rows of +-1 on fixed columns whose unit entries fp16 holds exactly, so every cosine is an exact multiple of
1/32 (1/8 at dim 32) in fp32 whatever the summation order: both histograms, both via / score tables (scores as uint32) and the summary must equal
tests/calib_oracle.py and the host twin bit for bit -- with 64 bins at dim 512 every score sits exactly on a bin edge -- with canary bytes behind
every output.  Positions are cut into tiles of 128: the stores cover one tile, the 127 | 128 seam, three tiles and, at 2 049 positions, the edge of
a super-tile of 16 tiles."""
import ctypes as C

import numpy as np
import pytest

import calib_cases as K
import calib_oracle as O
from test_gpu_range_join import CANARY, canary_i32, gallery_rows

pytestmark = pytest.mark.gpu

PAGE = 4096


@pytest.fixture(scope="module")
def ctx():
    from scrfd_arcface_facerecognition_amd._lib import default_context
    return default_context(0)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


# ---- the entry point -----------------------------------------------------------------------------------------------------------------------------
def hist_call(ctx, gal, rows_dev, labels_dev, n, bins, outputs, null_ctx=False):
    """fid_gallery_score_hist's return code; outputs = (hist, imp_via, imp_score, gen_via, gen_score, summary) device buffers (or None)"""
    from scrfd_arcface_facerecognition_amd._lib import _ptr
    return ctx.lib.fid_gallery_score_hist(None if null_ctx else ctx.handle, None if gal is None else gal.handle, _ptr(rows_dev), _ptr(labels_dev),
                                          int(n), int(bins), *[_ptr(o) for o in outputs])


def canary_outputs(ctx, n, bins):
    from scrfd_arcface_facerecognition_amd._lib import check
    bufs = [ctx.empty((2 * bins + PAGE // 8,), np.uint64)] + [ctx.empty((n + PAGE // 4,), dt) for dt in (np.int32, np.float32, np.int32, np.float32)] + \
           [ctx.empty((4 + PAGE // 8,), np.uint64)]
    for b in bufs:
        check(ctx.lib.fid_memset(ctx.handle, C.c_void_p(b.ptr), CANARY, b.nbytes))
    return bufs


def fetch(bufs, n, bins):
    """-> hist [2, bins], imp_via, imp_score, gen_via, gen_score [n], summary (4); nothing beyond may have been written"""
    host = [b.download() for b in bufs]
    for h, m in zip(host, (2 * bins, n, n, n, n, 4)):
        assert (h[m:].view(np.int32) == canary_i32()).all()
    return host[0][:2 * bins].reshape(2, bins), host[1][:n], host[2][:n], host[3][:n], host[4][:n], tuple(int(v) for v in host[5][:4])


def run_hist(ctx, gal, rows, labels, bins, n=None):
    """rows: int32 array, or None = every gallery row"""
    from scrfd_arcface_facerecognition_amd._lib import check
    m = gal.G if rows is None else len(rows)
    bufs = canary_outputs(ctx, m, bins)
    rows_dev = None if rows is None else ctx.to_device(np.ascontiguousarray(rows, dtype=np.int32))
    labels_dev = ctx.to_device(np.ascontiguousarray(labels, dtype=np.int32))
    check(hist_call(ctx, gal, rows_dev, labels_dev, m if n is None else n, bins, bufs))
    return fetch(bufs, m, bins)


def host_twin(g16, rows, labels, bins):
    from test_calib_cpu import host_call
    rc, got = host_call(g16, rows, labels, bins)
    assert rc == 0
    n = len(g16) if rows is None else len(rows)
    return got[0], got[1][:n], got[2][:n], got[3][:n], got[4][:n], got[5]


class Store:
    """a gallery of exact rows (plants: the -0.0 marker row is put in place) and its stored bytes on the host"""

    def __init__(self, ctx, g, plants=None):
        from scrfd_arcface_facerecognition_amd.engine import Gallery
        self.ctx, self.gal = ctx, Gallery(ctx, g)
        view = gallery_rows(ctx, self.gal)
        self.before = view.download()
        assert np.array_equal(bits(self.before[:len(g)]), bits(K.unit_f16(g)))      # the stored rows are the exact ones
        if plants is not None:
            bits(self.before)[plants["marker_row"], 0] = 0x8000
            view.upload(self.before)
        self.g16 = self.before[:self.gal.G]

    def check(self, rows, labels, bins, what=""):
        want = O.score_hist(self.g16, rows, labels, bins)
        got = run_hist(self.ctx, self.gal, rows, labels, bins)
        assert K.same(got, want) is None, (what, bins, K.same(got, want))
        return want

    def unchanged(self):
        return np.array_equal(bits(gallery_rows(self.ctx, self.gal).download()), bits(self.before))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.gal.close()


# ---- exact stores ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, dim", K.PROBE_SHAPES)
def test_exact_stores_equal_the_host_twin_and_the_oracle(ctx, n, dim):
    g, rows, labels, plants = K.exact_case(n, dim)
    assert n < 3 or not np.array_equal(rows, np.sort(rows))
    with Store(ctx, g, plants) as st:
        G = st.gal.G
        all_labels = (np.arange(G) % 5).astype(np.int32)
        all_labels[::11] = -1
        for bins in K.BINS:
            want = st.check(rows, labels, bins, "rows")
            assert K.same(host_twin(st.g16, rows, labels, bins), want) is None
            took = want[5][0]
            assert want[5][1] + want[5][2] == took * (took - 1) // 2 and want[5][3] == 0
            want = st.check(None, all_labels, bins, "NULL rows")
            assert K.same(host_twin(st.g16, None, all_labels, bins), want) is None
        hist, imp_via, imp_score, gen_via, gen_score, summary = O.score_hist(st.g16, rows, labels, 64)
        if n >= 17:
            a, c = plants["dup_other"]
            assert hist[0][63] >= 1 and hist[1][63] >= 1 and hist[1][0] >= 1 and imp_via[a] == c and imp_score[a] == 1.0
            assert gen_via[plants["lonely"]] == -1 and summary[0] < n
        if n >= 129:
            t, u, v = plants["tie"]
            assert imp_via[t] == u and (n < 300 or u // 128 != v // 128)
        assert st.unchanged()                                                        # the gallery is never written


def test_more_tiles_than_one_super_tile(ctx, monkeypatch):
    """2 049 positions are 17 tiles: two super-tiles of 16 per side, the second one tile wide, and the skipped lower half of the diagonal ones.
    With three workgroups each walks hundreds of tile pairs and flushes its LDS histogram every time it leaves a super-tile; the answer depends
    neither on that nor on the in-wave aggregation."""
    n, dim = 2049, 32
    g, rows, labels, plants = K.exact_case(n, dim, persons=40)
    with Store(ctx, g, plants) as st:
        want = O.score_hist(st.g16, rows, labels, 64)
        assert want[5][1] > 40000 and want[5][2] > 2000000
        tiles = {(min(k, v) // 128, max(k, v) // 128) for k, v in enumerate(want[1]) if v >= 0}
        assert any(b < 16 for a, b in tiles) and any(a < 16 <= b for a, b in tiles)
        for grid, peel in ((None, None), ("3", None), ("40", "4"), (None, "4")):
            for name, v in (("FID_HIST_GRID", grid), ("FID_HIST_PEEL", peel)):
                monkeypatch.delenv(name, raising=False) if v is None else monkeypatch.setenv(name, v)
            got = run_hist(ctx, st.gal, rows, labels, 64)
            assert K.same(got, want) is None, (grid, peel, K.same(got, want))
        monkeypatch.delenv("FID_HIST_GRID", raising=False)
        monkeypatch.delenv("FID_HIST_PEEL", raising=False)
        assert K.same(run_hist(ctx, st.gal, rows, labels, 4096), O.score_hist(st.g16, rows, labels, 4096)) is None


@pytest.mark.parametrize("peel", ["4", "0"])
def test_every_pair_in_one_bin(ctx, monkeypatch, peel):
    """300 identical rows: all 44 850 pairs score exactly 1 and go into ONE counter (two with alternating labels): the contention path"""
    monkeypatch.setenv("FID_HIST_PEEL", peel)
    n = 300
    with Store(ctx, K.one_row_case(n)) as st:
        for bins in (64, 2, 4096):
            hist, imp_via, imp_score, gen_via, gen_score, summary = st.check(None, np.zeros(n, np.int32), bins, "one label")
            assert hist[0][bins - 1] == n * (n - 1) // 2 == 44850 and hist.sum() == 44850 and summary == (n, 44850, 0, 0)
            assert (imp_via == -1).all() and gen_via[0] == 1 and (gen_via[1:] == 0).all() and (gen_score == 1.0).all()
            hist, imp_via, imp_score, gen_via, gen_score, summary = st.check(None, (np.arange(n) % 2).astype(np.int32), bins, "two labels")
            assert hist[0][bins - 1] == 2 * (150 * 149 // 2) and hist[1][bins - 1] == 150 * 150 and summary == (n, 22350, 22500, 0)
            assert summary[1] + summary[2] == n * (n - 1) // 2
            assert imp_via[0] == 1 and (imp_via[1::2] == 0).all() and (imp_via[2::2] == 1).all() and gen_via[0] == 2 and gen_via[1] == 3


def test_two_calls_in_a_row_on_the_same_outputs_give_the_same_bytes(ctx):
    """no synchronise between them; the second call reuses the scratch arena and the outputs of the first: prepare zeroes them again"""
    from scrfd_arcface_facerecognition_amd._lib import check
    g, rows, labels, plants = K.exact_case(300, 32)
    with Store(ctx, g, plants) as st:
        rows_dev, labels_dev = ctx.to_device(rows), ctx.to_device(labels)
        other = ctx.to_device(((np.arange(300) * 7) % 3).astype(np.int32))
        bufs = canary_outputs(ctx, 300, 64)
        check(hist_call(ctx, st.gal, rows_dev, labels_dev, 300, 64, bufs))
        first = [b.download() for b in bufs]
        check(hist_call(ctx, st.gal, rows_dev, other, 300, 64, bufs))               # other labels in between: nothing of them may stay
        check(hist_call(ctx, st.gal, rows_dev, labels_dev, 300, 64, bufs))
        second = [b.download() for b in bufs]
        assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(first, second))
        assert K.same(fetch(bufs, 300, 64), O.score_hist(st.g16, rows, labels, 64)) is None


def test_argument_checks_enqueue_nothing(ctx):
    g, rows, labels, plants = K.exact_case(17, 32)
    with Store(ctx, g) as st:
        gal = st.gal
        rows_dev, labels_dev = ctx.to_device(rows), ctx.to_device(labels)
        outs = canary_outputs(ctx, 17, 64)
        for bins in (0, 1, 63, -2, 4098, 5000):
            assert hist_call(ctx, gal, rows_dev, labels_dev, 17, bins, outs) == -1, bins
            assert ctx.lib.fid_last_error() != b""
        for n in (0, -3, (1 << 20) + 1):
            assert hist_call(ctx, gal, rows_dev, labels_dev, n, 64, outs) == -1, n
        assert b"1048576" in ctx.lib.fid_last_error()
        # (dim % 32 != 0 and a gallery beyond 4 GiB cannot be reached from here: fid_gallery_create refuses the one, the other needs the memory)
        assert hist_call(ctx, gal, rows_dev, labels_dev, 17, 64, outs, null_ctx=True) == -1
        assert hist_call(ctx, None, rows_dev, labels_dev, 17, 64, outs) == -1
        assert hist_call(ctx, gal, rows_dev, None, 17, 64, outs) == -1
        for i in range(6):
            assert hist_call(ctx, gal, rows_dev, labels_dev, 17, 64, [None if j == i else o for j, o in enumerate(outs)]) == -1, i
        ctx.sync()
        assert all((b.download().view(np.int32) == canary_i32()).all() for b in outs)
        assert st.unchanged()


# ---- realistic values ------------------------------------------------------------------------------------------------------------------------------
def test_random_unit_rows_against_float64_with_a_derived_margin(ctx):
    """30 persons x 10 noisy copies, dim 512, 64 bins.  The sums are not exact here.  The reference is float64 on the fp16 rows as stored, so the only
    difference left is the order of the fp32 sums, bounded for ANY order by dim * 2^-24 * sum|a_i b_i| per pair.  A pair whose float64 score lies
    within that margin of a bin edge is AMBIGUOUS: it may sit in either of the two bins at that edge.  Without the ambiguous pairs the device
    histogram must be the float64 one; with them, every ambiguous pair must be found in one of its two bins.  The class totals are exact.
    Measured on an MI355X: see the figures printed below (the condition, at most 1 % ambiguous pairs, is checked on the reference alone)."""
    from scrfd_arcface_facerecognition_amd.engine import Gallery
    n, dim, bins, half = 300, 512, 64, 32
    rng = np.random.default_rng(0)
    centres = rng.standard_normal((30, dim))
    x = (np.repeat(centres, 10, axis=0) + 0.7 * rng.standard_normal((n, dim))).astype(np.float32)
    labels = np.repeat(np.arange(30), 10).astype(np.int32)
    gal = Gallery(ctx, x)
    try:
        stored = gallery_rows(ctx, gal).download()[:n].astype(np.float64)
        got = run_hist(ctx, gal, None, labels, bins)
    finally:
        gal.close()
    S = stored @ stored.T
    margin = dim * 2.0 ** -24 * (np.abs(stored) @ np.abs(stored).T)
    iu = np.triu_indices(n, 1)
    s, m, imp = S[iu], margin[iu], (labels[iu[0]] != labels[iu[1]])
    edge = np.round(s * half)                                                        # the nearest edge, in units of the bin width
    amb = np.abs(s * half - edge) / half <= m
    print(f"ambiguous pairs: {int(amb.sum())} of {len(s)}; largest margin {m.max():.3g}")
    assert amb.sum() <= 0.01 * len(s)                                                # the condition (on the reference alone)
    hist, imp_via, imp_score, gen_via, gen_score, summary = got
    assert summary == (n, int((~imp).sum()), int(imp.sum()), 0) and summary[1] == 30 * 45
    for cls, of_class in enumerate((~imp, imp)):
        sure = np.bincount((np.floor(s[of_class & ~amb] * half) + half).astype(np.int64), minlength=bins)
        rest = hist[cls].astype(np.int64) - sure                                     # what the ambiguous pairs must account for
        assert (rest >= 0).all() and rest.sum() == (of_class & amb).sum()
        # pairs at edge e sit in bin e - 1 or e (0 < e < bins for unit rows this far from +-1); walk the bins upward: what is left of edge b
        # must be in bin b, the remainder of bin b comes from edge b + 1
        at_edge = np.bincount((edge[of_class & amb] + half).astype(np.int64), minlength=bins + 1)
        assert at_edge[0] == 0 and at_edge[bins] == 0
        left = 0
        for b in range(bins):
            assert left <= rest[b] <= left + at_edge[b + 1], (cls, b)
            left = at_edge[b + 1] - (rest[b] - left)
        assert left == 0
    # via: only where the best and the second-best candidate are more than twice the margin apart
    checked = 0
    for cls, (via, score, sign) in enumerate(((gen_via, gen_score, -1.0), (imp_via, imp_score, 1.0))):
        for k in range(n):
            cand = np.nonzero((labels != labels[k]) if cls else ((labels == labels[k]) & (np.arange(n) != k)))[0]
            order = cand[np.argsort(-sign * S[k, cand], kind="stable")]
            best, second = order[0], order[1]
            assert abs(float(score[k]) - S[k, via[k]]) <= margin[k, via[k]]
            if abs(S[k, best] - S[k, second]) > 2 * max(margin[k, best], margin[k, second]):
                assert via[k] == best, (cls, k)
                checked += 1
    assert checked > 500


# ---- through the Python layer ----------------------------------------------------------------------------------------------------------------------
def test_vector_gallery_score_distribution_with_string_labels_and_tuple_ids(ctx):
    from scrfd_arcface_facerecognition_amd import engine
    from utils.helpers import score_distribution
    g, _, _, _ = K.exact_case(300, 512)
    x = g[np.abs(g).sum(1) > 0][:200]
    rng = np.random.default_rng(2)
    ids = [(int(a), int(b)) for a, b in zip(rng.permutation(200) // 10, rng.permutation(200))]
    names = {i: (None if k % 17 == 0 else f"person {k % 9}") for k, i in enumerate(ids)}
    del names[ids[5]]                                                                 # a missing id = unlabelled
    vg = engine.VectorGallery(ctx, 512, capacity=256)
    try:
        vg.upsert(ids, x)
        res = vg.score_distribution(names, bins=64)
        order = sorted(ids)
        assert res.ids == order
        by_pos = [names.get(i) for i in order]
        want = score_distribution(x[[ids.index(i) for i in order]], by_pos, bins=64)
        for a, b in ((res.genuine, want.genuine), (res.impostor, want.impostor), (res.imp_via_pos, want.imp_via_pos), (res.gen_via_pos, want.gen_via_pos),
                     (res.imp_score_pos.view(np.uint32), want.imp_score_pos.view(np.uint32)),
                     (res.gen_score_pos.view(np.uint32), want.gen_score_pos.view(np.uint32)), (res.summary, want.summary)):
            assert np.array_equal(a, b)
        assert res.took_part == 200 - len([v for v in by_pos if v is None]) and res.genuine_pairs > 0 and res.impostor_pairs > 0
        assert res.far(-1.0) == 1.0 and res.frr(-1.0) == 0.0 and res.eer()[0] == want.eer()[0]
        top = res.hardest_impostors(3)
        assert len(top) == 3 and all(names.get(a) != names.get(b) and names.get(a) is not None for a, b, _ in top)
        assert [(order[p], order[q], s) for (p, q, s) in want.hardest_impostors(3)] == top
        sub = order[::3]
        part = vg.score_distribution(names, bins=2, ids=sub)
        assert part.ids == sub and part.genuine_pairs + part.impostor_pairs == part.took_part * (part.took_part - 1) // 2
        with pytest.raises(ValueError):
            vg.score_distribution(names, bins=3)
    finally:
        vg._gal.close()
    empty = engine.VectorGallery(ctx, 512, capacity=8)
    res = empty.score_distribution({}, bins=8)
    assert res.took_part == 0 and res.genuine.shape == (8,) and np.isnan(res.far(0.5)) and res.hardest_impostors(2) == []
    empty._gal.close()


def test_calibrate_faces_smoke(ctx, monkeypatch):
    """synthetic weights, a handful of small images: shapes and totals only"""
    monkeypatch.setenv("FID_AUTOTUNE", "0")
    from models import SCRFD
    from oracle import align as oalign
    from scrfd_arcface_facerecognition_amd import archs
    from scrfd_arcface_facerecognition_amd.app import FaceAnalysis
    from scrfd_arcface_facerecognition_amd.pipeline import calibrate_detector_bias
    from scrfd_arcface_facerecognition_amd.session import HipSession
    rng = np.random.default_rng(14)
    images = [rng.integers(0, 256, (240, 320, 3), dtype=np.uint8) for _ in range(4)]
    det_net = archs.scrfd_500m((320, 320))
    lb = np.stack([oalign.letterbox(im, (320, 320))[0] for im in images])
    det_P, _ = calibrate_detector_bias(ctx, det_net, archs.synth_params(det_net, 5), lb, target=30, max_batch=8)
    det = SCRFD("synthetic:scrfd_500m?seed=5", input_size=(320, 320), conf_thres=0.5, max_batch=8)
    det.session = HipSession(None, ctx=det.ctx, net=det_net, params=det_P, max_batch=8)
    app = FaceAnalysis("synthetic:scrfd_500m?seed=5", "synthetic:arcface_mbf?seed=5", det_size=(320, 320), max_faces=16)
    app.det = det
    images.append(np.zeros((240, 320, 3), np.uint8))                                 # (whatever the synthetic detector makes of it)
    labels = ["ann", "ann", "bob", None, "bob"]
    with_face = [b for b, fs in enumerate(app.get_batch(images, max_num=1)) if len(fs)]
    assert len(with_face) >= 4
    res = app.calibrate_faces(images, labels, bins=16)
    assert res.ids == with_face and res.genuine.shape == res.impostor.shape == (16,) and len(res.edges) == 17
    named = [labels[b] for b in with_face if labels[b] is not None]
    genuine = sum(named.count(v) * (named.count(v) - 1) // 2 for v in set(named))
    assert (res.took_part, res.genuine_pairs, res.non_finite) == (len(named), genuine, 0)
    assert res.genuine_pairs + res.impostor_pairs == len(named) * (len(named) - 1) // 2 and int(res.genuine.sum()) == genuine >= 1
    assert res.gen_via_pos[0] == 1 and res.gen_via_pos[1] == 0 and res.imp_via_pos[3] == -1 and res.gen_via_pos[3] == -1
    with pytest.raises(ValueError):
        app.calibrate_faces(images, ["ann"])
