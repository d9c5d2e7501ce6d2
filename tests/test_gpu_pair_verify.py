"""GPU: fid_pair_verify (csrc/pair_verify.hip) and the layers on it -- engine.verify_pairs, utils.helpers.compute_similarities,
FaceAnalysis.compare_pairs / process_face_comparisons.  The yardstick is tests/pair_oracle.py: the reference's formulas in float64; on the
probe rows every comparison is bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest

import pair_oracle as po
from oracle import align as oalign
from oracle import pipeline as opipe
from oracle import postprocess as pp

pytestmark = pytest.mark.gpu

TAIL = 3                                  # entries of score / verdict beyond P that must stay untouched
SCORE_FILL, VERDICT_FILL, COUNTER_FILL = np.float32(-123.25), np.int32(0x5A5A5A5A), np.int32(1000)


@pytest.fixture(scope="module")
def ctx():
    from scrfd_arcface_facerecognition_amd._lib import default_context
    return default_context(0)


class Call:
    """one fid_pair_verify call on pattern-filled outputs; `.rc`, `.score` / `.verdict` (the first P entries), `.counters`, `.untouched`"""

    def __init__(self, ctx, emb, n_rows, pairs, thresh, offsets=None, n_img=0, labels=None, counters=None, P=None, dim=None, emb_shift=0,
                 null_emb=False, null=()):
        emb = np.ascontiguousarray(emb, np.float32)
        pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        self.P = len(pairs) if P is None else P
        n = len(pairs)
        e = ctx.to_device(emb) if emb.size else ctx.empty((4,), np.float32)
        pr = ctx.to_device(pairs) if n else ctx.empty((2,), np.int32)
        off = ctx.to_device(np.ascontiguousarray(offsets, np.int32)) if offsets is not None else None
        lab = ctx.to_device(np.ascontiguousarray(labels, np.int32)) if labels is not None else None
        self.score_dev = ctx.to_device(np.full(n + TAIL, SCORE_FILL, np.float32))
        self.verdict_dev = ctx.to_device(np.full(n + TAIL, VERDICT_FILL, np.int32))
        self.counters_dev = counters if counters is not None else ctx.to_device(np.full(8, COUNTER_FILL, np.int32))
        def arg(name, buf):                                  # `null`: names of the pointers handed over as NULL
            return None if name in null else C.c_void_p(buf.ptr)
        self.rc = ctx.lib.fid_pair_verify(ctx.handle, None if null_emb else C.c_void_p(e.ptr + emb_shift), n_rows,
                                          emb.shape[1] if dim is None else dim, arg("pairs", pr), self.P, C.c_void_p(off.ptr) if off is not None else None,
                                          n_img, C.c_void_p(lab.ptr) if lab is not None else None, C.c_float(thresh), arg("score", self.score_dev),
                                          arg("verdict", self.verdict_dev), arg("counters", self.counters_dev))
        self.error = ctx.lib.fid_last_error().decode()
        s, v = self.score_dev.download(), self.verdict_dev.download()
        k = max(self.P, 0) if self.rc == 0 else 0
        self.score, self.verdict, self.counters = s[:k], v[:k], self.counters_dev.download()
        self.untouched = bool(np.all(s[k:].view(np.uint32) == SCORE_FILL.view(np.uint32)) and np.all(v[k:] == VERDICT_FILL))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def probe_set(dim, rng):
    """24 random probe rows, then partners of rows 0 .. 3 at cosine 1/2, -1/2, 0 and -1"""
    k = po.probe_k(dim)
    rows = po.probe_rows(24, dim, rng)
    extra = [po.probe_partner(rows[0], k // 2, rng), po.probe_partner(rows[1], -k // 2, rng), po.probe_partner(rows[2], 0, rng),
             po.probe_partner(rows[3], -k, rng)]
    return np.concatenate([rows, extra])


# ---- exact probes ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [4, 128, 512, 516])          # idle lanes; one round, half the lanes; two full rounds; a third round of one lane
def test_probes_are_bit_exact(ctx, dim):
    rng = np.random.default_rng(100 + dim)
    emb = probe_set(dim, rng)
    n = len(emb)
    for P in (1, 3, 4, 5, 257):                              # the four-pairs-per-workgroup seam, a partial last workgroup
        pairs = rng.integers(0, n, (P, 2)).astype(np.int32)
        pairs[0] = (5, 5)                                    # (r, r)
        if P >= 5:
            pairs[1], pairs[2], pairs[3], pairs[4] = (0, 24), (25, 1), (2, 26), (27, 3)
        ref_s, ref_v, ref_c = po.verify(emb, n, pairs, 0.5)              # (a score of exactly 1/2 is not above it)
        got = Call(ctx, emb, n, pairs, 0.5, counters=ctx.to_device(np.zeros(8, np.int32)))
        assert got.rc == 0, got.error
        assert np.array_equal(bits(got.score), bits(ref_s)), (dim, P)
        assert np.array_equal(got.verdict, ref_v) and got.untouched, (dim, P)
        assert got.score[0] == 1.0 and got.verdict[0] == po.SAME
        assert np.array_equal(got.counters, ref_c) and got.counters[0] == P and got.counters[3] == got.counters[4] == 0
        if P >= 5:
            assert got.score[1:5].tolist() == [0.5, -0.5, 0.0, -1.0] and got.verdict[1:5].tolist() == [po.DIFFERENT] * 4


def test_threshold_is_strict(ctx):
    rng = np.random.default_rng(7)
    row = po.probe_rows(1, 512, rng)[0]
    emb = np.stack([row, po.probe_partner(row, 32, rng)])
    below = np.nextafter(np.float32(0.5), np.float32(0))
    at, under = Call(ctx, emb, 2, [(0, 1)], 0.5), Call(ctx, emb, 2, [(0, 1)], float(below))
    assert at.rc == 0 and under.rc == 0
    assert at.score[0] == 0.5 and at.verdict[0] == po.DIFFERENT
    assert under.score[0] == 0.5 and under.verdict[0] == po.SAME


# ---- index handling ------------------------------------------------------------------------------------------------------

def test_row_index_form_never_reads_an_invalid_row(ctx):
    rng = np.random.default_rng(8)
    n_rows = 6
    emb = np.concatenate([probe_set(128, rng)[:n_rows], np.full((4, 128), np.nan, np.float32)])      # the allocation goes on with NaN rows
    big, small = 2 ** 31 - 1, -2 ** 31
    pairs = [(0, 1), (-1, 0), (0, -1), (-2, 0), (0, -2), (n_rows, 0), (0, n_rows), (big, 0), (0, big), (small, 0), (n_rows + 1, n_rows + 3),
             (-1, -2), (-2, -1), (n_rows, -1), (-1, big), (-1, -1), (-3, 2), (3, 3)]
    ref_s, ref_v, ref_c = po.verify(emb, n_rows, pairs, 0.4)
    got = Call(ctx, emb, n_rows, pairs, 0.4, counters=ctx.to_device(np.zeros(8, np.int32)))
    assert got.rc == 0, got.error
    assert not np.isnan(got.score).any()
    assert np.array_equal(got.verdict, ref_v) and np.array_equal(bits(got.score), bits(ref_s)) and got.untouched
    assert got.verdict.tolist() == [ref_v[0]] + [po.NO_IMAGE] * 2 + [po.NO_FACE] * 8 + [po.NO_IMAGE] * 5 + [po.NO_FACE, po.SAME]
    err = got.verdict >= po.NO_IMAGE
    assert np.array_equal(bits(got.score[err]), np.zeros(err.sum(), np.uint32))          # +0.0, bit for bit
    assert np.array_equal(got.counters, ref_c) and got.counters[3] == 7 and got.counters[4] == 9


def test_image_index_form_with_offsets(ctx):
    rng = np.random.default_rng(9)
    n_rows, n_img = 3, 6
    emb = np.concatenate([probe_set(128, rng)[:n_rows], np.full((3, 128), np.nan, np.float32)])
    offsets = np.array([0, 1, 1, 2, 3, 3, 4], np.int32)      # images 1 and 4: no face; image 5: its face is row 3 = past n_rows
    pairs = [(0, 2), (2, 3), (3, 3), (0, 1), (4, 2), (5, 0), (2, 5), (-1, 0), (0, 6), (2 ** 31 - 1, 1), (1, -2), (-1, 5), (4, -1), (1, 4)]
    labels = [1, 0, 1, 1, 0, -1, 1, 0, 1, 0, 7, 1, 0, -1]
    ref_s, ref_v, ref_c = po.verify(emb, n_rows, pairs, 0.4, offsets=offsets, n_img=n_img, labels=labels)
    got = Call(ctx, emb, n_rows, pairs, 0.4, offsets=offsets, n_img=n_img, labels=labels, counters=ctx.to_device(np.zeros(8, np.int32)))
    assert got.rc == 0, got.error
    assert not np.isnan(got.score).any()
    assert got.verdict.tolist()[3:] == [po.NO_FACE] * 4 + [po.NO_IMAGE] * 6 + [po.NO_FACE]
    assert got.verdict[2] == po.SAME and got.score[2] == 1.0
    assert np.array_equal(got.verdict, ref_v) and np.array_equal(bits(got.score), bits(ref_s)) and got.untouched
    assert np.array_equal(got.counters, ref_c) and got.counters[5] == 11
    # no image at all: the offsets are not read, every pair is a no-image error
    none = Call(ctx, np.zeros((0, 128), np.float32), 0, [(-1, -1), (0, 0)], 0.4, offsets=np.zeros(1, np.int32), n_img=0, null_emb=True,
                dim=128, counters=ctx.to_device(np.zeros(8, np.int32)))
    assert none.rc == 0 and none.verdict.tolist() == [po.NO_IMAGE] * 2 and none.counters.tolist() == [2, 0, 0, 2, 0, 0, 0, 0]
    # images, but no face in any of them (n_rows = 0, NULL embeddings)
    nof = Call(ctx, np.zeros((0, 128), np.float32), 0, [(0, 1), (-1, 1)], 0.4, offsets=np.zeros(3, np.int32), n_img=2, null_emb=True, dim=128,
               counters=ctx.to_device(np.zeros(8, np.int32)))
    assert nof.rc == 0 and nof.verdict.tolist() == [po.NO_FACE, po.NO_IMAGE] and nof.counters.tolist() == [2, 0, 0, 1, 1, 0, 0, 0]


# ---- counters ------------------------------------------------------------------------------------------------------

def test_counters_add_up_over_calls_and_labels_are_exact(ctx):
    rng = np.random.default_rng(10)
    emb = probe_set(512, rng)
    n = len(emb)
    P1, P2 = 9, 130
    pairs = rng.integers(-2, n + 1, (P1 + P2, 2)).astype(np.int32)          # -2, -1 and n among them
    labels = rng.integers(-1, 2, P1 + P2).astype(np.int32)
    counters = ctx.to_device(np.zeros(8, np.int32))
    a = Call(ctx, emb, n, pairs[:P1], 0.1, labels=labels[:P1], counters=counters)
    b = Call(ctx, emb, n, pairs[P1:], 0.1, labels=labels[P1:], counters=counters)          # no clear in between
    assert a.rc == 0 and b.rc == 0
    _, ref_v, ref_c = po.verify(emb, n, pairs, 0.1, labels=labels)
    assert np.array_equal(np.concatenate([a.verdict, b.verdict]), ref_v)
    assert np.array_equal(b.counters, ref_c)
    assert ref_c[0] == P1 + P2 and ref_c[5] == int((labels >= 0).sum()) and 0 < ref_c[6] < ref_c[5] and min(ref_c[1:5]) > 0
    assert ref_c[7] == 0
    c7 = Call(ctx, emb, n, pairs[:P1], 0.1)                  # slot 7 keeps the caller's value, the others are added to it
    assert c7.counters[7] == COUNTER_FILL and c7.counters[0] == COUNTER_FILL + P1


# ---- random embeddings, the zero row ---------------------------------------------------------------------------------

def test_random_embeddings_within_the_fp32_bound_and_reproducible(ctx):
    """|score - float64| <= 1e-4: three fp32 sums of 512 terms in any order, two square roots, a product and a quotient --
    about 2 * (512 + 3) * 2^-24 = 6.1e-5 relative to |a| |b|"""
    rng = np.random.default_rng(2026)
    emb = rng.standard_normal((64, 512)).astype(np.float32)
    emb[1] = emb[0] + 0.3 * emb[1]                           # a few pairs with a large cosine
    emb[3] = -emb[2]
    pairs = rng.integers(0, 64, (300, 2)).astype(np.int32)
    pairs[:3] = [(0, 1), (2, 3), (7, 7)]
    ref_s, ref_v, _ = po.verify(emb, 64, pairs, 0.4)
    one, two = Call(ctx, emb, 64, pairs, 0.4), Call(ctx, emb, 64, pairs, 0.4)
    assert one.rc == 0 and two.rc == 0
    d = np.abs(one.score.astype(np.float64) - ref_s)
    print("random embeddings: max |score - float64| =", d.max())
    assert d.max() <= 1e-4
    assert ref_s[0] > 0.9 and ref_s[1] < -0.999
    clear = np.abs(ref_s - np.float32(0.4)) > 1e-4
    assert np.array_equal(one.verdict[clear], ref_v[clear])
    assert np.array_equal(one.verdict, (one.score > np.float32(0.4)).astype(np.int32))
    assert np.array_equal(bits(one.score), bits(two.score)) and np.array_equal(one.verdict, two.verdict)


def test_zero_row_is_nan_and_different(ctx):
    emb = np.zeros((3, 128), np.float32)
    emb[1] = po.probe_rows(1, 128, np.random.default_rng(3))[0]
    got = Call(ctx, emb, 3, [(0, 1), (1, 0), (0, 2), (1, 1)], -1.0, labels=[0, 1, -1, 1], counters=ctx.to_device(np.zeros(8, np.int32)))
    assert got.rc == 0
    assert np.isnan(got.score[:3]).all() and got.score[3] == 1.0
    assert got.verdict.tolist() == [po.DIFFERENT] * 3 + [po.SAME]
    assert got.counters.tolist() == [4, 1, 3, 0, 0, 3, 2, 0]


# ---- validation ------------------------------------------------------------------------------------------------------

def test_invalid_arguments_enqueue_nothing(ctx):
    rng = np.random.default_rng(11)
    emb = probe_set(128, rng)
    n = len(emb)
    pairs = [(0, 1), (2, 3), (4, 5)]
    cases = [dict(P=-1), dict(n_rows=-1), dict(dim=0), dict(dim=-4), dict(dim=6), dict(dim=126), dict(emb_shift=4), dict(emb_shift=8),
             dict(null_emb=True), dict(n_img=-1, offsets=np.zeros(4, np.int32)),
             dict(null=("pairs",)), dict(null=("score",)), dict(null=("verdict",)), dict(null=("counters",))]      # a NULL table or output with P > 0
    for kw in cases:
        n_rows = kw.pop("n_rows", n)
        got = Call(ctx, emb, n_rows, pairs, 0.4, **kw)
        assert got.rc == -1 and got.error, kw
        assert got.untouched and np.all(got.counters == COUNTER_FILL), kw
    empty = Call(ctx, emb, n, pairs, 0.4, P=0)               # no pair: OK, no launch
    assert empty.rc == 0 and empty.untouched and np.all(empty.counters == COUNTER_FILL)
    assert Call(ctx, emb, n, pairs, 0.4, P=0, null=("pairs", "score", "verdict", "counters")).rc == 0      # ... whatever the pointers are
    good = Call(ctx, emb, n, pairs, 0.4)
    assert good.rc == 0 and good.untouched and good.counters[0] == COUNTER_FILL + 3


# ---- the host layers on embeddings ------------------------------------------------------------------------------------

def test_verify_pairs_and_compute_similarities(ctx):
    from scrfd_arcface_facerecognition_amd.engine import verify_pairs
    from utils.helpers import compute_similarities
    rng = np.random.default_rng(12)
    emb = probe_set(512, rng)
    ia, ib = rng.integers(0, len(emb), 37), rng.integers(0, len(emb), 37)
    ia[:2], ib[:2] = (0, 25), (24, 1)
    labels = rng.integers(-1, 2, 37)
    f1, f2 = emb[ia], emb[ib]
    ref = np.array([po.similarity64(a, b) for a, b in zip(f1, f2)])
    score, verdict, counters = verify_pairs(ctx, f1, f2, 0.3, labels)
    assert score.dtype == np.float32 and np.array_equal(bits(score), bits(ref)) and score[0] == 0.5 and score[1] == -0.5
    assert np.array_equal(verdict, (ref > np.float32(0.3)).astype(np.int32))
    want = [37, int(verdict.sum()), 37 - int(verdict.sum()), 0, 0, int((labels >= 0).sum()), int(((labels >= 0) & (labels == verdict)).sum()), 0]
    assert counters.tolist() == want
    sims = compute_similarities(f1, f2, ctx=ctx)
    assert sims.dtype == np.float32 and sims.shape == (37,) and np.array_equal(bits(sims), bits(ref))
    e0, v0, c0 = verify_pairs(ctx, np.zeros((0, 512), np.float32), np.zeros((0, 512), np.float32))
    assert e0.shape == (0,) and v0.shape == (0,) and not c0.any()


# ---- end to end: image pairs to verdicts ---------------------------------------------------------------------------------

DET_SHAPES = [(320, 320), (240, 427), (427, 240), (640, 640), (97, 33), (320, 320)]


def read_heads(cn, B):
    """the nine head tensors of every frame of the compiled net's last run, in the ONNX output order"""
    fused = {name: cn.read(name, B) for name in cn.low.outputs}
    per_frame = []
    for b in range(B):
        heads = []
        for part in range(3):
            for name in cn.low.outputs:
                h = cn.low.heads[name]
                off, c = (h["score"], h["bbox"], h["kps"])[part]
                heads.append(np.ascontiguousarray(fused[name][b][..., off:off + 2 * c]).reshape(-1, c))
        per_frame.append(heads)
    return per_frame


@pytest.fixture(scope="module")
def heuristic_plans():
    """nets created inside these tests take the heuristic kernel plans: no timing runs, and one batch size -> one set of kernels"""
    old = os.environ.get("FID_AUTOTUNE")
    os.environ["FID_AUTOTUNE"] = "0"
    yield
    if old is None:
        del os.environ["FID_AUTOTUNE"]
    else:
        os.environ["FID_AUTOTUNE"] = old


@pytest.fixture(scope="module")
def pair_app(ctx, heuristic_plans):
    """the recipe of test_gpu_mixed_sizes.py::mixed_detector: SCRFD-500M at 320x320, max_batch 8, cls bias calibrated on the letterboxed
    images; arcface_mbf behind it with max_faces 16, so a chunk is 4 pairs = 8 images"""
    from models import SCRFD
    from scrfd_arcface_facerecognition_amd import archs
    from scrfd_arcface_facerecognition_amd.app import FaceAnalysis
    from scrfd_arcface_facerecognition_amd.pipeline import calibrate_detector_bias
    from scrfd_arcface_facerecognition_amd.session import HipSession
    rng = np.random.default_rng(14)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in DET_SHAPES]
    det_net = archs.scrfd_500m((320, 320))
    lb = np.stack([oalign.letterbox(im, (320, 320))[0] for im in images])
    det_P, _ = calibrate_detector_bias(ctx, det_net, archs.synth_params(det_net, 5), lb, target=30, max_batch=8)
    det = SCRFD("synthetic:scrfd_500m?seed=5", input_size=(320, 320), conf_thres=0.5, max_batch=8)
    det.session = HipSession(None, ctx=det.ctx, net=det_net, params=det_P, max_batch=8)
    app = FaceAnalysis("synthetic:scrfd_500m?seed=5", "synthetic:arcface_mbf?seed=5", det_size=(320, 320), max_faces=16)
    assert app.ctx is det.ctx
    app.det = det
    return app, images


def test_compare_pairs_end_to_end(pair_app):
    from scrfd_arcface_facerecognition_amd.pipeline import pair_image_table
    app, im = pair_app
    det, rec = app.det, app.rec
    rec_net, rec_P = rec.session.net, rec.session.params
    cn = det.session.compiled((320, 320))
    blank = np.zeros((200, 300, 3), np.uint8)
    flipped = np.ascontiguousarray(im[0][::-1])
    # 5 pairs = 10 image slots: a chunk of 4 pairs (mixed sizes, one slot empty) and a chunk of 1 pair (two 320 x 320 images: the uniform path)
    A = [im[1], im[2], im[3], None, im[5]]
    B = [im[4], im[2], blank, im[0], flipped]
    labels = [True, False, True, None, False]
    T = 0.99                                                 # (random images through random weights: every cosine is high; this one tells the pairs apart)
    P = len(A)
    # which images have a face at all: conf_thres between the blank image's best score and the weakest of the others (GPU heads)
    det._detect_chunk_ragged(im + [blank, flipped], 0, "max")
    mx = [max(float(h.max()) for h in heads[:3]) for heads in read_heads(cn, 8)]
    print("best score per image:", mx)
    assert mx[6] + 0.02 < min(mx[:6] + mx[7:]), mx
    thr = float((mx[6] + min(mx[:6] + mx[7:])) / 2)
    old_thr = det.conf_thres
    try:
        det.conf_thres = thr
        res, counters = app.compare_pairs(A, B, T, labels=labels, return_embeddings=True)
        assert len(res) == P
        # 1. / 2. per chunk: the same batch once more (same kernels, same bits), the oracle's post-process on its heads, the oracle's embedding
        present = ([x is not None for x in A], [x is not None for x in B])
        sides = (A, B)
        n_checked = 0
        for p0 in (0, 4):
            run, table = pair_image_table(present[0], present[1], p0, min(p0 + 4, P))
            imgs = [sides[s][p] for p, s in run]
            assert len(imgs) == (7, 2)[p0 // 4]
            if len({x.shape for x in imgs}) > 1:
                det._detect_chunk_ragged(imgs, 0, "max")
            else:
                det._detect_chunk(np.stack(imgs), 0, "max")
            heads = read_heads(cn, len(imgs))
            for i, (p, s) in enumerate(run):
                odet, okps = pp.detect_from_heads(heads[i], imgs[i].shape[:2], (320, 320), thr, 0.4, 0, "max")
                e, bb = res[p][f"embedding{s + 1}"], res[p][f"bbox{s + 1}"]
                assert (len(odet) > 0) == (imgs[i] is not blank), (p, s)
                if not len(odet):
                    assert e is None and bb is None, (p, s)
                    continue
                assert np.array_equal(bb, odet[0]), (p, s)                   # faces[0]: the first NMS survivor
                ref, _ = opipe.embed(imgs[i], okps[0], rec_net, rec_P)
                assert e.shape == (512,) and e.dtype == np.float32
                assert 1 - po.similarity64(ref, e) < 1e-3, (p, s)
                n_checked += 1
        assert n_checked == 8
        # 3. / 4. / 5. the records
        assert [r["error"] for r in res] == [None, None, po.ERR_NO_FACE, po.ERR_NO_IMAGE, None]
        for p, r in enumerate(res):
            assert set(r) == {"same_person", "confidence", "threshold_used", "error", "embedding1", "embedding2", "bbox1", "bbox2"}
            assert r["threshold_used"] == T and isinstance(r["same_person"], bool) and isinstance(r["confidence"], float)
            if r["error"]:
                assert r["same_person"] is False and r["confidence"] == 0.0
                continue
            want = po.similarity64(r["embedding1"], r["embedding2"])
            print("pair", p, "confidence", r["confidence"], "float64 on the returned embeddings", want)
            assert abs(r["confidence"] - want) <= 1e-4, p
            assert r["same_person"] == bool(np.float32(r["confidence"]) > np.float32(T)), p
        assert res[3]["embedding1"] is None and res[3]["embedding2"] is not None  # (the second image of a pair without its first one still ran)
        assert res[2]["embedding1"] is not None and res[2]["embedding2"] is None
        assert res[1]["confidence"] >= 1 - 1e-3 and res[1]["same_person"] is True
        same = [r["same_person"] for r in res]
        n_same = sum(same)
        agree = sum(1 for v, s in zip(labels, same) if v is not None and v == s)
        assert counters == {"processed": 5, "same_person": n_same, "different_person": 3 - n_same, "no_image": 1, "no_face": 1, "errors": 2,
                            "labelled": 4, "label_matches": agree}
        # without return_embeddings: the same records, nothing else
        plain, counters2 = app.compare_pairs(A, B, T, labels=labels)
        assert counters2 == counters
        for r, q in zip(res, plain):
            assert set(q) == {"same_person", "confidence", "threshold_used", "error"}
            assert all(q[k] == r[k] for k in q), (q, r)
        # 6. process_face_comparisons with a dict loader
        store = {f"a{p}": A[p] for p in range(P)}
        store.update({f"b{p}": B[p] for p in range(P)})
        records = [{"comparison_id": 100 + p, "event_id": p, "branch_id": 1, "created_at": "2024-01-01", "customer_info": {"n": p}, "matched_info": {},
                    "approve": labels[p], "image1_url": f"a{p}", "image2_url": f"b{p}", "raw_data": {"k": p}} for p in range(P)]
        out = app.process_face_comparisons(records, loader=store.get, threshold=T)
        ref = po.summary(records, res)
        assert set(out) == set(ref) == {"total_comparisons", "processed", "same_person", "different_person", "errors", "accuracy_vs_api", "api_matches",
                                        "total_with_api_data", "results"}
        for k in ref:
            if k != "results":
                assert out[k] == ref[k], k
        assert out["total_with_api_data"] == 5 and out["accuracy_vs_api"] == ref["api_matches"] / 5 * 100
        fields = {"comparison_id", "event_id", "branch_id", "created_at", "customer_info", "matched_info", "api_approve", "our_result", "confidence",
                  "threshold_used", "image1_url", "image2_url", "error", "match_status", "api_vs_our_match", "raw_data"}
        for p, (o, r, w) in enumerate(zip(out["results"], res, ref["results"])):
            assert set(o) == fields
            assert o["comparison_id"] == 100 + p and o["raw_data"] == {"k": p} and o["image1_url"] == f"a{p}"
            assert o["our_result"] == r["same_person"] and o["confidence"] == r["confidence"] and o["error"] == r["error"]
            assert all(o[k] == w[k] for k in w), (o, w)
        two = app.process_face_comparisons(records, loader=store.get, max_comparisons=2, threshold=T)
        assert two["total_comparisons"] == 2 and two["processed"] == 2 and two["errors"] == 0
        assert app.process_face_comparisons([]) == {"total_comparisons": 0, "processed": 0, "same_person": 0, "different_person": 0, "errors": 0,
                                                    "results": []}
    finally:
        det.conf_thres = old_thr
