"""GPU: mixed-size image batches (fid_letterbox_ragged / fid_scrfd_postprocess_ragged / fid_align_crops_ragged /
fid_align_crops_packed_ragged, SCRFD.detect_batch / FaceAnalysis.get_batch / build_targets_from_images on lists of differing shapes).
The yardsticks are the uniform entry points called per image with B = 1, the oracle, and the reference-generated goldens; every
comparison is bit for bit unless it says otherwise."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import dense_heads, load_golden
from oracle import align as oalign
from oracle import pipeline as opipe
from oracle import postprocess as pp

pytestmark = pytest.mark.gpu

LB_SHAPES = [(1080, 1920), (640, 640), (1280, 1280), (480, 853), (853, 480), (700, 500), (641, 639), (97, 33), (33, 97), (5, 7)]
ORACLE_SHAPES = [(1080, 1920), (480, 853), (1280, 1280), (640, 640), (700, 500), (853, 480)]
PAD = 2          # bytes in front of the first image: no offset of the letterbox batch is a multiple of 4 (residues 1, 2 and 3 all occur)


@pytest.fixture(scope="module")
def ctx():
    from scrfd_arcface_facerecognition_amd._lib import default_context
    return default_context(0)


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


def _i32(a):
    from scrfd_arcface_facerecognition_amd._lib import c_i32_p
    return a.ctypes.data_as(c_i32_p)


def _i64(a):
    from scrfd_arcface_facerecognition_amd._lib import c_i64_p
    return a.ctypes.data_as(c_i64_p)


# ---- 1. letterbox ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lb_batch(ctx):
    """the ten images as ONE allocation: PAD bytes, then the images in LB_SHAPES order; the last pixel of the (5,7) image is the last
    byte of the allocation"""
    from scrfd_arcface_facerecognition_amd._lib import pack_images
    rng = np.random.default_rng(11)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in LB_SHAPES]
    buf, hw, offsets = pack_images(images)
    offsets = offsets + PAD
    assert {int(o) % 4 for o in offsets} == {1, 2, 3}              # (641,639), (97,33) and (33,97) have odd sizes, so the residue moves
    host = np.concatenate([np.full(PAD, 0xEE, np.uint8), buf])
    assert int(offsets[-1]) + 5 * 7 * 3 == host.nbytes
    return images, ctx.to_device(host), host.nbytes, hw, offsets


def letterbox_per_image(ctx, image, in_h, in_w):
    """the yardstick: fid_letterbox with B = 1"""
    from scrfd_arcface_facerecognition_amd._lib import check
    fr = ctx.to_device(image[None])
    out = ctx.empty((1, in_h, in_w, 3), np.uint8)
    sc = C.c_double()
    check(ctx.lib.fid_letterbox(ctx.handle, C.c_void_p(fr.ptr), 1, image.shape[0], image.shape[1], C.c_void_p(out.ptr), in_h, in_w,
                                C.byref(sc)))
    return out.download()[0], sc.value


@pytest.mark.parametrize("in_h, in_w", [(640, 640), (64, 96), (63, 95)])       # the 4-pixel kernel, the byte kernel twice
def test_letterbox_equals_per_image_calls(ctx, lb_batch, in_h, in_w):
    from scrfd_arcface_facerecognition_amd._lib import check
    images, frames, nbytes, hw, offsets = lb_batch
    B = len(images)
    out = ctx.empty((B, in_h, in_w, 3), np.uint8)
    scales = np.zeros(B, np.float64)
    check(ctx.lib.fid_letterbox_ragged(ctx.handle, C.c_void_p(frames.ptr), nbytes, _i32(hw), _i64(offsets), B, C.c_void_p(out.ptr),
                                       in_h, in_w, scales.ctypes.data_as(C.POINTER(C.c_double))))
    got = out.download()
    for b, im in enumerate(images):
        ref, sc = letterbox_per_image(ctx, im, in_h, in_w)
        assert scales[b] == sc, (b, LB_SHAPES[b])
        assert np.array_equal(got[b], ref), (b, LB_SHAPES[b])
        if in_h == 640 and LB_SHAPES[b] in ORACLE_SHAPES:
            oref, osc = oalign.letterbox(im)
            assert osc == scales[b] and np.array_equal(got[b], oref), (b, LB_SHAPES[b])


def test_letterbox_two_calls_back_to_back_use_their_own_tables(ctx, lb_batch):
    """the list and its reverse, no synchronisation in between, and the host arrays overwritten as soon as each call has returned"""
    from scrfd_arcface_facerecognition_amd._lib import check
    images, frames, nbytes, hw, offsets = lb_batch
    B, in_h, in_w = len(images), 64, 96
    refs = [letterbox_per_image(ctx, im, in_h, in_w)[0] for im in images]
    for in_w_k in (96, 95):                                # both kernel forms (in_w % 4)
        refs_k = refs if in_w_k == 96 else [letterbox_per_image(ctx, im, in_h, in_w_k)[0] for im in images]
        out1, out2 = ctx.empty((B, in_h, in_w_k, 3), np.uint8), ctx.empty((B, in_h, in_w_k, 3), np.uint8)
        ctx.sync()
        hw1, off1 = hw.copy(), offsets.copy()
        hw2, off2 = hw[::-1].copy(), offsets[::-1].copy()
        rc1 = ctx.lib.fid_letterbox_ragged(ctx.handle, C.c_void_p(frames.ptr), nbytes, _i32(hw1), _i64(off1), B, C.c_void_p(out1.ptr),
                                           in_h, in_w_k, None)
        hw1[:] = 1; off1[:] = 0
        rc2 = ctx.lib.fid_letterbox_ragged(ctx.handle, C.c_void_p(frames.ptr), nbytes, _i32(hw2), _i64(off2), B, C.c_void_p(out2.ptr),
                                           in_h, in_w_k, None)
        hw2[:] = 1; off2[:] = 0
        check(rc1), check(rc2)
        got1, got2 = out1.download(), out2.download()
        for b in range(B):
            assert np.array_equal(got1[b], refs_k[b]), (in_w_k, b)
            assert np.array_equal(got2[b], refs_k[B - 1 - b]), (in_w_k, b)


# ---- 2. validation -----------------------------------------------------------------------------------------

def test_validation_is_all_or_nothing(ctx):
    rng = np.random.default_rng(12)
    shapes = [(40, 30), (9, 11), (16, 16)]
    from scrfd_arcface_facerecognition_amd._lib import pack_images
    buf, hw, offsets = pack_images([rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes])
    frames = ctx.to_device(buf)
    pattern = np.tile(np.arange(251, dtype=np.uint8), 64 * 96 * 3 * 3 // 251 + 1)[:3 * 64 * 96 * 3].reshape(3, 64, 96, 3)
    out = ctx.to_device(pattern)

    def call(hw_, off_, nbytes=buf.nbytes):
        rc = ctx.lib.fid_letterbox_ragged(ctx.handle, C.c_void_p(frames.ptr), nbytes, _i32(hw_), _i64(off_), 3, C.c_void_p(out.ptr), 64, 96, None)
        return rc, ctx.lib.fid_last_error().decode()

    cases = []
    h = hw.copy(); h[1, 0] = 0                                           # a zero dimension
    cases.append((h, offsets, buf.nbytes, 1))
    h = hw.copy(); h[2, 1] = -4
    cases.append((h, offsets, buf.nbytes, 2))
    o = offsets.copy(); o[2] = buf.nbytes + 5                            # an offset past the end
    cases.append((hw, o, buf.nbytes, 2))
    o = offsets.copy(); o[0] = -1
    cases.append((hw, o, buf.nbytes, 0))
    cases.append((hw, offsets, buf.nbytes - 1, 2))                       # offsets[b] + size == frames_bytes + 1
    o = offsets.copy(); o[1] = buf.nbytes + 1 - 9 * 11 * 3
    cases.append((hw, o, buf.nbytes, 1))
    h = hw.copy(); h[1] = (2, 640); o = offsets.copy(); o[1] = 0         # (2,640) into 64x96: new_h == 0 (2*640*3 bytes lie inside)
    assert 2 * 640 * 3 <= buf.nbytes
    cases.append((h, o, buf.nbytes, 1))
    for hw_, off_, nbytes, idx in cases:
        rc, msg = call(np.ascontiguousarray(hw_), np.ascontiguousarray(off_), nbytes)
        assert rc == -1 and f"image {idx}:" in msg, (idx, rc, msg)
    # the warp and the post-process validate the same way
    kp, cn, crops = ctx.to_device(np.zeros((3, 1, 10), np.float32)), ctx.to_device(np.zeros(3, np.int32)), ctx.empty((3, 112, 112, 3), np.uint8)
    h = hw.copy(); h[2, 0] = 0
    assert ctx.lib.fid_align_crops_ragged(ctx.handle, C.c_void_p(frames.ptr), buf.nbytes, _i32(h), _i64(offsets), 3, C.c_void_p(kp.ptr),
                                          C.c_void_p(cn.ptr), 1, 1, C.c_void_p(crops.ptr), None) == -1
    assert "image 2:" in ctx.lib.fid_last_error().decode()
    assert ctx.lib.fid_align_crops_packed_ragged(ctx.handle, C.c_void_p(frames.ptr), buf.nbytes - 1, _i32(hw), _i64(offsets), 3, C.c_void_p(kp.ptr),
                                                 1, C.c_void_p(cn.ptr), 3, C.c_void_p(crops.ptr), None) == -1
    assert "image 2:" in ctx.lib.fid_last_error().decode()
    assert np.array_equal(out.download(), pattern)                       # nothing was enqueued
    rc, _ = call(hw, offsets)                                            # ... and the good batch runs
    assert rc == 0 and not np.array_equal(out.download(), pattern)


# ---- 3. post-process ---------------------------------------------------------------------------------------

def run_post_ragged(ctx, heads_per_frame, hw, max_num=0, metric=0, conf=0.5, iou=0.4, cap=1024):
    from scrfd_arcface_facerecognition_amd.engine import HeadViews, PostProcessor
    B = len(heads_per_frame)
    bufs = [ctx.to_device(np.stack([h[k] for h in heads_per_frame])) for k in range(9)]
    post = PostProcessor(ctx, B, cap=cap, cand_cap=4096)
    post.run_ragged(HeadViews.from_onnx_layout(bufs), B, (640, 640), np.asarray(hw, np.int32), conf, iou, max_num, metric)
    return post.fetch(B)


def test_postprocess_goldens_as_ragged_batches(ctx):
    """tests/golden/detect.npz: the 16 cases of each (max_num, metric) -- four image sizes, det_scale 1, 1/3, 1/2, 3/4 -- as ONE batch"""
    g = load_golden("detect.npz")
    groups = {}
    for ci in range(int(g["n_cases"])):
        groups.setdefault((int(g[f"c{ci}_max_num"]), int(g[f"c{ci}_metric"])), []).append(ci)
    assert sorted(groups) == [(0, 0), (1, 0), (3, 0), (3, 1)] and all(len(v) == 16 for v in groups.values())
    for (max_num, metric), cases in groups.items():
        heads = [dense_heads(g[f"c{ci}_pos"], g[f"c{ci}_pos_score"], g[f"c{ci}_pos_bbox"], g[f"c{ci}_pos_kps"]) for ci in cases]
        hw = [tuple(int(v) for v in g[f"c{ci}_shape"]) for ci in cases]
        assert len(set(hw)) == 4
        res = run_post_ragged(ctx, heads, hw, max_num, metric)
        for ci, (det, kps) in zip(cases, res):
            assert det.shape == g[f"c{ci}_det"].shape and kps.shape == g[f"c{ci}_kps"].shape, ci
            assert np.array_equal(det, g[f"c{ci}_det"]), ci
            assert np.array_equal(kps, g[f"c{ci}_kps"]), ci


def test_postprocess_portrait_and_tiny_sizes_match_oracle(ctx):
    """the six random head sets of test_gpu_postprocess.py::test_batched_frames_match_oracle, each frame with its own image size"""
    rng = np.random.default_rng(0)
    frames = []
    for b in range(6):
        K = [0, 3, 40, 400, 1500, 90][b]
        total = 16800
        scores = rng.uniform(0.0, 0.45, total).astype(np.float32)
        pos = rng.choice(total, K, replace=False)
        scores[pos] = rng.permutation(np.linspace(0.5, 0.99, max(K, 1)))[:K].astype(np.float32)
        bbox = rng.uniform(-1, 8, (total, 4)).astype(np.float32)
        kps = rng.uniform(-6, 6, (total, 10)).astype(np.float32)
        o = np.cumsum([0, 12800, 3200, 800])
        frames.append([scores[o[i]:o[i + 1], None] for i in range(3)] + [bbox[o[i]:o[i + 1]] for i in range(3)]
                      + [kps[o[i]:o[i + 1]] for i in range(3)])
    hw = [(853, 480), (97, 33), (1080, 1920), (640, 640), (33, 97), (700, 500)]
    for max_num, metric in ((0, "max"), (2, "max"), (5, "default")):
        res = run_post_ragged(ctx, frames, hw, max_num, 0 if metric == "max" else 1)
        for b, (det, kps) in enumerate(res):
            odet, okps = pp.detect_from_heads(frames[b], hw[b], max_num=max_num, metric=metric)
            assert np.array_equal(det, odet), (b, max_num)
            assert np.array_equal(kps, okps), (b, max_num)


# ---- 4. warp -----------------------------------------------------------------------------------------------

def test_warp_equals_per_image_calls_and_oracle(ctx):
    from scrfd_arcface_facerecognition_amd._lib import check
    rng = np.random.default_rng(13)
    shapes = [(480, 640), (97, 33), (1080, 1920), (200, 300)]
    counts = np.array([2, 1, 0, 2], np.int32)
    B, F = len(shapes), 2
    images = [rng.integers(1, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]
    lms = load_golden("umeyama.npz")["landmarks"].astype(np.float64)
    kps = np.zeros((B, F, 10), np.float32)
    for b, (H, W) in enumerate(shapes):
        for f in range(F):
            lm = lms[7 * b + 3 * f + 1]
            # scaled so that the lowest / rightmost landmark lies on the image border: the crop's margin around the landmarks samples outside
            kps[b, f] = (lm * min(W / lm[:, 0].max(), H / lm[:, 1].max())).astype(np.float32).reshape(-1)
        n_out = sum(int(oalign.norm_crop_image(np.full((H, W, 3), 255, np.uint8), kps[b, f].reshape(5, 2)).min() < 255) for f in range(int(counts[b])))
        assert n_out >= 1 or counts[b] == 0, b              # BORDER_CONSTANT taps in at least one face of the image
    batch = ctx.image_batch(images)
    kp, cn = ctx.to_device(kps), ctx.to_device(counts)
    crops, M = ctx.empty((B * F, 112, 112, 3), np.uint8), ctx.empty((B * F, 6), np.float64)
    check(ctx.lib.fid_align_crops_ragged(ctx.handle, *batch.args(), B, C.c_void_p(kp.ptr), C.c_void_p(cn.ptr), F, F, C.c_void_p(crops.ptr),
                                         C.c_void_p(M.ptr)))
    got, gotM = crops.download().reshape(B, F, 112, 112, 3), M.download().reshape(B, F, 6)
    for b, im in enumerate(images):
        fr = ctx.to_device(im[None])
        kp1, cn1 = ctx.to_device(kps[b:b + 1]), ctx.to_device(counts[b:b + 1])
        c1, M1 = ctx.empty((F, 112, 112, 3), np.uint8), ctx.empty((F, 6), np.float64)
        check(ctx.lib.fid_align_crops(ctx.handle, C.c_void_p(fr.ptr), 1, im.shape[0], im.shape[1], C.c_void_p(kp1.ptr), C.c_void_p(cn1.ptr),
                                      F, F, C.c_void_p(c1.ptr), C.c_void_p(M1.ptr)))
        assert np.array_equal(got[b], c1.download()), b
        assert np.array_equal(gotM[b], M1.download()), b
        for f in range(F):
            if f < counts[b]:
                ref = oalign.norm_crop_image(im, kps[b, f].reshape(5, 2))
                assert np.array_equal(got[b, f], ref) and ref.max() > 0, (b, f)
            else:
                assert not got[b, f].any() and not gotM[b, f].any(), (b, f)
    # packed form: rows in shuffled cross-frame order, two empty rows, 7 rows
    src = np.array([3 * F + 1, 0 * F + 0, -1, 1 * F + 0, 3 * F + 0, -1, 0 * F + 1], np.int32)
    n = len(src)
    sd = ctx.to_device(src)
    pc, pM = ctx.empty((n, 112, 112, 3), np.uint8), ctx.empty((n, 6), np.float64)
    check(ctx.lib.fid_align_crops_packed_ragged(ctx.handle, *batch.args(), B, C.c_void_p(kp.ptr), F, C.c_void_p(sd.ptr), n, C.c_void_p(pc.ptr),
                                                C.c_void_p(pM.ptr)))
    pc, pM = pc.download(), pM.download()
    for i, s in enumerate(src):
        if s < 0:
            assert not pc[i].any() and not pM[i].any(), i
        else:
            assert np.array_equal(pc[i], got[s // F, s % F]) and np.array_equal(pM[i], gotM[s // F, s % F]), i


# ---- 5. / 6. the Python layer on mixed lists -----------------------------------------------------------------

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
def mixed_detector(ctx, heuristic_plans):
    """SCRFD-500M at 320x320, max_batch 8, its cls bias calibrated on the oracle-letterboxed DET_SHAPES images: every one of them has
    candidates by construction"""
    from models import SCRFD
    from scrfd_arcface_facerecognition_amd import archs
    from scrfd_arcface_facerecognition_amd.pipeline import calibrate_detector_bias
    from scrfd_arcface_facerecognition_amd.session import HipSession
    rng = np.random.default_rng(14)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in DET_SHAPES]
    det_net = archs.scrfd_500m((320, 320))
    lb = np.stack([oalign.letterbox(im, (320, 320))[0] for im in images])
    det_P, _ = calibrate_detector_bias(ctx, det_net, archs.synth_params(det_net, 5), lb, target=30, max_batch=8)
    det = SCRFD("synthetic:scrfd_500m?seed=5", input_size=(320, 320), conf_thres=0.5, max_batch=8)
    det.session = HipSession(None, ctx=det.ctx, net=det_net, params=det_P, max_batch=8)
    return det, images


def test_detect_batch_mixed_list_equals_oracle_on_the_gpu_heads(mixed_detector):
    det, images = mixed_detector
    cn = det.session.compiled((320, 320))
    for max_num, metric in ((0, "max"), (1, "max"), (3, "default")):
        res = det.detect_batch(images, max_num=max_num, metric=metric)
        assert len(res) == len(images)
        heads = read_heads(cn, len(images))
        for b, (d, k) in enumerate(res):
            odet, okps = pp.detect_from_heads(heads[b], DET_SHAPES[b], (320, 320), det.conf_thres, 0.4, max_num, metric)
            assert len(d) >= 1, b
            assert d.dtype == np.float32 and k.dtype == np.float32 and k.shape == (len(d), 5, 2)
            assert np.array_equal(d, odet) and np.array_equal(k, okps), (b, max_num)


def test_ragged_chunk_of_one_shape_equals_the_uniform_chunk(mixed_detector):
    """same batch, same detector bytes, same kernels: exactly equal"""
    det, _ = mixed_detector
    rng = np.random.default_rng(15)
    for shape in ((240, 427), (320, 320)):                 # letterboxed, and the shape the uniform path hands to the net as it is
        images = [rng.integers(0, 256, shape + (3,), dtype=np.uint8) for _ in range(6)]
        for max_num, metric in ((0, "max"), (2, "default")):
            uni = det._detect_chunk(np.stack(images), max_num, metric)
            rag = det._detect_chunk_ragged(images, max_num, metric)
            assert len(uni) == len(rag) == 6
            assert sum(len(d) for d, _ in uni) > 0
            for (d0, k0), (d1, k1) in zip(uni, rag):
                assert np.array_equal(d0, d1) and np.array_equal(k0, k1)
        assert all(np.array_equal(a[0], b[0]) for a, b in zip(det.detect_batch(images), det._detect_chunk(np.stack(images), 0, "max")))


def close_to(got, one):
    """the project's batch-n against batch-1 tolerance (test_gpu_models_api.py:91-96): confident boxes within 1.0 px and 5e-3 in score"""
    strong = one[one[:, 4] > 0.55]
    for row in strong:
        if not len(got):
            return -1
        dist = np.abs(got[:, :4] - row[:4]).max(axis=1)
        j = int(dist.argmin())
        if not (dist[j] < 1.0 and abs(got[j, 4] - row[4]) < 5e-3):
            return -1
    return len(strong)


def test_detect_batch_eleven_mixed_images_in_input_order(mixed_detector):
    det, images = mixed_detector
    many = images + [np.ascontiguousarray(im[::-1]) for im in images[:5]]      # 11 images: a chunk of 8, a chunk of 3
    assert len(many) == 11
    res = det.detect_batch(many)
    assert len(res) == 11
    n_strong = 0
    for im, (d, _) in zip(many, res):
        k = close_to(d, det.detect(im)[0])
        assert k >= 0
        n_strong += k
    assert n_strong >= 1
    # ... and exactly what the two chunks give on their own: the same batches through the same kernels
    for (d, k), (d0, k0) in zip(res, det._detect_chunk_ragged(many[:8], 0, "max") + det._detect_chunk_ragged(many[8:], 0, "max")):
        assert np.array_equal(d, d0) and np.array_equal(k, k0)


def test_get_batch_and_build_targets_on_mixed_lists(ctx, mixed_detector, caplog):
    import logging
    from scrfd_arcface_facerecognition_amd.app import FaceAnalysis
    from scrfd_arcface_facerecognition_amd.pipeline import build_targets_from_images
    det, images = mixed_detector
    images = [images[1], np.zeros((200, 300, 3), np.uint8), images[2], images[4], images[0]]
    shapes = [im.shape[:2] for im in images]
    names = ["alice", "blank", "bob", "carol", "dave"]
    B = len(images)
    # which images have a face at all: conf_thres into the widest gap of the per-image score maxima of the GPU heads
    cn = det.session.compiled((320, 320))
    old_thr = det.conf_thres
    det._detect_chunk_ragged(images, 0, "max")
    mx = [max(float(h.max()) for h in heads[:3]) for heads in read_heads(cn, B)]
    srt = np.sort(mx)
    k = int(np.argmax(srt[1:] - srt[:-1]))
    assert srt[k + 1] - srt[k] > 0.02, mx
    thr = float((srt[k] + srt[k + 1]) / 2)
    has_face = [m > thr for m in mx]
    assert any(has_face) and not all(has_face), mx
    app = FaceAnalysis("synthetic:scrfd_500m?seed=5", "synthetic:arcface_mbf?seed=5", det_size=(320, 320), max_faces=16)
    assert app.ctx is det.ctx
    app.det = det                                            # the calibrated detector
    rec = app.rec
    rec_net, rec_P = rec.session.net, rec.session.params
    try:
        det.conf_thres = thr
        faces = app.get_batch(images, max_num=2)
        heads = read_heads(cn, B)
        assert len(faces) == B
        oracle_emb = {}
        for b, fl in enumerate(faces):
            odet, okps = pp.detect_from_heads(heads[b], shapes[b], (320, 320), thr, 0.4, 2, "max")
            assert (len(fl) > 0) == has_face[b] and len(fl) == len(odet), b
            one = app.get(images[b], max_num=0)
            if len(fl):
                got = np.array([list(f.bbox) + [f.det_score] for f in fl], np.float32)
                ref1 = np.array([list(f.bbox) + [f.det_score] for f in one], np.float32).reshape(-1, 5)
                assert close_to(ref1, got) >= 0, b          # every confident face of the batch is a face of app.get(image)
            for i, f in enumerate(fl):
                assert np.array_equal(f.bbox, odet[i, :4]) and f.det_score == odet[i, 4] and np.array_equal(f.kps, okps[i]), (b, i)
                ref, _ = opipe.embed(images[b], okps[i], rec_net, rec_P)
                oracle_emb[okps[i].tobytes()] = ref
                assert f.embedding.shape == (512,) and 1 - float(ref @ f.embedding / np.linalg.norm(ref) / np.linalg.norm(f.embedding)) < 1e-3, (b, i)
                assert abs(np.linalg.norm(f.normed_embedding) - 1) < 2e-3
                assert set(f.quality) == {"overall", "blur", "pose", "lighting", "size"} and isinstance(f.is_side_face, bool)
                for g in one:                                # the same face from app.get(image): batch-1 kernels, fp16 noise
                    if np.abs(g.kps - f.kps).max() < 0.25:
                        assert 1 - float(g.embedding @ f.embedding / np.linalg.norm(g.embedding) / np.linalg.norm(f.embedding)) < 1e-3
        # build_targets_from_images: names, order and the skip warning are exact
        with caplog.at_level(logging.WARNING):
            targets = build_targets_from_images(det, rec, images, names)
        heads = read_heads(cn, B)
        assert [t[1] for t in targets] == [nm for nm, h in zip(names, has_face) if h]
        warned = [r.getMessage() for r in caplog.records if "No face detected" in r.getMessage()]
        assert warned == [f"No face detected in {nm}. Skipping..." for nm, h in zip(names, has_face) if not h]
        ti = 0
        for b in range(B):
            if not has_face[b]:
                continue
            odet, okps = pp.detect_from_heads(heads[b], shapes[b], (320, 320), thr, 0.4, 1, "max")
            assert len(okps) == 1
            ref = oracle_emb.get(okps[0].tobytes())
            if ref is None:
                ref, _ = opipe.embed(images[b], okps[0], rec_net, rec_P)
            e = targets[ti][0]
            assert e.shape == (512,) and e.dtype == np.float32
            assert 1 - float(ref @ e / np.linalg.norm(ref) / np.linalg.norm(e)) < 1e-3, b
            ti += 1
        assert ti == len(targets)
    finally:
        det.conf_thres = old_thr
