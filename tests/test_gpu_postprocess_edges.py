"""GPU: the detector post-process (csrc/postproc.hip) at the seams of its NMS paths, at non-square detector inputs, at its output capacity,
through fid_distance2bbox / fid_distance2kps, and on non-finite and signed-zero values.  Everything is bit for bit against the oracle
(oracle/postprocess.py, oracle/align.py, tests/tile_oracle.py): no tolerances.  The planted lists and the mirror of the path choice are
tests/nms_cases.py; tests/test_nms_cases_cpu.py shows on the CPU that those lists tell a greedy loop with a slip at a seam from the right one."""
import ctypes as C
import json
import os
import re
import subprocess
import sys
import warnings

import numpy as np
import pytest

import nms_cases as nc
from conftest import ROOT, load_golden
from oracle import align as oalign
from oracle import postprocess as pp
from tile_oracle import merge_tiles, random_heads

pytestmark = pytest.mark.gpu

IN640 = (640, 640)


@pytest.fixture(scope="module")
def ctx():
    """a context of its own: these tests move the candidate capacity, which the shared default context's post-processors rely on"""
    from scrfd_arcface_facerecognition_amd._lib import Context
    c = Context(0)
    yield c
    c.close()


def upload_heads(ctx, heads_per_frame):
    from scrfd_arcface_facerecognition_amd.engine import HeadViews
    bufs = [ctx.to_device(np.stack([h[k] for h in heads_per_frame])) for k in range(9)]
    return HeadViews.from_onnx_layout(bufs), bufs


def run_post(ctx, heads_per_frame, in_hw, img_hw, max_num=0, metric=0, conf=0.5, iou=0.4, cap=1024, cand_cap=4096):
    from scrfd_arcface_facerecognition_amd.engine import PostProcessor
    B = len(heads_per_frame)
    hv, bufs = upload_heads(ctx, heads_per_frame)
    post = PostProcessor(ctx, B, cap=cap, cand_cap=cand_cap)
    post.run(hv, B, in_hw, img_hw, conf, iou, max_num, metric)
    return post.fetch(B)


def gpu_nms(ctx, dets, thr):
    from scrfd_arcface_facerecognition_amd._lib import check
    K = len(dets)
    d = ctx.to_device(np.ascontiguousarray(dets, np.float32))
    keep, cnt = ctx.empty((K,), np.int32), ctx.empty((1,), np.int32)
    check(ctx.lib.fid_nms(ctx.handle, C.c_void_p(d.ptr), K, float(thr), C.c_void_p(keep.ptr), C.c_void_p(cnt.ptr)))
    n = int(cnt.download()[0])
    assert 0 <= n <= K
    return [int(k) for k in keep.download()[:n]]


def same(a, b):
    """bit for bit, a NaN equal to a NaN (the payload of a NaN an operation makes is the processor's own)"""
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


# ---- a. the NMS paths through fid_nms: cand_cap = K ---------------------------------------------------------------------------------------------
NMS_LISTS = [(K, path, v) for K, path in nc.NMS_K for v in nc.variants(K, K)]


@pytest.mark.parametrize("K, path, v", NMS_LISTS, ids=[f"K{K}-{path}-{v}" for K, path, v in NMS_LISTS])
def test_nms_at_every_seam(ctx, K, path, v):
    assert nc.nms_regime(K, K)[2] == path
    dets, _ = nc.case(K, K, v)
    keep = gpu_nms(ctx, dets, nc.THR)
    want = list(nc.oracle_keep(K, K, v))
    assert len(keep) == len(want), (len(keep), len(want))
    assert keep == want, next((i, a, b) for i, (a, b) in enumerate(zip(keep, want)) if a != b)


# ---- b. the NMS paths through fid_scrfd_postprocess, batches of two -------------------------------------------------------------------------------
def _post_batches():
    out = []
    for cc, ks in nc.POST_CASES:
        lists = [(K, path, v) for K, path in ks for v in nc.variants(cc, K)]
        out += [(cc, lists[i], lists[(i + 1) % len(lists)]) for i in range(len(lists))]
    return out


POST_BATCHES = _post_batches()


@pytest.mark.parametrize("cc, first, second", POST_BATCHES, ids=[f"cap{cc}-K{a[0]}.{a[2]}+K{b[0]}.{b[2]}" for cc, a, b in POST_BATCHES])
def test_postprocess_at_every_seam(ctx, cc, first, second):
    """frame 0 is the case, frame 1 another list of the same capacity: the per-frame offsets and counts differ"""
    frames = []
    for K, path, v in (first, second):
        assert nc.nms_regime(cc, K) == (nc.N_BOX[cc], cc <= 13652, path)
        frames.append(nc.heads_from_dets(nc.case(cc, K, v)[0], IN640, seed=v))
    (K, _, v) = first
    assert np.array_equal(pp.detect_from_heads(frames[0], IN640, iou_thres=nc.THR)[0], nc.case(cc, K, v)[0][list(nc.oracle_keep(cc, K, v))])
    for max_num, metric in ((0, 0), (0, 1), (5, 0), (5, 1)):
        res = run_post(ctx, frames, IN640, IN640, max_num, metric, iou=nc.THR, cap=1024, cand_cap=cc)
        for b, (det, kps) in enumerate(res):
            odet, okps = pp.detect_from_heads(frames[b], IN640, iou_thres=nc.THR, max_num=max_num, metric="max" if metric == 0 else "d")
            assert len(odet) == (5 if max_num else len(odet)) and len(odet) >= 5
            assert det.shape == odet.shape, (b, max_num, metric, det.shape, odet.shape)
            assert np.array_equal(det, odet), (b, max_num, metric)
            assert np.array_equal(kps, okps), (b, max_num, metric)


# ---- the mirror of the path choice against the library -----------------------------------------------------------------------------------------
CHILD = r"""
import ctypes as C, json, os, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import nms_cases as nc
from scrfd_arcface_facerecognition_amd._lib import Context, check
from scrfd_arcface_facerecognition_amd.engine import HeadViews, PostProcessor
ctx = Context(0)
heads = nc.empty_heads((64, 64))
bufs = [ctx.to_device(h[None]) for h in heads]
hv = HeadViews.from_onnx_layout(bufs)
for i, (kind, cc) in enumerate(json.loads(sys.argv[2])):
    sys.stderr.write("[klog] case %d\n" % i)
    sys.stderr.flush()
    if kind == "post":
        post = PostProcessor(ctx, 1, cap=16, cand_cap=cc)
        post.run(hv, 1, (64, 64), (64, 64), 0.5, 0.4)
        assert post.fetch(1)[0][0].shape == (0, 5)
    else:
        d = ctx.to_device(np.zeros((cc, 5), np.float32))
        keep, cnt = ctx.empty((cc,), np.int32), ctx.empty((1,), np.int32)
        check(ctx.lib.fid_nms(ctx.handle, C.c_void_p(d.ptr), cc, 0.4, C.c_void_p(keep.ptr), C.c_void_p(cnt.ptr)))
        assert int(cnt.download()[0]) == 1
    ctx.sync()
ctx.close()
"""


def test_library_picks_the_path_values_the_mirror_names():
    """FID_KLOG=1: the launcher prints cand_cap, n_box and whether a mask area exists, as it hands them to nms_select"""
    cases = [("post", cc) for cc, _ in nc.POST_CASES] + [("nms", K) for K, _ in nc.NMS_K]
    p = subprocess.run([sys.executable, "-c", CHILD, ROOT, json.dumps(cases)], env=dict(os.environ, FID_KLOG="1"), capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    seen, case = {}, None
    for line in p.stderr.splitlines():
        m = re.match(r"\[klog\] case (\d+)", line)
        if m:
            case = int(m.group(1))
        m = re.match(r"\[klog\] nms cand_cap (\d+) n_box (\d+) masks (\d+)", line)
        if m and case is not None:
            seen.setdefault(case, []).append(tuple(int(v) for v in m.groups()))
    for i, (kind, cc) in enumerate(cases):
        n_box, masks, _ = nc.nms_regime(cc, 1)
        assert seen.get(i) == [(cc, n_box, int(masks))], (kind, cc, seen.get(i))


# ---- c. non-square detector input -----------------------------------------------------------------------------------------------------------------
NONSQUARE = [(96, 160), (160, 96)]
IMAGES = [(1080, 1920), (700, 500), (96, 160)]         # at (96, 160): an image ratio below, above and exactly at the model ratio


@pytest.fixture(scope="module")
def nonsquare_heads():
    rng = np.random.default_rng(51)
    return {in_hw: [random_heads(rng, K, in_hw=in_hw) for K in (60, 57, 64)] for in_hw in NONSQUARE}


@pytest.mark.parametrize("in_hw", NONSQUARE, ids=lambda v: f"{v[0]}x{v[1]}")
def test_postprocess_non_square_input(ctx, nonsquare_heads, in_hw):
    heads = nonsquare_heads[in_hw]
    assert sum(len(h) for h in heads[0][:3]) == 630
    for img_hw in IMAGES:
        for max_num, metric in ((0, 0), (3, 0), (3, 1)):
            res = run_post(ctx, heads, in_hw, img_hw, max_num, metric)
            for b, (det, kps) in enumerate(res):
                odet, okps = pp.detect_from_heads(heads[b], img_hw, input_size=(in_hw[1], in_hw[0]), max_num=max_num,
                                                  metric="max" if metric == 0 else "d")
                assert len(odet) >= 3
                assert np.array_equal(det, odet) and np.array_equal(kps, okps), (img_hw, max_num, metric, b)


@pytest.mark.parametrize("in_hw", NONSQUARE, ids=lambda v: f"{v[0]}x{v[1]}")
def test_decode_non_square_input(ctx, nonsquare_heads, in_hw):
    from scrfd_arcface_facerecognition_amd._lib import check, c_void_pp
    heads = nonsquare_heads[in_hw]
    B = len(heads)
    hv, bufs = upload_heads(ctx, heads)
    check(ctx.lib.fid_scrfd_set_candidate_capacity(ctx.handle, 4096))
    rec, cnt = ctx.empty((B, 4096, 16), np.float32), ctx.empty((B,), np.int32)
    check(ctx.lib.fid_scrfd_decode(ctx.handle, C.cast(hv.ptrs, c_void_pp), hv.pix, hv.anc, hv.bstride, B, in_hw[0], in_hw[1], 2, 0.5,
                                   C.c_void_p(rec.ptr), C.c_void_p(cnt.ptr)))
    counts, recs = cnt.download(), rec.download()
    bounds = np.cumsum([(in_hw[0] // s) * (in_hw[1] // s) * 2 for s in (8, 16, 32)])
    for b in range(B):
        s, bb, kk = pp.decode_heads(heads[b], in_hw, 0.5)
        assert counts[b] == sum(len(x) for x in s)
        r = recs[b, :counts[b]]
        flat = r[:, 15].view(np.int32)
        assert (np.diff(flat) > 0).all()
        level = np.searchsorted(bounds, flat, side="right")
        for lv in range(3):
            m = level == lv
            assert np.array_equal(r[m, 4:5], s[lv]) and np.array_equal(r[m, 0:4], bb[lv]), (b, lv)
            assert np.array_equal(r[m, 5:15].reshape(-1, 5, 2), kk[lv]), (b, lv)


def test_ragged_postprocess_non_square_input(ctx, nonsquare_heads):
    from scrfd_arcface_facerecognition_amd.engine import PostProcessor
    in_hw = (96, 160)
    heads = nonsquare_heads[in_hw]
    hv, bufs = upload_heads(ctx, heads)
    for max_num, metric in ((0, 0), (3, 1)):
        post = PostProcessor(ctx, 3, cap=1024, cand_cap=4096)
        post.run_ragged(hv, 3, in_hw, np.asarray(IMAGES, np.int32), 0.5, 0.4, max_num, metric)
        for b, (det, kps) in enumerate(post.fetch(3)):
            odet, okps = pp.detect_from_heads(heads[b], IMAGES[b], input_size=(160, 96), max_num=max_num, metric="max" if metric == 0 else "d")
            assert len(odet) >= 3 and np.array_equal(det, odet) and np.array_equal(kps, okps), (b, max_num)


def test_tiled_postprocess_non_square_input(ctx):
    from scrfd_arcface_facerecognition_amd.engine import PostProcessor
    from scrfd_arcface_facerecognition_amd.pipeline import tile_plan
    in_hw, img = (96, 160), (170, 290)
    tiles = tile_plan(img[0], img[1], in_hw, 16, True, 1)
    assert tiles[:, 1:3].tolist() == [[0, 0], [130, 0], [0, 74], [130, 74], [0, 0]] and tiles[:, 5].tolist() == [0, 0, 0, 0, 1]     # 2 x 2 and the overview
    rng = np.random.default_rng(52)
    heads = [random_heads(rng, K, in_hw=in_hw) for K in (40, 55, 30, 62, 48)]
    hv, bufs = upload_heads(ctx, heads)
    for edge_margin, max_num, metric in ((-1, 0, 0), (4, 0, 0), (4, 3, 1)):
        post = PostProcessor(ctx, 1, cap=1024, cand_cap=4096)
        post.run_tiled(hv, tiles, 1, in_hw, img, 0.5, 0.4, edge_margin, max_num, metric)
        (det, kps), = post.fetch(1)
        (odet, okps), = merge_tiles(heads, tiles, img, in_hw, 0.5, 0.4, edge_margin, max_num, "max" if metric == 0 else "default")
        assert len(odet) >= 3 and np.array_equal(det, odet) and np.array_equal(kps, okps), (edge_margin, max_num)


LB_IMAGES = [(54, 96), (97, 33), (33, 97), (128, 192), (64, 96)]     # at (64, 96): (128, 192) is the exact 2x, (64, 96) the identity


@pytest.mark.parametrize("in_h, in_w", [(64, 96), (96, 64), (63, 95)])
def test_letterbox_non_square_input_equals_oracle(ctx, in_h, in_w):
    from scrfd_arcface_facerecognition_amd._lib import check
    rng = np.random.default_rng(53)
    for H, W in LB_IMAGES:
        image = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        fr = ctx.to_device(image[None])
        out = ctx.to_device(np.full((1, in_h, in_w, 3), 0xA5, np.uint8))
        sc = C.c_double()
        check(ctx.lib.fid_letterbox(ctx.handle, C.c_void_p(fr.ptr), 1, H, W, C.c_void_p(out.ptr), in_h, in_w, C.byref(sc)))
        ref, osc = oalign.letterbox(image, (in_w, in_h))
        assert sc.value == osc, (H, W, sc.value, osc)
        got = out.download()[0]
        assert np.array_equal(got, ref), (H, W, np.argwhere(got != ref)[:4].tolist())
    if (in_h, in_w) == (64, 96):
        assert np.array_equal(ref, image)                          # the last image: the identity


@pytest.fixture(scope="module")
def wide_detector():
    """SCRFD-500M at 160 wide x 96 high on heuristic kernel plans (no timing runs), its cls bias calibrated on the oracle-letterboxed images"""
    from models import SCRFD
    from scrfd_arcface_facerecognition_amd import archs
    from scrfd_arcface_facerecognition_amd._lib import default_context
    from scrfd_arcface_facerecognition_amd.pipeline import calibrate_detector_bias
    from scrfd_arcface_facerecognition_amd.session import HipSession
    old = os.environ.get("FID_AUTOTUNE")
    os.environ["FID_AUTOTUNE"] = "0"
    try:
        dctx = default_context(0)
        rng = np.random.default_rng(54)
        images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((270, 480), (200, 150), (192, 320))]     # wide, tall, the model's ratio
        det_net = archs.scrfd_500m((96, 160))
        lb = np.stack([oalign.letterbox(im, (160, 96))[0] for im in images])
        det_P, _ = calibrate_detector_bias(dctx, det_net, archs.synth_params(det_net, 5), lb, target=30, max_batch=4)
        det = SCRFD("synthetic:scrfd_500m?seed=5", input_size=(160, 96), conf_thres=0.5, max_batch=4)
        det.session = HipSession(None, ctx=det.ctx, net=det_net, params=det_P, max_batch=4)
        yield det, images
    finally:
        if old is None:
            del os.environ["FID_AUTOTUNE"]
        else:
            os.environ["FID_AUTOTUNE"] = old


def test_detect_end_to_end_at_a_non_square_input(wide_detector):
    """image -> fid_letterbox -> net -> fid_scrfd_postprocess through models/scrfd.py: the oracle on the GPU's own heads.  A (w, h) / (h, w) slip
    anywhere between input_size, the session's input_hw and the C entry points changes the anchor grid or det_scale."""
    from test_gpu_mixed_sizes import read_heads
    det, images = wide_detector
    cn = det.session.compiled((96, 160))
    for im in images:
        for max_num, metric in ((0, "max"), (3, "default")):
            d, k = det.detect(im, max_num=max_num, metric=metric)
            heads, = read_heads(cn, 1)
            assert [len(h) for h in heads[:3]] == [480, 120, 30]
            odet, okps = pp.detect_from_heads(heads, im.shape[:2], (160, 96), det.conf_thres, det.iou_thres, max_num, metric)
            assert len(d) >= 1 and d.dtype == np.float32 and k.shape == (len(d), 5, 2)
            assert np.array_equal(d, odet) and np.array_equal(k, okps), (im.shape, max_num)


# ---- d. output capacity ---------------------------------------------------------------------------------------------------------------------------
def disjoint_dets(n_keep, n_dup, seed):
    """n_keep boxes far apart, n_dup near copies of some of them with lower scores; distinct scores >= 0.5 in shuffled rows"""
    rng = np.random.default_rng(seed)
    n = n_keep + n_dup
    boxes = np.zeros((n, 4), np.float32)
    for i in range(n_keep):
        x, y, w, h = 40 * (i % 12) + 4, 40 * (i // 12) + 4, int(rng.integers(12, 30)), int(rng.integers(12, 30))
        boxes[i] = [x, y, x + w, y + h]
    for i in range(n_dup):
        boxes[n_keep + i] = boxes[i % n_keep] + [1, 0, 1, 0]
    scores = (0.5 + (n - np.arange(n)) / 256.0).astype(np.float32)
    rows = rng.permutation(n)
    return np.concatenate([boxes, scores[:, None]], axis=1)[rows]


SENTINEL = np.float32(-777.25)


def run_post_raw(ctx, frames, cap, max_num=0, metric=0):
    """-> (post, counts, det [B,cap,5], kps [B,cap,10]) without fid_scrfd_check; the output buffers start as SENTINEL"""
    from scrfd_arcface_facerecognition_amd.engine import PostProcessor
    B = len(frames)
    hv, bufs = upload_heads(ctx, frames)
    post = PostProcessor(ctx, B, cap=cap, cand_cap=4096)
    post.det, post.kps = ctx.to_device(np.full((B, cap, 5), SENTINEL)), ctx.to_device(np.full((B, cap, 10), SENTINEL))
    post.counts = ctx.to_device(np.full(B, -1, np.int32))
    post.run(hv, B, IN640, IN640, 0.5, 0.4, max_num, metric)
    ctx.sync()
    return post, post.counts.download(), post.det.download(), post.kps.download()


def test_more_survivors_than_the_output_holds(ctx):
    from scrfd_arcface_facerecognition_amd._lib import FaceIdError
    frames = [nc.heads_from_dets(disjoint_dets(20, 9, 61), IN640, seed=1), nc.heads_from_dets(disjoint_dets(3, 2, 62), IN640, seed=2)]
    want = [pp.detect_from_heads(f, IN640) for f in frames]
    assert [len(d) for d, _ in want] == [20, 3]
    post, counts, det, kps = run_post_raw(ctx, frames, cap=8)
    with pytest.raises(FaceIdError) as e:
        post.fetch(2)
    assert e.value.code == -3 and "20" in str(e.value) and "8" in str(e.value)
    assert counts.tolist() == [8, 3]
    assert np.array_equal(det[0], want[0][0][:8]) and np.array_equal(kps[0].reshape(8, 5, 2), want[0][1][:8])
    assert np.array_equal(det[1, :3], want[1][0]) and np.array_equal(kps[1, :3].reshape(3, 5, 2), want[1][1])
    assert (det[1, 3:] == SENTINEL).all() and (kps[1, 3:] == SENTINEL).all()      # frame 0's rows 8.. went nowhere: not into frame 1's rows
    # max_num above the capacity: the first 8 of the 12 the oracle selects
    for metric in (0, 1):
        odet, okps = pp.detect_from_heads(frames[0], IN640, max_num=12, metric="max" if metric == 0 else "d")
        assert len(odet) == 12
        post, counts, det, kps = run_post_raw(ctx, frames, cap=8, max_num=12, metric=metric)
        with pytest.raises(FaceIdError) as e:
            post.check()
        assert e.value.code == -3 and "12" in str(e.value)
        assert counts.tolist() == [8, 3]
        assert np.array_equal(det[0], odet[:8]) and np.array_equal(kps[0].reshape(8, 5, 2), okps[:8]), metric
        assert np.array_equal(det[1, :3], want[1][0]) and (det[1, 3:] == SENTINEL).all()
    # the report was consumed: an in-capacity run on the same context passes its check
    post, counts, det, kps = run_post_raw(ctx, frames, cap=20)
    assert post.check() == 29
    assert counts.tolist() == [20, 3] and np.array_equal(det[0], want[0][0]) and np.array_equal(det[1, :3], want[1][0])
    post, counts, det, kps = run_post_raw(ctx, frames, cap=8, max_num=8)
    post.check()
    assert counts.tolist() == [8, 3]


# ---- e. fid_distance2bbox / fid_distance2kps --------------------------------------------------------------------------------------------------------
def test_distance2bbox_and_kps_on_the_device(ctx):
    from scrfd_arcface_facerecognition_amd._lib import check
    g = load_golden("decode.npz")
    points, dist, kdist = g["points"], g["dist"], g["kdist"]
    assert len(points) == 500
    for n in (500, 1):
        p, d, kd = ctx.to_device(points[:n].copy()), ctx.to_device(dist[:n].copy()), ctx.to_device(kdist[:n].copy())
        guard = 8
        out = ctx.to_device(np.full(n * 4 + guard, SENTINEL))
        check(ctx.lib.fid_distance2bbox(ctx.handle, C.c_void_p(p.ptr), C.c_void_p(d.ptr), n, C.c_void_p(out.ptr)))
        got = out.download()
        assert np.array_equal(got[:n * 4].reshape(n, 4), g["bbox"][:n]) and (got[n * 4:] == SENTINEL).all(), n
        assert np.array_equal(g["bbox"][:n], pp.distance2bbox(points[:n], dist[:n]))
        out = ctx.to_device(np.full(n * 10 + guard, SENTINEL))
        check(ctx.lib.fid_distance2kps(ctx.handle, C.c_void_p(p.ptr), C.c_void_p(kd.ptr), n, 10, C.c_void_p(out.ptr)))
        got = out.download()
        assert np.array_equal(got[:n * 10].reshape(n, 10), g["kps"][:n]) and (got[n * 10:] == SENTINEL).all(), n
        # one landmark per point: ncol = 2
        kd2 = np.ascontiguousarray(kdist[:n, 4:6])
        kd2_dev = ctx.to_device(kd2)
        out = ctx.to_device(np.full(n * 2 + guard, SENTINEL))
        check(ctx.lib.fid_distance2kps(ctx.handle, C.c_void_p(p.ptr), C.c_void_p(kd2_dev.ptr), n, 2, C.c_void_p(out.ptr)))
        got = out.download()
        assert np.array_equal(got[:n * 2].reshape(n, 2), pp.distance2kps(points[:n], kd2)) and (got[n * 2:] == SENTINEL).all(), n


# ---- f. non-finite and signed-zero values -------------------------------------------------------------------------------------------------------------
def oracle_quiet(*a, **kw):
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        return pp.detect_from_heads(*a, **kw)


def few_heads(n=7, seed=71):
    """n disjoint candidates of different sizes at (640, 640); -> (heads, the stride-8 anchors of the candidates in score order)"""
    dets = disjoint_dets(n, 0, seed)
    heads = nc.heads_from_dets(dets, IN640, seed=seed)
    anchors = np.nonzero(heads[0][:, 0] >= 0.5)[0]
    return heads, anchors[np.argsort(-heads[0][anchors, 0])]


@pytest.mark.parametrize("zero_height", [False, True], ids=["inf-area", "nan-area"])
def test_max_num_with_an_infinite_box(ctx, zero_height):
    """One kept box with x2 = +inf.  Under the default metric its value is inf - inf = NaN; with a height of zero its area inf * 0 is NaN under
    both metrics.  np.argsort(values)[::-1] puts a NaN first: the oracle returns the infinite box, then the best finite ones."""
    heads, order = few_heads()
    a = order[3]
    heads[3][a, 2] = np.inf
    if zero_height:
        heads[3][a, 1], heads[3][a, 3] = 1.0, -1.0
    for max_num in (2, 3):
        for metric in (0, 1):
            odet, okps = oracle_quiet(heads, IN640, max_num=max_num, metric="max" if metric == 0 else "d")
            assert len(odet) == max_num and np.isinf(odet[0, 2]) and np.isfinite(odet[1:]).all()
            (det, kps), = run_post(ctx, [heads], IN640, IN640, max_num, metric)
            print(f"\nzero_height {zero_height} max_num {max_num} metric {metric}: device scores {det[:, 4].tolist()} oracle {odet[:, 4].tolist()}")
            assert same(det, odet) and same(kps, okps), (max_num, metric)


@pytest.mark.parametrize("which", [0, 3], ids=["best", "middle"])
def test_nan_box_distance(ctx, which):
    heads, order = few_heads(seed=72)
    heads[3][order[which], 0] = np.nan
    for max_num, metric in ((0, 0), (2, 0), (2, 1)):
        odet, okps = oracle_quiet(heads, IN640, max_num=max_num, metric="max" if metric == 0 else "d")
        (det, kps), = run_post(ctx, [heads], IN640, IN640, max_num, metric)
        print(f"\nNaN distance on candidate {which}, max_num {max_num} metric {metric}: device {det[:, 4].tolist()} oracle {odet[:, 4].tolist()}")
        assert len(odet) >= 1 and same(det, odet) and same(kps, okps), (max_num, metric)


def test_nan_score_is_never_a_candidate(ctx):
    """NaN >= threshold is false, at conf_thres 0.0 too (every other anchor of the 64 x 64 input is a candidate there)"""
    rng = np.random.default_rng(73)
    heads = random_heads(rng, 60)
    best = int(np.argmax(heads[0][:, 0]))
    clean = oracle_quiet(heads, (64, 64), input_size=(64, 64))[0]
    heads[0][[best, 5], 0] = np.nan
    heads[2][1, 0] = np.nan
    for conf in (0.5, 0.0):
        odet, okps = oracle_quiet(heads, (64, 64), input_size=(64, 64), conf_thres=conf)
        (det, kps), = run_post(ctx, [heads], (64, 64), (64, 64), conf=conf)
        assert len(odet) >= 3 and not np.isnan(odet).any() and odet[0, 4] < clean[0, 4] and same(det, odet) and same(kps, okps), conf


def test_nms_signed_zero_scores(ctx):
    """numpy's stable sort compares -0.0 equal to +0.0 and leaves equal scores in index order (reversed: the larger index first)"""
    s = np.float32([0.0, -0.0, 0.0, -0.0])
    disjoint = np.float32([[0, 0, 9, 9], [20, 0, 29, 9], [40, 0, 49, 9], [60, 0, 69, 9]])
    overlapping = np.float32([[0, 0, 9, 9], [1, 0, 10, 9], [40, 0, 49, 9], [41, 0, 50, 9]])
    for n in (3, 4):
        for boxes in (disjoint, overlapping):
            dets = np.concatenate([boxes[:n], s[:n, None]], axis=1)
            want = [int(i) for i in pp.nms(dets, 0.4)]
            got = gpu_nms(ctx, dets, 0.4)
            print(f"\nscores {s[:n].tolist()} {'disjoint' if boxes is disjoint else 'overlapping'}: device {got} oracle {want}")
            assert got == want
    assert [int(i) for i in pp.nms(np.concatenate([disjoint[:3], s[:3, None]], axis=1), 0.4)] == [2, 1, 0]


def test_head_path_with_a_negative_zero_score(ctx):
    """conf_thres 0.0 admits -0.0 (it is >= 0.0); among the zero scores the order is the anchor order, whatever the sign"""
    rng = np.random.default_rng(74)
    heads = random_heads(rng, 60)
    heads[0][[9, 30, 77], 0] = np.float32([0.0, -0.0, 0.0])
    heads[1][[3, 4], 0] = np.float32([-0.0, 0.0])
    for i, (lv, a) in enumerate(((0, 9), (0, 30), (0, 77), (1, 3), (1, 4))):     # their boxes: 8 pixels wide, far from every other and 160 apart
        heads[3 + lv][a] = np.float32([-(100 + 20 * i), 0.0, 100 + 20 * i + 1, 1.0]) * np.float32(8 / (8, 16)[lv])
    n_all = len(oracle_quiet(heads, (64, 64), input_size=(64, 64), conf_thres=0.0)[0])
    for max_num, metric in ((0, 0), (n_all - 1, 1)):
        odet, okps = oracle_quiet(heads, (64, 64), input_size=(64, 64), conf_thres=0.0, max_num=max_num, metric="max" if metric == 0 else "d")
        (det, kps), = run_post(ctx, [heads], (64, 64), (64, 64), max_num, metric, conf=0.0)
        zeros = np.nonzero(odet[:, 4] == 0)[0]
        assert len(zeros) >= 4 and np.signbit(odet[zeros, 4]).any() and not np.signbit(odet[zeros, 4]).all()
        assert det.shape == odet.shape and np.array_equal(det, odet) and np.array_equal(kps, okps), max_num
        assert np.array_equal(np.signbit(det[:, 4]), np.signbit(odet[:, 4]))
