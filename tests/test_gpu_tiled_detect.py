"""GPU: tiled detection (fid_tile_cut / fid_scrfd_postprocess_tiled, PostProcessor.run_tiled, SCRFD.detect_tiled, FacePipeline(tiling=...)).
The yardsticks are tests/tile_oracle.py (numpy, on the oracle's decode / sort / NMS), fid_letterbox and fid_scrfd_postprocess; every comparison is
bit for bit.  Synthetic head tensors use a 64x64 detector input (168 anchors)."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import postprocess as pp
from tile_oracle import cut_tiles, merge_tiles, random_heads, tile_candidates

pytestmark = pytest.mark.gpu

IN = (64, 64)
IMG = (150, 203)              # odd width: unaligned source rows; both axes end in a clamped tile at overlap 16


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


def plan(H, W, in_hw=IN, overlap=16, overview=True, batch=1):
    from scrfd_arcface_facerecognition_amd.pipeline import tile_plan
    return tile_plan(H, W, in_hw, overlap, overview, batch)


# ---- 1. cut ------------------------------------------------------------------------------------------------

def letterbox_whole(ctx, frames, in_h, in_w):
    from scrfd_arcface_facerecognition_amd._lib import check
    B, H, W, _ = frames.shape
    fr = ctx.to_device(frames)
    out = ctx.empty((B, in_h, in_w, 3), np.uint8)
    check(ctx.lib.fid_letterbox(ctx.handle, C.c_void_p(fr.ptr), B, H, W, C.c_void_p(out.ptr), in_h, in_w, None))
    return out.download()


@pytest.mark.parametrize("in_h, in_w", [(64, 64), (48, 62)])            # the 4-pixel kernel, the byte kernel
@pytest.mark.parametrize("B, H, W", [(2, 150, 203), (1, 40, 203)])       # clamped last tiles on both axes; a frame lower than the input: zero fill
def test_cut_equals_slices_and_letterbox(ctx, B, H, W, in_h, in_w):
    from scrfd_arcface_facerecognition_amd._lib import check
    rng = np.random.default_rng(31)
    frames = rng.integers(1, 256, (B, H, W, 3), dtype=np.uint8)           # no zero byte: the zero fill is told from copied pixels
    tiles = plan(H, W, (in_h, in_w), batch=B)
    T = len(tiles)
    assert T == B * ((12 if H > in_h else 4) + 1) if (in_h, in_w) == IN else T > B
    fr = ctx.to_device(frames)
    nbytes = T * in_h * in_w * 3
    assert nbytes % 4 == 0
    out = ctx.to_device(np.full(nbytes + 4, 0xA5, np.uint8))
    check(ctx.lib.fid_tile_cut(ctx.handle, C.c_void_p(fr.ptr), B, H, W, _i32(tiles), T, C.c_void_p(out.ptr), in_h, in_w))
    raw = out.download()
    got = raw[:nbytes].reshape(T, in_h, in_w, 3)
    assert (raw[nbytes:] == 0xA5).all()                                   # the word after the last tile
    want = cut_tiles(frames, tiles, (in_h, in_w))
    for t in range(T):
        assert np.array_equal(got[t], want[t]), (t, tiles[t].tolist())
    lb = letterbox_whole(ctx, frames, in_h, in_w)
    ov = np.nonzero(tiles[:, 5] == 1)[0]
    assert len(ov) == B
    for b, t in enumerate(ov):
        assert np.array_equal(got[t], lb[b]), b


def test_cut_letterboxes_a_rectangle_of_a_frame(ctx):
    """kind 1 on a part of a frame (rows W pixels apart), bilinear, identity and exact 2x: the letterbox of the slice as its own image"""
    from scrfd_arcface_facerecognition_amd._lib import check
    rng = np.random.default_rng(32)
    frames = rng.integers(1, 256, (2, 150, 203, 3), dtype=np.uint8)
    tiles = np.array([[0, 7, 3, 131, 100, 1], [1, 33, 11, 64, 64, 1], [1, 75, 22, 128, 128, 1], [1, 1, 0, 50, 149, 1]], np.int32)
    out = ctx.empty((4, 64, 64, 3), np.uint8)
    fr = ctx.to_device(frames)
    check(ctx.lib.fid_tile_cut(ctx.handle, C.c_void_p(fr.ptr), 2, 150, 203, _i32(tiles), 4, C.c_void_p(out.ptr), 64, 64))
    got = out.download()
    for t, (b, x0, y0, w, h, _) in enumerate(tiles.tolist()):
        ref = letterbox_whole(ctx, np.ascontiguousarray(frames[b:b + 1, y0:y0 + h, x0:x0 + w]), 64, 64)[0]
        assert np.array_equal(got[t], ref), t


# ---- 2. merge against the oracle ------------------------------------------------------------------------------

def run_tiled(ctx, heads_per_tile, tiles, B, img_hw, edge_margin, max_num=0, metric=0, conf=0.5, iou=0.4, cap=1024, cand_cap=4096, fetch=True):
    from scrfd_arcface_facerecognition_amd.engine import HeadViews, PostProcessor
    bufs = [ctx.to_device(np.stack([h[k] for h in heads_per_tile])) for k in range(9)]
    hv = HeadViews.from_onnx_layout(bufs)
    post = PostProcessor(ctx, B, cap=cap, cand_cap=cand_cap)
    post.run_tiled(hv, tiles, B, IN, img_hw, conf, iou, edge_margin, max_num, metric)
    return (post.fetch(B) if fetch else post), bufs, hv


def edge_probe_heads(rng, x0, m):
    """heads of the tile at (x0 > 0, y0 = 0) whose three best boxes have a frame x1 one unit in the last place below x0 + m, exactly on it and
    one above: stride-8 anchors at cx = 16, cy = 8 / 24 / 40 (8 pixels high, so they never overlap); x1 = (16 - 8 * d) + x0 in fp32"""
    heads = random_heads(rng, 20, hi=0.9)
    edge = np.float32(x0 + m)
    targets = [np.nextafter(edge, np.float32(-np.inf)), edge, np.nextafter(edge, np.float32(np.inf))]
    d0 = np.float32((16 - m) / 8.0)
    found = {}
    for k in range(-64, 65):
        d = d0
        for _ in range(abs(k)):
            d = np.nextafter(d, np.float32(np.inf if k > 0 else -np.inf))
        x1 = (np.float32(16) - d * np.float32(8)) / np.float32(1.0) + np.float32(x0)
        for ti, tv in enumerate(targets):
            if x1 == tv and ti not in found:
                found[ti] = d
    assert sorted(found) == [0, 1, 2], found
    for ti, cy in enumerate((8, 24, 40)):
        i = ((cy // 8) * 8 + 2) * 2                     # stride 8, 8 x 8 map, 2 anchors per pixel: pixel (x = 2, y = cy / 8), anchor 0
        heads[0][i, 0] = np.float32(0.999 - 0.001 * ti)                 # above every other score of the frame
        heads[3][i] = np.float32([found[ti], 0.5, 2.0, 0.5])
    return heads, targets


@pytest.fixture(scope="module")
def merge_case():
    """a 12 + 1 tile plan on two frames; per-tile candidate counts from none to every anchor; tile 1 of frame 0 holds the edge probes"""
    rng = np.random.default_rng(33)
    tiles = plan(*IMG, batch=2)
    assert len(tiles) == 26
    counts = [0, 3, 40, 120, 168, 1, 17, 64, 5, 90, 0, 33, 150, 168, 12, 0, 7, 48, 99, 2, 130, 25, 0, 60, 9, 111]
    heads = [random_heads(rng, K) for K in counts]
    assert tiles[1].tolist() == [0, 48, 0, 64, 64, 0]
    heads[1], targets = edge_probe_heads(rng, 48, 2)
    return tiles, heads, targets


@pytest.mark.parametrize("edge_margin", [-1, 0, 2])
@pytest.mark.parametrize("max_num, metric", [(0, 0), (2, 0), (5, 1)])
def test_merge_equals_oracle(ctx, merge_case, max_num, metric, edge_margin):
    tiles, heads, targets = merge_case
    res, _, _ = run_tiled(ctx, heads, tiles, 2, IMG, edge_margin, max_num, metric)
    want = merge_tiles(heads, tiles, IMG, IN, 0.5, 0.4, edge_margin, max_num, "max" if metric == 0 else "default")
    for b in range(2):
        assert len(want[b][0]) > 0
        assert np.array_equal(res[b][0], want[b][0]), (b, max_num, edge_margin)
        assert np.array_equal(res[b][1], want[b][1]), (b, max_num, edge_margin)
    if max_num == 0:
        # the probes: their scores are the frame's three best, 8-pixel-high boxes in different rows, so each is a survivor unless the rule drops it
        x1 = {float(s): float(x) for x, s in zip(res[0][0][:, 0], res[0][0][:, 4])}
        below, on, above = (np.float32(0.999 - 0.001 * k) for k in range(3))
        assert x1.get(float(on)) == float(targets[1]) and x1.get(float(above)) == float(targets[2])
        assert (float(below) in x1) == (edge_margin != 2)                 # x1 < x0 + m by one unit in the last place: dropped at m = 2 only
        if edge_margin != 2:
            assert x1[float(below)] == float(targets[0])


# ---- 3. the two identities, against fid_scrfd_postprocess on the same device buffers -------------------------------

@pytest.mark.parametrize("max_num, metric", [(0, 0), (3, 1)])
def test_overview_only_plan_is_the_untiled_postprocess(ctx, max_num, metric):
    from scrfd_arcface_facerecognition_amd.engine import PostProcessor
    rng = np.random.default_rng(34)
    heads = [random_heads(rng, K) for K in (40, 0, 168)]
    tiles = np.array([[b, 0, 0, IMG[1], IMG[0], 1] for b in range(3)], np.int32)
    got, bufs, hv = run_tiled(ctx, heads, tiles, 3, IMG, 2, max_num, metric)
    post = PostProcessor(ctx, 3, cap=1024)
    post.run(hv, 3, IN, IMG, 0.5, 0.4, max_num, metric)
    ref = post.fetch(3)
    assert [len(d) for d, _ in ref][1] == 0 and len(ref[0][0]) > 0
    for b in range(3):
        assert np.array_equal(got[b][0], ref[b][0]) and np.array_equal(got[b][1], ref[b][1]), b


def test_one_native_tile_is_the_untiled_postprocess_plus_the_offset(ctx):
    from scrfd_arcface_facerecognition_amd.engine import PostProcessor
    rng = np.random.default_rng(35)
    heads = [random_heads(rng, 60)]
    x0, y0 = 139, 86
    tiles = np.array([[0, x0, y0, 64, 64, 0]], np.int32)
    ((det, kps),), bufs, hv = run_tiled(ctx, heads, tiles, 1, IMG, -1)
    post = PostProcessor(ctx, 1, cap=1024)
    post.run(hv, 1, IN, IN, 0.5, 0.4)
    (rdet, rkps), = post.fetch(1)
    assert len(rdet) > 3
    assert np.array_equal(det, rdet + np.array([x0, y0, x0, y0, 0], np.float32))
    assert np.array_equal(kps, rkps + np.array([x0, y0], np.float32))


# ---- 4. equal scores --------------------------------------------------------------------------------------------

def test_equal_scores_fall_in_tile_rank_then_anchor_order(ctx):
    """the same heads in two far-apart tiles of frame 0 and in a tile of frame 1: every score occurs twice in frame 0, the copy of the lower
    tile rank first, and once in frame 1"""
    rng = np.random.default_rng(36)
    h = random_heads(rng, 50)
    h[0][[10, 11, 12, 40], 0] = np.float32(0.97)                        # ... and ties inside a tile: anchor order
    img = (150, 403)
    tiles = np.array([[0, 0, 0, 64, 64, 0], [0, 300, 40, 64, 64, 0], [1, 300, 40, 64, 64, 0]], np.int32)
    res, _, _ = run_tiled(ctx, [h, h, h], tiles, 2, img, -1)
    want = merge_tiles([h, h, h], tiles, img, IN, 0.5, 0.4, -1)
    for b in range(2):
        assert np.array_equal(res[b][0], want[b][0]) and np.array_equal(res[b][1], want[b][1]), b
    d0, d1 = res[0][0], res[1][0]
    assert len(d0) == 2 * len(d1) and len(d1) > 5
    rank = (d0[:, 0] > 200).astype(int)                                   # which tile a survivor of frame 0 came from
    assert ((d0[:, 2] < 200) == (rank == 0)).all()
    for s in np.unique(d0[:, 4]):
        r = rank[d0[:, 4] == s]
        assert r.tolist() == [0] * (len(r) // 2) + [1] * (len(r) // 2), (s, r)       # rank 0 before rank 1 at every equal score
    assert np.array_equal(d0[rank == 1], d1)                              # frame 1 holds its own tile only, in the same (anchor) order
    (single, _), = merge_tiles([h], np.array([[0, 300, 40, 64, 64, 0]], np.int32), img, IN, 0.5, 0.4, -1)
    assert np.array_equal(d1, single)


# ---- 5. capacity --------------------------------------------------------------------------------------------------

def test_candidates_of_a_frames_tiles_together_exceed_the_capacity(ctx):
    from scrfd_arcface_facerecognition_amd._lib import FaceIdError, check
    rng = np.random.default_rng(37)
    heads = [random_heads(rng, K) for K in (40, 40, 40, 30)]             # each tile below the capacity of 64, frame 0 at 120
    tiles = np.array([[0, 0, 0, 64, 64, 0], [0, 139, 0, 64, 64, 0], [0, 0, 86, 64, 64, 0], [1, 48, 48, 64, 64, 0]], np.int32)
    try:
        post, _, _ = run_tiled(ctx, heads, tiles, 2, IMG, -1, cand_cap=64, fetch=False)
        with pytest.raises(FaceIdError) as e:
            post.check()
        assert e.value.code == -3 and "120" in str(e.value)
        n = int(post.counts.download()[1])
        det, kps = post.det.download()[1, :n], post.kps.download()[1, :n].reshape(-1, 5, 2)
        want = merge_tiles(heads, tiles, IMG, IN, 0.5, 0.4, -1)[1]
        assert n > 0 and np.array_equal(det, want[0]) and np.array_equal(kps, want[1])
    finally:
        check(ctx.lib.fid_scrfd_set_candidate_capacity(ctx.handle, 4096))


# ---- 6. validation --------------------------------------------------------------------------------------------------

BAD_ROWS = [("frame below 0", [-1, 0, 0, 64, 64, 0]), ("frame past the batch", [2, 0, 0, 64, 64, 0]), ("leaves the frame right", [1, 140, 0, 64, 64, 0]),
            ("leaves the frame below", [1, 0, 87, 64, 64, 0]), ("negative origin", [1, -1, 0, 64, 64, 0]), ("zero width", [1, 0, 0, 0, 64, 0]),
            ("negative height", [1, 0, 0, 64, -3, 0]), ("native tile wider than the input", [1, 0, 0, 65, 64, 0]),
            ("native tile higher than the input", [1, 0, 0, 64, 65, 0]), ("degenerate letterbox", [1, 0, 0, 203, 1, 1]),
            ("frames not ascending", [0, 0, 0, 64, 64, 0]), ("unknown kind", [1, 0, 0, 64, 64, 2])]


def test_validation_is_all_or_nothing(ctx):
    from scrfd_arcface_facerecognition_amd.engine import HeadViews
    rng = np.random.default_rng(38)
    frames = ctx.to_device(rng.integers(0, 256, (2, 150, 203, 3), dtype=np.uint8))
    good = np.array([[0, 0, 0, 64, 64, 0], [0, 0, 0, 203, 150, 1], [1, 0, 0, 64, 64, 0], [1, 100, 50, 64, 64, 0]], np.int32)
    T = len(good)
    pattern = np.tile(np.arange(251, dtype=np.uint8), T * 64 * 64 * 3 // 251 + 1)[:T * 64 * 64 * 3]
    out = ctx.to_device(pattern)
    heads = [random_heads(rng, 30) for _ in range(T)]
    bufs = [ctx.to_device(np.stack([h[k] for h in heads])) for k in range(9)]
    hv = HeadViews.from_onnx_layout(bufs)
    det_s, kps_s, cnt_s = np.full((2, 16, 5), 7.5, np.float32), np.full((2, 16, 10), -7.5, np.float32), np.full(2, 1234, np.int32)
    det, kps, cnt = ctx.to_device(det_s), ctx.to_device(kps_s), ctx.to_device(cnt_s)
    ctx.sync()
    for row in (1, 2, 3):
        for what, bad in BAD_ROWS:
            if what == "frames not ascending" and row != 3:
                continue                                                  # (frame 0 behind frame 0 is in order: only row 3 follows a frame 1)
            tiles = good.copy()
            tiles[row] = bad
            rc =ctx.lib.fid_tile_cut(ctx.handle, C.c_void_p(frames.ptr), 2, 150, 203, _i32(tiles), T, C.c_void_p(out.ptr), 64, 64)
            msg = ctx.lib.fid_last_error().decode()
            assert rc == -1 and f"tile {row}:" in msg, (what, row, rc, msg)
            rc = ctx.lib.fid_scrfd_postprocess_tiled(ctx.handle, C.cast(hv.ptrs, C.POINTER(C.c_void_p)), hv.pix, hv.anc, hv.bstride, _i32(tiles), T,
                                                     64, 64, 2, 2, 150, 203, 0.5, 0.4, 2, 0, 0, C.c_void_p(det.ptr), C.c_void_p(kps.ptr),
                                                     C.c_void_p(cnt.ptr), 16)
            msg = ctx.lib.fid_last_error().decode()
            assert rc == -1 and f"tile {row}:" in msg, (what, row, rc, msg)
    ctx.sync()
    assert np.array_equal(out.download(), pattern)
    assert np.array_equal(det.download(), det_s) and np.array_equal(kps.download(), kps_s) and np.array_equal(cnt.download(), cnt_s)
    # ... and the table they were derived from passes
    assert ctx.lib.fid_tile_cut(ctx.handle, C.c_void_p(frames.ptr), 2, 150, 203, _i32(good), T, C.c_void_p(out.ptr), 64, 64) == 0
    assert not np.array_equal(out.download(), pattern)


# ---- 7. end to end ------------------------------------------------------------------------------------------------

FRAME_HW = (500, 700)


@pytest.fixture(scope="module")
def tiled_detector(ctx, heuristic_plans):
    """SCRFD-500M at 320x320, max_batch 8, its cls bias calibrated on the frame's own 7 tiles (as test_gpu_mixed_sizes.py calibrates on its
    letterboxed images): every tile has candidates at conf_thres 0.5 by construction"""
    from models import SCRFD
    from scrfd_arcface_facerecognition_amd import archs
    from scrfd_arcface_facerecognition_amd.pipeline import calibrate_detector_bias
    from scrfd_arcface_facerecognition_amd.session import HipSession
    rng = np.random.default_rng(39)
    frame = rng.integers(0, 256, FRAME_HW + (3,), dtype=np.uint8)
    tiles = plan(*FRAME_HW, (320, 320), overlap=64)
    assert len(tiles) == 7 and int((tiles[:, 5] == 0).sum()) == 6
    cut = cut_tiles(frame[None], tiles, (320, 320))
    det_net = archs.scrfd_500m((320, 320))
    det_P, _ = calibrate_detector_bias(ctx, det_net, archs.synth_params(det_net, 5), cut, target=30, max_batch=8)
    det = SCRFD("synthetic:scrfd_500m?seed=5", input_size=(320, 320), conf_thres=0.5, max_batch=8)
    det.session = HipSession(None, ctx=det.ctx, net=det_net, params=det_P, max_batch=8)
    assert det.ctx is ctx
    return det, frame, tiles, cut


def test_detect_tiled_end_to_end(ctx, tiled_detector):
    from test_gpu_mixed_sizes import read_heads
    from scrfd_arcface_facerecognition_amd._lib import check
    from scrfd_arcface_facerecognition_amd.engine import CompiledNet, resolve_model
    from scrfd_arcface_facerecognition_amd.pipeline import FacePipeline
    det, frame, tiles, cut = tiled_detector
    F = 4
    for max_num in (0, F):
        d, k = det.detect_tiled(frame, max_num=max_num, overlap=64, edge_margin=8)
        # the chain on the host: cut, the detector's existing batch path on the 7 tiles, the heads read back, the oracle's merge
        cn = det.session.compiled((320, 320))
        cn.run(cut)
        heads = read_heads(cn, len(tiles))
        (od, ok), = merge_tiles(heads, tiles, FRAME_HW, (320, 320), det.conf_thres, det.iou_thres, 8, max_num)
        assert d.dtype == np.float32 and k.shape == (len(d), 5, 2)
        assert np.array_equal(d, od) and np.array_equal(k, ok), max_num
        if max_num == 0:
            native = np.concatenate([tile_candidates(heads[t], tiles[t], FRAME_HW, (320, 320), det.conf_thres, 8)[1] for t in range(6)])
            from_native = [any(np.array_equal(row[:4], c) for c in native) for row in d]
            print(f"\ntiled detections: {len(d)}, of them from native tiles: {sum(from_native)}")
            assert len(d) > 0 and any(from_native)
    # the same frame through FacePipeline(tiling=...): same det / kps, and the embeddings of fid_align_crops + the recogniser on those kps
    rec_net, rec_P = resolve_model("synthetic:arcface_mbf")
    rec = CompiledNet(ctx, rec_net, rec_P, max_batch=F)
    pipe = FacePipeline(ctx, det.session.compiled((320, 320)), rec, batch=1, faces_per_frame=F, conf_thres=det.conf_thres, iou_thres=det.iou_thres,
                        tiling=dict(overlap=64, edge_margin=8, overview=True))
    fr = ctx.to_device(frame[None])
    pipe.detect(fr, *FRAME_HW)
    pipe.embed(fr, *FRAME_HW)
    (pd, pk), = pipe.post.fetch(1)
    assert np.array_equal(pd, d) and np.array_equal(pk, k)                  # (d, k: detect_tiled at max_num = F)
    n = len(d)
    assert 0 < n <= F
    emb = pipe.embeddings()[:n].copy()
    kp = ctx.to_device(np.ascontiguousarray(np.concatenate([k.reshape(n, 10), np.zeros((F - n, 10), np.float32)])[None]))
    cnt = ctx.to_device(np.array([n], np.int32))
    crops = ctx.empty((F, 112, 112, 3), np.uint8)
    check(ctx.lib.fid_align_crops(ctx.handle, C.c_void_p(fr.ptr), 1, FRAME_HW[0], FRAME_HW[1], C.c_void_p(kp.ptr), C.c_void_p(cnt.ptr), F, F,
                                  C.c_void_p(crops.ptr), None))
    rec.run_device(crops, F)
    ref = rec.read(rec.low.outputs[0], F).reshape(F, -1)[:n]
    assert np.array_equal(emb, ref)
    assert np.abs(emb).max() > 0
    # the keyword reaches the other pipelines: same detections from their detect stage
    from scrfd_arcface_facerecognition_amd.pipeline import GroupedFacePipeline, PackedFacePipeline
    tiling = dict(overlap=64, edge_margin=8)
    packed = PackedFacePipeline(ctx, pipe.det, rec, batch=1, row_cap=F, max_num=F, conf_thres=det.conf_thres, iou_thres=det.iou_thres, tiling=tiling)
    packed.detect(fr, *FRAME_HW)
    grouped = GroupedFacePipeline(ctx, pipe.det, rec, batch=1, faces_per_frame=F, group=1, conf_thres=det.conf_thres, iou_thres=det.iou_thres,
                                  tiling=tiling)
    grouped.collect(fr, *FRAME_HW)
    for p in (packed, grouped):
        (qd, qk), = p.post.fetch(1)
        assert np.array_equal(qd, d) and np.array_equal(qk, k)
    with pytest.raises(AssertionError):                                   # 2 frames x 7 tiles do not fit the detector's max_batch of 8
        FacePipeline(ctx, pipe.det, CompiledNet(ctx, rec_net, rec_P, max_batch=2 * F), batch=2, faces_per_frame=F, tiling=tiling).detect(
            ctx.to_device(np.stack([frame, frame])), *FRAME_HW)


def test_face_analysis_tiled_get_and_get_batch(ctx, tiled_detector):
    """FaceAnalysis.prepare(tiled=True): get and get_batch on uniform input detect tiled; a mixed-size list keeps the ragged path"""
    from scrfd_arcface_facerecognition_amd.app import FaceAnalysis
    det, frame, tiles, cut = tiled_detector
    app = FaceAnalysis("synthetic:scrfd_500m?seed=5", "synthetic:arcface_mbf?seed=5", det_size=(320, 320), max_faces=16)
    app.det = det
    app.prepare(det_size=(320, 320), tiled=True, tile_overlap=64, tile_margin=8)
    d, k = det.detect_tiled(frame, overlap=64, edge_margin=8)
    faces = app.get(frame)
    assert len(faces) == min(len(d), 16) > 0
    assert all(np.array_equal(f.bbox, d[i, :4]) and np.array_equal(f.kps, k[i]) for i, f in enumerate(faces))
    batch = app.get_batch(np.stack([frame, frame[::-1].copy()]))
    assert len(batch) == 2 and len(batch[0]) == len(d)
    assert all(np.array_equal(f.bbox, d[i, :4]) for i, f in enumerate(batch[0]))
    assert all(np.array_equal(a.embedding, b.embedding) for a, b in zip(batch[0][:16], faces))
    small = frame[:200, :300].copy()
    mixed = app.get_batch([frame, small])
    ref = det.detect_batch([frame, small])
    assert [len(m) for m in mixed] == [len(r[0]) for r in ref]
