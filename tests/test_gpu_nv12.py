"""GPU: NV12 frames (fid_nv12_to_bgr, fid_letterbox_nv12, fid_tile_cut_nv12, fid_align_crops_nv12, fid_align_crops_packed_nv12; Nv12Frames through
PackedFacePipeline and video.StreamRunner).  The yardsticks are tests/nv12_oracle.py for the conversion and, for every fused call, its BGR
namesake on the converted frames: each comparison is np.array_equal.

The small batch: two frames of 46 x 62 with pitch 64, four padding rows in front of the UV plane and slack between the frames; the allocation
ends with the last UV row of the last frame.  W is no multiple of 4, pitch != W, every chroma sample serves a 2 x 2 group and bilinear taps
straddle two samples; every byte the layout does not let the library read is 0xFF."""
import ctypes as C
import os

import numpy as np
import pytest

import nv12_oracle as oracle

pytestmark = pytest.mark.gpu

NB, NH, NW = 2, 46, 62
LAYOUT = dict(pitch=64, uv_offset=64 * (NH + 4), frame_stride=64 * (NH + 4) + 64 * (NH // 2) + 96)
STANDARDS = list(oracle.COEFFS)


@pytest.fixture(scope="module")
def ctx():
    from scrfd_arcface_facerecognition_amd._lib import default_context
    return default_context(0)


class Batch:
    """random NV12 frames on the device (allocated at exactly the layout's size), their layout and their BGR conversion by the oracle"""

    def __init__(self, ctx, seed, B, H, W, standard="bt601", **layout):
        from scrfd_arcface_facerecognition_amd._lib import Nv12Frames
        self.B, self.H, self.W, self.standard = B, H, W, standard
        self.buf, self.layout = oracle.random_batch(seed, B, H, W, fill=0xFF, **layout)
        assert self.buf.size == self.layout["frame_stride"] * (B - 1) + self.layout["uv_offset"] + self.layout["pitch"] * (H // 2)
        self.bgr = oracle.nv12_to_bgr(self.buf, B, H, W, standard=standard, **self.layout)
        self.dev = ctx.to_device(self.buf)
        self.frames = Nv12Frames(self.dev, H, W, standard=standard, **self.layout)
        self.bgr_dev = ctx.to_device(self.bgr)


@pytest.fixture(scope="module")
def small(ctx):
    return Batch(ctx, 5, NB, NH, NW, **LAYOUT)


def _i32(a):
    from scrfd_arcface_facerecognition_amd._lib import c_i32_p
    return a.ctypes.data_as(c_i32_p)


# ---- the conversion alone ----
@pytest.mark.parametrize("standard", STANDARDS)
def test_nv12_to_bgr_equals_the_oracle(ctx, standard):
    from scrfd_arcface_facerecognition_amd._lib import check
    outs = []
    for fill in (0xFF, 0x00):                          # the bytes that must never be read, both ways
        buf, lay = oracle.random_batch(5, NB, NH, NW, fill=fill, **LAYOUT)
        from scrfd_arcface_facerecognition_amd._lib import Nv12Frames
        fr = Nv12Frames(ctx.to_device(buf), NH, NW, standard=standard, **lay)
        out = ctx.empty((NB * NH * NW * 3 + 64,), np.uint8)
        out.upload(np.full(NB * NH * NW * 3 + 64, 0xA5, np.uint8))
        check(ctx.lib.fid_nv12_to_bgr(ctx.handle, *fr.args(), NB, NH, NW, C.c_void_p(out.ptr)))
        got = out.download()
        assert (got[NB * NH * NW * 3:] == 0xA5).all()                  # nothing written behind the frames
        got = got[:NB * NH * NW * 3].reshape(NB, NH, NW, 3)
        assert np.array_equal(got, oracle.nv12_to_bgr(buf, NB, NH, NW, standard=standard, **lay))
        outs.append(got)
    assert np.array_equal(outs[0], outs[1])


def test_device_calls_refuse_a_bad_layout(ctx, small):
    """all or nothing, before anything is enqueued: the output keeps its fill"""
    from scrfd_arcface_facerecognition_amd._lib import nv12_desc
    lib, h = ctx.lib, ctx.handle
    out = ctx.empty((NB, NH, NW, 3), np.uint8)
    out.upload(np.full((NB, NH, NW, 3), 0xA5, np.uint8))
    p, o = C.c_void_p(small.dev.ptr), C.c_void_p(out.ptr)
    bad = [nv12_desc(NH, NW, pitch=NW - 2, uv_offset=LAYOUT["uv_offset"], frame_stride=LAYOUT["frame_stride"]),
           nv12_desc(NH, NW, pitch=64, uv_offset=64 * NH - 1, frame_stride=LAYOUT["frame_stride"]),
           nv12_desc(NH, NW, pitch=64, uv_offset=64 * NH, frame_stride=64 * NH + 64 * (NH // 2) - 1),
           nv12_desc(NH, NW, standard=3, **LAYOUT)]
    tiles = np.array([[0, 0, 0, NW, NH, 1]], np.int32)
    for d in bad:
        d = C.byref(d)
        assert lib.fid_nv12_to_bgr(h, p, d, NB, NH, NW, o) == -1 and lib.fid_last_error()
        assert lib.fid_letterbox_nv12(h, p, d, NB, NH, NW, o, 32, 32, None) == -1
        assert lib.fid_tile_cut_nv12(h, p, d, NB, NH, NW, _i32(tiles), 1, o, 32, 32) == -1
        assert lib.fid_align_crops_nv12(h, p, d, NB, NH, NW, o, o, 1, 1, o, None) == -1
        assert lib.fid_align_crops_packed_nv12(h, p, d, NB, NH, NW, o, 1, o, 1, o, None) == -1
    good = C.byref(nv12_desc(NH, NW, **LAYOUT))
    assert lib.fid_nv12_to_bgr(h, p, good, NB, NH - 1, NW, o) == -1                    # odd H
    assert lib.fid_letterbox_nv12(h, p, good, NB, NH, NW - 1, o, 32, 32, None) == -1    # odd W
    ctx.sync()
    assert (out.download() == 0xA5).all()


# ---- the letterbox: three regimes ----
def letterbox_both(ctx, batch, in_h, in_w):
    from scrfd_arcface_facerecognition_amd._lib import check
    B, H, W = batch.B, batch.H, batch.W
    outs, scales = [], []
    for nv in (True, False):
        out = ctx.empty((B, in_h, in_w, 3), np.uint8)
        out.upload(np.full((B, in_h, in_w, 3), 0xA5, np.uint8))
        sc = C.c_double(-1.0)
        if nv:
            check(ctx.lib.fid_letterbox_nv12(ctx.handle, *batch.frames.args(), B, H, W, C.c_void_p(out.ptr), in_h, in_w, C.byref(sc)))
        else:
            check(ctx.lib.fid_letterbox(ctx.handle, C.c_void_p(batch.bgr_dev.ptr), B, H, W, C.c_void_p(out.ptr), in_h, in_w, C.byref(sc)))
        outs.append(out.download())
        scales.append(sc.value)
    return outs, scales


@pytest.mark.parametrize("in_w,new_h", [(32, 23), (30, 22)])           # (the BGR yardstick: its four-pixel kernel / its one-pixel kernel)
def test_letterbox_general_bilinear(ctx, small, in_w, new_h):
    (nv, bgr), (s_nv, s_bgr) = letterbox_both(ctx, small, 32, in_w)
    assert np.array_equal(nv, bgr) and s_nv == s_bgr == new_h / 46
    assert nv[:, :new_h].any() and not nv[:, new_h:].any()             # 46 x 62 -> new_h x in_w: the rows below are the zero fill


@pytest.mark.parametrize("hw", [(64, 64), (60, 60)])                    # -> 32 x 32 and 30 x 30
def test_letterbox_exact_2x(ctx, hw):
    H, W = hw
    b = Batch(ctx, 6, 2, H, W, pitch=68, uv_offset=68 * (H + 2), frame_stride=68 * (H + 2) + 68 * (H // 2) + 40)
    (nv, bgr), (s_nv, s_bgr) = letterbox_both(ctx, b, H // 2, W // 2)
    assert np.array_equal(nv, bgr) and s_nv == s_bgr == 0.5
    s = b.bgr.astype(np.int64)
    want = (s[:, 0::2, 0::2] + s[:, 0::2, 1::2] + s[:, 1::2, 0::2] + s[:, 1::2, 1::2] + 2) >> 2      # four CONVERTED pixels, then the mean
    assert np.array_equal(nv, want.astype(np.uint8))


@pytest.mark.parametrize("hw", [(32, 32), (30, 30)])
def test_letterbox_identity(ctx, hw):
    H, W = hw
    b = Batch(ctx, 7, 2, H, W, standard="bt709", pitch=48, uv_offset=48 * H, frame_stride=48 * (H + H // 2) + 16)
    (nv, bgr), (s_nv, s_bgr) = letterbox_both(ctx, b, H, W)
    assert np.array_equal(nv, bgr) and np.array_equal(nv, b.bgr) and s_nv == s_bgr == 1.0      # every pixel, the last one of the last frame too


# ---- the tile cut ----
@pytest.mark.parametrize("in_w", [32, 30])                              # both kernels: four output pixels per thread / one
def test_tile_cut_native_odd_origin_and_overview(ctx, small, in_w):
    from scrfd_arcface_facerecognition_amd._lib import check
    # frame, x0, y0, w, h, kind: native tiles whose origin disagrees with the chroma grid (one smaller than the input, one that ends on the
    # frame's last pixel) and a letterboxed overview tile per frame
    tiles = np.array([[0, 7, 5, in_w, 32, 0], [0, 13, 9, 21, 17, 0], [0, 0, 0, NW, NH, 1],
                      [1, 29, 13, in_w, 32, 0], [1, NW - 15, NH - 11, 15, 11, 0], [1, 0, 0, NW, NH, 1], [1, 3, 1, 40, 36, 1]], np.int32)
    T = len(tiles)
    outs = []
    for nv in (True, False):
        out = ctx.empty((T, 32, in_w, 3), np.uint8)
        out.upload(np.full((T, 32, in_w, 3), 0xA5, np.uint8))
        if nv:
            check(ctx.lib.fid_tile_cut_nv12(ctx.handle, *small.frames.args(), NB, NH, NW, _i32(tiles), T, C.c_void_p(out.ptr), 32, in_w))
        else:
            check(ctx.lib.fid_tile_cut(ctx.handle, C.c_void_p(small.bgr_dev.ptr), NB, NH, NW, _i32(tiles), T, C.c_void_p(out.ptr), 32, in_w))
        outs.append(out.download())
    assert np.array_equal(outs[0], outs[1])
    assert np.array_equal(outs[0][0], small.bgr[0, 5:37, 7:7 + in_w])                          # a native tile is the converted rectangle itself
    assert np.array_equal(outs[0][4, :11, :15], small.bgr[1, NH - 11:, NW - 15:]) and not outs[0][4, 11:].any() and not outs[0][4, :, 15:].any()


# ---- the warp ----
TEMPLATE = np.array([[38.2946, 51.6963], [73.5318, 51.5014], [56.0252, 71.7366], [41.5493, 92.3655], [70.7299, 92.2041]], np.float64)


def landmarks(scale, degrees, cx, cy):
    """the ArcFace template scaled, rotated and moved so that the crop's centre (56, 56) lands on (cx, cy) of the frame"""
    a = np.deg2rad(degrees)
    R = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    return (((TEMPLATE - 56.0) * scale) @ R.T + [cx, cy]).astype(np.float32).reshape(10)


CAP = 6
FACES = {                                                               # (frame, slot) -> landmarks
    (0, 0): landmarks(0.35, 0.0, 31.0, 23.0),                           # upright, inside the frame
    (0, 1): landmarks(0.30, 30.0, 28.5, 22.25),                         # rotated about 30 degrees
    (0, 2): np.tile(np.float32([20.0, 20.0]), 5),                       # degenerate: five identical points -> zero crop, NaN M
    (1, 0): landmarks(0.45, -8.0, NW - 6.0, NH - 5.0),                  # reaches past the right and the bottom edge: zero border taps,
    (1, 1): landmarks(0.25, 0.0, 20.0, 18.0),                           # ... and the last pixel of the last frame is sampled
}
COUNTS = np.array([3, 2], np.int32)


@pytest.fixture(scope="module")
def face_arrays(ctx):
    kps = np.zeros((NB, CAP, 10), np.float32)
    for (b, f), lm in FACES.items():
        kps[b, f] = lm
    return ctx.to_device(kps), ctx.to_device(COUNTS)


def check_crops(crops, M, small):
    """what the comparison must not be vacuous about: rows = [(0,0), (0,1), (0,2) degenerate, (1,0) border, (1,1), empty]"""
    assert crops[0].all(axis=2).any() and crops[1].any() and crops[4].any()
    assert not crops[2].any() and np.isnan(M[2]).all()                                   # degenerate
    assert not crops[5].any() and not M[5].any()                                         # empty slot / src = -1
    border = crops[3]
    assert border.any() and not border[-1].any() and not border[:, -1].any()             # past the frame on two sides: zeros there
    # the inverse map of the border face puts the frame's last pixel inside the crop: it is sampled
    m = M[3].reshape(2, 3)
    px = m[:, :2] @ np.array([NW - 1.0, NH - 1.0]) + m[:, 2]
    assert (px > 1).all() and (px < 110).all(), px
    assert np.isfinite(M[[0, 1, 3, 4]]).all()


def test_align_crops_slots(ctx, small, face_arrays):
    from scrfd_arcface_facerecognition_amd._lib import check
    kp, cn = face_arrays
    got = []
    for nv in (True, False):
        crops, M = ctx.empty((NB * CAP, 112, 112, 3), np.uint8), ctx.empty((NB * CAP, 6), np.float64)
        crops.upload(np.full(crops.shape, 0xA5, np.uint8))
        tail = (NB, NH, NW, C.c_void_p(kp.ptr), C.c_void_p(cn.ptr), CAP, CAP, C.c_void_p(crops.ptr), C.c_void_p(M.ptr))
        if nv:
            check(ctx.lib.fid_align_crops_nv12(ctx.handle, *small.frames.args(), *tail))
        else:
            check(ctx.lib.fid_align_crops(ctx.handle, C.c_void_p(small.bgr_dev.ptr), *tail))
        got.append((crops.download(), M.download()))
    (c_nv, m_nv), (c_bgr, m_bgr) = got
    assert np.array_equal(c_nv, c_bgr) and np.array_equal(m_nv.view(np.uint64), m_bgr.view(np.uint64))
    rows = [0, 1, 2, CAP + 0, CAP + 1, 3]
    check_crops(c_nv[rows], m_nv[rows], small)


def test_align_crops_packed(ctx, small, face_arrays):
    from scrfd_arcface_facerecognition_amd._lib import check
    kp, _ = face_arrays
    src = np.array([0, 1, 2, CAP + 0, CAP + 1, -1, -1], np.int32)
    sd = ctx.to_device(src)
    n = len(src)
    got = []
    for nv in (True, False):
        crops, M = ctx.empty((n, 112, 112, 3), np.uint8), ctx.empty((n, 6), np.float64)
        crops.upload(np.full(crops.shape, 0xA5, np.uint8))
        tail = (NB, NH, NW, C.c_void_p(kp.ptr), CAP, C.c_void_p(sd.ptr), n, C.c_void_p(crops.ptr), C.c_void_p(M.ptr))
        if nv:
            check(ctx.lib.fid_align_crops_packed_nv12(ctx.handle, *small.frames.args(), *tail))
        else:
            check(ctx.lib.fid_align_crops_packed(ctx.handle, C.c_void_p(small.bgr_dev.ptr), *tail))
        got.append((crops.download(), M.download()))
    (c_nv, m_nv), (c_bgr, m_bgr) = got
    assert np.array_equal(c_nv, c_bgr) and np.array_equal(m_nv.view(np.uint64), m_bgr.view(np.uint64))
    check_crops(c_nv[:6], m_nv[:6], small)


# ---- end to end: the packed pipeline of tests/test_gpu_packed_faces.py (SCRFD-500M at 640 x 640, MobileFaceNet, 8 frames of 360 x 640) ----
PB, PH, PW = 8, 360, 640
THRESH = 0.02


class Scene:
    pass


@pytest.fixture(scope="module")
def scene(ctx):
    old = os.environ.get("FID_AUTOTUNE")
    os.environ["FID_AUTOTUNE"] = "0"
    from oracle import align as oalign
    from scrfd_arcface_facerecognition_amd import archs
    from scrfd_arcface_facerecognition_amd.engine import CompiledNet, Gallery
    from scrfd_arcface_facerecognition_amd.pipeline import calibrate_detector_bias
    s = Scene()
    s.batch = Batch(ctx, 21, PB, PH, PW)                                 # dense layout: what a StreamRunner stages
    calib = oracle.nv12_to_bgr(oracle.random_batch(22, 4, PH, PW)[0], 4, PH, PW)
    s.det_net = archs.scrfd_500m((640, 640))
    lb = np.stack([oalign.letterbox(f)[0] for f in calib])
    s.det_P, _ = calibrate_detector_bias(ctx, s.det_net, archs.synth_params(s.det_net, 2), lb, target=40, max_batch=4)
    s.rec_net = archs.mobilefacenet()
    s.rec_P = archs.synth_params(s.rec_net, 1)
    s.det = CompiledNet(ctx, s.det_net, s.det_P, max_batch=PB)
    s.rec = CompiledNet(ctx, s.rec_net, s.rec_P, max_batch=256)
    s.gallery = Gallery(ctx, np.random.default_rng(77).standard_normal((37, 512)).astype(np.float32))
    yield s
    if old is None:
        del os.environ["FID_AUTOTUNE"]
    else:
        os.environ["FID_AUTOTUNE"] = old


def step_outputs(ctx, s, frames, tiling):
    from scrfd_arcface_facerecognition_amd.pipeline import PackedFacePipeline
    pipe = PackedFacePipeline(ctx, s.det, s.rec, batch=PB, row_cap=256, tiling=tiling)
    pipe.run_step(frames, PH, PW, s.gallery, THRESH)
    res = pipe.results(s.gallery)
    assert pipe.overflow == 0
    out = dict(det=pipe.post.det.download(), kps=pipe.post.kps.download(), counts=pipe.post.counts.download(), crops=pipe.crops.download(),
               q=pipe.q.download().view(np.uint16), idx=pipe.idx.download(), score=pipe.score.download().view(np.uint32))
    return out, res


@pytest.mark.parametrize("tiling", [None, dict(overlap=128, edge_margin=8, overview=True)], ids=["letterboxed", "tiled"])
def test_packed_pipeline_on_nv12_equals_bgr(ctx, scene, tiling):
    s = scene
    nv, res_nv = step_outputs(ctx, s, s.batch.frames, tiling)
    bgr, res_bgr = step_outputs(ctx, s, s.batch.bgr_dev, tiling)
    n = int(np.clip(nv["counts"], 0, 256).sum())
    print(f"\ncounts per frame: {nv['counts'].tolist()}")
    assert n > 0 and np.array_equal(nv["counts"], bgr["counts"])
    # rows of det / kps behind a frame's count, and rows of q / idx / score behind the table's faces, are whatever the last step left there
    for b in range(PB):
        k = int(nv["counts"][b])
        assert np.array_equal(nv["det"][b, :k].view(np.uint32), bgr["det"][b, :k].view(np.uint32))
        assert np.array_equal(nv["kps"][b, :k].view(np.uint32), bgr["kps"][b, :k].view(np.uint32))
    for key in ("crops", "q", "idx", "score"):
        assert np.array_equal(nv[key], bgr[key]), key
    assert nv["crops"][:n].any()
    assert [len(r) for r in res_nv] == [len(r) for r in res_bgr]
    for ra, rb in zip(res_nv, res_bgr):
        for fa, fb in zip(ra, rb):
            assert np.array_equal(fa[0], fb[0]) and fa[1] == fb[1] and np.array_equal(fa[2], fb[2]) and fa[3:] == fb[3:]


def test_pipeline_on_nv12_frames_of_the_detector_size(ctx, scene):
    """H, W == the detector input: BGR frames go straight to the detector, NV12 frames through the letterbox's identity path"""
    from scrfd_arcface_facerecognition_amd.pipeline import FacePipeline
    s = scene
    b = Batch(ctx, 23, PB, 640, 640)
    outs = []
    for frames in (b.frames, b.bgr_dev):
        pipe = FacePipeline(ctx, s.det, s.rec, batch=PB, faces_per_frame=2)
        pipe.run_step(frames, 640, 640, s.gallery, THRESH)
        outs.append((pipe.post.counts.download(), pipe.crops.download(), pipe.idx.download(), pipe.score.download().view(np.uint32)))
    assert outs[0][0].sum() > 0
    for a, c in zip(*outs):
        assert np.array_equal(a, c)


@pytest.mark.parametrize("annotate", [False, True])
def test_stream_runner_nv12(ctx, scene, annotate):
    """five frames at batch 2 (a ragged tail): the NV12 runner yields what the BGR runner yields on the converted frames"""
    from scrfd_arcface_facerecognition_amd.pipeline import PackedFacePipeline
    from scrfd_arcface_facerecognition_amd.video import StreamRunner
    s = scene
    nv12 = s.batch.buf.reshape(PB, PH * 3 // 2, PW)[:5]
    bgr = s.batch.bgr[:5]
    got = []
    for fmt, items in (("nv12", nv12), ("bgr", bgr)):
        pipe = PackedFacePipeline(ctx, s.det, s.rec, batch=2, row_cap=256)
        runner = StreamRunner(pipe, s.gallery, (PH, PW), similarity_thresh=THRESH, annotate=annotate, pixel_format=fmt)
        assert runner.upload_bytes == 2 * PH * PW * (3 if fmt == "bgr" else 1.5)
        got.append(list(runner.run(iter(items))))
        runner.close()
    a, b = got
    assert len(a) == len(b) == 5
    faces_a, faces_b = ([x[0] for x in a], [x[0] for x in b]) if annotate else (a, b)
    assert sum(len(r) for r in faces_a) > 0
    for ra, rb in zip(faces_a, faces_b):
        assert len(ra) == len(rb)
        for fa, fb in zip(ra, rb):
            assert np.array_equal(fa[0], fb[0]) and fa[1] == fb[1] and np.array_equal(fa[2], fb[2]) and fa[3:] == fb[3:]
    if annotate:
        for i, ((_, fa), (_, fb)) in enumerate(zip(a, b)):
            assert fa.shape == (PH, PW, 3) and np.array_equal(fa, fb), i
            assert (fa != bgr[i]).any(), i                                               # something was drawn
