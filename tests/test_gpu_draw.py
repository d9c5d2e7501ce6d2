"""GPU: the overlay on the device (fid_labels_*, fid_draw_faces; FacePipeline.draw and its subclasses; video.StreamRunner(annotate=True)).
The yardstick is tests/draw_oracle.py, every comparison byte for byte over the whole buffer; the direct cases upload synthetic det / counts /
idx / score / track arrays, no network runs in them.  64 guard bytes behind the frames and every input are checked by every direct call."""
import ctypes as C
import os

import numpy as np
import pytest

import draw_oracle as O
from draw_calls import c_style, device_draw, host_draw

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from scrfd_arcface_facerecognition_amd._lib import default_context
    return default_context(0)


@pytest.fixture(scope="module")
def glyphs(ctx):
    out = np.zeros(95 * 7, np.uint8)
    assert ctx.lib.fid_draw_glyphs(out.ctypes.data_as(C.c_void_p)) == 0
    return out.reshape(95, 7)


def frames_of(n, H, W, seed=3):
    return np.random.default_rng(seed).integers(0, 256, (n, H, W, 3), dtype=np.uint8)


# ---- the entry point ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H, W", [(48, 80), (37, 67)])
def test_case_list_equals_the_oracle(ctx, glyphs, H, W):
    """W = 80: rows are dword-aligned, W = 67: every store is a byte store; both have tiles cut by the right and the bottom edge"""
    frames = frames_of(O.B, H, W)
    for name, kw in O.cases(H, W):
        got = device_draw(ctx, frames, O.CAP, **kw)
        want = O.draw(frames, cap=O.CAP, glyphs=glyphs, **kw)
        assert np.array_equal(got, want), (name, np.argwhere(got != want)[:6])
        if name == "an empty frame between two drawn ones":
            assert np.array_equal(got[1], frames[1]) and (got[0] != frames[0]).any() and (got[2] != frames[2]).any()


def wide_scene():
    """40 x 136: three tile columns (64 | 64 | 8) and three tile rows (16 | 16 | 8).  Face 0's extent covers every tile; its thick arms and
    its bar fill whole aligned groups of four pixels (the dword stores) and cross every tile boundary"""
    H, W, cap = 40, 136, 6
    boxes = [[(8, 8, 110, 38), (60, 12, 70, 20), (120, 2, 134, 38), (-5, 14, 66, 18)],
             [(0, 0, 135, 39), (62, 14, 66, 18)],
             []]
    det, counts = np.zeros((3, cap, 5), np.float32), np.array([len(b) for b in boxes], np.int32)
    for b, fr in enumerate(boxes):
        if fr:
            det[b, :len(fr), :4] = fr
    idx = np.array([[0, -1, 1, 2, 0, 0], [3, 0, 0, 0, 0, 0], [0] * 6], np.int32)
    score = np.array([[0.9, 0, 0.5, 0.25, 0, 0], [1.0, 0.4, 0, 0, 0, 0], [0] * 6], np.float32)
    return H, W, cap, dict(det=det, counts=counts, idx=idx, score=score, id_stride=cap, names=O.NAMES)


@pytest.mark.parametrize("style", [O.Style(thickness=7, text_scale=1), O.Style(thickness=15, text_scale=2, proportion=0.5), O.Style(thickness=1, text_scale=0)])
def test_three_by_three_tiles(ctx, glyphs, style):
    H, W, cap, kw = wide_scene()
    frames = frames_of(3, H, W, seed=4)
    got = device_draw(ctx, frames, cap, style=style, **kw)
    want = O.draw(frames, cap=cap, glyphs=glyphs, style=style, **kw)
    assert np.array_equal(got, want), np.argwhere(got != want)[:6]
    assert np.array_equal(got[2], frames[2])
    if style.thickness > 1:                                                # four adjacent covered pixels at a multiple of four: the dword path ran
        m = (got[0] != frames[0]).any(axis=2)
        assert m.reshape(H, W // 4, 4).all(axis=2).any()


def test_device_and_host_agree_on_a_random_case(ctx, glyphs):
    rng = np.random.default_rng(17)
    Bn, cap, H, W, G = 4, 16, 90, 200, 6
    frames = frames_of(Bn, H, W, seed=6)
    det = np.zeros((Bn, cap, 5), np.float32)
    x1, y1 = rng.uniform(-20, W - 10, (Bn, cap)), rng.uniform(-10, H - 10, (Bn, cap))
    det[..., 0], det[..., 1] = x1, y1
    det[..., 2], det[..., 3] = x1 + rng.uniform(4, 90, (Bn, cap)), y1 + rng.uniform(4, 60, (Bn, cap))
    counts = np.array([16, 9, 0, 13], np.int32)
    idx = rng.integers(-1, G + 1, (Bn, cap)).astype(np.int32)
    score = rng.uniform(-0.1, 1.05, (Bn, cap)).astype(np.float32)
    track = np.stack([rng.integers(-1, 3000, (Bn, cap)), np.zeros((Bn, cap))], axis=2).astype(np.int32)
    names = [f"person{g}".encode() for g in range(G)]
    style = O.Style(flags=O.TRACK_ID, text_scale=1)
    kw = dict(det=det, counts=counts, idx=idx, score=score, id_stride=cap, track=track, names=names, style=style)
    got = device_draw(ctx, frames, cap, **kw)
    rc, host = host_draw(ctx.lib, frames, cap, **kw)
    assert rc == 0 and np.array_equal(got, host), np.argwhere(got != host)[:6]
    assert np.array_equal(got, O.draw(frames, cap=cap, glyphs=glyphs, **kw))
    assert np.array_equal(got[2], frames[2]) and all((got[b] != frames[b]).any() for b in (0, 1, 3))


def test_more_faces_than_one_cull_pass(ctx, glyphs):
    """cap = 300: the tile list is built 256 faces at a time and stays in ascending order across the passes"""
    cap, H, W = 300, 32, 96
    frames = frames_of(1, H, W, seed=7)
    det = np.zeros((1, cap, 5), np.float32)
    f = np.arange(cap)
    det[0, :, 0], det[0, :, 1] = (f * 7) % 70, (f * 5) % 14
    det[0, :, 2], det[0, :, 3] = det[0, :, 0] + 20, det[0, :, 1] + 16
    kw = dict(det=det, counts=np.array([cap], np.int32), idx=(f % 5 - 1).astype(np.int32).reshape(1, cap), score=np.full((1, cap), 0.5, np.float32),
              id_stride=cap, names=O.NAMES, style=O.Style(text_scale=0))
    got = device_draw(ctx, frames, cap, **kw)
    assert np.array_equal(got, O.draw(frames, cap=cap, glyphs=glyphs, **kw))


def test_refusals_leave_the_frames_untouched(ctx):
    lib, h = ctx.lib, ctx.handle
    H, W, Bn, cap = 20, 32, 2, 4
    frames = frames_of(Bn, H, W)
    det = np.zeros((Bn, cap, 5), np.float32)
    det[:, :, :4] = (3, 3, 15, 15)
    d_fr, d_det, d_counts = ctx.to_device(frames), ctx.to_device(det), ctx.to_device(np.full(Bn, 2, np.int32))
    d_idx, d_score = ctx.to_device(np.zeros(Bn * cap, np.int32)), ctx.to_device(np.ones(Bn * cap, np.float32))
    d_off = ctx.to_device(np.array([0, 2, 4], np.int32))
    p = lambda b: C.c_void_p(b.ptr)
    S = O.Style

    def draw(ctx_h=h, fr=p(d_fr), Bn=Bn, H=H, W=W, det=p(d_det), counts=p(d_counts), cap=cap, idx=p(d_idx), score=p(d_score), id_stride=cap, off=None,
             n_rows=0, style=S()):
        return lib.fid_draw_faces(ctx_h, fr, Bn, H, W, det, counts, cap, idx, score, id_stride, off, n_rows, None, None,
                                  C.byref(c_style(style)) if style is not None else None)

    bad = [dict(ctx_h=None), dict(fr=None), dict(det=None), dict(counts=None), dict(style=None), dict(Bn=0), dict(H=0), dict(W=-1), dict(cap=0),
           dict(Bn=1 << 20, cap=1 << 12), dict(H=1 << 15, W=1 << 15), dict(style=S(thickness=2)), dict(style=S(thickness=17)), dict(style=S(thickness=0)),
           dict(style=S(text_scale=5)), dict(style=S(text_scale=-1)), dict(style=S(proportion=np.nan)), dict(style=S(proportion=1.5)),
           dict(style=S(proportion=-0.1)), dict(score=None), dict(id_stride=0), dict(off=p(d_off), n_rows=-1), dict(n_rows=-1)]
    for kw in bad:
        assert draw(**kw) == -1 and len(lib.fid_last_error()) > 0, kw
    assert np.array_equal(d_fr.download(), frames)
    assert draw(off=p(d_off), n_rows=4, id_stride=0) == 0                  # (the rows form does not read id_stride)
    assert (d_fr.download() != frames).any()
    lab = C.c_void_p()
    from scrfd_arcface_facerecognition_amd._lib import c_i32_p
    off = np.array([0, 2, 1], np.int32)
    assert lib.fid_labels_create(h, b"abc", off.ctypes.data_as(c_i32_p), None, 2, C.byref(lab)) == -1
    assert lib.fid_labels_create(h, b"abc", off.ctypes.data_as(c_i32_p), None, 0, C.byref(lab)) == -1
    assert lib.fid_labels_create(h, b"abc", None, None, 2, C.byref(lab)) == -1 and lib.fid_labels_create(h, b"abc", off.ctypes.data_as(c_i32_p), None, 1, None) == -1
    assert lib.fid_labels_destroy(h, None) == 0


# ---- the pipelines ----------------------------------------------------------------------------------------------

H = W = 320
PB = 4
THRESH = -1.0                 # every face with a positive best cosine is named


class Scene:
    pass


@pytest.fixture(scope="module")
def scene(ctx):
    """SCRFD-500M at 320x320 and MobileFaceNet with seeded weights (the nets of the packed and tracked tests); 6 random frames"""
    old = os.environ.get("FID_AUTOTUNE")
    os.environ["FID_AUTOTUNE"] = "0"
    from scrfd_arcface_facerecognition_amd.engine import CompiledNet, Gallery, resolve_model
    from scrfd_arcface_facerecognition_amd.pipeline import calibrate_detector_bias
    s = Scene()
    s.frames = np.random.default_rng(41).integers(0, 256, (6, H, W, 3), dtype=np.uint8)
    det_net, det_P0 = resolve_model("synthetic:scrfd_500m?seed=5", (H, W))
    det_P, _ = calibrate_detector_bias(ctx, det_net, det_P0, s.frames[:4], target=30, max_batch=4)
    rec_net, rec_P = resolve_model("synthetic:arcface_mbf?seed=5")
    s.det = CompiledNet(ctx, det_net, det_P, max_batch=PB)
    s.rec = CompiledNet(ctx, rec_net, rec_P, max_batch=256)
    s.gallery = Gallery(ctx, np.random.default_rng(77).standard_normal((37, 512)).astype(np.float32))
    yield s
    if old is None:
        del os.environ["FID_AUTOTUNE"]
    else:
        os.environ["FID_AUTOTUNE"] = old


def make_pipe(ctx, s, kind):
    from scrfd_arcface_facerecognition_amd.pipeline import FacePipeline, PackedFacePipeline, TrackedFacePipeline
    if kind == "slots":
        return FacePipeline(ctx, s.det, s.rec, batch=PB, faces_per_frame=4)
    if kind == "rows":
        return PackedFacePipeline(ctx, s.det, s.rec, batch=PB, row_cap=256)
    return TrackedFacePipeline(ctx, s.det, s.rec, batch=PB, row_cap=256, refresh=1000, retry=1)


def oracle_of_step(pipe, kind, frames, names, glyphs, style):
    """the oracle fed with the downloaded det / counts / identities of the pipeline's last step"""
    det, counts, cap = pipe.post.det.download(), pipe.post.counts.download(), pipe.post.cap
    if kind == "slots":
        kw = dict(idx=pipe.idx.download().reshape(PB, pipe.F), score=pipe.score.download().reshape(PB, pipe.F), id_stride=pipe.F)
    elif kind == "rows":
        kw = dict(idx=pipe.idx.download(), score=pipe.score.download(), offsets=pipe.offsets.download(), n_rows=min(pipe.n_run, pipe.row_cap))
    else:
        kw = dict(idx=pipe.ident_idx.download(), score=pipe.ident_score.download(), id_stride=cap, track=pipe.track.download())
    return O.draw(frames, det, counts, cap, glyphs, names=names, style=style, **kw), int(np.clip(counts, 0, cap).sum())


@pytest.mark.parametrize("kind", ["slots", "rows", "tracked"])
def test_pipeline_draw_and_annotating_runner(ctx, scene, glyphs, kind):
    from scrfd_arcface_facerecognition_amd._lib import DRAW_TRACK_ID, DrawStyle
    from scrfd_arcface_facerecognition_amd.video import StreamRunner
    s = scene
    # one step, drawn with a style of the caller's
    pipe = make_pipe(ctx, s, kind)
    fr = ctx.to_device(s.frames[:PB])
    if kind == "tracked":
        pipe.detect(fr, H, W)
        pipe.embed(fr, H, W)
        with pytest.raises(RuntimeError):
            pipe.draw(fr, H, W, s.gallery)                                 # not identified yet
        pipe.match(s.gallery, THRESH)
    else:
        pipe.run_step(fr, H, W, s.gallery, THRESH)
    flags = DRAW_TRACK_ID if kind == "tracked" else 0
    pipe.draw(fr, H, W, s.gallery, DrawStyle(0.3, 5, 1, 1, flags, (0, 0, 255)))
    want, n_faces = oracle_of_step(pipe, kind, s.frames[:PB], s.gallery.names, glyphs, O.Style(0.3, 5, 1, 1, flags, (0, 0, 255)))
    got = fr.download()
    print(f"\n{kind}: {n_faces} faces, {int((got != s.frames[:PB]).any(axis=3).sum())} pixels drawn")
    assert n_faces > 0 and np.array_equal(got, want), np.argwhere(got != want)[:6]
    assert (got != s.frames[:PB]).any()
    if kind == "tracked":
        pipe.close()
    # the runner: 6 frames at B = 4, the second batch is padded
    pipe = make_pipe(ctx, s, kind)
    runner = StreamRunner(pipe, s.gallery, (H, W), similarity_thresh=THRESH, annotate=True)
    faces_a, want = [], None
    for i, (faces, frame) in enumerate(runner.run(iter(s.frames))):
        if i % PB == 0:                                                    # the step of this batch has run, the next one has not
            n = min(PB, 6 - i)
            batch = np.concatenate([s.frames[i:i + n], np.zeros((PB - n, H, W, 3), np.uint8)])
            want, _ = oracle_of_step(pipe, kind, batch, s.gallery.names, glyphs, O.Style())
        assert frame.shape == (H, W, 3) and np.array_equal(frame, want[i % PB]), i
        faces_a.append(faces)
    runner.close()
    if kind == "tracked":
        pipe.close()
    pipe = make_pipe(ctx, s, kind)
    runner = StreamRunner(pipe, s.gallery, (H, W), similarity_thresh=THRESH)
    faces_b = list(runner.run(iter(s.frames)))
    runner.close()
    if kind == "tracked":
        pipe.close()
    assert len(faces_a) == len(faces_b) == 6 and sum(len(r) for r in faces_b) > 0
    for ra, rb in zip(faces_a, faces_b):
        assert len(ra) == len(rb)
        for fa, fb in zip(ra, rb):
            assert np.array_equal(fa[0], fb[0]) and fa[1] == fb[1] and np.array_equal(fa[2], fb[2]) and fa[3:] == fb[3:]


def test_grouped_pipeline_refuses(ctx, scene):
    from scrfd_arcface_facerecognition_amd.pipeline import GroupedFacePipeline
    pipe = GroupedFacePipeline(ctx, scene.det, scene.rec, batch=PB, faces_per_frame=2, group=2)
    with pytest.raises(ValueError):
        pipe.draw(None, H, W, scene.gallery)


def test_label_table_is_cached_and_closed(ctx):
    from scrfd_arcface_facerecognition_amd.engine import Gallery, LabelTable
    g = Gallery(ctx, np.eye(3, 512, dtype=np.float32), ["a", "b", "c"])
    t = g.labels()
    assert isinstance(t, LabelTable) and g.labels() is t and t.G == 3
    g.close()
    assert t.handle is None
