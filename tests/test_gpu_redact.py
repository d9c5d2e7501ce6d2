"""GPU: fid_redact_faces / fid_redact_faces_nv12 against tests/redact_oracle.py and the host twins, byte for byte over whole allocations, guards
included; three tile columns by three tile rows; a cell whose sum passes 2^32; the refused calls; and the redaction inside the pipelines'
draw and the runner -- the redact oracle followed by the draw oracle on the step's downloaded det / counts / identities."""
import ctypes as C

import numpy as np
import pytest

import draw_nv12_oracle as N
import draw_oracle as O
import nv12_oracle
import redact_oracle as R
from draw_nv12_calls import GUARD, STANDARDS, background, layouts
from redact_calls import c_style, device_redact, device_redact_nv12, host_redact, host_redact_nv12, invalid_calls
from test_gpu_draw_nv12 import PB, PH, PW, THRESH, close, make_pipe, scene, step_faces  # noqa: F401  (scene: the fixture, set up once more here)

pytestmark = pytest.mark.gpu
INVALID = -1
BOTH = R.UNKNOWN | R.KNOWN


@pytest.fixture(scope="module")
def ctx():
    from scrfd_arcface_facerecognition_amd._lib import Context
    return Context(0)


@pytest.fixture(scope="module")
def glyphs(ctx):
    out = np.zeros(95 * 7, np.uint8)
    assert ctx.lib.fid_draw_glyphs(out.ctypes.data_as(C.c_void_p)) == 0
    return out.reshape(95, 7)


def frames_for(H, W, Bn=R.B):
    return np.random.default_rng(100 * H + W).integers(0, 256, (Bn, H, W, 3), dtype=np.uint8)


# ---- 1. the case list ----
@pytest.mark.parametrize("H, W", [(48, 80), (37, 67)])
def test_case_list_equals_the_oracle_and_the_host_bgr(ctx, H, W):
    frames = frames_for(H, W)
    for name, kw in R.cases(H, W):
        got = device_redact(ctx, frames, R.CAP, **kw)
        want = R.redact(frames, cap=R.CAP, **kw)
        rc, host = host_redact(ctx.lib, frames, R.CAP, **kw)
        assert rc == 0 and np.array_equal(host, want), name
        assert np.array_equal(got, want), (name, np.argwhere(got != want)[:6])


@pytest.mark.parametrize("standard", STANDARDS)
@pytest.mark.parametrize("lname", ["dwords", "w+6"])
@pytest.mark.parametrize("H, W", [(48, 80), (38, 68)])
def test_case_list_equals_the_oracle_and_the_host_nv12(ctx, H, W, lname, standard):
    lay = layouts(H, W)[lname]
    buf = background(H + W, R.B, H, W, lay, exact=True)
    assert lname == "dense" or (buf == GUARD).sum() > 100
    for name, kw in R.cases(H, W):
        got = device_redact_nv12(ctx, buf, R.B, H, W, lay, standard, R.CAP, **kw)
        want = R.redact_nv12(buf, R.B, H, W, cap=R.CAP, standard=standard, **lay, **kw)
        rc, host = host_redact_nv12(ctx.lib, buf, R.B, H, W, lay, standard, R.CAP, **kw)
        assert rc == 0 and np.array_equal(host, want), name
        assert np.array_equal(got, want), (name, np.argwhere(got != want)[:6])


# ---- 2. three tile columns, three tile rows ----
def wide_scene(W):
    """one region over every 64 x 16 tile of a 48 x W frame, one small region inside a tile, one across the corner of four tiles, one whose
    edges are no multiple of four"""
    det = np.zeros((1, 4, 5), np.float32)
    det[0, :, :4] = [(0, 0, W - 1, 47), (72, 19, 80, 27), (60, 12, 70, 21), (97, 3, 122, 30)]
    return det, np.array([4], np.int32)


@pytest.mark.parametrize("style", [R.Style(who=BOTH, expand=0.0), R.Style(who=BOTH, cells=16, expand=0.3), R.Style(mode=R.FILL, who=BOTH, fill_bgr=(9, 200, 77))])
@pytest.mark.parametrize("W", [192, 190])
def test_three_by_three_tiles(ctx, W, style):
    H = 48
    det, counts = wide_scene(W)
    frames = frames_for(H, W, 1)
    want = R.redact(frames, det, counts, 4, style=style)
    got = device_redact(ctx, frames, 4, det, counts, style=style)                              # W = 192: dword rows; 190: byte stores only
    assert (want != frames).mean() > 0.9 and np.array_equal(got, want), np.argwhere(got != want)[:6]
    for order in ([3, 2, 1, 0], [1, 0, 3, 2]):                                                 # the big region last: it hides the others
        d = det[:, order]
        assert np.array_equal(device_redact(ctx, frames, 4, d, counts, style=style), R.redact(frames, d, counts, 4, style=style)), order
    for lname in ("dwords", "w+6"):
        lay = layouts(H, W)[lname]
        buf = background(W, 1, H, W, lay, exact=True)
        got = device_redact_nv12(ctx, buf, 1, H, W, lay, "bt709", 4, det, counts, style=style)
        want = R.redact_nv12(buf, 1, H, W, det, counts, 4, standard="bt709", **lay, style=style)
        assert np.array_equal(got, want), (lname, np.argwhere(got != want)[:6])


def test_more_faces_than_one_cull_pass(ctx):
    """300 faces in one frame: the cull lists 256 at a time, and a face of the second pass lies over faces of the first"""
    H, W, n = 48, 192, 300
    rng = np.random.default_rng(5)
    det = np.zeros((1, n, 5), np.float32)
    x, y = rng.integers(-4, W - 4, n), rng.integers(-4, H - 4, n)
    det[0, :, 0], det[0, :, 1], det[0, :, 2], det[0, :, 3] = x, y, x + rng.integers(2, 30, n), y + rng.integers(2, 20, n)
    det[0, 299, :4] = (50, 10, 150, 40)
    frames = frames_for(H, W, 1)
    style = R.Style(who=BOTH, cells=4)
    got = device_redact(ctx, frames, n, det, np.array([n], np.int32), style=style)
    want = R.redact(frames, det, np.array([n]), n, style=style)
    assert np.array_equal(got, want), np.argwhere(got != want)[:6]


# ---- 3. a sum past 2^32 ----
def test_a_sum_past_32_bits(ctx):
    """4200 x 4200 of solid 255 under one cell: 17 640 000 x 255 = 4 498 200 000 per channel; one face per launch"""
    S = 4200
    det = np.zeros((1, 1, 5), np.float32)
    det[0, 0, :4] = (0, 0, S - 1, S - 1)
    style = R.Style(cells=1, expand=0.0)
    g = R.geometry(det[0, 0], style)
    assert g["c"] == S and R.clipped(g, S, S) == (0, 0, S - 1, S - 1) and S * S * 255 > 2 ** 32
    solid = np.full((1, S, S, 3), 255, np.uint8)
    got = device_redact(ctx, solid, 1, det, np.array([1], np.int32), style=style)
    assert np.array_equal(got, np.full((1, S, S, 3), 255, np.uint8))
    lay = nv12_oracle.dense_layout(S, S)
    got = device_redact_nv12(ctx, solid.reshape(-1)[:S * S * 3 // 2], 1, S, S, lay, "bt601", 1, det, np.array([1], np.int32), style=style)
    assert np.array_equal(got, np.full(S * S * 3 // 2, 255, np.uint8))
    # ... and a frame that is not flat: the mean of a half-and-half frame is (255 n / 2 + n / 2) / n = 128
    half = np.full((1, S, S, 3), 255, np.uint8)
    half[0, : S // 2] = 0
    got = device_redact(ctx, half, 1, det, np.array([1], np.int32), style=style)
    assert np.array_equal(got, np.full((1, S, S, 3), 128, np.uint8))


# ---- 4. refusals ----
def test_refusals_leave_the_frames_untouched(ctx):
    H, W = 48, 80
    frames = frames_for(H, W)
    base = dict(R.cases(H, W))["slots, who 3"]
    lay = layouts(H, W)["w+6"]
    buf = background(7, R.B, H, W, lay, exact=True)
    for what, over, style in invalid_calls(base["style"]):
        kw = dict(base, **over, style=style)
        cap = kw.pop("cap", R.CAP)
        assert np.array_equal(device_redact(ctx, frames, cap, expect=INVALID, **kw), frames), what
        assert np.array_equal(device_redact_nv12(ctx, buf, R.B, H, W, lay, "bt601", cap, expect=INVALID, **kw), buf), what
    for what, bad in (("pitch below W", dict(lay, pitch=W - 2)), ("overlapping planes", dict(lay, uv_offset=lay["pitch"] * H - 1)),
                      ("overlapping frames", dict(lay, frame_stride=lay["uv_offset"]))):
        assert np.array_equal(device_redact_nv12(ctx, buf, R.B, H, W, bad, "bt601", R.CAP, expect=INVALID, **base), buf), what
    assert np.array_equal(device_redact_nv12(ctx, buf, R.B, H, W, lay, 3, R.CAP, expect=INVALID, **base), buf)
    assert np.array_equal(device_redact_nv12(ctx, buf, R.B, H - 1, W, lay, "bt601", R.CAP, expect=INVALID, **base), buf)
    null = C.c_void_p(None)
    st = C.byref(c_style(base["style"]))
    assert ctx.lib.fid_redact_faces(None, null, 1, 8, 8, null, null, 1, null, null, 0, null, 0, st) == INVALID          # a NULL context
    assert ctx.lib.fid_redact_faces(ctx.handle, null, 1, 8, 8, null, null, 1, null, null, 0, null, 0, st) == INVALID    # NULL frames


# ---- 5. the pipelines and the runner ----
def redact_kw(kw):
    """the draw oracle's keywords of a step -> the redact oracle's"""
    return {k: v for k, v in kw.items() if k in ("det", "counts", "cap", "idx", "score", "id_stride", "offsets", "n_rows")}


def ostyle_of(rstyle):
    return R.Style(rstyle.mode, rstyle.who, rstyle.cells, rstyle.expand, tuple(rstyle.fill_bgr)[:3])


@pytest.mark.parametrize("kind", ["slots", "rows", "tracked"])
def test_pipeline_draw_with_redact(ctx, scene, glyphs, kind):
    """the four combinations of input format x out: the redact oracle, then the draw oracle"""
    from scrfd_arcface_facerecognition_amd._lib import DrawStyle, Nv12Frames, RedactStyle
    s = scene
    cstyle, ostyle = DrawStyle(0.3, 3, 1, 1, 0, (0, 0, 255)), O.Style(0.3, 3, 1, 1, 0, (0, 0, 255))
    rstyle = RedactStyle(who=BOTH, cells=6, expand=0.2)
    clean = s.nv12[:PB].reshape(-1)
    bgr_clean = nv12_oracle.nv12_to_bgr(clean, PB, PH, PW, standard="bt709")
    # NV12 in
    pipe = make_pipe(ctx, s, kind)
    dev = ctx.to_device(s.nv12[:PB])
    fr = Nv12Frames(dev, PH, PW, standard="bt709")
    pipe.run_step(fr, PH, PW, s.gallery, THRESH)
    kw, n_faces = step_faces(pipe, kind, s.gallery.names, ostyle)
    rk = redact_kw(kw)
    assert n_faces > 0 and len(list(R.selected_faces(PB, style=ostyle_of(rstyle), **rk))) > 0
    with pytest.raises(TypeError):
        pipe.draw(fr, PH, PW, s.gallery, cstyle, redact=cstyle)
    # ... out=None: the input stays, the pipeline's BGR buffer is redacted and drawn on
    ret = pipe.draw(fr, PH, PW, s.gallery, cstyle, redact=rstyle)
    assert ret is pipe.bgr and np.array_equal(dev.download().reshape(-1), clean)
    red = R.redact(bgr_clean, style=ostyle_of(rstyle), **rk)
    assert (red != bgr_clean).any() and np.array_equal(ret.download(), O.draw(red, glyphs=glyphs, **kw))
    # ... redact=None: today's result
    ret = pipe.draw(fr, PH, PW, s.gallery, cstyle)
    assert np.array_equal(ret.download(), O.draw(bgr_clean, glyphs=glyphs, **kw)) and np.array_equal(dev.download().reshape(-1), clean)
    # ... out="nv12": in place on the planes
    ret = pipe.draw(fr, PH, PW, s.gallery, cstyle, out="nv12", redact=rstyle)
    red = R.redact_nv12(clean, PB, PH, PW, standard="bt709", style=ostyle_of(rstyle), **rk)
    assert ret is fr and (red != clean).any()
    assert np.array_equal(dev.download().reshape(-1), N.draw_nv12(red, PB, PH, PW, glyphs=glyphs, standard="bt709", **kw))
    # ... redact() on its own: FILL over the unknown faces only, on fresh frames
    dev.upload(s.nv12[:PB])
    fill = RedactStyle(mode=R.FILL, who=R.UNKNOWN, fill_bgr=(10, 200, 30))
    assert pipe.redact(fr, PH, PW, fill) is fr
    assert np.array_equal(dev.download().reshape(-1), R.redact_nv12(clean, PB, PH, PW, standard="bt709", style=ostyle_of(fill), **rk))
    close(pipe, kind)
    # BGR in
    pipe = make_pipe(ctx, s, kind)
    pipe.nv12_standard = "bt601_full"
    bdev = ctx.to_device(s.bgr[:PB])
    pipe.run_step(bdev, PH, PW, s.gallery, THRESH)
    kw, n_faces = step_faces(pipe, kind, s.gallery.names, ostyle)
    rk = redact_kw(kw)
    want = O.draw(R.redact(s.bgr[:PB], style=ostyle_of(rstyle), **rk), glyphs=glyphs, **kw)
    assert pipe.draw(bdev, PH, PW, s.gallery, cstyle, redact=rstyle) is bdev and np.array_equal(bdev.download(), want)
    bdev.upload(s.bgr[:PB])
    ret = pipe.draw(bdev, PH, PW, s.gallery, cstyle, out="nv12", redact=rstyle)
    assert ret is pipe.nv12_out and np.array_equal(bdev.download(), want)
    assert np.array_equal(ret.buf.download().reshape(-1), N.bgr_to_nv12(want, np.zeros(clean.size, np.uint8), "bt601_full"))
    bdev.upload(s.bgr[:PB])
    assert pipe.draw(bdev, PH, PW, s.gallery, cstyle) is bdev and np.array_equal(bdev.download(), O.draw(s.bgr[:PB], glyphs=glyphs, **kw))
    # ... the default style hides the unknown faces: with a threshold nobody reaches, everybody (a fresh pipeline: a track keeps its name)
    close(pipe, kind)
    pipe = make_pipe(ctx, s, kind)
    bdev.upload(s.bgr[:PB])
    pipe.run_step(bdev, PH, PW, s.gallery, 2.0)
    kw, _ = step_faces(pipe, kind, s.gallery.names, ostyle)
    rk = redact_kw(kw)
    assert pipe.redact(bdev, PH, PW) is bdev
    red = R.redact(s.bgr[:PB], style=R.Style(), **rk)
    assert (red != s.bgr[:PB]).any() and np.array_equal(bdev.download(), red)
    close(pipe, kind)


@pytest.mark.parametrize("fmt, out", [("nv12", "nv12"), ("bgr", "bgr")])
@pytest.mark.parametrize("kind", ["slots", "tracked"])
def test_runner_redacts_like_a_manual_step(ctx, scene, glyphs, kind, fmt, out):
    """five frames at B = 2 (the last batch is padded): every yielded frame is the redact oracle, then the draw oracle, on that step's arrays"""
    from scrfd_arcface_facerecognition_amd._lib import RedactStyle
    from scrfd_arcface_facerecognition_amd.video import StreamRunner
    s = scene
    rstyle = RedactStyle(who=BOTH)
    items = s.nv12 if fmt == "nv12" else s.bgr
    pipe = make_pipe(ctx, s, kind)
    runner = StreamRunner(pipe, s.gallery, (PH, PW), similarity_thresh=THRESH, annotate=True, pixel_format=fmt, standard="bt709",
                          annotate_format=out, redact=rstyle)
    want, redacted = None, 0
    for i, (faces, frame) in enumerate(runner.run(iter(items))):
        if i % PB == 0:
            n = min(PB, 5 - i)
            kw, _ = step_faces(pipe, kind, s.gallery.names, O.Style())
            rk = redact_kw(kw)
            if fmt == "nv12":
                pad = np.zeros((PB - n, PH * 3 // 2, PW), np.uint8)
                pad[:, PH:] = 128
                batch = np.concatenate([s.nv12[i:i + n], pad]).reshape(-1)
                red = R.redact_nv12(batch, PB, PH, PW, standard="bt709", style=ostyle_of(rstyle), **rk)
                want = N.draw_nv12(red, PB, PH, PW, glyphs=glyphs, standard="bt709", **kw).reshape(PB, PH * 3 // 2, PW)
            else:
                batch = np.concatenate([s.bgr[i:i + n], np.zeros((PB - n, PH, PW, 3), np.uint8)])
                red = R.redact(batch, style=ostyle_of(rstyle), **rk)
                want = O.draw(red, glyphs=glyphs, **kw)
            redacted += int((red != batch).any())
        assert np.array_equal(frame, want[i % PB]), i
    runner.close()
    close(pipe, kind)
    assert redacted >= 2


@pytest.mark.parametrize("fmt", ["nv12", "bgr"])
def test_runner_yields_the_frames_of_a_manual_step(ctx, scene, fmt):
    """one batch through StreamRunner(annotate=True, redact=style), and the same batch through run_step + draw(redact=style) by hand"""
    from scrfd_arcface_facerecognition_amd._lib import Nv12Frames, RedactStyle
    from scrfd_arcface_facerecognition_amd.video import StreamRunner
    s = scene
    rstyle = RedactStyle(who=BOTH, cells=5)
    items = (s.nv12 if fmt == "nv12" else s.bgr)[:PB]
    pipe = make_pipe(ctx, s, "rows")
    runner = StreamRunner(pipe, s.gallery, (PH, PW), similarity_thresh=THRESH, annotate=True, pixel_format=fmt, standard="bt709",
                          annotate_format=fmt, redact=rstyle)
    got = [frame for _, frame in runner.run(iter(items))]
    runner.close()
    plain = StreamRunner(pipe, s.gallery, (PH, PW), similarity_thresh=THRESH, annotate=True, pixel_format=fmt, standard="bt709", annotate_format=fmt)
    unredacted = [frame for _, frame in plain.run(iter(items))]
    plain.close()
    pipe = make_pipe(ctx, s, "rows")
    dev = ctx.to_device(items)
    fr = Nv12Frames(dev, PH, PW, standard="bt709") if fmt == "nv12" else dev
    pipe.run_step(fr, PH, PW, s.gallery, THRESH)
    ret = pipe.draw(fr, PH, PW, s.gallery, out="nv12" if fmt == "nv12" else None, redact=rstyle)
    manual = (ret.buf if fmt == "nv12" else ret).download()
    assert len(got) == PB and all(np.array_equal(g, m) for g, m in zip(got, manual))
    assert any((g != u).any() for g, u in zip(got, unredacted))


def test_runner_and_grouped_refusals(ctx, scene):
    from scrfd_arcface_facerecognition_amd._lib import REDACT_KNOWN, RedactStyle
    from scrfd_arcface_facerecognition_amd.pipeline import GroupedFacePipeline
    from scrfd_arcface_facerecognition_amd.video import StreamRunner
    pipe = make_pipe(ctx, scene, "slots")
    with pytest.raises(ValueError):
        StreamRunner(pipe, scene.gallery, (PH, PW), redact=RedactStyle())                       # redact without annotate
    r = StreamRunner(pipe, scene.gallery, (PH, PW), annotate=True, redact=RedactStyle())
    r.close()
    grouped = GroupedFacePipeline(ctx, scene.det, scene.rec, batch=PB, faces_per_frame=2, group=2)
    with pytest.raises(ValueError):
        grouped.redact(None, PH, PW, RedactStyle(who=REDACT_KNOWN))
    # a grouped step has no identities yet: every detection is redacted as unknown
    bdev = ctx.to_device(scene.bgr[:PB])
    grouped.collect(bdev, PH, PW)
    assert grouped.redact(bdev, PH, PW) is bdev
    det, counts, cap = grouped.post.det.download(), grouped.post.counts.download(), grouped.post.cap
    want = R.redact(scene.bgr[:PB], det, counts, cap)
    assert (want != scene.bgr[:PB]).any() and np.array_equal(bdev.download(), want)
