"""GPU: annotated video out as NV12 (fid_bgr_to_nv12, fid_draw_faces_nv12; FacePipeline.draw(out="nv12") and its subclasses;
video.StreamRunner(annotate_format="nv12")).  The yardsticks are tests/draw_nv12_oracle.py and the host twins, every comparison byte for byte
over the WHOLE allocation, so that padding between W and pitch, between the planes and behind the frames is compared too (it holds 0xA5).
The direct cases upload synthetic det / counts / idx / score / track arrays; no network runs in them."""
import ctypes as C
import os

import numpy as np
import pytest

import draw_nv12_oracle as N
import draw_oracle as O
import nv12_oracle
from draw_calls import c_style
from draw_calls import device_draw as device_draw_bgr
from draw_nv12_calls import GUARD, STANDARDS, background, desc_of, device_draw, host_draw, layouts

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


# ---- 1. the conversion ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("standard", STANDARDS)
@pytest.mark.parametrize("H, W", [(16, 18), (32, 64)])
def test_bgr_to_nv12_equals_the_oracle(ctx, standard, H, W):
    """W = 18: no multiple of 4, the last thread of a row owns one group; W = 64 dense and "dwords": the dword path; "w+6": byte stores"""
    from scrfd_arcface_facerecognition_amd._lib import check
    Bn = 2
    frames = np.random.default_rng(H * W).integers(0, 256, (Bn, H, W, 3), dtype=np.uint8)
    src = ctx.to_device(frames)
    for name, lay in layouts(H, W).items():
        n = Bn * lay["frame_stride"] + 64
        out = ctx.to_device(np.full(n, GUARD, np.uint8))
        check(ctx.lib.fid_bgr_to_nv12(ctx.handle, C.c_void_p(src.ptr), Bn, H, W, C.c_void_p(out.ptr), C.byref(desc_of(H, W, lay, standard))))
        got = out.download()
        want = N.bgr_to_nv12(frames, np.full(n, GUARD, np.uint8), standard, **lay)
        assert np.array_equal(got, want), (name, np.argwhere(got != want)[:6])
        owned = np.zeros(n, np.uint8)
        for b in range(Bn):
            for plane in N.planes(owned, b, H, W, **lay):
                plane[...] = 1
        assert (got[owned == 0] == GUARD).all() and int(owned.sum()) == Bn * H * W * 3 // 2      # every other byte is still 0xA5
        rc = ctx.lib.fid_bgr_to_nv12_host(frames.ctypes.data_as(C.c_void_p), Bn, H, W, want.ctypes.data_as(C.c_void_p), C.byref(desc_of(H, W, lay, standard)))
        assert rc == 0 and np.array_equal(got, want)                                              # (the host twin rewrites the same bytes)
    assert np.array_equal(src.download(), frames)


# ---- 2. the overlay against the oracle and the host twin ---------------------------------------------------------------

@pytest.mark.parametrize("lname", ["dwords", "w+6"])
@pytest.mark.parametrize("H, W", [(48, 80), (38, 68)])
def test_case_list_equals_the_oracle_and_the_host(ctx, glyphs, H, W, lname):
    lay = layouts(H, W)[lname]
    buf = background(H + W, O.B, H, W, lay)
    for i, (name, kw) in enumerate(O.cases(H, W)):
        std = STANDARDS[i % 3]
        got = device_draw(ctx, buf, O.B, H, W, lay, std, O.CAP, **kw)
        want = N.draw_nv12(buf, O.B, H, W, cap=O.CAP, glyphs=glyphs, standard=std, **kw, **lay)
        assert np.array_equal(got, want), (name, np.argwhere(got != want)[:6])
        rc, host = host_draw(ctx.lib, buf, O.B, H, W, lay, std, O.CAP, **kw)
        assert rc == 0 and np.array_equal(got, host), name
        if name == "an empty frame between two drawn ones":
            fs = lay["frame_stride"]
            assert np.array_equal(got[fs:2 * fs], buf[fs:2 * fs]) and (got[:fs] != buf[:fs]).any() and (got[2 * fs:] != buf[2 * fs:]).any()


def wide_scene():
    """48 x 192: three tile columns and three tile rows of 64 x 16.  Face 0's extent covers every tile; its thick arms and its bar fill whole
    aligned groups of four pixels (the dword stores of both planes) and cross every tile boundary"""
    H, W, cap = 48, 192, 6
    boxes = [[(8, 8, 160, 44), (60, 12, 70, 20), (170, 2, 190, 44), (-5, 14, 66, 18)],
             [(0, 0, 191, 47), (62, 14, 66, 18)],
             []]
    det, counts = np.zeros((3, cap, 5), np.float32), np.array([len(b) for b in boxes], np.int32)
    for b, fr in enumerate(boxes):
        if fr:
            det[b, :len(fr), :4] = fr
    idx = np.array([[0, -1, 1, 2, 0, 0], [3, 0, 0, 0, 0, 0], [0] * 6], np.int32)
    score = np.array([[0.9, 0, 0.5, 0.25, 0, 0], [1.0, 0.4, 0, 0, 0, 0], [0] * 6], np.float32)
    return H, W, cap, dict(det=det, counts=counts, idx=idx, score=score, id_stride=cap, names=O.NAMES)


@pytest.mark.parametrize("lname", ["dwords", "w+6"])
@pytest.mark.parametrize("style", [O.Style(thickness=7, text_scale=1), O.Style(thickness=15, text_scale=2, proportion=0.5), O.Style(thickness=1, text_scale=0)])
def test_three_by_three_tiles(ctx, glyphs, style, lname):
    H, W, cap, kw = wide_scene()
    lay = layouts(H, W)[lname]
    buf = background(4, 3, H, W, lay)
    got = device_draw(ctx, buf, 3, H, W, lay, "bt709", cap, style=style, **kw)
    want = N.draw_nv12(buf, 3, H, W, cap=cap, glyphs=glyphs, standard="bt709", style=style, **kw, **lay)
    assert np.array_equal(got, want), np.argwhere(got != want)[:6]
    fs = lay["frame_stride"]
    assert np.array_equal(got[2 * fs:], buf[2 * fs:])
    if style.thickness > 1:        # four adjacent covered pixels at a multiple of four, two adjacent written pairs: the wide paths had work
        last = N.last_face(3, H, W, kw["det"], kw["counts"], cap, glyphs, **{k: v for k, v in kw.items() if k not in ("det", "counts")}, style=style)
        m = last[0] >= 0
        assert m.reshape(H, W // 4, 4).all(axis=2).any()
        assert m.reshape(H // 2, 2, W // 2, 2).any(axis=(1, 3)).reshape(H // 2, W // 4, 2).all(axis=2).any()


# ---- 3. chroma boundaries, by hand ---------------------------------------------------------------------------------------

BG_Y, BG_U, BG_V = 50, 90, 200


def flat_frame(H, W, lay, Bn=1):
    """background (BG_Y, BG_U, BG_V) in every byte the layout owns, GUARD elsewhere"""
    buf = np.full(Bn * lay["frame_stride"], GUARD, np.uint8)
    for b in range(Bn):
        y, uv = N.planes(buf, b, H, W, **lay)
        y[...] = BG_Y
        uv[...] = (BG_U, BG_V)
    return buf


THIN = O.Style(thickness=1, text_scale=0, bar=0, unknown_bgr=(255, 0, 0))


@pytest.mark.parametrize("lname", ["dwords", "w+6"])
def test_box_on_odd_edges(ctx, lname):
    """the outline x = 5 | 21, y = 7 | 19 cuts through groups: every group it touches gets the pair, their uncovered Y bytes stay"""
    H, W = 32, 48
    lay = layouts(H, W)[lname]
    buf = flat_frame(H, W, lay)
    det = np.zeros((1, 1, 5), np.float32)
    det[0, 0, :4] = (5, 7, 21, 19)
    got = device_draw(ctx, buf, 1, H, W, lay, "bt601", 1, det=det, counts=np.array([1], np.int32), style=THIN)
    yc, uc, vc = N.colour_yuv((255, 0, 0))
    assert yc != BG_Y and (uc, vc) != (BG_U, BG_V)
    y, uv = N.planes(got, 0, H, W, **lay)
    want_y = np.zeros((H, W), bool)
    want_y[7, 5:22] = want_y[19, 5:22] = want_y[7:20, 5] = want_y[7:20, 21] = True
    assert np.array_equal(y != BG_Y, want_y) and (y[want_y] == yc).all()
    want_uv = np.zeros((H // 2, W // 2), bool)
    want_uv[3, 2:11] = want_uv[9, 2:11] = want_uv[3:10, 2] = want_uv[3:10, 10] = True
    written = (uv != (BG_U, BG_V)).any(axis=2)
    assert np.array_equal(written, want_uv) and (uv[want_uv] == (uc, vc)).all()
    assert (uv[~want_uv] == (BG_U, BG_V)).all()                            # a group no face covers keeps its pair
    assert y[6, 4] == BG_Y and y[6, 5] == BG_Y and y[7, 4] == BG_Y and y[7, 5] == yc      # group (3, 2): one pixel of four is covered
    clean = flat_frame(H, W, lay)
    y0, uv0 = N.planes(clean, 0, H, W, **lay)
    y0[want_y] = yc
    uv0[want_uv] = (uc, vc)
    assert np.array_equal(got, clean)                                      # ... and nothing else anywhere, padding included


@pytest.mark.parametrize("later_first", [False, True])
def test_one_pixel_of_a_group_wins_the_pair(ctx, later_first):
    """group x 10..11, y 10..11: face A's top-left corner covers (10,10), (11,10), (10,11); face B's top-left corner covers (11,11) alone.
    Drawn A then B the pair is B's; drawn B then A it is A's"""
    H, W = 32, 48
    lay = layouts(H, W)["dwords"]
    buf = flat_frame(H, W, lay)
    A, B_ = (10, 10, 40, 28), (11, 11, 30, 30)
    colours = np.array([(10, 200, 30), (200, 40, 250)], np.uint8)
    det = np.zeros((1, 2, 5), np.float32)
    det[0, :, :4] = (B_, A) if later_first else (A, B_)
    idx = np.array([[1, 0]] if later_first else [[0, 1]], np.int32)
    got = device_draw(ctx, buf, 1, H, W, lay, "bt601", 2, det=det, counts=np.array([2], np.int32), idx=idx, score=np.zeros((1, 2), np.float32),
                      id_stride=2, names=[b"a", b"b"], bgr=colours, style=THIN)
    y, uv = N.planes(got, 0, H, W, **lay)
    ya, ua, va = N.colour_yuv(colours[0])
    yb, ub, vb = N.colour_yuv(colours[1])
    assert len({ya, yb, BG_Y}) == 3 and (ua, va) != (ub, vb)
    assert (y[10, 10], y[10, 11], y[11, 10], y[11, 11]) == (ya, ya, ya, yb)
    assert tuple(uv[5, 5]) == ((ua, va) if later_first else (ub, vb))


def test_pair_across_two_cull_passes(ctx, glyphs):
    """cap = 300: the tile's list is built 256 faces at a time.  Group x 80..81, y 20..21 is touched by face 10 (three pixels) and by face 290
    (three pixels, one of them its own alone): the pair is face 290's"""
    cap, H, W = 300, 32, 96
    lay = layouts(H, W)["dwords"]
    buf = flat_frame(H, W, lay)
    f = np.arange(cap)
    det = np.zeros((1, cap, 5), np.float32)
    det[0, :, 0], det[0, :, 1] = (f * 7) % 50, (f * 5) % 14
    det[0, :, 2], det[0, :, 3] = det[0, :, 0] + 6, det[0, :, 1] + 6
    det[0, 10, :4] = (80, 20, 90, 28)
    det[0, 290, :4] = (70, 10, 81, 21)
    names = [b"n%d" % g for g in range(cap)]
    kw = dict(det=det, counts=np.array([cap], np.int32), idx=f.astype(np.int32).reshape(1, cap), score=np.zeros((1, cap), np.float32), id_stride=cap,
              names=names, style=THIN)
    got = device_draw(ctx, buf, 1, H, W, lay, "bt601", cap, **kw)
    assert np.array_equal(got, N.draw_nv12(buf, 1, H, W, cap=cap, glyphs=glyphs, **kw, **lay))
    y, uv = N.planes(got, 0, H, W, **lay)
    y10, u10, v10 = N.colour_yuv(O.default_bgr(10))
    y290, u290, v290 = N.colour_yuv(O.default_bgr(290))
    assert (u10, v10) != (u290, v290) and y10 != y290
    assert (y[20, 80], y[20, 81], y[21, 80], y[21, 81]) == (y10, y290, y290, y290)
    assert tuple(uv[10, 40]) == (u290, v290)
    assert tuple(uv[10, 41]) == (u10, v10)                                 # the next group along face 10's top edge is face 10's alone


# ---- 4. relation to the BGR draw -----------------------------------------------------------------------------------------

def test_same_pixels_as_the_bgr_draw(ctx, glyphs):
    from scrfd_arcface_facerecognition_amd._lib import check
    H, W = 48, 80
    lay = layouts(H, W)["dense"]
    name, kw = O.cases(H, W)[0]
    faces = list(N.faces_in_order(O.B, H, W, kw["det"], kw["counts"], O.CAP, glyphs, **{k: v for k, v in kw.items() if k not in ("det", "counts")}))
    ys = {N.colour_yuv(c)[0] for _, _, _, c in faces}
    bg_y = next(v for v in range(60, 256) if v not in ys)                  # a luma no colour has
    buf = np.full(O.B * lay["frame_stride"], 128, np.uint8)                # neutral chroma: a grey background
    for b in range(O.B):
        N.planes(buf, b, H, W, **lay)[0][...] = bg_y
    clean_bgr = nv12_oracle.nv12_to_bgr(buf, O.B, H, W, **lay)
    assert all(tuple(int(v) for v in clean_bgr[0, 0, 0]) != c for _, _, _, c in faces)
    got = device_draw(ctx, buf, O.B, H, W, lay, "bt601", O.CAP, **kw)
    drawn_bgr = device_draw_bgr(ctx, clean_bgr, O.CAP, **kw)
    changed_bgr = (drawn_bgr != clean_bgr).any(axis=3)
    changed_y = np.stack([N.planes(got, b, H, W, **lay)[0] != bg_y for b in range(O.B)])
    assert changed_bgr.any() and np.array_equal(changed_y, changed_bgr)
    # a group wholly covered, all four pixels by the same last face: the drawn frame converts back to that face's colour within 2 levels
    last = N.last_face(O.B, H, W, kw["det"], kw["counts"], O.CAP, glyphs, **{k: v for k, v in kw.items() if k not in ("det", "counts")})
    g = last.reshape(O.B, H // 2, 2, W // 2, 2)
    whole = (g >= 0).all(axis=(2, 4)) & (g.max(axis=(2, 4)) == g.min(axis=(2, 4)))
    assert whole.sum() > 20
    dev = ctx.to_device(got)
    back = ctx.empty((O.B, H, W, 3), np.uint8)
    check(ctx.lib.fid_nv12_to_bgr(ctx.handle, C.c_void_p(dev.ptr), C.byref(desc_of(H, W, lay, "bt601")), O.B, H, W, C.c_void_p(back.ptr)))
    back = back.download().astype(np.int64)
    px = whole.repeat(2, axis=1).repeat(2, axis=2)
    err = np.abs(back - drawn_bgr.astype(np.int64))[px]
    print(f"\n{int(whole.sum())} whole groups, max error {err.max()}")
    assert err.max() <= 2


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_frames_untouched(ctx):
    from scrfd_arcface_facerecognition_amd._lib import nv12_desc
    lib, h = ctx.lib, ctx.handle
    H, W, Bn, cap = 20, 32, 2, 4
    lay = layouts(H, W)["dwords"]
    buf = background(1, Bn, H, W, lay)
    det = np.zeros((Bn, cap, 5), np.float32)
    det[:, :, :4] = (3, 3, 15, 15)
    d_fr, d_det, d_counts = ctx.to_device(buf), ctx.to_device(det), ctx.to_device(np.full(Bn, 2, np.int32))
    d_idx, d_score = ctx.to_device(np.zeros(Bn * cap, np.int32)), ctx.to_device(np.ones(Bn * cap, np.float32))
    d_off = ctx.to_device(np.array([0, 2, 4], np.int32))
    bgr = np.random.default_rng(2).integers(0, 256, (Bn, H, W, 3), dtype=np.uint8)
    d_bgr = ctx.to_device(bgr)
    p = lambda b: C.c_void_p(b.ptr)
    S = O.Style
    good = nv12_desc(H, W, **lay)

    def draw(ctx_h=h, fr=p(d_fr), desc=good, Bn=Bn, H=H, W=W, det=p(d_det), counts=p(d_counts), cap=cap, idx=p(d_idx), score=p(d_score), id_stride=cap,
             off=None, n_rows=0, style=S()):
        return lib.fid_draw_faces_nv12(ctx_h, fr, C.byref(desc) if desc is not None else None, Bn, H, W, det, counts, cap, idx, score, id_stride, off,
                                       n_rows, None, None, C.byref(c_style(style)) if style is not None else None)

    def convert(ctx_h=h, src=p(d_bgr), Bn=Bn, H=H, W=W, out=p(d_fr), desc=good):
        return lib.fid_bgr_to_nv12(ctx_h, src, Bn, H, W, out, C.byref(desc) if desc is not None else None)

    bad_layouts = [dict(W=W - 1), dict(H=H - 1), dict(desc=None),
                   dict(desc=nv12_desc(H, W, pitch=W - 2, uv_offset=lay["uv_offset"], frame_stride=lay["frame_stride"])),
                   dict(desc=nv12_desc(H, W, pitch=lay["pitch"], uv_offset=lay["pitch"] * H - 1, frame_stride=lay["frame_stride"])),
                   dict(desc=nv12_desc(H, W, pitch=lay["pitch"], uv_offset=lay["uv_offset"], frame_stride=lay["uv_offset"] + lay["pitch"] * (H // 2) - 1)),
                   dict(desc=nv12_desc(H, W, standard=3, **lay))]
    bad_draw = bad_layouts + [
        dict(ctx_h=None), dict(fr=None), dict(det=None), dict(counts=None), dict(style=None), dict(Bn=0), dict(H=0), dict(W=-2), dict(cap=0),
        dict(Bn=1 << 20, cap=1 << 12), dict(style=S(thickness=2)), dict(style=S(thickness=17)), dict(style=S(thickness=0)),
        dict(style=S(text_scale=5)), dict(style=S(text_scale=-1)), dict(style=S(proportion=np.nan)), dict(style=S(proportion=1.5)),
        dict(style=S(proportion=-0.1)), dict(score=None), dict(id_stride=0), dict(off=p(d_off), n_rows=-1), dict(n_rows=-1)]
    for kw in bad_draw:
        assert draw(**kw) == -1 and len(lib.fid_last_error()) > 0, kw
    bad_convert = bad_layouts + [dict(ctx_h=None), dict(src=None), dict(out=None), dict(Bn=0), dict(H=0), dict(W=-2),
                                 dict(src=p(d_fr)), dict(src=C.c_void_p(d_fr.ptr + 8))]                 # in and out overlap
    for kw in bad_convert:
        assert convert(**kw) == -1 and len(lib.fid_last_error()) > 0, kw
    ctx.sync()
    assert np.array_equal(d_fr.download(), buf) and np.array_equal(d_bgr.download(), bgr)
    assert draw(off=p(d_off), n_rows=4, id_stride=0) == 0                  # (the rows form does not read id_stride)
    after = d_fr.download()
    assert (after != buf).any()
    assert convert() == 0
    assert np.array_equal(d_fr.download(), N.bgr_to_nv12(bgr, after.copy(), **lay))


# ---- 6. the pipelines and the runner -----------------------------------------------------------------------------------------

PB, PH, PW, IN = 2, 240, 320, (320, 320)
THRESH = -1.0                 # every face with a positive best cosine is named


class Scene:
    pass


@pytest.fixture(scope="module")
def scene(ctx):
    """SCRFD-500M at 320 x 320 and MobileFaceNet with seeded weights; five random dense NV12 frames of 240 x 320 and their BGR conversion"""
    old = os.environ.get("FID_AUTOTUNE")
    os.environ["FID_AUTOTUNE"] = "0"
    from oracle import align as oalign
    from scrfd_arcface_facerecognition_amd import archs
    from scrfd_arcface_facerecognition_amd.engine import CompiledNet, Gallery
    from scrfd_arcface_facerecognition_amd.pipeline import calibrate_detector_bias
    s = Scene()
    s.nv12 = nv12_oracle.random_batch(31, 5, PH, PW)[0].reshape(5, PH * 3 // 2, PW)
    s.bgr = nv12_oracle.nv12_to_bgr(s.nv12.reshape(-1), 5, PH, PW)
    det_net = archs.scrfd_500m(IN)
    lb = np.stack([oalign.letterbox(f, IN)[0] for f in s.bgr[:4]])
    det_P, _ = calibrate_detector_bias(ctx, det_net, archs.synth_params(det_net, 5), lb, target=30, max_batch=4)
    rec_net = archs.mobilefacenet()
    s.det = CompiledNet(ctx, det_net, det_P, max_batch=PB)
    s.rec = CompiledNet(ctx, rec_net, archs.synth_params(rec_net, 5), max_batch=256)
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


def step_faces(pipe, kind, names, style):
    """the keywords of the oracles for the pipeline's last step, from its downloaded det / counts / identities"""
    det, counts, cap = pipe.post.det.download(), pipe.post.counts.download(), pipe.post.cap
    if kind == "slots":
        kw = dict(idx=pipe.idx.download().reshape(PB, pipe.F), score=pipe.score.download().reshape(PB, pipe.F), id_stride=pipe.F)
    elif kind == "rows":
        kw = dict(idx=pipe.idx.download(), score=pipe.score.download(), offsets=pipe.offsets.download(), n_rows=min(pipe.n_run, pipe.row_cap))
    else:
        kw = dict(idx=pipe.ident_idx.download(), score=pipe.ident_score.download(), id_stride=cap, track=pipe.track.download())
    return dict(det=det, counts=counts, cap=cap, names=names, style=style, **kw), int(np.clip(counts, 0, cap).sum())


def close(pipe, kind):
    if kind == "tracked":
        pipe.close()


@pytest.mark.parametrize("kind", ["slots", "rows", "tracked"])
def test_pipeline_draw_out_nv12(ctx, scene, glyphs, kind):
    from scrfd_arcface_facerecognition_amd._lib import DRAW_TRACK_ID, DrawStyle, Nv12Frames
    s = scene
    flags = DRAW_TRACK_ID if kind == "tracked" else 0
    cstyle, ostyle = DrawStyle(0.3, 5, 1, 1, flags, (0, 0, 255)), O.Style(0.3, 5, 1, 1, flags, (0, 0, 255))
    clean = s.nv12[:PB].reshape(-1)
    # NV12 frames: drawn in place, no BGR buffer
    pipe = make_pipe(ctx, s, kind)
    dev = ctx.to_device(s.nv12[:PB])
    fr = Nv12Frames(dev, PH, PW, standard="bt709")
    pipe.run_step(fr, PH, PW, s.gallery, THRESH)
    with pytest.raises(ValueError):
        pipe.draw(fr, PH, PW, s.gallery, cstyle, out="yuv")
    assert np.array_equal(dev.download().reshape(-1), clean)
    ret = pipe.draw(fr, PH, PW, s.gallery, cstyle, out="nv12")
    assert ret is fr and pipe.bgr is None and pipe.nv12_out is None
    kw, n_faces = step_faces(pipe, kind, s.gallery.names, ostyle)
    got = dev.download().reshape(-1)
    want = N.draw_nv12(clean, PB, PH, PW, glyphs=glyphs, standard="bt709", **kw)
    print(f"\n{kind}: {n_faces} faces, {int((got != clean).sum())} bytes drawn")
    assert n_faces > 0 and (got != clean).any() and np.array_equal(got, want), np.argwhere(got != want)[:6]
    # out=None on NV12 frames: today's behaviour -- the frames stay, the pipeline's BGR buffer is drawn on
    dev.upload(s.nv12[:PB])
    ret = pipe.draw(fr, PH, PW, s.gallery, cstyle)
    assert ret is pipe.bgr and ret.shape == (PB, PH, PW, 3) and np.array_equal(dev.download().reshape(-1), clean)
    bgr_clean = nv12_oracle.nv12_to_bgr(clean, PB, PH, PW, standard="bt709")
    assert np.array_equal(ret.download(), O.draw(bgr_clean, glyphs=glyphs, **kw))
    close(pipe, kind)
    # BGR frames: drawn in place as before, then converted once into the pipeline's dense buffer
    pipe = make_pipe(ctx, s, kind)
    pipe.nv12_standard = "bt601_full"
    bdev = ctx.to_device(s.bgr[:PB])
    pipe.run_step(bdev, PH, PW, s.gallery, THRESH)
    ret = pipe.draw(bdev, PH, PW, s.gallery, cstyle, out="nv12")
    kw, n_faces = step_faces(pipe, kind, s.gallery.names, ostyle)
    drawn = O.draw(s.bgr[:PB], glyphs=glyphs, **kw)
    assert n_faces > 0 and isinstance(ret, Nv12Frames) and ret is pipe.nv12_out and pipe.bgr is None
    assert np.array_equal(bdev.download(), drawn)
    assert np.array_equal(ret.buf.download().reshape(-1), N.bgr_to_nv12(drawn, np.zeros(clean.size, np.uint8), "bt601_full"))
    bdev.upload(s.bgr[:PB])
    assert pipe.draw(bdev, PH, PW, s.gallery, cstyle) is bdev and np.array_equal(bdev.download(), drawn)      # out=None: as before
    close(pipe, kind)


def same_faces(ra, rb):
    assert len(ra) == len(rb)
    for fa, fb in zip(ra, rb):
        assert np.array_equal(fa[0], fb[0]) and fa[1] == fb[1] and np.array_equal(fa[2], fb[2]) and fa[3:] == fb[3:]


@pytest.mark.parametrize("fmt", ["nv12", "bgr"])
@pytest.mark.parametrize("kind", ["slots", "rows", "tracked"])
def test_runner_annotates_as_nv12(ctx, scene, glyphs, kind, fmt):
    """five frames at B = 2: the last batch is padded"""
    from scrfd_arcface_facerecognition_amd.video import StreamRunner
    s = scene
    items = s.nv12 if fmt == "nv12" else s.bgr
    pipe = make_pipe(ctx, s, kind)
    runner = StreamRunner(pipe, s.gallery, (PH, PW), similarity_thresh=THRESH, annotate=True, pixel_format=fmt, standard="bt709",
                          annotate_format="nv12")
    assert runner.download_bytes == PB * PH * PW * 3 // 2 and runner.upload_bytes == PB * PH * PW * (3 if fmt == "bgr" else 1.5)
    faces_a, want = [], None
    for i, (faces, frame) in enumerate(runner.run(iter(items))):
        if i % PB == 0:                                                    # the step of this batch has run, the next one has not
            n = min(PB, 5 - i)
            kw, _ = step_faces(pipe, kind, s.gallery.names, O.Style())
            if fmt == "nv12":
                pad = np.zeros((PB - n, PH * 3 // 2, PW), np.uint8)
                pad[:, PH:] = 128
                want = N.draw_nv12(np.concatenate([s.nv12[i:i + n], pad]).reshape(-1), PB, PH, PW, glyphs=glyphs, standard="bt709", **kw)
            else:
                batch = np.concatenate([s.bgr[i:i + n], np.zeros((PB - n, PH, PW, 3), np.uint8)])
                want = N.bgr_to_nv12(O.draw(batch, glyphs=glyphs, **kw), np.zeros(PB * PH * PW * 3 // 2, np.uint8), "bt709")
            want = want.reshape(PB, PH * 3 // 2, PW)
        assert frame.shape == (PH * 3 // 2, PW) and frame.dtype == np.uint8 and np.array_equal(frame, want[i % PB]), i
        faces_a.append(faces)
    runner.close()
    assert pipe.bgr is None
    close(pipe, kind)
    pipe = make_pipe(ctx, s, kind)
    runner = StreamRunner(pipe, s.gallery, (PH, PW), similarity_thresh=THRESH, pixel_format=fmt, standard="bt709")
    assert runner.download_bytes == 0
    faces_b = list(runner.run(iter(items)))
    runner.close()
    close(pipe, kind)
    assert len(faces_a) == len(faces_b) == 5 and sum(len(r) for r in faces_b) > 0
    for ra, rb in zip(faces_a, faces_b):
        same_faces(ra, rb)


def test_runner_constructor(ctx, scene):
    from scrfd_arcface_facerecognition_amd.video import StreamRunner
    pipe = make_pipe(ctx, scene, "slots")
    for hw in ((PH + 1, PW), (PH, PW - 1)):
        with pytest.raises(ValueError):
            StreamRunner(pipe, scene.gallery, hw, annotate=True, annotate_format="nv12")
    with pytest.raises(ValueError):
        StreamRunner(pipe, scene.gallery, (PH, PW), annotate=True, annotate_format="i420")
    r = StreamRunner(pipe, scene.gallery, (PH + 1, PW - 1), annotate=True)             # BGR in, BGR out: any size, as before
    assert r.download_bytes == PB * (PH + 1) * (PW - 1) * 3
    r.close()


def test_grouped_pipeline_still_refuses(ctx, scene):
    from scrfd_arcface_facerecognition_amd.pipeline import GroupedFacePipeline
    pipe = GroupedFacePipeline(ctx, scene.det, scene.rec, batch=PB, faces_per_frame=2, group=2)
    with pytest.raises(ValueError):
        pipe.draw(None, PH, PW, scene.gallery, out="nv12")
