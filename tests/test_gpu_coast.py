"""GPU: fid_track_coast (csrc/coast.hip) against its host twin fid_track_coast_host, byte for byte -- the state through fid_coaster_read and
all five outputs, fillers and guard words included --, behind a real fid_track_step + fid_track_identify; the extended tables driving the
existing redact and draw kernels; the refused calls; and TrackedFacePipeline(coast=...) with and without a missed frame."""
import ctypes as C
import os

import numpy as np
import pytest

import coast_oracle as CO
import draw_oracle as O
import redact_oracle as R
from coast_calls import TRACK_CFG, host, same
from track_oracle import draw_rows, random_walk

pytestmark = pytest.mark.gpu
GUARD = 0x5A5A5A5A
NG = 4                        # guard words behind every output
INVALID = -1
BOTH = R.UNKNOWN | R.KNOWN


@pytest.fixture(scope="module")
def ctx():
    from scrfd_arcface_facerecognition_amd._lib import default_context
    return default_context(0)


@pytest.fixture(scope="module")
def glyphs(ctx):
    out = np.zeros(95 * 7, np.uint8)
    assert ctx.lib.fid_draw_glyphs(out.ctypes.data_as(C.c_void_p)) == 0
    return out.reshape(95, 7)


def _i32(a):
    from scrfd_arcface_facerecognition_amd._lib import c_i32_p
    return a.ctypes.data_as(c_i32_p)


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


class Device:
    """a fid_tracker and a fid_coaster of one shape and the buffers of one step; every coaster output carries NG guard words"""

    def __init__(self, ctx, S, T):
        from scrfd_arcface_facerecognition_amd._lib import TrackConfig, check
        self.ctx, self.S, self.T, self.check = ctx, S, T, check
        self.tcfg = TrackConfig(*TRACK_CFG)
        self.trk, self.coaster = C.c_void_p(), C.c_void_p()
        check(ctx.lib.fid_tracker_create(ctx.handle, S, T, C.byref(self.trk)))
        check(ctx.lib.fid_coaster_create(ctx.handle, S, T, C.byref(self.coaster)))

    def step(self, det, counts, stream):
        """fid_track_step on the device -> nothing; the tables stay on the device"""
        B, cap = det.shape[:2]
        self.B, self.cap, self.row_cap = B, cap, B * cap
        self.stream = np.ascontiguousarray(stream, np.int32)
        self.h_det, self.h_counts = np.ascontiguousarray(det, np.float32), np.ascontiguousarray(counts, np.int32)
        self.det, self.counts = self.ctx.to_device(self.h_det), self.ctx.to_device(self.h_counts)
        self.track, self.offsets, self.src = (self.ctx.empty((B, cap, 2), np.int32), self.ctx.empty((B + 1,), np.int32),
                                              self.ctx.empty((self.row_cap,), np.int32))
        self.check(self.ctx.lib.fid_track_step(self.ctx.handle, self.trk, C.c_void_p(self.det.ptr), C.c_void_p(self.counts.ptr), _i32(self.stream),
                                               B, cap, C.byref(self.tcfg), C.c_void_p(self.track.ptr), C.c_void_p(self.offsets.ptr),
                                               C.c_void_p(self.src.ptr), self.row_cap))

    def identify(self, idx, score):
        """fid_track_identify with rows as fid_match could have written them -> the step's host tables (stream, det, counts, track, ii, sc)"""
        B, cap = self.B, self.cap
        n = min(int(self.offsets.download()[B]), self.row_cap)
        di, ds = self.ctx.to_device(np.asarray(idx, np.int32)), self.ctx.to_device(np.asarray(score, np.float32))
        self.ii, self.sc = self.ctx.empty((B, cap), np.int32), self.ctx.empty((B, cap), np.float32)
        self.check(self.ctx.lib.fid_track_identify(self.ctx.handle, self.trk, C.c_void_p(self.counts.ptr), _i32(self.stream), B, cap,
                                                   C.c_void_p(self.track.ptr), C.c_void_p(self.offsets.ptr), C.c_void_p(self.src.ptr),
                                                   self.row_cap, C.c_void_p(di.ptr), C.c_void_p(ds.ptr), n, C.c_void_p(self.ii.ptr),
                                                   C.c_void_p(self.sc.ptr)))
        return self.stream, self.h_det, self.h_counts, self.track.download(), self.ii.download(), self.sc.download()

    def new_outputs(self):
        B, cap2 = self.B, self.cap + self.T
        self.sizes = [B * cap2 * 5, B, B * cap2 * 2, B * cap2, B * cap2]
        self.shapes = [(B, cap2, 5), (B,), (B, cap2, 2), (B, cap2), (B, cap2)]
        self.outs = [self.ctx.to_device(np.full(n + NG, GUARD, np.int32)) for n in self.sizes]

    def coast(self, cfg, ident=True, expect=0, fresh=True, **override):
        """fid_track_coast -> the five outputs as the host sees them (guards checked)"""
        if fresh:
            self.new_outputs()
        a = dict(stream=self.stream, B=self.B, cap=self.cap, det=C.c_void_p(self.det.ptr), cfg=C.byref(cfg) if cfg is not None else None)
        a.update(override)
        rc = self.ctx.lib.fid_track_coast(self.ctx.handle, self.coaster, self.trk, _i32(a["stream"]), a["B"], a["cap"], a["det"],
                                          C.c_void_p(self.counts.ptr), C.c_void_p(self.track.ptr), C.c_void_p(self.ii.ptr) if ident else None,
                                          C.c_void_p(self.sc.ptr) if ident else None, a["cfg"], *[C.c_void_p(o.ptr) for o in self.outs])
        assert rc == expect, (rc, expect)
        return self.read_outputs()

    def read_outputs(self):
        dts = (np.float32, np.int32, np.int32, np.int32, np.float32)
        got = []
        for o, n, shape, dt in zip(self.outs, self.sizes, self.shapes, dts):
            raw = o.download()
            assert (raw[n:] == GUARD).all(), "guard words behind an output were written"
            got.append(raw[:n].view(dt).reshape(shape))
        return got

    def state(self):
        e = np.empty((self.S, self.T, CO.WORDS), np.int32)
        self.check(self.ctx.lib.fid_coaster_read(self.ctx.handle, self.coaster, _i32(e)))
        return e

    def close(self):
        self.check(self.ctx.lib.fid_coaster_destroy(self.ctx.handle, self.coaster))
        self.check(self.ctx.lib.fid_tracker_destroy(self.ctx.handle, self.trk))


def ccfg(hold=4, predict=True, grow=0.05):
    from scrfd_arcface_facerecognition_amd._lib import CoastConfig
    return CoastConfig(hold, predict, grow)


def grid_det(B, cap, n, present):
    """n boxes on a grid, moving one pixel per frame, in the frames where present[b]; sub-pixel offsets make the arithmetic inexact"""
    det, counts = np.zeros((B, cap, 5), np.float32), np.zeros(B, np.int32)
    for b in range(B):
        if not present[b]:
            continue
        for i in range(n):
            x, y = 40.0 * (i % 10) + b + 0.3 * i, 40.0 * (i // 10) + 0.5 * b
            det[b, i] = (x, y, x + 20.25, y + 22.5, 1.0 - 0.01 * i)
        counts[b] = n
    return det, counts


def walk_inputs(seed, cap, B, S=3):
    """two steps of (det, counts, stream): a thinned random walk with sub-pixel jitter and a skipped frame"""
    rng = np.random.default_rng(700 + seed)
    n_rect, p = (3, 0.3) if cap < 64 else (80, 0.04)
    out = []
    for det, counts, stream in CO.thin(random_walk(seed, calls=2, B=B, cap=cap, S=S, n_rect=n_rect), seed, p=p):
        for b in range(B):
            det[b, :counts[b], :4] += rng.random((int(counts[b]), 4), dtype=np.float32) * np.float32(0.75)
        stream = stream.copy()
        stream[3::7] = -1
        out.append((det, counts, stream))
    return out


def run_against_the_twin(ctx, S, T, inputs, cfg, ident=True, seed=0):
    """every step on the device and through the host twin on the device tracker's own tables -> coasted rows per step"""
    rng = np.random.default_rng(seed)
    dev = Device(ctx, S, T)
    entries = CO.fresh(S, T)
    assert np.array_equal(dev.state(), entries)
    coasted = []
    for det, counts, stream in inputs:
        dev.step(det, counts, stream)
        tabs = dev.identify(*draw_rows(rng, dev.row_cap))
        got = dev.coast(cfg, ident)
        rc, want = host(entries, *(tabs if ident else tabs[:4] + (None, None)), cfg)
        assert rc == 0 and not same(got, want), same(got, want)
        assert np.array_equal(dev.state(), entries), np.argwhere(dev.state() != entries)[:6]
        coasted.append(CO.coasted(want, T))
    dev.close()
    return coasted


# ---- 1. the device against the host twin ----
@pytest.mark.parametrize("T, cap, B", [(64, 3, 9), (1, 3, 9), (5, 70, 9), (64, 70, 9)])
def test_walks_equal_the_host_twin(ctx, T, cap, B):
    """B = 9 frames over S = 3 interleaved streams with a skipped frame, two consecutive steps; cap = 70: two loads of 64, the second ragged"""
    inputs = walk_inputs(1, cap, B)
    assert all((s < 0).any() and len(set(s[s >= 0])) == 3 for _, _, s in inputs)
    if cap == 70:
        assert max(int(c.max()) for _, c, _ in inputs) > 64
    total = 0
    for hold, predict, grow, ident in ((4, True, 0.05, True), (1, False, 0.5, True), (4, True, 0.0, False), (0, True, 0.05, True)):
        coasted = run_against_the_twin(ctx, 3, T, inputs, ccfg(hold, predict, grow), ident, seed=T)
        n = sum(len(rows) for step in coasted for rows in step)
        assert (n == 0) == (hold == 0), (hold, n)
        total += n
    assert total >= 6


def test_all_64_lanes_coast_in_one_frame(ctx):
    """T = 64: every slot holds a track, a frame without a detection makes all of them coast, the next one matches all of them again"""
    B, cap = 6, 70
    det, counts = grid_det(B, cap, 64, [1, 1, 0, 0, 1, 0])
    coasted = run_against_the_twin(ctx, 1, 64, [(det, counts, np.zeros(B, np.int32))], ccfg(3, True, 0.05))[0]
    assert [len(r) for r in coasted] == [0, 0, 64, 64, 0, 64]
    assert [r[3] for r in coasted[3]] == [2] * 64 and [r[2] for r in coasted[5]] == list(range(64))


def test_reset_frees_one_stream_or_all(ctx):
    B, cap = 4, 4
    det, counts = grid_det(B, cap, 3, [1, 1, 1, 1])
    dev = Device(ctx, 2, 5)
    dev.step(det, counts, np.array([0, 1, 0, 1], np.int32))
    dev.identify(*draw_rows(np.random.default_rng(0), dev.row_cap))
    dev.coast(ccfg())
    e = dev.state()
    assert (e[:, :3, 0] >= 0).all()
    dev.check(ctx.lib.fid_coaster_reset(ctx.handle, dev.coaster, 1))
    after = dev.state()
    assert np.array_equal(after[0], e[0]) and np.array_equal(after[1], CO.fresh(1, 5)[0])
    assert ctx.lib.fid_coaster_reset(ctx.handle, dev.coaster, 2) == INVALID
    dev.check(ctx.lib.fid_coaster_reset(ctx.handle, dev.coaster, -1))
    assert np.array_equal(dev.state(), CO.fresh(2, 5))
    dev.close()


# ---- 2. the extended tables drive the existing kernels ----
H, W = 48, 80
KNOWN_NAMES = [b"ann", b"bob"]


def small_scene(ctx):
    """one stream, T = 4, cap = 3, four frames of 48 x 80: two faces; the second is dropped in frame 2, both in frame 3.  Track 0 is named."""
    a, b = np.array([5, 6, 30, 40], np.float32), np.array([44, 8, 70, 41], np.float32)
    det, counts = np.zeros((4, 3, 5), np.float32), np.array([2, 2, 1, 0], np.int32)
    for t in range(4):
        det[t, 0, :4], det[t, 0, 4] = a + np.float32(1.25 * t), 0.9
        det[t, 1, :4], det[t, 1, 4] = b + np.float32(0.75 * t), 0.8
    det[2, 1] = det[3, :2] = 0
    dev = Device(ctx, 1, 4)
    dev.step(det, counts, np.zeros(4, np.int32))
    idx, score = np.full(dev.row_cap, -1, np.int32), np.zeros(dev.row_cap, np.float32)
    idx[0], score[0] = 1, 0.625                                # the first row is track 0's first face: "bob"
    tabs = dev.identify(idx, score)
    return dev, tabs


def test_extended_tables_through_redact_and_draw(ctx, glyphs):
    from scrfd_arcface_facerecognition_amd._lib import DRAW_TRACK_ID, DrawStyle, check
    from scrfd_arcface_facerecognition_amd.engine import LabelTable
    from redact_calls import c_style
    dev, tabs = small_scene(ctx)
    cfg = ccfg(4, True, 0.05)
    got = dev.coast(cfg)
    want = CO.coast(CO.fresh(1, 4), *tabs, CO.Config(4, True, 0.05))
    assert not same(got, want), same(got, want)
    det_out, counts_out, track_out, idx_out, score_out = want
    assert list(counts_out) == [2, 2, 2, 2] and [len(r) for r in CO.coasted(want, 4)] == [0, 0, 1, 2]
    assert idx_out[3, 0] == 1 and idx_out[3, 1] == -1                       # the held boxes keep their tracks' identities
    cap2 = 3 + 4
    frames = np.random.default_rng(H * W).integers(0, 256, (4, H, W, 3), dtype=np.uint8)
    tables = [C.c_void_p(o.ptr) for o in dev.outs]                          # (det, counts, track, idx, score) where the coaster wrote them
    held = [tuple(int(v) for v in det_out[3, i, :4]) for i in range(2)]
    for style in (R.Style(mode=R.FILL, who=BOTH, fill_bgr=(9, 200, 77)), R.Style(mode=R.FILL, who=R.UNKNOWN, fill_bgr=(1, 2, 3)),
                  R.Style(who=BOTH, cells=4, expand=0.1)):
        buf = ctx.to_device(frames)
        check(ctx.lib.fid_redact_faces(ctx.handle, C.c_void_p(buf.ptr), 4, H, W, tables[0], tables[1], cap2, tables[3], tables[4], cap2, None, 0,
                                       C.byref(c_style(style))))
        out = buf.download()
        ref = R.redact(frames, det_out, counts_out, cap2, idx=idx_out, score=score_out, id_stride=cap2, style=style)
        assert np.array_equal(out, ref), np.argwhere(out != ref)[:6]
        # frame 3 has no detection at all: what changed there changed inside a held box
        changed = np.argwhere((out[3] != frames[3]).any(axis=2))
        assert len(changed) > 100
        x1, y1, x2, y2 = held[1]                                             # the stranger's: redacted under every style
        assert (out[3, y1 + 2:y2 - 1, x1 + 2:x2 - 1] != frames[3, y1 + 2:y2 - 1, x1 + 2:x2 - 1]).any()
        if style.who == R.UNKNOWN:                                           # the named track coasts in the clear
            x1, y1, x2, y2 = held[0]
            assert np.array_equal(out[3, y1:y2, x1:x1 + 10], frames[3, y1:y2, x1:x1 + 10])
    dstyle, ostyle = DrawStyle(0.3, 3, 1, 1, DRAW_TRACK_ID, (0, 0, 255)), O.Style(0.3, 3, 1, 1, DRAW_TRACK_ID, (0, 0, 255))
    labels = LabelTable(ctx, KNOWN_NAMES, None)
    buf = ctx.to_device(frames)
    check(ctx.lib.fid_draw_faces(ctx.handle, C.c_void_p(buf.ptr), 4, H, W, tables[0], tables[1], cap2, tables[3], tables[4], cap2, None, 0,
                                 tables[2], labels.handle, C.byref(dstyle)))
    out = buf.download()
    ref = O.draw(frames, det_out, counts_out, cap2, glyphs, idx=idx_out, score=score_out, id_stride=cap2, track=track_out, names=KNOWN_NAMES,
                 style=ostyle)
    assert np.array_equal(out, ref) and (out[3] != frames[3]).any()
    labels.close()
    dev.read_outputs()                                                        # (the consumers wrote nothing into the tables or their guards)
    dev.close()


# ---- 3. refusals ----
def test_refusals_leave_outputs_and_state_untouched(ctx):
    B, cap = 4, 4
    det, counts = grid_det(B, cap, 3, [1, 0, 1, 0])
    stream = np.zeros(B, np.int32)
    dev = Device(ctx, 1, 5)
    dev.step(det, counts, stream)
    dev.ii, dev.sc = ctx.empty((B, cap), np.int32), ctx.empty((B, cap), np.float32)
    dev.new_outputs()
    fresh = CO.fresh(1, 5)

    def untouched(state):
        assert all((bits(o.download()) == GUARD).all() for o in dev.outs)
        assert np.array_equal(dev.state(), state)

    dev.coast(ccfg(), expect=INVALID, fresh=False)                            # the step still waits for its identify
    untouched(fresh)
    tabs = dev.identify(*draw_rows(np.random.default_rng(3), dev.row_cap))
    for what, kw in (("another B", dict(B=B - 1)), ("another cap", dict(cap=cap + 1)), ("another stream array", dict(stream=np.array([0, 0, -1, 0], np.int32))),
                     ("a NULL det", dict(det=None))):
        dev.coast(ccfg(), expect=INVALID, fresh=False, **kw)
        untouched(fresh)
    dev.coast(None, expect=INVALID, fresh=False)                              # a NULL config
    untouched(fresh)
    for hold, grow, reserved in ((-1, 0.05, 0), (1024, 0.05, 0), (4, -0.01, 0), (4, 0.51, 0), (4, float("nan"), 0), (4, 0.05, 1)):
        bad = ccfg(hold, True, grow)
        bad.reserved = reserved
        dev.coast(bad, expect=INVALID, fresh=False)
        untouched(fresh)
    other = Device(ctx, 1, 6)                                                 # a coaster of another shape than the tracker
    rc = ctx.lib.fid_track_coast(ctx.handle, other.coaster, dev.trk, _i32(stream), B, cap, C.c_void_p(dev.det.ptr), C.c_void_p(dev.counts.ptr),
                                 C.c_void_p(dev.track.ptr), None, None, C.byref(ccfg()), *[C.c_void_p(o.ptr) for o in dev.outs])
    assert rc == INVALID
    untouched(fresh)
    other.close()
    got = dev.coast(ccfg(), fresh=False)                                      # the valid call goes through ...
    entries = CO.fresh(1, 5)
    rc, want = host(entries, *tabs, ccfg())
    assert rc == 0 and not same(got, want) and np.array_equal(dev.state(), entries)
    dev.new_outputs()
    dev.coast(ccfg(), expect=INVALID, fresh=False)                            # ... once per step
    untouched(entries)
    dev.close()


# ---- 4., 5. the pipeline ----
PH = PW = 320
PB = 4
THRESH = -1.0                 # every face with a positive best cosine is named: tracks become `known`


def smooth_image(rng, h, w, cell=24):
    """a low-pass random image (bilinear interpolation of a coarse random grid): a shift by a few pixels changes it little"""
    gh, gw = h // cell + 2, w // cell + 2
    grid = rng.integers(0, 256, (gh, gw, 3)).astype(np.float64)
    ys, xs = np.arange(h) / cell, np.arange(w) / cell
    y0, x0 = ys.astype(int), xs.astype(int)
    fy, fx = (ys - y0)[:, None, None], (xs - x0)[None, :, None]
    top = grid[y0][:, x0] * (1 - fx) + grid[y0][:, x0 + 1] * fx
    bot = grid[y0 + 1][:, x0] * (1 - fx) + grid[y0 + 1][:, x0 + 1] * fx
    return np.clip(np.rint(top * (1 - fy) + bot * fy), 0, 255).astype(np.uint8)


class Scene:
    pass


@pytest.fixture(scope="module")
def scene(ctx):
    """SCRFD-500M at 320x320 and MobileFaceNet with seeded weights; frames that are the previous one shifted by 2 pixels, and a flat frame"""
    old = os.environ.get("FID_AUTOTUNE")
    os.environ["FID_AUTOTUNE"] = "0"
    from scrfd_arcface_facerecognition_amd.engine import CompiledNet, Gallery, resolve_model
    from scrfd_arcface_facerecognition_amd.pipeline import calibrate_detector_bias
    s = Scene()
    rng = np.random.default_rng(41)
    wide = smooth_image(rng, PH, PW + 2 * 12)
    s.frames = np.stack([wide[:, 2 * t:2 * t + PW] for t in range(PB)])
    s.blank = np.full((PH, PW, 3), 85, np.uint8)                   # (at this calibration the detector finds nothing in it, nor at 68 or 102)
    det_net, det_P0 = resolve_model("synthetic:scrfd_500m?seed=5", (PH, PW))
    det_P, _ = calibrate_detector_bias(ctx, det_net, det_P0, s.frames, target=10, max_batch=4)
    rec_net, rec_P = resolve_model("synthetic:arcface_mbf?seed=5")
    s.det = CompiledNet(ctx, det_net, det_P, max_batch=PB)
    s.rec = CompiledNet(ctx, rec_net, rec_P, max_batch=256)
    s.gallery = Gallery(ctx, np.random.default_rng(77).standard_normal((37, 512)).astype(np.float32))
    yield s
    if old is None:
        del os.environ["FID_AUTOTUNE"]
    else:
        os.environ["FID_AUTOTUNE"] = old


def make_pipe(ctx, s, coast):
    from scrfd_arcface_facerecognition_amd.pipeline import TrackedFacePipeline
    return TrackedFacePipeline(ctx, s.det, s.rec, batch=PB, row_cap=256, refresh=1000, retry=1, max_tracks=64, coast=coast)


def step_tables(pipe):
    return (np.zeros(PB, np.int32), pipe.post.det.download(), pipe.post.counts.download(), pipe.track.download(), pipe.ident_idx.download(),
            pipe.ident_score.download())


def pipe_tables(pipe):
    return [pipe.coast_det.download(), pipe.coast_counts.download(), pipe.coast_track.download(), pipe.coast_idx.download(),
            pipe.coast_score.download()]


def test_pipeline_changes_nothing_when_nothing_coasts(ctx, scene, glyphs):
    """the same frame four times: every track is matched in every frame, so the extended tables hold the detections and nothing else"""
    from scrfd_arcface_facerecognition_amd._lib import CoastConfig, DrawStyle, RedactStyle
    from scrfd_arcface_facerecognition_amd.pipeline import TrackedFacePipeline
    s = scene
    frames = np.stack([s.frames[0]] * PB)
    with pytest.raises(ValueError):
        TrackedFacePipeline(ctx, s.det, s.rec, batch=PB, row_cap=256, max_age=3, coast=CoastConfig(hold=4))
    with pytest.raises(TypeError):
        make_pipe(ctx, s, coast=True)
    on, off = make_pipe(ctx, s, CoastConfig()), make_pipe(ctx, s, None)
    assert off.coaster is None and not hasattr(off, "coast_det")
    with pytest.raises(RuntimeError):
        off.results_coasted()
    outs = []
    for pipe in (on, off):
        fr = ctx.to_device(frames)
        pipe.run_step(fr, PH, PW, s.gallery, THRESH)
        drawn = pipe.draw(fr, PH, PW, s.gallery, DrawStyle(0.3, 3, 1, 1, 1, (0, 0, 255)), redact=RedactStyle(who=BOTH, cells=6)).download()
        fr2 = ctx.to_device(frames)
        red = pipe.redact(fr2, PH, PW, RedactStyle(mode=R.FILL, who=BOTH, fill_bgr=(10, 200, 30))).download()
        outs.append((drawn, red, pipe.results_tracked(s.gallery)))
    counts = off.post.counts.download()
    assert counts.min() > 0 and np.array_equal(on.coast_counts.download(), np.clip(counts, 0, off.post.cap))      # every c_b = 0
    assert all(len(r) == 0 for r in on.results_coasted(s.gallery))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    assert (outs[0][0] != frames).any() and (outs[0][1] != frames).any()
    assert repr(outs[0][2]) == repr(outs[1][2])
    on.close()
    off.close()


def test_pipeline_holds_the_redaction_through_a_missed_frame(ctx, scene):
    """frame 2 of the batch shows no face: with the coaster every live track is held there -- listed, named and painted --, without it the
    frame leaves untouched: the failure the feature removes"""
    from scrfd_arcface_facerecognition_amd._lib import CoastConfig, RedactStyle
    s = scene
    frames = s.frames.copy()
    frames[2] = s.blank
    fill = RedactStyle(mode=R.FILL, who=BOTH, fill_bgr=(10, 200, 30))
    ofill = R.Style(mode=R.FILL, who=BOTH, fill_bgr=(10, 200, 30))
    on, off = make_pipe(ctx, s, CoastConfig(hold=4, predict=True, grow=0.05)), make_pipe(ctx, s, None)
    red = {}
    for name, pipe in (("on", on), ("off", off)):
        fr = ctx.to_device(frames)
        pipe.run_step(fr, PH, PW, s.gallery, THRESH)
        red[name] = pipe.redact(fr, PH, PW, fill).download()
    tabs = step_tables(on)
    stream, det, counts, track, ii, sc = tabs
    assert counts[2] == 0 and counts[1] > 0 and counts[3] > 0, counts
    assert repr(on.results_tracked(s.gallery)) == repr(off.results_tracked(s.gallery))
    # the coaster's tables are the oracle's, and its state too
    entries = CO.fresh(1, 64)
    want = CO.coast(entries, *tabs, CO.Config(4, True, 0.05))
    assert not same(pipe_tables(on), want), same(pipe_tables(on), want)
    assert np.array_equal(on.coaster_state(), entries)
    # every live track coasts in frame 2: the ones matched in frame 1 with missed = 1, under their track's name
    cap = on.post.cap
    alive = {int(track[b, f, 0]) for b in (0, 1) for f in range(min(int(counts[b]), cap)) if track[b, f, 1] >= 0}
    last = {int(track[1, f, 0]): f for f in range(min(int(counts[1]), cap)) if track[1, f, 1] >= 0}
    listed = on.results_coasted(s.gallery)
    assert {row[4] for row in listed[2]} == alive and len(last) > 0
    by_id = {row[4]: row for row in listed[2]}
    for tid, f in last.items():
        bbox, conf, name, sim, _, missed = by_id[tid]
        assert missed == 1 and conf == float(det[1, f, 4]) and sim == float(sc[1, f])
        assert name == (s.gallery.names[ii[1, f]] if ii[1, f] >= 0 else "Unknown")
    assert any(row[2] != "Unknown" for row in listed[2])
    assert [len(r) for r in listed] == [len(r) for r in CO.coasted(want, 64)]
    # FILL paints the held boxes in the frame without a detection; without the coaster that frame is shown as it is
    ref = R.redact(frames, want[0], want[1], cap + 64, idx=want[3], score=want[4], id_stride=cap + 64, style=ofill)
    assert np.array_equal(red["on"], ref)
    assert (red["on"][2] != frames[2]).any() and np.array_equal(red["off"][2], frames[2])
    assert np.array_equal(red["off"], R.redact(frames, det, counts, cap, idx=ii, score=sc, id_stride=cap, style=ofill))
    # a step that was identified by hand has not been coasted: the extended tables would be the previous step's
    fr = ctx.to_device(frames)
    on.detect(fr, PH, PW)
    on.embed(fr, PH, PW)
    on.identify(0)
    with pytest.raises(RuntimeError):
        on.redact(fr, PH, PW, fill)
    with pytest.raises(RuntimeError):
        on.results_coasted(s.gallery)
    on.reset()
    assert np.array_equal(on.coaster_state(), CO.fresh(1, 64))
    on.close()
    off.close()
