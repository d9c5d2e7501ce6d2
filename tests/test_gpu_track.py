"""GPU: the face tracker (fid_tracker_*, fid_track_step, fid_track_identify; pipeline.TrackedFacePipeline; video.StreamRunner with a tracked pipe).
The yardstick is tests/track_oracle.py; every comparison is bit for bit, state included (floats as int32 views).  The tracker cases upload
synthetic det / counts arrays directly: no network runs in them."""
import ctypes as C
import os

import numpy as np
import pytest

from track_oracle import EMBED, STARTED, Tracker, draw_rows, random_walk

pytestmark = pytest.mark.gpu

GUARD = 0x5A5A5A5A
NG = 4                        # guard words behind every output


@pytest.fixture(scope="module")
def ctx():
    from scrfd_arcface_facerecognition_amd._lib import default_context
    return default_context(0)


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def _i32(a):
    from scrfd_arcface_facerecognition_amd._lib import c_i32_p
    return a.ctypes.data_as(c_i32_p)


def config(iou=0.3, max_age=1, refresh=3, retry=2):
    from scrfd_arcface_facerecognition_amd._lib import TrackConfig
    return TrackConfig(float(iou), int(max_age), int(refresh), int(retry))


class GpuTracker:
    """a fid_tracker and the buffers of one step; every output carries NG guard words, checked after every call"""

    def __init__(self, ctx, S, T):
        from scrfd_arcface_facerecognition_amd._lib import check
        self.ctx, self.S, self.T, self.check = ctx, S, T, check
        self.h = C.c_void_p()
        check(ctx.lib.fid_tracker_create(ctx.handle, S, T, C.byref(self.h)))

    def _out(self, n, dtype=np.int32):
        return self.ctx.to_device(np.full(n + NG, GUARD, np.int32).view(dtype))

    @staticmethod
    def _take(buf, n):
        raw = buf.download()
        assert (bits(raw[n:]) == GUARD).all(), "guard words behind an output were written"
        return raw[:n]

    def step(self, det, counts, stream, cfg, row_cap):
        B, cap = det.shape[:2]
        self.B, self.cap, self.row_cap = B, cap, row_cap
        self.stream = np.ascontiguousarray(stream, np.int32)
        self.det, self.counts = self.ctx.to_device(det.astype(np.float32)), self.ctx.to_device(counts.astype(np.int32))
        self.track, self.offsets, self.src = self._out(B * cap * 2), self._out(B + 1), self._out(row_cap)
        self.check(self.ctx.lib.fid_track_step(self.ctx.handle, self.h, C.c_void_p(self.det.ptr), C.c_void_p(self.counts.ptr), _i32(self.stream),
                                               B, cap, C.byref(cfg), C.c_void_p(self.track.ptr), C.c_void_p(self.offsets.ptr),
                                               C.c_void_p(self.src.ptr), row_cap))
        return self._take(self.track, B * cap * 2).reshape(B, cap, 2), self._take(self.offsets, B + 1), self._take(self.src, row_cap)

    def identify(self, idx, score, n_rows):
        B, cap = self.B, self.cap
        di = self.ctx.to_device(np.asarray(idx, np.int32)) if idx is not None else None
        ds = self.ctx.to_device(np.asarray(score, np.float32)) if score is not None else None
        oi, os_ = self._out(B * cap), self._out(B * cap, np.float32)
        self.check(self.ctx.lib.fid_track_identify(self.ctx.handle, self.h, C.c_void_p(self.counts.ptr), _i32(self.stream), B, cap,
                                                   C.c_void_p(self.track.ptr), C.c_void_p(self.offsets.ptr), C.c_void_p(self.src.ptr),
                                                   self.row_cap, C.c_void_p(di.ptr) if di else None, C.c_void_p(ds.ptr) if ds else None,
                                                   n_rows, C.c_void_p(oi.ptr), C.c_void_p(os_.ptr)))
        return self._take(oi, B * cap).reshape(B, cap), self._take(os_, B * cap).reshape(B, cap)

    def state(self):
        slots, streams = np.empty((self.S, self.T, 10), np.int32), np.empty((self.S, 2), np.int32)
        self.check(self.ctx.lib.fid_tracker_read(self.ctx.handle, self.h, _i32(slots), _i32(streams)))
        return slots, streams

    def reset(self, stream=-1):
        self.check(self.ctx.lib.fid_tracker_reset(self.ctx.handle, self.h, stream))

    def close(self):
        self.check(self.ctx.lib.fid_tracker_destroy(self.ctx.handle, self.h))


class Both:
    """the device tracker and the oracle, driven together; every call asserts bit equality of every output and of the state"""

    def __init__(self, ctx, S, T):
        self.gpu, self.ref = GpuTracker(ctx, S, T), Tracker(S, T)
        self.check_state()

    def check_state(self):
        (gs, gt), (rs, rt) = self.gpu.state(), self.ref.state()
        assert same(gt, rt), (gt, rt)
        assert same(gs, rs), np.argwhere(gs != rs)[:8]

    def step(self, det, counts, stream, cfg, row_cap):
        got = self.gpu.step(det, counts, stream, cfg, row_cap)
        want = self.ref.step(det, counts, stream, cfg.iou_thresh, cfg.max_age, cfg.refresh, cfg.retry, row_cap)
        for g, w, name in zip(got, want, ("track", "offsets", "src")):
            assert same(g, w), (name, g.reshape(-1)[:64], w.reshape(-1)[:64])
        return want

    def identify(self, idx, score, n_rows):
        got = self.gpu.identify(idx, score, n_rows)
        want = self.ref.identify(idx, score, n_rows)
        assert same(got[0], want[0]) and same(got[1], want[1]), (got, want)
        self.check_state()
        return want

    def close(self):
        self.gpu.close()


def frames_of(boxes_per_frame, cap):
    """[[box, ...], ...] -> det [B,cap,5], counts [B]"""
    B = len(boxes_per_frame)
    det, counts = np.zeros((B, cap, 5), np.float32), np.zeros(B, np.int32)
    for b, boxes in enumerate(boxes_per_frame):
        for f, box in enumerate(boxes):
            det[b, f, :4] = box
            det[b, f, 4] = 0.9
        counts[b] = len(boxes)
    return det, counts


def grid_box(i, size=20, pitch=40, per_row=10):
    x, y = (i % per_row) * pitch, (i // per_row) * pitch
    return (x, y, x + size, y + size)


A, A2, FAR = (0, 0, 9, 9), (0, 0, 9, 4), (100, 100, 140, 150)


# ---- random walks ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("row_cap, rows", [(96, "all"), (5, "all"), (96, "fewer")])
@pytest.mark.parametrize("seed", [1, 2])
def test_random_walks_equal_the_oracle(ctx, seed, row_cap, rows):
    """S = 2 interleaved streams, B = 12, cap = 8, T = 4: three consecutive step / identify calls on one tracker"""
    both = Both(ctx, 2, 4)
    cfg = config(0.3, 1, 3, 2)
    rng = np.random.default_rng(100 + seed)
    for det, counts, stream in random_walk(seed):
        track, offsets, src = both.step(det, counts, stream, cfg, row_cap)
        n = min(int(offsets[-1]), row_cap)
        n_rows = n if rows == "all" else max(n - 3, 0)                      # "fewer": the last rows of the table were not run
        idx, score = draw_rows(rng, row_cap)
        both.identify(idx, score, n_rows)
    assert both.ref.lost.sum() > 0 and (both.ref.next_id > 4).all()        # slots ran out and were reused
    both.close()


# ---- pinned rules -------------------------------------------------------------------------------------------

def test_tie_takes_the_lowest_slot_and_a_started_track_is_not_a_candidate(ctx):
    both = Both(ctx, 1, 4)
    cfg = config(0.3, 1, 3, 1)
    det, counts = frames_of([[FAR, FAR], [FAR]], cap=4)
    track, offsets, src = both.step(det, counts, np.zeros(2, np.int32), cfg, 8)
    # frame 0: the second identical box cannot take the track the first one started; frame 1: overlap 1.0 with both tracks -> slot 0
    assert track[0, 0].tolist() == [0, 0 | STARTED | EMBED] and track[0, 1].tolist() == [1, 1 | STARTED | EMBED]
    assert track[1, 0].tolist() == [0, 0 | EMBED] and offsets.tolist() == [0, 2, 3] and src[:3].tolist() == [0, 1, 4]
    both.identify(None, None, 0)
    assert both.ref.missed[0, :2].tolist() == [0, 1]
    both.close()


def test_threshold_is_strict(ctx):
    """track (0,0,9,9) against (0,0,9,4): the overlap is exactly 0.5 (50 / 100 with the +1 convention)"""
    below = np.nextafter(np.float32(0.5), np.float32(0), dtype=np.float32)
    for thr, continues in ((np.float32(0.5), False), (below, True)):
        both = Both(ctx, 1, 2)
        det, counts = frames_of([[A], [A2]], cap=2)
        track, _, _ = both.step(det, counts, np.zeros(2, np.int32), config(thr, 1, 5, 5), 4)
        assert track[1, 0].tolist() == ([0, 0] if continues else [1, 1 | STARTED | EMBED]), thr
        both.identify(None, None, 0)
        both.close()


def test_nan_never_hits(ctx):
    nan_box = (np.nan, 0, 9, 9)
    both = Both(ctx, 1, 4)
    det, counts = frames_of([[A], [nan_box], [nan_box], [A]], cap=2)
    track, _, _ = both.step(det, counts, np.zeros(4, np.int32), config(0.0, 5, 9, 9), 8)
    assert track[:, 0, 0].tolist() == [0, 1, 2, 0]                         # each NaN box starts a track of its own; the real one goes on
    assert (track[1:3, 0, 1] & STARTED).all() and not track[3, 0, 1] & STARTED
    both.identify(None, None, 0)
    both.close()


@pytest.mark.parametrize("max_age", [0, 1])
def test_ageing_and_slot_reuse_inside_one_call(ctx, max_age):
    """T = 1.  Call 1 names track 0.  Call 2: seen, absent, then another face: at max_age 0 the slot is freed in frame 1 and reused in frame
    2 -- identify gives the old identity to frame 0 and the reset one to frame 2; at max_age 1 the track survives and the new face is lost."""
    both = Both(ctx, 1, 1)
    cfg = config(0.3, max_age, 10, 1)
    det, counts = frames_of([[A]], cap=2)
    both.step(det, counts, np.zeros(1, np.int32), cfg, 4)
    both.identify(np.array([3, -1, -1, -1]), np.array([0.75, 0, 0, 0]), 1)
    det, counts = frames_of([[A], [], [FAR]], cap=2)
    track, offsets, src = both.step(det, counts, np.zeros(3, np.int32), cfg, 4)
    assert track[0, 0].tolist() == [0, 0]                                  # named: refresh 10, no embedding
    ii, sc = both.identify(np.array([4, -1, -1, -1]), np.array([0.5, 0, 0, 0]), 1)
    assert (ii[0, 0], sc[0, 0]) == (3, np.float32(0.75))
    if max_age == 0:
        assert track[2, 0].tolist() == [1, 0 | STARTED | EMBED] and offsets.tolist() == [0, 0, 0, 1]
        assert (ii[2, 0], sc[2, 0]) == (4, np.float32(0.5))                # reset first, then the new face's own row
        assert both.ref.lost[0] == 0
    else:
        assert track[2, 0].tolist() == [-1, -1] and both.ref.lost[0] == 1
        assert (ii[2, 0], sc[2, 0]) == (4, np.float32(0.5))                # an untracked face reports its own row
        assert both.ref.id[0, 0] == -1                                     # unmatched in frames 1 and 2: freed at the end of frame 2, too late
    # a third call: the freed / reset identity does not come back
    det, counts = frames_of([[FAR]], cap=2)
    both.step(det, counts, np.zeros(1, np.int32), cfg, 4)
    both.identify(np.array([-1, -1, -1, -1]), np.zeros(4), 1)
    both.close()


def test_counts_outside_the_capacity(ctx):
    both = Both(ctx, 1, 8)
    det, _ = frames_of([[grid_box(i) for i in range(4)]] * 3, cap=4)
    counts = np.array([9, -3, 4], np.int32)                                # > cap: cap faces; < 0: none
    track, offsets, _ = both.step(det, counts, np.zeros(3, np.int32), config(0.3, 1, 3, 1), 16)
    assert offsets.tolist() == [0, 4, 4, 8] and (track[1] == -1).all()
    both.identify(None, None, 0)
    both.close()


def test_skipped_frames_change_nothing(ctx):
    rng = np.random.default_rng(5)
    det, counts = frames_of([[A, FAR], [FAR, A], [A]], cap=3)
    cfg = config(0.3, 0, 3, 1)
    with_skip, without = Both(ctx, 2, 3), Both(ctx, 2, 3)
    t1, o1, s1 = with_skip.step(det, counts, np.array([1, -1, 1], np.int32), cfg, 8)
    t2, o2, s2 = without.step(det[[0, 2]], counts[[0, 2]], np.array([1, 1], np.int32), cfg, 8)
    assert (t1[1] == -1).all() and same(t1[[0, 2]], t2) and o1.tolist() == [0, 2, 2, 3] and o2.tolist() == [0, 2, 3]
    assert s1[:3].tolist() == [0, 1, 6] and s2[:3].tolist() == [0, 1, 3]
    idx, score = draw_rows(rng, 8)
    i1, c1 = with_skip.identify(idx, score, 3)
    i2, c2 = without.identify(idx, score, 3)
    assert (i1[1] == -1).all() and not c1[1].any() and same(i1[[0, 2]], i2) and same(c1[[0, 2]], c2)
    assert all(same(a, b) for a, b in zip(with_skip.gpu.state(), without.gpu.state()))
    with_skip.close()
    without.close()


def test_slot_overflow_and_row_overflow(ctx):
    """T = 4 with 6 detections: two are untracked (-1, with every flag bit), lost grows, they report their own rows; with row_cap 3 the
    total stays unclipped and src is cut (the guard words behind src and every output are checked by every call of these tests)"""
    for row_cap in (8, 3):
        both = Both(ctx, 1, 4)
        det, counts = frames_of([[grid_box(i) for i in range(6)]], cap=6)
        track, offsets, src = both.step(det, counts, np.zeros(1, np.int32), config(0.3, 1, 3, 1), row_cap)
        assert track[0, :4, 0].tolist() == [0, 1, 2, 3] and (track[0, 4:] == -1).all() and both.ref.lost[0] == 2
        assert offsets.tolist() == [0, 6] and src.tolist() == list(range(min(6, row_cap))) + [-1] * max(row_cap - 6, 0)
        idx = np.array([0, 1, 2, 3, 4, -1, 0, 0], np.int32)[:row_cap]
        score = np.array([.5, .5, .5, .5, .25, 0, .9, .9], np.float32)[:row_cap]
        ii, sc = both.identify(idx, score, min(6, row_cap))
        if row_cap == 8:
            assert ii[0].tolist() == [0, 1, 2, 3, 4, -1] and sc[0, 4] == np.float32(.25)
        else:
            assert ii[0].tolist() == [0, 1, 2, -1, -1, -1]
        both.close()


def test_all_64_lanes(ctx):
    """T = 64, cap = 80, 70 detections per frame (two chunks of the walk's 64-box loads); the second frame meets the tracks in another order"""
    rng = np.random.default_rng(9)
    boxes = [grid_box(i) for i in range(70)]
    perm = rng.permutation(70)
    det, counts = frames_of([boxes, [boxes[j] for j in perm]], cap=80)
    both = Both(ctx, 1, 64)
    track, offsets, src = both.step(det, counts, np.zeros(2, np.int32), config(0.3, 1, 3, 1), 200)
    assert track[0, :64, 0].tolist() == list(range(64)) and both.ref.lost[0] == 6 + int((perm >= 64).sum())
    assert sorted(track[1, :70, 0][perm < 64].tolist()) == list(range(64))
    idx, score = draw_rows(rng, 200)
    both.identify(idx, score, int(offsets[-1]))
    both.close()


def test_tracking_without_a_gallery(ctx):
    both = Both(ctx, 1, 4)
    det, counts = frames_of([[A, FAR], [A]], cap=2)
    both.step(det, counts, np.zeros(2, np.int32), config(0.3, 1, 3, 1), 4)
    ii, sc = both.identify(None, None, 0)                                  # NULL idx / score: only the resets
    assert (ii == -1).all() and not sc.any() and both.ref.ident_idx[0, :2].tolist() == [-1, -1]
    both.close()


@pytest.mark.parametrize("named", [True, False])
def test_known_switches_the_interval_only_after_identify(ctx, named):
    both = Both(ctx, 1, 2)
    cfg = config(0.3, 1, 3, 1)
    det, counts = frames_of([[A]] * 3, cap=1)
    track, offsets, _ = both.step(det, counts, np.zeros(3, np.int32), cfg, 4)
    assert offsets.tolist() == [0, 1, 2, 3]                                # nobody has named it yet: retry = 1, every frame
    both.identify(np.array([2 if named else -1, -1, -1, -1]), np.array([.5 if named else 0, 0, 0, 0]), 3)
    track, offsets, _ = both.step(det, counts, np.zeros(3, np.int32), cfg, 4)
    assert offsets.tolist() == ([0, 0, 0, 1] if named else [0, 1, 2, 3])   # named: refresh = 3
    both.identify(np.array([1, -1, -1, -1]), np.array([.5, 0, 0, 0]), int(offsets[-1]))   # an equal score does not replace the name
    assert both.ref.ident_idx[0, 0] == (2 if named else 1)
    both.close()


def test_reset(ctx):
    both = Both(ctx, 2, 3)
    det, counts = frames_of([[A], [FAR]], cap=1)
    both.step(det, counts, np.array([0, 1], np.int32), config(), 4)
    both.identify(np.array([1, 2, 0, 0]), np.array([.5, .5, 0, 0]), 2)
    both.gpu.reset(1)
    both.ref.reset(1)
    both.check_state()
    assert both.ref.next_id.tolist() == [1, 0]
    both.gpu.reset(-1)
    both.ref.reset(-1)
    both.check_state()
    both.close()


# ---- refusals -----------------------------------------------------------------------------------------------

def test_refusals(ctx):
    lib, h = ctx.lib, ctx.handle
    trk = C.c_void_p()
    for S, T in ((0, 4), (1, 0), (1, 65), (-1, 4)):
        assert lib.fid_tracker_create(h, S, T, C.byref(trk)) == -1 and b"tracker" in lib.fid_last_error()
    assert lib.fid_tracker_create(h, 1, 4, None) == -1
    g = GpuTracker(ctx, 2, 4)
    B, cap, row_cap = 2, 2, 4
    det, counts = frames_of([[A], [A]], cap=cap)
    d_det, d_counts = ctx.to_device(det), ctx.to_device(counts)
    outs = [ctx.to_device(np.full(n, GUARD, np.int32)) for n in (B * cap * 2, B + 1, row_cap, B * cap, B * cap)]
    d_track, d_off, d_src, d_ii, d_is = outs
    d_idx, d_score = ctx.to_device(np.zeros(row_cap, np.int32)), ctx.to_device(np.zeros(row_cap, np.float32))
    stream = np.zeros(B, np.int32)
    p = lambda b: C.c_void_p(b.ptr)

    def step(trk=g.h, det=p(d_det), counts=p(d_counts), stream=stream, B=B, cap=cap, cfg=config(), track=p(d_track), off=p(d_off), src=p(d_src),
             row_cap=row_cap):
        return lib.fid_track_step(h, trk, det, counts, _i32(stream) if stream is not None else None, B, cap,
                                  C.byref(cfg) if cfg is not None else None, track, off, src, row_cap)

    def identify(trk=g.h, counts=p(d_counts), stream=stream, B=B, cap=cap, track=p(d_track), off=p(d_off), src=p(d_src), row_cap=row_cap,
                 idx=p(d_idx), score=p(d_score), n_rows=row_cap, ii=p(d_ii), is_=p(d_is)):
        return lib.fid_track_identify(h, trk, counts, _i32(stream) if stream is not None else None, B, cap, track, off, src, row_cap, idx, score,
                                      n_rows, ii, is_)

    def untouched():
        return all((b.download() == GUARD).all() for b in outs)

    bad_steps = [dict(trk=None), dict(det=None), dict(counts=None), dict(stream=None), dict(cfg=None), dict(track=None), dict(off=None),
                 dict(src=None), dict(B=0), dict(B=-1), dict(cap=0), dict(B=1 << 20, cap=1 << 12, stream=np.zeros(1 << 20, np.int32)),
                 dict(row_cap=0), dict(row_cap=-5), dict(cfg=config(iou=np.nan)), dict(cfg=config(iou=1.0)), dict(cfg=config(iou=-0.1)),
                 dict(cfg=config(max_age=-1)), dict(cfg=config(refresh=0)), dict(cfg=config(retry=0)), dict(stream=np.array([0, 2], np.int32))]
    for kw in bad_steps:
        assert step(**kw) == -1, kw
        assert len(lib.fid_last_error()) > 0
    assert step(stream=np.array([0, 2], np.int32)) == -1 and b"stream[1] = 2" in lib.fid_last_error()
    assert step(cfg=config(iou=1.0)) == -1 and b"iou_thresh" in lib.fid_last_error()
    assert identify() == -1 and b"pending" in lib.fid_last_error()          # no step yet
    assert untouched()
    before = g.state()
    assert step() == 0
    assert step() == -1 and b"identify" in lib.fid_last_error()             # step after step
    assert lib.fid_tracker_reset(h, g.h, 0) == -1                           # one stream's reset between step and identify
    after_step = [b.download() for b in outs[3:]]
    bad_ident = [dict(trk=None), dict(counts=None), dict(stream=None), dict(track=None), dict(off=None), dict(src=None), dict(ii=None),
                 dict(is_=None), dict(idx=None), dict(score=None), dict(n_rows=-1), dict(n_rows=row_cap + 1), dict(B=0), dict(cap=0),
                 dict(row_cap=0), dict(stream=np.array([0, 2], np.int32)), dict(stream=np.array([0, 1], np.int32)), dict(B=1, stream=stream[:1]),
                 dict(cap=1), dict(row_cap=8, n_rows=4)]
    for kw in bad_ident:
        assert identify(**kw) == -1, kw
    assert identify(n_rows=row_cap + 1) == -1 and b"n_rows" in lib.fid_last_error()
    assert all((b.download() == a).all() for a, b in zip(after_step, outs[3:]))
    assert identify(idx=None, score=None, n_rows=0) == 0
    assert identify() == -1 and b"pending" in lib.fid_last_error()
    assert lib.fid_tracker_reset(h, g.h, 2) == -1 and lib.fid_tracker_reset(h, g.h, -2) == -1
    assert lib.fid_tracker_read(h, g.h, None, None) == -1
    assert before[0][0, 0, 0] == -1 and g.state()[0][0, 0, 0] == 0
    g.close()


# ---- the pipeline -------------------------------------------------------------------------------------------

H = W = 320
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
    """SCRFD-500M at 320x320 and MobileFaceNet with seeded weights; 12 frames, each the previous one shifted by 2 pixels"""
    old = os.environ.get("FID_AUTOTUNE")
    os.environ["FID_AUTOTUNE"] = "0"
    from scrfd_arcface_facerecognition_amd import archs
    from scrfd_arcface_facerecognition_amd.engine import CompiledNet, Gallery, resolve_model
    from scrfd_arcface_facerecognition_amd.pipeline import calibrate_detector_bias
    s = Scene()
    rng = np.random.default_rng(41)
    wide = smooth_image(rng, H, W + 2 * 12)
    s.frames = np.stack([wide[:, 2 * t:2 * t + W] for t in range(12)])
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


def oracle_step(ref, pipe, stream, n_frames=None):
    """feed the oracle what the pipeline's last step saw: the downloaded detections and the idx / score of the rows that ran"""
    n = pipe.B if n_frames is None else n_frames
    det, counts = pipe.post.det.download()[:n], pipe.post.counts.download()[:n]
    cfg = pipe.cfg
    out = ref.step(det, counts, np.asarray(stream)[:n], cfg.iou_thresh, cfg.max_age, cfg.refresh, cfg.retry, pipe.row_cap)
    ident = ref.identify(pipe.idx.download(), pipe.score.download(), pipe.n_run)
    return out, ident, det, counts


def test_tracked_pipeline_at_refresh_1_runs_the_packed_table(ctx, scene):
    from scrfd_arcface_facerecognition_amd.pipeline import PackedFacePipeline, TrackedFacePipeline
    s = scene
    fr = ctx.to_device(s.frames[:PB])
    packed = PackedFacePipeline(ctx, s.det, s.rec, batch=PB, row_cap=256)
    packed.run_step(fr, H, W, s.gallery, THRESH)
    want = packed.results(s.gallery)
    tracked = TrackedFacePipeline(ctx, s.det, s.rec, batch=PB, row_cap=256, refresh=1, retry=1, max_tracks=64)
    tracked.run_step(fr, H, W, s.gallery, THRESH)
    n = int(packed.offsets.download()[PB])
    print(f"\nfaces per frame: {[len(r) for r in want]}")
    assert 0 < n <= 256
    # every face is due every frame: the same table goes into the same kernels
    assert same(tracked.src.download(), packed.src.download()) and same(tracked.offsets.download(), packed.offsets.download())
    assert same(tracked.idx.download()[:n], packed.idx.download()[:n]) and same(tracked.score.download()[:n], packed.score.download()[:n])
    assert tracked.rows_embedded == n
    ref = Tracker(1, 64)
    (track, offsets, src), (ii, sc), det, counts = oracle_step(ref, tracked, np.zeros(PB, np.int32))
    assert same(tracked.track.download(), track) and same(tracked.ident_idx.download(), ii) and same(tracked.ident_score.download(), sc)
    res = tracked.results_tracked(s.gallery)
    for b in range(PB):
        assert len(res[b]) == counts[b] == len(want[b])
        for f, (bb, score, kps, name, sim, tid, started) in enumerate(res[b]):
            assert np.array_equal(bb, det[b, f, :4]) and score == det[b, f, 4] and kps.shape == (5, 2)
            assert tid == track[b, f, 0] and started == bool(track[b, f, 1] >= 0 and track[b, f, 1] & STARTED)
            assert name == (s.gallery.names[ii[b, f]] if ii[b, f] >= 0 else "Unknown") and sim == float(sc[b, f])
    gs, gt = tracked.tracker_state()
    assert same(gs, ref.state()[0]) and same(gt, ref.state()[1])
    tracked.reset()
    assert (tracked.tracker_state()[0][..., 0] == -1).all() and not tracked.tracker_state()[1].any()
    tracked.close()


@pytest.mark.parametrize("rows", ["capacity", "count"])
def test_tracked_pipeline_embeds_only_the_due_faces(ctx, scene, rows):
    from scrfd_arcface_facerecognition_amd.pipeline import PackedFacePipeline, TrackedFacePipeline
    s = scene
    packed = PackedFacePipeline(ctx, s.det, s.rec, batch=PB, row_cap=256)
    tracked = TrackedFacePipeline(ctx, s.det, s.rec, batch=PB, row_cap=256, refresh=1000, retry=1, max_tracks=64, rows=rows)
    ref = Tracker(1, 64)
    for step in range(3):
        fr = ctx.to_device(s.frames[step * PB:(step + 1) * PB])
        packed.run_step(fr, H, W, s.gallery, THRESH)
        n_packed = int(packed.offsets.download()[PB])
        tracked.run_step(fr, H, W, s.gallery, THRESH)
        (track, offsets, src), (ii, sc), det, counts = oracle_step(ref, tracked, np.zeros(PB, np.int32))
        print(f"\nstep {step}: faces {n_packed}, rows embedded {tracked.rows_embedded}, known tracks {int((ref.ident_idx[ref.id >= 0] >= 0).sum())}")
        assert tracked.rows_embedded == int(offsets[PB]) and same(tracked.src.download(), src)
        assert tracked.rows_embedded <= n_packed == int(counts.sum())
        if step > 0:
            assert tracked.rows_embedded < n_packed
        tracked.post.check()                                               # (raises on a capacity overflow)
        res = tracked.results(s.gallery)
        assert [len(r) for r in res] == counts.tolist() and all(len(face) == 5 for r in res for face in r)
        assert same(tracked.ident_idx.download(), ii) and same(tracked.ident_score.download(), sc)
        if rows == "count" and tracked.rows_embedded > 0:
            assert tracked.n_run in tracked.buckets and tracked.n_run >= tracked.rows_embedded > tracked.n_run - 64
    gs, gt = tracked.tracker_state()
    assert same(gs, ref.state()[0]) and same(gt, ref.state()[1])
    tracked.close()


def test_stream_runner_does_not_age_tracks_with_its_padding(ctx, scene):
    """6 frames at B = 4: the second step carries two black padding frames; the tracker ends where the oracle ends without them"""
    from scrfd_arcface_facerecognition_amd.pipeline import TrackedFacePipeline
    from scrfd_arcface_facerecognition_amd.video import StreamRunner
    s = scene
    tracked = TrackedFacePipeline(ctx, s.det, s.rec, batch=PB, row_cap=256, streams=2, refresh=1000, retry=1, max_age=0)
    runner = StreamRunner(tracked, s.gallery, (H, W), similarity_thresh=THRESH)
    ref = Tracker(2, 64)
    cams = [1, 1, 0, 1, 1, 0]
    got = []
    for i, faces in enumerate(runner.run((c, f) for c, f in zip(cams, s.frames[:6]))):
        if i % PB == 0:                                                    # the step of this batch has run, the next one has not
            n = min(PB, 6 - i)
            assert tracked._stream.tolist() == cams[i:i + n] + [-1] * (PB - n)
            oracle_step(ref, tracked, cams[i:i + n], n_frames=n)
            tail = tracked.results_tracked(s.gallery)[n:]
            assert tail == [[] for _ in range(PB - n)]
        got.append(faces)
    runner.close()
    assert len(got) == 6 and all(len(face) == 5 for r in got for face in r) and sum(len(r) for r in got) > 0
    gs, gt = tracked.tracker_state()
    assert same(gs, ref.state()[0]) and same(gt, ref.state()[1])
    assert (gs[..., 0] >= 0).any()                                         # (max_age 0: two more frames without a face would have freed them)
    tracked.close()
