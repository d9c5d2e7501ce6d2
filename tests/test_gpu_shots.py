"""GPU: the best-shot keeper (fid_shot_score, fid_shots_*, fid_track_keep; pipeline.TrackedFacePipeline(best_shot=True); video.StreamRunner).
The yardstick is tests/shot_oracle.py; every comparison is bit for bit: live meta, finished meta, q and crop bytes, count, dropped.  The
keeper cases drive the C-ABI with the synthetic detections of tests/test_gpu_track.py (its device tracker makes the track tables): no network
runs in them.  Live payloads are not readable through the ABI; every case ends with a flush, which moves them to the finished store."""
import ctypes as C

import numpy as np
import pytest

from shot_oracle import CROP, Keeper, Tracker, draw_rows, draw_scores, measure_rows, random_walk, row_payload, shot_score
from test_gpu_track import A, FAR, H, PB, THRESH, W, GpuTracker, _i32, bits, config, ctx, frames_of, grid_box, oracle_step, same, scene  # noqa: F401

pytestmark = pytest.mark.gpu

CROP_BYTES = int(np.prod(CROP))
MW = 16


class Shots:
    """a device tracker + keeper and their oracles, driven together; keep / flush / clear compare everything that can be read"""

    def __init__(self, ctx, S, T, dim=32, finished_cap=64, keep_crops=True, seed=0):
        from scrfd_arcface_facerecognition_amd._lib import check
        self.ctx, self.check, self.S, self.T, self.dim, self.cap_f, self.keep_crops = ctx, check, S, T, dim, finished_cap, keep_crops
        self.trk, self.ref_trk = GpuTracker(ctx, S, T), Tracker(S, T)
        self.ref = Keeper(S, T, dim, finished_cap, keep_crops)
        self.h = C.c_void_p()
        check(ctx.lib.fid_shots_create(ctx.handle, S, T, dim, finished_cap, int(keep_crops), C.byref(self.h)))
        self.rng = np.random.default_rng(900 + seed)
        self.calls = 0
        self.compare()

    def step(self, det, counts, stream, cfg, row_cap, n_rows=None):
        """tracker step + identify on the device and in the oracle -> (track, offsets, src); the identity of every face is drawn at random"""
        t = self.trk
        got = t.step(det, counts, stream, cfg, row_cap)
        want = self.ref_trk.step(det, counts, stream, cfg.iou_thresh, cfg.max_age, cfg.refresh, cfg.retry, row_cap)
        assert all(same(g, w) for g, w in zip(got, want))
        self.n = min(int(want[1][-1]), row_cap) if n_rows is None else n_rows
        idx, sc = draw_rows(self.rng, row_cap)
        t.ii, t.is_ = t.ctx.to_device(np.zeros(t.B * t.cap, np.int32)), t.ctx.to_device(np.zeros(t.B * t.cap, np.float32))
        di, ds = t.ctx.to_device(idx), t.ctx.to_device(sc)
        self.check(t.ctx.lib.fid_track_identify(t.ctx.handle, t.h, C.c_void_p(t.counts.ptr), _i32(t.stream), t.B, t.cap, C.c_void_p(t.track.ptr),
                                                C.c_void_p(t.offsets.ptr), C.c_void_p(t.src.ptr), row_cap, C.c_void_p(di.ptr), C.c_void_p(ds.ptr),
                                                self.n, C.c_void_p(t.ii.ptr), C.c_void_p(t.is_.ptr)))
        self.ident = self.ref_trk.identify(idx, sc, self.n)
        self.tables = want
        self.det_host = np.asarray(det, np.float32)
        return want

    def payload(self, score=None):
        """the step's rows: score (default: drawn), q, crops"""
        rc = self.trk.row_cap
        self.score = draw_scores(self.rng, rc) if score is None else np.asarray(list(score) + [0.5] * (rc - len(score)), np.float32)
        self.q, self.crops = row_payload(self.rng, rc, self.dim, self.calls)

    def keep_raw(self, ident=True, q_off=0, crop_off=0, **kw):
        """fid_track_keep on the last step's buffers -> return code; kw overrides single arguments (refusals)"""
        t, ctx = self.trk, self.ctx
        rc = t.row_cap
        self.d_score = ctx.to_device(self.score)
        qbuf = np.zeros(rc * self.dim * 2 + 16, np.uint8)
        qbuf[q_off:q_off + rc * self.dim * 2] = self.q.view(np.uint8).reshape(-1)
        cbuf = np.zeros(rc * CROP_BYTES + 16, np.uint8)
        cbuf[crop_off:crop_off + rc * CROP_BYTES] = self.crops.reshape(-1)
        self.d_q, self.d_crops = ctx.to_device(qbuf), ctx.to_device(cbuf)
        a = dict(shots=self.h, trk=t.h, stream=t.stream, B=t.B, cap=t.cap, track=C.c_void_p(t.track.ptr), offsets=C.c_void_p(t.offsets.ptr),
                 src=C.c_void_p(t.src.ptr), row_cap=rc, n_rows=self.n, score=C.c_void_p(self.d_score.ptr), q=C.c_void_p(self.d_q.ptr + q_off),
                 crops=C.c_void_p(self.d_crops.ptr + crop_off) if self.keep_crops else None, det=C.c_void_p(t.det.ptr),
                 ii=C.c_void_p(t.ii.ptr) if ident else None, is_=C.c_void_p(t.is_.ptr) if ident else None)
        a.update(kw)
        return ctx.lib.fid_track_keep(ctx.handle, a["shots"], a["trk"], _i32(a["stream"]) if a["stream"] is not None else None, a["B"], a["cap"],
                                      a["track"], a["offsets"], a["src"], a["row_cap"], a["n_rows"], a["score"], a["q"], a["crops"], a["det"],
                                      a["ii"], a["is_"])

    def keep(self, score=None, ident=True, **kw):
        self.payload(score)
        self.check(self.keep_raw(ident=ident, **kw))
        track, offsets, src = self.tables
        self.ref.keep(self.ref_trk.id, self.trk.stream, self.trk.cap, track, offsets, src, self.trk.row_cap, self.n, self.score, self.q,
                      self.crops, self.det_host, *(self.ident if ident else (None, None)))
        self.calls += 1
        self.compare()

    def flush(self, stream=-1):
        self.check(self.ctx.lib.fid_shots_flush(self.ctx.handle, self.h, stream))
        self.ref.flush(stream)
        self.compare()

    def clear(self):
        self.check(self.ctx.lib.fid_shots_clear_finished(self.ctx.handle, self.h))
        self.ref.clear_finished()
        self.compare()

    def read(self):
        """(live meta, count, dropped, finished meta / q / crops [count])"""
        ctx = self.ctx
        live = np.empty((self.S, self.T, MW), np.int32)
        self.check(ctx.lib.fid_shots_read(ctx.handle, self.h, _i32(live)))
        count, dropped = C.c_int32(-7), C.c_int32(-7)
        pm, pq, pc = C.c_void_p(), C.c_void_p(), C.c_void_p(1)
        self.check(ctx.lib.fid_shots_finished(ctx.handle, self.h, C.byref(count), C.byref(dropped), C.byref(pm), C.byref(pq), C.byref(pc)))
        n = count.value
        assert 0 <= n <= self.cap_f and (pc.value is None) == (not self.keep_crops)
        meta = ctx.borrow(pm.value, (self.cap_f, MW), np.int32).download()[:n]
        q = ctx.borrow(pq.value, (self.cap_f, self.dim), np.uint16).download()[:n]
        crops = ctx.borrow(pc.value, (self.cap_f,) + CROP, np.uint8).download()[:n] if self.keep_crops else None
        return live, n, dropped.value, meta, q, crops

    def compare(self):
        live, n, dropped, meta, q, crops = self.read()
        r = self.ref
        assert np.array_equal(live, r.live_meta), np.argwhere(live != r.live_meta)[:8]
        assert (n, dropped) == (r.count, r.dropped)
        assert np.array_equal(meta, r.fin_meta[:n]), np.argwhere(meta != r.fin_meta[:n])[:8]
        assert np.array_equal(q, r.fin_q[:n]), np.argwhere(q != r.fin_q[:n])[:8]
        if self.keep_crops:
            assert np.array_equal(crops, r.fin_crop[:n]), [int((crops[k] != r.fin_crop[k]).sum()) for k in range(n)]

    def close(self):
        self.check(self.ctx.lib.fid_shots_destroy(self.ctx.handle, self.h))
        self.trk.close()


def zeros(n):
    return np.zeros(n, np.int32)


# ---- random walks ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("row_cap", [96, 5])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_walks_equal_the_oracle(ctx, seed, row_cap):
    """S = 2 interleaved streams, B = 12, cap = 8, T = 4, dim = 32: three step / identify / keep calls on one keeper, then a flush"""
    sh = Shots(ctx, 2, 4, seed=seed)
    cfg = config(0.3, 1, 3, 2)
    for det, counts, stream in random_walk(seed):
        sh.step(det, counts, stream, cfg, row_cap)
        sh.keep()
    assert sh.ref.count > 2 and (sh.ref.live_meta[..., 1] != -1).any()
    sh.flush()
    assert not (sh.ref.live_meta[..., 1] != -1).any() and sh.ref.dropped == 0
    sh.close()


# ---- pinned rules -------------------------------------------------------------------------------------------

def test_tie_keeps_the_earlier_row(ctx):
    sh = Shots(ctx, 1, 2)
    det, counts = frames_of([[A]] * 3, cap=2)
    sh.step(det, counts, zeros(3), config(0.3, 1, 9, 1), 8)                # retry 1: a row per frame
    sh.keep(score=[0.25, 0.5, 0.5])
    m = sh.ref.live_meta[0, 0]
    assert (m[1], m[5], m[6]) == (0, 1, 3) and m[4] == bits(np.float32(0.5))[0]
    sh.flush()
    assert np.array_equal(sh.ref.fin_q[0], sh.q[1]) and np.array_equal(sh.ref.fin_crop[0], sh.crops[1])
    sh.close()


def test_nan_and_negative_scores_are_never_stored_and_a_zero_is(ctx):
    """track 0 (A): NaN, negative, 0.0, NaN -> the shot is the third row with score 0; track 1 (FAR): only NaN and negative rows -> it ends
    without a record"""
    sh = Shots(ctx, 1, 2)
    det, counts = frames_of([[A, FAR]] * 4, cap=2)
    sh.step(det, counts, zeros(4), config(0.3, 1, 9, 1), 16)
    nan = np.nan
    sh.keep(score=[nan, -1.0, -0.5, nan, 0.0, -0.25, nan, nan])
    assert sh.ref.live_meta[0, 0, 4] == 0 and sh.ref.live_meta[0, 0, 5] == 2 and sh.ref.live_meta[0, 0, 6] == 4
    assert sh.ref.live_meta[0, 1, 4] == bits(np.float32(-1))[0] and sh.ref.live_meta[0, 1, 6] == 4 and not sh.ref.live_meta[0, 1, 7:].any()
    sh.flush()
    assert sh.ref.count == 1 and sh.ref.fin_meta[0, 1] == 0 and np.array_equal(sh.ref.fin_crop[0], sh.crops[4])
    sh.close()


def test_rows_at_and_beyond_n_rows_are_ignored(ctx):
    sh = Shots(ctx, 1, 2)
    det, counts = frames_of([[A]] * 3, cap=2)
    sh.step(det, counts, zeros(3), config(0.3, 1, 9, 1), 8, n_rows=2)      # the table has three rows; only two were run
    sh.keep(score=[0.25, 0.125, 0.75])
    assert sh.ref.live_meta[0, 0, 6] == 2 and sh.ref.live_meta[0, 0, 5] == 0
    sh.flush()
    sh.close()


def test_untracked_rows_are_ignored(ctx):
    """T = 1 with two faces: the second one finds no slot (track word -1); its row has the best score and is not kept"""
    sh = Shots(ctx, 1, 1)
    det, counts = frames_of([[A, FAR]] * 2, cap=2)
    track, offsets, src = sh.step(det, counts, zeros(2), config(0.3, 1, 9, 1), 8)
    assert track[0, 1].tolist() == [-1, -1] and offsets[-1] == 4
    sh.keep(score=[0.25, 0.75, 0.125, 0.75])
    assert sh.ref.live_meta[0, 0, 6] == 2 and sh.ref.live_meta[0, 0, 4] == bits(np.float32(0.25))[0]
    sh.flush()
    assert sh.ref.count == 1
    sh.close()


def test_skipped_frames_neither_count_nor_finish(ctx):
    sh = Shots(ctx, 2, 2)
    det, counts = frames_of([[A], [FAR], [A]], cap=2)
    sh.step(det, counts, np.array([1, -1, 1], np.int32), config(0.3, 0, 9, 1), 8)
    sh.keep(score=[0.25, 0.5])
    assert sh.ref.frames.tolist() == [0, 2] and sh.ref.live_meta[1, 0, 5] == 1 and sh.ref.count == 0
    sh.step(det, counts, np.array([-1, -1, -1], np.int32), config(0.3, 0, 9, 1), 8)      # nothing but skipped frames
    sh.keep()
    assert sh.ref.frames.tolist() == [0, 2] and sh.ref.count == 0 and sh.ref.live_meta[1, 0, 1] == 0
    sh.flush()
    sh.close()


def test_a_track_ends_and_another_starts_in_its_slot_inside_one_call(ctx):
    """T = 1, max_age 0: A is seen, absent, then FAR takes the slot -- both have rows of this call; A's payload goes from its row straight to
    the finished store, FAR's row to the live store"""
    sh = Shots(ctx, 1, 1)
    det, counts = frames_of([[A], [], [FAR], [FAR]], cap=2)
    track, _, _ = sh.step(det, counts, zeros(4), config(0.3, 0, 9, 1), 8)
    assert track[0, 0, 0] == 0 and track[2, 0, 0] == 1
    sh.keep(score=[0.5, 0.25, 0.75])
    assert sh.ref.count == 1 and sh.ref.fin_meta[0, 1] == 0 and np.array_equal(sh.ref.fin_crop[0], sh.crops[0])
    assert sh.ref.live_meta[0, 0, 1] == 1 and sh.ref.live_meta[0, 0, 5] == 3
    sh.flush()
    assert np.array_equal(sh.ref.fin_crop[1], sh.crops[2])
    sh.close()


def test_copy_order_the_old_shot_leaves_before_the_new_row_lands(ctx):
    """Call 1 stores A's shot in live entry (0, 0).  Call 2: A is gone (max_age 0) and B starts in slot 0 with a candidate row: the SAME call
    finishes A out of the live entry and stores B's row into it.  A's record must hold call 1's bytes, B's (after the flush) call 2's."""
    sh = Shots(ctx, 1, 1, dim=512)
    cfg = config(0.3, 0, 9, 1)
    det, counts = frames_of([[A]], cap=2)
    sh.step(det, counts, zeros(1), cfg, 8)
    sh.keep(score=[0.5])
    q1, crop1 = sh.q[0].copy(), sh.crops[0].copy()
    det, counts = frames_of([[], [FAR]], cap=2)
    sh.step(det, counts, zeros(2), cfg, 8)
    sh.keep(score=[0.75])
    assert sh.ref.count == 1 and np.array_equal(sh.ref.fin_q[0], q1) and np.array_equal(sh.ref.fin_crop[0], crop1)
    assert not np.array_equal(sh.crops[0], crop1)                          # (the two calls' rows differ in every byte pattern)
    sh.flush()
    assert sh.ref.count == 2 and np.array_equal(sh.ref.fin_crop[1], sh.crops[0])
    sh.close()


def test_all_64_lanes(ctx):
    """T = 64, every slot live with a shot; the next step has no face at max_age 0: all 64 end in the closing slot walk, in slot order"""
    sh = Shots(ctx, 1, 64, finished_cap=64, keep_crops=False)
    cfg = config(0.3, 0, 9, 1)
    det, counts = frames_of([[grid_box(i) for i in range(64)], []], cap=64)
    sh.step(det, counts, np.array([0, -1], np.int32), cfg, 64)
    sh.keep()
    assert (sh.ref.live_meta[0, :, 1] == np.arange(64)).all()
    sh.step(det[::-1], counts[::-1], np.array([0, -1], np.int32), cfg, 64)
    sh.keep()
    live = sh.ref.live_meta[0, :, 1] != -1
    assert not live.any() and sh.ref.count == int((sh.ref.fin_meta[:sh.ref.count, 1] >= 0).sum()) > 20       # (the drawn scores: ~70 % >= 0)
    assert (np.diff(sh.ref.fin_meta[:sh.ref.count, 1]) > 0).all()
    sh.close()


def test_finished_store_overflow_drops_and_counts(ctx):
    sh = Shots(ctx, 1, 8, finished_cap=2)
    cfg = config(0.3, 0, 9, 1)
    det, counts = frames_of([[grid_box(i) for i in range(5)], []], cap=8)
    sh.step(det, counts, zeros(2), cfg, 8)
    sh.keep(score=[0.5, 0.25, 0.75, 0.125, 0.0])
    assert (sh.ref.count, sh.ref.dropped) == (2, 3) and sh.ref.fin_meta[:2, 1].tolist() == [0, 1]
    assert not (sh.ref.live_meta[..., 1] != -1).any()
    sh.clear()
    assert (sh.ref.count, sh.ref.dropped) == (0, 0)
    sh.close()


def test_flush_of_one_stream_and_of_all(ctx):
    sh = Shots(ctx, 2, 4)
    det, counts = frames_of([[A, FAR], [A, FAR]], cap=2)
    sh.step(det, counts, np.array([0, 1], np.int32), config(0.3, 1, 9, 1), 8)
    sh.keep(score=[0.5, 0.25, 0.125, 0.75])
    sh.flush(1)
    assert sh.ref.count == 2 and (sh.ref.fin_meta[:2, 0] == 1).all() and (sh.ref.live_meta[0, :2, 1] != -1).all()
    sh.flush(-1)
    assert sh.ref.count == 4 and (sh.ref.fin_meta[2:4, 0] == 0).all()
    sh.flush(-1)                                                           # nothing is live: nothing changes
    assert sh.ctx.lib.fid_shots_flush(ctx.handle, sh.h, 2) == -1 and sh.ctx.lib.fid_shots_flush(ctx.handle, sh.h, -2) == -1
    sh.compare()
    sh.close()


def test_tracker_reset_then_keep(ctx):
    """after fid_tracker_reset the ids begin again at 0: the orphaned entry (stream 0, slot 0, id 0) finishes when the new track 0 starts in
    its slot; stream 1, reset too and without a face in the next step, loses its entry in the closing slot walk"""
    sh = Shots(ctx, 2, 2)
    cfg = config(0.3, 5, 9, 1)
    det, counts = frames_of([[A], [FAR]], cap=2)
    sh.step(det, counts, np.array([0, 1], np.int32), cfg, 8)
    sh.keep(score=[0.5, 0.25])
    sh.trk.reset(-1)
    sh.ref_trk.reset(-1)
    det, counts = frames_of([[FAR]], cap=2)
    track, _, _ = sh.step(det, counts, zeros(1), cfg, 8)
    assert track[0, 0, 0] == 0
    sh.keep(score=[0.125])
    assert sh.ref.count == 2 and sh.ref.fin_meta[:2, 0].tolist() == [0, 1] and sh.ref.fin_meta[0, 4] == bits(np.float32(0.5))[0]
    assert sh.ref.live_meta[0, 0, 4] == bits(np.float32(0.125))[0] and sh.ref.live_meta[0, 0, 6] == 1
    sh.flush()
    sh.close()


@pytest.mark.parametrize("dim, q_off, crop_off, crops", [(32, 0, 0, False), (512, 0, 0, True), (6, 2, 0, True), (32, 0, 4, True)])
def test_payload_sizes_and_alignments(ctx, dim, q_off, crop_off, crops):
    """keep_crops = 0 with a NULL crop pointer; dim = 512 (16-byte vectors); dim = 6 behind a pointer offset by 2 bytes (12-byte rows); a crop
    pointer offset by 4 bytes (byte loads).  Both copy paths: row -> finished store (a track that ends in the call it started in) and
    row -> live store -> finished store."""
    sh = Shots(ctx, 1, 2, dim=dim, keep_crops=crops)
    cfg = config(0.3, 0, 1, 1)                                             # (refresh 1: a row per frame whatever name the track drew)
    det, counts = frames_of([[A, FAR], [FAR], [grid_box(7)]], cap=2)
    sh.step(det, counts, zeros(3), cfg, 8)                                 # rows: A, FAR | FAR | a third face in A's slot
    sh.keep(score=[0.5, 0.25, 0.75, 0.125], q_off=q_off, crop_off=crop_off)
    assert sh.ref.count == 2 and sh.ref.fin_meta[:2, 1].tolist() == [0, 1] and sh.ref.live_meta[0, 0, 1] == 2
    q3, crop3 = sh.q[3].copy(), sh.crops[3].copy()
    det, counts = frames_of([[grid_box(7)]], cap=2)
    sh.step(det, counts, zeros(1), cfg, 8)
    sh.keep(score=[0.0625], q_off=q_off, crop_off=crop_off)                # a weaker row: the live payload of the first call stays
    sh.flush()
    assert sh.ref.count == 3 and np.array_equal(sh.ref.fin_q[2], q3) and sh.ref.fin_meta[2, 6] == 2
    assert not crops or np.array_equal(sh.ref.fin_crop[2], crop3)
    sh.close()


def test_refusals_leave_state_and_finished_store_unchanged(ctx):
    lib, h = ctx.lib, ctx.handle
    out = C.c_void_p()
    for args in ((0, 4, 32, 8, 1), (1, 0, 32, 8, 1), (1, 65, 32, 8, 1), (1, 4, 0, 8, 1), (1, 4, 32, 0, 1), (-1, 4, 32, 8, 0)):
        assert lib.fid_shots_create(h, *args, C.byref(out)) == -1 and b"shots" in lib.fid_last_error(), args
    assert lib.fid_shots_create(h, 1, 4, 32, 8, 1, None) == -1
    sh = Shots(ctx, 2, 4)
    cfg = config(0.3, 1, 9, 1)
    det, counts = frames_of([[A, FAR], [A]], cap=2)
    stream = np.array([0, 1], np.int32)
    sh.trk.step(det, counts, stream, cfg, 8)                               # a step whose identify has not run
    sh.ref_trk.step(det, counts, stream, cfg.iou_thresh, cfg.max_age, cfg.refresh, cfg.retry, 8)
    sh.n = 0
    sh.payload()
    sh.trk.ii = sh.trk.is_ = ctx.to_device(np.zeros(4, np.int32))
    assert sh.keep_raw() == -1 and b"identify" in lib.fid_last_error()
    sh.trk.identify(None, None, 0)
    sh.ref_trk.identify(None, None, 0)
    sh.step(det, counts, stream, cfg, 8)
    sh.keep()                                                              # live entries and, after the flush of stream 1, a finished record
    sh.flush(1)
    sh.step(det, counts, stream, cfg, 8)
    sh.payload()
    other = GpuTracker(ctx, 2, 2)
    fresh = GpuTracker(ctx, 2, 4)
    bad = [dict(shots=None), dict(trk=None), dict(stream=None), dict(track=None), dict(offsets=None), dict(src=None), dict(score=None),
           dict(q=None), dict(crops=None), dict(det=None), dict(ii=None), dict(is_=None), dict(n_rows=-1), dict(n_rows=9), dict(B=1),
           dict(B=0), dict(cap=3), dict(cap=0), dict(row_cap=16), dict(row_cap=0), dict(stream=np.array([0, 0], np.int32)),
           dict(trk=other.h), dict(trk=fresh.h)]
    before = sh.read()
    for kw in bad:
        assert sh.keep_raw(**kw) == -1, kw
        assert len(lib.fid_last_error()) > 0
    assert sh.keep_raw(n_rows=9) == -1 and b"n_rows" in lib.fid_last_error()
    assert sh.keep_raw(trk=fresh.h) == -1 and b"step" in lib.fid_last_error()
    assert lib.fid_shots_read(h, sh.h, None) == -1 and lib.fid_shots_finished(h, sh.h, None, None, None, None, None) == -1
    after = sh.read()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    sh.compare()
    sh.keep()                                                              # the good call goes through ...
    assert sh.keep_raw() == -1 and b"kept already" in lib.fid_last_error()  # ... once per step
    sh.compare()
    sh.step(det, counts, stream, cfg, 8)                                   # skipping a step's keep is allowed
    sh.step(det, counts, stream, cfg, 8)
    sh.keep()
    sh.flush()
    other.close()
    fresh.close()
    sh.close()


def test_shot_score_equals_the_host_twin(ctx):
    from scrfd_arcface_facerecognition_amd._lib import MeasureConfig
    lib, h = ctx.lib, ctx.handle
    for norms in ((100.0, 40.0, 8.0), (37.5, 11.0, 3.25)):
        stats, measure = measure_rows(3, n=300, norms=norms)
        cfg = MeasureConfig(*norms)
        host = np.empty(len(stats), np.float32)
        assert lib.fid_shot_score_host(stats.ctypes.data_as(C.c_void_p), measure.ctypes.data_as(C.c_void_p), len(stats), C.byref(cfg),
                                       host.ctypes.data_as(C.c_void_p)) == 0
        d_stats, d_measure = ctx.to_device(stats), ctx.to_device(measure)
        out = ctx.to_device(np.full(len(stats) + 4, 7.0, np.float32))
        assert lib.fid_shot_score(h, C.c_void_p(d_stats.ptr), C.c_void_p(d_measure.ptr), len(stats), C.byref(cfg), C.c_void_p(out.ptr)) == 0
        got = out.download()
        diff = np.flatnonzero(bits(got[:len(stats)]) != bits(host))
        assert len(diff) == 0, [(int(i), hex(bits(got)[i] & 0xFFFFFFFF), hex(bits(host)[i] & 0xFFFFFFFF), measure[i].tolist()) for i in diff[:4]]
        assert (got[len(stats):] == 7.0).all() and same(host, shot_score(stats, measure, *norms))
    assert lib.fid_shot_score(h, None, None, 0, None, None) == -1 and lib.fid_shot_score(h, C.c_void_p(d_stats.ptr), C.c_void_p(d_measure.ptr), 0,
                                                                                      C.byref(cfg), C.c_void_p(out.ptr)) == 0
    assert lib.fid_shot_score(h, C.c_void_p(d_stats.ptr), C.c_void_p(d_measure.ptr), 4, C.byref(MeasureConfig(0.0, 40.0, 8.0)),
                              C.c_void_p(out.ptr)) == -1
    assert (out.download()[:4] == got[:4]).all()


# ---- the pipeline -------------------------------------------------------------------------------------------

def oracle_keep(kp, ref_trk, pipe, stream, names):
    """feed the oracle keeper what the pipeline's last step saw: the downloaded tables, helpers.measure_crops on the downloaded crops, q"""
    from scrfd_arcface_facerecognition_amd.utils import helpers
    (track, offsets, src), (ii, sc), det, counts = oracle_step(ref_trk, pipe, stream)
    n, cap = pipe.n_run, pipe.post.cap
    live = min(int(offsets[-1]), n)
    crops, q = pipe.crops.download(), np.asarray(pipe.q.download()).view(np.uint16)
    stats, measure = np.zeros((n, 8), np.int64), np.zeros((n, 8), np.float32)
    if live:
        kps, M = pipe.post.kps.download().reshape(-1, 10)[src[:live]], pipe.M.download()[:live]
        for i, d in enumerate(helpers.measure_crops(crops[:live], kps.reshape(live, 5, 2), M.reshape(live, 2, 3))):
            stats[i, 7] = 1 | (2 if d["pose_valid"] else 0)
            measure[i, :7] = [d[k] for k in ("sharpness", "mean", "contrast", "clipped", "yaw", "pitch", "residual")]
    c = pipe.mcfg
    score = shot_score(stats, measure, c.sharpness_normalization, c.contrast_normalization, c.residual_normalization)
    if n:
        assert same(pipe.shot_score.download()[:n], score)
    kp.keep(ref_trk.id, stream, cap, track, offsets, src, pipe.row_cap, n, score, q, crops, det, ii, sc)


def check_records(recs, kp, names):
    assert len(recs) == kp.count
    for r, m, q, crop in zip(recs, kp.fin_meta, kp.fin_q, kp.fin_crop):
        f = m.view(np.float32)
        assert (r["stream"], r["track_id"], r["frame"], r["rows"]) == (m[0], m[1], m[5], m[6])
        assert r["name"] == (names[m[2]] if m[2] >= 0 else "Unknown") and r["similarity"] == float(f[3]) and r["shot_score"] == float(f[4])
        assert same(r["bbox"], f[7:11]) and r["det_score"] == float(f[11])
        if r["embedding"] is not None:
            assert np.array_equal(r["embedding"].view(np.uint16), q) and np.array_equal(r["crop"], crop)


def test_pipeline_best_shots_equal_the_oracle_and_group_where_they_lie(ctx, scene):
    from scrfd_arcface_facerecognition_amd.engine import VectorGallery
    from scrfd_arcface_facerecognition_amd.pipeline import TrackedFacePipeline
    s = scene
    pipes = [TrackedFacePipeline(ctx, s.det, s.rec, batch=PB, row_cap=256, refresh=3, retry=1, max_age=0, best_shot=True) for _ in range(2)]
    keepers, trackers = [Keeper(1, 64, 512, 256) for _ in range(2)], [Tracker(1, 64) for _ in range(2)]
    assert pipes[0].measure and pipes[0].shots
    for pipe, kp, trk in zip(pipes, keepers, trackers):
        for step in range(3):
            if step == 2:                                                  # the tracker forgets its tracks: the next keep finishes the orphans
                pipe.reset()
                trk.reset()
            pipe.run_step(ctx.to_device(s.frames[step * PB:(step + 1) * PB]), H, W, s.gallery, THRESH)
            oracle_keep(kp, trk, pipe, np.zeros(PB, np.int32), s.gallery.names)
            assert np.array_equal(pipe.shots_state(), kp.live_meta)
        ended = kp.count
        pipe.finish_all()
        kp.flush()
        assert kp.count > ended > 0 and kp.dropped == 0                    # tracks ended during the steps (the reset at the latest) and at the flush
    recs = pipes[0].finished()
    check_records(recs, keepers[0], s.gallery.names)
    assert all(r["embedding"] is not None and r["crop"].shape == (112, 112, 3) for r in recs) and pipes[0].finished_dropped == 0
    assert pipes[0].finished() == []                                       # cleared
    # the second pipe's records go to a store on the device; the same embeddings, downloaded, through group_visits into another store
    n = keepers[1].count
    emb = keepers[1].fin_q[:n].view(np.float16).astype(np.float32)
    want = VectorGallery(ctx, 512).group_visits(emb)
    exact = VectorGallery(ctx, 512).group_device(ctx.to_device(keepers[1].fin_q[:n]), n)
    store = VectorGallery(ctx, 512)
    recs2, groups = pipes[1].group_finished(store)
    check_records(recs2, keepers[1], s.gallery.names)
    assert groups == exact and len(groups) == n                            # the same fp16 rows, uploaded: the same records to the bit
    # group_visits normalises the fp32 copy again before it rounds to fp16: a unit row comes back as itself up to the last place, so the
    # verdicts and persons are the same and a similarity moves by at most two fp16 roundings of a unit vector's dot product (2 * 2^-11)
    assert [(g["verdict"], g["person_id"]) for g in groups] == [(g["verdict"], g["person_id"]) for g in want]
    assert all(abs(g["similarity"] - w["similarity"]) <= 2 ** -10 for g, w in zip(groups, want))
    assert len(store) == len([g for g in groups if g["verdict"] == "new"]) > 0
    assert pipes[1].finished() == []
    for p in pipes:
        p.close()


def test_best_shot_off_launches_nothing_new(ctx, scene):
    from scrfd_arcface_facerecognition_amd.pipeline import TrackedFacePipeline
    s = scene
    plain = TrackedFacePipeline(ctx, s.det, s.rec, batch=PB, row_cap=256, refresh=3, retry=1)
    off = TrackedFacePipeline(ctx, s.det, s.rec, batch=PB, row_cap=256, refresh=3, retry=1, best_shot=False)
    assert off.shots is None and not off.measure and not hasattr(off, "shot_score")
    for step in range(2):
        fr = ctx.to_device(s.frames[step * PB:(step + 1) * PB])
        plain.run_step(fr, H, W, s.gallery, THRESH)
        off.run_step(fr, H, W, s.gallery, THRESH)
        a, b = plain.results_tracked(s.gallery), off.results_tracked(s.gallery)
        assert len(a) == len(b) and all(len(x) == len(y) for x, y in zip(a, b))
        for x, y in zip(a, b):
            for fa, fb in zip(x, y):
                assert same(fa[0], fb[0]) and fa[1] == fb[1] and same(fa[2], fb[2]) and fa[3:] == fb[3:]
        assert all(same(u, v) for u, v in zip(plain.tracker_state(), off.tracker_state()))
    with pytest.raises(RuntimeError):
        off.finished()
    plain.close()
    off.close()


def test_stream_runner_finishes_at_the_end_of_the_video(ctx, scene):
    from scrfd_arcface_facerecognition_amd.pipeline import TrackedFacePipeline
    from scrfd_arcface_facerecognition_amd.video import StreamRunner
    s = scene
    pipe = TrackedFacePipeline(ctx, s.det, s.rec, batch=PB, row_cap=256, streams=2, refresh=3, retry=1, best_shot=True, keep_crops=False)
    runner = StreamRunner(pipe, s.gallery, (H, W), similarity_thresh=THRESH)
    cams = [1, 1, 0, 1, 1, 0]
    got = list(runner.run((c, f) for c, f in zip(cams, s.frames[:6])))
    assert len(got) == 6 and not (pipe.shots_state()[..., 1] != -1).any()  # run() ended with finish_all()
    recs = runner.finished()
    assert len(recs) > 0 and {r["stream"] for r in recs} <= {0, 1} and all(r["crop"] is None and r["rows"] >= 1 for r in recs)
    assert [r["stream"] for r in recs] == sorted(r["stream"] for r in recs)
    assert all(0 <= r["frame"] < (2 if r["stream"] == 0 else 4) for r in recs)
    runner.close()
    pipe.close()
