"""GPU: fid_track_relink (csrc/relink.hip) against its host twin fid_track_relink_host, bit for bit -- the person table with guard words
behind it and the whole state through fid_relinker_read, q stores included --, behind a real fid_track_step + fid_track_identify; live
word 0 against fid_tracker_read; the refused calls; random unit rows against the oracle where its float64 scores show every decision to be
far from its threshold; and TrackedFacePipeline(relink=...) on a scene whose faces leave and return."""
import ctypes as C
import os

import numpy as np
import pytest

import draw_oracle as DO
import relink_oracle as O
from relink_calls import (DIMS, SHAPES, THRESH, TRACK_CFG, WALKS, WINDOW, config, differs, fresh, host, row_keys, rows_for, split_step,
                          walk_case, walk_inputs)

pytestmark = pytest.mark.gpu
GUARD = 0x5A5A5A5A
NG = 4                        # guard words behind the output
INVALID = -1
NEW = (1 << 8) | (1 << 9)


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


class Device:
    """a fid_tracker and a fid_relinker of one shape and the buffers of one step; the person table carries NG guard words"""

    def __init__(self, ctx, S, T, L, dim, max_age=1):
        from scrfd_arcface_facerecognition_amd._lib import TrackConfig, check
        self.ctx, self.S, self.T, self.L, self.dim, self.check = ctx, S, T, L, dim, check
        self.tcfg = TrackConfig(TRACK_CFG[0], max_age, TRACK_CFG[1], TRACK_CFG[2])
        self.trk, self.rl = C.c_void_p(), C.c_void_p()
        check(ctx.lib.fid_tracker_create(ctx.handle, S, T, C.byref(self.trk)))
        check(ctx.lib.fid_relinker_create(ctx.handle, S, T, L, dim, C.byref(self.rl)))

    def step(self, det, counts, stream, identify=True):
        """fid_track_step and fid_track_identify (no row has a name) -> the step's host tables (stream, counts, track, offsets, src)"""
        B, cap = det.shape[:2]
        lib, h = self.ctx.lib, self.ctx.handle
        self.B, self.cap, self.row_cap = B, cap, B * cap
        self.stream = np.ascontiguousarray(stream, np.int32)
        self.h_counts = np.ascontiguousarray(counts, np.int32)
        self.det, self.counts = self.ctx.to_device(np.ascontiguousarray(det, np.float32)), self.ctx.to_device(self.h_counts)
        self.track, self.offsets, self.src = (self.ctx.empty((B, cap, 2), np.int32), self.ctx.empty((B + 1,), np.int32),
                                              self.ctx.empty((self.row_cap,), np.int32))
        self.check(lib.fid_track_step(h, self.trk, C.c_void_p(self.det.ptr), C.c_void_p(self.counts.ptr), _i32(self.stream), B, cap,
                                      C.byref(self.tcfg), C.c_void_p(self.track.ptr), C.c_void_p(self.offsets.ptr), C.c_void_p(self.src.ptr),
                                      self.row_cap))
        if identify:
            self.identify()
        return self.stream, self.h_counts, self.track.download(), self.offsets.download(), self.src.download()

    def identify(self):
        B, cap = self.B, self.cap
        self.ii, self.sc = self.ctx.empty((B, cap), np.int32), self.ctx.empty((B, cap), np.float32)
        self.check(self.ctx.lib.fid_track_identify(self.ctx.handle, self.trk, C.c_void_p(self.counts.ptr), _i32(self.stream), B, cap,
                                                   C.c_void_p(self.track.ptr), C.c_void_p(self.offsets.ptr), C.c_void_p(self.src.ptr),
                                                   self.row_cap, None, None, 0, C.c_void_p(self.ii.ptr), C.c_void_p(self.sc.ptr)))

    def new_output(self):
        self.person = self.ctx.to_device(np.full(self.B * self.cap * 2 + NG, GUARD, np.int32))

    def relink(self, rows, config, expect=0, fresh_out=True, **override):
        """fid_track_relink on the unit rows -> the person table as the host sees it (guards checked); override: arguments to replace"""
        q, cfg = rows, config
        if fresh_out:
            self.new_output()
        self.q = self.ctx.to_device(np.ascontiguousarray(q, np.float16) if len(q) else np.zeros((1, self.dim), np.float16))
        a = dict(rl=self.rl, stream=self.stream, B=self.B, cap=self.cap, counts=C.c_void_p(self.counts.ptr), track=C.c_void_p(self.track.ptr),
                 offsets=C.c_void_p(self.offsets.ptr), src=C.c_void_p(self.src.ptr), row_cap=self.row_cap, n_rows=len(q),
                 q=C.c_void_p(self.q.ptr), cfg_ptr=C.byref(cfg) if cfg is not None else None, person=C.c_void_p(self.person.ptr))
        a.update(override)
        rc = self.ctx.lib.fid_track_relink(self.ctx.handle, a["rl"], self.trk, _i32(a["stream"]), a["B"], a["cap"], a["counts"], a["track"],
                                           a["offsets"], a["src"], a["row_cap"], a["n_rows"], a["q"], a["cfg_ptr"], a["person"])
        assert rc == expect, (rc, expect)
        return self.read_output()

    def read_output(self):
        raw = self.person.download()
        n = self.B * self.cap * 2
        assert (raw[n:] == GUARD).all(), "guard words behind the person table were written"
        return raw[:n].reshape(self.B, self.cap, 2)

    def state(self):
        S, T, L, dim = self.S, self.T, self.L, self.dim
        st = [np.empty((S, T, 8), np.int32), np.empty((S, L, 8), np.int32), np.empty(S, np.int32), np.empty((S, T, dim), np.float16),
              np.empty((S, L, dim), np.float16)]
        self.check(self.ctx.lib.fid_relinker_read(self.ctx.handle, self.rl, _i32(st[0]), _i32(st[1]), _i32(st[2]),
                                                  st[3].ctypes.data_as(C.c_void_p), st[4].ctypes.data_as(C.c_void_p)))
        return st

    def slot_ids(self):
        slots, per = np.empty((self.S, self.T, 10), np.int32), np.empty((self.S, 2), np.int32)
        self.check(self.ctx.lib.fid_tracker_read(self.ctx.handle, self.trk, _i32(slots), _i32(per)))
        return slots[..., 0]

    def close(self):
        self.check(self.ctx.lib.fid_relinker_destroy(self.ctx.handle, self.rl))
        self.check(self.ctx.lib.fid_tracker_destroy(self.ctx.handle, self.trk))


def run_against_the_twin(ctx, S, T, L, dim, inputs, cfg, parts=1):
    """every step on the device and through the host twin on the device tracker's own tables -> (device, twin's state, persons per step).
    parts > 1: the twin takes the step in `parts` calls of B / parts frames (the device always in one)."""
    dev = Device(ctx, S, T, L, dim, cfg.max_age)
    state = fresh(S, T, L, dim)
    assert not differs(dev.state(), state)
    persons = []
    for det, counts, stream in inputs:
        tabs = dev.step(det, counts, stream)
        n_rows = min(int(tabs[3][-1]), dev.row_cap)
        keys = row_keys(det, stream, tabs[4], n_rows, dev.cap)
        q = rows_for(keys, dim)
        got = dev.relink(q, cfg)
        want = []
        for sub in split_step(tabs + (q,), parts) if parts > 1 else [tabs + (q,)]:
            rc, p = host(state, sub, cfg)
            assert rc == 0
            want.append(p)
        want = np.concatenate(want)
        assert np.array_equal(got, want), np.argwhere(got != want)[:6]
        now = dev.state()
        assert not differs(now, state), differs(now, state)
        assert np.array_equal(now[0][..., 0], dev.slot_ids())          # steps 1 and 4 mirror the tracker's slot life
        persons.append(want)
    return dev, state, persons


# ---- 1. the device against the host twin ----
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("T, cap, L", SHAPES)
def test_walks_equal_the_host_twin(ctx, T, cap, L, dim):
    """the walks of the CPU tests (the oracle has shown them to hold links, a chain and an overwrite of a full pool), tracked by the device"""
    _, want, _ = walk_case(T, cap, L, dim)
    dev, state, persons = run_against_the_twin(ctx, WALKS[(T, cap)][1], T, L, dim, walk_inputs(T, cap), config())
    assert all(np.array_equal(p, w[0]) for p, w in zip(persons, want))                   # the device tracker's tables are the oracle's
    assert not differs(state, want[-1][1])
    dev.close()


def test_one_call_equals_frame_by_frame_calls(ctx):
    T, cap, L = 5, 3, 4
    B = WALKS[(T, cap)][2]
    for parts in (B, 3):
        run_against_the_twin(ctx, 2, T, L, 40, walk_inputs(T, cap), config(), parts=parts)[0].close()


def grid_det(B, cap, n, present):
    det, counts = np.zeros((B, cap, 5), np.float32), np.zeros(B, np.int32)
    for b in range(B):
        if present[b]:
            for i in range(n):
                x, y = 40.0 * (i % 10), 40.0 * (i // 10)
                det[b, i] = (x, y, x + 20 + i, y + 22, 1.0 - 0.01 * i)       # (every box has its own width: its own row)
            counts[b] = n
    return det, counts


def test_all_64_slots_retire_in_one_frame_and_64_tracks_link_in_one(ctx):
    B, cap = 6, 70
    det, counts = grid_det(B, cap, 64, [1, 0, 0, 1, 1, 0])
    dev, state, persons = run_against_the_twin(ctx, 1, 64, 64, 64, [(det, counts, np.zeros(B, np.int32))], config(0.75, 10, 1))
    p = persons[0]
    assert np.array_equal(p[3, :64, 0], np.arange(64)) and (p[3, :64, 1] & (1 << 11)).all() and (p[0, :64, 1] & (1 << 11) == 0).all()
    assert np.array_equal(p[4, :64, 0], np.arange(64)) and np.array_equal(state[0][0, :, 6], np.arange(64))
    assert (state[1][0, :, 0] == -1).all() and (state[0][0, :, 0] >= 64).all()
    dev.close()


def test_a_pool_of_one(ctx):
    B, cap = 12, 3
    det, counts = grid_det(B, cap, 2, [1, 0, 0, 1, 0, 0, 1, 1, 0, 0, 1, 1])
    dev, state, persons = run_against_the_twin(ctx, 1, 4, 1, 8, [(det, counts, np.zeros(B, np.int32))], config(0.75, 100, 1))
    p = persons[0]
    # both tracks retire in frame 2, slots ascending: track 1 overwrites track 0 in the pool, so only the second rectangle is known again
    assert [tuple(v) for v in p[3, :2]] == [(2, 0 | NEW), (1, 1 | NEW | (1 << 11))]
    assert [tuple(v) for v in p[6, :2]] == [(4, 0 | NEW), (1, 1 | NEW | (1 << 11))] and tuple(p[11, 1]) == (1, 1 | (1 << 9) | (1 << 11))
    dev.close()


def test_reset_of_one_stream_and_of_all(ctx):
    B, cap = 4, 4
    det, counts = grid_det(B, cap, 3, [1, 1, 1, 1])
    dev, state, _ = run_against_the_twin(ctx, 2, 5, 3, 16, [(det, counts, np.array([0, 1, 0, 1], np.int32))], config())
    assert (state[0][:, :3, 0] >= 0).all() and (state[3] != 0).any()
    dev.check(ctx.lib.fid_relinker_reset(ctx.handle, dev.rl, 1))
    after, blank = dev.state(), fresh(2, 5, 3, 16)
    assert all(np.array_equal(a[0], s[0]) and np.array_equal(a[1], f[1]) for a, s, f in zip(after, state, blank))
    assert ctx.lib.fid_relinker_reset(ctx.handle, dev.rl, 2) == INVALID and ctx.lib.fid_relinker_reset(ctx.handle, dev.rl, -2) == INVALID
    dev.check(ctx.lib.fid_relinker_reset(ctx.handle, dev.rl, -1))
    assert not differs(dev.state(), blank)
    dev.close()


# ---- 2. refusals ----
def test_refusals_leave_outputs_and_state_untouched(ctx):
    B, cap, dim = 4, 4, 16
    det, counts = grid_det(B, cap, 3, [1, 0, 1, 0])
    stream = np.zeros(B, np.int32)
    dev = Device(ctx, 1, 5, 3, dim)
    tabs = dev.step(det, counts, stream, identify=False)
    q = rows_for(row_keys(det, stream, tabs[4], min(int(tabs[3][-1]), dev.row_cap), cap), dim)
    dev.new_output()
    blank = fresh(1, 5, 3, dim)

    def untouched(state):
        assert (dev.person.download() == GUARD).all()
        assert not differs(dev.state(), state)

    dev.relink(q, config(), expect=INVALID, fresh_out=False)                   # the step still waits for its identify
    untouched(blank)
    dev.identify()
    nan, inf = float("nan"), float("inf")
    other = Device(ctx, 1, 6, 3, dim)                                          # a relinker of another shape than the tracker
    cases = [dict(B=B - 1), dict(cap=cap + 1), dict(row_cap=dev.row_cap - 1), dict(stream=np.array([0, 0, -1, 0], np.int32)), dict(n_rows=-1),
             dict(n_rows=dev.row_cap + 1), dict(cfg_ptr=None), dict(rl=other.rl)]
    cases += [dict(cfg_ptr=C.byref(config(*c))) for c in ((1.0, 10, 1), (-0.01, 10, 1), (nan, 10, 1), (inf, 10, 1), (0.5, -1, 1), (0.5, 10, -1))]
    cases += [{name: None} for name in ("rl", "counts", "track", "offsets", "src", "q", "person")]
    for kw in cases:
        dev.relink(q, config(), expect=INVALID, fresh_out=False, **kw)
        untouched(blank)
    assert not differs(other.state(), fresh(1, 6, 3, dim))
    other.close()
    for shape in ((0, 5, 3, 16), (1, 0, 3, 16), (1, 65, 3, 16), (1, 5, 0, 16), (1, 5, 65, 16), (1, 5, 3, 0), (1, 5, 3, 12), (1, 5, 3, 4)):
        h = C.c_void_p()
        assert ctx.lib.fid_relinker_create(ctx.handle, *shape, C.byref(h)) == INVALID and not h.value, shape
    got = dev.relink(q, config(), fresh_out=False)                             # the valid call goes through ...
    state = fresh(1, 5, 3, dim)
    rc, want = host(state, tabs + (q,), config())
    assert rc == 0 and np.array_equal(got, want) and not differs(dev.state(), state)
    dev.new_output()
    dev.relink(q, config(), expect=INVALID, fresh_out=False)                   # ... once per step
    untouched(state)
    dev.close()


# ---- 3. random unit rows ----
def test_random_rows_equal_the_oracle_where_it_is_sure(ctx):
    """dim 512, random unit fp16 rows (a returning rectangle's row is its earlier row plus noise).  The oracle's float64 scores must show
    every score further than 2^-10 from thresh and every attempt's best further than 2^-10 from its second best -- far above the fp32
    summation bound 512 * 2^-24 --; then persons and every integer state word but the link score's bits must be the oracle's."""
    T, cap, L, dim = 5, 3, 4, 512
    S = WALKS[(T, cap)][1]
    inputs = walk_inputs(T, cap)
    margin = 2.0 ** -10
    for seed in range(20):
        base = {}

        def rows(keys, rng=np.random.default_rng(seed)):
            out = np.zeros((len(keys), dim), np.float64)
            for i, k in enumerate(keys):
                if k not in base:
                    base[k] = rng.standard_normal(dim)
                out[i] = base[k] + 0.6 * rng.standard_normal(dim)
            return (out / np.sqrt((out ** 2).sum(1, keepdims=True))).astype(np.float16) if len(keys) else np.zeros((0, dim), np.float16)

        dev = Device(ctx, S, T, L, dim)
        ref = O.Relinker(S, T, L, dim)
        steps = []
        for det, counts, stream in inputs:
            tabs = dev.step(det, counts, stream)
            q = rows(row_keys(det, stream, tabs[4], min(int(tabs[3][-1]), dev.row_cap), cap))
            want = ref.step(*tabs, dev.row_cap, len(q), q, 0.45, WINDOW, 1)
            steps.append((q, want, ref.state()))
        sure = all(min(abs(s - t) for s in sc) > margin and (len(sc) < 2 or sorted(sc)[-1] - sorted(sc)[-2] > margin) for t, sc in ref.attempts)
        if not sure:
            dev.close()
            continue
        assert sure and len(ref.links) >= 4 and len(ref.attempts) > len(ref.links)      # links and refusals both occur
        dev.close()
        dev = Device(ctx, S, T, L, dim)
        for (det, counts, stream), (q, want, state) in zip(inputs, steps):
            dev.step(det, counts, stream)
            got = dev.relink(q, config(0.45, WINDOW, 1))
            assert np.array_equal(got, want)
            now = dev.state()
            now[0][..., 3] = state[0][..., 3] = 0                                        # (the link score's bits are not compared here)
            assert not differs(now, state), differs(now, state)
        dev.close()
        return
    pytest.fail("no seed gave the oracle its margins")


# ---- 4. the pipeline ----
PH = PW = 320
PB = 4


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
    s.blank = np.full((PH, PW, 3), 85, np.uint8)                   # (at this calibration the detector finds nothing in it)
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


def make_pipe(ctx, s, **kw):
    from scrfd_arcface_facerecognition_amd.pipeline import TrackedFacePipeline
    return TrackedFacePipeline(ctx, s.det, s.rec, batch=PB, row_cap=256, refresh=1000, retry=1, max_tracks=64, max_age=1, **kw)


def test_pipeline_without_a_relinker_is_unchanged(ctx, scene):
    """relink=None: byte-identical track / ident / results_tracked() to a pipe built without the argument, and nothing is allocated"""
    s = scene
    a, b = make_pipe(ctx, s), make_pipe(ctx, s, relink=None)
    assert b.relinker is None and not hasattr(b, "person")
    with pytest.raises(RuntimeError):
        b.results_persons()
    with pytest.raises(RuntimeError):
        b.relinker_state()
    with pytest.raises(TypeError):
        make_pipe(ctx, s, relink=True)
    outs = []
    for pipe in (a, b):
        for frames in (s.frames, np.stack([s.blank] * 3 + [s.frames[3]])):
            pipe.run_step(ctx.to_device(frames), PH, PW, s.gallery, -1.0)
            outs.append((pipe.track.download(), pipe.ident_idx.download(), pipe.ident_score.download(), repr(pipe.results_tracked(s.gallery))))
    for x, y in zip(outs[:2], outs[2:]):
        assert all(np.array_equal(u.view(np.uint8), v.view(np.uint8)) for u, v in zip(x[:3], y[:3])) and x[3] == y[3]
    assert (outs[0][0][..., 0] >= 0).any()
    a.close()
    b.close()


def test_pipeline_gives_returning_faces_their_person_ids(ctx, scene, glyphs):
    """max_age = 1: the scene's frames, then three blank frames -- every track ends --, then the last frame again: identical crops, so every
    new track's first embedding is a pooled track's own (score 1.0 up to the fp16 rounding of the unit rows).  results_tracked() shows new
    track ids, results_persons() the old ones with `relinked` set, and the overlay prints the old number"""
    from scrfd_arcface_facerecognition_amd._lib import DRAW_TRACK_ID, DrawStyle, RelinkConfig
    s = scene
    rcfg = RelinkConfig(thresh=0.45, window=300, pool=32)
    pipe = make_pipe(ctx, s, relink=rcfg)
    cap = pipe.post.cap
    ref = O.Relinker(1, 64, 32, 512)

    def step(frames):
        pipe.run_step(ctx.to_device(frames), PH, PW, None)
        stream, counts, track = np.zeros(PB, np.int32), pipe.post.counts.download(), pipe.track.download()
        offsets, src = pipe.offsets.download(), pipe.src.download()
        n = min(pipe.n_run, pipe.row_cap)
        want = ref.step(stream, counts, track, offsets, src, pipe.row_cap, n, pipe.q.download()[:n], 0.45, 300, 1)
        return pipe.results_persons(), want

    first, want1 = step(s.frames)
    assert np.array_equal(pipe.person.download(), want1)
    old = {tuple(np.round(f[0], 3)): f[5] for f in first[3] if f[5] >= 0}     # box -> track id in the last frame
    assert len(old) >= 2 and all(f[7] == f[5] and not f[8] for fr in first for f in fr)
    frames2 = np.stack([s.blank] * 3 + [s.frames[3]])
    second, want2 = step(frames2)
    assert np.array_equal(pipe.person.download(), want2)
    st, want_state = pipe.relinker_state(), ref.state()
    assert (st["live"][..., 3] != 0).sum() == len(old)
    st["live"][..., 3] = want_state[0][..., 3] = 0            # (the device sums in another order: the link score's bits may differ)
    assert not differs([st[k] for k in ("live", "pool", "frames")], want_state[:3]) and st["frames"][0] == 2 * PB
    assert [len(fr) for fr in second[:3]] == [0, 0, 0] and len(second[3]) == len(first[3])
    print("link scores:", sorted(round(l[5], 4) for l in ref.links), "attempts:", [sorted(np.round(sc, 3))[-2:] for _, sc in ref.attempts])
    linked = 0
    for f in second[3]:
        key = tuple(np.round(f[0], 3))
        if f[5] < 0:
            continue
        assert f[6] and f[5] not in old.values()                               # a new track with a new id ...
        assert key in old and f[7] == old[key] and f[8], (f[5], f[7], old.get(key))      # ... and the person it was before
        linked += 1
    assert linked == len(old)
    assert repr([[f[:7] for f in fr] for fr in second]) == repr(pipe.results_tracked())
    # the overlay prints the person id: the draw oracle fed the person table
    dstyle, ostyle = DrawStyle(0.3, 3, 1, 1, DRAW_TRACK_ID, (0, 0, 255)), DO.Style(0.3, 3, 1, 1, DRAW_TRACK_ID, (0, 0, 255))
    out = pipe.draw(ctx.to_device(frames2), PH, PW, None, dstyle).download()
    det, counts = pipe.post.det.download(), pipe.post.counts.download()
    ii, sc = pipe.ident_idx.download(), pipe.ident_score.download()
    by_person = DO.draw(frames2, det, counts, cap, glyphs, idx=ii, score=sc, id_stride=cap, track=want2, names=None, style=ostyle)
    by_track = DO.draw(frames2, det, counts, cap, glyphs, idx=ii, score=sc, id_stride=cap, track=pipe.track.download(), names=None, style=ostyle)
    assert np.array_equal(out, by_person) and not np.array_equal(by_person, by_track)
    pipe.reset()
    assert not differs([pipe.relinker_state()[k] for k in ("live", "pool", "frames", "live_q", "pool_q")], fresh(1, 64, 32, 512))
    pipe.close()
