"""Shared by the relinker's tests: tracked walks in which rectangles leave for longer than max_age and return (tests/track_oracle.py's Tracker
and random_walk, with gaps cut in), one exact unit row per rectangle, and the ctypes call of the host twin.  Not a test module."""
import ctypes as C
import functools

import numpy as np

import relink_oracle as O
from track_oracle import Tracker, random_walk
from scrfd_arcface_facerecognition_amd import _lib

SHAPES = [(1, 3, 1), (5, 3, 4), (64, 3, 64), (64, 70, 32)]    # (T, cap, L)
DIMS = (8, 40, 512)
STATE = ("live", "pool", "frames", "live_q", "pool_q")
THRESH, WINDOW = 0.75, 1000
# (T, cap) -> seed, S, B, calls, rectangles per stream, chance per frame that a rectangle leaves: tried on the oracle alone until every case
# had its links, a chain and an overwrite of a full pool (walk_case asserts it)
WALKS = {(1, 3): (2, 2, 12, 12, 1, 0.2), (5, 3): (1, 2, 12, 6, 3, 0.12), (64, 3): (1, 2, 12, 40, 3, 0.12), (64, 70): (1, 3, 9, 4, 80, 0.15)}


def ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def i32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32)) if a is not None else None


def config(thresh=THRESH, window=WINDOW, max_age=1):
    return _lib.RelinkConfigC(thresh, window, max_age)


def exact_row(key, dim):
    """a unit row with 4 non-zeros (+-0.5) or, where dim allows, 16 (+-0.25), deterministic in `key`: every score among such rows is a
    multiple of 1/64 in any summation order"""
    rng = np.random.default_rng([7, *[int(v) & 0xFFFFFFFF for v in key]])
    nnz = 16 if dim >= 16 and rng.random() < 0.5 else 4
    row = np.zeros(dim, np.float16)
    row[rng.choice(dim, nnz, replace=False)] = rng.choice([-1.0, 1.0], nnz) / np.sqrt(nnz)
    return row


def fresh(S, T, L, dim):
    """the state arrays of a new relinker: live, pool, frames, live_q, pool_q"""
    return O.Relinker(S, T, L, dim).state()


def person_out(B, cap, fill=0x5A):
    out = np.empty((B, cap, 2), np.int32)
    out.view(np.uint8)[...] = fill
    return out


def host(state, step, cfg, person=None, dim=None, n_rows=None):
    """fid_track_relink_host on the state arrays (updated in place) -> (rc, person)"""
    live, pool, frames, live_q, pool_q = state
    stream, counts, track, offsets, src, q = step
    S, T = live.shape[:2]
    B, cap = track.shape[:2]
    if person is None:
        person = person_out(B, cap)
    rc = _lib.load().fid_track_relink_host(i32p(live), ptr(live_q), i32p(pool), ptr(pool_q), i32p(frames), S, T, pool.shape[1],
                                           live_q.shape[2] if dim is None else dim, i32p(stream), B, cap, ptr(counts), ptr(track), ptr(offsets),
                                           ptr(src), len(src), len(q) if n_rows is None else n_rows, ptr(q),
                                           C.byref(cfg) if cfg is not None else None, ptr(person))
    return rc, person


def differs(got, want):
    """byte equality of two states -> the names that differ"""
    return [n for n, g, w in zip(STATE, got, want) if g.shape != w.shape or not np.array_equal(np.ascontiguousarray(g).view(np.uint8),
                                                                                                np.ascontiguousarray(w).view(np.uint8))]


def cut_gaps(walk, seed, S, gap, p):
    """every rectangle (a stream's boxes of one size) now and then leaves for `gap` frames of its stream"""
    rng = np.random.default_rng(4000 + seed)
    left = {}
    out = []
    for det, counts, stream in walk:
        det, counts = det.copy(), counts.copy()
        for b in range(len(counts)):
            s = int(stream[b])
            keep = []
            gone_now = set()
            for f in range(int(counts[b])):
                x1, y1, x2, y2 = det[b, f, :4]
                key = (s, int(x2 - x1), int(y2 - y1))
                if key not in gone_now and left.get(key, 0) == 0 and rng.random() < p:
                    left[key] = gap
                if left.get(key, 0) > 0:
                    gone_now.add(key)
                else:
                    keep.append(f)
            for key in gone_now:
                left[key] -= 1
            rows = det[b, keep].copy()
            det[b] = 0
            det[b, :len(keep)] = rows
            counts[b] = len(keep)
        out.append((det, counts, stream))
    return out


TRACK_CFG = (0.3, 4, 1)                                       # iou, refresh, retry (max_age comes with the case)


def row_keys(det, stream, src, n_rows, cap):
    """the rectangle (stream, width, height) behind every row of a step's table"""
    keys = []
    for i in range(n_rows):
        b, f = divmod(int(src[i]), cap)
        x1, y1, x2, y2 = det[b, f, :4]
        keys.append((int(stream[b]), int(x2 - x1), int(y2 - y1)))
    return keys


def rows_for(keys, dim):
    return np.stack([exact_row(k, dim) for k in keys]) if len(keys) else np.zeros((0, dim), np.float16)


@functools.lru_cache(maxsize=None)
def walk_inputs(T, cap, max_age=1):
    """the detections of a walk with returning rectangles: per step (det, counts, stream); every 7th frame is skipped (stream -1)"""
    seed, S, B, calls, n_rect, p_gap = WALKS[(T, cap)]
    out = []
    for det, counts, stream in cut_gaps(random_walk(seed, calls=calls, B=B, cap=cap, S=S, n_rect=n_rect), seed, S, max_age + 2, p_gap):
        stream = stream.copy()
        stream[3::7] = -1
        for a in (det, counts, stream):
            a.setflags(write=False)
        out.append((det, counts, stream))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def walk_tables(T, cap, max_age=1):
    """The steps of the walk through the tracker's oracle, without embeddings: per step (stream, counts, track, offsets, src, key per row,
    tracker slot ids after the step).  A row's key names its rectangle."""
    S, B = WALKS[(T, cap)][1:3]
    trk = Tracker(S, T)
    steps = []
    for det, counts, stream in walk_inputs(T, cap, max_age):
        row_cap = B * cap
        track, offsets, src = trk.step(det, counts, stream, TRACK_CFG[0], max_age, TRACK_CFG[1], TRACK_CFG[2], row_cap)
        n_rows = min(int(offsets[-1]), row_cap)
        trk.identify(np.full(row_cap, -1, np.int32), np.zeros(row_cap, np.float32), n_rows)
        keys = row_keys(det, stream, src, n_rows, cap)
        for a in (track, offsets, src):
            a.setflags(write=False)
        steps.append((stream, counts, track, offsets, src, tuple(keys), trk.id.copy()))
    return tuple(steps)


@functools.lru_cache(maxsize=None)
def walk_case(T, cap, L, dim, max_age=1):
    """-> (steps (stream, counts, track, offsets, src, q), per step the oracle's (person, state), tracker ids per step).  The oracle must
    show that the case is not vacuous: links, a chain of two links that keeps the first id, an overwrite of a full pool."""
    tables = walk_tables(T, cap, max_age)
    S = WALKS[(T, cap)][1]
    ref = O.Relinker(S, T, L, dim)
    steps, want, ids = [], [], []
    for stream, counts, track, offsets, src, keys, slot_ids in tables:
        q = rows_for(keys, dim)
        q.setflags(write=False)
        person = ref.step(stream, counts, track, offsets, src, len(src), len(q), q, THRESH, WINDOW, max_age)
        steps.append((stream, counts, track, offsets, src, q))
        want.append((person, ref.state()))
        ids.append(slot_ids)
        assert np.array_equal(ref.live[..., 0], slot_ids)        # steps 1 and 4 mirror the tracker's slot life
    assert len(ref.links) >= 4 and len(ref.chains()) >= 1 and ref.overwrites >= 1, (len(ref.links), len(ref.chains()), ref.overwrites)
    return tuple(steps), tuple(want), tuple(ids)


def split_step(step, parts):
    """one step of B frames as `parts` steps of B / parts frames (row_cap = the frames' rows: it cuts no row)"""
    stream, counts, track, offsets, src, q = step
    B = len(stream)
    assert B % parts == 0
    n = B // parts
    cap = track.shape[1]
    out = []
    for c in range(parts):
        lo, hi = int(offsets[c * n]), int(offsets[(c + 1) * n])
        sub_src = np.full(max(hi - lo, 1), -1, np.int32)
        sub_src[:hi - lo] = src[lo:hi] - c * n * cap
        out.append((np.ascontiguousarray(stream[c * n:(c + 1) * n]), np.ascontiguousarray(counts[c * n:(c + 1) * n]),
                    np.ascontiguousarray(track[c * n:(c + 1) * n]), np.ascontiguousarray(offsets[c * n:(c + 1) * n + 1] - lo), sub_src,
                    np.ascontiguousarray(q[lo:hi])))
    return out
