"""Shared by the coaster's tests: the tables of tracked walks in which tracks coast (tests/track_oracle.py's Tracker and random_walk, with
detections deleted by coast_oracle.thin), and the ctypes call of the host twin.  Not a test module."""
import ctypes as C
import functools

import numpy as np

import coast_oracle as O
from track_oracle import Tracker, draw_rows, random_walk
from scrfd_arcface_facerecognition_amd import _lib

TRACK_CFG = (0.3, 6, 16, 1)                                   # iou, max_age, refresh, retry
NAMES = ("det_out", "counts_out", "track_out", "idx_out", "score_out")


def ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def i32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32)) if a is not None else None


def config(hold=5, predict=True, grow=0.05):
    return _lib.CoastConfig(hold, predict, grow), O.Config(hold, predict, grow)


def out_arrays(B, cap, T, fill=0x5A):
    """the five outputs, filled with a byte pattern no rule writes"""
    cap2 = cap + T
    outs = [np.empty((B, cap2, 5), np.float32), np.empty(B, np.int32), np.empty((B, cap2, 2), np.int32), np.empty((B, cap2), np.int32),
            np.empty((B, cap2), np.float32)]
    for o in outs:
        o.view(np.uint8)[...] = fill
    return outs


def host(entries, stream, det, counts, track, ii, sc, cfg, outs=None, S=None, T=None, B=None, cap=None):
    """fid_track_coast_host -> (rc, outs); every array may be None (a NULL pointer)"""
    S = entries.shape[0] if S is None else S
    T = entries.shape[1] if T is None else T
    B = det.shape[0] if B is None else B
    cap = det.shape[1] if cap is None else cap
    if outs is None:
        outs = out_arrays(B, cap, T)
    rc = _lib.load().fid_track_coast_host(i32p(entries), S, T, i32p(stream), B, cap, ptr(det), ptr(counts), ptr(track), ptr(ii), ptr(sc),
                                          C.byref(cfg) if cfg is not None else None, *[ptr(o) for o in outs])
    return rc, outs


def same(got, want):
    """byte equality of two lists of arrays -> the names that differ"""
    return [n for n, g, w in zip(NAMES, got, want) if g.shape != w.shape or not np.array_equal(np.ascontiguousarray(g).view(np.uint8),
                                                                                                 np.ascontiguousarray(w).view(np.uint8))]


@functools.lru_cache(maxsize=None)
def walk_tables(seed, T, cap, S=3, B=12, calls=2, skip=True):
    """`calls` steps of a tracked walk: per step (stream, det, counts, track, ident_idx, ident_score).  Sub-pixel jitter makes the
    velocities and the growth inexact in fp32; every 7th frame is skipped (stream -1)."""
    rng = np.random.default_rng(900 + seed)
    n_rect, p = (3, 0.3) if cap < 64 else (80, 0.04)          # the wide walk keeps more than 64 detections in a frame
    trk = Tracker(S, T)
    steps = []
    for det, counts, stream in O.thin(random_walk(seed, calls=calls, B=B, cap=cap, S=S, n_rect=n_rect), seed, p=p):
        det = det.copy()
        for b in range(B):
            det[b, :counts[b], :4] += rng.random((int(counts[b]), 4), dtype=np.float32) * np.float32(0.75)
        stream = stream.copy()
        if skip:
            stream[3::7] = -1
        row_cap = B * cap
        track, offsets, src = trk.step(det, counts, stream, *TRACK_CFG, row_cap)
        idx, score = draw_rows(rng, row_cap)
        ii, sc = trk.identify(idx, score, min(int(offsets[-1]), row_cap))
        for a in (stream, det, counts, track, ii, sc):
            a.setflags(write=False)
        steps.append((stream, det, counts, track, ii, sc))
    return tuple(steps)
