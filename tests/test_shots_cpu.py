"""CPU: the best-shot keeper's binding, its score's host twin against the numpy restatement (bit for bit), and the invariants of the keeper's
rules on the tracker's random walks (tests/shot_oracle.py)."""
import ctypes as C

import numpy as np
import pytest

from shot_oracle import Keeper, Tracker, draw_rows, draw_scores, measure_rows, random_walk, row_payload, shot_score
from scrfd_arcface_facerecognition_amd import _lib


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def test_binding_names_and_meta_words():
    lib = _lib.load()
    for name in ("fid_shot_score", "fid_shot_score_host", "fid_shots_create", "fid_shots_destroy", "fid_track_keep", "fid_shots_flush",
                 "fid_shots_finished", "fid_shots_clear_finished", "fid_shots_read"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert _lib.SHOT_META_WORDS == 16
    header = open(__import__("os").path.join(__import__("conftest").ROOT, "include", "faceid.h")).read()
    assert "#define FID_SHOT_META_WORDS 16" in header


def host_score(stats, measure, cfg):
    lib = _lib.load()
    stats, measure = np.ascontiguousarray(stats, np.int64), np.ascontiguousarray(measure, np.float32)
    out = np.full(len(stats), 7.0, np.float32)
    rc = lib.fid_shot_score_host(stats.ctypes.data_as(C.c_void_p), measure.ctypes.data_as(C.c_void_p), len(stats), C.byref(cfg),
                                 out.ctypes.data_as(C.c_void_p))
    return rc, out


@pytest.mark.parametrize("norms", [(100.0, 40.0, 8.0), (37.5, 11.0, 3.25)])
def test_host_score_equals_the_oracle_to_the_bit(norms):
    stats, measure = measure_rows(3, norms=norms)
    cfg = _lib.MeasureConfig(*norms)
    rc, got = host_score(stats, measure, cfg)
    want = shot_score(stats, measure, *norms)
    assert rc == 0 and np.array_equal(bits(got), bits(want)), np.flatnonzero(bits(got) != bits(want))
    assert (want[(stats[:, 7] & 1) == 0] == -1).all() and (want[stats[:, 7] == 1] == 0).all()
    assert (want[np.isfinite(want)] <= 1).all() and (want[stats[:, 7] == 3] >= 0).sum() > 20


def test_score_seams():
    """at sharpness == n_s and contrast == n_c the min is exactly 1; at residual == n_r the pose term is exactly 0; clipped == 1 gives 0"""
    f = np.float32
    row = lambda **kw: [kw.get("sharp", 100.0), 128.0, kw.get("contrast", 40.0), kw.get("clipped", 0.0), 0, 0, kw.get("res", 0.0), 0]
    measure = np.array([row(), row(sharp=np.nextafter(f(100), f(0))), row(sharp=1e9), row(res=8.0), row(res=np.nextafter(f(8), f(0))),
                        row(res=9.0), row(clipped=1.0), row(contrast=20.0, res=4.0)], np.float32)
    stats = np.zeros((len(measure), 8), np.int64)
    stats[:, 7] = 3
    rc, got = host_score(stats, measure, _lib.MeasureConfig())
    assert rc == 0 and np.array_equal(bits(got), bits(shot_score(stats, measure)))
    assert got[0] == 1 and 0 < got[1] < 1 and got[2] == 1 and got[3] == 0 and 0 < got[4] < 1e-6 and got[5] == 0 and got[6] == 0
    assert got[7] == f(0.25)


def test_host_score_refusals():
    lib = _lib.load()
    stats, measure = measure_rows(1, n=4)
    out = np.full(len(stats), 7.0, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    cfg = _lib.MeasureConfig()
    assert lib.fid_shot_score_host(p(stats), p(measure), 0, C.byref(cfg), p(out)) == 0
    assert lib.fid_shot_score_host(None, p(measure), 4, C.byref(cfg), p(out)) == -1
    assert lib.fid_shot_score_host(p(stats), None, 4, C.byref(cfg), p(out)) == -1
    assert lib.fid_shot_score_host(p(stats), p(measure), 4, None, p(out)) == -1
    assert lib.fid_shot_score_host(p(stats), p(measure), 4, C.byref(cfg), None) == -1
    assert lib.fid_shot_score_host(p(stats), p(measure), -1, C.byref(cfg), p(out)) == -1
    for bad in (0.0, -1.0, np.nan, np.inf):
        for k in range(3):
            v = [100.0, 40.0, 8.0]
            v[k] = bad
            assert lib.fid_shot_score_host(p(stats), p(measure), 4, C.byref(_lib.MeasureConfig(*v)), p(out)) == -1, (bad, k)
            assert b"normalisation" in lib.fid_last_error()
    assert (out == 7.0).all()


def run_walk(seed, row_cap, finished_cap=512, T=4, cfg=(0.3, 1, 3, 2)):
    """the tracker's random walk through Tracker and Keeper -> (keeper, per (stream, id): the (call, row, score) of every row it had)"""
    rng = np.random.default_rng(500 + seed)
    trk, kp = Tracker(2, T), Keeper(2, T, 8, finished_cap)
    rows_of = {}
    for call, (det, counts, stream) in enumerate(random_walk(seed, calls=4)):
        cap = det.shape[1]
        track, offsets, src = trk.step(det, counts, stream, *cfg, row_cap)
        n = min(int(offsets[-1]), row_cap)
        idx, sc = draw_rows(rng, row_cap)
        ii, is_ = trk.identify(idx, sc, n)
        score = draw_scores(rng, row_cap)
        q, crops = row_payload(rng, row_cap, 8, call)
        for i in range(n):
            b, f = divmod(int(src[i]), cap)
            if track[b, f, 1] >= 0:
                rows_of.setdefault((int(stream[b]), int(track[b, f, 0])), []).append((call, i, score[i], q[i].copy(), crops[i].copy()))
        kp.keep(trk.id, stream, cap, track, offsets, src, row_cap, n, score, q, crops, det, ii, is_)
    kp.flush(-1)
    return kp, rows_of


@pytest.mark.parametrize("row_cap", [96, 5])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_oracle_invariants_on_random_walks(seed, row_cap):
    kp, rows_of = run_walk(seed, row_cap)
    assert kp.dropped == 0 and kp.count == len(kp.log) > 4 and not (kp.live_meta[..., 1] != -1).any()
    seen = set()
    for m, q, crop in zip(kp.fin_meta[:kp.count], kp.fin_q, kp.fin_crop):
        key = (int(m[0]), int(m[1]))
        assert key not in seen, f"track {key} finished twice"
        seen.add(key)
        rows = rows_of[key]
        assert m[6] == len(rows)                                   # rows = the track's row count
        cands = [r for r in rows if r[2] >= 0]
        best = max(r[2] for r in cands)
        first = next(r for r in cands if r[2] == best)             # the maximum of the candidates' scores, and the earliest such row
        assert m[4] == int(np.float32(best).view(np.int32)) and np.array_equal(q, first[3]) and np.array_equal(crop, first[4])
    for key, rows in rows_of.items():                              # a track finished iff it ever had a candidate
        assert (key in seen) == any(r[2] >= 0 for r in rows), key
    assert kp.frames.sum() == 4 * 12


def test_oracle_drops_beyond_the_finished_capacity():
    kp, _ = run_walk(1, 96, finished_cap=2)
    assert kp.count == 2 and kp.dropped == len(kp.log) - 2 > 0
    for k in range(2):
        assert np.array_equal(kp.fin_meta[k], kp.log[k][0]) and np.array_equal(kp.fin_crop[k], kp.log[k][2])
