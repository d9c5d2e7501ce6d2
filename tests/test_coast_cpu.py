"""CPU: fid_track_coast_host (csrc/coast_core.h through the library) against tests/coast_oracle.py, bit for bit: the state and all five
outputs, fillers included.  The inputs are tracked walks (tests/track_oracle.py, unmodified) with detections deleted so that tracks coast;
the pinned cases are tables written by hand.  No device involved."""
import numpy as np
import pytest

import coast_oracle as O
from coast_calls import config, host, out_arrays, same, walk_tables
from scrfd_arcface_facerecognition_amd import _lib
from scrfd_arcface_facerecognition_amd.utils.helpers import coast_tracks

QNAN = 0x7FC00000
SHAPES = [(1, 3), (5, 3), (64, 3), (5, 70), (64, 70)]                      # (T, cap)
CONFIGS = [(h, p, g) for h in (0, 1, 4) for p in (False, True) for g in (0.0, 0.05, 0.5)]
# coasted rows at hold = 4 per (T, cap): floors the ORACLE alone reaches on every seed below (chosen on the CPU, before any kernel ran)
MIN_COASTED = {(1, 3): 8, (5, 3): 30, (64, 3): 30, (5, 70): 20, (64, 70): 300}


def run_both(steps, T, cfg_c, cfg_o, S=3):
    """both sides over consecutive calls -> the oracle's outputs per call, after asserting equality"""
    e_host, e_ref = O.fresh(S, T), O.fresh(S, T)
    all_ref = []
    for call, (stream, det, counts, track, ii, sc) in enumerate(steps):
        rc, got = host(e_host, stream, det, counts, track, ii, sc, cfg_c)
        assert rc == 0
        want = O.coast(e_ref, stream, det, counts, track, ii, sc, cfg_o)
        assert not same(got, want), (call, same(got, want))
        assert np.array_equal(e_host, e_ref), (call, np.argwhere(e_host != e_ref)[:6])
        all_ref.append(want)
    return all_ref, e_ref


# (one seed of the wide walks: the oracle tracker is slow on 60 rectangles)
@pytest.mark.parametrize("seed, T, cap", [(seed, T, cap) for T, cap in SHAPES for seed in ((1, 2, 3) if cap == 3 else (1,))])
def test_random_walks_match_the_oracle(seed, T, cap):
    steps = walk_tables(seed, T, cap)
    assert any((s < 0).any() for s, *_ in steps) and all(len(set(s[s >= 0])) == 3 for s, *_ in steps)      # 3 streams, skipped frames
    if cap == 70:
        assert max(int(c.max()) for _, _, c, *_ in steps) > 64                                               # a ragged second load of 64
    for hold, predict, grow in CONFIGS:
        cfg_c, cfg_o = config(hold, predict, grow)
        ref, state = run_both(steps, T, cfg_c, cfg_o)
        n = sum(len(rows) for outs in ref for rows in O.coasted(outs, T))
        if hold == 0:
            assert n == 0
        if hold == 4:
            assert n >= MIN_COASTED[T, cap], (n, T, cap, seed)
            if cap == 3:
                assert (state[..., 1] > 4).any() or T == 1                 # entries past hold are still remembered
            if predict and cap == 3:
                assert any(len(rows) and max(r[3] for r in rows) >= 2 for outs in ref for rows in O.coasted(outs, T))


def test_identity_arrays_may_be_absent():
    steps = walk_tables(1, 5, 3)
    cfg_c, cfg_o = config(4, True, 0.05)
    e_host, e_ref = O.fresh(3, 5), O.fresh(3, 5)
    for stream, det, counts, track, _, _ in steps:
        rc, got = host(e_host, stream, det, counts, track, None, None, cfg_c)
        want = O.coast(e_ref, stream, det, counts, track, None, None, cfg_o)
        assert rc == 0 and not same(got, want) and np.array_equal(e_host, e_ref)
        assert (got[3] == -1).all() and (got[4].view(np.int32) == 0).all()


def test_the_helper_wraps_the_twin():
    stream, det, counts, track, ii, sc = walk_tables(2, 5, 3)[0]
    e1, e2 = O.fresh(3, 5), O.fresh(3, 5)
    got = coast_tracks(e1, stream, det, counts, track, ii, sc, _lib.CoastConfig(4, True, 0.05))
    want = O.coast(e2, stream, det, counts, track, ii, sc, O.Config(4, True, 0.05))
    assert not same(got, want) and np.array_equal(e1, e2)
    d = _lib.CoastConfig()
    assert (d.hold, d.predict, d.reserved) == (5, 1, 0) and np.float32(d.grow) == np.float32(0.05)
    assert _lib.TRACK_COASTED == O.COASTED == 1 << 10 and _lib.COAST_WORDS == O.WORDS == 16


# ---- pinned cases: one stream, tables by hand ------------------------------------------------------------------------------------------

def frames(rows, cap=2):
    """rows: per frame a list of (id, word, box[4], conf) -> stream, det, counts, track, ii, sc"""
    B = len(rows)
    det, track = np.zeros((B, cap, 5), np.float32), np.full((B, cap, 2), -1, np.int32)
    counts = np.array([len(r) for r in rows], np.int32)
    ii, sc = np.full((B, cap), -1, np.int32), np.zeros((B, cap), np.float32)
    for b, r in enumerate(rows):
        for f, (tid, word, box, conf) in enumerate(r):
            det[b, f, :4], det[b, f, 4], track[b, f] = box, conf, (tid, word)
            ii[b, f], sc[b, f] = tid % 3, 0.5 + 0.01 * tid
    return np.zeros(B, np.int32), det, counts, track, ii, sc


def both(tabs, T, hold=4, predict=True, grow=0.05, entries=None):
    cfg_c, cfg_o = config(hold, predict, grow)
    e_host = O.fresh(1, T) if entries is None else entries.copy()
    e_ref = e_host.copy()
    rc, got = host(e_host, *tabs, cfg_c)
    want = O.coast(e_ref, *tabs, cfg_o)
    assert rc == 0 and not same(got, want), same(got, want)
    assert np.array_equal(e_host, e_ref)
    return got, e_host


BOX = (10.25, 20.5, 50.75, 81.125)


def test_hold_zero_emits_nothing_and_copies_exactly():
    tabs = frames([[(0, 0 | O.STARTED, BOX, 0.9)], [], [(0, 0, BOX, 0.8)]])
    (det_out, counts_out, track_out, idx_out, score_out), e = both(tabs, 2, hold=0)
    assert list(counts_out) == [1, 0, 1]
    assert np.array_equal(det_out[:, :2], tabs[1]) and np.array_equal(track_out[:, :2], tabs[3])
    assert np.array_equal(idx_out[:, :2], tabs[4]) and np.array_equal(score_out[:, :2], tabs[5])
    assert (det_out[:, 2:] == 0).all() and (track_out[:, 2:] == -1).all()
    assert e[0, 0, 1] == 0 and e[0, 0, 2] == 1                            # the entry was remembered through the gap all the same


def test_without_growth_and_prediction_the_last_box_leaves_bit_for_bit():
    odd = np.array([-0.0, 1e-42, np.inf, 3.3], np.float32)                 # a negative zero, a denormal, an infinity
    tabs = frames([[(7, 1 | O.STARTED, odd, 0.9)], [(7, 1, odd, 0.7)], [], []])
    (det_out, counts_out, track_out, idx_out, score_out), _ = both(tabs, 2, hold=4, predict=False, grow=0.0)
    assert list(counts_out) == [1, 1, 1, 1]
    for b, missed in ((2, 1), (3, 2)):
        assert np.array_equal(det_out[b, 0, :4].view(np.int32), odd.view(np.int32))
        assert det_out[b, 0, 4] == np.float32(0.7)
        assert tuple(track_out[b, 0]) == (7, 1 | O.COASTED | (missed << 16))
        assert idx_out[b, 0] == 7 % 3 and score_out[b, 0] == np.float32(0.5 + 0.07)


def test_velocity_after_a_gap_divides_by_missed_plus_one():
    a, b = np.array([10, 10, 40, 40], np.float32), np.array([20, 17, 51, 48], np.float32)
    tabs = frames([[(0, O.STARTED, a, 1)], [], [], [(0, 0, b, 1)], []])
    (det_out, counts_out, track_out, _, _), e = both(tabs, 1, hold=4, predict=True, grow=0.0)
    vel = (b - a) / np.float32(3)
    assert np.array_equal(e[0, 0, 9:13], vel.view(np.int32)) and e[0, 0, 2] == 1
    assert list(counts_out) == [1, 1, 1, 1, 1]
    assert np.array_equal(det_out[1, 0, :4], a) and np.array_equal(det_out[2, 0, :4], a)       # no velocity yet: held in place
    assert np.array_equal(det_out[4, 0, :4], b + vel * np.float32(1))
    assert track_out[2, 0, 1] == 0 | O.COASTED | (2 << 16)


def test_a_started_row_ends_a_coasting_entry_under_the_same_id():
    a, b = np.array([10, 10, 40, 40], np.float32), np.array([100, 100, 140, 150], np.float32)
    tabs = frames([[(0, O.STARTED, a, 1)], [(0, 0, a + 2, 1)], [], [(0, O.STARTED, b, 1)], []])  # a reset: ids begin again at 0
    (det_out, counts_out, _, _, _), e = both(tabs, 1, hold=4, predict=True, grow=0.0)
    assert e[0, 0, 2] == 0 and (e[0, 0, 9:13] == 0).all()                  # a new entry: no velocity from the old track
    assert np.array_equal(det_out[4, 0, :4], b) and counts_out[4] == 1
    tabs2 = frames([[(0, O.STARTED, a, 1)], [(0, 0, a + 2, 1)], [], [(0, 0, b, 1)], []])         # the same rows without STARTED: it continues
    _, e2 = both(tabs2, 1, hold=4, predict=True, grow=0.0)
    assert e2[0, 0, 2] == 1 and (e2[0, 0, 9:13] != 0).all()


def test_an_entry_past_hold_resumes_with_the_long_gap_velocity():
    a, b = np.array([0, 0, 30, 30], np.float32), np.array([70, 35, 100, 65], np.float32)
    tabs = frames([[(3, O.STARTED, a, 1)]] + [[]] * 6 + [[(3, 0, b, 1)], []])
    (det_out, counts_out, _, _, _), e = both(tabs, 1, hold=2, predict=True, grow=0.0)
    assert list(counts_out) == [1, 1, 1, 0, 0, 0, 0, 1, 1]                 # held for two frames, then silent, never forgotten
    vel = (b - a) / np.float32(7)
    assert np.array_equal(e[0, 0, 9:13], vel.view(np.int32))
    assert np.array_equal(det_out[8, 0, :4], b + vel)


def test_a_slot_named_twice_takes_the_higher_detection():
    a, b = np.array([0, 0, 30, 30], np.float32), np.array([5, 5, 36, 37], np.float32)
    tabs = frames([[(0, O.STARTED, a, 1)], [(0, 0, a + 1, 0.5), (0, 0, b, 0.25)], []])
    (det_out, counts_out, _, _, _), e = both(tabs, 1, hold=4, predict=False, grow=0.0)
    assert np.array_equal(e[0, 0, 5:9], b.view(np.int32)) and np.array_equal(e[0, 0, 9:13], (b - a).view(np.int32))
    assert counts_out[2] == 1 and np.array_equal(det_out[2, 0, :4], b) and det_out[2, 0, 4] == np.float32(0.25)
    tabs = frames([[(0, O.STARTED, a, 1)], [(0, 0, a + 1, 0.5), (9, O.STARTED, b, 0.25)], []])   # ... also when it is another track
    _, e = both(tabs, 1, hold=4)
    assert e[0, 0, 0] == 9 and e[0, 0, 2] == 0


def test_untracked_detections_touch_no_entry():
    a = np.array([0, 0, 30, 30], np.float32)
    tabs = frames([[(0, O.STARTED, a, 1)], [(-1, -1, a + 50, 1), (4, 5, a, 1)], [(-1, 0, a, 1)]])  # untracked; slot 5 >= T; id < 0
    (_, counts_out, track_out, _, _), e = both(tabs, 2, hold=4)
    assert list(counts_out) == [1, 3, 2] and e[0, 0, 0] == 0 and e[0, 0, 1] == 2 and e[0, 1, 0] == -1
    assert track_out[1, 2, 1] == 0 | O.COASTED | (1 << 16)


def test_counts_outside_the_capacity():
    a = np.array([0, 0, 30, 30], np.float32)
    tabs = list(frames([[(0, O.STARTED, a, 1), (1, 1 | O.STARTED, a + 40, 1)], [(0, 0, a, 1), (1, 1, a + 40, 1)], [(0, 0, a, 1), (1, 1, a + 40, 1)]]))
    tabs[2] = np.array([2, -3, 1000], np.int32)
    (_, counts_out, _, _, _), e = both(tuple(tabs), 2, hold=4)
    assert list(counts_out) == [2, 2, 2] and list(e[0, :, 1]) == [0, 0]    # -3 is no detection (both coast), 1000 is cap


def test_a_non_finite_box_propagates_as_the_quiet_nan():
    neg_nan = np.array([0xFFC12345], np.uint32).view(np.float32)[0]
    a = np.array([0, 0, 30, 30], np.float32)
    bad = np.array([neg_nan, 5, np.inf, 40], np.float32)
    tabs = list(frames([[(0, O.STARTED, a, 1)], [(0, 0, bad, neg_nan)], []]))
    tabs[5] = tabs[5].copy()
    tabs[5][1, 0] = neg_nan
    (det_out, counts_out, _, _, score_out), e = both(tuple(tabs), 1, hold=4, predict=True, grow=0.05)
    assert det_out[1, 0].view(np.uint32)[0] == 0xFFC12345 and score_out[1, 0].view(np.uint32) == 0xFFC12345   # a detection's row: copied
    assert e[0, 0, 5] == QNAN and e[0, 0, 9] == QNAN and e[0, 0, 13] == QNAN and e[0, 0, 4] == QNAN
    assert counts_out[2] == 1
    words = det_out[2, 0].view(np.uint32)
    assert words[0] == QNAN and words[4] == QNAN and score_out[2, 0].view(np.uint32) == QNAN
    assert words[2] == QNAN                                                # inf - NaN in the growth: a NaN the call made itself


def test_missed_saturates():
    entries = O.fresh(1, 1)
    entries[0, 0, 0], entries[0, 0, 1] = 5, (1 << 20) - 1
    tabs = frames([[], [], []], cap=1)
    (_, counts_out, _, _, _), e = both(tabs, 1, hold=1023, entries=entries)
    assert e[0, 0, 1] == 1 << 20 and list(counts_out) == [0, 0, 0]


def test_every_refusal_of_the_host_twin():
    stream, det, counts, track, ii, sc = [np.array(a) for a in walk_tables(1, 5, 3)[0]]
    good, _ = config(4, True, 0.05)
    B, cap = det.shape[:2]

    def refused(entries=True, outs_none=None, **kw):
        e = O.fresh(3, 5)
        e[1, 2, 0] = 4
        before = e.copy()
        args = dict(stream=stream, det=det, counts=counts, track=track, ii=ii, sc=sc, cfg=good)
        shape = {k: kw.pop(k) for k in ("S", "T", "B", "cap") if k in kw}
        args.update(kw)
        outs = out_arrays(B, cap, 5)
        mark = [o.copy() for o in outs]
        passed = [None if outs_none == i else o for i, o in enumerate(outs)]
        rc, _ = host(e if entries else None, args["stream"], args["det"], args["counts"], args["track"], args["ii"], args["sc"], args["cfg"],
                     outs=passed, **dict(dict(S=3, T=5, B=B, cap=cap), **shape))
        assert rc != 0, (kw, shape)
        assert np.array_equal(e, before) and not same(outs, mark)

    refused(entries=False)
    for name in ("stream", "det", "counts", "track", "cfg"):
        refused(**{name: None})
    for i in range(5):
        refused(outs_none=i)
    refused(ii=None)
    refused(sc=None)
    for shape in (dict(S=0), dict(T=0), dict(T=65), dict(B=0), dict(cap=0), dict(B=-1), dict(B=1 << 20, cap=1 << 11)):
        refused(**shape)
    bad_stream = stream.copy()
    bad_stream[-1] = 3
    refused(stream=bad_stream)
    for hold, grow, reserved in ((-1, 0.05, 0), (1024, 0.05, 0), (4, -0.01, 0), (4, 0.51, 0), (4, float("nan"), 0), (4, 0.05, 1)):
        c = _lib.CoastConfig(hold, True, grow)
        c.reserved = reserved
        refused(cfg=c)
    for hold, grow in ((0, 0.0), (1023, 0.5)):                             # the ends of the ranges are fine
        rc, _ = host(O.fresh(3, 5), stream, det, counts, track, ii, sc, _lib.CoastConfig(hold, False, grow))
        assert rc == 0
