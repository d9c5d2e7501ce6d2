"""CPU: the tracker's oracle (tests/track_oracle.py) keeps its own invariants on the sequences the GPU tests use, the sequence generator is
deterministic, and the binding names the new entry points."""
import numpy as np
import pytest

from track_oracle import EMBED, STARTED, Tracker, draw_rows, ovr, random_walk


def test_new_entry_points_are_bound():
    from scrfd_arcface_facerecognition_amd import _lib
    for name in ("fid_tracker_create", "fid_tracker_destroy", "fid_tracker_reset", "fid_tracker_read", "fid_track_step", "fid_track_identify"):
        assert name in _lib.SIGNATURES, name
    assert (_lib.TRACK_STARTED, _lib.TRACK_EMBED, _lib.TRACK_SLOT_WORDS) == (STARTED, EMBED, 10)
    assert [f[0] for f in _lib.TrackConfig._fields_] == ["iou_thresh", "max_age", "refresh", "retry"]
    import ctypes as C
    assert C.sizeof(_lib.TrackConfig) == 16


def test_sequence_generator_is_deterministic():
    a, b, c = random_walk(7), random_walk(7), random_walk(8)
    for (d0, c0, s0), (d1, c1, s1) in zip(a, b):
        assert np.array_equal(d0, d1) and np.array_equal(c0, c1) and np.array_equal(s0, s1)
    assert any(not np.array_equal(x[0], y[0]) for x, y in zip(a, c))
    # what the walks are for: both streams occur, some frame is crowded beyond T = 4, a box is repeated within a frame
    det, counts, stream = a[0]
    assert set(stream.tolist()) == {0, 1} and max(int(c.max()) for _, c, _ in a) > 4
    assert any(np.array_equal(d[b, f, :4], d[b, g, :4]) for d, c, _ in a for b in range(len(c)) for f in range(c[b]) for g in range(f))


def test_overlap_is_the_nms_arithmetic():
    assert ovr((0, 0, 9, 9), (0, 0, 9, 4)) == np.float32(0.5)              # 50 / (100 + 50 - 50), the +1 convention
    assert ovr((0, 0, 9, 9), (20, 20, 29, 29)) == 0
    assert np.isnan(ovr((0, 0, 9, 9), (np.nan, 0, 9, 9)))
    assert ovr((3, 4, 40, 50), (3, 4, 40, 50)) == 1


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("row_cap", [96, 5])
def test_oracle_invariants_on_random_walks(seed, row_cap):
    S, T, B, cap = 2, 4, 12, 8
    trk = Tracker(S, T)
    rng = np.random.default_rng(100 + seed)
    last_id = np.full(S, -1)
    for det, counts, stream in random_walk(seed):
        track, offsets, src = trk.step(det, counts, stream, 0.3, 1, 3, 2, row_cap)
        flags = (track[..., 1] & EMBED) != 0
        for b in range(B):
            k = int(counts[b])
            assert (track[b, k:] == -1).all()
            words = track[b, :k, 1]
            slots = words[words >= 0] & 0xFF
            assert len(set(slots.tolist())) == len(slots) and (slots < T).all()        # a slot is never owned twice in a frame
            started = track[b, :k][(words >= 0) & ((words & STARTED) != 0), 0]
            s = int(stream[b])
            for tid in started.tolist():                                                # ids strictly increase per stream
                assert tid > last_id[s]
                last_id[s] = tid
            assert (track[b, :k][words < 0] == -1).all()
            flags[b, k:] = False
        assert np.array_equal(offsets, np.concatenate([[0], np.cumsum(flags.sum(axis=1))]))   # offsets: the prefix sum of the EMBED flags
        n = min(int(offsets[B]), row_cap)
        assert np.array_equal(src[:n], np.flatnonzero(flags.reshape(-1))[:n]) and (src[n:] == -1).all()
        idx, score = draw_rows(rng, row_cap)
        ii, sc = trk.identify(idx, score, n)
        slots_state, streams_state = trk.state()
        free = slots_state[..., 0] == -1
        assert not slots_state[free][:, 1:].any()                                       # a free slot: id -1, every other word 0
        assert (streams_state[:, 0] == last_id + 1).all()
        assert ((ii >= -1) & (ii < 5)).all() and (sc[ii < 0] == 0).all()
    assert trk.lost.sum() > 0 and (trk.next_id > T).all()                               # slots ran out, and slots were reused
