"""CPU: fid_track_relink_host (csrc/relink_core.h's walk, the host twin of csrc/relink.hip) against tests/relink_oracle.py, bit for bit on
the person table and on every state word, q stores included -- on tracked walks with returning rectangles and on hand-made frames at every
edge of the rules."""
import numpy as np
import pytest

import relink_oracle as O
from relink_calls import DIMS, SHAPES, THRESH, WINDOW, config, differs, fresh, host, person_out, split_step, walk_case
from scrfd_arcface_facerecognition_amd import _lib

STARTED, EMBED, RELINKED = 1 << 8, 1 << 9, 1 << 11


def test_constants():
    assert _lib.TRACK_RELINKED == RELINKED == O.RELINKED and _lib.RELINK_WORDS == O.WORDS == 8
    c = _lib.RelinkConfig()
    assert (c.thresh, c.window, c.pool) == (0.45, 300, 32) and c.c(7).max_age == 7


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("T, cap, L", SHAPES)
def test_walks_equal_the_oracle(T, cap, L, dim):
    steps, want, _ = walk_case(T, cap, L, dim)
    state = fresh(3 if cap >= 64 else 2, T, L, dim)
    cfg = config()
    for call, step in enumerate(steps):
        rc, person = host(state, step, cfg)
        assert rc == 0
        assert np.array_equal(person, want[call][0]), call
        assert not differs(state, want[call][1]), (call, differs(state, want[call][1]))


@pytest.mark.parametrize("T, cap, L", [(5, 3, 4), (64, 70, 32)])
def test_split_calls_equal_one_call(T, cap, L):
    dim = 40
    steps, want, _ = walk_case(T, cap, L, dim)
    B = len(steps[0][0])
    for parts in (B, 3):
        state = fresh(3 if cap >= 64 else 2, T, L, dim)
        for call, step in enumerate(steps):
            persons = []
            for sub in split_step(step, parts):
                rc, person = host(state, sub, config())
                assert rc == 0
                persons.append(person)
            assert np.array_equal(np.concatenate(persons), want[call][0]), (parts, call)
            assert not differs(state, want[call][1]), (parts, call)


# ---- hand-made frames ------------------------------------------------------------------------------

def unit(dim, cols, signs=None):
    row = np.zeros(dim, np.float16)
    row[list(cols)] = (np.ones(len(cols)) if signs is None else np.asarray(signs, np.float64)) / np.sqrt(len(cols))
    return row


def frames_step(frames, cap, dim, counts=None):
    """frames: per frame (stream, [(track id, word, row or None)]) -> the step's tables; a face with a row gets one, in order"""
    B = len(frames)
    stream = np.array([f[0] for f in frames], np.int32)
    track = np.full((B, cap, 2), -1, np.int32)
    cnt = np.zeros(B, np.int32)
    offsets = np.zeros(B + 1, np.int32)
    src, q = [], []
    for b, (_, faces) in enumerate(frames):
        cnt[b] = len(faces)
        for f, (tid, word, row) in enumerate(faces):
            track[b, f] = (tid, word)
            if row is not None:
                src.append(b * cap + f)
                q.append(row)
        offsets[b + 1] = len(src)
    src_a = np.full(max(len(src), 1) + 2, -1, np.int32)
    src_a[:len(src)] = src
    q_a = np.stack(q).astype(np.float16) if q else np.zeros((0, dim), np.float16)
    return stream, (cnt if counts is None else np.asarray(counts, np.int32)), track, offsets, src_a, q_a


def both(S, T, L, dim, steps, thresh=THRESH, window=WINDOW, max_age=1):
    """the steps through the host twin and the oracle; both must agree -> (oracle, persons per step)"""
    ref = O.Relinker(S, T, L, dim)
    state = fresh(S, T, L, dim)
    persons = []
    for step in steps:
        stream, counts, track, offsets, src, q = step
        want = ref.step(stream, counts, track, offsets, src, len(src), len(q), q, thresh, window, max_age)
        rc, person = host(state, step, config(thresh, window, max_age))
        assert rc == 0
        assert np.array_equal(person, want)
        assert not differs(state, ref.state()), differs(state, ref.state())
        persons.append(want)
    return ref, persons


DIM = 16
A, A34 = unit(DIM, (0, 1, 2, 3)), unit(DIM, (0, 1, 2, 4))      # A . A34 = 0.75 exactly
NEW = STARTED | EMBED


def leave_and_return(first, second, gap=2, second_row=True, dim=DIM):
    """track 0 with row `first` in slot 0, `gap` empty frames (max_age 1: it retires), then track 1 STARTS in slot 0 with row `second`"""
    frames = [(0, [(0, 0 | NEW, first)])] + [(0, [])] * gap + [(0, [(1, 0 | NEW, second if second_row else None)])]
    return frames_step(frames, 2, dim)


def test_score_equal_to_thresh_does_not_link():
    ref, persons = both(1, 2, 2, DIM, [leave_and_return(A, A34)], thresh=0.75)
    assert not ref.links and tuple(persons[0][3, 0]) == (1, 0 | NEW)
    below = float(np.nextafter(np.float32(0.75), np.float32(0)))
    ref, persons = both(1, 2, 2, DIM, [leave_and_return(A, A34)], thresh=below)
    assert len(ref.links) == 1 and ref.links[0][5] == 0.75
    assert tuple(persons[0][3, 0]) == (0, 0 | NEW | RELINKED)
    assert tuple(ref.live[0, 0]) == (1, 0, 1, np.float32(0.75).view(np.int32), 3, 0, 0, 0) and ref.pool[0, 0, 0] == -1


def test_equal_scores_the_lower_pool_index_wins():
    # tracks 0 and 1 hold the same row in slots 0 and 1 and retire in one frame, slots ascending: pool 0 = track 0, pool 1 = track 1
    frames = [(0, [(0, 0 | NEW, A), (1, 1 | NEW, A)]), (0, []), (0, []), (0, [(2, 0 | NEW, A)]), (0, [(2, 0, None), (3, 1 | NEW, A)])]
    ref, persons = both(1, 2, 2, DIM, [frames_step(frames, 2, DIM)])
    assert [(l[2], l[3]) for l in ref.links] == [(2, 0), (3, 1)]
    assert tuple(persons[0][4, 0]) == (0, 0 | RELINKED) and tuple(persons[0][4, 1]) == (1, 1 | NEW | RELINKED)


def test_window_edge():
    # the track's seen is frame 0; it is scored in frame `gap + 1`
    for window, links in ((3, 1), (2, 0)):
        ref, _ = both(1, 2, 2, DIM, [leave_and_return(A, A, gap=2)], window=window)
        assert len(ref.links) == links, window


def test_started_without_a_row_links_later():
    frames = [(0, [(0, 0 | NEW, A)]), (0, [(1, 0 | STARTED, None)]), (0, [(1, 0, None)]), (0, [(1, 0 | EMBED, A)])]
    ref, persons = both(1, 1, 1, DIM, [frames_step(frames, 1, DIM)])
    assert [tuple(p[0]) for p in persons[0]] == [(0, NEW), (1, STARTED), (1, 0), (0, EMBED | RELINKED)]
    assert ref.links == [(0, 3, 1, 0, 0, 1.0)]


def test_a_zero_row_never_links():
    zero = np.zeros(DIM, np.float16)
    ref, _ = both(1, 2, 2, DIM, [leave_and_return(zero, zero)], thresh=0.0)
    assert not ref.links and ref.attempts == [(0.0, [0.0])]


def test_chain_keeps_the_first_id_and_a_full_pool_is_overwritten():
    B_, C_ = unit(DIM, (4, 5, 6, 7)), unit(DIM, (8, 9, 10, 11))
    frames = [(0, [(0, 0 | NEW, A)]), (0, []), (0, []), (0, [(1, 0 | NEW, A)]), (0, []), (0, []), (0, [(2, 0 | NEW, A)]),
              (0, [(3, 0 | NEW, B_)]), (0, [(4, 0 | NEW, C_)]), (0, [(5, 0 | NEW, A)])]
    ref, persons = both(1, 1, 1, DIM, [frames_step(frames, 1, DIM)])
    assert [(l[2], l[3], l[4]) for l in ref.links] == [(1, 0, 0), (2, 0, 1)] and len(ref.chains()) == 1
    assert ref.overwrites == 2 and tuple(persons[0][9, 0]) == (5, NEW)      # L = 1: A was overwritten by B, B by C


def test_counts_far_outside_and_untracked_faces_and_rows():
    frames = [(0, [(0, 0 | NEW, A), (-1, -1, A), (7, 63, A)]), (1, [(0, 1 | NEW, A)]), (0, [(0, 0, None)]), (1, [(0, 1, None)])]
    step = frames_step(frames, 3, DIM, counts=[2 ** 31 - 1, -2 ** 31, 1, 5])
    ref, persons = both(2, 2, 2, DIM, [step])
    assert [tuple(v) for v in persons[0][0]] == [(0, NEW), (-1, -1), (-1, -1)]       # slot 63 >= T: untracked, and so is its row
    assert (persons[0][1] == -1).all()                                                # a count below 0: no detection, its row is ignored
    assert tuple(persons[0][3, 0]) == (0, 1) and ref.live[1, 1, 2] == 0               # a count above cap is cap; track 0 of stream 1 never got a row


def test_skipped_frames_do_not_age():
    frames = [(0, [(0, 0 | NEW, A)]), (-1, [(9, 0 | NEW, A)]), (-1, []), (-1, []), (0, [(0, 0, None)])]
    ref, persons = both(1, 1, 1, DIM, [frames_step(frames, 1, DIM)])
    assert ref.frames[0] == 2 and tuple(ref.live[0, 0]) == (0, 0, 1, 0, 0, 0, -1, 0) and (persons[0][1:4] == -1).all()


def test_n_rows_below_the_row_table():
    step = leave_and_return(A, A)
    stream, counts, track, offsets, src, q = step
    ref = O.Relinker(1, 2, 2, DIM)
    want = ref.step(stream, counts, track, offsets, src, len(src), 1, q, THRESH, WINDOW, 1)
    state = fresh(1, 2, 2, DIM)
    rc, person = host(state, step, config(), n_rows=1)
    assert rc == 0 and np.array_equal(person, want) and not differs(state, ref.state())
    assert not ref.links and ref.live[0, 0, 2] == 0               # the returning track's row lies beyond n_rows: no q yet


def test_refusals_leave_everything_untouched():
    step = leave_and_return(A, A)
    nan = float("nan")
    bad = [dict(cfg=config(thresh=1.0)), dict(cfg=config(thresh=-0.1)), dict(cfg=config(thresh=nan)), dict(cfg=config(thresh=float("inf"))),
           dict(cfg=config(window=-1)), dict(cfg=config(max_age=-1)), dict(cfg=None), dict(n_rows=-1), dict(n_rows=len(step[4]) + 1), dict(dim=12),
           dict(dim=0)]
    for kw in bad:
        state = fresh(1, 2, 2, DIM)
        before = [a.copy() for a in state]
        person = person_out(4, 2)
        rc, _ = host(state, step, kw.pop("cfg", config()), person=person, **kw)
        assert rc == -1, kw
        assert not differs(state, before) and (person.view(np.uint8) == 0x5A).all()
    for hole in range(6):                                         # every table pointer NULL in turn
        state = fresh(1, 2, 2, DIM)
        holed = list(step)
        holed[hole] = None
        person = person_out(4, 2)
        assert _call_with_holes(state, holed, person) == -1, hole
        assert (person.view(np.uint8) == 0x5A).all()
    assert _call_with_holes(fresh(1, 2, 2, DIM), list(step), None) == -1


def _call_with_holes(state, step, person):
    import ctypes as C
    live, pool, frames, live_q, pool_q = state
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    i = lambda a: None if a is None else a.ctypes.data_as(_lib.c_i32_p)
    stream, counts, track, offsets, src, q = step
    cfg = config()
    return _lib.load().fid_track_relink_host(i(live), p(live_q), i(pool), p(pool_q), i(frames), 1, 2, 2, DIM, i(stream), 4, 2, p(counts), p(track),
                                             p(offsets), p(src), 6, 2, p(q), C.byref(cfg), p(person))


def test_the_numpy_helper_is_the_host_twin():
    from scrfd_arcface_facerecognition_amd.utils.helpers import relink_state, relink_tracks
    T, cap, L, dim = 5, 3, 4, 40
    steps, want, _ = walk_case(T, cap, L, dim)
    state = relink_state(2, T, L, dim)
    for call, (stream, counts, track, offsets, src, q) in enumerate(steps):
        person = relink_tracks(state, stream, counts, track, offsets, src, q, config=_lib.RelinkConfig(THRESH, WINDOW, L), max_age=1)
        assert np.array_equal(person, want[call][0])
        assert not differs([state[k] for k in ("live", "pool", "frames", "live_q", "pool_q")], want[call][1])
    with pytest.raises(ValueError):
        relink_tracks(state, *steps[0], config=_lib.RelinkConfig(pool=L + 1))
