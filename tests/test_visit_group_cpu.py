"""CPU: the host half of the visit grouping -- the fid_gallery_group symbol with its argument check, the oracle of tests/visit_oracle.py on
hand-made three-dimensional cases (the sequential answer, not a connected-components one), and engine.visit_counters."""
import ctypes as C

import numpy as np
import pytest

from oracle import match
from scrfd_arcface_facerecognition_amd import _lib
from visit_oracle import DEFERRED, DUPLICATE, NEW, NO_FACE, RECOGNISED, best, group_visits

DUP, GROUP, SEARCH = 0.95, 0.5, 0.4


def test_group_entry_point_is_bound_and_rejects_null_arguments():
    assert "fid_gallery_group" in _lib.SIGNATURES
    lib = _lib.load()
    assert lib.fid_gallery_group(None, None, None, 1, C.c_float(0.9), C.c_float(0.5), C.c_float(0.4), None, 0, None, None, None, None) == -1
    assert lib.fid_last_error().decode() != ""


def at(cos, axis=1):
    """a unit vector at cosine `cos` from e0, the rest along `axis`"""
    v = np.zeros(3)
    v[0], v[axis] = cos, np.sqrt(1 - cos * cos)
    return v


def f16(rows):
    return np.asarray(rows, np.float64).astype(np.float16)


def test_chain_is_sequential_not_connected_components():
    # A = e0; B at 0.8 from A; C at 0.8 from B and 0.28 from A (0.8 * 0.8 - 0.6 * 0.6)
    A, B = at(1.0), at(0.8)
    Cv = np.array([0.8 * 0.8 - 0.6 * 0.6, 2 * 0.8 * 0.6, 0.0])
    q = f16([A, B, Cv])
    q64 = q.astype(np.float64)
    assert abs(q64[1] @ q64[0] - 0.8) < 2e-3 and abs(q64[2] @ q64[1] - 0.8) < 2e-3 and abs(q64[2] @ q64[0] - 0.28) < 2e-3
    store = np.zeros((4, 3), np.float16)
    verdict, row, score, summary, after = group_visits(store, q, [2, 0, 1], DUP, GROUP, SEARCH)
    # B is recognised as A and NOT stored, so C only sees A (0.28) and is a new person; a connected-components answer would chain A - B - C
    assert list(verdict) == [NEW, RECOGNISED, NEW]
    assert list(row) == [2, 2, 0] and summary == (2, 3)
    assert score[0] == 0.0 and abs(score[1] - 0.8) < 2e-3 and score[2] == 0.0          # 0.28 < search: the reported similarity is 0
    assert np.array_equal(after[2], q[0]) and np.array_equal(after[0], q[2]) and not after[[1, 3]].any()
    # with similarity_threshold below 0.28 the new person reports the similarity it was found at
    _, _, score, _, _ = group_visits(store, q, [2, 0, 1], DUP, GROUP, 0.2)
    assert abs(score[2] - 0.28) < 2e-3


def test_duplicate_of_a_person_created_in_the_same_batch_and_a_zero_row():
    q = f16([at(1.0), [0, 0, 0], at(0.97), at(0.0, 2), at(1.0)])
    q[1, 0] = np.float16(-0.0)                                # the marker row of an empty slot: still a zero row
    store = np.zeros((3, 3), np.float16)
    verdict, row, score, summary, after = group_visits(store, q, [0, 1, 2], DUP, GROUP, SEARCH)
    assert list(verdict) == [NEW, NO_FACE, DUPLICATE, NEW, DUPLICATE]
    assert list(row) == [0, -1, 0, 1, 0] and summary == (2, 5)
    assert score[1] == 0.0 and score[4] == 1.0 and abs(score[2] - 0.97) < 2e-3
    assert not after[2].any()                                 # the zero row was never stored, row 2 stays free


def test_equal_scores_resolve_to_the_lower_row():
    # two stored rows hold the same vector: the lower row is the hit
    v = f16([at(0.6)])[0]
    store = np.zeros((4, 3), np.float16)
    store[3] = store[1] = v
    verdict, row, score, _, _ = group_visits(store, f16([at(0.6)]), [0], DUP, GROUP, SEARCH)
    assert list(verdict) == [DUPLICATE] and row[0] == 1 and score[0] == float(v.astype(np.float64) @ v.astype(np.float64))
    # a stored row w and an in-batch new person u, both at EXACTLY the same cosine from visit x (u . w = 0.36: u is new): the lower ROW wins,
    # whichever of the two that is
    u, w, x = at(0.6, 1), at(0.6, 2), at(1.0)
    q = f16([u, x])
    for new_row, want in ((0, 0), (3, 2)):
        store = np.zeros((4, 3), np.float16)
        store[2] = f16([w])[0]
        verdict, row, score, _, after = group_visits(store, q, [new_row, 1], DUP, GROUP, SEARCH)
        assert list(verdict) == [NEW, RECOGNISED] and list(row) == [new_row, want]
        s = after.astype(np.float64) @ q[1].astype(np.float64)
        assert s[new_row] == s[2] == score[1]


def test_deferred_suffix_equals_a_second_call_on_the_suffix():
    rng = np.random.default_rng(3)
    dirs = rng.standard_normal((12, 3))
    q = f16(dirs / np.linalg.norm(dirs, axis=1, keepdims=True))
    q[5] = 0
    store = np.zeros((16, 3), np.float16)
    rows = [7, 3, 9, 1, 0, 12, 15, 2, 4, 5, 6, 8]
    full = group_visits(store, q, rows, 0.99, 0.9, 0.8)
    k = full[3][0]
    assert k >= 5 and full[3][1] == len(q)
    short = group_visits(store, q, rows[:k - 2], 0.99, 0.9, 0.8)
    d = short[3][1]
    assert short[3][0] == k - 2 and d < len(q) and full[0][d] == NEW
    assert list(short[0][:d]) == list(full[0][:d]) and list(short[1][:d]) == list(full[1][:d]) and list(short[2][:d]) == list(full[2][:d])
    assert all(v in (DEFERRED, NO_FACE) for v in short[0][d:]) and (short[1][d:] == -1).all() and (short[2][d:] == 0).all()
    assert short[0][5] == NO_FACE or d > 5
    rest = group_visits(short[4], q[d:], rows[k - 2:], 0.99, 0.9, 0.8)
    assert list(rest[0]) == list(full[0][d:]) and list(rest[1]) == list(full[1][d:]) and list(rest[2]) == list(full[2][d:])
    assert np.array_equal(rest[4], full[4])
    # no row at all: deferred from the first visit that needs one
    none = group_visits(store, q, [], 0.99, 0.9, 0.8)
    assert none[3] == (0, 0) and none[0][0] == DEFERRED and not none[4].any()


def test_best_is_the_first_hit_of_the_reference_search_on_unit_rows():
    """`best` against oracle.match.search_similar / is_duplicate_embedding where their semantics fit: rows whose fp16 norm is exactly 1"""
    rng = np.random.default_rng(9)
    store = np.zeros((40, 32), np.float64)
    for r in range(40):
        store[r, rng.permutation(32)[:16]] = rng.choice([-0.25, 0.25], 16)
    store[17] = store[4]                                      # an exact tie
    ids = list(range(40))
    for r in (4, 11, 39):
        q = store[r].copy()
        j, s = best(store, q)
        hits = match.search_similar(q, ids, store, k=5, threshold=0.4)
        assert hits[0] == (j, s) and s == 1.0
        assert match.is_duplicate_embedding(q, ids, store, 0.95)
    assert best(store, store[17])[0] == 4
    assert best(store, -store[4] * 0)[0] == -1 and best(np.zeros((3, 32)), store[0]) == (-1, 0.0)


def test_visit_counters():
    from scrfd_arcface_facerecognition_amd.engine import VISIT_VERDICTS, visit_counters
    assert VISIT_VERDICTS == ("new", "recognised", "duplicate", "no face", "deferred")
    recs = [{"verdict": v} for v in ("new", "recognised", "recognised", "duplicate", "no face", "new", "no face")]
    c = visit_counters(recs)
    assert c == {"processed": 4, "recognized": 2, "new_persons": 2, "no_faces": 2, "low_quality": 0, "download_failed": 0, "duplicate_faces": 1,
                 "low_similarity": 0}
    assert c["processed"] + c["no_faces"] + c["duplicate_faces"] == len(recs)
    assert visit_counters([])["processed"] == 0
    with pytest.raises(ValueError):
        visit_counters([{"verdict": "deferred"}])
