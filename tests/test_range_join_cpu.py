"""CPU: the host half of the range join -- engine.merge_from_pairs against the oracle's restatement of the reference's greedy merge loop
(smart_face_recognition.py:2755-2792), and the fid_gallery_range symbol with its argument check."""
import ctypes as C

import numpy as np

from oracle import match
from scrfd_arcface_facerecognition_amd import _lib


def duplicate_store(rng, n=120):
    """tests/test_gpu_align_match.py::_duplicate_store restated (that module builds a GPU context): person embeddings with tight clusters, a CHAIN
    a ~ b ~ c whose ends are below the threshold (the greedy order decides who absorbs whom), near-copies (>= 0.95) and unrelated persons"""
    base = rng.standard_normal((n, 512)).astype(np.float32)

    def near(v, cos):                                        # a vector at cosine `cos` from v
        v = v / np.linalg.norm(v)
        r = rng.standard_normal(512).astype(np.float32)
        r -= (r @ v) * v
        r /= np.linalg.norm(r)
        return (cos * v + np.sqrt(1 - cos * cos) * r).astype(np.float32) * np.float32(rng.uniform(0.5, 2.0))
    for i, j, c in ((40, 3, 0.93), (77, 3, 0.90), (78, 40, 0.97), (15, 90, 0.86), (91, 15, 0.99), (60, 61, 0.96)):
        base[i] = near(base[j], c)
    base[100] = near(base[50], 0.88)                         # chain: 50 ~ 100 ~ 101, 50 !~ 101
    v50 = base[50] / np.linalg.norm(base[50])
    v100 = base[100] / np.linalg.norm(base[100])
    away = v100 - (v100 @ v50) * v50
    away /= np.linalg.norm(away)
    base[101] = (0.88 * v100 + np.sqrt(1 - 0.88 ** 2) * (0.9 * away + np.sqrt(1 - 0.81) * near(away, 0.0) / np.linalg.norm(near(away, 0.0)))).astype(np.float32)
    return base


def host_pairs(ids, emb, threshold):
    """[(id_a, id_b, cosine)] of every pair at or above the threshold, in float64 on the host (the arithmetic of oracle.match.search_similar)"""
    e = np.asarray(emb, np.float64)
    unit = e / np.linalg.norm(e, axis=1, keepdims=True)
    out = []
    for i in range(len(ids)):
        s = unit @ unit[i]
        out += [(ids[i], ids[j], float(s[j])) for j in range(i + 1, len(ids)) if s[j] >= threshold]
    return out


def test_merge_from_pairs_equals_the_oracle_on_the_planted_store():
    from scrfd_arcface_facerecognition_amd.engine import merge_from_pairs
    rng = np.random.default_rng(55)
    emb = duplicate_store(rng)
    ids = [int(i) for i in rng.permutation(1000)[:len(emb)]]
    unit = emb.astype(np.float64) / np.linalg.norm(emb.astype(np.float64), axis=1, keepdims=True)
    S = (unit @ unit.T)[np.triu_indices(len(emb), 1)]
    assert np.abs(np.abs(S) - 0.8).min() > 2e-3                      # no pair within 2e-3 of the threshold
    want, survivors = match.find_and_merge_duplicates(ids, emb, 0.8)
    pairs = host_pairs(ids, emb, 0.8)
    assert len(want) >= 7 and len(pairs) > len(want)                  # (clusters: more pairs than merges)
    got = merge_from_pairs(ids, pairs, 0.8)
    assert [(a, b) for a, b, _ in got] == [(a, b) for a, b, _ in want]
    assert max(abs(g[2] - w[2]) for g, w in zip(got, want)) < 1e-12
    assert sorted(set(ids) - {b for _, b, _ in got}) == survivors
    # the pair list's own order and orientation do not matter
    shuffled = [(b, a, s) if k % 2 else (a, b, s) for k, (a, b, s) in enumerate(pairs)]
    shuffled = [shuffled[k] for k in rng.permutation(len(shuffled))]
    assert merge_from_pairs(ids, shuffled, 0.8) == got
    # pairs below the threshold in the list are ignored
    assert merge_from_pairs(ids, host_pairs(ids, emb, 0.5), 0.8) == got


def test_merge_from_pairs_breaks_equal_scores_by_ascending_id():
    from scrfd_arcface_facerecognition_amd.engine import merge_from_pairs
    # person 5 sees 9 and 7 at EXACTLY the same cosine (0.8 / 1.0 in both products); 7 and 9 are at 0.64 from each other, below the threshold
    emb = np.array([[1.0, 0.0, 0.0], [0.8, 0.6, 0.0], [0.8, 0.0, 0.6]])
    ids = [5, 9, 7]
    pairs = host_pairs(ids, emb, 0.7)
    assert sorted((a, b) for a, b, _ in pairs) == [(5, 7), (5, 9)] and pairs[0][2] == pairs[1][2]
    want, survivors = match.find_and_merge_duplicates(ids, emb, 0.7)
    got = merge_from_pairs(ids, pairs, 0.7)
    assert [(a, b) for a, b, _ in want] == [(5, 7), (5, 9)]
    assert got == [(5, 7, pairs[0][2]), (5, 9, pairs[0][2])] and survivors == [5]
    # a higher score still goes first, whatever its id
    assert [(a, b) for a, b, _ in merge_from_pairs([1, 2, 3], [(1, 2, 0.85), (1, 3, 0.9)], 0.8)] == [(1, 3), (1, 2)]
    # an absorbed id absorbs nobody: 2 is gone when its turn comes, so 4 survives
    assert merge_from_pairs([1, 2, 4], [(1, 2, 0.9), (2, 4, 0.9)], 0.8) == [(1, 2, 0.9)]
    assert merge_from_pairs([1, 2], [], 0.8) == []


def test_range_entry_point_is_bound_and_rejects_null_arguments():
    assert "fid_gallery_range" in _lib.SIGNATURES
    lib = _lib.load()
    assert lib.fid_gallery_range(None, None, None, 1, C.c_float(0.5), None, None, 16, None) == -1
    assert lib.fid_last_error().decode() != ""
