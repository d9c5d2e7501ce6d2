"""CPU: the keeper walk (tests/dedup_oracle.py, the rule fid_gallery_dedup computes) and engine.merges_from_keepers against the reference's greedy
loop as engine.merge_from_pairs restates it -- on random graphs with shuffled ids, repeated scores and scores exactly at the threshold."""
import numpy as np

from dedup_oracle import walk_scores

THRESH = 0.8


def graph_case(rng, n_ids, density):
    """-> ids (shuffled), pairs [(id_a, id_b, score)] each unordered pair at most once in either orientation, S by ascending-id position"""
    ids = [int(i) for i in rng.permutation(1000)[:n_ids]]
    pos = {i: k for k, i in enumerate(sorted(ids))}
    levels = np.asarray([0.5, 0.79, THRESH, THRESH, 0.85, 0.85, 0.9, 0.97], np.float32)     # below, exactly at (inclusive) and above; repeated
    pairs, S = [], np.zeros((n_ids, n_ids), np.float32)
    for a in range(n_ids):
        for b in range(a + 1, n_ids):
            if rng.random() < density:
                s = float(levels[int(rng.integers(0, len(levels)))])
                x, y = (ids[a], ids[b]) if rng.random() < 0.5 else (ids[b], ids[a])
                pairs.append((x, y, s))
                S[pos[x], pos[y]] = S[pos[y], pos[x]] = s
    order = rng.permutation(len(pairs))
    return ids, [pairs[int(k)] for k in order], S


def test_walk_and_merges_from_keepers_equal_the_greedy_loop():
    from scrfd_arcface_facerecognition_amd.engine import merge_from_pairs, merges_from_keepers
    rng = np.random.default_rng(2726)
    merged = at_threshold = 0
    for case in range(600):
        n_ids = int(rng.integers(1, 14))
        ids, pairs, S = graph_case(rng, n_ids, (0.15, 0.4, 0.8)[case % 3])
        want = merge_from_pairs(ids, pairs, THRESH)
        keeper, score, summary = walk_scores(S, np.ones(n_ids, bool), np.float32(THRESH))
        got = merges_from_keepers(sorted(ids), keeper, score)
        assert got == want, (case, got, want)
        assert summary == (len(want), n_ids)
        merged += len(want)
        at_threshold += sum(1 for m in want if m[2] == float(np.float32(THRESH)))
    assert merged > 1000 and at_threshold > 100


def test_a_path_of_300_alternates():
    n = 300
    S = np.zeros((n, n), np.float32)
    k = np.arange(n - 1)
    S[k, k + 1] = S[k + 1, k] = 0.5
    keeper, score, summary = walk_scores(S, np.ones(n, bool), 0.49)
    pos = np.arange(n)
    assert np.array_equal(keeper, np.where(pos % 2 == 1, pos - 1, -1))                 # 150 levels deep: odd positions go to their left neighbour
    assert np.array_equal(score, np.where(pos % 2 == 1, np.float32(0.5), np.float32(0)))
    assert summary == (150, 300)


def test_first_alive_not_best():
    from scrfd_arcface_facerecognition_amd.engine import merge_from_pairs, merges_from_keepers
    S = np.zeros((3, 3), np.float32)
    S[0, 2] = S[2, 0] = 0.81                                                           # the low-rank survivor hits c weakly,
    S[1, 2] = S[2, 1] = 0.99                                                           # the higher-rank survivor strongly
    keeper, score, _ = walk_scores(S, np.ones(3, bool), THRESH)
    assert list(keeper) == [-1, -1, 0] and score[2] == np.float32(0.81)
    assert merges_from_keepers([10, 20, 30], keeper, score) == merge_from_pairs([30, 10, 20], [(30, 10, float(S[0, 2])), (20, 30, float(S[1, 2]))], THRESH)


def test_an_absorbed_person_absorbs_nobody_and_a_missing_one_takes_no_part():
    S = np.zeros((4, 4), np.float32)
    S[0, 1] = S[1, 0] = 0.9                                                            # 0 absorbs 1; 1 ~ 2 but 1 is gone; 0 !~ 2
    S[1, 2] = S[2, 1] = 0.9
    S[2, 3] = S[3, 2] = 0.9
    keeper, _, summary = walk_scores(S, np.ones(4, bool), THRESH)
    assert list(keeper) == [-1, 0, -1, 2] and summary == (2, 4)
    keeper, _, summary = walk_scores(S, np.asarray([True, True, False, True]), THRESH)  # the embedding of 2 is gone (:2757-2759): 3 survives
    assert list(keeper) == [-1, 0, -1, -1] and summary == (1, 3)


def test_merge_order_is_keeper_then_score_then_id():
    from scrfd_arcface_facerecognition_amd.engine import merges_from_keepers
    ids = [3, 5, 8, 9, 12]
    keeper = np.asarray([-1, -1, 1, 0, 0], np.int32)
    score = np.asarray([0, 0, 0.9, 0.85, 0.85], np.float32)
    assert merges_from_keepers(ids, keeper, score) == [(3, 9, float(np.float32(0.85))), (3, 12, float(np.float32(0.85))), (5, 8, float(np.float32(0.9)))]
    assert merges_from_keepers(ids, np.full(5, -1, np.int32), np.zeros(5, np.float32)) == []
