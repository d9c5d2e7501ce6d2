"""CPU: the host half of the fused top-k tests (tests/test_gpu_topk_fused.py runs them on the device) -- the conditions that keep the device
comparisons from passing vacuously, asserted for every shape and k they run, and a numpy mirror of the packed keys and their merge
(fid_topk_keys -> fid_topk_merge) that pins the key format, the "0 = no candidate" rule and the G_total rule without a device.

Fixtures and reference are tests/test_match_exact_cpu.py's: probe rows whose cosines are exact multiples of 1/64 in any summation order, so every
comparison is bit for bit, and which tie all the time, so the index decides who is in a top-k list."""
import numpy as np
import pytest

from test_gpu_range_join import unit_f16
from test_match_exact_cpu import build_queries, cosines, large_case, ref_topk, shard_bounds, small_case

SHAPES = ((129, 32, 17), (300, 96, 129), (1000, 64, 129), (1000, 512, 17), (2100, 64, 130))      # (G, dim, n)
KS = (1, 3, 5, 7, 10, 16, 17, 32)
TOPK_MAX = 32
LOW, HIGH = 0.05, 0.75


# ---- the numpy mirror of the packed keys -----------------------------------------------------------------------------------------------------------
def sortable(s32):
    u = np.ascontiguousarray(s32, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def keys_of(S, first_row, k):
    """fid_topk_keys on the scores [n, rows] of one shard: uint64 [n, k], descending, 0 = no candidate; only scores > 0 that are not NaN"""
    S = np.asarray(S, np.float32)
    rows = first_row + np.arange(S.shape[1], dtype=np.int64)
    key = (sortable(S).astype(np.uint64) << np.uint64(32)) | (~rows.astype(np.uint32)).astype(np.uint64)[None]
    with np.errstate(invalid="ignore"):
        key = np.where(S > 0, key, np.uint64(0))                                     # (a NaN fails the comparison)
    out = np.zeros((len(S), k), np.uint64)
    top = np.sort(key, axis=1)[:, ::-1][:, :k]
    out[:, :top.shape[1]] = top
    return out


def unpack(keys):
    u = (keys >> np.uint64(32)).astype(np.uint32)
    score = np.where(u & np.uint32(0x80000000), u & np.uint32(0x7FFFFFFF), ~u).astype(np.uint32).view(np.float32)
    return (~keys.astype(np.uint32)).view(np.int32), score


def merge_keys(keys_all, k, G_total, thresh):
    """fid_topk_merge on keys [parts, n, k]: the k largest of a query's parts x k keys, without the 0 keys and those whose index is >= G_total,
    then the strict threshold -> (idx int32 [n, k], score float32 [n, k]), padded with (-1, 0.0)"""
    parts, n, _ = keys_all.shape
    flat = keys_all.transpose(1, 0, 2).reshape(n, -1).copy()
    idx, _ = unpack(flat)
    flat[(idx < 0) | (idx >= G_total)] = 0
    best = np.sort(flat, axis=1)[:, ::-1][:, :k]
    idx, score = unpack(best)
    ok = (best != 0) & (score > max(0.0, float(np.float32(thresh))))
    return np.where(ok, idx, -1).astype(np.int32), np.where(ok, score, np.float32(0)).astype(np.float32)


def same(got, want):
    return np.array_equal(got[0], want[0]) and got[1].dtype == np.float32 and np.array_equal(got[1], want[1])


# ---- the conditions --------------------------------------------------------------------------------------------------------------------------------
def topk_conditions(S, k):
    """what the reference answer on scores S has to offer a top-k test"""
    n, G = S.shape
    srt = -np.sort(-S, axis=1)
    hits_low, hits_high = (S > LOW).sum(1), (S > HIGH).sum(1)
    idx = ref_topk(S, k, LOW)[0]
    tiles = [len({int(r) // 128 for r in row if r >= 0}) for row in idx]
    return dict(tie_at_k=bool(G > k and ((hits_low >= k) & (srt[:, k - 1] == srt[:, min(k, G - 1)]) & (srt[:, k - 1] > LOW)).any()),
                tie_share=float(((srt[:, k - 1] == srt[:, min(k, G - 1)]) & (srt[:, k - 1] > LOW)).mean()) if G > k else 0.0,
                two_tiles=max(tiles) >= 2, no_hit=bool((hits_low == 0).any()),
                padded=bool(((hits_high >= 1) & (hits_high <= k - 1)).any()))


@pytest.mark.parametrize("G,dim,n", SHAPES)
def test_small_fixtures_meet_the_topk_conditions(G, dim, n):
    g, q, _ = small_case(G, dim, n)
    S = cosines(unit_f16(q), unit_f16(g))
    for k in KS:
        c = topk_conditions(S, k)
        assert c["tie_at_k"] and c["no_hit"], (k, c)
        assert k < 3 or c["two_tiles"], (k, c)
        assert k < 2 or c["padded"], (k, c)                                           # (k = 1: a list of one has no room for "some, but fewer")


def test_large_fixture_meets_the_topk_conditions():
    g, info, Gp, dim, _ = large_case("full64", 256)
    S = cosines(unit_f16(build_queries(129, g, info, 10 * 129 + dim)), unit_f16(g))
    for k in (5, 16, 32):
        c = topk_conditions(S, k)
        assert c["tie_at_k"] and c["no_hit"] and c["two_tiles"] and c["padded"], (k, c)


# ---- the mirror ------------------------------------------------------------------------------------------------------------------------------------
def test_key_order_is_score_descending_then_row_ascending():
    S = np.array([[0.5, 0.75, 0.75, 0.25, 0.0, -0.5, np.nan, 1.0 / 64]], np.float32)
    keys = keys_of(S, 100, 8)
    idx, score = unpack(keys[0])
    assert idx[:5].tolist() == [101, 102, 100, 103, 107] and score[:5].tolist() == [0.75, 0.75, 0.5, 0.25, 1.0 / 64]
    assert not keys[0, 5:].any()                                                      # 0, a negative score and the NaN are no candidates
    assert (keys[0, :4] > keys[0, 1:5]).all()
    assert int(keys[0, 0]) == (0x80000000 | 0x3F400000) << 32 | (~101 & 0xFFFFFFFF)  # sortable(0.75) << 32 | ~row
    i, s = merge_keys(keys[None], 3, 102, 0.3)                                        # row 102 is outside a gallery of 102 rows
    assert i.tolist() == [[101, 100, -1]] and s.tolist() == [[0.75, 0.5, 0.0]]
    assert merge_keys(keys[None], 2, 1000, 0.75)[0].tolist() == [[-1, -1]]            # the threshold is strict


@pytest.mark.parametrize("G,dim,n", SHAPES)
def test_sharded_keys_merge_equals_the_whole_search(G, dim, n):
    g, q, _ = small_case(G, dim, n)
    q16 = unit_f16(q)
    q16[5] = np.nan                                                                   # an all-NaN query: k x (-1, 0.0)
    S = cosines(q16, unit_f16(g))
    b = shard_bounds(G, 3) if G > 600 else [0, G // 3 + 1, 2 * G // 3 + 2, G]
    for k in KS:
        keys = np.stack([keys_of(S[:, lo:hi], lo, k) for lo, hi in zip(b, b[1:])])
        assert (keys[:, :, :-1] >= keys[:, :, 1:]).all()
        for thresh in (LOW, HIGH, 0.0, -1.0):
            want = ref_topk(S, k, thresh)
            assert same(merge_keys(keys, k, G, thresh), want), (k, thresh)
            assert same(merge_keys(keys_of(S, 0, k)[None], k, G, thresh), want), (k, thresh)      # one part = the unsharded search
        assert (merge_keys(keys, k, G, LOW)[0][5] == -1).all()
        # G_total cuts the answer off: a last shard whose rows all lie at or past it is ignored = the search over the shorter gallery
        assert same(merge_keys(keys, k, b[2], LOW), ref_topk(S[:, :b[2]], k, LOW)), k
