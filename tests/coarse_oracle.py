"""numpy restatement of the two-stage gallery search (include/faceid.h, fid_gallery_search_coarse; csrc/quant_core.h): the int8 quantisation rule,
the exact coarse scores, the packed keys of the shortlist, the fp16 rerank and the merge.  Everything up to the shortlist is integer arithmetic
and power-of-two scaling, so it predicts the device's keys bit for bit on ANY input; the rerank (a float64 product of the fp16 rows, rounded to
fp32) is exact wherever the fp32 sums are -- on probe rows, as cosines() of tests/test_match_exact_cpu.py argues -- and within summation-order
rounding elsewhere."""
import numpy as np

DIM_MAX = 1024
E_RANGE = np.arange(-31, 12)                         # wider than what fp16 magnitudes need (-30 .. 10)


def quantise(unit_f16):
    """fp16 [n, dim] -> (codes int8 [n, dim], exps int8 [n]).  e = the smallest integer with max|u| <= 127 * 2^e, found by trying them all;
    a row with max|u| == 0 or a NaN / inf element: e = 0, every code 0."""
    u = np.ascontiguousarray(unit_f16, np.float16)
    assert u.ndim == 2
    with np.errstate(invalid="ignore"):
        x = u.astype(np.float64)
        m = np.abs(x).max(1) if u.shape[1] else np.zeros(len(u))
    live = np.isfinite(x).all(1) & (m > 0)
    fits = np.where(live, m, 1.0)[:, None] <= 127.0 * 2.0 ** E_RANGE[None, :]
    e = np.where(live, E_RANGE[fits.argmax(1)], 0)
    assert (fits.any(1)).all()
    scaled = np.where(live[:, None], x, 0.0) * 2.0 ** (-e.astype(np.float64))[:, None]      # exact: a power-of-two scaling
    codes = np.rint(scaled)                                                               # ties to even
    assert (np.abs(codes) <= 127).all()
    return codes.astype(np.int8), e.astype(np.int8)


def coarse_scores(q16, g16):
    """-> (dot int64 [n, G], score float32 [n, G]) with score = ldexp(dot, e_q + e_g): exact (|dot| < 2^24, a normal fp32 result)"""
    qc, qe = quantise(q16)
    gc, ge = quantise(g16)
    assert q16.shape[1] == g16.shape[1] and q16.shape[1] % 64 == 0 and q16.shape[1] <= DIM_MAX
    dot = qc.astype(np.int64) @ gc.astype(np.int64).T
    assert np.abs(dot).max(initial=0) < 1 << 24
    s = np.ldexp(dot.astype(np.float64), qe.astype(np.int64)[:, None] + ge.astype(np.int64)[None, :])
    assert np.array_equal(s.astype(np.float32).astype(np.float64), s)
    return dot, s.astype(np.float32)


def sortable(s32):
    u = np.ascontiguousarray(s32, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def make_keys(score32, rows, ok):
    """(order-preserving bits of the score << 32) | ~row where ok, else 0"""
    key = (sortable(score32).astype(np.uint64) << np.uint64(32)) | (~np.asarray(rows, np.int64)).astype(np.uint32).astype(np.uint64)
    return np.where(ok, key, np.uint64(0))


def unpack(keys):
    u = (keys >> np.uint64(32)).astype(np.uint32)
    score = np.where(u & np.uint32(0x80000000), u & np.uint32(0x7FFFFFFF), ~u).astype(np.uint32).view(np.float32)
    return (~keys.astype(np.uint32)).view(np.int32), score


def best_keys(keys, R):
    """the R largest of every row, descending, padded with 0"""
    out = np.zeros((keys.shape[0], R), np.uint64)
    srt = np.sort(keys, axis=1)[:, ::-1][:, :R]
    out[:, :srt.shape[1]] = srt
    return out


def coarse_keys(q16, g16, R, first_row=0, scores=None):
    """fid_coarse_keys on one shard: uint64 [n, R], descending, 0 = no candidate; only dot > 0 makes a key.  scores: coarse_scores(q16, g16),
    where the caller has them already"""
    dot, s = scores if scores is not None else coarse_scores(q16, g16)
    rows = first_row + np.arange(g16.shape[0], dtype=np.int64)
    return best_keys(make_keys(s, rows[None, :], dot > 0), R)


def rerank(q16, g16, keys, first_row=0):
    """fid_rerank_keys: every non-zero key that names a row of this shard gets the score of the fp16 rows (float64 product, rounded to fp32);
    score <= 0 or NaN -> 0; each query's keys descending"""
    idx, _ = unpack(keys)
    local = idx.astype(np.int64) - first_row
    ok = (keys != 0) & (local >= 0) & (local < g16.shape[0])
    local = np.where(ok, local, 0)
    q, g = q16.astype(np.float64), g16.astype(np.float64)
    with np.errstate(invalid="ignore"):
        s = np.einsum("nd,nrd->nr", q, g[local]).astype(np.float32)
        ok &= s > 0
    return best_keys(make_keys(s, local + first_row, ok), keys.shape[1])


def merge(keys_all, k, G_total, thresh):
    """fid_topk_merge on keys [parts, n, R] -> (idx int32 [n, k], score float32 [n, k]), padded with (-1, 0.0); strict > max(0, thresh)"""
    parts, n, _ = keys_all.shape
    flat = keys_all.transpose(1, 0, 2).reshape(n, -1).copy()
    idx, _ = unpack(flat)
    flat[(idx < 0) | (idx >= G_total)] = 0
    best = best_keys(flat, k)
    idx, score = unpack(best)
    ok = (best != 0) & (score > max(0.0, float(np.float32(thresh))))
    return np.where(ok, idx, -1).astype(np.int32), np.where(ok, score, np.float32(0)).astype(np.float32)


def search_coarse(q16, g16, k, R, thresh, bounds=None):
    """fid_gallery_search_coarse; bounds = [0, b1, ..., G]: the same over contiguous row shards (shortlist and rerank per shard, one merge)"""
    assert 1 <= k <= R
    bounds = bounds or [0, g16.shape[0]]
    parts = []
    for lo, hi in zip(bounds, bounds[1:]):
        parts.append(rerank(q16, g16[lo:hi], coarse_keys(q16, g16[lo:hi], R, lo), lo))
    return merge(np.stack(parts), k, g16.shape[0], thresh)
