"""Genuine / impostor score distributions in numpy: what fid_gallery_score_hist and fid_score_hist_host must return.  Imports nothing of the product.

Positions k = 0 .. n - 1.  A position takes part when its row is inside the gallery, the row holds a non-zero element (the sign bit does not count)
and its label is >= 0.  Every unordered pair i < j of positions that take part is counted once; s = the fp32 cosine of the two stored fp16 rows.
  class     = genuine when the two labels are equal, impostor otherwise
  bin       = a non-finite s: no bin, counted in summary[3]; otherwise floor(fp32(s * fp32(bins / 2))) + bins / 2, clamped to [0, bins - 1]
  imp_via[k] = the position j != k of another label with the HIGHEST finite score, gen_via[k] = the position j != k of the same label with the LOWEST;
              the lowest position among equal scores; imp_score / gen_score = that score; -1 / 0.0 without such a pair
  summary   = (took part, genuine pairs, impostor pairs, non-finite pairs)
Scores are ordered by sortable(): the order of the numbers, and -0.0 BELOW +0.0 -- the two are equal as numbers, so this pins a corner that a sum
starting from +0.0 never reaches."""
import numpy as np


def sortable(s):
    """float32 array -> uint64 words whose unsigned order is the order of the scores, -0.0 below +0.0"""
    u = np.ascontiguousarray(s, np.float32).view(np.uint32).astype(np.uint64)
    return np.where(u & 0x80000000, u ^ 0xFFFFFFFF, u | 0x80000000)


def bin_of(s, bins):
    """the bin of finite float32 scores: ONE rounded fp32 multiply, then floor and clamp"""
    half = bins // 2
    with np.errstate(over="ignore"):
        f = np.floor(np.asarray(s, np.float32) * np.float32(half))                   # (float32 * float32 -> float32)
    assert f.dtype == np.float32
    return (np.clip(f.astype(np.float64), -half, half - 1) + half).astype(np.int64)


def hist_scores(S, part, labels, bins):
    """S [n, n] symmetric float32 scores, part [n] bool (labels already counted in), labels [n] ->
    hist uint64 [2, bins], imp_via int32 [n], imp_score float32 [n], gen_via int32 [n], gen_score float32 [n], summary (4 ints)"""
    S = np.asarray(S, np.float32)
    n = S.shape[0]
    part = np.asarray(part, bool)
    labels = np.asarray(labels, np.int64)
    pair = part[:, None] & part[None, :] & ~np.eye(n, dtype=bool)
    fin = np.isfinite(S)
    same = labels[:, None] == labels[None, :]
    upper = np.triu(np.ones((n, n), bool), 1)
    hist = np.zeros((2, bins), np.uint64)
    for cls, of_class in enumerate((same, ~same)):
        m = upper & pair & fin & of_class
        hist[cls] = np.bincount(bin_of(S[m], bins), minlength=bins).astype(np.uint64)
    non_finite = int((upper & pair & ~fin).sum())
    w = sortable(S)
    pos = np.arange(n)
    out = []
    for of_class, highest in ((~same, True), (same, False)):
        via, score = np.full(n, -1, np.int32), np.zeros(n, np.float32)
        cand = pair & fin & of_class
        for k in np.nonzero(cand.any(1))[0]:
            js = pos[cand[k]]
            ws = w[k, js]
            best = js[ws == (ws.max() if highest else ws.min())][0]                  # (the first = the lowest position among equal scores)
            via[k], score[k] = best, S[k, best]
        out += [via, score]
    return (hist, *out, (int(part.sum()), int(hist[0].sum()), int(hist[1].sum()), non_finite))


def scores(gallery16, rows):
    """-> S float32 [n, n], has [n] bool (row inside the gallery with a non-zero element).  The cosines are the float64 sums of the fp16 products
    rounded to fp32: for rows whose products and sums are exact in fp32 that is the fp32 sum in ANY order (+ 0.0: a sum that starts from +0.0 is
    never -0.0)."""
    g = np.asarray(gallery16)
    G = g.shape[0]
    rows = np.arange(G) if rows is None else np.asarray(rows, np.int64)
    inside = (rows >= 0) & (rows < G)
    x = np.zeros((len(rows), g.shape[1]), np.float16)
    x[inside] = g[rows[inside]]
    has = (np.ascontiguousarray(x).view(np.uint16) & 0x7FFF).any(axis=1)
    x64 = x.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        S = (x64 @ x64.T + 0.0).astype(np.float32)
    return S, has


def score_hist(gallery16, rows, labels, bins):
    """gallery16: the stored fp16 rows [G, dim]; rows: gallery row per position (an entry outside [0, G) takes no part), None = 0 .. G - 1;
    labels: int [n], negative = unlabelled"""
    S, has = scores(gallery16, rows)
    labels = np.asarray(labels, np.int64)
    return hist_scores(S, has & (labels >= 0), labels, bins)
