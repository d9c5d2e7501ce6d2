"""The duplicate-merge walk in numpy: what fid_gallery_dedup must return.  Imports nothing of the product.

Positions k = 0 .. n - 1 are the persons in ascending id:  keeper[k] = the LOWEST position j < k with keeper[j] == -1 and hit(j, k), else -1
(reference smart_face_recognition.py:2755-2792: every person still alive absorbs each alive larger id its search returns; the first alive one
that hits k therefore gets it).  hit = fp32 cosine >= thresh and > 0; a NaN never hits."""
import numpy as np


def walk_scores(S, part, thresh):
    """S [n, n]: S[j, k] = score of positions j and k (only j < k is read); part [n]: the position takes part.
    -> keeper int32 [n], score float32 [n], summary (absorbed, took part)"""
    S = np.asarray(S, np.float32)
    n = S.shape[0]
    t = np.float32(thresh)
    keeper, score = np.full(n, -1, np.int32), np.zeros(n, np.float32)
    alive = np.zeros(n, bool)
    with np.errstate(invalid="ignore"):
        hit = (S >= t) & (S > 0)
    for k in range(n):
        if not part[k]:
            continue
        cand = np.nonzero(alive[:k] & hit[:k, k])[0]
        if len(cand):
            keeper[k], score[k] = cand[0], S[cand[0], k]
        else:
            alive[k] = True
    return keeper, score, (int((keeper >= 0).sum()), int(np.count_nonzero(part)))


def walk(gallery16, rows, thresh):
    """gallery16: the stored fp16 rows [G, dim]; rows: gallery row per position (an entry outside [0, G) takes no part).  The cosines are the
    float64 sums of the fp16 products rounded to fp32: for rows whose products and sums are exact in fp32 that is the fp32 sum in ANY order."""
    g = np.asarray(gallery16)
    G = g.shape[0]
    rows = np.asarray(rows, np.int64)
    inside = (rows >= 0) & (rows < G)
    x = np.zeros((len(rows), g.shape[1]), np.float16)
    x[inside] = g[rows[inside]]
    part = (np.ascontiguousarray(x).view(np.uint16) & 0x7FFF).any(axis=1)
    x64 = x.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        S = (x64 @ x64.T).astype(np.float32)
    return walk_scores(S, part, thresh)


def applied(gallery16, rows, keeper):
    """the gallery after apply != 0: the absorbed positions' rows are all +0.0, every other byte is unchanged"""
    out = np.array(gallery16, copy=True)
    out[np.asarray(rows, np.int64)[np.asarray(keeper) >= 0]] = 0
    return out
