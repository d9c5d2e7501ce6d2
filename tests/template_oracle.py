"""The rule of fid_gallery_templates (include/faceid.h) in numpy, written from the header's text: int64 sums, the pinned fp64 norm, two roundings
to fp16, int64 dot products.  Rows that occur at several positions are summed once per distinct row with their total weight -- integer sums do
not care -- so the case at the bound (2^20 positions) takes a moment, not minutes."""
import numpy as np

I32 = np.iinfo(np.int32)


def fixed(g16):
    """fp16 [.., dim] with |x| <= 2 -> x * 2^24 as int64, exact"""
    return np.rint(np.asarray(g16, np.float16).astype(np.float64) * 16777216.0).astype(np.int64)


def norm(S):
    d = S.astype(np.float64)
    q = d * d
    q = np.concatenate([q, np.zeros((-len(q)) % 512)]).reshape(-1, 64, 8)
    v = np.zeros(64, np.float64)
    for j in range(q.shape[0]):
        for e in range(8):
            v = v + q[j, :, e]
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[np.arange(64) ^ o]
    return np.sqrt(v[0])


def template_of(S):
    """-> (fp16 row, nrm)"""
    nrm = norm(S)
    if not nrm > 0:
        return np.zeros(len(S), np.float16), 0.0
    return (S.astype(np.float64) / nrm).astype(np.float32).astype(np.float16), float(nrm)


def takes_part(g16, rows, labels, weights, P):
    """-> (member mask [n], eligible-but-rejected count)"""
    G = len(g16)
    bits = np.ascontiguousarray(g16).view(np.uint16) & 0x7FFF
    row_ok = (bits.max(1) <= 0x4000) & (bits.max(1) > 0)
    elig = (rows >= 0) & (rows < G) & (labels >= 0) & (labels < P) & (weights >= 1) & (weights <= 255)
    good = np.zeros(len(rows), bool)
    good[elig] = row_ok[rows[elig]]
    return elig & good, int((elig & ~good).sum())


def templates(g16, rows, labels, weights, P, min_score):
    """-> (templates fp16 [P, dim], score fp32 [n], kept int32 [n], person int32 [P, 4], cohesion fp32 [P], summary (6 ints))"""
    g16 = np.ascontiguousarray(g16, np.float16)
    G, dim = g16.shape
    n = G if rows is None else len(rows)
    rows = np.arange(G, dtype=np.int64) if rows is None else np.asarray(rows, np.int64)
    labels = np.asarray(labels, np.int64)
    weights = np.ones(n, np.int64) if weights is None else np.asarray(weights, np.int64)
    min_score = np.float32(min_score)
    member, rejected = takes_part(g16, rows, labels, weights, P)
    tpl = np.zeros((P, dim), np.float16)
    score, kept = np.zeros(n, np.float32), np.full(n, -1, np.int32)
    person, cohesion = np.zeros((P, 4), np.int32), np.zeros(P, np.float32)
    person[:, 2:] = -1
    dropped = zero = 0
    order = np.argsort(np.where(member, labels, P), kind="stable")
    bounds = np.searchsorted(np.where(member, labels, P)[order], np.arange(P + 1))

    def weighted_sum(pos):
        if len(pos) == 0:
            return np.zeros(dim, np.int64), 0
        ur, inv = np.unique(rows[pos], return_inverse=True)
        w = np.bincount(inv, weights=weights[pos].astype(np.float64)).astype(np.int64)          # (<= 2^28: exact in float64)
        return (w[:, None] * fixed(g16[ur])).sum(0), int(w.sum())

    for p in range(P):
        pos = np.sort(order[bounds[p]:bounds[p + 1]])
        S, W = weighted_sum(pos)
        t, nrm = template_of(S)
        if len(pos):
            ur, inv = np.unique(rows[pos], return_inverse=True)
            D = (fixed(g16[ur]) * fixed(t)[None, :]).sum(1)
            s = (D.astype(np.float64) * 2.0 ** -48).astype(np.float32)[inv]
            keep = np.ones(len(pos), bool) if min_score <= np.float32(-2) else s >= min_score
            score[pos], kept[pos] = s, keep
            lo, hi = pos[s == s.min()][0], pos[s == s.max()][0]
            person[p] = (len(pos), int(keep.sum()), lo, hi)
            if not keep.all():
                S, W = weighted_sum(pos[keep])
                t, nrm = template_of(S)
                dropped += int((~keep).sum())
        tpl[p] = t
        zero += not nrm > 0
        cohesion[p] = np.float32(nrm / (float(W) * 16777216.0)) if nrm > 0 else np.float32(0)
    return tpl, score, kept, person, cohesion, (int(member.sum()), int((person[:, 0] > 0).sum()), int(zero), dropped, rejected, 0)
