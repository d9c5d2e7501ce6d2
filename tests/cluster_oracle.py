"""Density clusters in numpy: what fid_gallery_cluster and fid_cluster_host must return.  Imports nothing of the product.

Positions k = 0 .. n - 1.  A position takes part when its row is inside the gallery and holds a non-zero element (the sign bit does not count).
hit(j, k) = fp32 cosine >= thresh and > 0 between two positions that take part; a NaN never hits.
  degree[k] = 1 + the other positions that hit k (0 for a position that takes no part);  core[k] = degree[k] >= min_pts
  cluster   = a connected component of the hit graph restricted to cores (breadth-first search); its label is its lowest core position
  via[k]    = the core c != k that hits k with the highest score, the lowest position among equal scores; score[k] = that cosine; -1 / 0 without
  label[k]  = a core's cluster; a non-core position with via >= 0 (a border) takes via's label; everything else -1 (noise if it takes part)
  summary   = (clusters, cores, borders, noise, took part, 0)"""
from collections import deque

import numpy as np


def cluster_scores(S, part, thresh, min_pts):
    """S [n, n] symmetric scores, part [n] bool -> label, degree, via int32 [n], score float32 [n], summary (6 ints)"""
    S = np.asarray(S, np.float32)
    n = S.shape[0]
    part = np.asarray(part, bool)
    with np.errstate(invalid="ignore"):
        hit = (S >= np.float32(thresh)) & (S > 0)
    hit &= part[:, None] & part[None, :]
    hit &= ~np.eye(n, dtype=bool)
    hit = hit | hit.T                                        # (S is symmetric; this only states that a hit has no direction)
    degree = np.where(part, 1 + hit.sum(1), 0).astype(np.int32)
    core = part & (degree >= min_pts)
    label = np.full(n, -1, np.int32)
    for k in range(n):                                       # ascending: the first core of a component to be met is its lowest
        if not core[k] or label[k] >= 0:
            continue
        label[k] = k
        todo = deque([k])
        while todo:
            i = todo.popleft()
            for j in np.nonzero(hit[i] & core & (label < 0))[0]:
                label[j] = k
                todo.append(j)
    via, score = np.full(n, -1, np.int32), np.zeros(n, np.float32)
    for k in np.nonzero(part)[0]:
        cand = np.nonzero(hit[k] & core)[0]
        if len(cand):
            best = cand[np.argmax(S[k, cand])]               # (argmax returns the first = lowest position among equal scores)
            via[k], score[k] = best, S[k, best]
            if not core[k]:
                label[k] = label[best]
    border = part & ~core & (via >= 0)
    noise = part & (label < 0)
    clusters = int(np.count_nonzero(core & (label == np.arange(n))))
    return label, degree, via, score, (clusters, int(core.sum()), int(border.sum()), int(noise.sum()), int(part.sum()), 0)


def cluster(gallery16, rows, thresh, min_pts):
    """gallery16: the stored fp16 rows [G, dim]; rows: gallery row per position (an entry outside [0, G) takes no part), None = 0 .. G - 1.
    The cosines are the float64 sums of the fp16 products rounded to fp32: for rows whose products and sums are exact in fp32 that is the fp32
    sum in ANY order."""
    g = np.asarray(gallery16)
    G = g.shape[0]
    rows = np.arange(G) if rows is None else np.asarray(rows, np.int64)
    inside = (rows >= 0) & (rows < G)
    x = np.zeros((len(rows), g.shape[1]), np.float16)
    x[inside] = g[rows[inside]]
    part = (np.ascontiguousarray(x).view(np.uint16) & 0x7FFF).any(axis=1)
    x64 = x.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        S = (x64 @ x64.T).astype(np.float32)
    return cluster_scores(S, part, thresh, min_pts)


def partition(label):
    """the clusters as a set of frozensets of positions (names dropped)"""
    label = np.asarray(label)
    return {frozenset(int(k) for k in np.nonzero(label == l)[0]) for l in np.unique(label[label >= 0])}
