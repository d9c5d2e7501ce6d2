"""Stores for the score-distribution tests (test_calib_cpu.py, test_calib_host_sanitized.py, test_gpu_calib.py), numpy only.  Every row is +-1 on
a fixed set of columns -- 64 of 512 (unit entries 1/8) or 16 of 32 (unit entries 1/4) -- so its unit entries are exact in fp16 and every cosine is
an exact multiple of 1/32 (1/8 at dim 32) in fp32 whatever the summation order: host, device and oracle must agree bit for bit.  With 64 bins at dim
512 EVERY score sits exactly on a bin edge, the worst case for the bin rule."""
import numpy as np

PROBE_SHAPES = [(n, dim) for dim in (32, 512) for n in (1, 17, 129, 300)]
BINS = (64, 2, 4096, 100)


def support(dim):
    return np.arange(64) * 8 if dim == 512 else np.arange(16) * 2


def unit_f16(x):
    """the unit rows as the gallery stores them -- exact for these rows; a zero row stays zero"""
    nrm = np.sqrt((x.astype(np.float64) ** 2).sum(1, keepdims=True))
    return np.where(nrm > 0, x / np.where(nrm > 0, nrm, 1), 0).astype(np.float16)


def exact_case(n, dim, persons=7, seed=0):
    """-> g [n + 7, dim] float32 (seven free holes; hole `marker` is to hold the -0.0-first row of an empty slot, see with_marker), rows [n] int32
    (a shuffle, some entries outside the gallery or on holes), labels [n] int32 (position % persons, some unlabelled), plants {name: position(s)}.
    Planted, as far as n has room for them:
      dup_same (a, b)     the same row under the same label: s = 1, the top bin, and gen_score 1 unless a weaker partner exists
      dup_other (a, c)    the same row under another label: s = 1 on the impostor side
      negated (d, e)      row e = -row d: s = -1, bin 0
      unlabelled [..]     positions with label -1;  outside [..] rows outside [0, G);  hole [..] a free (zero) row;  marker: the -0.0 row
      lonely p            its label is its own: the position that would share it (p + persons) is unlabelled -> gen_via -1
      tie (t, u, v)       u < v hold the same row, one flip away from t's, under labels other than t's: two equal best impostors of t, the lower and
                          the higher one in different tiles of 128 when n >= 300 -> imp_via[t] = u"""
    rng = np.random.default_rng(1000 * seed + 10 * n + dim)
    sup = support(dim)
    x = np.zeros((n, dim), np.float32)
    x[:, sup] = rng.choice(np.float32([-1, 1]), (n, len(sup)))
    labels = (np.arange(n) % persons).astype(np.int32)
    G = n + 7
    perm = rng.permutation(G)
    rows = perm[:n].astype(np.int32)
    free = perm[n:]
    plants = {"marker_row": int(free[0])}
    if n >= 17:
        a, b, c = 1, 1 + persons, 3
        x[b] = x[a]
        x[c] = x[a]
        d, e = 4, 12
        x[e] = -x[d]
        plants.update(dup_same=(a, b), dup_other=(a, c), negated=(d, e))
        plants["unlabelled"] = [5, n - 2]
        labels[plants["unlabelled"]] = -1
        plants["outside"] = [6, 9]
        rows[6], rows[9] = G + 5, -1
        plants["hole"] = [10]
        rows[10] = free[1]
        plants["marker"] = [13]
        rows[13] = free[0]
        p = 2
        labels[p] = persons + 3                              # a label of its own ...
        if p + persons < n:
            labels[p + persons] = -1                         # ... whose other holder is unlabelled
            plants["unlabelled"].append(p + persons)
        plants["lonely"] = p
    if n >= 129:
        t, u, v = (150, 20, 280) if n >= 300 else (100, 20, 128)
        x[u] = x[t]
        x[u, sup[0]] = -x[u, sup[0]]
        x[v] = x[u]
        labels[t], labels[u], labels[v] = 0, 1, 2
        plants["tie"] = (t, u, v)
    g = np.zeros((G, dim), np.float32)
    inside = (rows >= 0) & (rows < G)
    keep = inside & ~np.isin(rows, free)
    g[rows[keep]] = x[keep]
    return g, rows, labels, plants


def with_marker(g16, plants):
    """the stored rows with the -0.0-first marker row of an empty slot in place"""
    g16 = np.ascontiguousarray(g16, np.float16).copy()
    g16.view(np.uint16)[plants["marker_row"], 0] = 0x8000
    return g16


def one_row_case(n=300, dim=64):
    """every position the same row: all n (n - 1) / 2 pairs score exactly 1 and land in ONE counter"""
    row = np.zeros(dim, np.float32)
    row[::4] = [1, -1] * (dim // 8)
    return np.tile(row, (n, 1))


def pack_case(g16, rows, labels, bins):
    """the input file of tests/calib_host_driver.cpp"""
    g16 = np.ascontiguousarray(g16, np.float16)
    G, dim = g16.shape
    n = G if rows is None else len(rows)
    out = np.array([G, dim, n, 0 if rows is None else 1, bins], np.int32).tobytes() + g16.tobytes()
    if rows is not None:
        out += np.ascontiguousarray(rows, np.int32).tobytes()
    return out + np.ascontiguousarray(labels, np.int32).tobytes()


NAMES = ("hist", "imp_via", "imp_score", "gen_via", "gen_score", "summary")


def same(got, want):
    """-> None, or the name of the first output that differs (scores compared as bits)"""
    for name, a, b in zip(NAMES, got, want):
        if name == "summary":
            if tuple(int(v) for v in a) != tuple(int(v) for v in b):
                return name
        elif name.endswith("score"):
            if not np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32)):
                return name
        elif not np.array_equal(np.asarray(a).astype(np.int64).ravel(), np.asarray(b).astype(np.int64).ravel()):
            return name
    return None
