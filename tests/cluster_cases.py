"""Stores for the clustering tests (test_cluster_cpu.py, test_cluster_host_sanitized.py, test_gpu_cluster.py), numpy only.  Every row is +-1 / 0
with 4 or 16 (or 64) non-zeros, so its unit entries are exact in fp16 and every cosine is an exact multiple of 1/64 in fp32 whatever the summation
order: host, device and oracle must agree bit for bit, also at a threshold that is itself attained."""
import numpy as np

ABOVE = float(np.nextafter(np.float32(0.75), np.float32(1.0)))
PROBE_SHAPES = [(n, dim) for dim in (32, 512) for n in (1, 17, 129, 300)]


def unit_f16(x):
    """the unit rows as the gallery stores them -- exact for these rows; a zero row stays zero"""
    nrm = np.sqrt((x.astype(np.float64) ** 2).sum(1, keepdims=True))
    return np.where(nrm > 0, x / np.where(nrm > 0, nrm, 1), 0).astype(np.float16)


def probe_case(n, dim):
    """test_gpu_dedup.probe_case: g [n + 7, dim] with seven free holes, rows [n] a shuffle (not ascending), planted pairs inside a block, across
    the 127 | 128 seam and two blocks apart (positions 5 and 290, exactly 0.75)"""
    from test_gpu_dedup import probe_case as case
    return case(n, dim)


def path_case(n, dim, seed=0):
    """sliding windows: path row t has +1 at columns t .. t + 3 (unit entries 0.5): neighbours score exactly 0.75, two apart 0.5, further apart
    <= 0.25.  Positions are shuffled, so the path zigzags between the blocks of 128; position 0 holds an END of the path.
    -> g [n + 5, dim], rows [n], t_of [n] (the path row at every position)"""
    assert n + 3 <= dim
    rng = np.random.default_rng(seed + n)
    t_of = rng.permutation(n)
    k = int(np.nonzero(t_of == 0)[0][0])
    t_of[[0, k]] = t_of[[k, 0]]
    x = np.zeros((n, dim), np.float32)
    for pos, t in enumerate(t_of):
        x[pos, t:t + 4] = 1
    rows = rng.permutation(n + 5)[:n].astype(np.int32)
    g = np.zeros((n + 5, dim), np.float32)
    g[rows] = x
    return g, rows, t_of


def tie_case(equal, p_low, n=260, dim=32):
    """Two cores P and Q of DIFFERENT clusters (P.Q = 0.5) and one non-core row x between them, for thresh 0.625 and min_pts 4:
    equal: x.P = x.Q = 0.75; otherwise x.P = 0.875 and x.Q = 0.625.  P and Q get two more neighbours each (three flips: 0.625, borders; at most 0.5 from x), so that their degree
    is 4 and x's is 3.  p_low: P sits at the lower position.  The seven rows are spread over three blocks of 128; every other position is a
    zero row, a row outside the gallery or a free hole.  -> g, rows, positions {name: position}"""
    sup = np.arange(16) * 2                                  # 16 of the 32 columns
    def row(flips):
        r = np.zeros(dim, np.float32)
        r[sup] = 1
        r[sup[list(flips)]] = -1
        return r
    P, Q = row(()), row((0, 1, 2, 3))
    x = row((0, 1)) if equal else row((0,))
    lo, hi = 3, 200
    pos = {"P": lo if p_low else hi, "Q": hi if p_low else lo, "x": 130, "p2": 127, "p3": 128, "q2": 64, "q3": 259}
    vec = {"P": P, "Q": Q, "x": x, "p2": row((4, 5, 6)), "p3": row((7, 8, 9)), "q2": row((0, 1, 2, 3, 10, 11, 12)),
           "q3": row((0, 1, 2, 3, 13, 14, 15))}
    G = 40
    g = np.zeros((G, dim), np.float32)
    rows = np.full(n, -1, np.int32)
    rows[1::3] = G + 5                                       # outside the gallery
    rows[2::3] = 39                                          # a zero row (many positions name it: it takes no part)
    for k, (name, p) in enumerate(pos.items()):
        g[5 * k + 1] = vec[name]
        rows[p] = 5 * k + 1
    return g, rows, pos


def chain_case(order):
    """A ~ B ~ C with A !~ C at thresh 0.75 (sliding windows 0, 1, 2), stored under the ids order[0], order[1], order[2].
    -> g [3, 32] in ascending id order (position k = the k-th lowest id), name_of [3] (which of A, B, C sits at position k)"""
    x = np.zeros((3, 32), np.float32)
    name_of = [None] * 3
    for t, name in enumerate("ABC"):
        k = sorted(order).index(order[t])
        x[k, t:t + 4] = 1
        name_of[k] = name
    return x, name_of


def pack_case(g16, rows, thresh, min_pts):
    """the input file of tests/cluster_host_driver.cpp"""
    g16 = np.ascontiguousarray(g16, np.float16)
    G, dim = g16.shape
    n = G if rows is None else len(rows)
    out = np.array([G, dim, n, 0 if rows is None else 1, min_pts], np.int32).tobytes() + np.array([thresh], np.float32).tobytes() + g16.tobytes()
    if rows is not None:
        out += np.ascontiguousarray(rows, np.int32).tobytes()
    return out


def same(got, want):
    """-> None, or the name of the first output that differs (scores compared as bits)"""
    for name, a, b in zip(("label", "degree", "via"), got[:3], want[:3]):
        if not np.array_equal(np.asarray(a, np.int32), np.asarray(b, np.int32)):
            return name
    if not np.array_equal(np.asarray(got[3], np.float32).view(np.uint32), np.asarray(want[3], np.float32).view(np.uint32)):
        return "score"
    if tuple(int(v) for v in got[4]) != tuple(int(v) for v in want[4]):
        return "summary"
    return None
