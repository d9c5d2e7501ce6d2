"""Fixtures of the identity-template tests (CPU host twin, sanitizer driver, GPU): a case is a dict g16 fp16 [G, dim], rows int32 [n] or None,
labels int32 [n], weights int32 [n] or None, P, min_score.  KEEP_ALL (-2) switches trimming off."""
import struct

import numpy as np

from scrfd_arcface_facerecognition_amd._lib import TEMPLATE_CHUNK as CHUNK

KEEP_ALL = -2.0
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
ABOVE_ONE = float(np.nextafter(np.float32(1), np.float32(2)))


def gaussian_unit(seed, n, dim):
    x = np.random.default_rng(seed).standard_normal((n, dim))
    return (x / np.sqrt((x * x).sum(1, keepdims=True))).astype(np.float16)


def case(g16, rows, labels, weights, P, min_score=KEEP_ALL):
    i32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.int32)
    return dict(g16=np.ascontiguousarray(g16, np.float16), rows=i32(rows), labels=i32(labels), weights=i32(weights), P=int(P), min_score=float(min_score))


def n_of(c):
    return len(c["g16"]) if c["rows"] is None else len(c["rows"])


def sizes(dim):
    """the member counts at which the device takes another path: one lane, one batch of 64 and its neighbours, one chunk, a split person"""
    out = {"n1": case(gaussian_unit(1, 1, dim), None, [0], None, 1),
           "one_person_300": case(gaussian_unit(2, 300, dim), None, np.zeros(300), None, 1),
           "300_singletons": case(gaussian_unit(3, 300, dim), None, np.arange(300)[::-1], None, 300)}
    counts = [1, 2, 63, 64, 65, CHUNK, 2 * CHUNK + 1]
    rng = np.random.default_rng(4)
    labels = rng.permutation(np.repeat(np.arange(7), counts))
    n = len(labels)
    rows = rng.permutation(n + 5)[:n]
    rows[::9] = rows[1]                                                               # one row at many positions
    out["seven"] = case(gaussian_unit(5, n + 5, dim), rows, labels, rng.integers(1, 256, n), 7)
    out["seven_trimmed"] = dict(out["seven"], min_score=0.05)
    return out


def outside():
    """positions outside the rule, one at a time: 21 positions on a gallery of 12 rows, P = 3; positions 0 .. 5 are plain members"""
    g = gaussian_unit(6, 12, 32)
    b = g.view(np.uint16)
    g[6] = 0
    b[6, 3] = 0x8000                                                                  # an all-zero row (a -0.0 does not count)
    g[7, 5], g[8, 31] = np.inf, np.nan
    g[9, 0] = 2.0                                                                     # takes part
    b[10, 1] = 0x4001                                                                 # the next fp16 above 2.0: does not
    b[11, 2] = 0xC001                                                                 # ... nor its negative
    rows = [0, 1, 2, 3, 4, 5, I32_MIN, I32_MAX, 12, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11]
    labels = [0, 1, 2, 0, 1, 2, 0, 1, 2, -1, 3, I32_MAX, 0, 1, 2, 0, 1, 2, 0, 1, 2]
    weights = [1, 2, 3, 255, 9, 7, 1, 1, 1, 1, 1, 1, 0, -3, 256, 4, 4, 4, 4, 4, 4]
    return case(g, rows, labels, weights, 3)


def cancellation():
    g = gaussian_unit(7, 2, 512)
    g[1] = -g[0]
    return case(g, [0, 1, 0, 1], [0, 0, 0, 0], [7, 7, 100, 100], 1)


def planted_outlier():
    """three persons of 12 noisy copies of a centre; one face of person 1 is a stranger"""
    rng = np.random.default_rng(8)
    centres = rng.standard_normal((3, 512))
    x = np.repeat(centres, 12, axis=0) + 0.5 * rng.standard_normal((36, 512))
    x[17] = rng.standard_normal(512)
    g = (x / np.sqrt((x * x).sum(1, keepdims=True))).astype(np.float16)
    return case(g, None, np.repeat(np.arange(3), 12), rng.integers(1, 256, 36), 3, 0.5), 17


def opposed_pair():
    """a person of two faces with cosine < -0.5: both score sqrt((1 + c) / 2) < 0.5 against their mean; the second person is fine"""
    rng = np.random.default_rng(9)
    a = rng.standard_normal(512)
    b = -a + 0.3 * rng.standard_normal(512)
    x = np.stack([a, b, a, a + 0.1 * rng.standard_normal(512)])
    g = (x / np.sqrt((x * x).sum(1, keepdims=True))).astype(np.float16)
    assert float(g[0].astype(np.float64) @ g[1].astype(np.float64)) < -0.5
    return case(g, None, [0, 0, 1, 1], None, 2, 0.5)


def one_hot(min_score):
    """five persons, each a set of equal one-hot rows: the template is the row and every score is exactly 1.0f"""
    g = np.zeros((5, 32), np.float16)
    g[np.arange(5), [0, 7, 8, 30, 31]] = [1, -1, 1, 1, -1]
    rows = np.repeat(np.arange(5), [1, 2, 3, 70, 4])
    return case(g, rows, rows, np.arange(len(rows)) % 255 + 1, 5, min_score)


def random_rows(min_score=KEEP_ALL):
    rng = np.random.default_rng(10)
    n, P, dim = 1000, 37, 512
    return case(gaussian_unit(11, n, dim), None, rng.integers(0, P, n), rng.integers(1, 256, n), P, min_score)


def at_the_bound():
    """2^20 positions of weight 255 on two rows of +-2.0, two persons: all but one position are person 0 on row 0, so its sums reach
    (2^20 - 1) * 255 * 2^25, one position short of the header's bound, over 2^20 / CHUNK chunks"""
    g = np.full((2, 32), 2.0, np.float16)
    g[1, ::2] = -2.0
    n = 1 << 20
    labels = np.zeros(n, np.int32)
    labels[n // 3] = 1
    return case(g, labels.copy(), labels, np.full(n, 255), 2)


def permuted(c, seed=12):
    """the same case with its positions in another order -> (case, perm): position k of the new case is position perm[k] of the old one"""
    n = n_of(c)
    perm = np.random.default_rng(seed).permutation(n)
    rows = np.arange(n, dtype=np.int32) if c["rows"] is None else c["rows"]
    weights = None if c["weights"] is None else c["weights"][perm]
    return dict(c, rows=np.ascontiguousarray(rows[perm]), labels=np.ascontiguousarray(c["labels"][perm]), weights=weights), perm


def all_cases():
    out = {}
    for dim in (32, 512):
        out.update({f"{k}_dim{dim}": v for k, v in sizes(dim).items()})
    # wider rows: two and three blocks of 512 columns (the second, on the device, with an empty fourth block behind them)
    out.update(seven_trimmed_dim1024=sizes(1024)["seven_trimmed"], seven_trimmed_dim1536=sizes(1536)["seven_trimmed"])
    out.update(outside=outside(), cancellation=cancellation(), planted_outlier=planted_outlier()[0], opposed_pair=opposed_pair(),
               one_hot_at=one_hot(1.0), one_hot_above=one_hot(ABOVE_ONE), random=random_rows(), random_trimmed=random_rows(0.17))
    return out


NAMES = ("templates", "score", "kept", "person", "cohesion", "summary")


def same(got, want):
    """None, or which output differs first (compared as bytes: -0.0 is not +0.0)"""
    for name, a, b in zip(NAMES, got, want):
        if name == "summary":
            if tuple(int(v) for v in a) != tuple(int(v) for v in b):
                return f"summary {tuple(int(v) for v in a)} != {tuple(b)}"
            continue
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        if a.shape != b.shape or a.dtype.itemsize != b.dtype.itemsize:
            return f"{name}: {a.shape} {a.dtype} != {b.shape} {b.dtype}"
        u = {2: np.uint16, 4: np.uint32}[a.dtype.itemsize]
        bad = np.nonzero(a.view(u).reshape(-1) != b.view(u).reshape(-1))[0]
        if len(bad):
            return f"{name}: {len(bad)} differ, first at {int(bad[0])}: {a.reshape(-1)[bad[0]]!r} != {b.reshape(-1)[bad[0]]!r}"
    return None


def pack_case(c):
    """the input file of tests/template_host_driver.cpp"""
    g = c["g16"]
    n = n_of(c)
    head = struct.pack("<6if", g.shape[0], g.shape[1], n, c["rows"] is not None, c["weights"] is not None, c["P"], c["min_score"])
    return head + g.tobytes() + (b"" if c["rows"] is None else c["rows"].tobytes()) + c["labels"].tobytes() + \
        (b"" if c["weights"] is None else c["weights"].tobytes())
