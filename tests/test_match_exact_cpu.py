"""CPU: the host half of the exact probes for the gallery match family (tests/test_gpu_match_exact.py runs them on the device) -- the planted
fixtures, the float64 reference of fid_match / fid_gallery_topk / fid_cosine_matrix, the mirror of the kernel dispatch, the rounding rule for
fid_l2_normalize_f16 -- and the conditions that keep the device tests from passing vacuously, asserted here for every shape they run.

Probe rows (tests/test_gpu_range_join.py): 4, 16 or 64 entries of +-1, so the unit rows (+-0.5, +-0.25, +-0.125) are exact in fp16 and every cosine
is a multiple of 1/64, exact in fp32 whatever the summation order.  Planted on top of them, all from prototype 0 (16 non-zeros, support s[0..15]):
  row 0                      the prototype itself;
  pair k = rows (lo, hi)     two exact copies of the prototype with the support positions s[4 + b] flipped for every set bit b of k + 1 -- at
                             127 | 128, 255 | 256, both sides of every border the caller names (workgroup ranges of the 256 x 256 scan, shard
                             borders) and ((G - 1) // 2, G - 1).  Two different pairs are at cosine <= 0.875 from each other, so the query that
                             copies pair k has its maximum 1.0 at exactly lo and hi: the lower index must be reported;
  the pair's other queries   one more flip at s[0] = 0.875 to both rows, two more (s[0], s[1]) = 0.75 to both: an attained threshold AND a tie.
Ten rows from prototype 1 (the prototype, two one-flip, three two-flip, four three-flip variants, in shuffled row order) give the query that
copies prototype 1 the score ladder 1, .875 x 2, .75 x 3, .625 x 4: a tie across position k for k = 2, 4, 5, 8.  A third of the other rows are
copies of earlier rows (galleries beyond 4 096 rows: a 4 096-row block repeated, the odd rows negated in the repeats), so queries that copy a
gallery row tie across tiles and workgroup ranges all the time."""
import os
import re

import numpy as np
import pytest

from test_gpu_range_join import probe_rows, prototypes, unit_f16

CF_OUT_F32, CF_ARGMAX = 4, 8                        # csrc/conv.h:11-12
KS = (1, 2, 4, 5, 8)                                # the instantiated topk_rows<K> (csrc/match.hip:305)
BELOW = float(np.nextafter(np.float32(0.75), np.float32(0.0)))
BELOW_ONE = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
THRESHOLDS = (0.0, BELOW, 0.75, 0.4, BELOW_ONE, 1.0)  # (the last two: the strict '>' on a maximum of exactly 1.0, which query 0 has whatever n is)
BLOCK = 4096                                        # rows of the repeated block of a large gallery
SMALL_DIMS, SMALL_GS, SMALL_NS = (32, 64, 96, 512), (1, 33, 96, 127, 128, 129, 288, 300), (1, 17, 128, 129)
ZERO_ROW, NAN_QUERY = 3, 5                          # a deleted gallery row (G >= 33); where the match tests put their all-NaN query (n > 5)


def cdiv(a, b):
    return -(-a // b)


# ---- the dispatch mirror ---------------------------------------------------------------------------------------------------------------------------
def expected_path(n, Gp, dim, cus, flags, env=None):
    """The kernel gemm_vs_gallery (csrc/match.hip:135-163) launches for n queries against Gp padded rows: ("scan256",), ("rs", bm, bn, bk) = the
    register-staged conv_mfma_kernel, or ("dma", bm, bn, bk) = the LDS-DMA ring conv_mfma_dma_kernel.  env: the FID_* variables that are set
    (FID_CONV_V1 / FID_CONV_FORCE, experiment hooks of conv_plan, are not mirrored: the tests never set them)."""
    env = env or {}
    # csrc/match_gemm.hip:194-197 match_scan256_applicable (CK = 32, TG = TQ = 256), asked for at csrc/match.hip:136 (flags == CF_ARGMAX only)
    if flags == CF_ARGMAX and "FID_NO_MATCH256" not in env:
        if n > 128 and dim % 32 == 0 and dim >= 64 and cdiv(Gp, 256) * cdiv(n, 256) >= cus:
            return ("scan256",)
    # csrc/match.hip:159-161: the 128 x 128 x 64 override
    if cdiv(n, 128) * cdiv(Gp, 128) >= 2 * cus and dim % 64 == 0 and "FID_MATCH_DMA" not in env:
        return ("rs", 128, 128, 64)
    # csrc/conv.hip:798-807, conv_plan's generation-2 branch with M = n, Cin_p = dim, Cout_p = Gp (ksplit stays 1: allow_split is false)
    bk = 64 if dim % 64 == 0 else 32                                                  # :798
    bm = 128                                                                          # :799
    if Gp % 128 == 0:                                                                 # :800-803
        bn = 128
    elif Gp % 96 == 0:
        bn = 96
    elif Gp > 64:
        bn = 128
    else:
        bn = 64 if Gp > 32 else 32
    tiles = lambda: cdiv(n, bm) * cdiv(Gp, bn)
    if tiles() < cus and bn == 128:                                                   # :805
        bn = 64
    if tiles() < cus and bn == 64 and bk == 64:                                       # :806
        bm = 64
    if bk == 64 and bn not in (128, 64):                                              # :807
        bn = 128 if Gp > 64 else 64
    return ("dma", bm, bn, bk)


def klog_path(name):
    """a "[klog] kernel" name (csrc/ctx.hip:47; mangled or demangled) -> the tuple expected_path returns, or None for another kernel"""
    if "match_scan256" in name:
        return ("scan256",)
    m = re.search(r"conv_mfma_(dma_)?kernel(?:ILi|<)(\d+)(?:ELi|, ?)(\d+)(?:ELi|, ?)(\d+)", name)
    return ("dma" if m.group(1) else "rs", int(m.group(2)), int(m.group(3)), int(m.group(4))) if m else None


def scan_ranges(n, Gp, cus):
    """(rows per workgroup range, number of ranges) of match_scan256_launch (csrc/match_gemm.hip:203-206)"""
    n_qt, n_gt = cdiv(n, 256), cdiv(Gp, 256)
    ranges = max(1, min(n_gt, cus // n_qt))
    gt_per_wg = cdiv(n_gt, ranges)
    return 256 * gt_per_wg, cdiv(n_gt, gt_per_wg)


def large_shapes(cus):
    """{name: (Gp, G, dim, (n, ...))}: the smallest galleries that reach the large-gallery paths on `cus` compute units, G = Gp - 31 real rows
    but for the ragged tile.  "full" carries the override and ring shapes (n <= 128) next to the scan's (n > 128)."""
    out = {}
    for dim in (64, 96, 512):
        out["full%d" % dim] = (256 * cus, 256 * cus - 31, dim, (1, 128, 129, 256))    # one query tile, gt_per_wg = 1; n <= 128: override / ring
        out["half%d" % dim] = (128 * cus, 128 * cus - 31, dim, (257,))                # two query tiles, gt_per_wg = 1
    out["ragged_tile"] = (256 * cus - 224, 256 * cus - 224, 64, (129, 256))           # the last gallery tile has 32 rows, all of them real
    out["ragged_range"] = (256 * cus + 64, 256 * cus + 33, 96, (129, 256))            # gt_per_wg = 2, the last range holds one tile (33 real rows)
    return out


def shard_bounds(G, parts):
    """contiguous shards with borders that are no multiple of 128.  Three parts: two of about G / 2 rows and a last one of 201 rows (with 257
    queries the first two take the 256 x 256 scan, the last one the generic GEMM); otherwise equal parts."""
    b = [0, G // 2 - 59, G - 201, G] if parts == 3 else [G * i // parts for i in range(parts + 1)]
    b = [0] + [x + 37 if x % 128 == 0 else x for x in b[1:-1]] + [G]
    assert all(lo < hi for lo, hi in zip(b, b[1:])) and all(x % 128 for x in b[1:-1])
    return b


def large_case(name, cus):
    """-> (gallery rows, info, Gp, dim, ns) of one of large_shapes: a planted pair in front of every workgroup-range border of the scan and, in the
    gallery the shard tests use (full64), of the shard borders of both splits; info["tail"] = the first row of the scan's last workgroup range
    (the last gallery tile where gt_per_wg = 1), which holds a pair of its own and a row that is one query's only maximum"""
    Gp, G, dim, ns = large_shapes(cus)[name]
    shards = sorted(set(shard_bounds(G, 3)[1:-1]) | set(shard_bounds(G, 8)[1:-1])) if name == "full64" else []
    step = 512 if name == "ragged_range" else 256
    tail = (cdiv(Gp, step) - 1) * step
    assert G - tail >= 32
    g, info = build_gallery(G, dim, Gp + dim, sorted(set(range(step, G, step)) | set(shards)), shards, tail)
    return g, info, Gp, dim, ns


# ---- fixtures --------------------------------------------------------------------------------------------------------------------------------------
def pair_flips(k):
    return tuple(4 + b for b in range(12) if (k + 1) >> b & 1)


LADDER = ((), (0,), (1,), (0, 1), (2, 3), (4, 5), (0, 1, 2), (3, 4, 5), (6, 7, 8), (9, 10, 11))


def variant(proto, flips):
    v = proto[0].copy()
    v[proto[1][list(flips)]] *= -1
    return v


def build_gallery(G, dim, seed, borders=(), marked=(), tail=None):
    """-> (fp32 [G, dim] probe rows with the planted structure of the module docstring, info for build_queries); the pairs in front of the
    `marked` borders get a query each whatever n is (n >= 17).  tail: rows tail + 2 and tail + 9 become one more pair and row tail + 5 a variant
    no other row shares (a "pair" with lo == hi), both with a query: answers that only the rows from `tail` on can give."""
    rng = np.random.default_rng(seed)
    protos = prototypes(rng, dim)
    if G <= BLOCK:
        g = probe_rows(rng, G, dim, protos[2:], {})
        later = [r for r in range(1, G) if rng.random() < 1 / 3]
        for r in later:
            g[r] = g[int(rng.integers(0, r))]
    else:
        blk = probe_rows(rng, BLOCK, dim, protos[2:], {})
        g = np.tile(blk, (cdiv(G, BLOCK), 1))[:G]
        g[BLOCK + 1::2] *= -1                                                     # (BLOCK is even: the odd rows of every repeat)
        later = [int(r) for r in BLOCK + 2 * rng.integers(0, (G - BLOCK) // 2, 64)]
    used = {0}
    g[0] = protos[0][0]
    if G >= 33:
        g[ZERO_ROW] = 0.0
        used.add(ZERO_ROW)
    pairs = []
    in_tail = [] if tail is None else [(tail + 2, tail + 9), (tail + 5, tail + 5)]
    marked = set(marked) | {hi for _, hi in in_tail}
    for lo, hi in [(127, 128), (255, 256)] + [(b - 1, b) for b in borders] + in_tail + [((G - 1) // 2, G - 1)]:
        if 0 < lo <= hi < G and lo not in used and hi not in used:
            g[lo] = g[hi] = variant(protos[0], pair_flips(len(pairs)))
            pairs.append((lo, hi))
            used |= {lo, hi}
    free = [int(r) for r in rng.permutation(G) if r not in used][:len(LADDER)]
    if len(free) == len(LADDER):
        for r, flips in zip(free, LADDER):                                        # (free is in shuffled order: score order is not row order)
            g[r] = variant(protos[1], flips)
    else:
        free = []
    later = [r for r in later if r not in used and r not in free]
    return g, dict(protos=protos, pairs=pairs, later=later, ladder=free, tail=tail, marked=[k for k, (lo, hi) in enumerate(pairs) if hi in marked])


def build_queries(n, g, info, seed):
    """fp32 [n, dim]: the first rows are the planted queries in a fixed order (so that a prefix of 1, 3, 5 or 17 rows holds what its test needs),
    the others alternate between copies of gallery rows that have an earlier copy and fresh probe rows"""
    rng = np.random.default_rng(seed)
    protos, pairs, dim = info["protos"], info["pairs"], g.shape[1]
    p0 = protos[0]
    flips = [pair_flips(k) for k in range(len(pairs))]
    head = [variant(p0, flips[0]) if pairs else p0[0].copy(),                     # 0: 1.0 at both rows of the first pair (row 0 if there is none)
            variant(p0, (flips[0] if pairs else ()) + (0, 1)),                    # 1: exactly 0.75 to them
            np.zeros(dim, np.float32),                                            # 2: a zero query: every score 0
            protos[1][0].copy(),                                                  # 3: the ladder
            variant(p0, flips[1]) if len(pairs) > 1 else variant(p0, (0,)),       # 4: the second pair (255 | 256 where G > 256)
            -p0[0],                                                               # 5: (the match tests overwrite it with NaNs)
            variant(p0, flips[-1]) if pairs else variant(p0, (1,)),               # 6: the pair that ends in the last real row
            variant(p0, (flips[-1] if pairs else ()) + (0,)),                     # 7: 0.875 to it
            -protos[1][0]]                                                        # 8: every ladder row at or below 0
    sampled = list(np.unique(np.linspace(0, len(pairs) - 1, max(24, n // 3)).astype(int))) if pairs else []
    for k in info["marked"] + sampled:                                            # 9 ...: the marked pairs, then a third of the queries on pairs
        head.append(variant(p0, flips[k] + ((0, 1) if k % 3 == 2 and k not in info["marked"] else ())))   # spread evenly over the gallery
    q = probe_rows(rng, n, dim, protos[2:], {})
    if info["later"]:
        for i in range(0, n, 2):
            q[i] = g[info["later"][int(rng.integers(0, len(info["later"])))]]
    m = min(n, len(head))
    q[:m] = np.stack(head[:m])
    return q


def f16_nan_row(dim):
    return np.full(dim, np.nan, np.float16)


# ---- the reference ---------------------------------------------------------------------------------------------------------------------------------
def cosines(q16, g16):
    """[n, G] cosines of fp16 unit rows.  float64; beyond 2^22 products float32, which is exact as well for probe rows: every product is a multiple
    of 1/64 below 1 and every partial sum of at most 512 of them a multiple of 1/64 below 2^9, which 24 bits hold.  (NaN queries give NaN rows.)"""
    t = np.float64 if q16.shape[0] * g16.shape[0] <= 1 << 22 else np.float32
    with np.errstate(invalid="ignore"):
        return q16.astype(t) @ g16.astype(t).T


def ref_match(S, thresh):
    """fid_match: the first index of the row maximum if it is > 0 and > thresh, else (-1, 0.0); a NaN score never wins"""
    Sm = np.where(np.isnan(S), -np.inf, S)
    j = Sm.argmax(1)                                                              # (numpy: the first maximum)
    m = Sm[np.arange(len(S)), j]
    ok = (m > 0) & (m > np.float32(thresh))
    return np.where(ok, j, -1).astype(np.int32), np.where(ok, m, 0.0).astype(np.float32)


def ref_topk(S, k, thresh):
    """fid_gallery_topk: the k best (-score, index) pairs with score > max(0, thresh), padded with (-1, 0.0)"""
    idx, sc = np.full((len(S), k), -1, np.int32), np.zeros((len(S), k), np.float32)
    floor_ = max(0.0, float(np.float32(thresh)))
    for i, s in enumerate(S):
        cand = np.argpartition(-s, min(k + 64, len(s) - 1))[:k + 65] if len(s) > 4 * (k + 65) else np.arange(len(s))
        if len(cand) < len(s):                                                    # (the partition may cut a run of equal scores: take all of it)
            cand = np.flatnonzero(s >= s[cand].min())
        order = cand[np.lexsort((cand, -s[cand]))][:k]
        order = order[s[order] > floor_]
        idx[i, :len(order)], sc[i, :len(order)] = order, s[order]
    return idx, sc


def ref_cosine_matrix(S, Gp):
    out = np.zeros((S.shape[0], Gp), np.float32)
    out[:, :S.shape[1]] = S
    return out


def conditions(S, range_rows=None, tail=None):
    """what the fixtures have to offer, from the reference scores of the queries without NaNs.  range_rows: the rows of a workgroup range of the
    scan; tail: the first row of the last one"""
    n, G = S.shape
    m = S.max(1)
    winners = [np.flatnonzero(S[i] == m[i]) for i in range(n)]
    tied = [w for w, mx in zip(winners, m) if len(w) >= 2 and mx > 0]
    top = -np.sort(-S, axis=1)[:, :9] if G <= 4 * BLOCK else -np.sort(np.partition(-S, 9, axis=1)[:, :9], axis=1)
    first = [w[0] for w, mx in zip(winners, m) if mx > 0]                          # the rows fid_match reports at threshold 0
    cut = S.copy()
    cut[:, G if tail is None else tail:] = 0.0                                    # ... and what it would report were the tail all zeros
    return dict(tail_unique=tail is not None and any(len(w) == 1 and w[0] >= tail and mx > 0 for w, mx in zip(winners, m)),
                tail_tie=tail is not None and any(w[0] >= tail for w in tied),
                tail_matters=int((ref_match(cut, 0.0)[0] != ref_match(S, 0.0)[0]).sum()),
                ranges_won=sorted({r // range_rows for r in first}) if range_rows else [],
                tie_share=len(tied) / n,
                seam128=any(w[0] % 128 == 127 and w[1] == w[0] + 1 for w in tied),
                seam256=any(w[0] % 256 == 255 and w[1] == w[0] + 1 for w in tied),
                ranges=range_rows is not None and any(w[0] // range_rows != w[-1] // range_rows for w in tied),
                attained=bool((m == 0.75).any()), not_attained=bool((m != 0.75).any()), nonpositive=bool((m <= 0).any()),
                topk={k: bool(G > k and ((top[:, k - 1] == top[:, k]) & (top[:, k] > 0.05)).any()) for k in KS})


def small_case(G, dim, n):
    g = build_gallery(G, dim, 1000 * G + dim)
    q = build_queries(n, g[0], g[1], 10 * n + dim)
    return g[0], q, g[1]


# ---- the rounding rule of fid_l2_normalize_f16 -----------------------------------------------------------------------------------------------------
def normalise_rule(out16, x):
    """-> (elements that break the rule, share of excepted elements).  The rule: out == float16(x / norm) with the quotient in float64, except where
    that quotient lies within relative 1e-6 of the midpoint of two neighbouring fp16 values -- there either neighbour is accepted (an fp32
    evaluation carries a relative error of a few 2^-24 into the fp16 rounding, which only matters that close to a midpoint)."""
    x = x.astype(np.float64)
    want = x / np.sqrt((x * x).sum(1, keepdims=True))
    near = want.astype(np.float16)
    other = np.nextafter(near, np.where(want >= near.astype(np.float64), np.float16(np.inf), np.float16(-np.inf)).astype(np.float16))
    mid = (near.astype(np.float64) + other.astype(np.float64)) / 2
    excepted = np.abs(want - mid) <= 1e-6 * np.abs(mid)
    good = (out16 == near) | (excepted & (out16 == other))
    return int((~good).sum()), float(excepted.mean())


def normal_rows(n, dim):
    """random normal rows scaled by 1e-3, 1 and 1e3 in turn.  (Seed dim + 1: about 0.3 % of all elements fall under the exception of normalise_rule, but
    a prefix of three rows of 32 holds 96 elements and a single excepted one is more than the 1 % it may be -- which a seed's inputs alone decide.)"""
    x = np.random.default_rng(dim + 1).standard_normal((n, dim)).astype(np.float32)
    return x * np.float32([1e-3, 1.0, 1e3])[np.arange(n) % 3][:, None]


def degenerate_rows(dim):
    """[5, dim]: all zero, one NaN, one inf, squares that overflow fp32, squares that underflow to zero -- each becomes an all-+0.0 row"""
    x = np.random.default_rng(dim).standard_normal((5, dim)).astype(np.float32)
    x[0] = 0.0
    x[1, dim // 2] = np.nan
    x[2, dim - 1] = np.inf
    x[3] = 1e20
    x[4] = 1e-25
    return x


SLOT_F, SLOT_COUNTS = 5, (5, 0, 3, 1, 5, 2, 4, 0, 1)  # the face slots of the device test: 45 rows, the last block of four holds one
MARKER = 0x8000                                     # an empty slot: -0.0 first, then +0.0 (include/faceid.h, fid_l2_normalize_f16_slots)


def marker_row(dim):
    r = np.zeros(dim, np.uint16)
    r[0] = MARKER
    return r


# ---- tests -----------------------------------------------------------------------------------------------------------------------------------------
def test_unit_rows_are_exact():
    for dim in SMALL_DIMS:
        g, q, _ = small_case(300, dim, 129)
        for x in (g, q):
            x = x[np.abs(x).sum(1) > 0]
            assert set(np.abs(x).sum(1)) <= {4.0, 16.0, 64.0}
            assert np.array_equal(unit_f16(x).astype(np.float64), x.astype(np.float64) / np.sqrt((x.astype(np.float64) ** 2).sum(1, keepdims=True)))
        S = cosines(unit_f16(q), unit_f16(g))
        assert S.dtype == np.float64 and np.array_equal(S * 64, np.round(S * 64))
        assert np.array_equal(S, unit_f16(q).astype(np.float32) @ unit_f16(g).astype(np.float32).T)     # ... and float32 sums are exact too


@pytest.mark.parametrize("dim", SMALL_DIMS)
@pytest.mark.parametrize("G", SMALL_GS)
def test_small_fixtures_meet_their_conditions(G, dim):
    """For every n of the device test.  What cannot hold is left out by rule, not by looking at results: a tie needs two real rows (G >= 33 of the
    list), a 128-row seam G > 128; one query (n = 1) is the first planted query alone and must be its tie, the other conditions need n = 17."""
    for n in SMALL_NS:
        g, q, info = small_case(G, dim, n)
        S = cosines(unit_f16(q), unit_f16(g))
        c = conditions(S)
        want0 = info["pairs"][0][0] if info["pairs"] else 0
        assert ref_match(S, 0.0)[0][0] == want0 and S[0, want0] == 1.0
        if G == 1:
            assert S.shape[1] == 1 and (n < 3 or (S[1, 0] == 0.75 and S[2, 0] == 0.0))
            continue
        assert S[0, info["pairs"][0][1]] == 1.0                                   # query 0 aims at the higher copy and must get the lower
        assert ref_match(S[:1], BELOW_ONE)[0][0] == want0 and ref_match(S[:1], 1.0)[0][0] == -1      # the strict threshold on query 0's own maximum
        if n == 1:
            assert c["tie_share"] == 1.0 and (G <= 128 or c["seam128"])
            continue
        assert c["tie_share"] >= 0.25, c
        assert c["seam128"] == (G > 128), c
        assert c["seam256"] == (G > 256), c
        assert c["attained"] and c["not_attained"] and c["nonpositive"], c
        assert all(c["topk"].values()), c
        hi = info["pairs"][-1][1]
        assert hi == G - 1 and ref_match(S[6:7], 0.0)[0][0] == info["pairs"][-1][0]      # the last real row is the higher copy of a pair
        assert ref_match(S[1:2], BELOW)[0][0] >= 0 and ref_match(S[1:2], 0.75)[0][0] == -1


@pytest.mark.parametrize("cus", [256, 40])
def test_large_fixtures_meet_their_conditions(cus):
    """... and, so that no part of a large gallery can be dropped or zeroed unseen: the last workgroup range of the scan (the ragged tile / range
    where there is one) holds a row that is one query's only maximum and the lower row of a tie, and the reported rows fall in at least n / 4
    different workgroup ranges (all of them where there are fewer), the first and the last among them.  (n queries reach at most n ranges; the fixed planted queries and the
    copies of repeated rows, whose first copy lies in the first 4 096 rows, take more than half of them.)"""
    for name, (Gp, G, dim, ns) in large_shapes(cus).items():
        g, info = large_case(name, cus)[:2]
        g16 = unit_f16(g)
        assert len(g) == G and 0 < Gp - G < 32 or name == "ragged_tile" and G == Gp and G - info["tail"] == 32
        for n in ns:
            S = cosines(unit_f16(build_queries(n, g, info, 10 * n + dim)), g16)
            path = expected_path(n, Gp, dim, cus, CF_ARGMAX)
            if n == 1:
                assert path == (("rs", 128, 128, 64) if dim % 64 == 0 else ("dma", 128, 128, 32)) and (S[0] == 1.0).sum() == 2
                continue
            range_rows, R = scan_ranges(max(n, 129), Gp, cus)
            c = conditions(S, range_rows, info["tail"])
            assert info["tail"] == (R - 1) * range_rows and c["tail_unique"] and c["tail_tie"] and c["tail_matters"] >= 2, (name, n, c)
            assert len(c["ranges_won"]) >= min(n // 4, R) and c["ranges_won"][0] == 0 and c["ranges_won"][-1] == R - 1, (name, n, c["ranges_won"])
            assert c["tie_share"] >= 0.25 and c["seam128"] and c["attained"] and c["not_attained"] and c["nonpositive"], (name, n, c)
            assert all(c["topk"].values()), (name, n, c)
            if n > 128:
                assert path == ("scan256",) and c["seam256"] and c["ranges"], (name, n, c)
                assert range_rows == (512 if name == "ragged_range" else 256) and R == cdiv(cdiv(Gp, 256), range_rows // 256)
            else:
                assert path == (("rs", 128, 128, 64) if dim % 64 == 0 else ("dma", 128, 128, 32))
            assert expected_path(n, Gp, dim, cus, CF_ARGMAX, {"FID_NO_MATCH256": "1"})[0] == ("rs" if dim % 64 == 0 else "dma")
            assert expected_path(n, Gp, dim, cus, CF_ARGMAX, {"FID_NO_MATCH256": "1", "FID_MATCH_DMA": "1"})[0] == "dma"
    Gp = 256 * cus
    assert Gp % 256 == 0 and cdiv(Gp - 224, 256) == cus and (Gp - 224) % 256 == 32      # the ragged tile holds 32 rows
    assert scan_ranges(256, Gp + 64, cus) == (512, cus // 2 + 1) and cdiv(Gp + 64, 256) % 2 == 1   # ... the ragged range one tile


@pytest.mark.parametrize("cus", [256, 40])
def test_shards_take_the_paths_the_test_is_about(cus):
    G, n = 256 * cus - 31, 257
    b3, b8 = shard_bounds(G, 3), shard_bounds(G, 8)
    paths = [expected_path(n, cdiv(hi - lo, 32) * 32, 64, cus, CF_ARGMAX)[0] for lo, hi in zip(b3, b3[1:])]
    assert paths == ["scan256", "scan256", "dma"]
    assert all(expected_path(n, cdiv(hi - lo, 32) * 32, 64, cus, CF_ARGMAX)[0] != "scan256" for lo, hi in zip(b8, b8[1:]))
    g, info = large_case("full64", cus)[:2]
    S = cosines(unit_f16(build_queries(n, g, info, 10 * n + 64)), unit_f16(g))
    for b in (b3, b8):
        for border in b[1:-1]:
            assert (border - 1, border) in info["pairs"]
        shard_of = lambda r: np.searchsorted(b, r, side="right")
        tied = [w for w in (np.flatnonzero(S[i] == S[i].max()) for i in range(n) if S[i].max() > 0) if len(w) >= 2]
        assert any(w[1] == w[0] + 1 and shard_of(w[0]) != shard_of(w[1]) for w in tied)          # a planted pair across a shard border
        assert sum(shard_of(w[0]) != shard_of(w[-1]) for w in tied) >= n // 4


def test_expected_path_on_known_shapes():
    A, F = CF_ARGMAX, CF_OUT_F32
    assert expected_path(129, 65536, 64, 256, A) == ("scan256",)
    assert expected_path(128, 65536, 64, 256, A) == ("rs", 128, 128, 64)                 # n <= 128: never the scan
    assert expected_path(129, 65536, 32, 256, A) == ("dma", 128, 128, 32)                # dim < 64: never the scan, dim % 64: never the override
    assert expected_path(129, 65536 - 256, 64, 256, A) == ("rs", 128, 128, 64)           # one tile short of the scan: two query tiles of 128
    assert expected_path(128, 65536 - 256, 64, 256, A) == ("dma", 128, 128, 64)          # ... and of the override
    assert expected_path(300, 65536, 64, 256, F) == ("rs", 128, 128, 64)                 # the scan serves the arg-max only
    assert expected_path(3, 65536, 512, 256, F) == ("rs", 128, 128, 64)
    assert expected_path(3, 65536, 512, 256, F, {"FID_MATCH_DMA": "1"}) == ("dma", 128, 128, 64)
    assert expected_path(17, 96, 32, 256, A) == ("dma", 128, 96, 32) == expected_path(17, 288, 96, 256, F)
    assert expected_path(17, 96, 64, 256, A) == ("dma", 128, 128, 64)                    # no 96-wide tile at bk = 64
    assert expected_path(17, 32, 32, 256, A) == ("dma", 128, 32, 32) and expected_path(17, 32, 64, 256, A) == ("dma", 128, 64, 64)
    assert expected_path(17, 64, 96, 256, A) == ("dma", 128, 64, 32)
    assert expected_path(17, 128, 64, 256, A) == ("dma", 64, 64, 64) and expected_path(17, 128, 96, 256, A) == ("dma", 128, 64, 32)
    assert expected_path(129, 320, 512, 256, A) == ("dma", 64, 64, 64) and expected_path(129, 160, 32, 256, F) == ("dma", 128, 64, 32)
    # every tile the mirror can name for the device tests' shapes is one csrc/conv.hip instantiates (GEMM_TILES, :765-777)
    have = {(128, 128, 64), (128, 64, 64), (64, 64, 64), (128, 128, 32), (128, 96, 32), (128, 64, 32), (128, 32, 32)}
    for dim in SMALL_DIMS:
        for G in SMALL_GS:
            for n in SMALL_NS:
                for f in (A, F):
                    assert expected_path(n, cdiv(G, 32) * 32, dim, 256, f)[1:] in have
    for dim in (32, 96):
        for G in (96, 288):
            assert expected_path(17, G, dim, 256, A) == ("dma", 128, 96, 32)             # the 96-wide column tile
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scrfd_arcface_facerecognition_amd", "csrc", "conv.h")
    text = open(src).read()
    assert "CF_OUT_F32 = %d," % F in text and "CF_ARGMAX = %d," % A in text


def test_klog_names():
    assert klog_path("_ZN3fid12_GLOBAL__N_113match_scan256ENS0_6MGArgsE") == ("scan256",)
    assert klog_path("_ZN3fid12_GLOBAL__N_116conv_mfma_kernelILi128ELi128ELi64ELi2ELi2EEEvNS_8ConvArgsE") == ("rs", 128, 128, 64)
    assert klog_path("void fid::(anonymous namespace)::conv_mfma_dma_kernel<128, 96, 32, 4, 2, 2, false>(fid::ConvArgs)") == ("dma", 128, 96, 32)
    assert klog_path("_ZN3fid12_GLOBAL__N_114match_finalizeEPKyiiifPiPf") is None


def test_reference_on_a_hand_made_case():
    S = np.array([[0.5, 0.75, 0.75, 0.25], [0.0, -0.5, 0.0, -1.0], [np.nan] * 4, [1.0, 1.0, 1.0, 1.0]])
    i, s = ref_match(S, 0.4)
    assert i.tolist() == [1, -1, -1, 0] and s.tolist() == [0.75, 0.0, 0.0, 1.0]
    assert ref_match(S, 0.75)[0].tolist() == [-1, -1, -1, 0] and ref_match(S, BELOW)[0].tolist() == [1, -1, -1, 0]
    assert ref_match(S, -1.0)[0].tolist() == [1, -1, -1, 0]                                   # never a match at or below 0
    i, s = ref_topk(S[[0, 1, 3]], 2, 0.05)
    assert i.tolist() == [[1, 2], [-1, -1], [0, 1]] and s.tolist() == [[0.75, 0.75], [0.0, 0.0], [1.0, 1.0]]
    i, s = ref_topk(S[[0]], 5, 0.3)
    assert i.tolist() == [[1, 2, 0, -1, -1]] and s.tolist() == [[0.75, 0.75, 0.5, 0.0, 0.0]]
    assert ref_topk(S[[0]], 1, 0.75)[0].tolist() == [[-1]]
    big = np.zeros((1, 5000))
    big[0, [4999, 17, 300]] = 0.5                                                             # a run of equal scores beyond the partition's cut
    big[0, 1000:1200] = 0.25
    assert ref_topk(big, 8, 0.05)[0].tolist() == [[17, 300, 4999, 1000, 1001, 1002, 1003, 1004]]
    assert ref_cosine_matrix(S[:1], 32).shape == (1, 32) and not ref_cosine_matrix(S[:1], 32)[:, 4:].any()


@pytest.mark.parametrize("dim", [32, 96, 500, 512])
def test_float32_numpy_meets_the_rounding_rule(dim):
    """the rule asked of the device is one plain fp32 arithmetic can meet: numpy's own float32 evaluation of the same quotient, on the same rows"""
    x = normal_rows(1023, dim)
    out = (x / np.sqrt((x * x).sum(1, keepdims=True, dtype=np.float32))).astype(np.float16)
    assert out.dtype == np.float16 and (x * x).dtype == np.float32
    for n in (1, 3, 4, 5, 1023):                                                              # the prefixes the device tests normalise
        bad, excepted = normalise_rule(out[:n], x[:n])
        assert bad == 0 and excepted < 0.01, (n, bad, excepted)
    valid = np.concatenate([np.arange(SLOT_F) < c for c in SLOT_COUNTS])
    assert normalise_rule(out[:45][valid], x[:45][valid])[1] < 0.01                           # ... and the valid face slots
    wrong = out.copy()
    wrong[5, 7] = np.nextafter(wrong[5, 7], np.float16(1.0))                                  # one ulp off is seen
    assert normalise_rule(wrong, x)[0] == 1
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        d = degenerate_rows(dim)
        nrm = np.sqrt((d * d).sum(1, dtype=np.float32))
    assert nrm[0] == 0 and np.isnan(nrm[1]) and np.isinf(nrm[2]) and np.isinf(nrm[3]) and nrm[4] == 0   # none has a norm in (0, inf)
