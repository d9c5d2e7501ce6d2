"""GPU: fid_gallery_range (range search and self-join, csrc/range_join.hip) and the Python layer above it.

Exact probes: rows with exactly 4, 16 or 64 non-zero entries of +-1 have norm 2, 4 or 8, so their unit entries (+-0.5, +-0.25, +-0.125) are exact in
fp16 and every cosine is an exact multiple of 1/64 in fp32 whatever the summation order -- the hit set and the scores must equal a float64 reference
bit for bit, including at thresholds that are themselves attained.  Rows derived from one prototype by sign flips sit at 1 - |flips differ| / 8
from each other (1, 0.875, 0.75, 0.625 ...); they are planted at the last row / column and on both sides of the tile seam at 127 | 128."""
import ctypes as C

import numpy as np
import pytest

from oracle import match
from test_range_join_cpu import duplicate_store

pytestmark = pytest.mark.gpu

CANARY = 0x7B


@pytest.fixture(scope="module")
def ctx():
    from scrfd_arcface_facerecognition_amd._lib import Context
    c = Context(0)
    yield c
    c.close()


# ---- fixtures on the host ------------------------------------------------------------------------------------------------------------------------
def prototypes(rng, dim):
    """six rows of 16 non-zero +-1 entries -> [(row, support)]"""
    out = []
    for _ in range(6):
        sup = rng.permutation(dim)[:16]
        p = np.zeros(dim, np.float32)
        p[sup] = rng.choice([-1.0, 1.0], 16)
        out.append((p, sup))
    return out


def probe_rows(rng, rows, dim, protos, special):
    """[rows, dim] of +-1 / 0 with 4, 16 or 64 non-zeros per row (64 only where dim has room).  About a quarter of the rows are variants of the
    prototypes (up to three sign flips); `special` = {row: flip positions within prototype 0's support} fixes the planted rows."""
    x = np.zeros((rows, dim), np.float32)
    sizes = [4, 16, 64] if dim >= 96 else [4, 16]
    for r in range(rows):
        if rng.random() < 0.25:
            p, sup = protos[int(rng.integers(0, len(protos)))]
            x[r] = p
            x[r, rng.permutation(sup)[:int(rng.integers(0, 4))]] *= -1
        else:
            nz = int(rng.choice(sizes))
            x[r, rng.permutation(dim)[:nz]] = rng.choice([-1.0, 1.0], nz)
    for r, flips in special.items():
        if 0 <= r < rows:
            x[r] = protos[0][0]
            x[r, protos[0][1][list(flips)]] *= -1
    return x


def unit_f16(x):
    """the unit rows as the device stores them -- exact for probe rows; a zero row stays zero"""
    nrm = np.sqrt((x.astype(np.float64) ** 2).sum(1, keepdims=True))
    return np.where(nrm > 0, x / np.where(nrm > 0, nrm, 1), 0).astype(np.float16)


def gallery_special(G):
    return {0: (), 126: (4,), 127: (2,), 128: (2, 3), G - 1: (2, 3)}        # (a later key wins where two coincide: G - 1 is always (2, 3))


def query_special(n):
    return {0: (2,), 16: (3,), 127: (2, 3), n - 1: ()}                        # query n - 1 x gallery row G - 1 = exactly 0.75


def reference_hits(q16, g16, thresh, self_join=False):
    """{(query, row): score} in float64 on the fp16 rows: score >= thresh and > 0; the self-join keeps row > query"""
    S = q16.astype(np.float64) @ g16.astype(np.float64).T
    ok = (S >= float(thresh)) & (S > 0)
    if self_join:
        ok &= np.triu(np.ones_like(ok), 1)
    return {(int(i), int(j)): S[i, j] for i, j in zip(*np.nonzero(ok))}


# ---- the entry point -----------------------------------------------------------------------------------------------------------------------------
def gallery_rows(ctx, gal):
    from scrfd_arcface_facerecognition_amd.engine import _gallery_ptr
    return ctx.borrow(_gallery_ptr(gal), (gal.Gp, gal.dim), np.float16)


def run_range(ctx, gal, q, n, thresh, cap, page=0):
    """fid_gallery_range -> (pairs [cap (+ page), 2], scores [cap (+ page)], total); the arrays are pre-filled with the canary byte and, with
    page > 0, allocated `page` bytes larger than hit_cap asks for.  q: a DeviceBuffer / device address of fp16 rows, or None = self-join."""
    from scrfd_arcface_facerecognition_amd._lib import _ptr, check
    pairs = ctx.empty((cap + page // 8, 2), np.int32)
    scores = ctx.empty((cap + page // 4,), np.float32)
    total = ctx.empty((1,), np.uint64)
    for b in (pairs, scores, total):
        check(ctx.lib.fid_memset(ctx.handle, C.c_void_p(b.ptr), CANARY, b.nbytes))
    check(ctx.lib.fid_gallery_range(ctx.handle, gal.handle, _ptr(q), int(n), C.c_float(thresh), C.c_void_p(pairs.ptr), C.c_void_p(scores.ptr),
                                    cap, C.c_void_p(total.ptr)))
    return pairs.download(), scores.download(), int(total.download()[0])


def canary_i32():
    return np.frombuffer(bytes([CANARY] * 4), np.int32)[0]


def assert_exact(pairs, scores, total, want, cap):
    assert total == len(want) <= cap
    got = {(int(a), int(b)): s for (a, b), s in zip(pairs[:total], scores[:total])}
    assert len(got) == total                                          # every record distinct
    assert got.keys() == want.keys()
    assert all(np.float64(got[k]) == want[k] for k in want)           # bit for bit: every cosine is a multiple of 1/64
    assert (pairs[total:] == canary_i32()).all() and (scores[total:].view(np.int32) == canary_i32()).all()


ABOVE = float(np.nextafter(np.float32(0.75), np.float32(1.0)))


@pytest.mark.parametrize("dim", [32, 96, 512])
@pytest.mark.parametrize("n", [1, 17, 129])
@pytest.mark.parametrize("G", [1, 33, 127, 128, 129, 300])
def test_range_exact_probes(ctx, G, n, dim):
    from scrfd_arcface_facerecognition_amd.engine import Gallery
    rng = np.random.default_rng(1000 * G + 10 * n + dim)
    protos = prototypes(rng, dim)
    g, q = probe_rows(rng, G, dim, protos, gallery_special(G)), probe_rows(rng, n, dim, protos, query_special(n))
    g16, q16 = unit_f16(g), unit_f16(q)
    gal = Gallery(ctx, g)
    try:
        assert np.array_equal(gallery_rows(ctx, gal).download()[:G], g16)          # the stored rows are the exact ones
        qd = ctx.to_device(q16)
        cap = n * G
        want = reference_hits(q16, g16, 0.75)
        assert want[(n - 1, G - 1)] == 0.75                                        # the threshold itself is attained, in the last row and column
        assert_exact(*run_range(ctx, gal, qd, n, 0.75, cap), want, cap)
        above = reference_hits(q16, g16, ABOVE)
        assert (n - 1, G - 1) not in above and len(above) < len(want)
        assert_exact(*run_range(ctx, gal, qd, n, ABOVE, cap), above, cap)
        if G > 128 and n > 128:
            assert {(127, 127), (127, 128), (128, 127), (128, 128)} <= want.keys()   # all four tiles that meet at the seam
    finally:
        gal.close()


@pytest.mark.parametrize("dim", [32, 96, 512])
@pytest.mark.parametrize("G", [2, 129, 300])
def test_self_join_exact_probes(ctx, G, dim):
    from scrfd_arcface_facerecognition_amd.engine import Gallery
    rng = np.random.default_rng(77 * G + dim)
    g = probe_rows(rng, G, dim, prototypes(rng, dim), gallery_special(G))
    g16 = unit_f16(g)
    gal = Gallery(ctx, g)
    try:
        cap = G * G
        for thresh in (0.75, ABOVE):
            want = reference_hits(g16, g16, thresh, self_join=True)
            pairs, scores, total = run_range(ctx, gal, None, 0, thresh, cap)
            assert_exact(pairs, scores, total, want, cap)
            assert all(a < b for a, b in pairs[:total])                            # never (i, i), never both orders
            assert ((0, G - 1) in want) == (thresh == 0.75)                        # exactly 0.75, across the whole matrix
            if G > 128:
                assert (127, 128) in want and want[(127, 128)] == 0.875            # a pair that straddles the tile seam
            # ... and it is the general join of the gallery against its own rows, filtered to i < j
            gp, gs, gt = run_range(ctx, gal, gallery_rows(ctx, gal), G, thresh, cap)
            full = {(int(a), int(b)): s for (a, b), s in zip(gp[:gt], gs[:gt])}
            assert all((i, i) in full and full[(i, i)] == 1.0 for i in range(G))   # the diagonal the self-join must leave out
            assert {k: v for k, v in full.items() if k[0] < k[1]} == {(int(a), int(b)): s for (a, b), s in zip(pairs[:total], scores[:total])}
    finally:
        gal.close()


@pytest.mark.parametrize("G,n,super_tile", [(700, 300, "1"), (700, 300, "2"), (700, 300, "4"), (700, 300, "5"), (2200, 2100, None)])
def test_tile_pair_orders(ctx, monkeypatch, G, n, super_tile):
    """The tile pairs are walked super-tile by super-tile (16 x 16 by default, FID_RANGE_SUPER overrides): ragged last super-tiles and the skipped
    lower half of a diagonal one, at 6 tiles under small super-tiles and at 18 tiles (two super-tiles per side, the second ragged) under the default"""
    from scrfd_arcface_facerecognition_amd.engine import Gallery
    if super_tile:
        monkeypatch.setenv("FID_RANGE_SUPER", super_tile)
    else:
        monkeypatch.delenv("FID_RANGE_SUPER", raising=False)
    rng = np.random.default_rng(G)
    protos = prototypes(rng, 32)
    g, q = probe_rows(rng, G, 32, protos, gallery_special(G)), probe_rows(rng, n, 32, protos, query_special(n))
    g16, q16 = unit_f16(g), unit_f16(q)
    gal = Gallery(ctx, g)
    try:
        cap = 1 << 19
        want = reference_hits(g16, g16, 0.75, self_join=True)
        assert (0, G - 1) in want and len({(i // 128, j // 128) for i, j in want}) == (G // 128 + 1) * (G // 128 + 2) // 2    # hits in every tile pair
        assert_exact(*run_range(ctx, gal, None, 0, 0.75, cap), want, cap)
        want = reference_hits(q16, g16, 0.75)
        assert len({(i // 128, j // 128) for i, j in want}) == (n // 128 + 1) * (G // 128 + 1)
        assert_exact(*run_range(ctx, gal, ctx.to_device(q16), n, 0.75, cap), want, cap)
    finally:
        gal.close()


def test_self_join_dense_tile(ctx):
    """200 identical rows: every wave of every launched tile reserves slots at once"""
    from scrfd_arcface_facerecognition_amd.engine import Gallery
    row = np.zeros(64, np.float32)
    row[::4] = [1, -1] * 8
    gal = Gallery(ctx, np.tile(row, (200, 1)))
    try:
        pairs, scores, total = run_range(ctx, gal, None, 0, 0.9, 20000)
        assert total == 19900
        assert {(int(a), int(b)) for a, b in pairs[:total]} == {(i, j) for i in range(200) for j in range(i + 1, 200)}
        assert (scores[:total] == 1.0).all()
    finally:
        gal.close()


def test_deleted_rows_and_zero_queries_never_hit(ctx):
    from scrfd_arcface_facerecognition_amd.engine import Gallery
    rng = np.random.default_rng(5)
    G, n, dim = 300, 17, 96
    protos = prototypes(rng, dim)
    g, q = probe_rows(rng, G, dim, protos, {}), probe_rows(rng, n, dim, protos, {})
    dead = [0, 5, 127, 128, 299]
    g[dead] = 0.0
    q[3] = 0.0
    q[16] = g[200]
    g16, q16 = unit_f16(g), unit_f16(q)
    gal = Gallery(ctx, g)
    try:
        qd = ctx.to_device(q16)
        for thresh in (0.5, 0.0, -1.0):
            want = reference_hits(q16, g16, thresh)
            pairs, scores, total = run_range(ctx, gal, qd, n, thresh, n * G)
            assert_exact(pairs, scores, total, want, n * G)
            assert total > 0 and not np.isin(pairs[:total, 1], dead).any() and not (pairs[:total, 0] == 3).any()
            assert (scores[:total] > 0).all()
        assert reference_hits(q16, g16, 0.0).keys() == reference_hits(q16, g16, -1.0).keys()
        # self-join: the dead rows are at cosine 0 from everything, themselves included
        for thresh in (0.5, -1.0):
            pairs, scores, total = run_range(ctx, gal, None, 0, thresh, G * G)
            assert_exact(pairs, scores, total, reference_hits(g16, g16, thresh, self_join=True), G * G)
            assert not np.isin(pairs[:total], dead).any()
    finally:
        gal.close()


def test_no_hits_leaves_the_outputs_untouched(ctx):
    from scrfd_arcface_facerecognition_amd.engine import Gallery
    rng = np.random.default_rng(6)
    g = probe_rows(rng, 300, 96, prototypes(rng, 96), gallery_special(300))
    gal = Gallery(ctx, g)
    try:
        for q, n in ((ctx.to_device(unit_f16(g[:40])), 40), (None, 0)):
            pairs, scores, total = run_range(ctx, gal, q, n, 1.5, 64)
            assert total == 0
            assert (pairs == canary_i32()).all() and (scores.view(np.int32) == canary_i32()).all()
    finally:
        gal.close()


def test_capacity_overflow_counts_on_and_stays_inside(ctx):
    from scrfd_arcface_facerecognition_amd.engine import Gallery
    rng = np.random.default_rng(8)
    G, n, dim = 300, 129, 96
    protos = prototypes(rng, dim)
    g, q = probe_rows(rng, G, dim, protos, gallery_special(G)), probe_rows(rng, n, dim, protos, {})
    q[::3] = g[rng.integers(0, G, len(q[::3]))]
    g16, q16 = unit_f16(g), unit_f16(q)
    gal = Gallery(ctx, g)
    try:
        want = reference_hits(q16, g16, 0.0)
        cap = len(want) // 3
        assert cap > 500
        pairs, scores, total = run_range(ctx, gal, ctx.to_device(q16), n, 0.0, cap, page=4096)
        assert total == len(want)                                                  # the counter is not clipped
        got = {(int(a), int(b)): s for (a, b), s in zip(pairs[:cap], scores[:cap])}
        assert len(got) == cap and all(k in want and want[k] == np.float64(s) for k, s in got.items())   # cap distinct, true hits
        assert (pairs[cap:] == canary_i32()).all() and (scores[cap:].view(np.int32) == canary_i32()).all()
        assert len(pairs) == cap + 512 and len(scores) == cap + 1024
    finally:
        gal.close()


def test_argument_checks(ctx):
    from scrfd_arcface_facerecognition_amd.engine import Gallery
    gal = Gallery(ctx, np.eye(32, dtype=np.float32))
    try:
        buf = ctx.empty((64,), np.int64)
        p = C.c_void_p(buf.ptr)
        call = ctx.lib.fid_gallery_range
        assert call(ctx.handle, gal.handle, p, 4, C.c_float(0.5), p, p, 0, p) == -1                       # hit_cap <= 0
        assert call(ctx.handle, gal.handle, p, 0, C.c_float(0.5), p, p, 8, p) == -1                       # no queries behind a query pointer
        assert call(ctx.handle, gal.handle, p, 4, C.c_float(float("nan")), p, p, 8, p) == -1              # NaN threshold
        assert b"NaN" in ctx.lib.fid_last_error()
        assert call(ctx.handle, gal.handle, p, 2 ** 31 - 1, C.c_float(0.5), p, p, 8, p) == -1             # queries beyond the 4 GiB buffer range
        assert b"4 GiB" in ctx.lib.fid_last_error()
        for bad in ((None, gal.handle, p, p, p), (ctx.handle, None, p, p, p), (ctx.handle, gal.handle, None, p, p),
                    (ctx.handle, gal.handle, p, None, p), (ctx.handle, gal.handle, p, p, None)):
            assert call(bad[0], bad[1], p, 4, C.c_float(0.5), bad[2], bad[3], 8, bad[4]) == -1
    finally:
        gal.close()


# ---- realistic values ----------------------------------------------------------------------------------------------------------------------------
def near_copy_store(rng, n=700):
    """Gaussian 512-dim embeddings with near-copies planted across the whole store (so that pairs land in every tile pair of a 700-row table)"""
    base = rng.standard_normal((n, 512)).astype(np.float32)
    for k in range(60):
        i, j = rng.permutation(n)[:2]
        cos = rng.uniform(0.6, 0.995)
        v = base[j] / np.linalg.norm(base[j])
        r = rng.standard_normal(512).astype(np.float32)
        r -= (r @ v) * v
        r /= np.linalg.norm(r)
        base[i] = (cos * v + np.sqrt(1 - cos * cos) * r) * np.float32(rng.uniform(0.5, 2.0))
    return base


def shuffled_store(ctx, rng, emb, capacity):
    from scrfd_arcface_facerecognition_amd.engine import VectorGallery
    ids = [int(i) for i in rng.permutation(5000)[:len(emb)]]
    order = rng.permutation(len(ids))
    vg = VectorGallery(ctx, 512, capacity=capacity)
    vg.upsert([ids[j] for j in order], emb[order])
    return vg, ids


# (the seeds were picked on the CPU, with the fp16 rounding emulated, so that no pair lies within 1e-4 of the threshold; asserted below on the
# rows the device actually stores)
@pytest.mark.parametrize("which,seed,query_seed", [("duplicates120", 55, 7), ("copies700", 11, 4)])
def test_realistic_values_against_float64_on_the_stored_rows(ctx, which, seed, query_seed):
    """The reference is float64 on the fp16 unit rows as stored, so the only difference left is the order of the fp32 sums, bounded by
    (K - 1) * 2^-24 * sum|a_i b_i| <= 511 * 6e-8 ~ 3e-5 for unit rows: scores within 1e-4, hit sets equal."""
    from scrfd_arcface_facerecognition_amd._lib import check
    rng = np.random.default_rng(seed)
    emb = duplicate_store(rng) if which == "duplicates120" else near_copy_store(rng)
    vg, ids = shuffled_store(ctx, rng, emb, 128 if which == "duplicates120" else 1024)
    gal = vg._gal
    rows = gallery_rows(ctx, gal).download()[:gal.G]
    S = rows.astype(np.float64) @ rows.astype(np.float64).T
    iu = np.triu_indices(gal.G, 1)
    assert np.abs(S[iu] - 0.8).min() > 1e-4
    want = {(int(i), int(j)): S[i, j] for i, j in zip(*iu) if S[i, j] >= 0.8}
    assert len(want) >= 8
    if which == "copies700":
        assert len({(i // 128, j // 128) for i, j in want}) > 3                    # more than one tile pair holds hits
    pairs, scores, total = run_range(ctx, gal, None, 0, 0.8, 4096)
    got = {(int(a), int(b)): float(s) for (a, b), s in zip(pairs[:total], scores[:total])}
    assert total == len(got) and got.keys() == want.keys()
    assert max(abs(got[k] - want[k]) for k in want) < 1e-4
    # general join: noisy copies of stored embeddings, normalised on the device
    n = 150
    rng = np.random.default_rng(query_seed)
    src = rng.integers(0, len(emb), n)
    queries = (emb[src] + rng.uniform(0.0, 1.0, (n, 1)).astype(np.float32) * rng.standard_normal((n, 512)).astype(np.float32))
    e, q = ctx.to_device(queries), ctx.empty((n, 512), np.float16)
    check(ctx.lib.fid_l2_normalize_f16(ctx.handle, C.c_void_p(e.ptr), n, 512, C.c_void_p(q.ptr)))
    Sq = q.download().astype(np.float64) @ rows.astype(np.float64).T
    assert np.abs(Sq - 0.8).min() > 1e-4
    want = {(int(i), int(j)): Sq[i, j] for i, j in zip(*np.nonzero(Sq >= 0.8))}
    pairs, scores, total = run_range(ctx, gal, q, n, 0.8, 4096)
    got = {(int(a), int(b)): float(s) for (a, b), s in zip(pairs[:total], scores[:total])}
    assert total == len(got) >= 20 and got.keys() == want.keys()
    assert max(abs(got[k] - want[k]) for k in want) < 1e-4


# ---- through the Python layer ------------------------------------------------------------------------------------------------------------------
def test_range_search_equals_the_oracle_and_survives_a_small_buffer(ctx):
    rng = np.random.default_rng(55)
    emb = duplicate_store(rng)
    vg, ids = shuffled_store(ctx, rng, emb, 64)                                     # (64 -> 128 rows: one capacity doubling, eight free rows)
    unit = emb.astype(np.float64) / np.linalg.norm(emb.astype(np.float64), axis=1, keepdims=True)
    S = unit @ unit.T
    assert np.abs(S[np.triu_indices(len(emb), 1)] - 0.8).min() > 2e-3             # fp16 rows move a score by < 1e-3: no hit can change sides
    probes = np.stack([emb[7] * 3.0 + 0.01 * rng.standard_normal(512), rng.standard_normal(512)]).astype(np.float32)
    queries = np.concatenate([emb, probes])
    want = [match.search_similar(qv, ids, emb, k=len(ids), threshold=0.8) for qv in queries]
    # the oracle's order is only a fair demand where its scores are further apart than the fp16 rows can move them
    assert all(a[1] - b[1] > 2e-3 for w in want for a, b in zip(w, w[1:]))
    assert sum(len(w) > 1 for w in want) >= 12 and want[-1] == []
    for cap in (None, 5):
        if cap:
            vg.hit_capacity = cap                                                  # far below the ~150 hits: the call must grow and repeat
        got = vg.range_search(queries, 0.8)
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert [i for i, _ in g] == [i for i, _ in w]
            assert all(abs(a[1] - b[1]) < 1e-3 for a, b in zip(g, w))
    # equal scores: ascending row.  Two stored copies of one vector, queried by that vector
    vg.upsert([9001, 9002], np.stack([emb[20], emb[20] * 2.0]))
    hit = vg.range_search(emb[20][None], 0.99)[0]
    assert len(hit) == 3 and hit[0][1] == hit[1][1] == hit[2][1]
    assert [vg.row_of[i] for i, _ in hit] == sorted(vg.row_of[i] for i, _ in hit)


def test_merge_via_join_equals_the_oracle_and_the_matrix_path(ctx):
    rng = np.random.default_rng(55)
    emb = duplicate_store(rng)
    vg, ids = shuffled_store(ctx, rng, emb, 64)
    vm, ids_m = shuffled_store(ctx, np.random.default_rng(55 + 1), emb, 64)        # an identical second store (other rows, other ids order ...)
    vm.delete(ids_m)
    vm.upsert(ids, emb)                                                            # ... refilled with the SAME ids
    want, survivors = match.find_and_merge_duplicates(ids, emb, 0.8)
    pairs = vg.similar_pairs(0.8)
    assert all(vg.row_of[a] < vg.row_of[b] for a, b, _ in pairs)
    assert [(vg.row_of[a], vg.row_of[b]) for a, b, _ in pairs] == sorted((vg.row_of[a], vg.row_of[b]) for a, b, _ in pairs)
    vg.hit_capacity = 4                                                            # the merge must not depend on the first buffer's size
    got = vg.find_and_merge_duplicates(0.8, via="join")
    assert len(want) >= 7 and [(a, b) for a, b, _ in got] == [(a, b) for a, b, _ in want]
    assert max(abs(g[2] - w[2]) for g, w in zip(got, want)) < 1e-3
    assert sorted(vg.row_of) == survivors and len(vg) == len(ids) - len(want)
    dense = vm.find_and_merge_duplicates(0.8)                                      # the default is the matrix path
    assert [(a, b) for a, b, _ in dense] == [(a, b) for a, b, _ in got]
    assert max(abs(d[2] - g[2]) for d, g in zip(dense, got)) < 1e-3
    assert vg.find_and_merge_duplicates(0.8, via="join") == [] and vg.similar_pairs(0.8) == []
    with pytest.raises(ValueError):
        vg.find_and_merge_duplicates(0.8, via="dense")
