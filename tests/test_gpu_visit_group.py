"""GPU: fid_gallery_group (csrc/visit_group.hip) and the Python layer above it (VectorGallery.group_visits / group_device, FaceAnalysis.process_visits)
against the float64 oracle of tests/visit_oracle.py.

Exact probes (the generators of test_gpu_range_join.py): rows with 4, 16 or 64 entries of +-1 have exact unit rows in fp16 and every cosine is an
exact multiple of 1/64 in fp32 in any summation order, so every verdict, row and score must equal the oracle BIT FOR BIT, thresholds that are
attained included.  Variants of one 16-entry prototype (sign flips inside its support) sit at 1 - |flips that differ| / 8 from each other: 1, 0.875,
0.75, 0.625, 0.5 ...; the thresholds are dup = 0.875, group = 0.625, search = 0.5 and the same three one float32 step above.

In the shape tests G is the size of the store BEFORE the call (rows 0 and G - 1 occupied, a few free holes inside); the gallery has G + n rows so
that every visit can become a person, and new_rows (the holes and the rows behind G, shuffled) is never ascending."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_mixed_sizes import heuristic_plans, mixed_detector          # noqa: F401  (fixtures: the calibrated synthetic SCRFD-500M)
from test_gpu_range_join import CANARY, canary_i32, gallery_rows, probe_rows, prototypes, unit_f16
from visit_oracle import DEFERRED, DUPLICATE, NEW, NO_FACE, RECOGNISED, group_visits

pytestmark = pytest.mark.gpu

BASE = (0.875, 0.625, 0.5)                                                  # dup, group, search
ABOVE = tuple(float(np.nextafter(np.float32(t), np.float32(2.0))) for t in BASE)
PAGE = 4096


@pytest.fixture(scope="module")
def ctx():
    from scrfd_arcface_facerecognition_amd._lib import default_context
    return default_context(0)


# ---- the entry point -----------------------------------------------------------------------------------------------------------------------------
def group_call(ctx, gal, q_ptr, n, thr, new_rows, n_new_rows=None, outputs=None):
    """fid_gallery_group's return code; outputs = (verdict, row, score, summary) device buffers"""
    from scrfd_arcface_facerecognition_amd._lib import _ptr
    rows = np.ascontiguousarray(new_rows, dtype=np.int32)
    rows_dev = ctx.to_device(rows if len(rows) else np.zeros(1, np.int32))
    v, r, s, m = outputs
    return ctx.lib.fid_gallery_group(ctx.handle, gal.handle, _ptr(q_ptr), int(n), C.c_float(thr[0]), C.c_float(thr[1]), C.c_float(thr[2]),
                                     C.c_void_p(rows_dev.ptr), len(rows) if n_new_rows is None else int(n_new_rows), _ptr(v), _ptr(r), _ptr(s), _ptr(m))


def run_group(ctx, gal, q_ptr, n, thr, new_rows, n_new_rows=None):
    """-> verdict [n], row [n], score [n], summary (new, first deferred).  The outputs are canary-filled and one page larger than needed: nothing
    beyond n entries (2 for the summary) may be written."""
    from scrfd_arcface_facerecognition_amd._lib import check
    bufs = [ctx.empty((n + PAGE // 4,), np.int32), ctx.empty((n + PAGE // 4,), np.int32), ctx.empty((n + PAGE // 4,), np.float32),
            ctx.empty((2 + PAGE // 4,), np.int32)]
    for b in bufs:
        check(ctx.lib.fid_memset(ctx.handle, C.c_void_p(b.ptr), CANARY, b.nbytes))
    check(group_call(ctx, gal, q_ptr, n, thr, new_rows, n_new_rows, bufs))
    v, r, s, m = (b.download() for b in bufs)
    assert (v[n:] == canary_i32()).all() and (r[n:] == canary_i32()).all() and (s[n:].view(np.int32) == canary_i32()).all()
    assert (m[2:] == canary_i32()).all()
    return v[:n], r[:n], s[:n], (int(m[0]), int(m[1]))


def assert_equals_oracle(got, want, what=""):
    v, r, s, m = got
    assert np.array_equal(v, want[0]), (what, np.nonzero(v != want[0])[0][:8])
    assert np.array_equal(r, want[1]), (what, np.nonzero(r != want[1])[0][:8])
    assert np.array_equal(s.astype(np.float64), want[2]), (what, np.nonzero(s != want[2])[0][:8])      # bit for bit: multiples of 1/64
    assert m == tuple(want[3]), what


def bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


def assert_gallery(ctx, gal, before, q16, verdict, new_rows, used):
    """rows new_rows[:used] hold the NEW visits' query rows bit for bit, in visit order; every other row (padding included) is unchanged"""
    want = before.copy()
    new = np.nonzero(verdict == NEW)[0]
    assert len(new) == used
    want[np.asarray(new_rows[:used], dtype=np.int64)] = q16[new]
    after = gallery_rows(ctx, gal).download()
    assert np.array_equal(bits(after), bits(want))
    return after


# ---- planted probe batches -----------------------------------------------------------------------------------------------------------------------
def variant(proto, flips=()):
    p, sup = proto
    x = p.copy()
    x[sup[list(flips)]] *= -1
    return x


def build_case(n, G, dim, layout, seed=0):
    """-> g [G + n, dim] (+-1 / 0 rows; rows >= G and the holes are free), q16 [n, dim] unit fp16 visits, new_rows, plants {name: visit}"""
    rng = np.random.default_rng(100000 * seed + 1000 * G + 10 * n + dim + {"seam": 1, "chain": 2, "zeros": 3}[layout])
    P = prototypes(rng, dim) + prototypes(rng, dim)          # 0 .. 7 are planted, the random variants of the fill come from 8 .. 11
    Gt = G + n
    g = np.zeros((Gt, dim), np.float32)
    g[:G] = probe_rows(rng, G, dim, P[8:], {})
    holes = [r for r in (2, 31, 32) if r < G - 1]
    g[holes] = 0.0
    q = probe_rows(rng, n, dim, P[8:], {})
    plants, marker = {}, []

    def put(name, pos, row):
        if 0 <= pos < n and pos not in plants.values():
            q[pos] = row
            plants[name] = pos
            return True
        return False

    g[G - 1] = variant(P[6])                                 # the best of one visit is the last row of the old store, of another its row 0
    if G > 1:
        g[0] = variant(P[7])
    if layout == "seam":
        b = 127 if n > 127 else 0                            # a NEW visit at 127, its DUPLICATE (0.875) and RECOGNISED (0.625) followers at 128 and 129
        put("new", b, variant(P[0]))
        put("dup", b + 1, variant(P[0], (0,)))
        put("rec", b + 2, variant(P[0], (0, 1, 2)))
        put("far", n - 1, variant(P[0], (1, 2)))
    if layout == "chain":
        for name, (i, j, k), proto in (("c", (3, 8, 12), P[1]), ("s", (120, 127, 128), P[2])):    # within a block; across the 127 | 128 seam
            if k < n:
                put(name + "A", i, variant(proto))
                put(name + "B", j, variant(proto, (0, 1)))               # 0.75 from A: recognised, NOT stored
                put(name + "C", k, variant(proto, (0, 1, 2, 3)))         # 0.75 from B, 0.5 from A: new
        if G >= 33 and n >= 17:                              # equal scores between a row of the old store and a person of this batch
            g[10], g[11] = variant(P[3], (2, 3)), variant(P[4], (2, 3))
            put("tie_lo_U", 14, variant(P[3], (0, 1)))                   # 0.5 from row 10: new -- it will be stored BELOW row 10 (hole 2)
            put("tie_lo_X", 16, variant(P[3]))                           # 0.75 from both
            put("tie_hi_U", 13, variant(P[4], (0, 1)))                   # ... and this one ABOVE row 11
            put("tie_hi_X", 15, variant(P[4]))
            put("tie_lo_far", 260, variant(P[3]))                        # the same ties seen from another block
            put("tie_hi_far", 261, variant(P[4]))
    if layout == "zeros":
        for name, pos in (("z0", 0), ("z127", 127), ("z128", 128), ("zlast", n - 1)):
            if put(name, pos, np.zeros(dim, np.float32)):
                if len([k for k in plants if k.startswith("z")]) % 2 == 1:       # alternately the -0.0 marker row and the all +0.0 row
                    marker.append(pos)
        if 12 < n:
            put("cA", 3, variant(P[1]))
            put("cB", 8, variant(P[1], (0, 1)))
            put("cC", 12, variant(P[1], (0, 1, 2, 3)))
    put("last_row", 5, variant(P[6], (0, 1)))                # 0.75 from row G - 1
    if G > 1:
        put("row0", 6, variant(P[7], (0,)))                  # 0.875 from row 0
    q16 = unit_f16(q)
    for pos in marker:
        bits(q16)[pos, 0] = 0x8000                           # the -0.0-first marker row of an empty slot
    plants["marker"] = marker
    new_rows = [int(r) for r in rng.permutation(holes + list(range(G, Gt)))]
    if len(new_rows) > 1 and new_rows == sorted(new_rows):
        new_rows.reverse()                                   # deliberately not ascending
    if "tie_lo_U" in plants:
        # the k-th NEW visit gets new_rows[k]; which visits are NEW does not depend on the rows, so one oracle pass tells the k of both U visits
        v0 = group_visits(unit_f16(g), q16, new_rows, *BASE)[0]
        k, j = int((v0[:plants["tie_lo_U"]] == NEW).sum()), new_rows.index(2)
        new_rows[k], new_rows[j] = new_rows[j], new_rows[k]      # (every other free row lies above row 11: nothing to arrange for tie_hi_U)
        assert np.array_equal(group_visits(unit_f16(g), q16, new_rows, *BASE)[0], v0)
    return g, q16, new_rows, plants


_CASES = {}


def planted_case(n, G, dim, layout):
    """build_case under the first seed whose ORACLE answer shows every planted situation (at dim 32 a random fill row now and then comes closer to
    a planted visit than its planted partner): the choice looks at the oracle alone.  -> g, q16, new_rows, plants, {thresholds: oracle answer}"""
    key = (n, G, dim, layout)
    if key not in _CASES:
        for seed in range(64):
            g, q16, new_rows, plants = build_case(n, G, dim, layout, seed)
            want = {thr: group_visits(unit_f16(g), q16, new_rows, *thr) for thr in (BASE, ABOVE)}
            try:
                for thr in (BASE, ABOVE):
                    assert_planted(want[thr], plants, G, n, thr)
            except AssertionError:
                continue
            _CASES[key] = (g, q16, new_rows, plants, want)
            break
    return _CASES[key]                                       # (KeyError: no seed shows the plants -- a mistake in build_case)


def assert_planted(want, plants, G, n, thr):
    """the planted situations are in the oracle's answer (before the device is asked)"""
    v, r, s, _, _ = want
    base = thr == BASE
    p = plants
    if "new" in p:
        assert v[p["new"]] == NEW
        if "dup" in p:
            assert s[p["dup"]] == 0.875 and r[p["dup"]] == r[p["new"]] and v[p["dup"]] == (DUPLICATE if base else RECOGNISED)
        if "rec" in p:
            assert s[p["rec"]] == 0.625 and v[p["rec"]] == (RECOGNISED if base else NEW)           # `>=`: attained is enough, one step above is not
            if base:
                assert r[p["rec"]] == r[p["new"]]
        if "far" in p and base:
            assert v[p["far"]] == RECOGNISED and r[p["far"]] == r[p["new"]] and s[p["far"]] == 0.75
    for c in "cs":
        if c + "C" in p:
            A, B, Cc = p[c + "A"], p[c + "B"], p[c + "C"]
            assert v[A] == NEW and v[B] == RECOGNISED and r[B] == r[A] and s[B] == 0.75
            assert v[Cc] == NEW and r[Cc] != r[A] and s[Cc] == (0.5 if base else 0.0)               # 0.5 = search: reported; one step above: 0
    if "tie_lo_X" in p and base:                             # (new_rows is arranged for the NEW count of the base thresholds)
        assert v[p["tie_lo_U"]] == NEW and r[p["tie_lo_U"]] == 2 and v[p["tie_hi_U"]] == NEW and r[p["tie_hi_U"]] > 11
        for x in [p["tie_lo_X"], p["tie_hi_X"]] + [p[k] for k in ("tie_lo_far", "tie_hi_far") if k in p]:
            assert v[x] == RECOGNISED and s[x] == 0.75
        assert r[p["tie_lo_X"]] == 2 and r[p["tie_hi_X"]] == 11                                     # the lower ROW, whoever holds it
        if "tie_lo_far" in p:
            assert r[p["tie_lo_far"]] == 2 and r[p["tie_hi_far"]] == 11
    for z in ("z0", "z127", "z128", "zlast"):
        if z in p:
            assert v[p[z]] == NO_FACE and r[p[z]] == -1 and s[p[z]] == 0
    if "last_row" in p:
        assert v[p["last_row"]] == RECOGNISED and r[p["last_row"]] == G - 1 and s[p["last_row"]] == 0.75
    if "row0" in p:
        assert r[p["row0"]] == 0 and s[p["row0"]] == 0.875 and v[p["row0"]] == (DUPLICATE if base else RECOGNISED)


@pytest.mark.parametrize("layout", ["seam", "chain", "zeros"])
@pytest.mark.parametrize("dim", [32, 512])
@pytest.mark.parametrize("G", [1, 33, 129, 300])
@pytest.mark.parametrize("n", [1, 2, 17, 128, 129, 300])
def test_group_exact_probes(ctx, n, G, dim, layout):
    from scrfd_arcface_facerecognition_amd.engine import Gallery
    g, q16, new_rows, plants, wants = planted_case(n, G, dim, layout)
    g16 = unit_f16(g)
    assert len(new_rows) < 2 or new_rows != sorted(new_rows)
    if layout == "zeros":
        assert plants["marker"] and "z0" in plants
    if n == 300:
        assert {"seam": {"new", "dup", "rec", "far"}, "chain": {"cC", "sC"} | ({"tie_lo_far"} if G >= 33 else set()), "zeros": {"z127", "z128", "zlast"}}[layout] <= set(plants)
    qd = ctx.to_device(q16)
    for thr in (BASE, ABOVE):
        want = wants[thr]
        assert_planted(want, plants, G, n, thr)
        assert want[3][1] == n                                                     # room for everybody: nothing is deferred here
        gal = Gallery(ctx, g)
        try:
            before = gallery_rows(ctx, gal).download()
            assert np.array_equal(bits(before[:G + n]), bits(g16)) and not before[G + n:].any()
            got = run_group(ctx, gal, qd, n, thr, new_rows)
            assert_equals_oracle(got, want, thr)
            after = assert_gallery(ctx, gal, before, q16, got[0], new_rows, got[3][0])
            assert np.array_equal(bits(after[:G + n]), bits(want[4]))
        finally:
            gal.close()


# ---- split invariance: the strongest check ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,layout", [(32, "chain"), (512, "seam"), (512, "chain")])
def test_split_invariance(ctx, dim, layout):
    """one call on 300 visits == two calls on [0, k) and [k, 300) == (on a prefix of 40) forty calls of one visit: verdicts, rows, scores, gallery"""
    from scrfd_arcface_facerecognition_amd.engine import Gallery
    n, G = 300, 129
    g, q16, new_rows, plants, wants = planted_case(n, G, dim, layout)
    want = wants[BASE]
    assert_planted(want, plants, G, n, BASE)
    qd = ctx.to_device(q16)
    row_bytes = dim * 2

    def fresh():
        return Gallery(ctx, g)

    gal = fresh()
    try:
        full = run_group(ctx, gal, qd, n, BASE, new_rows)
        assert_equals_oracle(full, want)
        full_rows = gallery_rows(ctx, gal).download()
    finally:
        gal.close()
    for k in (1, 127, 128, 200):
        gal = fresh()
        try:
            a = run_group(ctx, gal, qd, k, BASE, new_rows)
            assert a[3][1] == k
            b = run_group(ctx, gal, qd.ptr + k * row_bytes, n - k, BASE, new_rows[a[3][0]:])
            for i in range(3):
                assert np.array_equal(np.concatenate([a[i], b[i]]), full[i]), (k, i)
            assert a[3][0] + b[3][0] == full[3][0] and b[3][1] == n - k
            assert np.array_equal(bits(gallery_rows(ctx, gal).download()), bits(full_rows))
        finally:
            gal.close()
    m = 40
    gal, one = fresh(), fresh()
    try:
        prefix = run_group(ctx, one, qd, m, BASE, new_rows)
        assert all(np.array_equal(prefix[i], full[i][:m]) for i in range(3))
        used = 0
        for i in range(m):
            v, r, s, (k, d) = run_group(ctx, gal, qd.ptr + i * row_bytes, 1, BASE, new_rows[used:])
            assert (v[0], r[0], s[0]) == (full[0][i], full[1][i], full[2][i]) and d == 1 and k == int(v[0] == NEW)
            used += k
        assert used == prefix[3][0] > 5
        assert np.array_equal(bits(gallery_rows(ctx, gal).download()), bits(gallery_rows(ctx, one).download()))
    finally:
        gal.close()
        one.close()


# ---- DEFERRED --------------------------------------------------------------------------------------------------------------------------------------
def test_deferred_suffix_is_completed_by_a_second_call(ctx):
    from scrfd_arcface_facerecognition_amd.engine import Gallery
    n, G, dim = 300, 129, 512
    g, q16, new_rows, _, wants = planted_case(n, G, dim, "zeros")
    g16 = unit_f16(g)
    want = wants[BASE]
    k = want[3][0]
    assert k > 100
    short_want = group_visits(g16, q16, new_rows[:k - 2], *BASE)
    d = short_want[3][1]
    assert d < n - 1 and short_want[3][0] == k - 2 and want[0][d] == NEW
    assert NO_FACE in short_want[0][d:] and (short_want[0][d:] != NO_FACE).sum() >= 2            # a zero row behind the deferred visit stays NO_FACE
    qd = ctx.to_device(q16)
    gal = Gallery(ctx, g)
    try:
        before = gallery_rows(ctx, gal).download()
        got = run_group(ctx, gal, qd, n, BASE, new_rows, n_new_rows=k - 2)                      # (the array is longer than the call may use)
        assert_equals_oracle(got, short_want)
        assert got[3] == (k - 2, d)
        assert all(np.array_equal(got[i][:d], want[i][:d].astype(got[i].dtype)) for i in range(3))     # the prefix is the full answer's prefix
        assert ((got[0][d:] == DEFERRED) | (got[0][d:] == NO_FACE)).all() and (got[1][d:] == -1).all() and (got[2][d:] == 0).all()
        assert_gallery(ctx, gal, before, q16, got[0], new_rows, k - 2)
        rest = run_group(ctx, gal, qd.ptr + d * dim * 2, n - d, BASE, new_rows[k - 2:k])          # two more rows complete it
        assert all(np.array_equal(rest[i], want[i][d:].astype(rest[i].dtype)) for i in range(3)) and rest[3] == (2, n - d)
        assert np.array_equal(bits(gallery_rows(ctx, gal).download()[:G + n]), bits(want[4]))
    finally:
        gal.close()
    # no row at all: deferred from the first visit that needs one; nothing is written
    none_want = group_visits(g16, q16, [], *BASE)
    d0 = none_want[3][1]
    assert none_want[3][0] == 0 and d0 < 20 and (none_want[0][:d0] != NEW).all()
    gal = Gallery(ctx, g)
    try:
        before = gallery_rows(ctx, gal).download()
        got = run_group(ctx, gal, qd, n, BASE, new_rows, n_new_rows=0)
        assert_equals_oracle(got, none_want)
        assert np.array_equal(bits(gallery_rows(ctx, gal).download()), bits(before))
    finally:
        gal.close()


def test_rows_outside_the_gallery_are_not_stored(ctx):
    """new_rows cannot be checked on the host without a synchronise: the kernel skips the store (and the visit is nobody's candidate)"""
    from scrfd_arcface_facerecognition_amd.engine import Gallery
    n, G, dim = 17, 33, 32
    g, q16, new_rows, _, _ = planted_case(n, G, dim, "chain")
    bad = list(new_rows)
    bad[1], bad[3] = G + n, -5                                                     # one past the last row; negative
    want = group_visits(unit_f16(g), q16, bad, *BASE)
    assert want[3][0] > 4 and (want[1][want[0] == NEW] == -1).sum() == 2
    gal = Gallery(ctx, g)
    try:
        before = gallery_rows(ctx, gal).download()
        got = run_group(ctx, gal, ctx.to_device(q16), n, BASE, bad)
        assert_equals_oracle(got, want)
        exp = before.copy()
        new = np.nonzero(got[0] == NEW)[0]
        for visit, r in zip(new, bad):
            if 0 <= r < G + n:
                exp[r] = q16[visit]
        assert np.array_equal(bits(gallery_rows(ctx, gal).download()), bits(exp))
    finally:
        gal.close()


def test_argument_checks_enqueue_nothing(ctx):
    from scrfd_arcface_facerecognition_amd._lib import check
    from scrfd_arcface_facerecognition_amd.engine import Gallery
    g, q16, new_rows, _, _ = planted_case(17, 33, 32, "seam")
    gal = Gallery(ctx, g)
    try:
        before = gallery_rows(ctx, gal).download()
        qd = ctx.to_device(q16)
        outs = [ctx.empty((64,), np.int32), ctx.empty((64,), np.int32), ctx.empty((64,), np.float32), ctx.empty((64,), np.int32)]
        for b in outs:
            check(ctx.lib.fid_memset(ctx.handle, C.c_void_p(b.ptr), CANARY, b.nbytes))
        nan = float("nan")
        for thr in ((nan, 0.6, 0.5), (0.9, nan, 0.5), (0.9, 0.6, nan), (0.0, 0.6, 0.5), (0.9, 0.0, 0.5), (0.9, 0.6, 0.0), (-0.5, 0.6, 0.5), (0.9, 0.6, -1.0)):
            assert group_call(ctx, gal, qd, 17, thr, new_rows, None, outs) == -1, thr
            assert ctx.lib.fid_last_error() != b""
        assert group_call(ctx, gal, qd, 0, BASE, new_rows, None, outs) == -1
        assert group_call(ctx, gal, qd, -3, BASE, new_rows, None, outs) == -1
        assert group_call(ctx, gal, qd, 65537, BASE, new_rows, None, outs) == -1
        assert group_call(ctx, gal, qd, 17, BASE, new_rows, -1, outs) == -1
        assert group_call(ctx, gal, None, 17, BASE, new_rows, None, outs) == -1
        for i in range(4):
            assert group_call(ctx, gal, qd, 17, BASE, new_rows, None, [None if j == i else o for j, o in enumerate(outs)]) == -1, i
        ctx.sync()
        assert all((b.download().view(np.int32) == canary_i32()).all() for b in outs)
        assert np.array_equal(bits(gallery_rows(ctx, gal).download()), bits(before))
    finally:
        gal.close()


# ---- realistic values ------------------------------------------------------------------------------------------------------------------------------
def near(rng, v, cos):
    """a vector at cosine `cos` from v (the helper inside test_range_join_cpu.duplicate_store)"""
    v = v / np.linalg.norm(v)
    r = rng.standard_normal(512).astype(np.float32)
    r -= (r @ v) * v
    r /= np.linalg.norm(r)
    return (cos * v + np.sqrt(1 - cos * cos) * r).astype(np.float32) * np.float32(rng.uniform(0.5, 2.0))


REAL_THR = (0.95, 0.4, 0.3)                                                       # dup, group, search
REAL_SEED = 3


def realistic_data(seed=REAL_SEED):
    """40 identities (random centres); a store of 500 rows = one member of 20 of them among unrelated rows; 1000 visits at cosine ~0.75 from their
    centre (members of one person ~0.56 from each other), 30 of them near-copies (0.99) of a stored member, of a person
    created earlier in the batch or of any earlier visit"""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((40, 512)).astype(np.float32)
    store = rng.standard_normal((500, 512)).astype(np.float32)
    where = rng.permutation(500)[:20]
    for k, r in enumerate(where):
        store[r] = near(rng, centres[k], 0.75)
    who = rng.integers(0, 40, 1000)
    visits = np.stack([near(rng, centres[w], 0.75) for w in who])
    first = {w: int(np.nonzero(who == w)[0][0]) for w in range(20, 40)}       # the visit that creates each person the store does not know
    spots = [int(i) for i in rng.permutation(np.arange(max(first.values()) + 1, 1000))[:30]]
    for k, i in enumerate(spots):                            # near-copies of stored members, of persons created in this batch, of any earlier visit
        src = store[where[k]] if k < 10 else visits[first[20 + k - 10]] if k < 20 else visits[int(rng.integers(0, i))]
        visits[i] = near(rng, src, 0.99)
    return store, visits


def assert_margins(rows16, q16, new_rows, want):
    """No best score within 1e-3 of a threshold and every runner-up more than 1e-3 below its best, on the float64 oracle (1e-3 is the project's
    cosine tolerance; the fp32-accumulation error of a 512-term dot product of unit fp16 rows is ~3e-5).  A seed that violates this is replaced,
    the margin is not widened."""
    verdict, row, score, _, final = want
    store = np.array(rows16, dtype=np.float64)
    Q = q16.astype(np.float64)
    k = 0
    for i in range(len(Q)):
        s = store @ Q[i]
        top = np.sort(s)[-2:]
        assert top[1] - top[0] > 1e-3, (i, top)
        assert min(abs(top[1] - t) for t in REAL_THR) > 1e-3, (i, top)
        if verdict[i] == NEW:
            store[new_rows[k]] = Q[i]
            k += 1


def test_realistic_values_and_the_loop_baseline(ctx):
    from scrfd_arcface_facerecognition_amd._lib import check
    from scrfd_arcface_facerecognition_amd.engine import VISIT_VERDICTS, VectorGallery, _gallery_ptr
    store, visits = realistic_data()
    n = len(visits)
    twins = []
    for _ in range(2):
        vg = VectorGallery(ctx, 512, capacity=1024)
        vg.upsert(list(range(1000, 1500)), store)
        twins.append(vg)
    vg, vl = twins
    while len(vg._free) < n:
        vg._grow()                                                                 # (group_visits would do the same: the oracle needs the rows it will see)
    new_rows = list(reversed(vg._free))[:n]
    rows16 = ctx.borrow(_gallery_ptr(vg._gal), (vg._gal.Gp, 512), np.float16).download()[:vg._gal.G]
    e, q = ctx.to_device(visits), ctx.empty((n, 512), np.float16)
    check(ctx.lib.fid_l2_normalize_f16(ctx.handle, C.c_void_p(e.ptr), n, 512, C.c_void_p(q.ptr)))
    q16 = q.download()
    want = group_visits(rows16, q16, new_rows, *REAL_THR)
    assert_margins(rows16, q16, new_rows, want)
    counts = np.bincount(want[0], minlength=5)
    assert counts[NEW] >= 20 and counts[RECOGNISED] > 800 and counts[DUPLICATE] >= 5 and counts[DEFERRED] == 0
    recs = vg.group_visits(visits, duplicate_threshold=REAL_THR[0], grouping_threshold=REAL_THR[1], similarity_threshold=REAL_THR[2])
    assert [r["verdict"] for r in recs] == [VISIT_VERDICTS[v] for v in want[0]]                       # all 1000 visits
    assert [vg.row_of[r["person_id"]] for r in recs] == list(want[1])
    assert max(abs(r["similarity"] - s) for r, s in zip(recs, want[2])) < 1e-3
    assert len(vg) == 500 + counts[NEW]
    loop = vl.group_visits(visits, duplicate_threshold=REAL_THR[0], grouping_threshold=REAL_THR[1], similarity_threshold=REAL_THR[2], via="loop")
    assert [(r["verdict"], r["person_id"]) for r in loop] == [(r["verdict"], r["person_id"]) for r in recs]
    assert max(abs(a["similarity"] - b["similarity"]) for a, b in zip(loop, recs)) < 1e-3


# ---- VectorGallery ---------------------------------------------------------------------------------------------------------------------------------
def test_group_visits_binds_ids_restores_the_free_list_and_grows(ctx):
    from scrfd_arcface_facerecognition_amd.engine import VectorGallery, _gallery_ptr
    rng = np.random.default_rng(12)
    people = rng.standard_normal((200, 512)).astype(np.float32)                    # unrelated: every one a new person
    vg = VectorGallery(ctx, 512, capacity=64)
    first = np.concatenate([people[:3], people[1:2] * 2.0, np.zeros((1, 512), np.float32), near(rng, people[0], 0.7)[None]])
    free_before = list(vg._free)
    recs = vg.group_visits(first, ids=["a", "b", "c", "d", "e", "f"])
    assert [r["verdict"] for r in recs] == ["new", "new", "new", "duplicate", "no face", "recognised"]
    assert [r["person_id"] for r in recs] == ["a", "b", "c", "b", None, "a"]
    assert recs[0]["similarity"] == 1.0 and recs[1]["similarity"] == 0.0           # the first person of an EMPTY store reports 1.0
    assert abs(recs[3]["similarity"] - 1.0) < 1e-3 and abs(recs[5]["similarity"] - 0.7) < 2e-3 and recs[4]["similarity"] == 0.0
    assert len(vg) == 3 and [vg.row_of[i] for i in "abc"] == [0, 1, 2] and [vg.id_of[r] for r in (0, 1, 2)] == ["a", "b", "c"]
    assert vg._free == free_before[:-3]                                            # three rows consumed, the rest back in their old order
    assert [len(h) for h in vg.search(people[:3], k=1, score_threshold=0.9)] == [1, 1, 1]
    # a second call recognises the persons the first one created; default ids are fresh integers above the largest integer id
    vg.upsert([41], people[10:11])
    again = vg.group_visits(np.stack([near(rng, people[2], 0.8), people[11], near(rng, people[10], 0.8)]))
    assert [(r["verdict"], r["person_id"]) for r in again] == [("recognised", "c"), ("new", 42), ("recognised", 41)]
    assert again[1]["similarity"] == 0.0                                           # not an empty store any more
    # growth: a store of capacity 64 receives 200 new persons
    big = VectorGallery(ctx, 512, capacity=64)
    recs = big.group_visits(people)
    assert [r["verdict"] for r in recs] == ["new"] * 200 and [r["person_id"] for r in recs] == list(range(200))
    assert len(big) == 200 and big._gal.G == 256 and len(big._free) == 56 and len(set(big._free) | set(big.id_of)) == 256
    back = big.group_visits(people[::-1] * 3.0)
    assert [(r["verdict"], r["person_id"]) for r in back] == [("duplicate", i) for i in range(199, -1, -1)]
    with pytest.raises(ValueError):
        big.group_visits(people[:2], via="matrix")
    # ids that clash are refused BEFORE anything is written: the store stays as it was
    state = (dict(big.row_of), list(big._free), bits(ctx.borrow(_gallery_ptr(big._gal), (big._gal.Gp, 512), np.float16).download()).copy())
    for bad_ids in ([7, "x"], ["x", "x"]):
        with pytest.raises(ValueError):
            big.group_visits(rng.standard_normal((2, 512)).astype(np.float32), ids=bad_ids)
    assert (big.row_of, big._free) == state[:2]
    assert np.array_equal(bits(ctx.borrow(_gallery_ptr(big._gal), (big._gal.Gp, 512), np.float16).download()), state[2])
    # group_device: unit rows that are already on the device
    q = ctx.to_device(unit_f16(people[:4] * 1.0))
    dev = big.group_device(q, 4, grouping_threshold=0.45)
    assert [(r["verdict"], r["person_id"]) for r in dev] == [("duplicate", i) for i in range(4)]


# ---- FaceAnalysis.process_visits -------------------------------------------------------------------------------------------------------------------
def test_process_visits_equals_best_face_and_the_loop(ctx, mixed_detector):
    from scrfd_arcface_facerecognition_amd._lib import GateConfig
    from scrfd_arcface_facerecognition_amd.app import VERDICTS, FaceAnalysis
    from scrfd_arcface_facerecognition_amd.engine import VectorGallery
    det, images = mixed_detector
    # two sizes; two repeated images (duplicates of the persons their first copies created) and a blank one, whose best detection stays below
    # the reference's confidence_threshold of 0.6 (no face)
    images = [images[0], images[1], np.zeros((240, 427, 3), np.uint8), images[0], images[5], images[1]]
    app = FaceAnalysis("synthetic:scrfd_500m?seed=5", "synthetic:arcface_mbf?seed=5", det_size=(320, 320), max_faces=16, gate_config=GateConfig())
    assert app.ctx is det.ctx
    app.det = det
    # (the synthetic recogniser's embeddings of different images sit at cosine 0.93 .. 0.993 from each other: thresholds above that tell them apart)
    thr = dict(duplicate_threshold=0.999, grouping_threshold=0.99, similarity_threshold=0.98)
    store = VectorGallery(app.ctx, 512, capacity=64)
    records, counters = app.process_visits(images, store, **thr)
    assert len(records) == len(images)
    assert counters["processed"] + counters["no_faces"] + counters["duplicate_faces"] == len(images)
    assert counters["processed"] == counters["recognized"] + counters["new_persons"] and counters["new_persons"] == len(store)
    # image by image: best_face, then the reference's own sequence on a second store
    twin = VectorGallery(app.ctx, 512, capacity=64)
    for i, im in enumerate(images):
        face = app.best_face(im)
        assert records[i]["gate"] == app.last_verdict and (face is None) == (records[i]["gate"] != VERDICTS[0])
        emb = face.embedding if face is not None else np.zeros(512, np.float32)
        one = twin.group_visits(emb[None], via="loop", **thr)[0]
        assert (one["verdict"], one["person_id"]) == (records[i]["verdict"], records[i]["person_id"]), i
        assert abs(one["similarity"] - records[i]["similarity"]) < 2e-3
    assert records[2]["verdict"] == "no face" and records[2]["gate"] == "confidence too low" and counters["no_faces"] == 1
    assert records[0]["verdict"] == records[1]["verdict"] == "new" and records[0]["similarity"] == 1.0          # (the store was empty)
    assert [(records[i]["verdict"], records[i]["person_id"]) for i in (3, 5)] == [("duplicate", records[0]["person_id"]), ("duplicate", records[1]["person_id"])]
    assert counters["duplicate_faces"] == 2 and counters["new_persons"] >= 2
