"""GPU: fid_gallery_dedup (the duplicate-merge walk on the device, csrc/dedup.hip) and VectorGallery.find_and_merge_duplicates(via="device").

Exact probes (test_gpu_range_join.py): rows of +-1 / 0 with 4, 16 or 64 non-zeros have unit entries that fp16 holds exactly, so every cosine is an exact
multiple of 1/64 in fp32 whatever the summation order: keeper, score, summary and the gallery bytes afterwards must equal tests/dedup_oracle.py
bit for bit, also at a threshold that is itself attained.  Positions are cut into blocks of 128: the planted pairs sit inside a block, across the
127 | 128 seam and two blocks apart, the gallery has free holes and `rows` is deliberately not ascending."""
import ctypes as C

import numpy as np
import pytest

from dedup_oracle import applied, walk
from test_gpu_range_join import CANARY, canary_i32, gallery_rows, near_copy_store, probe_rows, prototypes, shuffled_store, unit_f16

pytestmark = pytest.mark.gpu

PAGE = 4096
ABOVE = float(np.nextafter(np.float32(0.75), np.float32(1.0)))


@pytest.fixture(scope="module")
def ctx():
    from scrfd_arcface_facerecognition_amd._lib import default_context
    return default_context(0)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


# ---- the entry point -----------------------------------------------------------------------------------------------------------------------------
def dedup_call(ctx, gal, rows_dev, n, thresh, apply, outputs, null_ctx=False):
    """fid_gallery_dedup's return code; outputs = (keeper, score, summary) device buffers (or None); gal may be None, null_ctx passes a NULL context"""
    from scrfd_arcface_facerecognition_amd._lib import _ptr
    k, s, m = outputs
    return ctx.lib.fid_gallery_dedup(None if null_ctx else ctx.handle, None if gal is None else gal.handle, _ptr(rows_dev), int(n),
                                     C.c_float(thresh), int(apply), _ptr(k), _ptr(s), _ptr(m))


def canary_outputs(ctx, n):
    from scrfd_arcface_facerecognition_amd._lib import check
    bufs = [ctx.empty((n + PAGE // 4,), np.int32), ctx.empty((n + PAGE // 4,), np.float32), ctx.empty((2 + PAGE // 4,), np.int32)]
    for b in bufs:
        check(ctx.lib.fid_memset(ctx.handle, C.c_void_p(b.ptr), CANARY, b.nbytes))
    return bufs


def fetch(bufs, n):
    """-> keeper [n], score [n], summary; nothing beyond n entries (2 for the summary) may have been written"""
    k, s, m = (b.download() for b in bufs)
    assert (k[n:] == canary_i32()).all() and (s[n:].view(np.int32) == canary_i32()).all() and (m[2:] == canary_i32()).all()
    return k[:n], s[:n], (int(m[0]), int(m[1]))


def run_dedup(ctx, gal, rows, thresh, apply):
    from scrfd_arcface_facerecognition_amd._lib import check
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    bufs = canary_outputs(ctx, len(rows))
    check(dedup_call(ctx, gal, ctx.to_device(rows), len(rows), thresh, apply, bufs))
    return fetch(bufs, len(rows))


def assert_equals_oracle(got, want, what=""):
    assert np.array_equal(got[0], want[0]), (what, np.nonzero(got[0] != want[0])[0][:8])
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), (what, np.nonzero(got[1] != want[1])[0][:8])     # bit for bit
    assert got[2] == tuple(want[2]), what


def check_case(ctx, g, rows, thresh, what=""):
    """dry run, then the applying run, then a second applying run: each against the oracle on the gallery as it then is"""
    from scrfd_arcface_facerecognition_amd.engine import Gallery
    gal = Gallery(ctx, g)
    try:
        before = gallery_rows(ctx, gal).download()
        assert np.array_equal(bits(before[:len(g)]), bits(unit_f16(g)))             # the stored rows are the exact ones
        want = walk(before[:gal.G], rows, thresh)
        assert_equals_oracle(run_dedup(ctx, gal, rows, thresh, 0), want, what)
        assert np.array_equal(bits(gallery_rows(ctx, gal).download()), bits(before))                    # apply = 0 writes nothing
        assert_equals_oracle(run_dedup(ctx, gal, rows, thresh, 1), want, what)
        after = gallery_rows(ctx, gal).download()
        exp = before.copy()
        exp[:gal.G] = applied(before[:gal.G], rows, want[0])
        assert np.array_equal(bits(after), bits(exp))                               # exactly the absorbed rows are +0.0, padding rows included
        again = run_dedup(ctx, gal, rows, thresh, 1)
        assert_equals_oracle(again, walk(after[:gal.G], rows, thresh), what)
        assert again[2] == (0, want[2][1] - want[2][0]) and (again[0] == -1).all()
        assert np.array_equal(bits(gallery_rows(ctx, gal).download()), bits(after))
        return want
    finally:
        gal.close()


# ---- planted probe stores ------------------------------------------------------------------------------------------------------------------------
def flipped(proto, flips=()):
    p, sup = proto
    x = p.copy()
    x[sup[list(flips)]] *= -1
    return x


def probe_case(n, dim):
    """-> g [Gt, dim] of +-1 / 0 rows with free holes, rows [n] (a shuffle: not ascending), plants {name: (keeper position, position)}"""
    rng = np.random.default_rng(1000 * n + dim)
    fill, mine = prototypes(rng, dim), prototypes(rng, dim)
    x = probe_rows(rng, n, dim, fill, {})
    plants = {}
    # (kept prototype, flips of the later row) -> cosine 0.875 / 0.75 / 0.5 by one / two / four flips
    for name, j, k, proto, flips in (("block", 3, 9, 0, (1,)), ("seam", 127, 128, 1, (2,)), ("far", 5, 290, 2, (0, 3)), ("half", 6, 40, 3, (0, 1, 2, 3)),
                                     ("pair", 0, 1, 4, (5, 6))):
        if k < n:
            x[j], x[k] = flipped(mine[proto]), flipped(mine[proto], flips)
            plants[name] = (j, k)
    Gt = n + 7
    rows = rng.permutation(Gt)[:n]                                                  # seven rows stay free: holes anywhere in the gallery
    g = np.zeros((Gt, dim), np.float32)
    g[rows] = x
    return g, rows.astype(np.int32), plants


@pytest.mark.parametrize("dim", [32, 512])
@pytest.mark.parametrize("n", [1, 2, 127, 128, 129, 300])
def test_dedup_exact_probes(ctx, n, dim):
    g, rows, plants = probe_case(n, dim)
    assert n < 3 or not np.array_equal(rows, np.sort(rows))
    want = check_case(ctx, g, rows, 0.75, "0.75")
    keeper, score, summary = want
    assert summary[1] == n
    x16 = unit_f16(g)[rows].astype(np.float64)
    for name, (j, k) in plants.items():
        assert x16[j] @ x16[k] == {"block": 0.875, "seam": 0.875, "far": 0.75, "half": 0.5, "pair": 0.75}[name]
    # the planted rows are absorbed, by their planted keeper unless an earlier survivor of the random fill reaches them first
    for name in ("block", "seam", "far", "pair"):
        if name in plants:
            j, k = plants[name]
            assert 0 <= keeper[k] <= j and (keeper[j] >= 0 or keeper[k] == j), name
    if "seam" in plants:
        assert keeper[128] == 127 and score[128] == 0.875                          # across the 127 | 128 seam
    if "far" in plants:
        assert keeper[290] == 5 and score[290] == 0.75                             # two blocks apart, exactly at the threshold
    if "half" in plants:
        assert keeper[40] != 6
    if n > 2:
        above = check_case(ctx, g, rows, ABOVE, "above")
        assert above[2][0] < summary[0]
        if "far" in plants:
            assert above[0][290] == -1


# ---- constructed rows: operands exact in fp16, so the sums are exact in any order ------------------------------------------------------------------
def test_a_path_of_300_is_resolved_to_any_depth(ctx):
    """two-hot rows e_k + e_(k+1): components 0.70703125 = 181 / 256, neighbours at (181 / 256)^2 = 0.4998931884765625 (one product, exact in
    fp32), every other pair at 0"""
    n, dim = 300, 512
    x = np.zeros((n, dim), np.float32)
    x[np.arange(n), np.arange(n)] = 1
    x[np.arange(n), np.arange(n) + 1] = 1
    rng = np.random.default_rng(300)
    rows = rng.permutation(n + 20)[:n].astype(np.int32)
    g = np.zeros((n + 20, dim), np.float32)
    g[rows] = x
    assert float(unit_f16(x)[0, 0]) == 0.70703125
    keeper, score, summary = check_case(ctx, g, rows, 0.49)
    pos = np.arange(n)
    assert np.array_equal(keeper, np.where(pos % 2 == 1, pos - 1, -1))
    assert np.float32(0.4998931884765625) == np.float32(181.0 / 256.0) ** 2
    assert np.array_equal(score, np.where(pos % 2 == 1, np.float32(0.4998931884765625), np.float32(0)))
    assert summary == (150, 300)


def test_first_alive_not_best_and_the_threshold_is_inclusive(ctx):
    """four-hot rows with components exactly 0.5: a.c = 0.25, b.c = 0.75, a.b = 0"""
    dim = 32
    x = np.zeros((3, dim), np.float32)
    x[0, 0:4] = 1
    x[1, 4:8] = 1
    x[2, [0, 4, 5, 6]] = 1
    g = np.zeros((9, dim), np.float32)
    rows = np.asarray([7, 2, 4], np.int32)
    g[rows] = x
    keeper, score, summary = check_case(ctx, g, rows, 0.25)
    assert list(keeper) == [-1, -1, 0] and score[2] == 0.25 and summary == (1, 3)                  # `>=`: the low-rank survivor, weakly
    keeper, score, summary = check_case(ctx, g, rows, float(np.nextafter(np.float32(0.25), np.float32(1.0))))
    assert list(keeper) == [-1, -1, 1] and score[2] == 0.75 and summary == (1, 3)


# ---- rows that take no part ------------------------------------------------------------------------------------------------------------------------
def test_zero_and_marker_rows_survive_uncounted(ctx):
    from scrfd_arcface_facerecognition_amd.engine import Gallery
    n, dim = 200, 32
    g, rows, _ = probe_case(n, dim)
    zero, marker = [0, 64, 130, 199], [1, 127, 128]
    gal = Gallery(ctx, g)
    try:
        view = gallery_rows(ctx, gal)
        host = view.download()
        host[rows[zero + marker]] = 0
        bits(host)[rows[marker], 0] = 0x8000                                        # the -0.0-first marker row of an empty slot
        view.upload(host)
        want = walk(host[:gal.G], rows, 0.75)
        assert want[2][1] == n - 7 and want[2][0] > 10
        assert (want[0][zero + marker] == -1).all() and not np.isin(want[0], zero + marker).any()
        assert_equals_oracle(run_dedup(ctx, gal, rows, 0.75, 1), want)
        exp = host.copy()
        exp[:gal.G] = applied(host[:gal.G], rows, want[0])
        assert np.array_equal(bits(gallery_rows(ctx, gal).download()), bits(exp))  # the marker rows keep their sign bit
    finally:
        gal.close()


def test_rows_outside_the_gallery_take_no_part(ctx):
    from scrfd_arcface_facerecognition_amd.engine import Gallery
    n, dim = 140, 32
    g, rows, plants = probe_case(n, dim)
    G = len(g)
    bad = rows.copy()
    bad[plants["block"][0]], bad[plants["seam"][1]] = -1, G                         # a keeper and an absorbed position of the planted pairs
    gal = Gallery(ctx, g)
    try:
        before = gallery_rows(ctx, gal).download()
        want = walk(before[:G], bad, 0.75)
        assert want[2][1] == n - 2 and want[0][128] == -1 and want[1][128] == 0 and want[0][3] == -1
        good = walk(before[:G], rows, 0.75)
        assert good[0][128] == 127 and not np.array_equal(good[0], want[0])
        assert_equals_oracle(run_dedup(ctx, gal, bad, 0.75, 0), want)               # (run_dedup checks the canaries around all three outputs)
        assert np.array_equal(bits(gallery_rows(ctx, gal).download()), bits(before))
        assert_equals_oracle(run_dedup(ctx, gal, bad, 0.75, 1), want)
        exp = before.copy()
        inside = (bad >= 0) & (bad < G) & (want[0] >= 0)
        exp[bad[inside]] = 0
        assert np.array_equal(bits(gallery_rows(ctx, gal).download()), bits(exp))
    finally:
        gal.close()


def test_two_calls_back_to_back(ctx):
    """no synchronise between them: the second call sees the rows the first one cleared"""
    from scrfd_arcface_facerecognition_amd._lib import check
    from scrfd_arcface_facerecognition_amd.engine import Gallery
    g, rows, _ = probe_case(300, 32)
    gal = Gallery(ctx, g)
    try:
        before = gallery_rows(ctx, gal).download()
        want = walk(before[:gal.G], rows, 0.75)
        rows_dev = ctx.to_device(rows)
        first, second = canary_outputs(ctx, 300), canary_outputs(ctx, 300)
        check(dedup_call(ctx, gal, rows_dev, 300, 0.75, 1, first))
        check(dedup_call(ctx, gal, rows_dev, 300, 0.75, 1, second))
        assert_equals_oracle(fetch(first, 300), want)
        k, s, m = fetch(second, 300)
        assert (k == -1).all() and (s == 0).all() and m == (0, want[2][1] - want[2][0]) and want[2][0] > 20
    finally:
        gal.close()


def test_argument_checks_enqueue_nothing(ctx):
    from scrfd_arcface_facerecognition_amd.engine import Gallery
    g, rows, _ = probe_case(17, 32)
    gal = Gallery(ctx, g)
    try:
        before = gallery_rows(ctx, gal).download()
        rows_dev = ctx.to_device(rows)
        outs = canary_outputs(ctx, 17)
        for thr in (float("nan"), 0.0, -0.5):
            assert dedup_call(ctx, gal, rows_dev, 17, thr, 1, outs) == -1, thr
            assert ctx.lib.fid_last_error() != b""
        for n in (0, -3, (1 << 20) + 1):
            assert dedup_call(ctx, gal, rows_dev, n, 0.75, 1, outs) == -1, n
        assert b"1048576" in ctx.lib.fid_last_error()
        # (dim % 32 != 0 cannot be reached from here: fid_gallery_create refuses such a gallery)
        assert dedup_call(ctx, gal, rows_dev, 17, 0.75, 1, outs, null_ctx=True) == -1
        assert dedup_call(ctx, None, rows_dev, 17, 0.75, 1, outs) == -1
        assert dedup_call(ctx, gal, None, 17, 0.75, 1, outs) == -1
        for i in range(3):
            assert dedup_call(ctx, gal, rows_dev, 17, 0.75, 1, [None if j == i else o for j, o in enumerate(outs)]) == -1, i
        ctx.sync()
        assert all((b.download().view(np.int32) == canary_i32()).all() for b in outs)
        assert np.array_equal(bits(gallery_rows(ctx, gal).download()), bits(before))
    finally:
        gal.close()


# ---- realistic values, through the Python layer ------------------------------------------------------------------------------------------------
def twin_stores(ctx, emb, seed, capacity):
    """three stores with the same ids on the same embeddings, in the same rows"""
    out = []
    for _ in range(3):
        vg, ids = shuffled_store(ctx, np.random.default_rng(seed), emb, capacity)
        out.append(vg)
    return out, ids


def test_merge_via_device_equals_the_join_and_the_matrix_path(ctx):
    """Gaussian 512-dim embeddings with planted near-copies (test_gpu_range_join.near_copy_store), shuffled ids, 700 persons in 1 024 rows.  The
    scores get the tolerance test_realistic_values_against_float64_on_the_stored_rows grants fid_gallery_range's: the same operands and the same
    accumulation length, (K - 1) * 2^-24 * sum|a_i b_i| <= 3e-5 for unit rows -> 1e-4.  The decisions are only a fair demand where no pair's
    float64 cosine lies within 2e-3 of the threshold: asserted on the oracle's numbers first."""
    emb = near_copy_store(np.random.default_rng(11))
    (vd, vj, vm), ids = twin_stores(ctx, emb, 11, 1024)
    assert vd.row_of == vj.row_of == vm.row_of and vd._free == vj._free
    stored = gallery_rows(ctx, vd._gal).download()
    order = sorted(ids)
    rows = np.asarray([vd.row_of[i] for i in order])
    S = stored[rows].astype(np.float64) @ stored[rows].astype(np.float64).T
    assert np.abs(S[np.triu_indices(len(order), 1)] - 0.8).min() > 2e-3
    keeper, score, summary = walk(stored[:vd._gal.G], rows, 0.8)
    assert summary[0] >= 8 and summary[1] == len(ids)
    dry = vd.duplicate_keepers(0.8)
    assert dry.keys() == {order[k] for k in np.nonzero(keeper >= 0)[0]}
    assert all(dry[order[k]][0] == order[keeper[k]] and abs(dry[order[k]][1] - S[keeper[k], k]) < 1e-4 for k in np.nonzero(keeper >= 0)[0])
    assert np.array_equal(bits(gallery_rows(ctx, vd._gal).download()), bits(stored)) and vd.row_of == vj.row_of     # the dry run changed nothing
    got = vd.find_and_merge_duplicates(0.8, via="device")
    join = vj.find_and_merge_duplicates(0.8, via="join")
    dense = vm.find_and_merge_duplicates(0.8)
    assert len(got) == summary[0]
    assert [(a, b) for a, b, _ in got] == [(a, b) for a, b, _ in join] == [(a, b) for a, b, _ in dense]
    pos = {i: k for k, i in enumerate(order)}
    assert max(abs(s - S[pos[a], pos[b]]) for a, b, s in got) < 1e-4
    assert max(abs(g[2] - j[2]) for g, j in zip(got, join)) < 1e-4 and max(abs(g[2] - d[2]) for g, d in zip(got, dense)) < 1e-4
    assert vd.row_of == vj.row_of == vm.row_of and vd.id_of == vj.id_of and vd._free == vj._free == vm._free
    after = gallery_rows(ctx, vd._gal).download()
    assert np.array_equal(bits(after), bits(gallery_rows(ctx, vj._gal).download()))
    assert np.array_equal(bits(after), bits(gallery_rows(ctx, vm._gal).download()))
    assert vd.find_and_merge_duplicates(0.8, via="device") == [] and vd.duplicate_keepers(0.8) == {}
    with pytest.raises(ValueError):
        vd.find_and_merge_duplicates(0.8, via="dense")


def test_device_merge_of_an_empty_store_and_the_size_limit(ctx, monkeypatch):
    from scrfd_arcface_facerecognition_amd import engine
    vg = engine.VectorGallery(ctx, 512, capacity=8)
    assert vg.find_and_merge_duplicates(0.8, via="device") == [] and vg.duplicate_keepers(0.8) == {}
    vg.upsert([4, 2, 9], np.eye(3, 512, dtype=np.float32))
    monkeypatch.setattr(engine, "DEDUP_MAX_ROWS", 2)
    with pytest.raises(ValueError, match='via="join"'):
        vg.find_and_merge_duplicates(0.8, via="device")
    assert len(vg) == 3
