"""GPU: fid_gallery_templates (identity templates on the device, csrc/template.hip), fid_gallery_put_rows_f16, VectorGallery.templates /
enroll_templates and FaceAnalysis.enroll_faces.

The rule takes its sums in integers, so the device must equal tests/template_oracle.py BYTE FOR BYTE on every output buffer and on any input --
also on random rows whose sums no float order would reproduce -- with canary bytes behind every output.  The cases are those of
tests/template_cases.py: the member counts at which the kernels take another path (one lane, a batch of 64 and its neighbours, one chunk, a
split person), positions outside the rule, cancellation, trimming, and the largest sums the rule admits."""
import ctypes as C

import numpy as np
import pytest

import template_cases as K
import template_oracle as O
from test_gpu_range_join import CANARY, canary_i32, gallery_rows

pytestmark = pytest.mark.gpu

PAGE = 4096
CASES = K.all_cases()


@pytest.fixture(scope="module")
def ctx():
    from scrfd_arcface_facerecognition_amd._lib import default_context
    return default_context(0)


def oracle(c):
    return O.templates(c["g16"], c["rows"], c["labels"], c["weights"], c["P"], c["min_score"])


class Store:
    """a gallery that holds the fp16 rows of a case exactly as given (they are written into the gallery's memory, not normalised)"""

    def __init__(self, ctx, g16):
        from scrfd_arcface_facerecognition_amd.engine import Gallery
        self.ctx, self.gal = ctx, Gallery(ctx, np.zeros(g16.shape, np.float32))
        self.before = np.zeros((self.gal.Gp, g16.shape[1]), np.float16)
        self.before[:len(g16)] = g16
        gallery_rows(ctx, self.gal).upload(self.before)

    def unchanged(self):
        return np.array_equal(gallery_rows(self.ctx, self.gal).download().view(np.uint16), self.before.view(np.uint16))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.gal.close()


def canary_outputs(ctx, n, P, dim):
    from scrfd_arcface_facerecognition_amd._lib import check
    bufs = [ctx.empty((P * dim + PAGE // 2,), np.float16), ctx.empty((n + PAGE // 4,), np.float32), ctx.empty((n + PAGE // 4,), np.int32),
            ctx.empty((4 * P + PAGE // 4,), np.int32), ctx.empty((P + PAGE // 4,), np.float32), ctx.empty((6 + PAGE // 8,), np.int64)]
    for b in bufs:
        check(ctx.lib.fid_memset(ctx.handle, C.c_void_p(b.ptr), CANARY, b.nbytes))
    return bufs


def fetch(bufs, n, P, dim):
    """-> the six outputs; nothing beyond them may have been written"""
    host = [b.download() for b in bufs]
    for h, m in zip(host, (P * dim, n, n, 4 * P, P, 6)):
        assert (h[m:].view(np.uint8) == CANARY).all()
    return (host[0][:P * dim].reshape(P, dim), host[1][:n], host[2][:n], host[3][:4 * P].reshape(P, 4), host[4][:P],
            tuple(int(v) for v in host[5][:6]))


def call(ctx, gal, rows_dev, labels_dev, weights_dev, n, P, min_score, outputs, null_ctx=False):
    from scrfd_arcface_facerecognition_amd._lib import _ptr
    return ctx.lib.fid_gallery_templates(None if null_ctx else ctx.handle, None if gal is None else gal.handle, _ptr(rows_dev), _ptr(labels_dev),
                                         _ptr(weights_dev), int(n), int(P), C.c_float(min_score), *[_ptr(o) for o in outputs])


def device_inputs(ctx, c):
    up = lambda a: None if a is None else ctx.to_device(a)
    return up(c["rows"]), up(c["labels"]), up(c["weights"])


def run(ctx, st, c, bufs=None):
    from scrfd_arcface_facerecognition_amd._lib import check
    n, P, dim = K.n_of(c), c["P"], c["g16"].shape[1]
    bufs = bufs or canary_outputs(ctx, n, P, dim)
    rows_dev, labels_dev, weights_dev = device_inputs(ctx, c)
    check(call(ctx, st.gal, rows_dev, labels_dev, weights_dev, n, P, c["min_score"], bufs))
    return fetch(bufs, n, P, dim)


# ---- the cases, byte for byte ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_device_equals_the_oracle_byte_for_byte(ctx, name):
    c = CASES[name]
    with Store(ctx, c["g16"]) as st:
        got, want = run(ctx, st, c), oracle(c)
        assert K.same(got, want) is None, K.same(got, want)
        assert st.unchanged()                                                         # the gallery is never written


def test_at_the_bound(ctx, monkeypatch):
    """2^20 positions of weight 255 on rows of +-2.0, all but one of them one person: per column |S| = (2^20 - 1) * 255 * 2^25, one position
    short of the header's bound, over 2^20 / CHUNK chunks that all add into one accumulator row -- and, in the second-pass form, store 4096
    partial rows that one wave adds up"""
    c = K.at_the_bound()
    want = oracle(c)
    with Store(ctx, c["g16"]) as st:
        for combine in ("atomics", "pass"):
            monkeypatch.setenv("FID_TEMPLATE_COMBINE", combine)
            got = run(ctx, st, c)
            assert K.same(got, want) is None, (combine, K.same(got, want))
        assert got[5] == (1 << 20, 2, 0, 0, 0, 0) and got[3][:, 0].tolist() == [(1 << 20) - 1, 1]


def test_order_freedom_and_two_runs(ctx):
    """the same case under a random permutation of its positions: byte-identical per-person outputs, permuted per-position outputs; and two
    calls in a row on the same outputs (no synchronise between them, the second reuses the scratch arena) give identical bytes"""
    from scrfd_arcface_facerecognition_amd._lib import check
    c = CASES["random_trimmed"]
    q, perm = K.permuted(c)
    n, P, dim = K.n_of(c), c["P"], 512
    with Store(ctx, c["g16"]) as st:
        t0, s0, k0, p0, c0, m0 = run(ctx, st, c)
        t1, s1, k1, p1, c1, m1 = run(ctx, st, q)
        assert m0 == m1 and np.array_equal(t0.view(np.uint16), t1.view(np.uint16)) and np.array_equal(c0.view(np.uint32), c1.view(np.uint32))
        assert np.array_equal(s0[perm].view(np.uint32), s1.view(np.uint32)) and np.array_equal(k0[perm], k1) and np.array_equal(p0[:, :2], p1[:, :2])
        assert np.array_equal(perm[p1[:, 2]], p0[:, 2]) or np.array_equal(s0[p0[:, 2]], s1[p1[:, 2]])      # (equal scores: the lowest position of each order)
        bufs = canary_outputs(ctx, n, P, dim)
        rows_dev, labels_dev, weights_dev = device_inputs(ctx, c)
        other = ctx.to_device(((np.arange(n) * 7) % P).astype(np.int32))
        check(call(ctx, st.gal, rows_dev, labels_dev, weights_dev, n, P, c["min_score"], bufs))
        first = [b.download() for b in bufs]
        check(call(ctx, st.gal, rows_dev, other, weights_dev, n, P, 0.5, bufs))        # other labels in between: nothing of them may stay
        check(call(ctx, st.gal, rows_dev, labels_dev, weights_dev, n, P, c["min_score"], bufs))
        second = [b.download() for b in bufs]
        assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(first, second))
        assert K.same(fetch(bufs, n, P, dim), oracle(c)) is None


def test_other_chunk_sizes_give_the_same_bytes(ctx, monkeypatch):
    """FID_TEMPLATE_CHUNK in the environment moves the split: 16 makes five of the seven persons split ones; FID_TEMPLATE_COMBINE=pass
    combines them through partial rows and a second pass instead of the atomics.  At dim 512 and at dim 1536 (three blocks of columns)."""
    for name in ("seven_trimmed_dim512", "seven_trimmed_dim1536"):
        c = CASES[name]
        want = oracle(c)
        with Store(ctx, c["g16"]) as st:
            for combine in ("atomics", "pass"):
                monkeypatch.setenv("FID_TEMPLATE_COMBINE", combine)
                for chunk in ("16", "64", "4096"):
                    monkeypatch.setenv("FID_TEMPLATE_CHUNK", chunk)
                    assert K.same(run(ctx, st, c), want) is None, (name, combine, chunk)


def test_argument_checks_enqueue_nothing(ctx):
    c = CASES["seven_dim32"]
    n, P = K.n_of(c), c["P"]
    with Store(ctx, c["g16"]) as st:
        rows_dev, labels_dev, weights_dev = device_inputs(ctx, c)
        outs = canary_outputs(ctx, n, P, 32)
        bad = lambda **k: call(ctx, **dict(dict(gal=st.gal, rows_dev=rows_dev, labels_dev=labels_dev, weights_dev=weights_dev, n=n, P=P,
                                                min_score=0.3, outputs=outs), **k))
        for m in (0, -3, (1 << 20) + 1):
            assert bad(n=m) == -1, m
        assert b"1048576" in ctx.lib.fid_last_error()
        for p in (0, -1, n + 1):
            assert bad(P=p) == -1, p
        for ms in (float("nan"), float("inf"), float("-inf")):
            assert bad(min_score=ms) == -1, ms
        assert bad(null_ctx=True) == -1 and bad(gal=None) == -1 and bad(labels_dev=None) == -1
        for i in range(6):
            assert bad(outputs=[None if j == i else o for j, o in enumerate(outs)]) == -1, i
        assert bad(outputs=outs[:5] + [outs[5].ptr + 4]) == -1                        # a misaligned summary
        assert bad(outputs=[outs[0].ptr + 2] + outs[1:]) == -1                        # ... and templates
        # (dim % 32 != 0, dim > 4096 and a gallery beyond 4 GiB cannot be reached from here: fid_gallery_create refuses the first, the others need the memory)
        ctx.sync()
        assert all((b.download().view(np.int32) == canary_i32()).all() for b in outs)
        assert st.unchanged()


# ---- fid_gallery_put_rows_f16 ----------------------------------------------------------------------------------------------------------------------
def test_put_rows_f16_copies_bytes_and_refuses_rows_outside(ctx):
    from scrfd_arcface_facerecognition_amd._lib import check
    g = K.gaussian_unit(20, 40, 64)
    with Store(ctx, g) as st:
        src = np.arange(5 * 64, dtype=np.uint16).reshape(5, 64) * 13 + 0x3001          # any bytes: these are no unit rows
        src_dev = ctx.to_device(src.view(np.float16))

        def put(rows, m):
            rows_dev = ctx.to_device(np.int32(rows))
            rc = ctx.lib.fid_gallery_put_rows_f16(ctx.handle, st.gal.handle, C.c_void_p(rows_dev.ptr), C.c_void_p(src_dev.ptr), m)
            ctx.sync()                                                                # (rows_dev is read by the copy)
            return rc
        for rows in ([3, 40, 7, 8, 9], [3, -1, 7, 8, 9], [0, 1, 2, 3, 2 ** 31 - 1]):
            assert put(rows, 5) == -1 and st.unchanged()                              # one row outside refuses the whole call
        assert put([1, 2, 3, 4, 5], 0) == -1 and st.unchanged()
        check(put([39, 0, 17, 5, 6], 5))
        now = gallery_rows(ctx, st.gal).download().view(np.uint16)
        want = st.before.view(np.uint16).copy()
        want[[39, 0, 17, 5, 6]] = src
        assert np.array_equal(now, want)                                              # the bytes of the source; every other row, and the padding, unchanged


# ---- through the Python layer ----------------------------------------------------------------------------------------------------------------------
def noisy_persons(seed, persons, copies, noise=0.5):
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((persons, 512))
    return (np.repeat(centres, copies, axis=0) + noise * rng.standard_normal((persons * copies, 512))).astype(np.float32)


def test_templates_and_enroll_templates_through_the_vector_gallery(ctx):
    from scrfd_arcface_facerecognition_amd import engine
    from scrfd_arcface_facerecognition_amd._lib import check
    x = noisy_persons(21, 8, 10)
    x[23] = np.random.default_rng(22).standard_normal(512)                            # a stranger under person 2's name
    x[71] = -x[70]
    ids = [(k % 3, 1000 - k) for k in range(80)]                                      # tuples, in no order
    names = {i: f"person {k // 10}" for k, i in enumerate(ids)}
    names[ids[71]] = names[ids[70]] = "cancels"                                       # a ninth person whose two faces cancel
    names[ids[5]] = None
    quality = {i: 1.0 - 0.01 * (k % 7) for k, i in enumerate(ids)}
    quality[ids[70]] = quality[ids[71]] = 1.0
    quality[ids[6]] = 0.0
    src, into = engine.VectorGallery(ctx, 512, capacity=128), engine.VectorGallery(ctx, 512, capacity=4)
    try:
        src.upsert(ids, x)
        into.upsert(["person 0", "someone else"], np.stack([x[40], np.random.default_rng(24).standard_normal(512).astype(np.float32)]))
        # (person 0 is known already, under a face of person 4: its row is overwritten)
        stored = gallery_rows(ctx, src._gal).download()
        order = sorted(ids)
        g16 = np.stack([stored[src.row_of[i]] for i in order])
        codes, w = engine.label_codes(order, names), engine.weight_codes(order, quality)
        res = src.templates(names, quality, 0.5)
        want = O.templates(g16, None, codes, w, 9, 0.5)
        got = (res.templates, res.score_pos, res.kept_pos, res.person_pos, res.cohesion, tuple(res.summary))
        assert K.same(got, want) is None, K.same(got, want)
        assert res.ids == order and len(res.persons) == 9 and res.zero == ["cancels"]
        assert res.dropped == sorted([ids[23], ids[70], ids[71]])                     # the stranger, and the two that cancel: they score 0 against a zero row
        assert ids[5] not in res.scores and ids[6] not in res.scores and res.counts["took_part"] == 78
        assert {i for i, _ in res.weakest(3)} == {ids[23], ids[70], ids[71]}          # the two that cancel score 0 against their zero template
        # enrol: the non-zero templates enter `into` under the person, byte for byte, without passing through the host
        into._gal._quant = True                                                       # (as if an int8 copy were current)
        res2 = src.enroll_templates(names, into, quality, 0.5)
        assert np.array_equal(res2.templates.view(np.uint16), res.templates.view(np.uint16)) and into._gal._quant is False
        assert sorted(map(str, into.row_of)) == sorted([f"person {p}" for p in range(8)] + ["someone else"]) and "cancels" not in into.row_of
        rows_now = gallery_rows(ctx, into._gal).download()
        for p, person in enumerate(res.persons):
            if person != "cancels":
                assert np.array_equal(rows_now[into.row_of[person]].view(np.uint16), res.templates[p].view(np.uint16)), person
        # every kept member finds its person in the target store, at the oracle's score against the FINAL template up to the order of the
        # search's fp32 sum: |difference| <= dim * 2^-24 * sum |q_c t_c| for any order (products of two fp16 values are exact in fp32)
        kept = [k for k in range(80) if res.kept_pos[k] == 1]
        q16 = np.ascontiguousarray(g16[kept])
        idx, sc, q_dev = ctx.empty((len(kept), 1), np.int32), ctx.empty((len(kept), 1), np.float32), ctx.to_device(q16)
        check(ctx.lib.fid_gallery_search(ctx.handle, into._gal.handle, C.c_void_p(q_dev.ptr), len(kept), 1, C.c_float(0.0),
                                         C.c_void_p(idx.ptr), C.c_void_p(sc.ptr)))
        I, S = idx.download()[:, 0], sc.download()[:, 0]
        for j, k in enumerate(kept):
            p = int(codes[k])
            assert into.id_of[int(I[j])] == res.persons[p], (k, p)
            D = int((O.fixed(g16[k]) * O.fixed(res.templates[p])).sum())
            exact = np.float32(np.float64(D) * 2.0 ** -48)
            margin = 512 * 2.0 ** -24 * float(np.abs(g16[k].astype(np.float64) * res.templates[p].astype(np.float64)).sum())
            assert abs(float(S[j]) - float(exact)) <= margin, (k, S[j], exact)
        hit = into.search(x[[0, 15, 33]], k=1)                                        # ... and through the public search
        assert [h[0][0] for h in hit] == ["person 0", "person 1", "person 3"]
        with pytest.raises(ValueError):
            src.enroll_templates(names, src)
        sub = src.templates(names, ids=order[::2])
        assert sub.ids == order[::2] and sub.dropped == [] and sub.counts["dropped"] == 0
    finally:
        src._gal.close()
        into._gal.close()
    empty = engine.VectorGallery(ctx, 512, capacity=8)
    res = empty.templates({})
    assert res.persons == [] and res.templates.shape == (0, 512) and res.weakest(2) == []
    empty._gal.close()


def test_merge_targets_on_the_device_equals_the_host_twin_on_stored_rows(ctx):
    from scrfd_arcface_facerecognition_amd.pipeline import merge_targets
    x = noisy_persons(23, 3, 4)
    names = ["ann", "bob", "cy"]
    targets = [(x[k], names[k // 4]) for k in (4, 0, 8, 1, 5, 9, 2, 6, 10, 3, 7, 11)]
    merged = merge_targets(ctx, targets)
    assert [m[1] for m in merged] == ["bob", "ann", "cy"]
    host = merge_targets(None, targets)
    for (a, _), (b, _) in zip(merged, host):                                          # (the device normalises in fp32, the host in fp64: stored rows may differ in the last fp16 place)
        assert float(a @ b) > 0.9999


def test_enroll_faces_smoke(ctx, monkeypatch):
    """synthetic weights, a handful of small images: one row per labelled person with a face"""
    monkeypatch.setenv("FID_AUTOTUNE", "0")
    from models import SCRFD
    from oracle import align as oalign
    from scrfd_arcface_facerecognition_amd import archs
    from scrfd_arcface_facerecognition_amd.app import FaceAnalysis
    from scrfd_arcface_facerecognition_amd.pipeline import calibrate_detector_bias
    from scrfd_arcface_facerecognition_amd.session import HipSession
    rng = np.random.default_rng(14)
    images = [rng.integers(0, 256, (240, 320, 3), dtype=np.uint8) for _ in range(4)]
    det_net = archs.scrfd_500m((320, 320))
    lb = np.stack([oalign.letterbox(im, (320, 320))[0] for im in images])
    det_P, _ = calibrate_detector_bias(ctx, det_net, archs.synth_params(det_net, 5), lb, target=30, max_batch=8)
    det = SCRFD("synthetic:scrfd_500m?seed=5", input_size=(320, 320), conf_thres=0.5, max_batch=8)
    det.session = HipSession(None, ctx=det.ctx, net=det_net, params=det_P, max_batch=8)
    app = FaceAnalysis("synthetic:scrfd_500m?seed=5", "synthetic:arcface_mbf?seed=5", det_size=(320, 320), max_faces=16)
    app.det = det
    images.append(np.zeros((240, 320, 3), np.uint8))                                 # (whatever the synthetic detector makes of it)
    labels = ["ann", "ann", "bob", None, "bob"]
    with_face = [b for b, fs in enumerate(app.get_batch(images, max_num=1)) if len(fs)]
    assert len(with_face) >= 4
    store, res = app.enroll_faces(images, labels)
    try:
        named = [labels[b] for b in with_face if labels[b] is not None]
        assert res.ids == with_face and res.persons == list(dict.fromkeys(named)) and res.counts["took_part"] == len(named)
        assert res.count.tolist() == [named.count(p) for p in res.persons] and res.dropped == []
        assert sorted(store.row_of) == sorted(p for p, c in zip(res.persons, res.cohesion) if c > 0) and len(store) >= 1
        assert res.templates.shape == (len(res.persons), 512)
    finally:
        store._gal.close()
    with pytest.raises(ValueError):
        app.enroll_faces(images, ["ann"])
