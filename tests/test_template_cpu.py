"""CPU: identity templates without a device -- fid_templates_host (csrc/template_core.h) and utils.helpers.identity_templates against
tests/template_oracle.py byte for byte on every case of tests/template_cases.py, the refusals, the TemplateResult accessors, the weight mapping
and pipeline.merge_targets."""
import ctypes as C

import numpy as np
import pytest

import template_cases as K
import template_oracle as O
from scrfd_arcface_facerecognition_amd import _lib, engine

CASES = K.all_cases()
FILL = 0x5A


def host_call(c, drop=None, **over):
    """-> (return code, the six outputs); outputs are pre-filled with 0x5A bytes; drop = the name of an output to pass as NULL"""
    c = dict(c, **over)
    g, n, P = c["g16"], K.n_of(c), max(c["P"], 0)
    dim = g.shape[1]
    outs = dict(templates=np.empty((P, dim), np.float16), score=np.empty(n, np.float32), kept=np.empty(n, np.int32), person=np.empty((P, 4), np.int32),
                cohesion=np.empty(P, np.float32), summary=np.empty(6, np.int64))
    for a in outs.values():
        a.view(np.uint8).reshape(-1)[:] = FILL
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = _lib.load().fid_templates_host(p(g), c.get("G", g.shape[0]), c.get("dim", dim), p(c["rows"]), p(c["labels"]), p(c["weights"]),
                                        c.get("n", n), c["P"], C.c_float(c["min_score"]), *[None if k == drop else p(a) for k, a in outs.items()])
    return rc, (outs["templates"], outs["score"], outs["kept"], outs["person"], outs["cohesion"], tuple(int(v) for v in outs["summary"]))


def oracle(c):
    return O.templates(c["g16"], c["rows"], c["labels"], c["weights"], c["P"], c["min_score"])


@pytest.fixture(scope="module")
def wants():
    return {name: oracle(c) for name, c in CASES.items()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_twin_equals_the_oracle(wants, name):
    rc, got = host_call(CASES[name])
    assert rc == 0 and K.same(got, wants[name]) is None, K.same(got, wants[name])


def test_the_cases_do_what_they_are_for(wants):
    tpl, score, kept, person, cohesion, summary = wants["outside"]
    assert kept[:6].tolist() == [1] * 6 and (kept[6:18] == -1).all() and kept[18] == 1 and kept[19] == kept[20] == -1
    assert summary == (7, 3, 0, 0, 5, 0) and (score[kept < 0] == 0).all()           # rejected: the zero row, inf, NaN, above 2, below -2
    tpl, score, kept, person, cohesion, summary = wants["cancellation"]
    assert not tpl.view(np.uint16).any() and summary[:3] == (4, 1, 1) and cohesion[0] == 0 and (kept == 1).all() and (score == 0).all()
    tpl, score, kept, person, cohesion, summary = wants["planted_outlier"]
    assert np.nonzero(kept == 0)[0].tolist() == [K.planted_outlier()[1]] and person[1].tolist()[:3] == [12, 11, 17] and summary[3] == 1
    tpl, score, kept, person, cohesion, summary = wants["opposed_pair"]
    assert kept.tolist() == [0, 0, 1, 1] and not tpl[0].view(np.uint16).any() and tpl[1].view(np.uint16).any() and summary[2:4] == (1, 2)
    assert (score[:2] < 0.5).all() and cohesion[0] == 0 and person[0].tolist()[:2] == [2, 0]
    tpl, score, kept, person, cohesion, summary = wants["one_hot_at"]
    assert (score.view(np.uint32) == 0x3F800000).all() and (kept == 1).all() and (cohesion == 1).all() and person[3].tolist() == [70, 70, 6, 6]
    tpl, score, kept, person, cohesion, summary = wants["one_hot_above"]
    assert (score.view(np.uint32) == 0x3F800000).all() and (kept == 0).all() and not tpl.view(np.uint16).any() and summary[2:4] == (5, 80)
    tpl, score, kept, person, cohesion, summary = wants["random_trimmed"]
    assert 100 < summary[3] < 900 and summary[2] == 0                                # the re-sum path is really taken
    counts = wants["seven_dim512"][3][:, 0].tolist()
    assert counts == [1, 2, 63, 64, 65, K.CHUNK, 2 * K.CHUNK + 1]
    tpl = wants["random"][0].astype(np.float64)
    assert np.abs(np.sqrt((tpl * tpl).sum(1)) - 1).max() < 2e-3                       # unit rows, up to fp16 rounding


def test_keep_all_makes_first_and_final_templates_coincide(wants):
    c = CASES["random"]
    for ms in (-2.0, -5.0, -1e30):
        rc, got = host_call(c, min_score=ms)
        assert rc == 0 and K.same(got, wants["random"]) is None
    rc, got = host_call(c, min_score=-1.0)                                            # nothing scores below -1: the same answer through the other branch
    assert rc == 0 and K.same(got, wants["random"]) is None


def test_order_freedom_of_the_rule():
    c = CASES["random_trimmed"]
    q, perm = K.permuted(c)
    (t0, s0, k0, p0, c0, m0), (rc, (t1, s1, k1, p1, c1, m1)) = oracle(c), host_call(q)
    assert rc == 0 and m0 == m1
    assert np.array_equal(t0.view(np.uint16), t1.view(np.uint16)) and np.array_equal(c0.view(np.uint32), c1.view(np.uint32))
    assert np.array_equal(s0[perm].view(np.uint32), s1.view(np.uint32)) and np.array_equal(k0[perm], k1) and np.array_equal(p0[:, :2], p1[:, :2])
    assert np.array_equal(s0[p0[:, 2]], s1[p1[:, 2]]) and np.array_equal(s0[p0[:, 3]], s1[p1[:, 3]])      # (the position words name other positions)


def test_at_the_bound_on_the_host():
    c = K.at_the_bound()
    rc, got = host_call(c)
    want = oracle(c)
    assert rc == 0 and K.same(got, want) is None
    # |S| per column = (2^20 - 1) positions * 255 * 2^25: below 2^53, so the norm's squares come from exact doubles
    assert got[5] == (1 << 20, 2, 0, 0, 0, 0) and got[3][:, 0].tolist() == [(1 << 20) - 1, 1]
    assert np.array_equal(np.sign(got[0].astype(np.float32)), np.sign(c["g16"].astype(np.float32)))


def test_refusals_leave_the_outputs_untouched():
    c = CASES["seven_dim32"]
    n = K.n_of(c)
    bad = [dict(P=0), dict(P=-1), dict(P=n + 1), dict(n=0), dict(n=-4), dict(n=(1 << 20) + 1), dict(min_score=float("nan")),
           dict(min_score=float("inf")), dict(min_score=float("-inf")), dict(dim=0), dict(dim=4097), dict(G=0)]
    for over in bad:
        rc, got = host_call(c, **over)
        assert rc == -1 and _lib.load().fid_last_error() != b"", over
        assert all((np.ascontiguousarray(a).view(np.uint8) == FILL).all() for a in got[:5]) and got[5] == (0x5A5A5A5A5A5A5A5A,) * 6, over
    for name in K.NAMES:
        rc, got = host_call(c, drop=name)
        assert rc == -1, name
        assert all((np.ascontiguousarray(a).view(np.uint8) == FILL).all() for a in got[:5])
    assert host_call(dict(c, labels=None))[0] == -1


def test_f16_rounding_of_the_core_against_numpy():
    """the core's own fp32 -> fp16 rounding against numpy's, on templates with elements 2^10 and 2^24 times smaller than the largest: normal,
    small and subnormal halves, over a sweep of weights that moves the quotients across many roundings"""
    g = np.zeros((3, 32), np.float16)
    g[0, 0], g[1, 1], g[2, 2] = 1.0, 2.0 ** -10, 2.0 ** -24
    seen_subnormal = False
    for w0 in (1, 3, 255):
        for w1 in (1, 7, 254):
            c = K.case(g, [0, 1, 2, 2], [0, 0, 0, 0], [w0, w1, 5, 250], 1)
            rc, got = host_call(c)
            want = oracle(c)
            assert rc == 0 and K.same(got, want) is None
            seen_subnormal |= bool(0 < (int(want[0].view(np.uint16)[0, 2]) & 0x7FFF) < 0x0400)
    assert seen_subnormal


def test_weight_mapping():
    ids = list("abcdefghi")
    q = dict(a=1.0, b=0.5, c=0.001, d=0.0, e=-0.3, f=float("nan"), g=2.0, h=0.25)    # i is missing
    assert engine.weight_codes(ids, q).tolist() == [255, 128, 1, 0, 0, 0, 255, 64, 0]
    assert engine.weight_codes(ids, None).tolist() == [1] * 9 and engine.weight_codes(ids, None).dtype == np.int32
    assert engine.weight_codes(["x"], {"x": 0.0999}).tolist() == [25] and engine.weight_codes(["x"], {"x": 0.5 / 255}).tolist() == [1]   # rint(0.5) = 0 -> 1


def test_identity_templates_and_the_result_accessors():
    from utils.helpers import identity_templates
    c = CASES["planted_outlier"]
    x = c["g16"].astype(np.float32) * 3.5                                             # any scale: normalised again (to the same fp16 rows or a neighbour)
    names = ["ann"] * 12 + ["bob"] * 12 + ["cy"] * 12
    names[31] = None
    quality = [(k % 5) / 4 for k in range(36)]                                        # every fifth face has quality 0: it takes no part
    res = identity_templates(x, names, quality, 0.5)
    ids = list(range(36))
    codes, w = engine.label_codes(ids, dict(enumerate(names))), engine.weight_codes(ids, dict(enumerate(quality)))
    n = np.sqrt((x.astype(np.float64) ** 2).sum(1, keepdims=True))
    want = O.templates((x / n).astype(np.float16), None, codes, w, 3, 0.5)
    got = (res.templates, res.score_pos, res.kept_pos, res.person_pos, res.cohesion, tuple(res.summary))
    assert K.same(got, want) is None
    assert res.persons == ["ann", "bob", "cy"] and res.templates.dtype == np.float16 and res.templates.shape == (3, 512)
    part = [k for k in ids if k % 5 and k != 31]
    assert sorted(res.scores) == part and res.dropped == [17] and res.zero == [] and res.count.tolist() == [9, 10, 8] and res.kept.tolist() == [9, 9, 8]
    assert res.counts == dict(took_part=27, persons=3, zero=0, dropped=1, rejected=0)
    assert res.weakest(1)[0][0] == 17 and [i for i, _ in res.weakest(3)] == sorted(part, key=lambda k: (res.scores[k], k))[:3]
    assert res.weakest(0) == [] and len(res.weakest(100)) == 27
    assert res.lowest[1] == 17 and res.highest[1] in part and np.array_equal(res.template("cy"), res.templates[2])
    assert (res.cohesion > 0.8).all() and (res.cohesion <= 1).all()
    # a mapping instead of sequences, and nobody labelled
    again = identity_templates(x, dict(enumerate(names)), dict(enumerate(quality)), 0.5)
    assert np.array_equal(again.templates.view(np.uint16), res.templates.view(np.uint16))
    empty = identity_templates(x, [None] * 36)
    assert empty.persons == [] and empty.templates.shape == (0, 512) and empty.scores == {} and empty.weakest(3) == [] and empty.counts["took_part"] == 0
    lost = identity_templates(c["g16"][[0, 12]], ["ann", "ann"], None, 0.9)          # two strangers under one name: both dropped
    assert lost.zero == ["ann"] and lost.dropped == [0, 1] and lost.cohesion[0] == 0 and lost.counts["zero"] == 1
    with pytest.raises(ValueError):
        identity_templates(x, names[:5])
    with pytest.raises(ValueError):
        identity_templates(x, names, quality[:5])


def test_merge_targets_on_the_host():
    from scrfd_arcface_facerecognition_amd.pipeline import merge_targets
    from utils.helpers import identity_templates
    c = CASES["planted_outlier"]
    x = c["g16"].astype(np.float32)
    names = ["bob"] * 12 + ["ann"] * 12 + ["cy"] * 12
    order = np.random.default_rng(3).permutation(36)
    targets = [(x[k] * 2.0, names[k]) for k in order]
    merged = merge_targets(None, targets)
    first_seen = list(dict.fromkeys(names[k] for k in order))
    assert [m[1] for m in merged] == first_seen and all(m[0].dtype == np.float32 and m[0].shape == (512,) for m in merged)
    res = identity_templates(x[order] * 2.0, [names[k] for k in order])
    for (emb, name), row in zip(merged, res.templates):
        assert np.array_equal(emb, row.astype(np.float32))
    trimmed = merge_targets(None, targets, min_score=0.5)
    assert [m[1] for m in trimmed] == first_seen and not np.array_equal(trimmed[first_seen.index("ann")][0], merged[first_seen.index("ann")][0])
    assert merge_targets(None, []) == []
    assert [m[1] for m in merge_targets(None, [(x[0], "a"), (-x[0], "a"), (x[1], "b")])] == ["b"]       # a's two entries cancel: no template
