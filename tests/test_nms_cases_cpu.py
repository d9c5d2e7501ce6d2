"""CPU: the planted NMS lists of tests/nms_cases.py against the oracle alone.  Every list holds what it claims (the overlaps recomputed with the
oracle's arithmetic), goes through the head tensors unchanged, keeps between a quarter and three quarters of its candidates with the last one
among them -- and is SHARP: five wrong versions of the greedy loop, each the kind of slip nms_select's seams invite, return another keep list on
every list they apply to.  tests/test_gpu_postprocess_edges.py runs the same lists on the device."""
import numpy as np
import pytest

import nms_cases as nc
from oracle import postprocess as pp

CASES = nc.all_cases()
IDS = [f"cap{cc}-K{K}-{v}" for cc, K, _, v in CASES]


def iou(a, b):
    """oracle/postprocess.py nms, one pair, fp32"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    area = lambda r: (r[2] - r[0] + 1) * (r[3] - r[1] + 1)
    w = np.maximum(np.float32(0.0), np.minimum(a[2], b[2]) - np.maximum(a[0], b[0]) + 1)
    h = np.maximum(np.float32(0.0), np.minimum(a[3], b[3]) - np.maximum(a[1], b[1]) + 1)
    inter = w * h
    return inter / (area(a) + area(b) - inter)


def oracle_keep(cc, K, v):
    return list(nc.oracle_keep(cc, K, v))


def nms_mutant(dets, thr, word_blind=False, transitive=False, truncated=False, n_box=None, strict=False):
    """pp.nms with one slip.  word_blind: candidates whose ranks lie in different blocks of 64 never suppress each other;  transitive: a
    suppressed candidate still suppresses;  truncated: the last-ranked candidate is ignored;  n_box: candidates of rank >= n_box neither suppress
    nor get suppressed;  strict: ovr < thr keeps, in place of <=."""
    x1, y1, x2, y2, scores = dets[:, 0], dets[:, 1], dets[:, 2], dets[:, 3], dets[:, 4]
    areas = (x2 - x1 + 1) * (y2 - y1 + 1)
    order = scores.argsort(kind="stable")[::-1]
    K = len(order) - (1 if truncated else 0)
    removed = np.zeros(len(order), bool)
    keep = []
    for r in range(K):
        i = order[r]
        if not removed[r]:
            keep.append(int(i))
        elif not transitive:
            continue
        rest = order[r + 1:K]
        w = np.maximum(0.0, np.minimum(x2[i], x2[rest]) - np.maximum(x1[i], x1[rest]) + 1)
        h = np.maximum(0.0, np.minimum(y2[i], y2[rest]) - np.maximum(y1[i], y1[rest]) + 1)
        inter = w * h
        ovr = inter / (areas[i] + areas[rest] - inter)
        hit = ~(ovr < thr) if strict else ~(ovr <= thr)
        ranks = np.arange(r + 1, K)
        if word_blind:
            hit &= (ranks >> 6) == (r >> 6)
        if n_box is not None:
            hit &= (ranks < n_box) & (r < n_box)
        removed[r + 1:K] |= hit
    return keep


def test_mutant_without_a_slip_is_the_oracle():
    for cc, K, v in ((513, 513, 0), (4096, 1025, 0)):
        assert nms_mutant(nc.case(cc, K, v)[0], nc.THR) == oracle_keep(cc, K, v)


def test_regime_mirror_on_the_values_worked_out_by_hand():
    """csrc/postproc.hip nms_lds_bytes: 160 KB of LDS, 9 bytes per candidate in front of the boxes, 32 KB of masks behind at least 512 boxes"""
    assert nc.nms_regime(4096, 40) == (1024, True, "mask")
    assert nc.nms_regime(12742, 1024)[:2] == (1024, True) and nc.nms_regime(12743, 1024) == (1023, True, "loop_mixed")
    assert nc.nms_regime(13000, 879) == (879, True, "loop_lds")
    assert nc.nms_regime(13652, 512) == (512, True, "mask") and nc.nms_regime(13653, 512) == (511, False, "loop_mixed")
    assert nc.nms_regime(16800, 40) == (511, False, "loop_lds")
    assert {cc: nc.nms_regime(cc, 1)[0] for cc in nc.N_BOX} == nc.N_BOX


@pytest.mark.parametrize("cc, K, path, v", CASES, ids=IDS)
def test_case_takes_the_path_it_names(cc, K, path, v):
    assert nc.nms_regime(cc, K)[2] == path


@pytest.mark.parametrize("cc, K, path, v", CASES, ids=IDS)
def test_planted_structure_is_what_it_claims(cc, K, path, v):
    dets, plan = nc.case(cc, K, v)
    rank = plan["rank"]
    row = np.argsort(rank)                                        # rank -> row
    s = dets[:, 4]
    assert dets.dtype == np.float32 and dets.shape == (K, 5)
    assert np.array_equal(np.argsort(-s.astype(np.float64), kind="stable"), row) and len(np.unique(s)) == K and s.min() >= 0.5 and s.max() < 1
    assert np.array_equal(dets[:, :4], np.round(dets[:, :4]))
    assert K < 3 or not np.array_equal(rank, np.arange(K))        # shuffled: rank != row
    box = lambda r: dets[row[r], :4]
    keep = set(int(rank[i]) for i in oracle_keep(cc, K, v))      # the survivors, as ranks
    if plan["last"] is None:                                      # variant 1 of a list whose last rank is a seam: suppressed across it
        assert v == 1 and K - 1 not in keep and (K - 2, K - 1) in plan["pairs"] and nc.case(cc, K, 0)[1]["last"] == K - 1
    else:
        assert plan["last"] == K - 1 and K - 1 in keep
    if K < nc.MIN_PLANTED:
        assert len(keep) == K
        return
    seams = nc.boundaries_for(cc, K)
    for a, b in plan["pairs"]:
        assert a < b and iou(box(a), box(b)) > nc.THR and a in keep and b not in keep, (a, b)
    for a, b, c in plan["triples"]:
        assert a < b < c and iou(box(a), box(b)) > nc.THR and iou(box(b), box(c)) > nc.THR and iou(box(a), box(c)) <= nc.THR, (a, b, c)
        assert a in keep and b not in keep and c in keep, (a, b, c)
    for m in seams:
        if m != plan["last"]:                                     # rank m - 1 itself suppresses rank m, unless the seam under m took it
            assert any(b == m and (a == m - 1 or m - 1 in seams) for a, b in plan["pairs"]), m
        if m != K - 1 or plan["last"] is not None:
            assert any(b < m <= c for _, b, c in plan["triples"]), m
    assert plan["triples"]
    first, far = plan["far"]
    assert first == 0 and far >= K - 8 and iou(box(first), box(far)) > nc.THR and far not in keep
    p, q = plan["exact"]
    assert iou(box(p), box(q)) == np.float32(nc.THR) and p in keep and q in keep
    # nothing else: a candidate is suppressed exactly when the plan says so
    planned = {b for _, b in plan["pairs"]} | {b for _, b, _ in plan["triples"]} | {far}
    assert keep == set(range(K)) - planned
    # the fixture's condition: a quarter to three quarters survive
    assert 0.25 * K <= len(keep) <= 0.75 * K, (len(keep), K)


@pytest.mark.parametrize("cc, K, path, v", [c for c in CASES if c[1] <= 1025 and c[0] != c[1]], ids=lambda x: str(x))
def test_heads_decode_to_the_list(cc, K, path, v):
    dets, _ = nc.case(cc, K, v)
    heads = nc.heads_from_dets(dets, (640, 640), seed=v)
    det, kps = pp.detect_from_heads(heads, (640, 640), conf_thres=0.5, iou_thres=nc.THR)
    assert np.array_equal(det, dets[oracle_keep(cc, K, v)])
    assert kps.shape == (len(det), 5, 2) and np.abs(kps).max() > 0


def test_heads_decode_to_the_list_at_a_non_square_input():
    dets, _ = nc.case(16800, 40, 0)
    heads = nc.heads_from_dets(dets, (96, 160))
    det, _ = pp.detect_from_heads(heads, (96, 160), input_size=(160, 96), conf_thres=0.5, iou_thres=nc.THR)
    assert np.array_equal(det, dets[oracle_keep(16800, 40, 0)])


MUTANTS = {
    # K = 65: the one candidate of the second word is the last, a survivor in variant 0 whatever the words do; variant 1 catches the slip
    "word_blind": (dict(word_blind=True), lambda cc, K, path, last: K > 65 or (K == 65 and last is None)),
    # a list of fewer than MIN_PLANTED candidates (K = 1, 2) has no suppression at all
    "transitive": (dict(transitive=True), lambda cc, K, path, last: K >= nc.MIN_PLANTED),
    "truncated": (dict(truncated=True), lambda cc, K, path, last: last is not None),
    # K = n_box + 1: the one candidate past n_box is the last.  Where it survives (the fixture's own condition) it survives blind or not; the
    # case's variant 1, whose last rank is suppressed across the seam, is the list that catches this slip
    "box_blind": (None, lambda cc, K, path, last: path == "loop_mixed" and (K > nc.nms_regime(cc, K)[0] + 1 or last is None)),
    "strict": (dict(strict=True), lambda cc, K, path, last: K >= nc.MIN_PLANTED),
}


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_every_mutant_is_caught_on_every_case_it_applies_to(name):
    kw, applies = MUTANTS[name]
    n = 0
    for cc, K, path, v in CASES:
        dets, plan = nc.case(cc, K, v)
        if not applies(cc, K, path, plan["last"]):
            continue
        got = nms_mutant(dets, nc.THR, **(kw if kw is not None else dict(n_box=nc.nms_regime(cc, K)[0])))
        assert got != oracle_keep(cc, K, v), (name, cc, K, v)
        n += 1
    assert n >= {"box_blind": 6}.get(name, 20), n               # box_blind: every loop_mixed case, through its variant 1 where K = n_box + 1
