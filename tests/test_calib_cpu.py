"""CPU: the score-distribution rule (tests/calib_oracle.py, what fid_gallery_score_hist computes), the host twin (fid_score_hist_host,
utils.helpers.score_distribution) against the oracle bit for bit on the exact stores of tests/calib_cases.py, and engine.ScoreDistribution's
rates, thresholds and rankings on hand-made histograms with known answers."""
import ctypes as C
import math

import numpy as np
import pytest

import calib_cases as K
import calib_oracle as O

FILL, FILL64 = 0x4D4D4D4D, 0x4D4D4D4D4D4D4D4D


def host_call(g16, rows, labels, bins, n=None, null=None):
    """fid_score_hist_host -> (rc, (hist, imp_via, imp_score, gen_via, gen_score, summary)); null: the index of an output to pass as NULL"""
    from scrfd_arcface_facerecognition_amd import _lib
    g16 = np.ascontiguousarray(g16, np.float16)
    G, dim = g16.shape
    n = (G if rows is None else len(rows)) if n is None else n
    m = max(min(n, 1 << 12), len(labels), 1)
    b = bins if 2 <= bins <= 4096 else 4096
    outs = (np.full((2, b), FILL64, np.uint64), np.full(m, FILL, np.int32), np.full(m, FILL, np.int32).view(np.float32), np.full(m, FILL, np.int32),
            np.full(m, FILL, np.int32).view(np.float32), np.full(4, FILL64, np.uint64))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    r = None if rows is None else np.ascontiguousarray(rows, np.int32)
    lab = np.ascontiguousarray(labels, np.int32)
    rc = _lib.load().fid_score_hist_host(p(g16), G, dim, None if r is None else p(r), p(lab), n, bins,
                                         *[None if i == null else p(o) for i, o in enumerate(outs)])
    return rc, outs


def untouched(outs):
    return all((np.ascontiguousarray(o).view(np.uint32) == FILL).all() for o in outs)


# ---- the host twin ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, dim", K.PROBE_SHAPES)
def test_host_twin_equals_the_oracle_on_the_exact_stores(n, dim):
    g, rows, labels, plants = K.exact_case(n, dim)
    g16 = K.with_marker(K.unit_f16(g), plants)
    for bins in K.BINS:
        want = O.score_hist(g16, rows, labels, bins)
        rc, got = host_call(g16, rows, labels, bins)
        assert rc == 0 and K.same(got, want) is None, (bins, K.same(got, want))
        hist, imp_via, imp_score, gen_via, gen_score, summary = want
        took = summary[0]
        assert summary[1] + summary[2] == took * (took - 1) // 2 and summary[3] == 0
        # NULL rows: every gallery row is a position
        all_labels = (np.arange(len(g16)) % 5).astype(np.int32)
        all_labels[::11] = -1
        rc, got = host_call(g16, None, all_labels, bins)
        assert rc == 0 and K.same(got, O.score_hist(g16, None, all_labels, bins)) is None, bins
    if n >= 17:
        hist, imp_via, imp_score, gen_via, gen_score, summary = O.score_hist(g16, rows, labels, 64)
        off = plants["unlabelled"] + plants["outside"] + plants["hole"] + plants["marker"]
        assert summary[0] == n - len(set(off))
        assert (imp_via[off] == -1).all() and (gen_via[off] == -1).all() and (imp_score[off] == 0).all() and (gen_score[off] == 0).all()
        assert not np.isin(imp_via, off).any() and not np.isin(gen_via, off).any()
        a, b = plants["dup_same"]
        a, c = plants["dup_other"]
        assert hist[0][63] >= 1 and hist[1][63] >= 1                                    # s = 1 is clamped into the top bin on both sides
        assert imp_via[a] == c and imp_score[a] == 1.0 and imp_via[c] == a
        d, e = plants["negated"]
        assert labels[d] != labels[e] and hist[1][0] >= 1                               # s = -1: bin 0 of the impostor side
        assert gen_via[plants["lonely"]] == -1 and gen_score[plants["lonely"]] == 0 and imp_via[plants["lonely"]] >= 0
    if n >= 129:
        t, u, v = plants["tie"]
        S, _ = O.scores(g16, rows)
        assert S[t, u] == S[t, v] == imp_score[t] and imp_via[t] == u < v and (n < 300 or u // 128 != v // 128 != t // 128)


def test_every_score_sits_on_a_bin_edge_and_fp64_agrees():
    """the claim of calib_cases: at dim 512 every cosine is a multiple of 1/32, so fp32 and fp64 scores and bins are identical"""
    g, rows, labels, plants = K.exact_case(300, 512)
    g16 = K.unit_f16(g)
    S, has = O.scores(g16, rows)
    x = np.zeros((300, 512))
    ok = (rows >= 0) & (rows < len(g16))
    x[ok] = g16[rows[ok]].astype(np.float64)
    S64 = x @ x.T
    assert np.array_equal(S.astype(np.float64), S64) and np.array_equal(S64 * 32, np.round(S64 * 32))
    for bins in (64, 4096):
        assert np.array_equal(O.bin_of(S, bins), np.clip(np.floor(S64 * (bins // 2)) + bins // 2, 0, bins - 1).astype(np.int64))


def test_minus_zero_orders_below_plus_zero():
    w = O.sortable(np.float32([-1.0, -0.0, 0.0, 1e-30, 1.0]))
    assert (np.diff(w.astype(np.int64)) > 0).all()
    S = np.float32([[0, -0.0, 0.0], [-0.0, 0, 0.5], [0.0, 0.5, 0]])
    hist, imp_via, imp_score, gen_via, gen_score, summary = O.hist_scores(S, [True] * 3, [0, 1, 2], 2)
    assert imp_via[0] == 2 and np.signbit(imp_score[0]) == False                       # +0.0 beats -0.0 as the HIGHEST score
    hist, imp_via, imp_score, gen_via, gen_score, summary = O.hist_scores(S, [True] * 3, [0, 0, 0], 2)
    assert gen_via[0] == 1 and np.signbit(gen_score[0])                                 # -0.0 is the LOWEST
    assert tuple(hist[0]) == (0, 3)                                                     # both zeros fall into the bin that starts at 0


def test_non_finite_scores_are_counted_and_in_no_bin():
    x = np.zeros((6, 32), np.float32)
    x[:, K.support(32)] = np.random.default_rng(6).choice(np.float32([-1, 1]), (6, 16))
    g16 = K.unit_f16(x)
    g16[1, 0] = np.float16(np.inf)
    g16[2, 2] = np.float16(np.nan)
    labels = np.int32([0, 0, 1, 1, 0, 1])
    want = O.score_hist(g16, None, labels, 64)
    rc, got = host_call(g16, None, labels, 64)
    assert rc == 0 and K.same(got, want) is None
    assert want[5] == (6, want[5][1], want[5][2], 9) and want[5][1] + want[5][2] == 6           # rows 1 and 2 spoil 5 + 4 of the 15 pairs


def test_host_twin_argument_checks_write_nothing():
    g, rows, labels, plants = K.exact_case(17, 32)
    g16 = K.unit_f16(g)
    for bins, n in ((63, None), (0, None), (1, None), (-2, None), (4098, None), (5000, None), (64, 0), (64, -3), (64, (1 << 20) + 1)):
        rc, outs = host_call(g16, rows, labels, bins, n)
        assert rc == -1 and untouched(outs), (bins, n)
    for i in range(6):
        rc, outs = host_call(g16, rows, labels, 64, null=i)
        assert rc == -1 and untouched(outs), i
    from scrfd_arcface_facerecognition_amd import _lib
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    outs = host_call(g16, rows, labels, 64)[1]
    assert _lib.load().fid_score_hist_host(p(np.ascontiguousarray(g16)), len(g16), 32, p(rows), None, 17, 64, *[p(o) for o in outs]) == -1


def test_helper_normalises_and_names_rows():
    from utils.helpers import score_distribution
    g, rows, labels, plants = K.exact_case(129, 512)
    names = [None if l < 0 else f"person-{l}" for l in (np.arange(len(g)) % 5)]
    names[7] = None
    codes = np.int32([-1 if v is None else int(v.split("-")[1]) for v in names])
    res = score_distribution(g * 3.0, names, bins=64)                                   # (any scale: the helper normalises)
    want = O.score_hist(K.unit_f16(g), None, codes, 64)
    got = (np.stack([res.genuine, res.impostor]), res.imp_via_pos, res.imp_score_pos, res.gen_via_pos, res.gen_score_pos, res.summary)
    assert K.same(got, want) is None
    assert (res.took_part, res.genuine_pairs, res.impostor_pairs, res.non_finite) == want[5]
    assert res.edges[0] == -1 and res.edges[-1] == 1 and len(res.edges) == 65
    same_as_mapping = score_distribution(g, {k: v for k, v in enumerate(names) if v is not None}, bins=64)
    assert np.array_equal(same_as_mapping.impostor, res.impostor) and np.array_equal(same_as_mapping.gen_via_pos, res.gen_via_pos)
    with pytest.raises(ValueError):
        score_distribution(g, names, bins=7)


# ---- far(t) is the count of `s >= t` ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bins", [2, 64, 4096])
def test_far_times_impostor_pairs_is_a_brute_force_count_at_every_edge(bins):
    from scrfd_arcface_facerecognition_amd.engine import ScoreDistribution
    g, rows, labels, plants = K.exact_case(300, 512)
    g16 = K.with_marker(K.unit_f16(g), plants)
    want = O.score_hist(g16, rows, labels, bins)
    dist = ScoreDistribution(list(range(300)), *want)
    S, has = O.scores(g16, rows)
    part = has & (labels >= 0)
    iu = np.triu_indices(300, 1)
    ok = part[iu[0]] & part[iu[1]]
    s, imp = S[iu][ok], (labels[iu[0]] != labels[iu[1]])[ok]
    edges = range(bins) if bins <= 64 else range(0, bins, 61)
    for e in edges:                                                                     # (the last edge, 1.0, accepts nothing by definition)
        t = dist.edges[e]
        assert dist.far(t) * dist.impostor_pairs == pytest.approx(int((s[imp] >= np.float32(t)).sum()), abs=1e-6), e
        assert dist.frr(t) * dist.genuine_pairs == pytest.approx(int((s[~imp] < np.float32(t)).sum()), abs=1e-6), e
    assert dist.far(-1.0) == 1.0 and dist.frr(-1.0) == 0.0 and dist.far(1.0) == 0.0 and dist.frr(1.0) == 1.0


# ---- ScoreDistribution on hand-made histograms ----------------------------------------------------------------------------------------------------
def hand_made():
    from scrfd_arcface_facerecognition_amd.engine import ScoreDistribution
    #  bin:    0    1    2    3    4    5    6    7      edges -1, -.75, -.5, -.25, 0, .25, .5, .75, 1
    gen = [0, 0, 0, 1, 1, 2, 6, 10]                                                     # 20 pairs
    imp = [5, 10, 30, 40, 10, 4, 1, 0]                                                  # 100 pairs
    ids = ["a", "b", "c", "d", "e"]
    return ScoreDistribution(ids, [gen, imp], [1, 0, 4, -1, 2], [0.5, 0.5, 0.75, 0, 0.75], [2, -1, 0, 4, 3], [0.25, 0, 0.25, -0.5, -0.5],
                             [5, 20, 100, 0])


def test_rates_on_a_hand_made_histogram():
    d = hand_made()
    assert np.array_equal(d.edges, np.linspace(-1, 1, 9)) and d.bins == 8
    assert (d.took_part, d.genuine_pairs, d.impostor_pairs, d.non_finite) == (5, 20, 100, 0)
    assert d.far(0.0) == 15 / 100 and d.frr(0.0) == 1 / 20
    assert d.far(0.25) == 5 / 100 and d.frr(0.25) == 2 / 20
    assert d.far(0.1) == d.far(0.25) and d.frr(0.1) == d.frr(0.25)                      # the edge at or ABOVE the argument
    assert d.far(-1.0) == 1.0 and d.far(-7.0) == 1.0 and d.far(1.0) == 0.0 and d.far(3.0) == 0.0 and d.frr(3.0) == 1.0
    assert d.threshold_at_far(0.05) == (0.25, 0.05, 0.1)
    assert d.threshold_at_far(0.049) == (0.5, 0.01, 0.2)
    assert d.threshold_at_far(0.0) == (0.75, 0.0, 0.5)
    assert d.threshold_at_far(1.0) == (-1.0, 1.0, 0.0)
    # |far - frr| per edge: 1, .95, .85, .55, .10, .05, .19, .5, 1 -> the edge 0.25
    assert d.eer() == (0.25, 0.05, 0.1)


def test_eer_takes_the_lowest_edge_among_equals():
    from scrfd_arcface_facerecognition_amd.engine import ScoreDistribution
    d = ScoreDistribution([], [[0, 0, 2, 2], [2, 2, 0, 0]], [], [], [], [], [0, 4, 4, 0])
    # far: 1, .5, 0, 0, 0   frr: 0, 0, 0, .5, 1  -> the gap is 0 at edge 2 only
    assert d.eer() == (0.0, 0.0, 0.0)
    d = ScoreDistribution([], [[0, 2, 0, 2], [2, 0, 2, 0]], [], [], [], [], [0, 4, 4, 0])
    # far: 1, .5, .5, 0, 0  frr: 0, 0, .5, .5, 1 -> gap 1, .5, 0, .5, 1
    assert d.eer() == (0.0, 0.5, 0.5)
    d = ScoreDistribution([], [[0, 0, 0, 4], [4, 0, 0, 0]], [], [], [], [], [0, 4, 4, 0])
    # far: 1, 0, 0, 0, 0    frr: 0, 0, 0, 0, 1 -> gap 0 at edges 1, 2, 3: the lowest
    assert d.eer() == (-0.5, 0.0, 0.0)


def test_rankings_and_their_ties():
    d = hand_made()
    assert d.hardest_impostors(2) == [("c", "e", 0.75), ("e", "c", 0.75)]               # equal scores: the lower id first
    assert d.hardest_impostors(10) == [("c", "e", 0.75), ("e", "c", 0.75), ("a", "b", 0.5), ("b", "a", 0.5)]
    assert d.weakest_genuines(3) == [("d", "e", -0.5), ("e", "d", -0.5), ("a", "c", 0.25)]
    assert d.weakest_genuines(0) == [] and len(d.weakest_genuines(99)) == 4


def test_an_empty_class_gives_nan_and_nothing_raises():
    from scrfd_arcface_facerecognition_amd.engine import ScoreDistribution
    d = ScoreDistribution([], np.zeros((2, 4), np.uint64), [], [], [], [], [0, 0, 0, 0])
    assert math.isnan(d.far(0.3)) and math.isnan(d.frr(0.3)) and all(math.isnan(v) for v in d.eer() + d.threshold_at_far(0.01))
    assert d.hardest_impostors(3) == [] and d.weakest_genuines(3) == []
    d = ScoreDistribution(["x", "y"], [[0, 0, 0, 1], [0, 0, 0, 0]], [-1, -1], [0, 0], [1, 0], [0.9, 0.9], [2, 1, 0, 0])
    assert math.isnan(d.far(0.0)) and d.frr(0.0) == 0.0 and d.frr(1.0) == 1.0 and math.isnan(d.eer()[0]) and math.isnan(d.threshold_at_far(0.1)[0])


def test_label_codes_number_persons_in_order_of_appearance():
    from scrfd_arcface_facerecognition_amd.engine import label_codes
    got = label_codes([3, 5, (1, 2), "k", 9], {3: "ann", 5: ("bob", 1), (1, 2): "ann", "k": None})
    assert got.dtype == np.int32 and got.tolist() == [0, 1, 0, -1, -1]
