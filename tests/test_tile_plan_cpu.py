"""CPU: the tile planner of tiled detection (pipeline.tile_plan) and the numpy restatement of the merge (tests/tile_oracle.py)."""
import numpy as np
import pytest

from oracle import postprocess as pp
from scrfd_arcface_facerecognition_amd.pipeline import tile_origins, tile_plan
from tile_oracle import merge_tiles, random_heads

AXES = (1920, 1080, 700, 203, 150, 129, 65)
INPUTS = ((640, 128, 8), (320, 64, 8), (64, 16, 2), (640, 128, 0), (64, 16, 0), (64, 5, 2))     # (input length, overlap, margin)


def test_examples_of_the_rule():
    assert [o for o, _ in tile_origins(1920, 640, 128)] == [0, 512, 1024, 1280]
    assert [o for o, _ in tile_origins(1080, 640, 128)] == [0, 440]
    p = tile_plan(1080, 1920, (640, 640))
    assert p.dtype == np.int32 and p.shape == (9, 6)
    assert p[:8].tolist() == [[0, x, y, 640, 640, 0] for y in (0, 440) for x in (0, 512, 1024, 1280)]      # y-major
    assert p[8].tolist() == [0, 0, 0, 1920, 1080, 1]
    assert tile_plan(2160, 3840, (640, 640)).shape == (33, 6)
    assert len(tile_origins(3840, 640, 128)) == 8 and len(tile_origins(2160, 640, 128)) == 4
    assert tile_plan(1080, 1920, (640, 640), overview=False).shape == (8, 6)
    b = tile_plan(1080, 1920, (640, 640), batch=3)
    assert b.shape == (27, 6) and b[:, 0].tolist() == [0] * 9 + [1] * 9 + [2] * 9
    assert np.array_equal(b[9:18, 1:], p[:, 1:]) and np.array_equal(b[18:, 1:], p[:, 1:])


@pytest.mark.parametrize("n, overlap, margin", INPUTS)
def test_tiles_stay_inside_and_the_last_is_flush(n, overlap, margin):
    for L in AXES:
        t = tile_origins(L, n, overlap)
        assert t[0][0] == 0 and all(o >= 0 and e > 0 and o + e <= L and e <= n for o, e in t), (L, t)
        assert t[-1][0] + t[-1][1] == L, (L, t)
        assert [o for o, _ in t] == sorted({o for o, _ in t}), (L, t)
        if L <= n:
            assert t == [(0, L)]


def test_frame_that_fits_gets_one_overview_row():
    for H, W in ((640, 640), (40, 203 - 150), (64, 10), (1, 1)):
        for overview in (True, False):
            assert tile_plan(H, W, (640, 640), overview=overview, batch=2).tolist() == [[0, 0, 0, W, H, 1], [1, 0, 0, W, H, 1]]
    # narrower than the input on one axis only: native tiles of the frame's own extent there
    p = tile_plan(40, 203, (64, 64), overlap=16)
    assert p.tolist() == [[0, x, 0, 64, 40, 0] for x in (0, 48, 96, 139)] + [[0, 0, 0, 203, 40, 1]]


def test_bad_overlap_is_refused():
    with pytest.raises(ValueError):
        tile_plan(1080, 1920, (640, 640), overlap=640)
    with pytest.raises(ValueError):
        tile_plan(1080, 1920, (640, 640), overlap=-1)


@pytest.mark.parametrize("n, overlap, margin", INPUTS)
def test_coverage_guarantee_brute_force(n, overlap, margin):
    """every interval of length s <= overlap - 2 * margin lies in some tile with `margin` to spare on each interior side.  An interval of
    length s' < s lies inside one of length s (when the axis has room for it), so the longest length is the whole test."""
    smax = overlap - 2 * margin
    assert smax >= 1
    for L in AXES:
        tiles = tile_origins(L, n, overlap)
        s = min(smax, L)
        for a in range(0, L - s + 1):
            ok = any((o == 0 or a >= o + margin) and (o + e == L or a + s <= o + e - margin) for o, e in tiles)
            assert ok, (L, n, a, s)
        # the bound is tight to a pixel: integer intervals of overlap - 2 * margin + 1 still fit, two more than promised do not
        if len(tiles) > 1 and tiles[1][0] == n - overlap and tiles[1][0] + margin - 1 + smax + 2 <= L:
            a, s2 = tiles[1][0] + margin - 1, smax + 2
            assert not any((o == 0 or a >= o + margin) and (o + e == L or a + s2 <= o + e - margin) for o, e in tiles)


def _frames_heads(seed, counts):
    rng = np.random.default_rng(seed)
    return [random_heads(rng, K) for K in counts]


@pytest.mark.parametrize("max_num, metric", [(0, "max"), (2, "max"), (5, "default")])
def test_overview_only_plan_is_detect_from_heads(max_num, metric):
    heads = _frames_heads(21, [40, 0, 168])
    img_hw = (150, 203)
    tiles = np.array([[b, 0, 0, img_hw[1], img_hw[0], 1] for b in range(3)], np.int32)            # one overview row per frame
    got = merge_tiles(heads, tiles, img_hw, (64, 64), 0.5, 0.4, edge_margin=2, max_num=max_num, metric=metric)
    for b in range(3):
        det, kps = pp.detect_from_heads(heads[b], img_hw, (64, 64), 0.5, 0.4, max_num, metric)
        assert np.array_equal(got[b][0], det) and np.array_equal(got[b][1], kps), b
    assert len(got[0][0]) > 0 and len(got[1][0]) == 0


def test_one_native_tile_is_the_shifted_single_image():
    heads = _frames_heads(22, [60])
    x0, y0 = 139, 86
    tiles = np.array([[0, x0, y0, 64, 64, 0]], np.int32)
    (det, kps), = merge_tiles(heads, tiles, (150, 203), (64, 64), 0.5, 0.4, edge_margin=-1)
    odet, okps = pp.detect_from_heads(heads[0], (64, 64), (64, 64), 0.5, 0.4)
    assert len(odet) > 3
    assert np.array_equal(det, odet + np.array([x0, y0, x0, y0, 0], np.float32))
    assert np.array_equal(kps, okps + np.array([x0, y0], np.float32))


def test_edge_rule_only_rejects_at_cuts():
    """a tile in the frame's corner rejects on its two interior sides only; margin -1 rejects nothing"""
    heads = _frames_heads(23, [168])
    from tile_oracle import tile_candidates
    row = np.array([0, 0, 0, 64, 64, 0], np.int32)
    all_s, all_b, _ = tile_candidates(heads[0], row, (150, 203), (64, 64), 0.5, -1)
    s, b, _ = tile_candidates(heads[0], row, (150, 203), (64, 64), 0.5, 2)
    assert len(all_s) == 168 and 0 < len(s) < 168
    keep = (all_b[:, 2] <= 62) & (all_b[:, 3] <= 62)
    assert np.array_equal(b, all_b[keep])
    assert (all_b[keep][:, 0] < 2).any()                       # touching the frame's boundary is no reason to drop
