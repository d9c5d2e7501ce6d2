"""The oracle's warp and resize against float64 sampling (tests/sampling_reference.py), without a GPU.

 a. oracle/align.py stays inside the derived envelopes on a ramp and a noise image, 60 poses and nine resize shapes;
 b. the envelopes have teeth: twelve deliberately wrong variants (half-pixel centre, inverse, axes, border, scale ...) leave them;
 c. the closed-form 2-D Umeyama estimate the kernel evaluates equals the oracle's SVD form at every rank >= 1.

tests/test_gpu_sampling_envelope.py runs the same inputs through the HIP kernels."""
import numpy as np
import pytest

import sampling_reference as sr
from conftest import load_golden
from oracle import align


@pytest.fixture(scope="module")
def frames():
    H, W = sr.FRAME_HW
    return {"ramp": sr.ramp_image(H, W), "noise": sr.noise_image(H, W)}


@pytest.fixture(scope="module")
def pose_M():
    """the 60 poses as the 2x3 matrices the pipeline would warp with (the oracle's fp64 estimate)"""
    return [align.estimate_norm(lm, f64=True)[0] for lm in sr.poses()]


@pytest.fixture(scope="module")
def ramp_exact(frames, pose_M):
    return [sr.exact_warp(frames["ramp"], M) for M in pose_M]


# ---- a. the oracle is inside ---------------------------------------------------------------------------------------------------

def test_ramp_has_the_slopes_it_promises(frames):
    r = frames["ramp"].astype(np.int64)
    dx, dy = np.abs(np.diff(r, axis=1)), np.abs(np.diff(r, axis=0))
    assert dx[..., 0].max() == 2 and dy[..., 1].max() == 3 and dx[..., 2].max() == 5 and dy[..., 2].max() == 2
    assert len({int(dx[..., 0].max()), int(dy[..., 1].max()), int(dx[..., 2].max() + dy[..., 2].max())}) == 3       # 2, 3 and 7 levels/px
    assert (r[..., 0] < 255).all() and (r[..., 1] < 255).all()                                                       # never clipped: every pixel shows its position
    unclipped = (r[..., 2] > 0) & (r[..., 2] < 255)
    assert unclipped.mean() > 0.25


@pytest.mark.parametrize("name", ["ramp", "noise"])
def test_oracle_warp_inside_envelope(frames, pose_M, name):
    assert len(pose_M) >= 60
    worst, inside_frame = 0.0, 0
    for i, M in enumerate(pose_M):
        exact, G = sr.exact_warp(frames[name], M)
        got = align.warp_affine(frames[name], M)
        r = sr.warp_ratio(got, exact, G)
        worst = max(worst, r)
        inside_frame += int(got.any())
        assert r <= 1.0, (name, i, r)
    assert inside_frame >= 50                                      # the poses look at the image, not past it
    print(f"oracle warp, {name}: max |byte - exact| / bound = {worst:.4f}")


@pytest.mark.parametrize("hw, in_hw", sr.RESIZE_CASES)
@pytest.mark.parametrize("name", ["ramp", "noise"])
def test_oracle_letterbox_inside_envelope(hw, in_hw, name):
    image = sr.ramp_image(*hw) if name == "ramp" else sr.noise_image(*hw)
    e = sr.letterbox_expect(image, *in_hw)
    det, scale = align.letterbox(image, (in_hw[1], in_hw[0]))
    assert scale == e["det_scale"]
    zero, up, down = sr.letterbox_check(det, e)
    print(f"oracle letterbox {hw} -> {in_hw} ({e['kind']}, {e['new_h']}x{e['new_w']}), {name}: upper {up:.3f}, lower {down:.3f}")
    assert zero and up <= 1.0 and down <= 1.0, (hw, in_hw, name, zero, up, down)


def test_resize_cases_cover_every_path():
    kinds = [sr.letterbox_expect(np.zeros(hw + (3,), np.uint8), *in_hw)["kind"] for hw, in_hw in sr.RESIZE_CASES]
    assert "identity" in kinds and "area2x" in kinds and kinds.count("linear") >= 6
    e = sr.letterbox_expect(np.zeros((270, 480, 3), np.uint8), 160, 160)
    assert (e["new_h"], e["new_w"]) == (90, 160)                   # the exact-3x case: integer source coordinates, weights 0 / 2048
    assert {in_hw[1] % 4 for _, in_hw in sr.RESIZE_CASES} == {0, 3}  # both kernels' widths


# ---- b. the envelope has teeth -------------------------------------------------------------------------------------------------

def _shift_source(M, s):
    """M' with  inverse(M')(p) = inverse(M)(p) + s:  the warp samples s px further along in the source"""
    M = np.array(M, np.float64)
    M[:, 2] -= M[:, :2] @ np.asarray(s, np.float64)
    return M


def _inverse(M):
    return np.linalg.inv(np.vstack([M, [0, 0, 1]]))[:2]


def _transposed(M):
    M = np.array(M, np.float64)
    M[0, 1], M[1, 0] = M[1, 0], M[0, 1]
    return M


def _replicated(image, M, pad=64):
    """BORDER_REPLICATE for `pad` px around the image"""
    return align.warp_affine(np.pad(image, ((pad, pad), (pad, pad), (0, 0)), mode="edge"), _shift_source(M, (-pad, -pad)))


WARP_VARIANTS = {
    "source shifted by half a pixel": lambda im, M: align.warp_affine(im, _shift_source(M, (0.5, 0.5))),
    "source shifted by 1/16 px in x": lambda im, M: align.warp_affine(im, _shift_source(M, (1.0 / 16, 0.0))),
    "M applied without inversion": lambda im, M: align.warp_affine(im, _inverse(M)),
    "rotation transposed": lambda im, M: align.warp_affine(im, _transposed(M)),
    "x and y swapped": lambda im, M: align.warp_affine(np.ascontiguousarray(im.transpose(1, 0, 2)), M),
    "channels reversed": lambda im, M: align.warp_affine(im, M)[..., ::-1],
    "border replicated": _replicated,
}


def test_shift_helper_shifts(frames, pose_M):
    """the helper the variants are built with: a whole-pixel shift of the source is the shifted image"""
    im = np.zeros_like(frames["noise"])
    im[4:-4, 4:-4] = frames["noise"][4:-4, 4:-4]                   # a zero rim: rolling wraps zeros only
    moved = np.roll(im, (-2, -1), axis=(0, 1))                     # moved[y, x] = im[y + 2, x + 1]
    for M in pose_M[:6]:
        a, b = sr.exact_warp(im, _shift_source(M, (1.0, 2.0)))[0], sr.exact_warp(moved, M)[0]
        assert np.abs(a - b).max() < 1e-6 and a.max() > 0


@pytest.mark.parametrize("variant", list(WARP_VARIANTS))
def test_wrong_warp_leaves_the_envelope(frames, pose_M, ramp_exact, variant):
    ratios = [sr.warp_ratio(WARP_VARIANTS[variant](frames["ramp"], M), exact, G) for M, (exact, G) in zip(pose_M, ramp_exact)]
    print(f"warp variant '{variant}': max ratio {max(ratios):.2f}, outside at {sum(r > 1 for r in ratios)} of {len(ratios)} poses")
    assert max(ratios) > 1.0, variant


def _float_resize(image, new_w, new_h, coord_x, coord_y, nearest=False):
    """A resize with pluggable source coordinates, float64 and rounded to nearest: with the right coordinates it is inside the envelope
    (test_float_resize_with_the_right_coordinates_is_inside), so whatever a variant changes is what takes it outside."""
    H, W = image.shape[:2]
    img = image.astype(np.float64)

    def axis(coord, n, m):
        c = np.clip(coord(np.arange(m, dtype=np.float64), n, m), 0.0, n - 1.0)
        if nearest:
            c = np.floor(c + 0.5)
        s = np.minimum(np.floor(c).astype(np.int64), max(n - 2, 0))
        return s, np.minimum(s + 1, n - 1), c - s
    sx, sx1, fx = axis(coord_x, W, new_w)
    sy, sy1, fy = axis(coord_y, H, new_h)
    fx, fy = fx[None, :, None], fy[:, None, None]
    v = (1 - fy) * ((1 - fx) * img[sy][:, sx] + fx * img[sy][:, sx1]) + fy * ((1 - fx) * img[sy1][:, sx] + fx * img[sy1][:, sx1])
    return np.clip(np.floor(v + 0.5), 0, 255).astype(np.uint8)


def _right(d, n, m):
    return (d + 0.5) * (n / m) - 0.5


def _letterboxed(resized, in_h, in_w, centred=False):
    det = np.zeros((in_h, in_w, 3), np.uint8)
    h, w = resized.shape[:2]
    y0, x0 = ((in_h - h) // 2, (in_w - w) // 2) if centred else (0, 0)
    det[y0:y0 + h, x0:x0 + w] = resized
    return det


RESIZE_VARIANTS = {
    "no half-pixel centre": lambda im, w, h: _float_resize(im, w, h, lambda d, n, m: d * (n / m), lambda d, n, m: d * (n / m)),
    "align-corners scale": lambda im, w, h: _float_resize(im, w, h, lambda d, n, m: d * ((n - 1) / (m - 1)), lambda d, n, m: d * ((n - 1) / (m - 1))),
    "nearest neighbour": lambda im, w, h: _float_resize(im, w, h, _right, _right, nearest=True),
    "scale_x used for both axes": lambda im, w, h: _float_resize(im, w, h, _right, lambda d, n, m: (d + 0.5) * (im.shape[1] / w) - 0.5),
}
# shapes whose scale is far from 1: at 97/95 (the (33, 97) case above) a missing half-pixel centre moves the sample by 0.01 px, below any quantisation
TEETH_SHAPES = [((97, 33), (64, 96)), ((100, 150), (64, 96)), ((60, 200), (63, 95))]


@pytest.mark.parametrize("hw, in_hw", TEETH_SHAPES)
def test_float_resize_with_the_right_coordinates_is_inside(hw, in_hw):
    image = sr.ramp_image(*hw)
    e = sr.letterbox_expect(image, *in_hw)
    zero, up, down = sr.letterbox_check(_letterboxed(_float_resize(image, e["new_w"], e["new_h"], _right, _right), *in_hw), e)
    assert zero and up <= 1.0 and down <= 1.0


@pytest.mark.parametrize("variant", list(RESIZE_VARIANTS))
def test_wrong_resize_leaves_the_envelope(variant):
    shapes = TEETH_SHAPES[:1] if variant == "scale_x used for both axes" else TEETH_SHAPES
    for hw, in_hw in shapes:
        image = sr.ramp_image(*hw)
        e = sr.letterbox_expect(image, *in_hw)
        assert e["kind"] == "linear"
        zero, up, down = sr.letterbox_check(_letterboxed(RESIZE_VARIANTS[variant](image, e["new_w"], e["new_h"]), *in_hw), e)
        print(f"resize variant '{variant}' {hw} -> {in_hw}: upper {up:.2f}, lower {down:.2f}")
        assert max(up, down) > 1.0, (variant, hw)


@pytest.mark.parametrize("hw, in_hw, kind", [((97, 33), (64, 96), "linear"), ((60, 200), (63, 95), "linear"), ((128, 100), (64, 96), "area2x"),
                                             ((54, 96), (64, 96), "identity")])          # shapes that leave a margin to centre in
def test_centred_paste_leaves_the_envelope(hw, in_hw, kind):
    image = sr.ramp_image(*hw)
    e = sr.letterbox_expect(image, *in_hw)
    assert e["kind"] == kind
    det, _ = align.letterbox(image, (in_hw[1], in_hw[0]))
    centred = _letterboxed(det[:e["new_h"], :e["new_w"]], *in_hw, centred=True)
    zero, up, down = sr.letterbox_check(centred, e)
    assert not zero, hw


# ---- c. closed form == SVD at every rank >= 1 ----------------------------------------------------------------------------------

def closed_form(lm):
    """csrc/align.hip's estimate, in numpy: fp64 from the fp32 landmarks and the fp32 template, no SVD"""
    src = np.asarray(lm, np.float32).astype(np.float64)
    dst = align.REFERENCE_ALIGNMENT[0].astype(np.float64)
    ms, md = src.mean(axis=0), dst.mean(axis=0)
    p, q = src - ms, dst - md
    a = (q[:, 0] * p[:, 0] + q[:, 1] * p[:, 1]).sum()
    b = (q[:, 1] * p[:, 0] - q[:, 0] * p[:, 1]).sum()
    var = (p * p).sum()
    with np.errstate(invalid="ignore", divide="ignore"):
        R = np.array([[a, -b], [b, a]]) / var
    return np.hstack([R, (md - R @ ms)[:, None]])


def rel_diff(M, ref):
    return np.abs(M - ref).max() / max(1.0, np.abs(ref).max())


def mirrored_template():
    t = align.REFERENCE_ALIGNMENT[0].astype(np.float64).copy()
    t[:, 0] = 112.0 - t[:, 0]
    return t.astype(np.float32)


def test_closed_form_equals_svd_on_rank1_and_mirrored_sets():
    sets = list(sr.rank1_sets()) + [mirrored_template()]
    for i, lm in enumerate(sets):
        d = lm.astype(np.float64) - lm.astype(np.float64).mean(axis=0)
        A = (align.REFERENCE_ALIGNMENT[0].astype(np.float64) - align.REFERENCE_ALIGNMENT[0].astype(np.float64).mean(axis=0)).T @ d / 5
        if i < 4:
            assert np.linalg.matrix_rank(A) == 1, i                # the sets are what they claim to be
        else:
            assert np.linalg.det(A) < 0                            # a reflection: the SVD form takes its d = [1, -1] branch
        ref, _ = align.estimate_norm(lm, f64=True)
        assert np.isfinite(ref).all()
        assert rel_diff(closed_form(lm), ref) < 1e-9, i


def test_closed_form_equals_svd_on_the_goldens():
    lms = load_golden("umeyama.npz")["landmarks"]
    assert len(lms) == 129
    for i, lm in enumerate(lms):
        ref, _ = align.estimate_norm(lm, f64=True)
        assert rel_diff(closed_form(lm), ref) < 1e-9, i


def test_five_identical_points_admit_no_transform():
    lm = np.tile(np.float32([[50.0, 40.0]]), (5, 1))
    ref, _ = align.estimate_norm(lm, f64=True)
    assert not np.isfinite(ref).any() and not np.isfinite(closed_form(lm)).any()
