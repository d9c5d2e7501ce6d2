"""Float64 sampling references for the image front end (the 112x112 face warp, the letterbox resize, the exact-2x decimation), with the
envelopes inside which the fixed-point bytes must lie.  Test infrastructure only; numpy only.

These are written from the mathematics of bilinear sampling, not from oracle/align.py, and must not import it: the oracle and the kernels
restate the same paragraphs of SURVEY.md (A.1, A.3), so a convention misread once is in both.  What is stated here independently:

  * the warp samples the zero-extended image at  inverse(M) @ (u, v, 1),  pixel centres at integer coordinates;
  * the resize samples the edge-replicated image at  (d + 0.5) * (n / m) - 0.5,  pixel centres at integer coordinates;
  * the letterbox pastes the resized image top-left on zeros.

An envelope cannot tell the last bit of cv2; it catches every geometric or convention error larger than the quantisation.  No bound below
has a term that its docstring does not derive; SLACK covers float64 round-off only.
"""
import numpy as np

SLACK = 1e-6                      # float64 round-off of the references themselves (inverse, products): nothing else

WARP_D = 1.0 / 64 + 1.0 / 1024    # px per axis, derived in exact_warp
RESIZE_C = 1.0 / 4096 + 2.0 ** -13  # px per axis, derived in exact_resize
RESIZE_UP = 0.5                   # byte - exact, derived in exact_resize
RESIZE_DOWN = 0.75 + 1.0 / 128    # exact - byte, derived in exact_resize


def _zero_extended(image, pad):
    H, W = image.shape[:2]
    Z = np.zeros((H + 2 * pad, W + 2 * pad) + image.shape[2:], np.float64)
    Z[pad:pad + H, pad:pad + W] = image
    return Z


def exact_warp(image, M, size=112):
    """Bilinear sample, in float64, of the zero-extended image (BORDER_CONSTANT 0) at  inverse(M) @ (u, v, 1)  for every output pixel
    (u, v) of a size x size crop.  M is the 2x3 matrix that maps source to crop; it is inverted as a 3x3 matrix by np.linalg.inv.

    -> (exact, G), both float64 [size, size, C].  With (x0, y0) = floor of the sample's coordinate, G is the largest absolute horizontal
    difference plus the largest absolute vertical difference between adjacent pixels of the zero-extended image inside the 4x4 window
    x0-1..x0+2, y0-1..y0+2, per channel.

    Envelope of the fixed-point warp (1/1024 coordinate grid, 1/32-pixel table, 10-bit weights):

        |byte - exact| <= 0.5 + d * G,      d = 1/64 + 1/1024 px per axis.

      * The coordinate is the sum of a per-row term and a per-column term, each rounded to the nearest 1/1024 px (error <= 1/2048 each):
        the sum is off by at most 1/1024 px per axis.
      * `(... + 16) >> 5` rounds that sum to the nearest point of the 1/32 px grid: at most 1/64 px more per axis.
      * The 5-bit fractions then form the exact bilinear sample at that grid point (the four products of two 5-bit numbers are exact
        and sum to 1024), taps outside the image counting as 0: this is the zero-extended bilinear surface itself.
      * That surface is continuous, and inside a cell its slope along x (y) is at most the largest horizontal (vertical) difference
        of the cell's taps.  A coordinate moved by less than one pixel per axis stays in the 3x3 cells around the sample's, whose taps
        are the 4x4 window: the value moves by at most d * (largest horizontal) + d * (largest vertical) = d * G.
      * `(acc + 512) >> 10` is one round-to-nearest of the result: at most 0.5.

    Source coordinates must stay far below 32768 px (the table's short range); the callers' poses do."""
    image = np.asarray(image)
    H, W = image.shape[:2]
    M3 = np.vstack([np.asarray(M, np.float64).reshape(2, 3), [0.0, 0.0, 1.0]])
    Minv = np.linalg.inv(M3)
    v, u = np.meshgrid(np.arange(size, dtype=np.float64), np.arange(size, dtype=np.float64), indexing="ij")
    dst = np.stack([u, v, np.ones_like(u)], axis=-1)                  # [size, size, 3] = (u, v, 1)
    src = dst @ Minv.T
    xs, ys = src[..., 0], src[..., 1]
    # everything further than 3 px outside samples zeros from a window of zeros: clamp there, so that the padded image stays small
    P = 6
    xs = np.clip(xs, -3.0, W + 2.0)
    ys = np.clip(ys, -3.0, H + 2.0)
    x0 = np.floor(xs).astype(np.int64)
    y0 = np.floor(ys).astype(np.int64)
    fx = (xs - x0)[..., None]
    fy = (ys - y0)[..., None]
    Z = _zero_extended(image, P)                                      # Z[y + P, x + P] = image[y, x]
    X, Y = x0 + P, y0 + P
    exact = ((1 - fy) * ((1 - fx) * Z[Y, X] + fx * Z[Y, X + 1]) + fy * ((1 - fx) * Z[Y + 1, X] + fx * Z[Y + 1, X + 1]))
    dh = np.abs(Z[:, 1:] - Z[:, :-1])                                 # dh[y, x] = |Z[y, x+1] - Z[y, x]|
    dv = np.abs(Z[1:, :] - Z[:-1, :])
    gh = np.zeros_like(exact)
    gv = np.zeros_like(exact)
    for j in range(-1, 3):
        for i in range(-1, 2):
            gh = np.maximum(gh, dh[Y + j, X + i])                     # rows y0-1..y0+2, pairs (x0-1,x0) (x0,x0+1) (x0+1,x0+2)
            gv = np.maximum(gv, dv[Y + i, X + j])
    return exact, gh + gv


def warp_ratio(got, exact, G):
    """max over pixels of |byte - exact| / (0.5 + d * G + SLACK): inside the envelope iff <= 1"""
    return float((np.abs(np.asarray(got, np.float64) - exact) / (0.5 + WARP_D * G + SLACK)).max())


def _resize_axis(n, m):
    c = np.clip((np.arange(m, dtype=np.float64) + 0.5) * (n / m) - 0.5, 0.0, n - 1.0)
    s = np.minimum(np.floor(c).astype(np.int64), max(n - 2, 0))      # the cell [s, s+1]; its far end at the last pixel
    return s, np.minimum(s + 1, n - 1), c - s


def exact_resize(image, new_w, new_h):
    """Bilinear sample, in float64, of the image at source coordinate  (d + 0.5) * (n / m) - 0.5  per axis (n source, m output
    pixels), clamped to [0, n-1] (replicate border).  -> (exact, G), float64 [new_h, new_w, C]; G is the largest absolute horizontal
    plus the largest absolute vertical difference between the four taps of the sample's 2x2 cell.

    Envelope of the fixed-point resize (float32 coordinate, 11-bit weights a0 + a1 = b0 + b1 = 2048, T = S0*a0 + S1*a1,
    byte = (((b0*(T0>>4))>>16) + ((b1*(T1>>4))>>16) + 2) >> 2).  It is asymmetric, because the right shifts truncate:

        byte - exact <= 0.5 + c * G
        exact - byte <= 3/4 + 1/128 + c * G,      c = 1/4096 + 2^-13 px per axis.

      * The coordinate is rounded to float32; below 4096 px a float32 is within 2^-13 of the value.  The fraction is then rounded to
        the nearest 1/2048 (a1 = round(f * 2048), a0 = 2048 - a1: both roundings are of numbers that sum to 2048, halves going to the
        even side on each): at most 1/4096 more.  Rounded fraction and clamped cell stay inside the closed cell, where the bilinear
        surface has slopes of at most the horizontal / vertical tap differences: the value E that the integer weights represent,
        E = (b0*T0 + b1*T1) / 2^22, is within c * G of the exact sample.
      * Write U_k = T_k >> 4 = T_k/16 - e_k and V_k = (b_k*U_k) >> 16 = b_k*U_k/65536 - g_k with e_k, g_k in [0, 1).  Then
        S = V_0 + V_1 = 4E - delta,  delta = (b0*e0 + b1*e1)/65536 + g0 + g1  in [0, 2 + 1/32)  because b0 + b1 = 2048.
      * byte = floor((S + 2) / 4) <= S/4 + 1/2 <= E + 1/2: the upper side.
      * S is an integer, so floor((S + 2) / 4) >= (S + 2)/4 - 3/4 = E - delta/4 - 1/4 > E - (1/2 + 1/128) - 1/4: the lower side.
        (Counting the last shift as a loss of up to 1 instead of 3/4 gives the looser 1 + 1/128; the two `>> 4` floors cost 1/128
        together, not 1/64, since each is scaled by b_k/65536 and b0 + b1 = 2048.)
      * E lies in [0, 255], so the final saturation never acts.

    Shapes must stay below 4096 px per axis (the float32 term)."""
    image = np.asarray(image)
    H, W = image.shape[:2]
    assert max(H, W, new_h, new_w) < 4096
    img = image.astype(np.float64)
    sx, sx1, fx = _resize_axis(W, new_w)
    sy, sy1, fy = _resize_axis(H, new_h)
    p00, p01 = img[sy][:, sx], img[sy][:, sx1]
    p10, p11 = img[sy1][:, sx], img[sy1][:, sx1]
    fx = fx[None, :, None]
    fy = fy[:, None, None]
    exact = (1 - fy) * ((1 - fx) * p00 + fx * p01) + fy * ((1 - fx) * p10 + fx * p11)
    G = np.maximum(np.abs(p01 - p00), np.abs(p11 - p10)) + np.maximum(np.abs(p10 - p00), np.abs(p11 - p01))
    return exact, G


def resize_ratios(got, exact, G):
    """(max (byte - exact) / upper bound, max (exact - byte) / lower bound): inside the envelope iff both <= 1"""
    diff = np.asarray(got, np.float64) - exact
    cg = RESIZE_C * G + SLACK
    return float((diff / (RESIZE_UP + cg)).max()), float((-diff / (RESIZE_DOWN + cg)).max())


def exact_area2x(image):
    """Exact 2x decimation (both sides even): floor(mean of the 2x2 block + 0.5).  An equality, not an envelope."""
    v = np.asarray(image).astype(np.float64)
    mean = (v[0::2, 0::2] + v[0::2, 1::2] + v[1::2, 0::2] + v[1::2, 1::2]) / 4.0       # exact in float64
    return np.floor(mean + 0.5).astype(np.uint8)


def letterbox_geometry(H, W, in_h, in_w):
    """Aspect-preserving fit of an H x W image into in_h x in_w, in Python floats with int() truncation (reference
    models/scrfd.py:125-134).  -> (new_h, new_w, det_scale)"""
    im_ratio = float(H) / W
    model_ratio = float(in_h) / in_w
    if im_ratio > model_ratio:
        new_h = in_h
        new_w = int(new_h / im_ratio)
    else:
        new_w = in_w
        new_h = int(new_w * im_ratio)
    return new_h, new_w, float(new_h) / H


def letterbox_expect(image, in_h, in_w):
    """What the letterbox of `image` into in_h x in_w must be.  -> dict:
         new_h, new_w, det_scale   the geometry
         kind                      "identity" (same size: the image itself), "area2x" (exactly half on both axes: exact_area2x),
                                   else "linear" (exact_resize and its envelope)
         equal                     uint8 [new_h, new_w, C] for identity / area2x, else None
         exact, G                  exact_resize's pair for linear, else None
    Everything outside the top-left new_h x new_w is exactly zero: letterbox_check asserts it for every kind."""
    image = np.asarray(image)
    H, W = image.shape[:2]
    new_h, new_w, det_scale = letterbox_geometry(H, W, in_h, in_w)
    e = dict(new_h=new_h, new_w=new_w, det_scale=det_scale, equal=None, exact=None, G=None)
    if (new_h, new_w) == (H, W):
        e["kind"], e["equal"] = "identity", image.copy()
    elif H == 2 * new_h and W == 2 * new_w:
        e["kind"], e["equal"] = "area2x", exact_area2x(image)
    else:
        e["kind"] = "linear"
        e["exact"], e["G"] = exact_resize(image, new_w, new_h)
    return e


def letterbox_check(out, expect):
    """`out` uint8 [in_h, in_w, C] against letterbox_expect's dict.  -> (zero region is zero, upper ratio, lower ratio); the ratios are
    0.0 / 1e9 (equal / not) for the identity and the exact 2x.  Inside iff the first is True and both ratios <= 1."""
    out = np.asarray(out)
    nh, nw = expect["new_h"], expect["new_w"]
    zero = not out[nh:].any() and not out[:, nw:].any()
    if expect["equal"] is not None:
        r = 0.0 if np.array_equal(out[:nh, :nw], expect["equal"]) else 1e9
        return zero, r, r
    up, down = resize_ratios(out[:nh, :nw], expect["exact"], expect["G"])
    return zero, up, down


# ---- the shared inputs of tests/test_sampling_envelope_cpu.py and tests/test_gpu_sampling_envelope.py ------------------------------

FRAME_HW = (96, 128)
N_POSES = 60
# (H, W) -> (in_h, in_w): bilinear down and up, both kernels' widths, the identity, the exact 2x and the exact 3x (integer coordinates)
RESIZE_CASES = [((97, 33), (64, 96)), ((54, 96), (64, 96)), ((128, 192), (64, 96)), ((64, 96), (64, 96)), ((33, 97), (63, 95)),
                ((5, 7), (64, 64)), ((100, 150), (64, 96)), ((480, 853), (640, 640)), ((270, 480), (160, 160))]
TEMPLATE = np.array([[38.2946, 51.6963], [73.5318, 51.5014], [56.0252, 71.7366], [41.5493, 92.3655], [70.7299, 92.2041]], np.float64)


def ramp_image(H, W):
    """three channels, a different slope each (2 to 7 levels per pixel in all), clipped to 0..255: a position error of e px moves a
    byte by slope * e.  Channel 0 rises along x over the whole of a 128 px row, channel 1 along y, channel 2 steeply along both."""
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    ch = [2.0 * x, 2.5 * y, 5.0 * x + 2.0 * y - 150.0]
    return np.clip(np.rint(np.stack(ch, axis=-1)), 0, 255).astype(np.uint8)


def noise_image(H, W, seed=7):
    return np.random.default_rng([seed, H, W]).integers(0, 256, (H, W, 3), dtype=np.uint8)


def poses(n=N_POSES, hw=FRAME_HW, seed=3):
    """n landmark sets float32 [n, 5, 2], drawn as tests/test_gpu_align_match.py::test_warp_bit_exact_vs_oracle draws them but wider:
    scale 0.15 to 3, rotation over the full circle, centres up to 20 px outside the frame; the last set is mirrored (x flipped)."""
    rng = np.random.default_rng(seed)
    H, W = hw
    out = np.zeros((n, 5, 2), np.float32)
    for i in range(n):
        s = np.exp(rng.uniform(np.log(0.15), np.log(3.0)))
        th = rng.uniform(-np.pi, np.pi)
        R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        t = np.array([rng.uniform(-20, W + 20), rng.uniform(-20, H + 20)])
        t5 = TEMPLATE - 56.0
        if i == n - 1:
            t5 = t5 * np.array([-1.0, 1.0])
        out[i] = (t5 @ R.T * s + t + rng.normal(0, 1.0, (5, 2))).astype(np.float32)
    return out


def rank1_sets():
    """landmark sets of rank 1 (every rank >= 1 case the closed form claims): horizontal, vertical and diagonal collinear sets and
    three points at A, two at B.  float32 [4, 5, 2], inside a 96x128 frame."""
    t = np.array([0.0, 1.0, 2.5, 3.0, 4.5])
    return np.stack([
        np.stack([30.0 + 12.0 * t, np.full(5, 40.0)], axis=1),
        np.stack([np.full(5, 64.0), 20.0 + 11.0 * t], axis=1),
        np.stack([20.0 + 10.0 * t, 15.0 + 7.0 * t], axis=1),
        np.array([[40.0, 30.0]] * 3 + [[90.0, 70.0]] * 2),
    ]).astype(np.float32)
