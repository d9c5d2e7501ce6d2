"""NV12 -> BGR restated in numpy from include/faceid.h (fid_nv12_to_bgr), not from csrc/yuv_core.h: int64 arithmetic, the three standards,
pitch, uv_offset and frame_stride.  Also the helpers the NV12 tests share: a random pitched batch with a chosen fill in every byte the
library promises never to read."""
import math

import numpy as np

# standard -> (the five coefficients, Y offset); the integers are floor(c * 2^20 + 0.5) of them
COEFFS = {
    "bt601": ((1.164, 2.018, -0.391, -0.813, 1.596), 16),
    "bt709": ((1.164, 2.112, -0.213, -0.533, 1.793), 16),
    "bt601_full": ((1.0, 1.772, -0.344136, -0.714136, 1.402), 0),
}
STANDARD_ID = {"bt601": 0, "bt709": 1, "bt601_full": 2}
SHIFT = 20


def table(standard):
    """(CY, CUB, CUG, CVG, CVR, Y offset) as integers"""
    cs, y0 = COEFFS[standard]
    return tuple(int(math.floor(c * (1 << SHIFT) + 0.5)) for c in cs) + (y0,)


def yuv_to_bgr(Y, U, V, standard="bt601"):
    """arrays of samples (any shape, broadcast together) -> uint8 [..., 3] BGR"""
    cy, cub, cug, cvg, cvr, y0 = table(standard)
    Y, U, V = (np.asarray(a).astype(np.int64) for a in (Y, U, V))
    yy = np.maximum(0, Y - y0) * cy
    u, v = U - 128, V - 128
    half = 1 << (SHIFT - 1)
    b = (yy + cub * u + half) >> SHIFT                      # (numpy's >> on int64 is the arithmetic shift)
    g = (yy + cug * u + cvg * v + half) >> SHIFT
    r = (yy + cvr * v + half) >> SHIFT
    return np.clip(np.stack(np.broadcast_arrays(b, g, r), axis=-1), 0, 255).astype(np.uint8)


def dense_layout(H, W):
    return dict(pitch=W, uv_offset=W * H, frame_stride=W * H * 3 // 2)


def nv12_to_bgr(buf, B, H, W, pitch=None, uv_offset=None, frame_stride=None, standard="bt601"):
    """buf: uint8 1-D (the allocation) -> uint8 [B,H,W,3]; chroma replicated: pixel (y, x) takes the pair at UV[y>>1][(x>>1)*2]"""
    d = dense_layout(H, W)
    pitch = d["pitch"] if pitch is None else pitch
    uv_offset = pitch * H if uv_offset is None else uv_offset
    frame_stride = uv_offset + pitch * (H // 2) if frame_stride is None else frame_stride
    buf = np.asarray(buf, np.uint8).reshape(-1)
    ys, xs = np.arange(H)[:, None], np.arange(W)[None, :]
    out = np.empty((B, H, W, 3), np.uint8)
    for b in range(B):
        f = b * frame_stride
        Y = buf[f + ys * pitch + xs]
        c = f + uv_offset + (ys >> 1) * pitch + (xs >> 1) * 2
        out[b] = yuv_to_bgr(Y, buf[c], buf[c + 1], standard)
    return out


def needed_bytes(B, H, W, pitch, uv_offset, frame_stride):
    """the smallest allocation the layout may be given: it ends with the last UV row of the last frame (its first W bytes when pitch > W)"""
    return frame_stride * (B - 1) + uv_offset + pitch * (H // 2 - 1) + W


def random_batch(seed, B, H, W, pitch=None, uv_offset=None, frame_stride=None, fill=0xFF, exact_end=True):
    """-> (buf uint8 1-D, layout dict).  Every byte the library may read is random; every other byte of the allocation -- between W and
    pitch, between the planes, between the frames -- is `fill`.  exact_end: the allocation stops at uv_offset + pitch * H/2 of the last frame
    (what include/faceid.h calls the frame's end), else `frame_stride` bytes are kept for the last frame too."""
    pitch = W if pitch is None else pitch
    uv_offset = pitch * H if uv_offset is None else uv_offset
    frame_stride = uv_offset + pitch * (H // 2) if frame_stride is None else frame_stride
    n = frame_stride * (B - 1) + uv_offset + pitch * (H // 2) if exact_end else frame_stride * B
    buf = np.full(n, fill, np.uint8)
    rng = np.random.default_rng(seed)
    for b in range(B):
        f = b * frame_stride
        for y in range(H):
            buf[f + y * pitch:f + y * pitch + W] = rng.integers(0, 256, W, dtype=np.uint8)
        for y in range(H // 2):
            o = f + uv_offset + y * pitch
            buf[o:o + W] = rng.integers(0, 256, W, dtype=np.uint8)
    return buf, dict(pitch=pitch, uv_offset=uv_offset, frame_stride=frame_stride)
