"""How the drawing tests call the library: one case of draw_oracle.cases() through fid_draw_faces_host (no GPU) or fid_draw_faces."""
import ctypes as C

import numpy as np

GUARD = 0xA5
NG = 64                       # guard bytes behind the frames


def c_style(s):
    from scrfd_arcface_facerecognition_amd._lib import DrawStyle
    return DrawStyle(s.proportion, s.thickness, s.text_scale, s.bar, s.flags, s.unknown_bgr)


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _arrays(det, counts, idx, score, offsets, track):
    f32 = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
    i32 = lambda a: None if a is None else np.ascontiguousarray(a, np.int32)
    return f32(det), i32(counts), i32(idx), f32(score), i32(offsets), i32(track)


def host_draw(lib, frames, cap, det, counts, idx=None, score=None, id_stride=0, offsets=None, n_rows=0, track=None, names=None, bgr=None,
              style=None):
    """-> (return code, the image after the call); frames is not modified"""
    from scrfd_arcface_facerecognition_amd._lib import label_arrays
    img = np.array(frames, dtype=np.uint8, copy=True)
    Bn, H, W = img.shape[:3]
    det, counts, idx, score, offsets, track = _arrays(det, counts, idx, score, offsets, track)
    raw, name_off, colours = (None, None, None) if names is None else label_arrays(names, bgr)
    rc = lib.fid_draw_faces_host(_p(img), Bn, H, W, _p(det), _p(counts), cap, _p(idx), _p(score), id_stride, _p(offsets), n_rows, _p(track), raw,
                                 _p(name_off), _p(colours), 0 if names is None else len(names), C.byref(c_style(style)))
    return rc, img


def device_draw(ctx, frames, cap, det, counts, idx=None, score=None, id_stride=0, offsets=None, n_rows=0, track=None, names=None, bgr=None,
                style=None):
    """-> the frames after fid_draw_faces; asserts the NG guard bytes behind them and every input unchanged"""
    from scrfd_arcface_facerecognition_amd._lib import check
    from scrfd_arcface_facerecognition_amd.engine import LabelTable
    frames = np.ascontiguousarray(frames, np.uint8)
    Bn, H, W = frames.shape[:3]
    det, counts, idx, score, offsets, track = _arrays(det, counts, idx, score, offsets, track)
    buf = ctx.to_device(np.concatenate([frames.reshape(-1), np.full(NG, GUARD, np.uint8)]))
    host = [det, counts, idx, score, offsets, track]
    dev = [None if a is None else ctx.to_device(a) for a in host]
    ptr = [None if d is None else C.c_void_p(d.ptr) for d in dev]
    labels = LabelTable(ctx, names, bgr) if names is not None else None
    check(ctx.lib.fid_draw_faces(ctx.handle, C.c_void_p(buf.ptr), Bn, H, W, ptr[0], ptr[1], cap, ptr[2], ptr[3], id_stride, ptr[4], n_rows,
                                 ptr[5], labels.handle if labels else None, C.byref(c_style(style))))
    raw = buf.download()
    assert (raw[frames.size:] == GUARD).all(), "guard bytes behind the frames were written"
    for a, d in zip(host, dev):
        if a is not None:
            assert np.array_equal(d.download().view(np.uint8), a.view(np.uint8)), "an input array was written"
    if labels:
        labels.close()
    return raw[:frames.size].reshape(frames.shape)
