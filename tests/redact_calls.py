"""How the redaction tests call the library: one case of redact_oracle.cases() through the host twins (no GPU) or the device entry points,
BGR or NV12.  A BGR batch is followed by NG guard bytes; an NV12 batch is one flat allocation whose every byte outside the layout is GUARD;
the comparisons run over everything."""
import ctypes as C

import numpy as np

from draw_calls import GUARD, NG, _arrays, _p
from draw_nv12_calls import desc_of


def c_style(s):
    from scrfd_arcface_facerecognition_amd._lib import RedactStyle
    return RedactStyle(s.mode, s.who, s.cells, s.expand, s.fill_bgr)


def _style_ref(style):
    """an oracle Style, a _lib.RedactStyle as it is, or None: the NULL pointer"""
    from scrfd_arcface_facerecognition_amd._lib import RedactStyle
    if style is None:
        return None
    return C.byref(style if isinstance(style, RedactStyle) else c_style(style))


def _ident(det, counts, idx, score, offsets):
    det, counts, idx, score, offsets, _ = _arrays(det, counts, idx, score, offsets, None)
    return det, counts, idx, score, offsets


def host_redact(lib, frames, cap, det, counts, idx=None, score=None, id_stride=0, offsets=None, n_rows=0, style=None):
    """-> (return code, the frames after fid_redact_faces_host); frames is not modified."""
    img = np.array(frames, dtype=np.uint8, copy=True)
    Bn, H, W = img.shape[:3]
    det, counts, idx, score, offsets = _ident(det, counts, idx, score, offsets)
    rc = lib.fid_redact_faces_host(_p(img), Bn, H, W, _p(det), _p(counts), cap, _p(idx), _p(score), id_stride, _p(offsets), n_rows, _style_ref(style))
    return rc, img


def host_redact_nv12(lib, buf, B, H, W, lay, standard, cap, det, counts, idx=None, score=None, id_stride=0, offsets=None, n_rows=0, style=None):
    """-> (return code, the allocation after fid_redact_faces_nv12_host); buf is not modified"""
    out = np.array(buf, dtype=np.uint8, copy=True)
    det, counts, idx, score, offsets = _ident(det, counts, idx, score, offsets)
    rc = lib.fid_redact_faces_nv12_host(_p(out), C.byref(desc_of(H, W, lay, standard)), B, H, W, _p(det), _p(counts), cap, _p(idx), _p(score),
                                        id_stride, _p(offsets), n_rows, _style_ref(style))
    return rc, out


def _upload(ctx, arrays):
    dev = [None if a is None else ctx.to_device(a) for a in arrays]
    return dev, [None if d is None else C.c_void_p(d.ptr) for d in dev]


def _inputs_unchanged(host, dev):
    for a, d in zip(host, dev):
        if a is not None:
            assert np.array_equal(d.download().view(np.uint8), a.view(np.uint8)), "an input array was written"


def device_redact(ctx, frames, cap, det, counts, idx=None, score=None, id_stride=0, offsets=None, n_rows=0, style=None, expect=0):
    """-> the frames after fid_redact_faces; asserts the return code, the NG guard bytes behind the frames and every input unchanged"""
    frames = np.ascontiguousarray(frames, np.uint8)
    Bn, H, W = frames.shape[:3]
    host = list(_ident(det, counts, idx, score, offsets))
    buf = ctx.to_device(np.concatenate([frames.reshape(-1), np.full(NG, GUARD, np.uint8)]))
    dev, ptr = _upload(ctx, host)
    rc = ctx.lib.fid_redact_faces(ctx.handle, C.c_void_p(buf.ptr), Bn, H, W, ptr[0], ptr[1], cap, ptr[2], ptr[3], id_stride, ptr[4], n_rows,
                                  _style_ref(style))
    assert rc == expect, (rc, expect)
    ctx.sync()
    raw = buf.download()
    assert (raw[frames.size:] == GUARD).all(), "guard bytes behind the frames were written"
    _inputs_unchanged(host, dev)
    return raw[:frames.size].reshape(frames.shape)


def device_redact_nv12(ctx, buf, B, H, W, lay, standard, cap, det, counts, idx=None, score=None, id_stride=0, offsets=None, n_rows=0, style=None,
                       expect=0):
    """-> the allocation after fid_redact_faces_nv12 (uploaded at exactly its size); asserts the return code and every input unchanged"""
    host = list(_ident(det, counts, idx, score, offsets))
    dev_buf = ctx.to_device(np.ascontiguousarray(buf, np.uint8))
    dev, ptr = _upload(ctx, host)
    rc = ctx.lib.fid_redact_faces_nv12(ctx.handle, C.c_void_p(dev_buf.ptr), C.byref(desc_of(H, W, lay, standard)), B, H, W, ptr[0], ptr[1], cap,
                                       ptr[2], ptr[3], id_stride, ptr[4], n_rows, _style_ref(style))
    assert rc == expect, (rc, expect)
    ctx.sync()
    got = dev_buf.download()
    _inputs_unchanged(host, dev)
    return got


def invalid_calls(style):
    """[(what, keyword overrides of a valid call, the style to pass)]: each must return FID_E_INVALID and leave the frames untouched.
    style: the valid call's (an oracle Style)"""
    def st(**kw):
        out = c_style(style)
        for k, v in kw.items():
            setattr(out, k, v)
        return out
    return [("a NULL style", {}, None), ("an unknown mode", {}, st(mode=2)), ("mode -1", {}, st(mode=-1)), ("who 0", {}, st(who=0)),
            ("who 4", {}, st(who=4)), ("cells 0", {}, st(cells=0)), ("cells 17", {}, st(cells=17)), ("expand NaN", {}, st(expand=float("nan"))),
            ("expand below 0", {}, st(expand=-0.01)), ("expand above 0.5", {}, st(expand=0.51)), ("reserved 1", {}, st(reserved=1)),
            ("idx without score", dict(score=None), st()), ("id_stride 0 in the slot form", dict(id_stride=0), st()),
            ("n_rows negative", dict(n_rows=-1), st()), ("cap 0", dict(cap=0), st())]
