"""How the NV12 drawing tests call the library: one case of draw_oracle.cases() through fid_draw_faces_nv12_host (no GPU) or
fid_draw_faces_nv12, and fid_bgr_to_nv12 / its host twin; the layouts the tests share.  A batch is one flat uint8 allocation; every byte a
layout does not own (between W and pitch, between the planes, behind a frame) is GUARD, and the comparisons run over the whole allocation."""
import ctypes as C

import numpy as np

import nv12_oracle
from draw_calls import _arrays, _p, c_style

GUARD = 0xA5
STANDARDS = ("bt601", "bt709", "bt601_full")


def layouts(H, W):
    """name -> layout: dense; every base and stride a multiple of 4 (the dword stores); pitch = W + 6 with a gap before the UV plane and a
    tail behind each frame, none a multiple of 4 (byte stores only)"""
    pa = (W + 3) // 4 * 4 + 8
    pu = W + 6
    return {"dense": dict(pitch=W, uv_offset=W * H, frame_stride=W * H * 3 // 2),
            "dwords": dict(pitch=pa, uv_offset=pa * (H + 2), frame_stride=pa * (H + 2) + pa * (H // 2) + 32),
            "w+6": dict(pitch=pu, uv_offset=pu * H + 10, frame_stride=pu * H + 10 + pu * (H // 2) + 7)}


def background(seed, B, H, W, lay, exact=False):
    """random frames in the layout, GUARD everywhere else; exact: the allocation ends with the last UV byte of the last frame"""
    buf, _ = nv12_oracle.random_batch(seed, B, H, W, fill=GUARD, **lay)
    return buf[:nv12_oracle.needed_bytes(B, H, W, **lay)].copy() if exact else buf


def desc_of(H, W, lay, standard):
    from scrfd_arcface_facerecognition_amd._lib import nv12_desc
    return nv12_desc(H, W, standard=standard, **lay)


def host_draw(lib, buf, B, H, W, lay, standard, cap, det, counts, idx=None, score=None, id_stride=0, offsets=None, n_rows=0, track=None, names=None,
              bgr=None, style=None):
    """-> (return code, the allocation after fid_draw_faces_nv12_host); buf is not modified"""
    from scrfd_arcface_facerecognition_amd._lib import label_arrays
    out = np.array(buf, dtype=np.uint8, copy=True)
    det, counts, idx, score, offsets, track = _arrays(det, counts, idx, score, offsets, track)
    raw, name_off, colours = (None, None, None) if names is None else label_arrays(names, bgr)
    rc = lib.fid_draw_faces_nv12_host(_p(out), C.byref(desc_of(H, W, lay, standard)), B, H, W, _p(det), _p(counts), cap, _p(idx), _p(score),
                                      id_stride, _p(offsets), n_rows, _p(track), raw, _p(name_off), _p(colours),
                                      0 if names is None else len(names), C.byref(c_style(style)))
    return rc, out


def device_draw(ctx, buf, B, H, W, lay, standard, cap, det, counts, idx=None, score=None, id_stride=0, offsets=None, n_rows=0, track=None,
                names=None, bgr=None, style=None):
    """-> the allocation after fid_draw_faces_nv12 (uploaded at exactly its size); asserts every input unchanged"""
    from scrfd_arcface_facerecognition_amd._lib import check
    from scrfd_arcface_facerecognition_amd.engine import LabelTable
    det, counts, idx, score, offsets, track = _arrays(det, counts, idx, score, offsets, track)
    dev_buf = ctx.to_device(np.ascontiguousarray(buf, np.uint8))
    host = [det, counts, idx, score, offsets, track]
    dev = [None if a is None else ctx.to_device(a) for a in host]
    ptr = [None if d is None else C.c_void_p(d.ptr) for d in dev]
    labels = LabelTable(ctx, names, bgr) if names is not None else None
    check(ctx.lib.fid_draw_faces_nv12(ctx.handle, C.c_void_p(dev_buf.ptr), C.byref(desc_of(H, W, lay, standard)), B, H, W, ptr[0], ptr[1], cap,
                                      ptr[2], ptr[3], id_stride, ptr[4], n_rows, ptr[5], labels.handle if labels else None,
                                      C.byref(c_style(style))))
    got = dev_buf.download()
    for a, d in zip(host, dev):
        if a is not None:
            assert np.array_equal(d.download().view(np.uint8), a.view(np.uint8)), "an input array was written"
    if labels:
        labels.close()
    return got
