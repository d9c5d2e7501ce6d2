#!/usr/bin/env python3
"""The overlay (fid_draw_faces) timed for docs/FINDINGS.md, on the bench workload's shape: 64 frames of 640 x 640, a seeded table of 14 faces
per frame (boxes 40 .. 160 pixels wide anywhere in the frame, every second one known), cap = 256, slots form with id_stride = 14.
Per variant -- with text (the default style) and without (text_scale 0) -- 5 warm-up calls, then 7 repeats of 200 calls between two HIP events
(fid_event_*); the median repeat, per call.  Beside them fid_memset over the same frames' bytes, the same way: the cost of writing every pixel
once, the yardstick of an in-place overlay.  Also the share of the pixels the overlay writes.  Needs nothing outside the repository.
bench_draw.py [--batch 64] [--size 640] [--faces 14] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARM, REPS, CALLS = 5, 7, 200


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--faces", type=int, default=14)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from scrfd_arcface_facerecognition_amd._lib import Context, DrawStyle, check
    from scrfd_arcface_facerecognition_amd.engine import LabelTable

    ctx = Context(0)
    B, HW, F, cap, G = args.batch, args.size, args.faces, 256, 1000
    rng = np.random.default_rng(2024)
    frames = rng.integers(0, 256, (B, HW, HW, 3), dtype=np.uint8)
    det = np.zeros((B, cap, 5), np.float32)
    w = rng.uniform(40, 160, (B, F))
    x1, y1 = rng.uniform(0, HW - 40, (B, F)), rng.uniform(0, HW - 40, (B, F))
    det[:, :F, 0], det[:, :F, 1], det[:, :F, 2], det[:, :F, 3], det[:, :F, 4] = x1, y1, x1 + w, y1 + w * rng.uniform(1.0, 1.4, (B, F)), 0.9
    idx = np.where(np.arange(F)[None, :] % 2 == 0, rng.integers(0, G, (B, F)), -1).astype(np.int32)
    score = rng.uniform(0.3, 0.9, (B, F)).astype(np.float32)
    d_frames, d_det, d_counts = ctx.to_device(frames), ctx.to_device(det), ctx.to_device(np.full(B, F, np.int32))
    d_idx, d_score = ctx.to_device(idx), ctx.to_device(score)
    labels = LabelTable(ctx, [f"person_{g:04d}" for g in range(G)])

    def draw(style):
        check(ctx.lib.fid_draw_faces(ctx.handle, C.c_void_p(d_frames.ptr), B, HW, HW, C.c_void_p(d_det.ptr), C.c_void_p(d_counts.ptr), cap,
                                     C.c_void_p(d_idx.ptr), C.c_void_p(d_score.ptr), F, None, 0, None, labels.handle, C.byref(style)))

    def memset():
        check(ctx.lib.fid_memset(ctx.handle, C.c_void_p(d_frames.ptr), 0, frames.nbytes))

    def timed(fn):
        for _ in range(WARM):
            fn()
        ctx.sync()
        ms = []
        for _ in range(REPS):
            ctx.event_record(0)
            for _ in range(CALLS):
                fn()
            ctx.event_record(1)
            ms.append(ctx.elapsed_ms(0, 1) / CALLS)
        return statistics.median(ms), min(ms), max(ms)

    out = dict(device=ctx.name(), batch=B, size=HW, faces_per_frame=F, cap=cap, frame_bytes=int(frames.nbytes))
    for key, style in (("text", DrawStyle()), ("no_text", DrawStyle(text_scale=0))):
        d_frames.upload(frames)
        draw(style)
        share = float((d_frames.download() != frames).any(axis=3).mean())
        med, lo, hi = timed(lambda: draw(style))
        out[key] = dict(ms_per_call=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4), pixels_changed_share=round(share, 5))
    med, lo, hi = timed(memset)
    out["memset"] = dict(ms_per_call=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4))
    labels.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
