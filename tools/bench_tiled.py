#!/usr/bin/env python3
"""Tiled against letterboxed detection on 1080p frames: ms per frame of the detect stage, split into its three parts.  Letterboxed: fid_letterbox,
the detector at batch B, fid_scrfd_postprocess.  Tiled: fid_tile_cut, the detector at batch 9 B (8 native 640x640 tiles at overlap 128 plus the
overview tile per frame), fid_scrfd_postprocess_tiled.  One process, the context's events around every part, the two paths taken in turn inside
every repeat (so drift hits them alike), one warm-up round (it also lets the executor pick its kernels for both batch sizes), the median of
--repeats timed rounds.  The detector's cls bias is calibrated on the frames' own tiles so that every input has a few dozen candidates, as a
trained detector would.  One JSON line.

    python tools/bench_tiled.py [--frames 4] [--repeats 7] [--arch scrfd_10g]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scrfd_arcface_facerecognition_amd import archs  # noqa: E402
from scrfd_arcface_facerecognition_amd._lib import Context, c_i32_p, check  # noqa: E402
from scrfd_arcface_facerecognition_amd.engine import CompiledNet, HeadViews, PostProcessor  # noqa: E402
from scrfd_arcface_facerecognition_amd.pipeline import calibrate_detector_bias, tile_plan  # noqa: E402

H, W, IN = 1080, 1920, (640, 640)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4, help="frames per step (the tiled path runs 9 detector inputs per frame)")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--arch", default="scrfd_10g", choices=["scrfd_500m", "scrfd_2_5g", "scrfd_10g"])
    ap.add_argument("--overlap", type=int, default=128)
    ap.add_argument("--edge-margin", type=int, default=8)
    args = ap.parse_args()
    assert args.repeats >= 5 and args.frames >= 1
    B = args.frames
    ctx = Context(0)
    lib, h = ctx.lib, ctx.handle
    rng = np.random.default_rng(0)
    frames = ctx.to_device(rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8))
    tiles = tile_plan(H, W, IN, args.overlap, True, B)
    T = len(tiles)
    assert T == 9 * B, tiles
    tile_buf, lb_buf = ctx.empty((T,) + IN + (3,), np.uint8), ctx.empty((B,) + IN + (3,), np.uint8)

    def cut():
        check(lib.fid_tile_cut(h, C.c_void_p(frames.ptr), B, H, W, tiles.ctypes.data_as(c_i32_p), T, C.c_void_p(tile_buf.ptr), IN[0], IN[1]))

    def letterbox():
        check(lib.fid_letterbox(h, C.c_void_p(frames.ptr), B, H, W, C.c_void_p(lb_buf.ptr), IN[0], IN[1], None))

    cut()
    net = archs.ARCHS[args.arch](IN)
    calib = tile_buf.download()[:9]                                   # frame 0's tiles: 8 native, 1 overview
    params, _ = calibrate_detector_bias(ctx, net, archs.synth_params(net, 0), calib, target=48, max_batch=9)
    det = CompiledNet(ctx, net, params, max_batch=T)
    hv = HeadViews.from_fused(det)
    post = PostProcessor(ctx, B, cap=1024)
    parts = {"letterboxed": (letterbox, lambda: det.run_device(lb_buf, B),
                             lambda: post.run(hv, B, IN, (H, W), 0.5, 0.4)),
             "tiled": (cut, lambda: det.run_device(tile_buf, T),
                       lambda: post.run_tiled(hv, tiles, B, IN, (H, W), 0.5, 0.4, args.edge_margin))}
    names = ("prepare", "detector", "postprocess")
    ms = {path: {n: [] for n in names} for path in parts}
    faces = {}
    for rep in range(args.repeats + 1):                               # round 0 warms up (kernel picks, scratch arenas, code objects)
        for path, calls in parts.items():
            ctx.event_record(0)
            for i, call in enumerate(calls):
                call()
                ctx.event_record(i + 1)
            for i, n in enumerate(names):
                t = ctx.elapsed_ms(i, i + 1)
                if rep:
                    ms[path][n].append(t)
            faces[path] = [len(d) for d, _ in post.fetch(B)]          # (also the capacity check)
    med = {path: {n: statistics.median(v) / B for n, v in d.items()} for path, d in ms.items()}
    total = {path: sum(d.values()) for path, d in med.items()}
    line = dict(frames=B, frame_hw=[H, W], det_input=list(IN), arch=args.arch, tiles_per_frame=9, overlap=args.overlap, edge_margin=args.edge_margin,
                repeats=args.repeats, ms_per_frame={p: {n: round(v, 4) for n, v in d.items()} for p, d in med.items()},
                ms_per_frame_total={p: round(v, 4) for p, v in total.items()}, tiled_over_letterboxed=round(total["tiled"] / total["letterboxed"], 3),
                detector_ms_min={p: round(min(ms[p]["detector"]) / B, 4) for p in ms}, detector_ms_max={p: round(max(ms[p]["detector"]) / B, 4) for p in ms},
                faces_per_frame=faces, device=ctx.name())
    print(json.dumps(line), flush=True)
    det.close()
    ctx.close()


if __name__ == "__main__":
    main()
