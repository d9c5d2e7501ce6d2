#!/usr/bin/env python3
"""NV12 against BGR input on 1080p frames, for docs/FINDINGS.md.  One process; the BGR frames are fid_nv12_to_bgr of the NV12 frames, so both
paths compute the same bytes (checked once before anything is timed).

 (a) stages: device-event time of the letterbox (1080p -> 640x640), the tile cut (9 tiles per frame) and the packed warp (--rows faces), the NV12
     call against its BGR namesake, plus fid_nv12_to_bgr alone (the pass the fused calls make unnecessary).  Every timed window holds --inner
     back-to-back calls; the two formats take turns inside every repeat; round 0 warms up; median, min and max of --repeats rounds.
 (b) steps: SCRFD-2.5G + MobileFaceNet (the nets of the bench's 1080p configuration), FacePipeline at --frames frames per step, letterboxed and tiled:
       upload   device-event time of one staging buffer's host-to-device copy (fid_upload_async_slot + fid_upload_wait_slot), and its GB/s;
       device   device-event time of run_step on frames that are already resident;
       runner   host wall time per step of video.StreamRunner over --steps steps (host fill of the pinned buffer, upload, step, results()).
     `upload_over_device` > 1 says the copy, not the kernels, bounds a double-buffered step.

One JSON line.   python tools/bench_nv12.py [--frames 32] [--repeats 7] [--inner 20] [--steps 12] [--rows 256] [--skip-steps]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scrfd_arcface_facerecognition_amd import archs  # noqa: E402
from scrfd_arcface_facerecognition_amd._lib import Context, Nv12Frames, c_i32_p, check  # noqa: E402
from scrfd_arcface_facerecognition_amd.engine import CompiledNet, Gallery  # noqa: E402
from scrfd_arcface_facerecognition_amd.pipeline import FacePipeline, calibrate_detector_bias, tile_plan  # noqa: E402
from scrfd_arcface_facerecognition_amd.video import StreamRunner  # noqa: E402

H, W, IN = 1080, 1920, (640, 640)
TEMPLATE = np.array([[38.2946, 51.6963], [73.5318, 51.5014], [56.0252, 71.7366], [41.5493, 92.3655], [70.7299, 92.2041]], np.float64)


def note(msg):
    print(f"[bench_nv12] {msg}", file=sys.stderr, flush=True)


def spread(v, per=1.0):
    return dict(median=round(statistics.median(v) / per, 4), min=round(min(v) / per, 4), max=round(max(v) / per, 4))


def synthetic_landmarks(rng, n, B):
    """n faces 80 .. 250 pixels wide, turned up to 20 degrees, anywhere in the frame (some reach past its edges): kps [B, cap, 10], src [n]"""
    cap = -(-n // B)
    kps = np.zeros((B, cap, 10), np.float32)
    src = np.empty(n, np.int32)
    for i in range(n):
        b, f = i % B, i // B
        s, a = rng.uniform(0.7, 2.2), np.deg2rad(rng.uniform(-20, 20))
        R = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
        kps[b, f] = (((TEMPLATE - 56.0) * s) @ R.T + [rng.uniform(0, W), rng.uniform(0, H)]).astype(np.float32).reshape(10)
        src[i] = b * cap + f
    return kps, src, cap


def bench_stages(ctx, nv, bgr, B, args):
    lib, h = ctx.lib, ctx.handle
    tiles = tile_plan(H, W, IN, 128, True, B)
    T = len(tiles)
    kps_h, src_h, cap = synthetic_landmarks(np.random.default_rng(1), args.rows, B)
    kps, src = ctx.to_device(kps_h), ctx.to_device(src_h)
    n = args.rows
    lb = {k: ctx.empty((B,) + IN + (3,), np.uint8) for k in ("nv12", "bgr")}
    tb = {k: ctx.empty((T,) + IN + (3,), np.uint8) for k in ("nv12", "bgr")}
    cr = {k: ctx.empty((n, 112, 112, 3), np.uint8) for k in ("nv12", "bgr")}
    conv = ctx.empty((B, H, W, 3), np.uint8)
    tp = tiles.ctypes.data_as(c_i32_p)
    calls = {
        "letterbox": {"nv12": lambda: check(lib.fid_letterbox_nv12(h, *nv.args(), B, H, W, C.c_void_p(lb["nv12"].ptr), IN[0], IN[1], None)),
                      "bgr": lambda: check(lib.fid_letterbox(h, C.c_void_p(bgr.ptr), B, H, W, C.c_void_p(lb["bgr"].ptr), IN[0], IN[1], None))},
        "tile_cut": {"nv12": lambda: check(lib.fid_tile_cut_nv12(h, *nv.args(), B, H, W, tp, T, C.c_void_p(tb["nv12"].ptr), IN[0], IN[1])),
                     "bgr": lambda: check(lib.fid_tile_cut(h, C.c_void_p(bgr.ptr), B, H, W, tp, T, C.c_void_p(tb["bgr"].ptr), IN[0], IN[1]))},
        "align_packed": {"nv12": lambda: check(lib.fid_align_crops_packed_nv12(h, *nv.args(), B, H, W, C.c_void_p(kps.ptr), cap, C.c_void_p(src.ptr), n,
                                                                                C.c_void_p(cr["nv12"].ptr), None)),
                         "bgr": lambda: check(lib.fid_align_crops_packed(h, C.c_void_p(bgr.ptr), B, H, W, C.c_void_p(kps.ptr), cap, C.c_void_p(src.ptr), n,
                                                                         C.c_void_p(cr["bgr"].ptr), None))},
        "nv12_to_bgr": {"nv12": lambda: check(lib.fid_nv12_to_bgr(h, *nv.args(), B, H, W, C.c_void_p(conv.ptr)))},
    }
    ms = {stage: {fmt: [] for fmt in fmts} for stage, fmts in calls.items()}
    for rep in range(args.repeats + 1):                               # round 0 warms up
        for stage, fmts in calls.items():
            for fmt, call in fmts.items():
                ctx.event_record(0)
                for _ in range(args.inner):
                    call()
                ctx.event_record(1)
                t = ctx.elapsed_ms(0, 1) / args.inner
                if rep:
                    ms[stage][fmt].append(t)
        if rep == 0:                                                  # the two paths wrote the same bytes
            for bufs in (lb, tb, cr):
                assert np.array_equal(bufs["nv12"].download(), bufs["bgr"].download())
            note("stage outputs equal; timing")
    out = {stage: {fmt: spread(v) for fmt, v in d.items()} for stage, d in ms.items()}
    for stage in ("letterbox", "tile_cut", "align_packed"):
        out[stage]["nv12_over_bgr"] = round(out[stage]["nv12"]["median"] / out[stage]["bgr"]["median"], 3)
    return dict(ms_per_call=out, tiles=T, rows=n)


def bench_steps(ctx, nv_host, bgr_host, B, args):
    lib, h = ctx.lib, ctx.handle
    det_net = archs.scrfd_2_5g(IN)
    # (the bias is calibrated on the frames' own letterboxes so that every input has a few dozen candidates, as a trained detector would)
    lbuf, fr4 = ctx.empty((4,) + IN + (3,), np.uint8), ctx.to_device(bgr_host[:4])
    check(lib.fid_letterbox(h, C.c_void_p(fr4.ptr), 4, H, W, C.c_void_p(lbuf.ptr), IN[0], IN[1], None))
    det_P, _ = calibrate_detector_bias(ctx, det_net, archs.synth_params(det_net, 0), lbuf.download(), target=48, max_batch=4)
    rec_net = archs.mobilefacenet()
    rec = CompiledNet(ctx, rec_net, archs.synth_params(rec_net, 0), max_batch=B)
    gallery = Gallery(ctx, np.random.default_rng(2).standard_normal((64, 512)).astype(np.float32))
    items = {"nv12": nv_host, "bgr": bgr_host}
    out = {}
    for mode, tiling in (("letterboxed", None), ("tiled", dict(overlap=128, edge_margin=8, overview=True))):
        note(f"steps: {mode}")
        det = CompiledNet(ctx, det_net, det_P, max_batch=B * (9 if tiling else 1))
        pipes = {fmt: FacePipeline(ctx, det, rec, batch=B, faces_per_frame=1, tiling=tiling) for fmt in items}
        runners = {fmt: StreamRunner(pipes[fmt], gallery, (H, W), pixel_format=fmt) for fmt in items}
        up, dev, wall, faces = ({fmt: [] for fmt in items} for _ in range(4))
        for rep in range(args.repeats + 1):                           # round 0 warms up (kernel picks, scratch arenas, code objects)
            for fmt, r in runners.items():
                r.host[0].array[...] = items[fmt]
                ctx.event_record(0)
                r._upload(0)
                check(lib.fid_upload_wait_slot(h, 0))
                ctx.event_record(1)
                pipes[fmt].run_step(r.frames[0], H, W, gallery, 0.4)
                ctx.event_record(2)
                check(lib.fid_upload_release(h, 0))
                t_up, t_dev = ctx.elapsed_ms(0, 1), ctx.elapsed_ms(1, 2)
                faces[fmt] = sum(len(f) for f in pipes[fmt].results(gallery))
                steps = args.steps if rep else 2
                t0 = time.perf_counter()
                n_out = sum(1 for _ in r.run(items[fmt][i % B] for i in range(steps * B)))
                t_wall = (time.perf_counter() - t0) * 1e3 / steps
                assert n_out == steps * B
                if rep:
                    up[fmt].append(t_up); dev[fmt].append(t_dev); wall[fmt].append(t_wall)
            note(f"  round {rep} done")
        assert faces["nv12"] == faces["bgr"], faces
        res = {}
        for fmt, r in runners.items():
            u = spread(up[fmt])
            res[fmt] = dict(upload_bytes_per_step=r.upload_bytes, upload_ms=u, upload_gb_per_s=round(r.upload_bytes / u["median"] / 1e6, 2),
                            device_step_ms=spread(dev[fmt]), runner_wall_ms_per_step=spread(wall[fmt]),
                            upload_over_device=round(u["median"] / statistics.median(dev[fmt]), 2), faces=faces[fmt])
            r.close()
        res["runner_wall_nv12_over_bgr"] = round(res["nv12"]["runner_wall_ms_per_step"]["median"] / res["bgr"]["runner_wall_ms_per_step"]["median"], 3)
        out[mode] = res
        det.close()
    rec.close()
    gallery.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32, help="frames per step")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20, help="calls per timed window of a stage")
    ap.add_argument("--steps", type=int, default=12, help="steps per timed StreamRunner run")
    ap.add_argument("--rows", type=int, default=256, help="faces of the packed warp")
    ap.add_argument("--skip-steps", action="store_true", help="stages only")
    args = ap.parse_args()
    assert args.repeats >= 5 and args.frames >= 4 and args.inner >= 1 and args.steps >= 2 and 0 < args.rows <= 65535
    B = args.frames
    ctx = Context(0)
    rng = np.random.default_rng(0)
    nv_host = rng.integers(0, 256, (B, H * 3 // 2, W), dtype=np.uint8)      # random planes, dense layout
    nv_dev = ctx.to_device(nv_host)
    nv = Nv12Frames(nv_dev, H, W)
    bgr = ctx.empty((B, H, W, 3), np.uint8)
    check(ctx.lib.fid_nv12_to_bgr(ctx.handle, *nv.args(), B, H, W, C.c_void_p(bgr.ptr)))
    line = dict(frames=B, frame_hw=[H, W], det_input=list(IN), repeats=args.repeats, inner=args.inner, device=ctx.name(),
                bytes_per_step=dict(nv12=int(nv_host.nbytes), bgr=B * H * W * 3))
    note("stages")
    line["stages"] = bench_stages(ctx, nv, bgr, B, args)
    note("stages: " + json.dumps(line["stages"]))
    if not args.skip_steps:
        line["steps_per_run"] = args.steps
        line["steps"] = bench_steps(ctx, nv_host, bgr.download(), B, args)
    print(json.dumps(line), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
