#!/usr/bin/env python3
"""The measured face quality (fid_face_measure) timed for docs/FINDINGS.md.
1. The call alone, at 128 and 4096 rows of seeded random crops with landmarks and matrices (every row a face): 5 warm-up calls, then 7 repeats of
   200 calls between two HIP events (fid_event_*); the median repeat, per call.  Beside the time, the bytes: 37 632 B per row is the algorithmic
   read (the whole crop once), 21 648 B per row is what the kernel loads (rows 15 .. 96, columns 12 .. 99), 96 B per row are written; the rates are
   those bytes over the call time -- the call, not the kernel: launch overhead is inside.
2. A PackedFacePipeline step (SCRFD-500M at 640 x 640, MobileFaceNet, seeded weights, `--batch` noise frames, row_cap 128, rows="capacity") with and
   without measure=True: 3 warm-up steps each, then 7 repeats of 20 steps, the two pipelines alternating inside every repeat; the median repeat,
   per step.  Needs nothing outside the repository.
bench_measure.py [--batch 8] [--out FILE]"""
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
STEP_WARM, STEP_CALLS = 3, 20
CROP_BYTES, LOADED_BYTES, WRITTEN_BYTES = 112 * 112 * 3, 82 * 22 * 12, 96


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from scrfd_arcface_facerecognition_amd._lib import Context, check
    from scrfd_arcface_facerecognition_amd.engine import CompiledNet, Gallery, resolve_model
    from scrfd_arcface_facerecognition_amd.pipeline import PackedFacePipeline, calibrate_detector_bias

    ctx = Context(0)
    rng = np.random.default_rng(2025)
    tmpl = np.array([38.2946, 51.6963, 73.5318, 51.5014, 56.0252, 71.7366, 41.5493, 92.3655, 70.7299, 92.2041], np.float32)

    def timed(fn, warm, calls):
        for _ in range(warm):
            fn()
        ctx.sync()
        ms = []
        for _ in range(REPS):
            ctx.event_record(0)
            for _ in range(calls):
                fn()
            ctx.event_record(1)
            ms.append(ctx.elapsed_ms(0, 1) / calls)
        return statistics.median(ms), min(ms), max(ms)

    out = dict(device=ctx.name(), crop_bytes=CROP_BYTES, loaded_bytes_per_row=LOADED_BYTES, written_bytes_per_row=WRITTEN_BYTES)
    for n in (128, 4096):
        crops = ctx.to_device(rng.integers(0, 256, (n, 112, 112, 3), dtype=np.uint8))
        kps = ctx.to_device((tmpl[None] + rng.normal(0, 2.0, (n, 10))).astype(np.float32))
        M = ctx.to_device(np.tile(np.array([1.0, 0, 0, 0, 1.0, 0]), (n, 1)) + rng.normal(0, 0.01, (n, 6)))
        stats, meas = ctx.empty((n, 8), np.int64), ctx.empty((n, 8), np.float32)

        def call():
            check(ctx.lib.fid_face_measure(ctx.handle, C.c_void_p(crops.ptr), n, C.c_void_p(kps.ptr), None, C.c_void_p(M.ptr), C.c_void_p(stats.ptr),
                                           C.c_void_p(meas.ptr)))

        med, lo, hi = timed(call, WARM, CALLS)
        out[f"rows_{n}"] = dict(us_per_call=round(med * 1e3, 2), us_min=round(lo * 1e3, 2), us_max=round(hi * 1e3, 2),
                                algorithmic_GBps=round(n * CROP_BYTES / (med * 1e-3) / 1e9, 1),
                                loaded_GBps=round(n * LOADED_BYTES / (med * 1e-3) / 1e9, 1))
        assert (stats.download()[:, 7] & 1).all()

    B, HW = args.batch, 640
    frames = rng.integers(0, 256, (B, HW, HW, 3), dtype=np.uint8)
    det_net, det_P0 = resolve_model("synthetic:scrfd_500m?seed=5", (HW, HW))
    det_P, _ = calibrate_detector_bias(ctx, det_net, det_P0, frames[:4], target=16, max_batch=4)
    rec_net, rec_P = resolve_model("synthetic:arcface_mbf?seed=5")
    det, rec = CompiledNet(ctx, det_net, det_P, max_batch=B), CompiledNet(ctx, rec_net, rec_P, max_batch=128)
    gallery = Gallery(ctx, rng.standard_normal((1000, 512)).astype(np.float32))
    fr = ctx.to_device(frames)
    pipes = {key: PackedFacePipeline(ctx, det, rec, batch=B, row_cap=128, measure=flag) for key, flag in (("plain", False), ("measure", True))}
    for p in pipes.values():
        for _ in range(STEP_WARM):
            p.run_step(fr, HW, HW, gallery, 0.4)
    ctx.sync()
    ms = {key: [] for key in pipes}
    for _ in range(REPS):
        for key, p in pipes.items():
            ctx.event_record(0)
            for _ in range(STEP_CALLS):
                p.run_step(fr, HW, HW, gallery, 0.4)
            ctx.event_record(1)
            ms[key].append(ctx.elapsed_ms(0, 1) / STEP_CALLS)
    faces = sum(len(r) for r in pipes["measure"].results(gallery))
    out["pipeline"] = dict(batch=B, size=HW, row_cap=128, faces=faces,
                           **{f"{key}_ms_per_step": round(statistics.median(v), 4) for key, v in ms.items()},
                           **{f"{key}_ms_min_max": [round(min(v), 4), round(max(v), 4)] for key, v in ms.items()})
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
