#!/usr/bin/env python3
"""Tracked faces (fid_track_step / fid_track_identify, pipeline.TrackedFacePipeline) measurements for docs/FINDINGS.md.
A video: one smooth random image, 640 x 640 windows of it sliding 2 pixels per frame, forth and back (period 256 frames = 4 steps of 64), so
that the sequence is continuous for any number of steps; SCRFD-10G + IResNet-50 with seeded weights, the detector's cls bias calibrated on the
first frames; a gallery of random rows at threshold 0 ("named" = the best cosine is positive: nearly every face) and, for the other regime,
at 0.99 (nobody is ever named: retry = 1 embeds every face every frame).
  pipelines: PackedFacePipeline (the yardstick: untouched by the tracker) and TrackedFacePipeline at refresh 1, 4, 16, all rows="count" with
             the same buckets, in ONE process.  Per configuration: warm(), 8 steps to reach the steady state, then 5 repeats of 4 consecutive
             steps between two HIP events (fid_event_*), the configurations alternating inside every repeat; median ms per step and the mean
             rows embedded per step (counted in a pass of its own).
  calls:     fid_track_step and fid_track_identify alone between events, median of 5, on the detections of the video (B = 64, cap = 256,
             T = 64) and on a crowded synthetic scene: 64 frames of 50 boxes each that move 2 pixels per frame.
Needs nothing outside the repository.  bench_track.py [--batch 64] [--row-cap N] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, STEPS, SETTLE = 5, 4, 8
HW = 640


def smooth_image(rng, h, w, cell=40):
    gh, gw = h // cell + 2, w // cell + 2
    grid = rng.integers(0, 256, (gh, gw, 3)).astype(np.float64)
    ys, xs = np.arange(h) / cell, np.arange(w) / cell
    y0, x0 = ys.astype(int), xs.astype(int)
    fy, fx = (ys - y0)[:, None, None], (xs - x0)[None, :, None]
    top = grid[y0][:, x0] * (1 - fx) + grid[y0][:, x0 + 1] * fx
    bot = grid[y0 + 1][:, x0] * (1 - fx) + grid[y0 + 1][:, x0 + 1] * fx
    return np.clip(np.rint(top * (1 - fy) + bot * fy), 0, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--row-cap", type=int, default=0, help="rows the pipelines hold (0: the multiple of 64 at or above 1.25 x the faces of the first step)")
    ap.add_argument("--gallery", type=int, default=1000)
    ap.add_argument("--target", type=int, default=10, help="anchors above 0.5 the calibration leaves in the quietest calibration frame")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    os.environ.setdefault("FID_AUTOTUNE", "0")            # heuristic kernel plans for every configuration: count mode meets many recogniser batch sizes
    from scrfd_arcface_facerecognition_amd import _lib, archs
    from scrfd_arcface_facerecognition_amd._lib import Context, check
    from scrfd_arcface_facerecognition_amd.engine import CompiledNet, Gallery
    from scrfd_arcface_facerecognition_amd.pipeline import PackedFacePipeline, TrackedFacePipeline, calibrate_detector_bias

    def log(msg):
        print(f"[bench_track] {msg}", file=sys.stderr, flush=True)

    ctx = Context(0)
    B = args.batch
    rng = np.random.default_rng(1234)
    half = 2 * B                                           # frames per direction
    wide = smooth_image(rng, HW, HW + 2 * half)
    tri = [t if t <= half else 2 * half - t for t in range(2 * half)]
    batches = [ctx.to_device(np.stack([wide[:, 2 * tri[(k * B + i) % (2 * half)]:2 * tri[(k * B + i) % (2 * half)] + HW] for i in range(B)]))
               for k in range(4)]
    det_net = archs.scrfd_10g((HW, HW))
    calib = np.stack([wide[:, 2 * t:2 * t + HW] for t in range(0, half, half // 8)][:8])
    det_P, _ = calibrate_detector_bias(ctx, det_net, archs.synth_params(det_net, seed=0), calib, target=args.target)
    rec_net = archs.iresnet50()
    det = CompiledNet(ctx, det_net, det_P, max_batch=B)
    probe = PackedFacePipeline(ctx, det, CompiledNet(ctx, archs.mobilefacenet(), archs.synth_params(archs.mobilefacenet(), 0), max_batch=8),
                               batch=B, row_cap=8)
    probe.detect(batches[0], HW, HW)                       # the face counts decide the shapes: one detector pass
    probe.post.check()
    found = int(np.clip(probe.post.counts.download()[:B], 0, probe.post.cap).sum())
    probe.rec.close()
    if args.row_cap <= 0:
        args.row_cap = max(64, -(-(found * 5 // 4) // 64) * 64)
    log(f"{found} faces in the first step, row_cap {args.row_cap}")
    # (IResNet-50's largest activation must stay below 2 GiB: 1 280 rows)
    assert 0 < found <= args.row_cap <= 1280, f"row_cap {args.row_cap} against {found} faces per step: lower --target"
    rec = CompiledNet(ctx, rec_net, archs.synth_params(rec_net, seed=0), max_batch=args.row_cap)
    gallery = Gallery(ctx, np.random.default_rng(99).standard_normal((args.gallery, 512)).astype(np.float32))
    buckets = list(range(64, args.row_cap, 64)) + [args.row_cap]
    kw = dict(batch=B, row_cap=args.row_cap, rows="count", buckets=buckets)
    configs = {"packed": (PackedFacePipeline(ctx, det, rec, **kw), 0.0)}
    for refresh in (1, 4, 16):
        configs[f"tracked_refresh_{refresh}"] = (TrackedFacePipeline(ctx, det, rec, refresh=refresh, retry=1, **kw), 0.0)
    configs["tracked_refresh_16_nobody_named"] = (TrackedFacePipeline(ctx, det, rec, refresh=16, retry=1, **kw), 0.99)

    step_no = {n: 0 for n in configs}

    def run(name, k):
        pipe, thr = configs[name]
        for _ in range(k):
            pipe.run_step(batches[step_no[name] % 4], HW, HW, gallery, thr)
            step_no[name] += 1

    first = True
    for name, (pipe, thr) in configs.items():
        log(f"warming {name}")
        if first:
            pipe.warm(batches[0], HW, HW, gallery, thr)    # every bucket once: the nets are shared, so once for all configurations
            first = False
        run(name, SETTLE)
        ctx.sync()
    pipe0 = configs["packed"][0]
    faces = pipe0.post.counts.download()[:B]
    log(f"faces per frame in the last packed step: min {faces.min()}, median {int(np.median(faces))}, max {faces.max()}")

    ms = {n: [] for n in configs}
    for r in range(REPS):
        for name in configs:                               # alternating: every repeat visits every configuration
            ctx.sync()
            ctx.event_record(0)
            run(name, STEPS)
            ctx.event_record(1)
            ms[name].append(ctx.elapsed_ms(0, 1) / STEPS)
        log(f"repeat {r}: " + ", ".join(f"{n} {ms[n][-1]:.3f}" for n in configs))
    rows = {n: [] for n in configs}
    total_faces = []
    for name, (pipe, thr) in configs.items():              # rows per step, in a pass of its own (the read-back is not in the timed steps)
        for _ in range(2 * STEPS):
            run(name, 1)
            rows[name].append(min(int(pipe.offsets.download()[B]), args.row_cap))
            if name == "packed":
                total_faces.append(int(np.clip(pipe.post.counts.download()[:B], 0, pipe.post.cap).sum()))
        if hasattr(pipe, "tracker_state"):
            slots, per_stream = pipe.tracker_state()
            log(f"{name}: live tracks {int((slots[..., 0] >= 0).sum())}, named {int(((slots[..., 0] >= 0) & (slots[..., 3] >= 0)).sum())}, "
                f"ids handed out {int(per_stream[0, 0])}, detections without a slot {int(per_stream[0, 1])}")

    # ---- the two calls alone -----------------------------------------------------------------------------------
    def time_calls(cap, n_frames, label, steps_of):
        trk = C.c_void_p()
        check(ctx.lib.fid_tracker_create(ctx.handle, 1, 64, C.byref(trk)))
        cfg = _lib.TrackConfig(0.3, 15, 16, 1)
        row_cap = args.row_cap
        track, offsets, src = ctx.empty((n_frames, cap, 2), np.int32), ctx.empty((n_frames + 1,), np.int32), ctx.empty((row_cap,), np.int32)
        idx, score = ctx.to_device(np.zeros(row_cap, np.int32)), ctx.to_device(np.full(row_cap, 0.5, np.float32))
        ii, sc = ctx.empty((n_frames, cap), np.int32), ctx.empty((n_frames, cap), np.float32)
        stream = np.zeros(n_frames, np.int32)
        t_step, t_ident, n_rows = [], [], []
        for rep in range(REPS + 2):
            d, c = steps_of(rep)
            ctx.sync()
            ctx.event_record(0)
            check(ctx.lib.fid_track_step(ctx.handle, trk, C.c_void_p(d.ptr), C.c_void_p(c.ptr), stream.ctypes.data_as(_lib.c_i32_p), n_frames, cap,
                                         C.byref(cfg), C.c_void_p(track.ptr), C.c_void_p(offsets.ptr), C.c_void_p(src.ptr), row_cap))
            ctx.event_record(1)
            a = ctx.elapsed_ms(0, 1)
            n = min(int(offsets.download()[n_frames]), row_cap)
            ctx.event_record(2)
            check(ctx.lib.fid_track_identify(ctx.handle, trk, C.c_void_p(c.ptr), stream.ctypes.data_as(_lib.c_i32_p), n_frames, cap,
                                             C.c_void_p(track.ptr), C.c_void_p(offsets.ptr), C.c_void_p(src.ptr), row_cap, C.c_void_p(idx.ptr),
                                             C.c_void_p(score.ptr), n, C.c_void_p(ii.ptr), C.c_void_p(sc.ptr)))
            ctx.event_record(3)
            b = ctx.elapsed_ms(2, 3)
            if rep >= 2:                                   # (the first call starts every track, the second is the first with names)
                t_step.append(a)
                t_ident.append(b)
                n_rows.append(n)
        check(ctx.lib.fid_tracker_destroy(ctx.handle, trk))
        out = dict(scene=label, frames=n_frames, cap=cap, step_ms=round(statistics.median(t_step), 4), identify_ms=round(statistics.median(t_ident), 4),
                   step_ms_min_max=[round(min(t_step), 4), round(max(t_step), 4)], rows_per_call=int(statistics.median(n_rows)))
        log(str(out))
        return out

    calls = []
    dets = []
    for k in range(4):                                     # the video's own detections, four consecutive steps
        pipe0.detect(batches[k], HW, HW)
        ctx.sync()
        dets.append((ctx.to_device(pipe0.post.det.download()), ctx.to_device(pipe0.post.counts.download())))
    calls.append(time_calls(pipe0.post.cap, B, f"video, {int(np.median(faces))} faces per frame", lambda rep: dets[rep % 4]))
    crowd = []
    for k in range(4):
        d = np.zeros((B, 256, 5), np.float32)
        for i in range(B):
            t = tri[(k * B + i) % (2 * half)]
            for f in range(50):
                x, y = 60 * (f % 10) + 2 * t, 70 * (f // 10)
                d[i, f] = (x, y, x + 40, y + 50, 0.9)
        crowd.append((ctx.to_device(d), ctx.to_device(np.full(B, 50, np.int32))))
    calls.append(time_calls(256, B, "synthetic, 50 faces per frame", lambda rep: crowd[rep % 4]))

    med = statistics.median
    line = {"tool": "bench_track", "device": ctx.name(), "date": time.strftime("%Y-%m-%d"), "batch": B, "det": "scrfd_10g", "rec": "arcface_r50",
            "gallery": args.gallery, "row_cap": args.row_cap, "autotune": os.environ["FID_AUTOTUNE"], "repeats": REPS, "steps_per_repeat": STEPS,
            "faces_per_step_mean": round(float(np.mean(total_faces)), 1),
            "configs": {n: {"ms_per_step": round(med(ms[n]), 4), "ms_per_step_min_max": [round(min(ms[n]), 4), round(max(ms[n]), 4)],
                            "rows_embedded_per_step_mean": round(float(np.mean(rows[n])), 1)} for n in configs},
            "calls": calls}
    out = json.dumps(line)
    print(out, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(out + "\n")


if __name__ == "__main__":
    main()
