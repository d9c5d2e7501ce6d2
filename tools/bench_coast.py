#!/usr/bin/env python3
"""Coasting (fid_track_coast, TrackedFacePipeline(coast=...)) measurements for docs/FINDINGS.md ("Coasting").  One process.

The video and the nets are tools/bench_track.py's: one smooth random image, 640 x 640 windows sliding 2 pixels per frame forth and back,
SCRFD-10G + IResNet-50 with seeded weights, B = 64, a gallery of random rows at threshold 0, refresh 16, retry 1, rows="count".
  steps   the tracked step in three forms, alternating inside every repeat: `parent_calls` -- a TrackedFacePipeline whose match() is the body
          it had before the coaster existed (PackedFacePipeline.match, then identify) --, `coast_none` (the default: must cost the same, nothing
          is launched or allocated) and `coast_on` (CoastConfig(): the two launches of fid_track_coast per step).  8 steps to settle, then
          5 repeats of 4 consecutive steps between two device events; median ms per step.
  calls   fid_track_step, fid_track_identify and fid_track_coast alone between device events on the video's own detections (cap = 256,
          T = 64), median of 5: the expectation to confirm or refute is that the coast costs about what the identify costs.
  overlay fid_redact_faces (mosaic and fill) and fid_draw_faces on the 64 frames over the step's own tables (cap slots) against the coaster's
          extended tables (cap + T slots): what the longer face tables cost the existing kernels.  Median of 5 rounds of 10 calls.
One JSON line on stdout, appended to --out.   python tools/bench_coast.py [--out profiles/coast/bench_coast.jsonl]"""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

REPS, STEPS, SETTLE, INNER = 5, 4, 8, 10
HW = 640


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--gallery", type=int, default=1000)
    ap.add_argument("--target", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coast", "bench_coast.jsonl"))
    args = ap.parse_args()
    os.environ.setdefault("FID_AUTOTUNE", "0")
    from bench_track import smooth_image
    from scrfd_arcface_facerecognition_amd import _lib, archs
    from scrfd_arcface_facerecognition_amd._lib import CoastConfig, Context, DrawStyle, RedactStyle, check
    from scrfd_arcface_facerecognition_amd.engine import CompiledNet, Gallery, LabelTable
    from scrfd_arcface_facerecognition_amd.pipeline import PackedFacePipeline, TrackedFacePipeline, calibrate_detector_bias

    def log(msg):
        print(f"[bench_coast] {msg}", file=sys.stderr, flush=True)

    class ParentCalls(TrackedFacePipeline):
        """match() as it was before the coaster: the launches of the parent commit's tracked step"""

        def match(self, gallery, thresh=0.4, q=None, n=None, idx=None, score=None):
            n = self.n_run if n is None else n
            PackedFacePipeline.match(self, gallery, thresh, q=q, n=n, idx=idx, score=score)
            self.identify(n, idx, score)

    ctx = Context(0)
    B = args.batch
    rng = np.random.default_rng(1234)
    half = 2 * B
    wide = smooth_image(rng, HW, HW + 2 * half)
    tri = [t if t <= half else 2 * half - t for t in range(2 * half)]
    batches = [ctx.to_device(np.stack([wide[:, 2 * tri[(k * B + i) % (2 * half)]:2 * tri[(k * B + i) % (2 * half)] + HW] for i in range(B)]))
               for k in range(4)]
    det_net = archs.scrfd_10g((HW, HW))
    calib = np.stack([wide[:, 2 * t:2 * t + HW] for t in range(0, half, half // 8)][:8])
    det_P, _ = calibrate_detector_bias(ctx, det_net, archs.synth_params(det_net, seed=0), calib, target=args.target)
    det = CompiledNet(ctx, det_net, det_P, max_batch=B)
    probe = PackedFacePipeline(ctx, det, CompiledNet(ctx, archs.mobilefacenet(), archs.synth_params(archs.mobilefacenet(), 0), max_batch=8),
                               batch=B, row_cap=8)
    probe.detect(batches[0], HW, HW)
    found = int(np.clip(probe.post.counts.download()[:B], 0, probe.post.cap).sum())
    probe.rec.close()
    row_cap = max(64, -(-(found * 5 // 4) // 64) * 64)
    log(f"{found} faces in the first step, row_cap {row_cap}")
    assert 0 < found <= row_cap <= 1280
    rec_net = archs.iresnet50()
    rec = CompiledNet(ctx, rec_net, archs.synth_params(rec_net, seed=0), max_batch=row_cap)
    gallery = Gallery(ctx, np.random.default_rng(99).standard_normal((args.gallery, 512)).astype(np.float32))
    kw = dict(batch=B, row_cap=row_cap, rows="count", buckets=list(range(64, row_cap, 64)) + [row_cap], refresh=16, retry=1)
    configs = {"parent_calls": ParentCalls(ctx, det, rec, **kw), "coast_none": TrackedFacePipeline(ctx, det, rec, **kw),
               "coast_on": TrackedFacePipeline(ctx, det, rec, coast=CoastConfig(), **kw)}
    step_no = {n: 0 for n in configs}

    def run(name, k):
        for _ in range(k):
            configs[name].run_step(batches[step_no[name] % 4], HW, HW, gallery, 0.0)
            step_no[name] += 1

    for i, (name, pipe) in enumerate(configs.items()):
        log(f"warming {name}")
        if i == 0:
            pipe.warm(batches[0], HW, HW, gallery, 0.0)
        run(name, SETTLE)
        ctx.sync()
    ms = {n: [] for n in configs}
    for r in range(REPS):
        for name in configs:
            ctx.sync()
            ctx.event_record(0)
            run(name, STEPS)
            ctx.event_record(1)
            ms[name].append(ctx.elapsed_ms(0, 1) / STEPS)
        log(f"repeat {r}: " + ", ".join(f"{n} {ms[n][-1]:.3f}" for n in configs))
    on = configs["coast_on"]
    coasted = []
    for _ in range(4):                                     # coasted rows per step, in a pass of its own
        run("coast_on", 1)
        coasted.append(sum(len(r) for r in on.results_coasted()))
    faces = int(np.clip(on.post.counts.download()[:B], 0, on.post.cap).sum())

    # ---- the three calls alone, on the video's detections
    cap, T = on.post.cap, 64
    dets = []
    for k in range(4):
        on.detect(batches[k], HW, HW)
        ctx.sync()
        dets.append((ctx.to_device(on.post.det.download()), ctx.to_device(on.post.counts.download())))
    trk, coaster = C.c_void_p(), C.c_void_p()
    check(ctx.lib.fid_tracker_create(ctx.handle, 1, T, C.byref(trk)))
    check(ctx.lib.fid_coaster_create(ctx.handle, 1, T, C.byref(coaster)))
    tcfg, ccfg = _lib.TrackConfig(0.3, 15, 16, 1), CoastConfig()
    track, offsets, src = ctx.empty((B, cap, 2), np.int32), ctx.empty((B + 1,), np.int32), ctx.empty((row_cap,), np.int32)
    idx, score = ctx.to_device(np.zeros(row_cap, np.int32)), ctx.to_device(np.full(row_cap, 0.5, np.float32))
    ii, sc = ctx.empty((B, cap), np.int32), ctx.empty((B, cap), np.float32)
    cap2 = cap + T
    ext = [ctx.empty((B, cap2, 5), np.float32), ctx.empty((B,), np.int32), ctx.empty((B, cap2, 2), np.int32), ctx.empty((B, cap2), np.int32),
           ctx.empty((B, cap2), np.float32)]
    stream = np.zeros(B, np.int32)
    sp = stream.ctypes.data_as(_lib.c_i32_p)
    p = lambda b: C.c_void_p(b.ptr)
    t_step, t_ident, t_coast = [], [], []
    for rep in range(REPS + 2):
        d, c = dets[rep % 4]
        ctx.sync()
        ctx.event_record(0)
        check(ctx.lib.fid_track_step(ctx.handle, trk, p(d), p(c), sp, B, cap, C.byref(tcfg), p(track), p(offsets), p(src), row_cap))
        ctx.event_record(1)
        a = ctx.elapsed_ms(0, 1)
        n = min(int(offsets.download()[B]), row_cap)
        ctx.event_record(0)
        check(ctx.lib.fid_track_identify(ctx.handle, trk, p(c), sp, B, cap, p(track), p(offsets), p(src), row_cap, p(idx), p(score), n, p(ii), p(sc)))
        ctx.event_record(1)
        b = ctx.elapsed_ms(0, 1)
        ctx.event_record(0)
        check(ctx.lib.fid_track_coast(ctx.handle, coaster, trk, sp, B, cap, p(d), p(c), p(track), p(ii), p(sc), C.byref(ccfg), *[p(o) for o in ext]))
        ctx.event_record(1)
        e = ctx.elapsed_ms(0, 1)
        if rep >= 2:
            t_step.append(a)
            t_ident.append(b)
            t_coast.append(e)
    med = statistics.median
    calls = dict(frames=B, cap=cap, T=T, step_ms=round(med(t_step), 4), identify_ms=round(med(t_ident), 4), coast_ms=round(med(t_coast), 4),
                 coast_ms_min_max=[round(min(t_coast), 4), round(max(t_coast), 4)], coast_over_identify=round(med(t_coast) / med(t_ident), 3))
    log(str(calls))

    # ---- the existing kernels over cap and over cap + T slots (the last step's tables; the coaster's hold the same faces plus the coasted)
    labels = LabelTable(ctx, [f"person_{g:04d}" for g in range(args.gallery)])
    d, c = dets[(REPS + 1) % 4]
    frames = batches[(REPS + 1) % 4]
    both = _lib.REDACT_UNKNOWN | _lib.REDACT_KNOWN
    mosaic, fill, dstyle = RedactStyle(_lib.REDACT_MOSAIC, both), RedactStyle(_lib.REDACT_FILL, both, fill_bgr=(40, 40, 40)), DrawStyle()
    short = (B, HW, HW, p(d), p(c), cap, p(ii), p(sc), cap, None, 0)
    long_ = (B, HW, HW, p(ext[0]), p(ext[1]), cap2, p(ext[3]), p(ext[4]), cap2, None, 0)
    kernels = {}
    for name, tail, trk_tab in (("cap", short, track), ("cap_plus_T", long_, ext[2])):
        kernels[f"fid_redact_faces/mosaic/{name}"] = lambda tail=tail: check(ctx.lib.fid_redact_faces(ctx.handle, p(frames), *tail, C.byref(mosaic)))
        kernels[f"fid_redact_faces/fill/{name}"] = lambda tail=tail: check(ctx.lib.fid_redact_faces(ctx.handle, p(frames), *tail, C.byref(fill)))
        kernels[f"fid_draw_faces/{name}"] = lambda tail=tail, t=trk_tab: check(ctx.lib.fid_draw_faces(ctx.handle, p(frames), *tail, p(t), labels.handle,
                                                                                                      C.byref(dstyle)))
    k_ms = {k: [] for k in kernels}
    for rep in range(REPS + 1):                            # round 0 warms up
        for k, call in kernels.items():
            ctx.event_record(0)
            for _ in range(INNER):
                call()
            ctx.event_record(1)
            t = ctx.elapsed_ms(0, 1) / INNER
            if rep:
                k_ms[k].append(t)
    overlay = {k: round(med(v), 4) for k, v in k_ms.items()}
    overlay["faces"] = int(np.clip(c.download(), 0, cap).sum())
    overlay["faces_and_coasted"] = int(ext[1].download().sum())
    log(str(overlay))
    check(ctx.lib.fid_coaster_destroy(ctx.handle, coaster))
    check(ctx.lib.fid_tracker_destroy(ctx.handle, trk))
    labels.close()

    line = {"tool": "bench_coast", "device": ctx.name(), "date": time.strftime("%Y-%m-%d"), "batch": B, "det": "scrfd_10g", "rec": "arcface_r50",
            "row_cap": row_cap, "repeats": REPS, "steps_per_repeat": STEPS, "faces_last_step": faces, "coasted_rows_per_step": coasted,
            "config": dict(hold=ccfg.hold, predict=ccfg.predict, grow=round(ccfg.grow, 4)),
            "steps_ms": {n: {"median": round(med(ms[n]), 4), "min_max": [round(min(ms[n]), 4), round(max(ms[n]), 4)]} for n in configs},
            "coast_none_over_parent_calls": round(med(ms["coast_none"]) / med(ms["parent_calls"]), 4),
            "coast_on_minus_none_ms": round(med(ms["coast_on"]) - med(ms["coast_none"]), 4),
            "calls": calls, "overlay_ms": overlay}
    text = json.dumps(line)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(text + "\n")
    for pipe in configs.values():
        pipe.close()


if __name__ == "__main__":
    main()
