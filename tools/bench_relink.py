#!/usr/bin/env python3
"""Re-linking (fid_track_relink, TrackedFacePipeline(relink=...)) measurements for docs/FINDINGS.md ("Re-linking").  One process.

The video and the nets are tools/bench_track.py's: one smooth random image, 640 x 640 windows sliding 2 pixels per frame forth and back,
SCRFD-10G + IResNet-50 with seeded weights, B = 64, a gallery of random rows at threshold 0, refresh 16, retry 1, rows="count".
  steps   the tracked step in three forms, alternating inside every repeat: `parent_calls` -- a TrackedFacePipeline whose match() is the body
          it had before the relinker existed (PackedFacePipeline.match, then identify) --, `relink_none` (the default: must cost the same,
          nothing is launched or allocated) and `relink_on` (RelinkConfig(): the one launch of fid_track_relink per step).  8 steps to
          settle, then 5 repeats of 4 consecutive steps between two device events; median ms per step.
  calls   fid_track_step, fid_track_identify, fid_track_keep (its walk and its two copy launches: the call cannot be split from outside) and
          fid_track_relink alone between device events on the video's own detections (cap = 256, T = 64, pool 32, dim 512, random unit
          rows), median of 5: the keep is the yardstick for a one-workgroup walk over the same rows.
One JSON line on stdout, appended to --out.   python tools/bench_relink.py [--out profiles/relink/bench_relink.jsonl]"""
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

REPS, STEPS, SETTLE = 5, 4, 8
HW = 640


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--gallery", type=int, default=1000)
    ap.add_argument("--target", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relink", "bench_relink.jsonl"))
    args = ap.parse_args()
    os.environ.setdefault("FID_AUTOTUNE", "0")
    from bench_track import smooth_image
    from scrfd_arcface_facerecognition_amd import _lib, archs
    from scrfd_arcface_facerecognition_amd._lib import Context, RelinkConfig, check
    from scrfd_arcface_facerecognition_amd.engine import CompiledNet, Gallery
    from scrfd_arcface_facerecognition_amd.pipeline import PackedFacePipeline, TrackedFacePipeline, calibrate_detector_bias

    def log(msg):
        print(f"[bench_relink] {msg}", file=sys.stderr, flush=True)

    class ParentCalls(TrackedFacePipeline):
        """match() as it was before the relinker: the launches of the parent commit's tracked step"""

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
    rcfg = RelinkConfig()
    configs = {"parent_calls": ParentCalls(ctx, det, rec, **kw), "relink_none": TrackedFacePipeline(ctx, det, rec, **kw),
               "relink_on": TrackedFacePipeline(ctx, det, rec, relink=rcfg, **kw)}
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
    on = configs["relink_on"]
    relinked = []
    for _ in range(4):                                     # relinked detections per step, in a pass of its own
        run("relink_on", 1)
        relinked.append(sum(1 for fr in on.results_persons() for f in fr if f[8]))
    faces = int(np.clip(on.post.counts.download()[:B], 0, on.post.cap).sum())

    # ---- the four calls alone, on the video's detections
    cap, T, L, dim = on.post.cap, 64, rcfg.pool, 512
    dets = []
    for k in range(4):
        on.detect(batches[k], HW, HW)
        ctx.sync()
        dets.append((ctx.to_device(on.post.det.download()), ctx.to_device(on.post.counts.download())))
    trk, shots, rl = C.c_void_p(), C.c_void_p(), C.c_void_p()
    check(ctx.lib.fid_tracker_create(ctx.handle, 1, T, C.byref(trk)))
    check(ctx.lib.fid_shots_create(ctx.handle, 1, T, dim, 256, 0, C.byref(shots)))
    check(ctx.lib.fid_relinker_create(ctx.handle, 1, T, L, dim, C.byref(rl)))
    tcfg, ccfg = _lib.TrackConfig(0.3, 15, 16, 1), rcfg.c(15)
    track, offsets, src = ctx.empty((B, cap, 2), np.int32), ctx.empty((B + 1,), np.int32), ctx.empty((row_cap,), np.int32)
    idx, score = ctx.to_device(np.zeros(row_cap, np.int32)), ctx.to_device(np.full(row_cap, 0.5, np.float32))
    ii, sc = ctx.empty((B, cap), np.int32), ctx.empty((B, cap), np.float32)
    rows = np.random.default_rng(5).standard_normal((row_cap, dim))
    q = ctx.to_device((rows / np.sqrt((rows ** 2).sum(1, keepdims=True))).astype(np.float16))
    shot_score = ctx.to_device(np.random.default_rng(6).random(row_cap).astype(np.float32))
    person = ctx.empty((B, cap, 2), np.int32)
    stream = np.zeros(B, np.int32)
    sp = stream.ctypes.data_as(_lib.c_i32_p)
    p = lambda b: C.c_void_p(b.ptr)
    t_step, t_ident, t_keep, t_relink, n_rows = [], [], [], [], []
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
        check(ctx.lib.fid_track_keep(ctx.handle, shots, trk, sp, B, cap, p(track), p(offsets), p(src), row_cap, n, p(shot_score), p(q), None, p(d),
                                     p(ii), p(sc)))
        ctx.event_record(1)
        e = ctx.elapsed_ms(0, 1)
        ctx.event_record(0)
        check(ctx.lib.fid_track_relink(ctx.handle, rl, trk, sp, B, cap, p(c), p(track), p(offsets), p(src), row_cap, n, p(q), C.byref(ccfg), p(person)))
        ctx.event_record(1)
        g = ctx.elapsed_ms(0, 1)
        if rep >= 2:
            t_step.append(a)
            t_ident.append(b)
            t_keep.append(e)
            t_relink.append(g)
            n_rows.append(n)
    med = statistics.median
    calls = dict(frames=B, cap=cap, T=T, pool=L, dim=dim, rows=n_rows, step_ms=round(med(t_step), 4), identify_ms=round(med(t_ident), 4),
                 keep_ms=round(med(t_keep), 4), relink_ms=round(med(t_relink), 4),
                 relink_ms_min_max=[round(min(t_relink), 4), round(max(t_relink), 4)], relink_over_keep=round(med(t_relink) / med(t_keep), 3))
    log(str(calls))
    check(ctx.lib.fid_relinker_destroy(ctx.handle, rl))
    check(ctx.lib.fid_shots_destroy(ctx.handle, shots))
    check(ctx.lib.fid_tracker_destroy(ctx.handle, trk))

    line = {"tool": "bench_relink", "device": ctx.name(), "date": time.strftime("%Y-%m-%d"), "batch": B, "det": "scrfd_10g", "rec": "arcface_r50",
            "row_cap": row_cap, "repeats": REPS, "steps_per_repeat": STEPS, "faces_last_step": faces, "relinked_detections_per_step": relinked,
            "config": dict(thresh=rcfg.thresh, window=rcfg.window, pool=rcfg.pool),
            "steps_ms": {n: {"median": round(med(ms[n]), 4), "min_max": [round(min(ms[n]), 4), round(max(ms[n]), 4)]} for n in configs},
            "relink_none_over_parent_calls": round(med(ms["relink_none"]) / med(ms["parent_calls"]), 4),
            "relink_on_minus_none_ms": round(med(ms["relink_on"]) - med(ms["relink_none"]), 4),
            "calls": calls}
    text = json.dumps(line)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(text + "\n")
    for pipe in configs.values():
        pipe.close()


if __name__ == "__main__":
    main()
